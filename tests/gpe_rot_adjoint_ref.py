"""Reference for the adjoint of the rotating-frame split step (csrc/gpe_rot_adjoint.hip): the step written in torch on
the CPU, at complex128 or complex64, differentiated by torch.autograd.  A helper, not a test.

    u1 = Lx(s) psi0;  a = Ly(s) u1;  c = a exp(-i (V + k |psi0|^2) tau);  psi1 = Lx(s) Ly(s) (c / sqrt(h^2 sum |c|^2))

with s = tau / 2, tau = dt time_scale, Lx(s) v = ifft_x[exp(s Ax) fft_x v], Ax = 0.5j (2 pi i kx)^2 - omega y (2 pi i kx),
Ly alike with Ay = 0.5j (2 pi i ky)^2 + omega x (2 pi i ky), V = ((1 + e) x^2 + (1 - e) y^2) / 2 (tests/gpe_rot_ref.py is
the same step in numpy).  States and cotangents are real arrays (B, nx, ny, 2) = (re, im); the parameters are a (B, 3)
array of (k, e, omega), one row per environment."""
import numpy as np
import torch

from pde_opt_amd.fieldmu import schedule


def _dtypes(double):
    return (torch.float64, torch.complex128) if double else (torch.float32, torch.complex64)


class Case:
    """grid and integrator numbers of one problem, as torch constants of one precision"""

    def __init__(self, domain, time_scale=1.0, double=True):
        self.real, self.cplx = _dtypes(double)
        x, y = domain.mesh()
        kx, ky = domain.fft_mesh()
        self.X, self.Y = torch.as_tensor(x, dtype=self.real), torch.as_tensor(y, dtype=self.real)
        self.ikx = torch.as_tensor(2j * np.pi * kx).to(self.cplx)
        self.iky = torch.as_tensor(2j * np.pi * ky).to(self.cplx)
        self.h2 = float(domain.dx[0]) ** 2
        self.time_scale = complex(time_scale)


def step(case, y, p, dt):
    """one substep of the real state y (B, nx, ny, 2) with the parameters p (B, 3) -> the same shape"""
    psi = torch.view_as_complex(y.contiguous())
    k, e, om = (p[:, j].reshape(-1, 1, 1) for j in range(3))
    tau = torch.tensor(dt * case.time_scale, dtype=case.cplx)
    s = 0.5 * tau
    ex = torch.exp(s * (0.5j * case.ikx**2 - (om * case.Y).to(case.cplx) * case.ikx))
    ey = torch.exp(s * (0.5j * case.iky**2 + (om * case.X).to(case.cplx) * case.iky))
    lx = lambda v: torch.fft.ifft(torch.fft.fft(v, dim=-2) * ex, dim=-2)
    ly = lambda v: torch.fft.ifft(torch.fft.fft(v, dim=-1) * ey, dim=-1)
    w = 0.5 * ((1 + e) * case.X**2 + (1 - e) * case.Y**2) + k * (psi.real**2 + psi.imag**2)
    c = ly(lx(psi)) * torch.exp(-1j * w.to(case.cplx) * tau)
    n = torch.sqrt(case.h2 * torch.sum(c.real**2 + c.imag**2, dim=(-2, -1), keepdim=True))
    return torch.view_as_real(lx(ly(c / n)))


def solve(case, y0, p, ts, dt0):
    """the saved states (len(ts), *y0.shape): constant steps, a clipped last step, linear interpolation inside a step
    (the schedule of integrate.diffeqsolve)"""
    steps, saves = schedule(ts, dt0)
    by_index = {}
    for q, (i, theta) in enumerate(saves):
        by_index.setdefault(i, []).append((q, theta))
    out = [None] * len(saves)
    y, prev = y0, None
    for i in range(len(steps) + 1):
        for q, theta in by_index.get(i, ()):
            out[q] = y if theta is None else prev + theta * (y - prev)
        if i == len(steps):
            break
        prev = y
        y = step(case, y, p, steps[i])
    return torch.stack(out)


def leaves(case, y0, p):
    y = torch.tensor(np.asarray(y0), dtype=case.real, requires_grad=True)
    q = torch.tensor(np.asarray(p, dtype=np.float64), dtype=case.real, requires_grad=True)
    return y, q


def step_vjp(case, y0, p, dt, lam1):
    """(per-environment gradient (B, 3) over (k, e, omega), lam0) of <lam1, step(y0)>"""
    y, q = leaves(case, y0, p)
    out = step(case, y, q, dt)
    gy, gq = torch.autograd.grad((out * torch.as_tensor(np.asarray(lam1), dtype=case.real)).sum(), (y, q))
    return gq.double().numpy(), gy.double().numpy()


def solve_grad(case, y0, p, ts, dt0, objective):
    """(J, ys, dJ/dp (B, 3), dJ/dy0) for objective(ys tensor) -> 0-d tensor"""
    y, q = leaves(case, y0, p)
    ys = solve(case, y, q, ts, dt0)
    J = objective(ys.double())
    gy, gq = torch.autograd.grad(J, (y, q))
    return float(J.detach()), ys.detach().double().numpy(), gq.double().numpy(), gy.double().numpy()
