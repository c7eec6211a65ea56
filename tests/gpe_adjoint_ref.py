"""Reference for the adjoint of the GPE's Strang step (csrc/gpe_adjoint.hip): the step written in torch on the CPU, at
complex128 or complex64, differentiated by torch.autograd.  A helper, not a test.

    a = K psi0;  beta = -(V_trap + lights(t0) + k |psi0|^2);  c = a exp(i beta tau);  psi1 = K (c / sqrt(h^2 sum |c|^2))

with K v = ifft2(exp(A_term tau / 2) fft2 v), tau = dt time_scale (numerics/solvers.py:99-122 of the reference).  States
and cotangents are real arrays (..., nx, ny, 2) = (re, im); a spot is the seven numbers (amp0, amp_rate, x0, x_rate, y0,
y_rate, width) in user units."""
import numpy as np
import torch

from pde_opt_amd.fieldmu import schedule


def _dtypes(double):
    return (torch.float64, torch.complex128) if double else (torch.float32, torch.complex64)


class Case:
    """grid, trap, interaction strength and integrator numbers of one problem, as torch constants of one precision"""

    def __init__(self, X, Y, trap, k, A_term, dx, time_scale, double=True):
        self.real, self.cplx = _dtypes(double)
        self.X, self.Y = torch.as_tensor(X, dtype=self.real), torch.as_tensor(Y, dtype=self.real)
        self.trap = torch.as_tensor(trap, dtype=self.real)
        self.k = float(k)
        self.A = torch.as_tensor(np.asarray(A_term, dtype=np.complex128)).to(self.cplx)
        self.h2 = float(dx) ** 2
        self.time_scale = complex(time_scale)

    @classmethod
    def of(cls, equation, solver, double=True):
        return cls(equation.xmesh, equation.ymesh, equation.trap_potential(), equation.k, np.asarray(solver.A_term), solver.dx,
                   solver.time_scale, double)


def lights(p, t, X, Y):
    """sum over the rows of p (S, 7) of (amp0 + amp_rate t) exp(-((x - x0 - x_rate t)^2 + (y - y0 - y_rate t)^2) / (2 w^2))"""
    out = torch.zeros_like(X)
    for q in p:
        dx, dy = X - (q[2] + q[3] * t), Y - (q[4] + q[5] * t)
        out = out + (q[0] + q[1] * t) * torch.exp(-(dx * dx + dy * dy) / (2.0 * q[6] * q[6]))
    return out


def step(case, y, p, t0, dt):
    """one Strang substep of the real state y (..., nx, ny, 2) -> the same shape"""
    psi = torch.view_as_complex(y.contiguous())
    tau = torch.tensor(dt * case.time_scale, dtype=case.cplx)
    E = torch.exp(case.A * (0.5 * tau))
    K = lambda v: torch.fft.ifft2(torch.fft.fft2(v) * E)
    a = K(psi)
    beta = -(case.trap + lights(p, t0, case.X, case.Y) + case.k * (psi.real**2 + psi.imag**2))
    c = a * torch.exp(1j * beta.to(case.cplx) * tau)
    n = torch.sqrt(case.h2 * torch.sum(c.real**2 + c.imag**2, dim=(-2, -1), keepdim=True))
    return torch.view_as_real(K(c / n))


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
        y = step(case, y, p, float(ts[0]) + i * float(dt0), steps[i])
    return torch.stack(out)


def leaves(case, y0, p):
    y = torch.tensor(np.asarray(y0), dtype=case.real, requires_grad=True)
    q = torch.tensor(np.asarray(p, dtype=np.float64), dtype=case.real, requires_grad=True)
    return y, q


def step_vjp(case, y0, p, t0, dt, lam1):
    """(grad (S, 7) in user units summed over the batch, per-environment grads (B, S, 7), lam0) of <lam1, step(y0)>"""
    y, q = leaves(case, y0, p)
    per = []
    out = step(case, y, q, t0, dt)
    w = torch.as_tensor(np.asarray(lam1), dtype=case.real)
    if y.ndim == 4:
        for b in range(y.shape[0]):
            (gb,) = torch.autograd.grad((out[b] * w[b]).sum(), q, retain_graph=True)
            per.append(gb.double().numpy())
    gy, gq = torch.autograd.grad((out * w).sum(), (y, q))
    return gq.double().numpy(), (np.stack(per) if per else None), gy.double().numpy()


def solve_grad(case, y0, p, ts, dt0, objective):
    """(J, ys, dJ/dp (S, 7), dJ/dy0) for objective(ys tensor) -> 0-d tensor"""
    y, q = leaves(case, y0, p)
    ys = solve(case, y, q, ts, dt0)
    J = objective(ys.double())
    gy, gq = torch.autograd.grad(J, (y, q))
    return float(J.detach()), ys.detach().double().numpy(), gq.double().numpy(), gy.double().numpy()
