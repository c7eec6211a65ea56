"""CPU reference of the field-mu path: a torch fp64 port of the finite-difference Cahn-Hilliard right-hand side (rolls)
and of the IMEX / Euler step (torch.fft), following oracle/np_oracle.py op for op, with mu_h supplied by a module.
torch.autograd through it is the reference gradient of the GPU's discrete adjoint (csrc/fieldmu.hip).

`python tests/fieldmu_ref.py` runs the end-to-end training problem of tests/test_gpu_fieldmu.py on the CPU (the same BFGS,
the gradient from autograd) and the reference-vs-reference distances that test records."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def nb(a, d, axis):
    return torch.roll(a, -d, axis)


def lap5(u, hx, hy):
    ddx = (nb(u, 1, -2) - 2 * u + nb(u, -1, -2)) / hx**2
    ddy = (nb(u, 1, -1) - 2 * u + nb(u, -1, -1)) / hy**2
    return ddx + ddy


def grad_face(a, h, axis):
    return (nb(a, 1, axis) - a) / h


def avg_face(a, axis):
    return 0.5 * (a + nb(a, 1, axis))


def div_face(F, h, axis):
    return (F - nb(F, -1, axis)) / h


def ch_rhs(u, muh, hx, hy, kappa, D):
    """np_oracle.ch_rhs_fd with mu_h(u) given as the field ``muh``; ``u`` is (..., nx, ny)"""
    mu = muh - kappa * lap5(u, hx, hy)
    gx = grad_face(mu, hx, -2)
    gy = grad_face(mu, hy, -1)
    Du = D(u)
    Fx = avg_face(Du, -2) * gx
    Fy = avg_face(Du, -1) * gy
    return div_face(Fx, hx, -2) + div_face(Fy, hy, -1)


def legendre_series(coeffs, x):
    res = coeffs[0] * torch.ones_like(x)
    if len(coeffs) > 1:
        res = res + coeffs[1] * x
    p_prev, p_cur = torch.ones_like(x), x
    for n in range(2, len(coeffs)):
        p_next = ((2 * n - 1) * x * p_cur - (n - 1) * p_prev) / n
        res = res + coeffs[n] * p_next
        p_prev, p_cur = p_cur, p_next
    return res


def diffusion_legendre(coeffs):
    """exp(Legendre(2c - 1)), np_oracle.diffusion_legendre"""
    return lambda c: torch.exp(legendre_series(list(coeffs), 2.0 * c - 1.0))


class PointwiseLegendreMu(torch.nn.Module):
    """Legendre(2c - 1) + log(c / (1 - c)) as a module with trainable coefficients: ChemicalPotentialLegendrePolynomials
    under the logit prior, for comparing the module path with the in-kernel closure"""

    def __init__(self, coeffs, dtype=torch.float64):
        super().__init__()
        self.coeffs = torch.nn.Parameter(torch.tensor(list(coeffs), dtype=dtype))

    def forward(self, x):
        return legendre_series(self.coeffs, 2.0 * x - 1.0) + torch.log(x / (1.0 - x))


def mu_of(module):
    """the module applied to a batch (B, nx, ny)"""
    return lambda u: module(u[:, None])[:, 0]


def step(u, module, dt, hx, hy, kappa, D, integrator, A=0.5, symbol=None):
    """np_oracle.euler_step / imex_step of a batch (B, nx, ny)"""
    f = ch_rhs(u, mu_of(module)(u), hx, hy, kappa, D)
    if integrator == "euler":
        return u + dt * f
    denom = 1.0 + A * dt * torch.as_tensor(symbol)
    return u + dt * torch.fft.ifftn(torch.fft.fftn(f, dim=(-2, -1)) / denom, dim=(-2, -1)).real


def solve_saveat(stepper, y0, ts, dt):
    """np_oracle.solve_saveat (constant steps, linear dense output) on tensors; ``stepper(y, dt) -> y``"""
    from oracle import np_oracle as O

    ts = [float(t) for t in ts]
    t0, t1 = ts[0], ts[-1]
    n_full, rem = O.constant_step_plan(t0, t1, dt)
    edges = [t0 + i * dt for i in range(n_full + 1)]
    if rem > 0.0:
        edges.append(t1)
    edges[-1] = t1
    out = []
    y_prev, y = y0, y0
    idx = 0
    for tq in ts:
        while idx < len(edges) - 1 and edges[idx] < tq - 1e-12 * max(1.0, abs(tq)):
            y_prev = y
            y = stepper(y, dt if idx < n_full else rem)
            idx += 1
        if idx == 0 or edges[idx] <= tq + 1e-12 * max(1.0, abs(tq)):
            out.append(y)
        else:
            a, b = edges[idx - 1], edges[idx]
            out.append(y_prev + ((tq - a) / (b - a)) * (y - y_prev))
    return torch.stack(out)


def mse(module, y0s, values, ts, dt, hx, hy, kappa, D, integrator, A=0.5, symbol=None):
    """mean(r^2), r = values - solve[1:], for y0s (B, nx, ny) and values (B, T - 1, nx, ny), as a tensor"""
    ys = solve_saveat(lambda y, h: step(y, module, h, hx, hy, kappa, D, integrator, A, symbol), torch.as_tensor(y0s), ts, dt)
    r = torch.as_tensor(values) - ys[1:].swapaxes(0, 1)
    return torch.mean(r**2)


def mse_and_grad(module, *args, **kw):
    """(mse, flat gradient over module.parameters()) by autograd"""
    for p in module.parameters():
        p.grad = None
    J = mse(module, *args, **kw)
    J.backward()
    return float(J.detach()), np.concatenate([p.grad.double().reshape(-1).numpy() for p in module.parameters()])


def vjp_rhs(u, muh, lam, hx, hy, kappa, D):
    """(g_u at fixed mu_h, g_mu) of <lam, ch_rhs(u, muh)>"""
    u = u.clone().requires_grad_(True)
    muh = muh.clone().requires_grad_(True)
    J = (lam * ch_rhs(u, muh, hx, hy, kappa, D)).sum()
    return torch.autograd.grad(J, [u, muh])


# ---- the shared problems of tests/test_gpu_fieldmu.py -------------------------------------------------------------------

KAPPA = 0.002
D_COEF = (-0.3, 0.2)
MU_TRUE = (0.0, -3.0, 0.4)
GRIDS = {"8x8": (8, 8), "16x32": (16, 32), "33x47": (33, 47), "64x64": (64, 64)}
BOX = ((0.0, 1.0), (0.0, 1.3))  # hx != hy on every grid


def spacing(shape):
    return (BOX[0][1] - BOX[0][0]) / shape[0], (BOX[1][1] - BOX[1][0]) / shape[1]


def rough_state(shape, B, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return np.clip(0.5 + 0.1 * rng.standard_normal((B,) + tuple(shape)), 0.1, 0.9).astype(dtype)


def smooth_state(shape, B, seed):
    rng = np.random.default_rng(seed)
    x, y = np.arange(shape[0]) / shape[0], np.arange(shape[1]) / shape[1]
    u = 0.5 + np.zeros((B,) + tuple(shape))
    for b in range(B):
        for _ in range(6):
            kx, ky = rng.integers(1, 3, 2)
            u[b] += 0.04 * rng.standard_normal() * np.cos(2 * np.pi * (kx * x[:, None] + ky * y[None, :]) + rng.uniform(0, 6))
    return u


def symbol_of(shape, spacing_xy=None):
    from oracle import np_oracle as O

    hx, hy = spacing_xy or spacing(shape)
    return O.ch_fourier_symbol(shape[0], shape[1], hx, hy, KAPPA).real


def seeded_cnn(hidden, seed, scale=0.3, dtype=torch.float64):
    """PeriodicCNN(1, hidden, 1) with parameters from a seeded numpy generator (the same on every machine)"""
    from pde_opt_amd import fieldmu
    from pde_opt_amd.numerics.functions.cnn import PeriodicCNN

    m = PeriodicCNN(1, hidden, 1).to(dtype)
    n = sum(p.numel() for p in m.parameters())
    fieldmu.unflatten_params(m, scale * np.random.default_rng(seed).standard_normal(n))
    return m


GRAD_SHAPE = (16, 32)
GRAD_TS = np.array([0.0, 1.75e-5, 4e-5])  # dt0 = 1e-6: 40 substeps, the middle save half-way into substep 18


def frames_of_truth(y0s, spacing_xy):
    """values (B, 2, nx, ny): the frames of the Legendre truth at GRAD_TS[1:] (IMEX)"""
    hx, hy = spacing_xy
    sym = symbol_of(y0s.shape[1:], spacing_xy)
    truth = PointwiseLegendreMu(MU_TRUE)
    with torch.no_grad():
        ys = solve_saveat(lambda y, h: step(y, truth, h, hx, hy, KAPPA, diffusion_legendre(D_COEF), "imex", 0.5, sym),
                          torch.as_tensor(y0s), GRAD_TS, 1e-6)
    return ys[1:].swapaxes(0, 1).numpy().copy()


def grad_problem():
    """(y0s (2, nx, ny), values (2, 2, nx, ny)) of the two-trajectory mse on BOX"""
    y0s = smooth_state(GRAD_SHAPE, 2, 21)
    return y0s, frames_of_truth(y0s, spacing(GRAD_SHAPE))


# end to end: the notebooks' spacing (0.01, here 0.013 along y), where the dynamics are fast enough for 40 substeps to
# tell chemical potentials apart
E2E_HIDDEN, E2E_SEED, E2E_STEPS = (8, 8), 5, 30
E2E_BOX = ((0.0, 0.01 * GRAD_SHAPE[0]), (0.0, 0.013 * GRAD_SHAPE[1]))
E2E_SPACING = (0.01, 0.013)


def e2e_problem():
    y0s = smooth_state(GRAD_SHAPE, 2, 21)
    return y0s, frames_of_truth(y0s, E2E_SPACING)


# what train_reference() gives (tests/test_fieldmu_cpu.py re-derives it): the mse before and after the 30 BFGS steps, a
# decrease of x 28.9.  tests/test_gpu_fieldmu.py gates the GPU run at 10 x the final value.
CPU_TRAIN = (8.845e-06, 3.060e-07)


def train_reference(max_steps=E2E_STEPS):
    """the end-to-end problem through the reference gradient and the package's BFGS: history of the mse"""
    from pde_opt_amd import fieldmu, fit

    hx, hy = E2E_SPACING
    y0s, values = e2e_problem()
    m = seeded_cnn(E2E_HIDDEN, E2E_SEED)
    args = (y0s, values, GRAD_TS, 1e-6, hx, hy, KAPPA, diffusion_legendre(D_COEF), "imex", 0.5, symbol_of(GRAD_SHAPE, E2E_SPACING))

    def vg(p):
        fieldmu.unflatten_params(m, p)
        return mse_and_grad(m, *args)

    def v(p):
        fieldmu.unflatten_params(m, p)
        with torch.no_grad():
            return float(mse(m, *args))

    _, hist = fit.minimize_bfgs(vg, v, fieldmu.flatten_params(m), max_steps=max_steps)
    return hist


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def solve_distance(shape, n_steps=200, dt=1e-6):
    """relative L2 distance after n IMEX substeps between this reference with the torch-evaluated mu_h and np_oracle"""
    from oracle import np_oracle as O

    hx, hy = spacing(shape)
    u0 = smooth_state(shape, 1, 3)
    sym = symbol_of(shape)
    mod = PointwiseLegendreMu(MU_TRUE)
    y = torch.as_tensor(u0)
    with torch.no_grad():
        for _ in range(n_steps):
            y = step(y, mod, dt, hx, hy, KAPPA, diffusion_legendre(D_COEF), "imex", 0.5, sym)
    mu_h = lambda c: O.chem_potential_legendre(MU_TRUE, c, lambda c: np.log(c / (1 - c)))
    Dn = lambda c: O.diffusion_legendre(D_COEF, c)
    z = u0[0]
    for _ in range(n_steps):
        z = O.imex_step(lambda t, w: O.ch_rhs_fd(w, hx, hy, KAPPA, mu_h, Dn), 0.0, z, dt, 0.5, sym)
    return _rel(y[0].numpy(), z)


def fp32_vjp_distance(shape, B):
    """max over (g_u, g_mu) of the reference VJP's own fp32-vs-fp64 distance, per entry relative to the field maximum,
    on the fp32 inputs the GPU test uses"""
    hx, hy = spacing(shape)
    u, muh, lam = vjp_inputs(shape, B, np.float32)
    D = diffusion_legendre(D_COEF)
    lo = vjp_rhs(torch.as_tensor(u), torch.as_tensor(muh), torch.as_tensor(lam), hx, hy, KAPPA, D)
    hi = vjp_rhs(torch.as_tensor(u).double(), torch.as_tensor(muh).double(), torch.as_tensor(lam).double(), hx, hy, KAPPA, D)
    return max(float((a.double() - b).abs().max() / b.abs().max()) for a, b in zip(lo, hi))


def vjp_inputs(shape, B, dtype):
    """(u, mu_h = the truth's mu_h(u), lambda) of the adjoint-kernel test"""
    from oracle import np_oracle as O

    u = rough_state(shape, B, 31, dtype)
    muh = O.chem_potential_legendre(MU_TRUE, u.astype(np.float64), lambda c: np.log(c / (1 - c))).astype(dtype)
    lam = np.random.default_rng(32).standard_normal(u.shape).astype(dtype)
    return u, muh, lam


if __name__ == "__main__":
    for name, shape in GRIDS.items():
        print(f"fp32 VJP reference distance {name}: B=1 {fp32_vjp_distance(shape, 1):.3e}  B=3 {fp32_vjp_distance(shape, 3):.3e}")
    for name in ("16x32", "33x47"):
        print(f"200 IMEX substeps, torch mu_h vs np_oracle, {name}: {solve_distance(GRIDS[name]):.3e}")
    hist = train_reference()
    print(f"end to end on the CPU: mse {hist[0]:.6e} -> {hist[-1]:.6e} in {len(hist) - 1} BFGS steps (x{hist[0] / hist[-1]:.1f})")
