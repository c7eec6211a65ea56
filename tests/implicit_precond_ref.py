"""numpy reference of the spectral preconditioner of the implicit Euler step (csrc/implicit.hip,
pdeopt_implicit_set_precond): the symbol of the finite-difference operator, the coefficient means, M^-1 by rfft2 / irfft2,
and right-preconditioned restarted GMRES with the Givens / modified Gram-Schmidt structure of ``implicit_ref.gmres``.
Also the problems the preconditioner tests share (tests/test_implicit_precond_cpu.py, tests/test_gpu_implicit_precond.py).
Test infrastructure only."""
import numpy as np

import implicit_problems as Q
import implicit_ref as R
import sens_ref as S

GRIDS = {"24x40": (24, 40), "45x33": (45, 33), "64x64": (64, 64), "96x80": (96, 80)}


def shell(points, hx, hy):
    """s(kx, ky) = (4 / hx^2) sin^2(pi kx / nx) + (4 / hy^2) sin^2(pi ky / ny) on the half spectrum (nx, ny // 2 + 1):
    minus the symbol of the 5-point Laplacian"""
    nx, ny = points
    sx = np.sin(np.pi * np.arange(nx) / nx) ** 2
    sy = np.sin(np.pi * np.arange(ny // 2 + 1) / ny) ** 2
    return (4.0 / hx**2) * sx[:, None] + (4.0 / hy**2) * sy[None, :]


def coefs(u, mu, mob, clamp=True):
    """(a, c) = (max(mean(D(u) mu_h'(u)), 0), mean D(u)) in fp64 from the values of u (any dtype)"""
    u64 = np.asarray(u, np.float64)
    D = np.asarray(mob(u64), np.float64) * np.ones_like(u64)
    a = float(np.mean(D * S.closure_dc(mu, u64)))
    return (max(a, 0.0) if clamp else a), float(np.mean(D))


def symbol(eq, points, dt, hx, hy, kappa, a, c):
    """M on the half spectrum: Cahn-Hilliard 1 + dt s (a + c kappa s), Allen-Cahn 1 + dt (a + c kappa s)"""
    s = shell(points, hx, hy)
    lin = a + c * kappa * s
    return 1.0 + dt * (s * lin if eq == "ch" else lin)


def minv(eq, u, v, dt, hx, hy, kappa, mu, mob):
    """M^-1 v at the state u, in v's dtype: fp64 means and symbol; the transforms and the multiply in v's precision"""
    a, c = coefs(u, mu, mob)
    M = symbol(eq, v.shape, dt, hx, hy, kappa, a, c)
    if v.dtype == np.float32:
        h = np.fft.rfft2(v).astype(np.complex64) * (1.0 / M).astype(np.float32)
        return np.fft.irfft2(h, s=v.shape).astype(np.float32)
    return np.fft.irfft2(np.fft.rfft2(v) / M, s=v.shape)


def gmres_right(op, pre, b, rtol, restart=20, max_iter=400):
    """restarted GMRES on op(pre(z)) = b from x = 0, x = pre(z): ``implicit_ref.gmres`` with z_j = pre(v_j), w = op(z_j)
    in the loop and one ``pre`` per cycle end; the estimate is the residual of op(x) = b.  Returns (x, iterations)"""
    x = np.zeros_like(b)
    bn = float(np.linalg.norm(b.astype(np.float64)))
    if bn == 0.0:
        return x, 0
    its = 0
    r = b.copy()
    while its < max_iter:
        beta = float(np.linalg.norm(r.astype(np.float64)))
        if beta <= rtol * bn:
            break
        V = [(r / b.dtype.type(beta))]
        H = np.zeros((restart + 1, restart))
        g = np.zeros(restart + 1)
        g[0] = beta
        cs, sn = np.zeros(restart), np.zeros(restart)
        k = 0
        for j in range(restart):
            w = op(pre(V[j]))
            for i in range(j + 1):
                H[i, j] = float(np.vdot(V[i].astype(np.float64), w.astype(np.float64)))
                w = w - b.dtype.type(H[i, j]) * V[i]
            hn = H[j + 1, j] = float(np.linalg.norm(w.astype(np.float64)))
            for i in range(j):
                a, c = H[i, j], H[i + 1, j]
                H[i, j], H[i + 1, j] = cs[i] * a + sn[i] * c, -sn[i] * a + cs[i] * c
            den = np.hypot(H[j, j], H[j + 1, j])
            cs[j], sn[j] = (H[j, j] / den, H[j + 1, j] / den) if den > 0 else (1.0, 0.0)
            H[j, j], H[j + 1, j] = den, 0.0
            g[j + 1], g[j] = -sn[j] * g[j], cs[j] * g[j]
            its += 1
            k = j + 1
            if abs(g[j + 1]) <= rtol * bn or its >= max_iter:
                break
            V.append(w / b.dtype.type(hn if hn > 0 else 1.0))
        yk = np.linalg.solve(H[:k, :k], g[:k]) if k else np.zeros(0)
        comb = np.zeros_like(b)
        for i in range(k):
            comb = comb + b.dtype.type(yk[i]) * V[i]
        x = x + pre(comb)
        if abs(g[k]) <= rtol * bn:
            break
        r = b - op(x)
    return x, its


def newton_counts(eq, y0, dt, hx, hy, kappa, mu, mob, rtol, atol, precond, krylov_rtol=1e-3, restart=20, max_newton=50):
    """the Newton solve of ``implicit_ref.newton`` by GMRES, with or without the preconditioner: (y1, Newton iterations,
    Krylov iterations of each linear solve)"""
    t = y0.dtype.type
    y = y0.copy()
    its = []
    for it in range(max_newton + 1):
        G = (y - y0) - t(dt) * R.rhs(eq, y, hx, hy, kappa, mu, mob)
        if R.rms(G) <= atol + rtol * R.rms(y):
            return y, it, its
        if it == max_newton:
            break
        op = lambda v: R.apply_op(eq, y, v, dt, hx, hy, kappa, mu, mob)
        if precond:
            pre = lambda v: minv(eq, y, v, dt, hx, hy, kappa, mu, mob)
            d, k = gmres_right(op, pre, -G, krylov_rtol, restart)
        else:
            d, k = R.gmres(op, -G, krylov_rtol, restart)
        its.append(k)
        y = y + d
    raise RuntimeError(f"reference Newton did not converge: rms(G) = {R.rms(G):.3e} after {max_newton} iterations")


# ---- the states of the iteration-count tests: the issue's ------------------------------------------------------------
def noise_state(points, seed, dtype=np.float64):
    """0.5 +- 0.01 uniform noise"""
    return (0.5 + 0.01 * np.random.default_rng(seed).uniform(-1.0, 1.0, points)).astype(dtype)


def stripe_state(points, dtype=np.float64):
    """two smooth stripes along axis 0, c from 0.1 to 0.9, under +- 0.01 noise (a field that varies along one axis only
    spans a Krylov space of a few dimensions, whatever the operator)"""
    nx, ny = points
    x = (np.arange(nx)[:, None] + 0.5) / nx
    noise = 0.01 * np.random.default_rng(8).uniform(-1.0, 1.0, points)
    return (0.5 + 0.39 * np.tanh(4.0 * np.sin(4.0 * np.pi * x)) + noise).astype(dtype)


STATES = {"noise": lambda points, dtype=np.float64: noise_state(points, 7, dtype), "stripe": stripe_state}


def count_problem(eq, grid, state, closures):
    """(points, mu, mobility, y0 in fp64, dt = 50 x the Euler limit at y0) of an iteration-count case"""
    points = GRIDS[grid]
    mu, mob = Q.CLOSURES[closures]
    y = STATES[state](points)
    return points, mu, mob, y, Q.step_size(eq, points, closures, y)
