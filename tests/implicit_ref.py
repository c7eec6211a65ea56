"""numpy reference of the implicit Euler step (csrc/implicit.hip), built on the oracle's primitives (oracle/np_oracle.py):
the exact linearisation J_f(u) v of ``ch_rhs_fd`` / ``ac_rhs_fd``, and a Newton solve of y - y0 - dt f(y) = 0 by two
routes -- a dense Jacobian with ``numpy.linalg.solve`` (small grids) and its own GMRES -- in fp64, or with every array
in float32.  Test infrastructure only."""
import numpy as np

from oracle import np_oracle as O
import sens_ref as S


def rhs(eq, u, hx, hy, kappa, mu, mob):
    """f(u) of equation ``eq`` ("ch" or "ac"), in u's dtype"""
    dt = u.dtype.type
    f = O.ch_rhs_fd if eq == "ch" else O.ac_rhs_fd
    return f(u, dt(hx), dt(hy), dt(kappa), lambda c: _cl(mu, c), lambda c: _cl(mob, c)).astype(u.dtype)


def _cl(desc, c):
    """a closure evaluated in c's dtype (the descriptors compute in fp64)"""
    return np.asarray(desc(c.astype(np.float64))).astype(c.dtype) if c.dtype == np.float32 else desc(c)


def _dc(desc, c):
    return np.asarray(S.closure_dc(desc, c.astype(np.float64))).astype(c.dtype)


def jac(eq, u, v, hx, hy, kappa, mu, mob):
    """J_f(u) v: Cahn-Hilliard  div( avg(D'(u) v) grad(mu) + avg(D(u)) grad(mu_h'(u) v - kappa lap v) ),
    Allen-Cahn  -R'(u) v m - R(u) (mu_h'(u) v - kappa lap v), with mu = m = mu_h(u) - kappa lap u"""
    t = u.dtype.type
    hx, hy, kappa = t(hx), t(hy), t(kappa)
    m = _cl(mu, u) - kappa * O.lap5(u, hx, hy)
    D = _cl(mob, u)
    dmu = _dc(mu, u) * v - kappa * O.lap5(v, hx, hy)
    dD = _dc(mob, u) * v
    if eq == "ac":
        return (-(dD * m) - D * dmu).astype(u.dtype)
    out = 0.0
    for ax, h in ((0, hx), (1, hy)):
        F = O.avg_face(dD, ax) * O.grad_face(m, h, ax) + O.avg_face(D, ax) * O.grad_face(dmu, h, ax)
        out = out + O.div_face(F, h, ax)
    return out.astype(u.dtype)


def apply_op(eq, u, v, dt, hx, hy, kappa, mu, mob):
    """(I - dt J_f(u)) v"""
    return v - u.dtype.type(dt) * jac(eq, u, v, hx, hy, kappa, mu, mob)


def rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, dtype=np.float64) ** 2)))


def gmres(op, b, rtol, restart=20, max_iter=400):
    """restarted GMRES (modified Gram-Schmidt, Givens) for op(x) = b from x = 0, to an estimate <= rtol |b|; returns
    (x, iterations)"""
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
            w = op(V[j])
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
        for i in range(k):
            x = x + b.dtype.type(yk[i]) * V[i]
        if abs(g[k]) <= rtol * bn:
            break
        r = b - op(x)
    return x, its


def dense_jacobian(eq, u, hx, hy, kappa, mu, mob):
    """J_f(u) as an (n, n) matrix, column by column from ``jac`` (small grids)"""
    n = u.size
    J = np.empty((n, n), dtype=u.dtype)
    e = np.zeros(n, dtype=u.dtype)
    for q in range(n):
        e[q] = 1
        J[:, q] = jac(eq, u, e.reshape(u.shape), hx, hy, kappa, mu, mob).ravel()
        e[q] = 0
    return J


def newton(eq, y0, dt, hx, hy, kappa, mu, mob, rtol, atol, route="gmres", krylov_rtol=1e-3, restart=20, max_newton=50):
    """y1 with y1 - y0 - dt f(y1) = 0 to rms(G) <= atol + rtol rms(y), first iterate y0, in y0's dtype.  ``route``:
    "dense" (numpy.linalg.solve on the assembled Jacobian) or "gmres".  Returns (y1, Newton iterations, rms(G))"""
    t = y0.dtype.type
    y = y0.copy()
    for it in range(max_newton + 1):
        G = (y - y0) - t(dt) * rhs(eq, y, hx, hy, kappa, mu, mob)
        if rms(G) <= atol + rtol * rms(y):
            return y, it, rms(G)
        if it == max_newton:
            break
        if route == "dense":
            A = np.eye(y.size, dtype=y.dtype) - t(dt) * dense_jacobian(eq, y, hx, hy, kappa, mu, mob)
            d = np.linalg.solve(A, -G.ravel()).reshape(y.shape).astype(y.dtype)
        else:
            d, _ = gmres(lambda v: apply_op(eq, y, v, dt, hx, hy, kappa, mu, mob), -G, krylov_rtol, restart)
        y = y + d
    raise RuntimeError(f"reference Newton did not converge: rms(G) = {rms(G):.3e} after {max_newton} iterations")


def euler_limit(eq, u, hx, hy, kappa, mu, mob):
    """the explicit Euler stability limit 2 / rho of the problem linearised at u, from the bound on the spectral radius
    rho of J_f that keeps only its stiffest part, the fourth-order (CH) or second-order (AC) term with the largest
    mobility: the 5-point Laplacian's largest eigenvalue is L = 4 / hx^2 + 4 / hy^2, so
      Cahn-Hilliard  rho <= max D (kappa L^2 + max|mu_h'| L),    Allen-Cahn  rho <= max R (kappa L + max|mu_h'|)"""
    L = 4.0 / hx**2 + 4.0 / hy**2
    u64 = u.astype(np.float64)
    dmax = float(np.max(np.abs(mob(u64))))
    m1 = float(np.max(np.abs(S.closure_dc(mu, u64))))
    rho = dmax * (kappa * L * L + m1 * L) if eq == "ch" else dmax * (kappa * L + m1)
    return 2.0 / rho
