"""numpy reference of the Butler-Volmer Allen-Cahn equations: the bodies of ``rhs_fd`` / ``get_voltage`` of the three
upstream classes (pde_opt/numerics/equations/allen_cahn.py:162-395) with ``np.roll`` stencils, in the dtype of the state
(float64 is the yardstick; float32 gives the rounding of the same expressions in single precision), the textbook
Euler / RK4 / Tsit5 steps of oracle/np_oracle.py around them, and the adaptive loop of ``integrate._solve_adaptive``
(trial step, scaled RMS error norm, ``_pid_update``, ``_clip_dt``) with its accept / reject record."""
import numpy as np

from oracle import np_oracle as O

MU = lambda c: np.log(c / (1.0 - c)) + 3.0 * (1.0 - 2.0 * c)  # noqa: E731  (notebooks/run_butler_volmer_sbm.ipynb)
J0 = lambda c: np.sqrt((1.0 - c) * c)  # noqa: E731


def lap(u, hx, hy):
    """_lap_2nd_2D (derivatives.py:8-12)"""
    return ((np.roll(u, -1, 0) - 2 * u + np.roll(u, 1, 0)) / hx**2 + (np.roll(u, -1, 1) - 2 * u + np.roll(u, 1, 1)) / hy**2)


def sbm_lap(u, psi, hx, hy):
    """divx(avgx(psi) gradx u) + divy(avgy(psi) grady u) (derivatives.py:24-61; allen_cahn.py:326-333)"""
    out = 0
    for ax, h in ((0, hx), (1, hy)):
        flux = 0.5 * (psi + np.roll(psi, -1, ax)) * ((np.roll(u, -1, ax) - u) / h)  # on the face between i and i + 1
        out = out + (flux - np.roll(flux, 1, ax)) / h
    return out


def mu_of(u, hx, hy, kappa, mu=MU, psi=None):
    if psi is None:
        return mu(u) - kappa * lap(u, hx, hy)
    return mu(u) - (kappa / psi) * sbm_lap(u, psi, hx, hy)


def sums(u, hx, hy, kappa, mu=MU, j0=J0, psi=None):
    """(I+, I-, mu)"""
    m = mu_of(u, hx, hy, kappa, mu, psi)
    w = 1.0 if psi is None else psi
    return np.sum(j0(u) * np.exp(0.5 * m) * w) * hx * hy, np.sum(j0(u) * np.exp(-0.5 * m) * w) * hx * hy, m


def voltage(u, hx, hy, kappa, C, mu=MU, j0=J0, psi=None):
    """get_voltage (allen_cahn.py:272-281, 356-383)"""
    ip, im, _ = sums(u, hx, hy, kappa, mu, j0, psi)
    y = (-C + np.sqrt(C**2 + 4.0 * ip * im)) / (2.0 * ip)
    return 2.0 * np.log(y)


def rate(u, m, v, alpha, j0=J0):
    eta = m + v
    return j0(u) * (np.exp(-alpha * eta) - np.exp((1.0 - alpha) * eta))


def rhs_voltage(u, hx, hy, kappa, alpha, v, mu=MU, j0=J0):
    """AllenCahn2DPeriodicButlerVolmer.rhs_fd(state, t, v) (allen_cahn.py:204-210)"""
    return rate(u, mu_of(u, hx, hy, kappa, mu), v, alpha, j0)


def rhs_current(u, hx, hy, kappa, alpha, C, mu=MU, j0=J0, psi=None):
    """the two constant-current rhs_fd bodies (allen_cahn.py:257-270, 323-354); ``psi`` selects the smoothed-boundary one"""
    ip, im, m = sums(u, hx, hy, kappa, mu, j0, psi)
    y = (-C + np.sqrt(C**2 + 4.0 * ip * im)) / (2.0 * ip)
    return rate(u, m, 2.0 * np.log(y), alpha, j0)


def current_scale(u, hx, hy, kappa, C, mu=MU, j0=J0, psi=None):
    """I+ y + I- / y: the size of the two terms whose difference is the total current (alpha = 1/2)"""
    ip, im, _ = sums(u, hx, hy, kappa, mu, j0, psi)
    y = (-C + np.sqrt(C**2 + 4.0 * ip * im)) / (2.0 * ip)
    return ip * y + im / y


def total_rate(k, hx, hy, psi=None):
    return np.sum(k * (1.0 if psi is None else psi)) * hx * hy


def notebook_state(rng, shape, dtype=np.float64):
    """clip(0.1 + 0.1 normal, 0.05, 1), as the notebook draws it"""
    return np.clip(0.1 + 0.1 * rng.standard_normal(shape), 0.05, 1.0).astype(dtype)


def disc_psi(nx, ny, floor=1e-6):
    """tanh disc with a floor, built like the smoothed-boundary tests' ``util.sbm_psi``"""
    x, y = np.arange(nx) + 0.5, np.arange(ny) + 0.5
    X, Y = np.meshgrid(x, y, indexing="ij")
    r = np.sqrt((X - 0.5 * nx) ** 2 + (Y - 0.5 * ny) ** 2)
    return floor + (1.0 - floor) * 0.5 * (1.0 + np.tanh((0.3 * min(nx, ny) - r) / 2.5))


def relaxed_state(seed, nx, ny, h=0.01, kappa=0.002, C=0.02, t_relax=0.01):
    """The notebook's state after the notebook's own adaptive solve (this module's loop, PIDController(1e-4, 1e-6), dt0 = 1e-6)
    has carried it to ``t_relax`` on the tanh disc.  The raw state is white noise clipped at 0.05 on h = 0.01: rates of
    1e5, which the notebook only ever meets with steps of 1e-6 -- a FIXED step of 1e-4 leaves (0, 1) in one step and the
    reference itself returns NaN.  Fixed-step comparisons start here instead (rates of order one)."""
    from pde_opt_amd.numerics.solvers import PIDController

    psi = disc_psi(nx, ny)
    f = lambda t, y: rhs_current(y, h, h, kappa, 0.5, C, psi=psi)  # noqa: E731
    u0 = notebook_state(np.random.default_rng(seed), (nx, ny))
    with np.errstate(all="ignore"):  # a rejected trial step may overflow
        _, _, saves, _ = adaptive(f, u0, 0.0, t_relax, 1e-6, PIDController(rtol=1e-4, atol=1e-6), 10**6, [t_relax])
    return saves[0]


def steps(f, y, dt, n, kind):
    """n fixed substeps of Euler / RK4 / Tsit5 of the autonomous f(t, y)"""
    step = {"euler": O.euler_step, "rk4": O.rk4_step, "tsit5": lambda f_, t, y_, h: O.tsit5_step(f_, t, y_, h)[0]}[kind]
    for i in range(n):
        y = step(f, i * dt, y, dt)
    return y


def adaptive(f, y0, t0, t1, dt0, controller, max_trials, save_ts=()):
    """the first ``max_trials`` trial steps of ``integrate._solve_adaptive`` (one environment): returns
    ``(accepts, err_norms, saves, t)`` -- the accept / reject flags and scaled error norms in trial order, the dense
    output at the save times reached, the time reached"""
    from pde_opt_amd.integrate import _clip_dt, _pid_update

    c = controller
    y, t, dt = np.asarray(y0, dtype=np.float64), float(t0), float(dt0)
    ts = [float(v) for v in save_ts]
    accepts, errs, saves = [], [], []
    prev = pprev = 1.0
    k1, qi = None, 0
    while t < t1 and len(accepts) < max_trials:
        h = min(dt, t1 - t)
        y1, err, k7, ks = O.tsit5_step(f, t, y, h, k1=k1, return_slopes=True)
        k1 = ks[0]
        sc = c.atol + c.rtol * np.maximum(np.abs(y), np.abs(y1))
        en = float(np.sqrt(np.mean((err / sc) ** 2)))
        keep, fac, inv = _pid_update(c, en, prev, pprev)
        accepts.append(keep)
        errs.append(en)
        if keep:
            t_new = t + h
            while qi < len(ts) and ts[qi] <= t_new + 1e-14 * max(1.0, abs(t_new)):
                saves.append(O.tsit5_dense(y, h, ks, min(1.0, max(0.0, (ts[qi] - t) / h))))
                qi += 1
            y, k1 = y1, k7
            t = t_new if t_new < t1 - 1e-14 * max(1.0, abs(t1)) else t1
            pprev, prev = prev, inv
        dt = _clip_dt(c, h * fac)
    return accepts, errs, saves, t
