"""numpy reference of the phase-field observables (csrc/pf_obs.hip): the eight sums, the
finite-difference right-hand sides they are consistent with, and a stepping loop.  ``dtype=np.float64`` is the reference;
``dtype=np.float32`` forms every per-cell term in fp32 -- the arithmetic of an fp32 kernel -- and still sums in fp64.

A problem is a dict ``spec``: ``eq`` in ("ch", "ac", "ch3d"), ``h`` the spacings, ``kappa``, ``mu`` and ``mob`` closures
(``Closure`` below: the in-kernel family, evaluated in the kernels' order of operations)."""
import dataclasses

import numpy as np

NAMES = ("mass", "u2", "f_bulk", "f_grad", "mu", "mu2", "diss", "nonfinite")


@dataclasses.dataclass(frozen=True)
class Closure:
    kind: str  # "poly": sum a_k c^k; "legendre": sum a_k P_k(2c - 1)
    coef: tuple
    logit: bool = False  # + log(c / (1 - c))
    exp: bool = False    # then exp(.)

    def desc(self):
        """the package's descriptor of the same closure"""
        from pde_opt_amd.numerics import closures as C

        flags = (C.LOGIT_PRIOR if self.logit else 0) | (C.EXP_WRAP if self.exp else 0)
        return C.ClosureDesc(C.POLY if self.kind == "poly" else C.LEGENDRE, flags, tuple(float(v) for v in self.coef))


def evaluate(cl, c):
    """closure value in c's dtype: Horner / the forward three-term recurrence (closures.hpp: series_generic)"""
    T = c.dtype.type
    a = [T(v) for v in cl.coef]
    if cl.kind == "poly":
        r = np.full_like(c, a[-1])
        for v in a[-2::-1]:
            r = r * c + v
    else:
        x = T(2) * c - T(1)
        r = np.full_like(c, a[0])
        if len(a) > 1:
            r = r + a[1] * x
        pm, pc = np.ones_like(x), x
        for k in range(2, len(a)):
            pn = (T(2 * k - 1) * x * pc - T(k - 1) * pm) / T(k)
            r = r + a[k] * pn
            pm, pc = pc, pn
    if cl.logit:
        r = r + np.log(c / (T(1) - c))
    if cl.exp:
        r = np.exp(r)
    return r


def antiderivative(cl, c):
    """f_h(c) = int_0^c of a closure without exp, in c's dtype (pf_obs.hip: antiderivative_generic)"""
    assert not cl.exp
    T = c.dtype.type
    a = [T(v) for v in cl.coef]
    n = len(a)
    if cl.kind == "poly":
        r = np.full_like(c, a[-1] / T(n))
        for k in range(n - 2, -1, -1):
            r = r * c + a[k] / T(k + 1)
        r = r * c
    else:
        x = T(2) * c - T(1)
        r = a[0] * c
        pm, pc = np.ones_like(x), x
        for k in range(1, n):
            pn = (T(2 * k + 1) * x * pc - T(k) * pm) / T(k + 1)
            r = r + a[k] * (pn - pm) / T(2 * (2 * k + 1))
            pm, pc = pc, pn
    if cl.logit:
        with np.errstate(divide="ignore", invalid="ignore"):
            r = r + np.where(c == 0, T(0), c * np.log(c)) + np.where(c == 1, T(0), (T(1) - c) * np.log(T(1) - c))
    return r


def second_derivative_bound(cl, lo, hi):
    """max |mu_h''| over [lo, hi] (the third derivative of f_h: what a central difference of F leaves behind)"""
    c = np.linspace(lo, hi, 2001)
    if cl.kind == "poly":
        d2 = np.polynomial.polynomial.polyval(c, np.polynomial.polynomial.polyder(np.asarray(cl.coef, float), 2)) if len(cl.coef) > 2 else 0 * c
    else:
        d2 = 4.0 * np.polynomial.legendre.legval(2 * c - 1, np.polynomial.legendre.legder(np.asarray(cl.coef, float), 2)) if len(cl.coef) > 2 else 0 * c
    if cl.logit:
        d2 = d2 - 1 / c**2 + 1 / (1 - c) ** 2
    return float(np.max(np.abs(d2)))


def _axes(spec):
    return 3 if spec["eq"] == "ch3d" else 2


def _recip(spec, T):
    return [T(1.0 / h) for h in spec["h"]], [T(1.0 / (h * h)) for h in spec["h"]]


def chem_pot(u, spec):
    """mu = mu_h(u) - kappa lap(u) over the trailing axes, the stage kernels' expression (lap_at / ch3d_mu_kernel)"""
    T = u.dtype.type
    nd = _axes(spec)
    _, r2 = _recip(spec, T)
    lap = None
    for ax in range(nd):
        a = u.ndim - nd + ax
        term = (np.roll(u, -1, a) - T(2) * u + np.roll(u, 1, a)) * r2[ax]
        lap = term if lap is None else lap + term
    return evaluate(spec["mu"], u) - T(spec["kappa"]) * lap


def rhs_fd(u, spec):
    """the finite-difference right-hand side (rhs_generic_point / ch3d_stage_kernel), in u's dtype"""
    T = u.dtype.type
    nd = _axes(spec)
    m, d = chem_pot(u, spec), evaluate(spec["mob"], u)
    if spec["eq"] == "ac":
        return -d * m
    r1, _ = _recip(spec, T)
    out = None
    for ax in range(nd):
        a = u.ndim - nd + ax
        flux = (T(0.5) * (d + np.roll(d, -1, a))) * ((np.roll(m, -1, a) - m) * r1[ax])  # at the forward face
        term = (flux - np.roll(flux, 1, a)) * r1[ax]
        out = term if out is None else out + term
    return out


def terms(u, spec, dtype=np.float64):
    """the per-cell terms, ``(8,) + u.shape`` float64, formed in ``dtype``"""
    T = np.dtype(dtype).type
    v = np.asarray(u).astype(dtype)
    nd = _axes(spec)
    r1, _ = _recip(spec, T)
    m, d = chem_pot(v, spec), evaluate(spec["mob"], v)
    g2, diss = np.zeros_like(v), np.zeros_like(v)
    for ax in range(nd):
        a = v.ndim - nd + ax
        g = (np.roll(v, -1, a) - v) * r1[ax]
        g2 = g2 + g * g
        if spec["eq"] != "ac":
            gm = (np.roll(m, -1, a) - m) * r1[ax]
            diss = diss + (T(0.5) * (d + np.roll(d, -1, a))) * gm * gm
    if spec["eq"] == "ac":
        diss = d * m * m
    bad = ~(np.isfinite(v) & np.isfinite(m))
    out = [v, v * v, antiderivative(spec["mu"], v), T(0.5) * T(spec["kappa"]) * g2, m, m * m, diss, bad]
    return np.stack([np.asarray(t, dtype=np.float64) for t in out])


def observables(u, spec, dtype=np.float64):
    """``(values (..., 8), scale (..., 8))`` of one state or a batch (leading axes): the sums over the grid times
    ``h = prod(spacings)`` (the count as it is), and ``h sum |term|`` -- the scale of a summation error bound"""
    t = terms(u, spec, dtype)
    nd = _axes(spec)
    axes = tuple(range(t.ndim - nd, t.ndim))
    h = float(np.prod(spec["h"]))
    w = np.array([h] * 7 + [1.0])
    return np.moveaxis(t.sum(axis=axes), 0, -1) * w, np.moveaxis(np.abs(t).sum(axis=axes), 0, -1) * w


def free_energy(u, spec):
    v, _ = observables(u, spec)
    return v[..., 2] + v[..., 3]


def euler_steps(u, spec, dt, n):
    for _ in range(n):
        u = u + dt * rhs_fd(u, spec)
    return u


def rk4_steps(u, spec, dt, n):
    for _ in range(n):
        k1 = rhs_fd(u, spec)
        k2 = rhs_fd(u + 0.5 * dt * k1, spec)
        k3 = rhs_fd(u + 0.5 * dt * k2, spec)
        k4 = rhs_fd(u + dt * k3, spec)
        u = u + dt / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
    return u


def imex_steps(u, spec, dt, n, A=0.5):
    """SemiImplicitFourierSpectral on a 2-D Cahn-Hilliard problem: u += dt ifft(fft(rhs_fd(u)) / (1 + A dt kappa k^4))"""
    nx, ny = u.shape[-2:]
    kx = 2 * np.pi * np.fft.fftfreq(nx, spec["h"][0])[:, None]
    ky = 2 * np.pi * np.fft.fftfreq(ny, spec["h"][1])[None, :]
    den = 1.0 + A * dt * spec["kappa"] * (kx**2 + ky**2) ** 2
    for _ in range(n):
        u = u + dt * np.real(np.fft.ifft2(np.fft.fft2(rhs_fd(u, spec)) / den))
    return u


def smooth_noise_states(shape, batch, seed=0, lo=0.05, hi=0.95):
    """``batch`` different smooth-plus-noise states with values in [lo, hi]"""
    rng = np.random.default_rng(seed)
    grids = np.meshgrid(*[np.arange(n) / n for n in shape], indexing="ij")
    out = []
    for b in range(batch):
        s = sum(np.sin(2 * np.pi * ((b % 2) + 1) * g + 0.7 * b + 0.3 * i) for i, g in enumerate(grids)) / len(shape)
        s = 0.5 + 0.3 * s + 0.15 * rng.uniform(-1, 1, shape)
        out.append(lo + (hi - lo) * np.clip(s, 0.0, 1.0))
    return np.stack(out)
