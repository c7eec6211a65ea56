"""fp64 numpy tangent-linear reference of the smoothed-boundary Allen-Cahn and Cahn-Hilliard right-hand sides and their
Euler / RK4 steps (stage times included), built on the oracle's primitives (oracle/np_oracle.py: sbm_inner, ac_sbm_rhs,
ch_sbm_rhs) and the closure derivatives of tests/sens_ref.py.  Test infrastructure only: the GPU tangents
(csrc/sens_sbm.hip) and the finite differences of the oracle are both checked against it.

A problem is a ``Problem``: equation ("ac" / "ch"), psi, spacings, kappa, the three closures (ClosureDesc), theta(t),
flux(t) and the mask.  The arithmetic follows the dtype of ``psi`` / ``u`` (float32 in, float32 out), so the reference's
own single-precision error can be measured."""
import dataclasses
from typing import Any, Callable

import numpy as np

from oracle import np_oracle as O
from sens_ref import MOB_ROLE, MU_ROLE, closure_dc, closure_dcoef, perturbed  # noqa: F401  (re-exported)


@dataclasses.dataclass
class Problem:
    eq: str  # "ac" (AllenCahn2DSmoothedBoundary) or "ch" (CahnHilliard2DSmoothedBoundary)
    psi: np.ndarray
    hx: float
    hy: float
    kappa: float
    f: Any
    mu: Any
    mob: Any  # R (ac) or D (ch)
    theta: Callable
    flux: Callable
    left_half: np.ndarray

    def with_closures(self, mu, mob):
        return dataclasses.replace(self, mu=mu, mob=mob)

    def astype(self, dtype):
        return dataclasses.replace(self, psi=self.psi.astype(dtype), left_half=self.left_half.astype(dtype))


def left_half(eq, shape):
    m = np.zeros(shape)
    if eq == "ac":
        m[:, :100] = 1.0  # allen_cahn.py:135
    else:
        m[:50, :] = 1.0  # cahn_hilliard.py:254
    return m


def wall_weight(p: Problem, t):
    """the field w(t) of the wall term, in the dtype of the mask"""
    dt = p.left_half.dtype.type
    th = p.theta(t)
    if p.eq == "ac":
        return dt(np.cos(th)) * p.left_half
    return dt(np.cos(th)) * p.left_half + dt(np.cos(np.pi - th)) * (1 - p.left_half)


def rhs(p: Problem, u, t):
    dt = u.dtype.type
    if p.eq == "ac":
        return O.ac_sbm_rhs(u, p.psi, dt(p.hx), dt(p.hy), dt(p.kappa), p.f, p.mu, p.mob, p.theta(t), p.left_half)
    return O.ch_sbm_rhs(u, p.psi, dt(p.hx), dt(p.hy), dt(p.kappa), p.f, p.mu, p.mob, p.theta(t), dt(p.flux(t)), p.left_half)


def _div_psi_grad(p, v):
    hx, hy = v.dtype.type(p.hx), v.dtype.type(p.hy)
    return O.div_face(O.avg_face(p.psi, 0) * O.grad_face(v, hx, 0), hx, 0) + O.div_face(
        O.avg_face(p.psi, 1) * O.grad_face(v, hy, 1), hy, 1)


def tangent_rhs(p: Problem, u, du, t, role, k):
    """J_f(u) du + d f / d p at time t, for the parameter coef[k] of closure `role` (MU_ROLE: mu, MOB_ROLE: R / D).  The
    source term g flux(t) has no tangent; where f(u) <= 0 the wall term's tangent is taken as 0."""
    T = u.dtype.type
    hx, hy, kappa = T(p.hx), T(p.hy), T(p.kappa)
    w = wall_weight(p, t).astype(u.dtype)
    g = O.sbm_norm_grad(p.psi, hx, hy)
    inner = O.sbm_inner(u, p.psi, hx, hy, kappa, p.f, p.mu, w)
    fe = p.f(u)
    with np.errstate(invalid="ignore", divide="ignore"):
        dsq = np.where(fe > 0, closure_dc(p.f, u) / np.sqrt(T(2) * fe), T(0)).astype(u.dtype)
    dinner = (closure_dc(p.mu, u) - np.sqrt(kappa) * g * w * dsq) * du - (kappa / p.psi) * _div_psi_grad(p, du)
    dmob = closure_dc(p.mob, u) * du
    if role == MU_ROLE:
        dinner = dinner + closure_dcoef(p.mu, k, u)
    else:
        dmob = dmob + closure_dcoef(p.mob, k, u)
    if p.eq == "ac":
        return (-dmob * inner - p.mob(u) * dinner).astype(u.dtype)
    D = p.mob(u)
    out = 0
    for ax, h in ((0, hx), (1, hy)):
        F = O.avg_face(p.psi, ax) * (O.avg_face(dmob, ax) * O.grad_face(inner, h, ax) + O.avg_face(D, ax) * O.grad_face(dinner, h, ax))
        out = out + O.div_face(F, h, ax)
    return (out / p.psi).astype(u.dtype)


def slopes(p, u, dus, params, t):
    return rhs(p, u, t), [tangent_rhs(p, u, du, t, r, k) for du, (r, k) in zip(dus, params)]


def step(p, u, dus, params, t, dt, integrator):
    """one Euler or classical RK4 step from time t of the state and its tangents; params = [(role, k), ...].  The RK4
    tangent is the derivative of the discrete step: every stage differentiates the right-hand side at the stage's own
    values and its own time (t, t + dt / 2, t + dt / 2, t + dt)"""
    f = lambda tt, v, dvs: slopes(p, v, dvs, params, tt)
    axpy = lambda a, k, dks: (u + a * k, [du + a * dk for du, dk in zip(dus, dks)])
    k1, d1 = f(t, u, dus)
    if integrator == "euler":
        return axpy(dt, k1, d1)
    assert integrator == "rk4", integrator
    k2, d2 = f(t + dt / 2, *axpy(dt / 2, k1, d1))
    k3, d3 = f(t + dt / 2, *axpy(dt / 2, k2, d2))
    k4, d4 = f(t + dt, *axpy(dt, k3, d3))
    comb = lambda a, b, c, d: (a + 2 * b + 2 * c + d) * (dt / 6)
    return u + comb(k1, k2, k3, k4), [du + comb(a, b, c, d) for du, a, b, c, d in zip(dus, d1, d2, d3, d4)]


def trajectory(p, u0, params, dt, n, integrator, t0=0.0):
    u, dus = u0, [np.zeros_like(u0) for _ in params]
    for s in range(n):
        u, dus = step(p, u, dus, params, t0 + s * dt, dt, integrator)
    return u, dus


def forward_trajectory(p, u0, dt, n, integrator, t0=0.0):
    return trajectory(p, u0, [], dt, n, integrator, t0)[0]
