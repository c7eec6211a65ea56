"""fp64 numpy tangent-linear reference of the Cahn-Hilliard FD right-hand side and its IMEX / Euler steps, built on
the oracle's primitives (oracle/np_oracle.py).  Test infrastructure only: the GPU tangents (csrc/sens.hip) and the
finite differences of the oracle are both checked against it."""
import numpy as np

from oracle import np_oracle as O
from pde_opt_amd.numerics.closures import EXP_WRAP, LOGIT_PRIOR, MIX_ENTROPY, POLY

MU_ROLE, MOB_ROLE = 0, 1


def _series_basis(desc, k, c):
    if desc.kind == POLY:
        return c ** k
    e = np.zeros(k + 1)
    e[k] = 1.0
    return np.polynomial.legendre.legval(2.0 * c - 1.0, e)


def _series_dc(desc, c):
    a = np.asarray(desc.coef, dtype=np.float64)
    if desc.kind == POLY:
        return np.polynomial.polynomial.polyval(c, np.polynomial.polynomial.polyder(a)) if len(a) > 1 else 0.0 * c
    return 2.0 * np.polynomial.legendre.legval(2.0 * c - 1.0, np.polynomial.legendre.legder(a)) if len(a) > 1 else 0.0 * c


def closure_dc(desc, c):
    """d f / d c of a closure-family member"""
    d = _series_dc(desc, c)
    if desc.flags & LOGIT_PRIOR:
        d = d + 1.0 / (c * (1.0 - c))
    if desc.flags & MIX_ENTROPY:
        d = d + np.log(c / (1.0 - c))
    if desc.flags & EXP_WRAP:
        d = d * desc(c)
    return d


def closure_dcoef(desc, k, c):
    """d f / d coef[k]"""
    b = _series_basis(desc, k, c)
    return b * desc(c) if desc.flags & EXP_WRAP else b


def ch_rhs(u, hx, hy, kappa, mu, mob):
    return O.ch_rhs_fd(u, hx, hy, kappa, mu, mob)


def tangent_rhs(u, du, hx, hy, kappa, mu, mob, role, k):
    """J_f(u) du + d f / d p for the parameter coef[k] of closure `role`"""
    m = O.chem_potential(u, hx, hy, kappa, mu)
    D = mob(u)
    dmu = closure_dc(mu, u) * du - kappa * O.lap5(du, hx, hy)
    dD = closure_dc(mob, u) * du
    if role == MU_ROLE:
        dmu = dmu + closure_dcoef(mu, k, u)
    else:
        dD = dD + closure_dcoef(mob, k, u)
    out = 0.0
    for ax, h in ((0, hx), (1, hy)):
        F = O.avg_face(dD, ax) * O.grad_face(m, h, ax) + O.avg_face(D, ax) * O.grad_face(dmu, h, ax)
        out = out + O.div_face(F, h, ax)
    return out


def step(u, dus, params, dt, hx, hy, kappa, mu, mob, integrator, A=0.5, symbol=None):
    """one IMEX (integrator "imex") or Euler step of the state and its tangents; params = [(role, k), ...]"""
    f = ch_rhs(u, hx, hy, kappa, mu, mob)
    dfs = [tangent_rhs(u, du, hx, hy, kappa, mu, mob, r, k) for du, (r, k) in zip(dus, params)]
    if integrator == "imex":
        L = 1.0 + A * dt * symbol
        solve = lambda g: np.fft.ifftn(np.fft.fftn(g) / L).real
        return u + dt * solve(f), [du + dt * solve(df) for du, df in zip(dus, dfs)]
    return u + dt * f, [du + dt * df for du, df in zip(dus, dfs)]


def trajectory(u0, params, dt, n, hx, hy, kappa, mu, mob, integrator, A=0.5, symbol=None):
    u, dus = u0, [np.zeros_like(u0) for _ in params]
    for _ in range(n):
        u, dus = step(u, dus, params, dt, hx, hy, kappa, mu, mob, integrator, A, symbol)
    return u, dus


def perturbed(mu, mob, role, k, eps):
    """(mu, mob) with coef[k] of closure `role` moved by eps"""
    def bump(d):
        c = list(d.coef)
        c[k] += eps
        return d.with_coef(c)

    return (bump(mu), mob) if role == MU_ROLE else (mu, bump(mob))
