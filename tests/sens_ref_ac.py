"""fp64 numpy tangent-linear reference of the Allen-Cahn FD right-hand side and its Euler / RK4 steps, built on the
oracle's primitives (oracle/np_oracle.py) and the closure derivatives of tests/sens_ref.py.  Test infrastructure only:
the GPU tangents (csrc/sens.hip) and the finite differences of the oracle are both checked against it."""
import numpy as np

from oracle import np_oracle as O
from sens_ref import MOB_ROLE, MU_ROLE, closure_dc, closure_dcoef, perturbed  # noqa: F401  (re-exported)

R_ROLE = MOB_ROLE  # the engine's second closure: Allen-Cahn's rate R


def ac_rhs(u, hx, hy, kappa, mu, R):
    return O.ac_rhs_fd(u, hx, hy, kappa, mu, R)


def tangent_rhs(u, du, hx, hy, kappa, mu, R, role, k):
    """J_f(u) du + d f / d p of f = -R(u) (mu_h(u) - kappa lap5 u), for the parameter coef[k] of closure `role`"""
    m = O.chem_potential(u, hx, hy, kappa, mu)
    dmu = closure_dc(mu, u) * du - kappa * O.lap5(du, hx, hy)
    dR = closure_dc(R, u) * du
    if role == MU_ROLE:
        dmu = dmu + closure_dcoef(mu, k, u)
    else:
        dR = dR + closure_dcoef(R, k, u)
    return -dR * m - R(u) * dmu


def slopes(u, dus, params, hx, hy, kappa, mu, R):
    return ac_rhs(u, hx, hy, kappa, mu, R), [tangent_rhs(u, du, hx, hy, kappa, mu, R, r, k) for du, (r, k) in zip(dus, params)]


def step(u, dus, params, dt, hx, hy, kappa, mu, R, integrator):
    """one Euler or classical RK4 step of the state and its tangents; params = [(role, k), ...].  The RK4 tangent is
    the derivative of the discrete step: every stage differentiates the right-hand side at the stage's own values"""
    f = lambda v, dvs: slopes(v, dvs, params, hx, hy, kappa, mu, R)
    axpy = lambda a, k, dks: (u + a * k, [du + a * dk for du, dk in zip(dus, dks)])
    k1, d1 = f(u, dus)
    if integrator == "euler":
        return axpy(dt, k1, d1)
    assert integrator == "rk4", integrator
    k2, d2 = f(*axpy(dt / 2, k1, d1))
    k3, d3 = f(*axpy(dt / 2, k2, d2))
    k4, d4 = f(*axpy(dt, k3, d3))
    comb = lambda a, b, c, d: (a + 2 * b + 2 * c + d) * (dt / 6)
    return u + comb(k1, k2, k3, k4), [du + comb(a, b, c, d) for du, a, b, c, d in zip(dus, d1, d2, d3, d4)]


def trajectory(u0, params, dt, n, hx, hy, kappa, mu, R, integrator):
    u, dus = u0, [np.zeros_like(u0) for _ in params]
    for _ in range(n):
        u, dus = step(u, dus, params, dt, hx, hy, kappa, mu, R, integrator)
    return u, dus
