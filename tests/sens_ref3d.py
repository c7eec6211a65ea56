"""fp64 numpy tangent-linear reference of the 3-D Cahn-Hilliard FD right-hand side (CahnHilliard3DPeriodic.rhs_fd,
cahn_hilliard.py:180-200) and its IMEX / Euler steps, built on the oracle (oracle/np_oracle.py: ch3d_rhs_fd, the face
operators, imex_step).  The closure derivatives are those of tests/sens_ref.py.  Test infrastructure only: the GPU
tangents (csrc/sens.hip, sens3d_*) and the finite differences of the oracle are both checked against it.

``h`` is the spacing triple ``(hx, hy, hz)``; fields are ``(nx, ny, nz)``."""
import numpy as np

from oracle import np_oracle as O
from sens_ref import MOB_ROLE, MU_ROLE, closure_dc, closure_dcoef, perturbed  # noqa: F401 (re-exported)


def lap7(u, h):
    """7-point Laplacian, in the oracle's order (x, y, z terms)"""
    return sum((O.nb(u, 1, ax) - 2 * u + O.nb(u, -1, ax)) / h[ax] ** 2 for ax in range(3))


def ch_rhs(u, h, kappa, mu, mob):
    return O.ch3d_rhs_fd(u, h[0], h[1], h[2], kappa, mu, mob)


def tangent_rhs(u, du, h, kappa, mu, mob, role, k):
    """J_f(u) du + d f / d p for the parameter coef[k] of closure `role`"""
    m = mu(u) - kappa * lap7(u, h)
    D = mob(u)
    dmu = closure_dc(mu, u) * du - kappa * lap7(du, h)
    dD = closure_dc(mob, u) * du
    if role == MU_ROLE:
        dmu = dmu + closure_dcoef(mu, k, u)
    else:
        dD = dD + closure_dcoef(mob, k, u)
    out = 0.0
    for ax in range(3):
        F = O.avg_face(dD, ax) * O.grad_face(m, h[ax], ax) + O.avg_face(D, ax) * O.grad_face(dmu, h[ax], ax)
        out = out + O.div_face(F, h[ax], ax)
    return out


def step(u, dus, params, dt, h, kappa, mu, mob, integrator, A=0.5, symbol=None):
    """one IMEX (integrator "imex") or Euler step of the state and its tangents; params = [(role, k), ...].  The
    implicit operator 1 + A dt symbol does not depend on the closure coefficients, so the tangents see the same
    implicit solve (oracle imex_step) applied to their linearised slope."""
    f = ch_rhs(u, h, kappa, mu, mob)
    dfs = [tangent_rhs(u, du, h, kappa, mu, mob, r, k) for du, (r, k) in zip(dus, params)]
    if integrator == "imex":
        adv = lambda y, g: O.imex_step(lambda t, _y: g, 0.0, y, dt, A, symbol)
        return adv(u, f), [adv(du, df) for du, df in zip(dus, dfs)]
    return u + dt * f, [du + dt * df for du, df in zip(dus, dfs)]


def trajectory(u0, params, dt, n, h, kappa, mu, mob, integrator, A=0.5, symbol=None):
    u, dus = u0, [np.zeros_like(u0) for _ in params]
    for _ in range(n):
        u, dus = step(u, dus, params, dt, h, kappa, mu, mob, integrator, A, symbol)
    return u, dus
