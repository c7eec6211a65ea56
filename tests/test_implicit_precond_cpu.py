"""The spectral preconditioner of ImplicitEuler without a GPU: the reference symbol (tests/implicit_precond_ref.py) inverts
the finite-difference operator exactly where that operator has constant coefficients, the states of the GPU tests are
ones the preconditioner helps on, and the keyword refuses what it does not know."""
import numpy as np
import pytest

import pde_opt_amd as P
from pde_opt_amd.numerics.closures import POLY, ClosureDesc

import implicit_problems as Q
import implicit_precond_ref as PR
import implicit_ref as R

LINEAR_MU = ClosureDesc(POLY, 0, (0.1, 1.5))  # mu_h = 0.1 + 1.5 c: slope > 0
CONST_D = ClosureDesc(POLY, 0, (0.7,))


# ---- (a) M equals A for constant D and linear mu_h ---------------------------------------------------------------------
@pytest.mark.parametrize("spacing", [(0.01, 0.01), (0.01, 0.013)])
@pytest.mark.parametrize("grid", ["24x40", "45x33", "64x64"])
@pytest.mark.parametrize("eq", ["ch", "ac"])
def test_symbol_inverts_the_constant_coefficient_operator(eq, grid, spacing):
    points = PR.GRIDS[grid]
    hx, hy = spacing
    rng = np.random.default_rng(5)
    u = rng.uniform(0.2, 0.8, points)
    v = rng.standard_normal(points)
    L = 4.0 / hx**2 + 4.0 / hy**2
    dt = 50.0 * 2.0 / (0.7 * (Q.KAPPA * L * L + 1.5 * L) if eq == "ch" else 0.7 * (Q.KAPPA * L + 1.5))
    z = PR.minv(eq, u, v, dt, hx, hy, Q.KAPPA, LINEAR_MU, CONST_D)
    back = R.apply_op(eq, u, z, dt, hx, hy, Q.KAPPA, LINEAR_MU, CONST_D)
    err = float(np.max(np.abs(back - v))) / float(np.max(np.abs(v)))
    print(f"A M^-1 v - v, {eq} {grid} h = {spacing}: {err:.3e} max|v|")
    assert err <= 1e-10
    if eq == "ch":  # M(0) = 1: the mean passes through
        assert abs(float(np.mean(z)) - float(np.mean(v))) <= 1e-13 * float(np.max(np.abs(v)))


# ---- (b) the states of the GPU iteration-count tests -------------------------------------------------------------------
@pytest.mark.parametrize("state", list(PR.STATES))
@pytest.mark.parametrize("closures", list(Q.CLOSURES))
@pytest.mark.parametrize("grid", list(PR.GRIDS))
@pytest.mark.parametrize("eq", ["ch", "ac"])
def test_preconditioned_reference_needs_at_most_half_the_iterations(eq, grid, closures, state):
    points, mu, mob, y, dt = PR.count_problem(eq, grid, state, closures)
    rtol, atol = Q.TOL[np.float64]
    y_plain, _, plain = PR.newton_counts(eq, y, dt, Q.H, Q.H, Q.KAPPA, mu, mob, rtol, atol, False)
    y_pre, _, pre = PR.newton_counts(eq, y, dt, Q.H, Q.H, Q.KAPPA, mu, mob, rtol, atol, True)
    print(f"reference Krylov counts {eq} {grid} {closures} {state}: plain {plain}, preconditioned {pre}")
    assert 2 * sum(pre) <= sum(plain)
    assert 2 * max(pre) <= max(plain)  # per Newton iterate as well
    assert R.rms(y_pre - y_plain) <= 10.0 * (atol + rtol * R.rms(y_plain))


# ---- (c) the keyword -----------------------------------------------------------------------------------------------------
def test_unknown_preconditioner_raises_at_construction():
    with pytest.raises(ValueError, match="precond"):
        P.ImplicitEuler(1e-8, 1e-10, precond="x")
    assert P.ImplicitEuler(1e-8, 1e-10).precond is None
    assert P.ImplicitEuler(1e-8, 1e-10, precond="spectral").precond == "spectral"
