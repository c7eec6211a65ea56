"""PDEModel.train / optimize on a constant-current Butler-Volmer run (tests/bv_fit_problem.py): mu and j0 recovered from
frames, with and without the voltage curve, and the gradient of a torch objective against the numpy reference's."""
import numpy as np
import pytest

import bv_fit_problem as F
import pde_opt_amd as P
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg

pytestmark = pytest.mark.gpu

CURRENT = P.AllenCahn2DPeriodicButlerVolmerConstantCurrent
OTHER = {"kappa": F.KAPPA, "alpha": F.ALPHA, "Crate": F.CRATE}

# The same fits on the CPU (fp64 numpy tangents under the same Levenberg-Marquardt: `python tests/bv_fit_problem.py`) end at
#   voltage_weight = 0:  max |p - p_true| over the identifiable entries = 5.548e-12, loss = 2.636e-34   (14 solves)
#   voltage_weight = 1:  max |p - p_true| = 2.779e-11, loss = 4.749e-31                                  (24 solves)
# and the GPU fit is gated at 10 x those values (the convention of tests/test_gpu_sens_ac.py).
CPU_FIT = {0.0: (5.548e-12, 2.636e-34), F.VOLTAGE_WEIGHT: (2.779e-11, 4.749e-31)}


def domain():
    return P.Domain((F.NX, F.NY), ((0.0, F.H * F.NX), (0.0, F.H * F.NY)), "dimensionless")


def truth():
    return {"mu": ChemLeg(np.array(F.MU_TRUE), F.logit), "j0": DiffLeg(np.array(F.J0_TRUE)), **OTHER}


@pytest.fixture(scope="module")
def problem():
    model = P.PDEModel(CURRENT, domain(), P.RK4)
    y0s = F.y0s()
    sol = model.solve(truth(), y0s, F.TS, {})  # (T, B, nx, ny): noise-free synthetic data
    eq = CURRENT(domain(), **truth())
    vs = np.stack([eq.get_voltage(sol[q]) for q in range(len(F.TS))])  # (T, B)
    return model, y0s, sol, vs


@pytest.mark.parametrize("voltage_weight", [0.0, F.VOLTAGE_WEIGHT])
def test_fit_recovers_mu_and_j0(problem, voltage_weight):
    model, y0s, sol, vs = problem
    B, T = len(y0s), len(F.TS)
    data = {"ys": [sol[q, b] for b in range(B) for q in range(T)], "ts": np.tile(F.TS, B),
            "vs": [vs[q, b] for b in range(B) for q in range(T)]}
    inds = [[b * T + q for q in range(T)] for b in range(B)]
    init = {"mu": ChemLeg(np.array(F.MU_INIT), F.logit), "j0": DiffLeg(np.array(F.J0_INIT))}
    res = model.train(data, inds, init, OTHER, {}, {}, 0.0, method="least_squares", max_steps=100, voltage_weight=voltage_weight)
    p = np.concatenate([res["mu"].expansion.params, res["j0"].expansion.params])
    err = F.param_error(p, bool(voltage_weight))
    values = np.swapaxes(sol, 0, 1)[:, 1:]
    final = model.mse(res, (y0s, values), {}, F.TS, {}, 0.0)
    if voltage_weight:
        eq = CURRENT(domain(), **res)
        pred = model.solve(res, y0s, F.TS, {})
        v_fit = np.stack([eq.get_voltage(pred[q]) for q in range(1, T)])
        final += voltage_weight * float(np.mean((vs[1:] - v_fit) ** 2))
    print(f"voltage_weight = {voltage_weight}: p = {p}, error = {err:.3e}, loss = {final:.3e}")
    cpu_err, cpu_final = CPU_FIT[voltage_weight]
    assert isinstance(res["mu"], ChemLeg) and res["mu"].prior_fn is F.logit and isinstance(res["j0"], DiffLeg)
    if voltage_weight:
        # the voltage curve pins mu's constant coefficient (dv / dmu_0 = -1)
        assert abs(p[0] - F.MU_TRUE[0]) < 0.1 * abs(F.MU_INIT[0] - F.MU_TRUE[0])
    else:
        # the frames cannot see it (v absorbs a shift of mu): it stays where it started, and the leading coefficient the
        # frames do see is mu's linear one
        assert abs(p[0] - F.MU_INIT[0]) <= 1e-6
        assert abs(p[1] - F.MU_TRUE[1]) < 0.1 * abs(F.MU_INIT[1] - F.MU_TRUE[1])
    assert err <= 10 * cpu_err
    assert final <= 10 * cpu_final


def test_optimize_gradient_matches_the_reference(problem):
    """the gradient optimize works with, for a torch objective on the final frame (one trajectory, the first 60 steps: the
    numpy reference advances five tangent fields on the CPU), then one optimize call"""
    import torch

    model, y0s, _, _ = problem
    y0, steps = y0s[:1], (30, 60)
    ts = np.array([0.0] + [k * F.DT for k in steps])
    target = torch.tensor(F.reference_solve(np.array(F.MU_TRUE + F.J0_TRUE), y0, tangents=False, save_steps=steps)[0][-1])
    objective = lambda ys: 0.5 * torch.sum((ys[-1] - target) ** 2)  # noqa: E731
    init = {"mu": ChemLeg(np.array(F.MU_INIT), F.logit), "j0": DiffLeg(np.array(F.J0_INIT))}
    value_and_grad, _, pmap = model._objective_functions(objective, y0, ts, init, OTHER, {}, {}, 0.0)
    p0 = pmap.flatten(init)
    J, g = value_and_grad(p0)
    ys, _, dys, _ = F.reference_solve(p0, y0, save_steps=steps)
    r = ys[-1] - target.numpy()
    J_ref = 0.5 * float(np.sum(r ** 2))
    g_ref = np.array([np.sum(r * dys[-1][:, j]) for j in range(len(F.PARAMS))])
    print(f"J = {J:.12e} (reference {J_ref:.12e}), gradient {g}, reference {g_ref}")
    assert abs(J - J_ref) <= 1e-8 * J_ref
    assert np.linalg.norm(g - g_ref) <= 1e-8 * np.linalg.norm(g_ref)
    res = model.optimize(objective, y0, ts, init, OTHER, {}, {}, 0.0, max_steps=1)
    assert model.last_optimize_history[-1] < model.last_optimize_history[0]
    assert isinstance(res["mu"], ChemLeg) and isinstance(res["j0"], DiffLeg)
