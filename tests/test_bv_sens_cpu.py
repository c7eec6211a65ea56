"""The numpy tangent reference of the Butler-Volmer equations (tests/bv_sens_ref.py) against central differences of
tests/bv_ref.py in fp64, the host-side voltage terms of the Gauss-Newton sums against a brute-force Jacobian, and the
refusals of the Butler-Volmer sensitivity path that need no GPU.

Measured here (fp64, the problem of bv_sens_ref: relaxed_state(3, 20, 70), P = 5, C = 0.02, 40 steps of 1e-4, central
differences with eps = 1e-5), worst relative L2 over the tangents:

    right-hand side   constant current 4.08e-10, smoothed boundary 3.40e-10, given voltage 4.18e-10   (asserted <= 5e-9)
    voltage tangents  within 5e-9 max(|dv|, 1) of the central difference for every parameter             (asserted)
    trajectories      Euler 1.34e-08, RK4 2.58e-08   (mu's constant coefficient apart: its state tangent is exactly 0)

The trajectory figure, bv_sens_ref.CD_MEASURED = 2.6e-8, is the measured value behind the central-difference
gate of tests/test_gpu_bv_sens.py (10 x CD_MEASURED)."""
import types

import numpy as np
import pytest

import bv_ref as R
import bv_sens_ref as S
import pde_opt_amd as P
from pde_opt_amd import fit
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg

NX, NY = 20, 70
MU, J0 = S.Closure(S.MU_DESC), S.Closure(S.J0_DESC)
EPS = S.CD_EPS


def logit(c):
    return np.log(c / (1.0 - c))


@pytest.fixture(scope="module")
def state():
    u = R.relaxed_state(3, NX, NY)
    assert 0.05 < u.min() and u.max() < 0.95
    return u


@pytest.fixture(scope="module")
def tangents():
    return list(0.05 * np.random.default_rng(11).standard_normal((len(S.PARAMS), NX, NY)))


def _cd(fn, j):
    """central difference of fn(mu, j0) in parameter j"""
    role, k = S.PARAMS[j]
    return (fn(*S.perturbed(MU, J0, role, k, EPS)) - fn(*S.perturbed(MU, J0, role, k, -EPS))) / (2 * EPS)


@pytest.mark.parametrize("kind", ["current", "sbm", "voltage"])
def test_tangent_rhs_against_central_differences(state, tangents, kind):
    psi = R.disc_psi(NX, NY) if kind == "sbm" else None
    C = S.CRATES[0]
    if kind == "voltage":
        f = lambda u, mu, j0: R.rhs_voltage(u, S.H, S.H, S.KAPPA, S.ALPHA, 0.05, mu, j0)  # noqa: E731
        _, dks = S.slopes_voltage(state, tangents, S.PARAMS, S.H, S.H, S.KAPPA, S.ALPHA, 0.05, MU, J0)
    else:
        f = lambda u, mu, j0: R.rhs_current(u, S.H, S.H, S.KAPPA, S.ALPHA, C, mu, j0, psi)  # noqa: E731
        _, dks = S.slopes_current(state, tangents, S.PARAMS, S.H, S.H, S.KAPPA, S.ALPHA, C, MU, J0, psi)
    worst = 0.0
    for j, du in enumerate(tangents):
        # d/d eps of f(u + eps du; p + eps e_j): the directional derivative the tangent right-hand side is
        role, k = S.PARAMS[j]
        hi = f(state + EPS * du, *S.perturbed(MU, J0, role, k, EPS))
        lo = f(state - EPS * du, *S.perturbed(MU, J0, role, k, -EPS))
        worst = max(worst, S.rel(dks[j], (hi - lo) / (2 * EPS)))
    print(f"{kind}: tangent rhs vs central differences {worst:.2e}")
    assert worst <= 5e-9


@pytest.mark.parametrize("kind", ["current", "sbm"])
def test_voltage_tangents_against_central_differences(state, tangents, kind):
    psi = R.disc_psi(NX, NY) if kind == "sbm" else None
    C = S.CRATES[1]
    v, dvs, _, _ = S.voltage_tangents(state, tangents, S.PARAMS, S.H, S.H, S.KAPPA, C, MU, J0, psi)
    assert v == R.voltage(state, S.H, S.H, S.KAPPA, C, MU, J0, psi)
    for j, du in enumerate(tangents):
        role, k = S.PARAMS[j]
        hi = R.voltage(state + EPS * du, S.H, S.H, S.KAPPA, C, *S.perturbed(MU, J0, role, k, EPS), psi)
        lo = R.voltage(state - EPS * du, S.H, S.H, S.KAPPA, C, *S.perturbed(MU, J0, role, k, -EPS), psi)
        cd = (hi - lo) / (2 * EPS)
        print(f"{kind} dv[{j}] = {dvs[j]:.6e}, central difference {cd:.6e}")
        assert abs(dvs[j] - cd) <= 5e-9 * max(abs(cd), 1.0)


def test_sqrt_wrapped_exchange_current(state, tangents):
    """the notebook's j0 = sqrt((1 - c) c), held fixed: its derivative in u enters the mu tangents"""
    j0 = S.Closure(S.J0_SQRT_DESC)
    np.testing.assert_allclose(j0(state), R.J0(state), rtol=1e-14)
    params = S.PARAMS[:3]
    C = S.CRATES[0]
    _, dks = S.slopes_current(state, tangents[:3], params, S.H, S.H, S.KAPPA, S.ALPHA, C, MU, j0)
    for j, (role, k) in enumerate(params):
        hi = R.rhs_current(state + EPS * tangents[j], S.H, S.H, S.KAPPA, S.ALPHA, C, MU.bumped(k, EPS), j0)
        lo = R.rhs_current(state - EPS * tangents[j], S.H, S.H, S.KAPPA, S.ALPHA, C, MU.bumped(k, -EPS), j0)
        assert S.rel(dks[j], (hi - lo) / (2 * EPS)) <= 5e-9
    # and as a trainable closure (not used by the classes, which train Legendre closures): d sqrt(r) / d coef
    d = j0.dcoef(1, state)
    cd = (j0.bumped(1, EPS)(state) - j0.bumped(1, -EPS)(state)) / (2 * EPS)
    assert S.rel(d, cd) <= 1e-8


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_tangent_trajectories_against_central_differences(state, integrator):
    """the measured value behind the central-difference gate of the GPU test"""
    C = S.CRATES[0]
    f = S.current_rhs(S.PARAMS, S.H, S.H, S.KAPPA, S.ALPHA, C, MU, J0)
    u, dus = S.trajectory(f, state, len(S.PARAMS), S.TRAJ_DT, S.TRAJ_STEPS, integrator)
    fwd = lambda mu, j0: R.steps(lambda t, y: R.rhs_current(y, S.H, S.H, S.KAPPA, S.ALPHA, C, mu, j0), state, S.TRAJ_DT,  # noqa: E731
                                 S.TRAJ_STEPS, integrator)
    assert S.rel(u, fwd(MU, J0)) <= 1e-13
    # mu's constant coefficient: at constant current a shift of mu is absorbed by v (I+- scale by e^{+-c/2}, so v -> v - c
    # and eta = mu + v stands still): its state tangent is identically zero, only the voltage feels it (dv/dp = -1)
    scale = np.linalg.norm(dus[1])
    assert np.linalg.norm(dus[0]) <= 1e-12 * scale and np.linalg.norm(_cd(fwd, 0)) <= 1e-9 * scale
    worst = max(S.rel(dus[j], _cd(fwd, j)) for j in range(1, len(S.PARAMS)))
    print(f"{integrator}: tangent trajectories vs central differences {worst:.2e}")
    assert worst <= S.CD_MEASURED


def test_voltage_terms_of_the_gauss_newton_sums_against_a_brute_force_jacobian():
    rng = np.random.default_rng(5)
    T1, B, Pn, M = 3, 2, 4, 640
    J_f, r_f = rng.standard_normal((M, Pn)), rng.standard_normal(M)  # the field part: r = data - pred, J = dpred/dp
    dv, r_v = rng.standard_normal((T1, B, Pn)), rng.standard_normal((T1, B))
    weight = 0.7
    w = weight * M / r_v.size
    got = fit.add_voltage_sums(float(r_f @ r_f), J_f.T @ r_f, J_f.T @ J_f, r_v, dv, w)
    # brute force: one stacked residual vector with the voltage rows scaled by sqrt(w)
    Jall = np.vstack([J_f, np.sqrt(w) * dv.reshape(-1, Pn)])
    rall = np.concatenate([r_f, np.sqrt(w) * r_v.reshape(-1)])
    np.testing.assert_allclose(got[0], rall @ rall, rtol=1e-13)
    np.testing.assert_allclose(got[1], Jall.T @ rall, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got[2], Jall.T @ Jall, rtol=1e-12, atol=1e-12)
    # folded into Objective(M = number of field residuals): ssr / M = mean(r_f^2) + weight mean(r_v^2)
    np.testing.assert_allclose(got[0] / M, np.mean(r_f ** 2) + weight * np.mean(r_v ** 2), rtol=1e-13)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _domain(psi=None):
    geo = None if psi is None else types.SimpleNamespace(smooth=psi)
    return P.Domain((NX, NY), ((0.0, S.H * NX), (0.0, S.H * NY)), "dimensionless", geo)


def _closures():
    return {"mu": ChemLeg(np.array(S.MU_COEF), logit), "j0": DiffLeg(np.array(S.J0_COEF))}


CURRENT = P.AllenCahn2DPeriodicButlerVolmerConstantCurrent
VOLTAGE = P.AllenCahn2DPeriodicButlerVolmer


def test_the_three_classes_are_accepted_with_euler_and_rk4():
    sbm = P.AllenCahn2DSmoothedBoundaryButlerVolmerConstantCurrent
    for cls, dom in ((CURRENT, _domain()), (VOLTAGE, _domain()), (sbm, _domain(R.disc_psi(NX, NY)))):
        for solver in (P.Euler, P.RK4):
            fit.reject_unsupported(P.PDEModel(cls, dom, solver))
        pm = fit.ParamMap.of(_closures(), cls)
        assert pm.sens_params() == S.PARAMS  # mu's constant coefficient is active, "j0" is the engine's second closure


def test_imex_and_tsit5_are_refused():
    for solver in (P.SemiImplicitFourierSpectral, P.Tsit5):
        try:
            model = P.PDEModel(CURRENT, _domain(), solver)
        except Exception:  # the pair may already be refused when the model is built
            continue
        with pytest.raises(NotImplementedError):
            fit.reject_unsupported(model)
        with pytest.raises(NotImplementedError):
            model.train({"ys": [], "ts": []}, [[0, 1]], _closures(), {}, {}, {}, 0.0)


def test_scalars_are_not_trainable():
    with pytest.raises(ValueError, match="other_parameters"):
        fit.ParamMap.of({"alpha": 0.5}, CURRENT)


def test_a_voltage_protocol_is_refused():
    model = P.PDEModel(VOLTAGE, _domain(), P.RK4)
    u = np.full((NX, NY), 0.3)
    other = {"kappa": S.KAPPA, "alpha": S.ALPHA, "v": lambda t: 0.1 * t}
    data = {"ys": [u, u], "ts": [0.0, 1e-6]}
    with pytest.raises(NotImplementedError, match="v\\(t\\)"):
        model.train(data, [[0, 1]], _closures(), other, {}, {}, 0.0)
    eq = VOLTAGE(_domain(), S.KAPPA, *_closures().values(), S.ALPHA, v=lambda t: 0.1 * t)
    with pytest.raises(NotImplementedError, match="v\\(t\\)"):
        fit.sensitivity_solve(None, eq, P.RK4(), u[None], [0.0, 1e-6], S.PARAMS)


def test_vs_on_a_given_voltage_class_is_refused():
    model = P.PDEModel(VOLTAGE, _domain(), P.RK4)
    u = np.full((NX, NY), 0.3)
    data = {"ys": [u, u], "ts": [0.0, 1e-6], "vs": [0.0, 0.0]}
    with pytest.raises(ValueError, match="voltage"):
        model.train(data, [[0, 1]], _closures(), {"kappa": S.KAPPA, "alpha": S.ALPHA, "v": 0.0}, {}, {}, 0.0, voltage_weight=1.0)
    with pytest.raises(NotImplementedError):
        model.voltage_sensitivities(_closures(), {"kappa": S.KAPPA, "alpha": S.ALPHA, "v": 0.0}, u[None], [0.0, 1e-6])


class _EdgeEngine:
    """stands in for the engine up to the first save point: the walk and its step-edge check are host code"""

    def __getattr__(self, name):
        if name == "sens_bv_voltage":
            return lambda: np.zeros((1, 1 + len(S.PARAMS)))
        return lambda *a, **k: None


def test_save_points_off_a_step_edge_are_refused():
    eq = CURRENT(_domain(), S.KAPPA, *_closures().values(), S.ALPHA, 0.02)
    u = np.full((1, NX, NY), 0.3)
    volt = []
    fit.sensitivity_solve(_EdgeEngine(), eq, P.RK4(), u, [0.0, 2e-6, 5e-6], S.PARAMS, dt0=1e-6, voltages=volt)
    assert len(volt) == 3
    with pytest.raises(ValueError, match="step edge"):
        fit.sensitivity_solve(_EdgeEngine(), eq, P.RK4(), u, [0.0, 2.5e-6, 5e-6], S.PARAMS, dt0=1e-6, voltages=[])
    with pytest.raises(ValueError, match="voltage"):  # a class without a voltage to solve for
        fit.sensitivity_solve(_EdgeEngine(), VOLTAGE(_domain(), S.KAPPA, *_closures().values(), S.ALPHA), P.RK4(), u, [0.0, 1e-6],
                              S.PARAMS, voltages=[])
