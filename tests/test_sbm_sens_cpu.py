"""Smoothed-boundary sensitivities without a GPU: the numpy tangent reference (tests/sbm_sens_ref.py) against central
differences of the oracle, the stability of the trajectory tests' step sizes, and the host logic of the fitting surface
(fit.py) for AllenCahn2DSmoothedBoundary / CahnHilliard2DSmoothedBoundary."""
import numpy as np
import pytest

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd import fit
from pde_opt_amd.numerics.closures import UnsupportedClosureError
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg
import sbm_sens_problem as Q
import sbm_sens_ref as S
from util import SBM_F, SBM_FLUX, SBM_THETA, sbm_domain, sbm_psi

T_EVAL = 0.17  # theta(0.17) = 0.80, flux(0.17) = 0.030: both time terms away from their t = 0 values
ALL_PARAMS = [(S.MU_ROLE, k) for k in range(3)] + [(S.MOB_ROLE, k) for k in range(2)]


def _fd_coef(p, u, role, k, eps=1e-6):
    lo, hi = (p.with_closures(*S.perturbed(p.mu, p.mob, role, k, s * eps)) for s in (-1, 1))
    return (S.rhs(hi, u, T_EVAL) - S.rhs(lo, u, T_EVAL)) / (2 * eps)


@pytest.mark.parametrize("mob", list(Q.MOBS))
@pytest.mark.parametrize("eq,shape", [("ac", "24x120"), ("ch", "67x40"), ("ac", "64x64"), ("ch", "64x64")])
def test_tangent_rhs_against_central_differences(eq, shape, mob):
    p = Q.problem(eq, shape, mob)
    u = Q.state(p.psi.shape, 3)
    assert np.all(p.f(u) > 0)  # no test input reaches the zero of f
    assert p.left_half.min() == 0.0 or shape == "64x64"
    zero = np.zeros_like(u)
    # in u, along a random direction: J_f(u) v = tangent(u, v) - tangent(u, 0)
    v = np.random.default_rng(5).standard_normal(u.shape)
    eps = 1e-6
    fd = (S.rhs(p, u + eps * v, T_EVAL) - S.rhs(p, u - eps * v, T_EVAL)) / (2 * eps)
    jv = S.tangent_rhs(p, u, v, T_EVAL, S.MOB_ROLE, 0) - S.tangent_rhs(p, u, zero, T_EVAL, S.MOB_ROLE, 0)
    assert Q.rel(jv, fd) <= 1e-6
    # in every coefficient
    for role, k in ALL_PARAMS:
        got = S.tangent_rhs(p, u, zero, T_EVAL, role, k)
        if eq == "ch" and (role, k) == (S.MU_ROLE, 0):
            # a constant added to `inner` drops out of grad(inner): this tangent is identically zero
            assert np.abs(got).max() <= 1e-12 and np.abs(_fd_coef(p, u, role, k)).max() <= 1e-6
            continue
        assert Q.rel(got, _fd_coef(p, u, role, k)) <= 1e-6, (role, k)


def test_wall_term_depends_on_time_and_source_term_has_no_tangent():
    p = Q.problem("ch", "67x40")
    u, v = Q.state(p.psi.shape, 3), np.random.default_rng(5).standard_normal(p.psi.shape)
    a = S.tangent_rhs(p, u, v, 0.0, S.MU_ROLE, 1)
    b = S.tangent_rhs(p, u, v, T_EVAL, S.MU_ROLE, 1)
    assert Q.rel(a, b) > 1e-3  # theta(t) enters the linearised wall term
    q = Q.problem("ch", "67x40", flux=lambda t: 5.0)
    np.testing.assert_array_equal(S.tangent_rhs(q, u, v, T_EVAL, S.MU_ROLE, 1), b)  # g flux(t): no u, no parameter
    assert Q.rel(S.rhs(q, u, T_EVAL), S.rhs(p, u, T_EVAL)) > 1e-3


def test_zero_of_f_gives_no_wall_tangent():
    import dataclasses

    p = Q.problem("ac", "24x120")
    coef = list(Q.F.coef)
    coef[0] -= 0.02  # SBM_F's minimum is 0.0006 at c = 0.07: lowered, f has a zero
    p = dataclasses.replace(p, f=Q.F.with_coef(coef))
    u = np.clip(Q.state(p.psi.shape, 3), 0.2, 0.8)
    u[3, 4] = 0.07  # f < 0 there: sqrt(2 f) is NaN in the forward value, the tangent of the wall term is taken as 0
    assert p.f(u)[3, 4] < 0 and np.all(np.delete(p.f(u).ravel(), 3 * 120 + 4) > 0)
    with np.errstate(invalid="ignore"):
        d = S.tangent_rhs(p, u, np.ones_like(u), T_EVAL, S.MOB_ROLE, 0)
    assert np.isfinite(np.delete(d.ravel(), 3 * 120 + 4)).all()


TRAJ_DT = Q.TRAJ_DT  # checked here on the oracle before the GPU tests rely on them


@pytest.mark.parametrize("eq", ["ac", "ch"])
@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_trajectory_step_sizes_are_stable_on_the_oracle(eq, integrator):
    p = Q.problem(eq, ((64, 64), (1.0, 1.0)))
    u0 = Q.smooth_state((64, 64), 3)
    u = S.forward_trajectory(p, u0, TRAJ_DT[eq], 200, integrator)
    assert np.isfinite(u).all() and 0.02 < u.min() and u.max() < 0.98
    assert np.all(p.f(u) > 0)
    half = S.forward_trajectory(p, u0, TRAJ_DT[eq] / 2, 400, integrator)
    assert Q.rel(u, half) < 1e-3  # converged in dt, not merely bounded


@pytest.mark.parametrize("eq,shape", [("ac", "24x120"), ("ch", "67x40")])
def test_rk4_tangent_trajectory_against_central_differences(eq, shape):
    """20 RK4 steps with the ramped theta(t) (and flux(t)): every stage at its own time"""
    p = Q.problem(eq, shape)
    u0 = Q.smooth_state(p.psi.shape, 7)
    dt, n, t0 = TRAJ_DT[eq], 20, Q.TRAJ_T0
    params = [q for q in ALL_PARAMS if not (eq == "ch" and q == (S.MU_ROLE, 0))]
    _, dus = S.trajectory(p, u0, params, dt, n, "rk4", t0)
    # eps = 1e-4: the differences of end states round at 1e-16 |u| / (eps |du|) ~ 2e-8, the truncation is O(eps^2)
    eps = 1e-4
    for (role, k), du in zip(params, dus):
        ends = [S.forward_trajectory(p.with_closures(*S.perturbed(p.mu, p.mob, role, k, s * eps)), u0, dt, n, "rk4", t0)
                for s in (-1, 1)]
        assert Q.rel(du, (ends[1] - ends[0]) / (2 * eps)) <= 1e-6, (role, k)
    # the stage times matter: a trajectory that starts at another time has other tangents
    _, other = S.trajectory(p, u0, params, dt, n, "rk4", 0.0)
    assert Q.rel(other[0], dus[0]) > 1e-4


# ---- host logic ---------------------------------------------------------------------------------------------------------

SBM = {"ac": P.AllenCahn2DSmoothedBoundary, "ch": P.CahnHilliard2DSmoothedBoundary}


def _mu():
    return ChemLeg(np.array([0.1, -3.0]), lambda c: np.log(c / (1 - c)))


def _model(eq, solver, points=(24, 40)):
    return P.PDEModel(SBM[eq], sbm_domain(P, sbm_psi(*points)), solver)


def _other(eq, **over):
    o = {"kappa": 1.5, "f": SBM_F, "theta": SBM_THETA, ("R" if eq == "ac" else "D"): DiffLeg(np.array([0.8, 0.2]))}
    if eq == "ch":
        o["flux"] = SBM_FLUX
    o.update(over)
    return o


def _train(model, opt, other):
    data = {"ys": [np.full(model.domain.points, 0.5)] * 3, "ts": [0.0, 1e-6, 2e-6]}
    return model.train(data, [[0, 1, 2]], opt, other, {}, {}, 0.0)


@pytest.mark.parametrize("eq", ["ac", "ch"])
@pytest.mark.parametrize("solver", ["Euler", "RK4"])
def test_reject_unsupported_accepts_the_smoothed_boundary_classes(eq, solver):
    fit.reject_unsupported(_model(eq, getattr(P, solver)))


@pytest.mark.parametrize("eq", ["ac", "ch"])
def test_tsit5_and_imex_are_refused(eq):
    name = SBM[eq].__name__
    with pytest.raises(NotImplementedError, match=f"{name} support the Euler and RK4 solvers, not Tsit5"):
        fit.reject_unsupported(_model(eq, P.Tsit5))
    model = _model(eq, P.RK4)
    model.solver_type = P.SemiImplicitFourierSpectral  # (the model cannot be built with it: no fourier_symbol)
    with pytest.raises(NotImplementedError, match="Euler and RK4 solvers, not SemiImplicitFourierSpectral"):
        fit.reject_unsupported(model)

    class Imex:
        integrator = L.INT_IMEX

    eqn = SBM[eq](domain=sbm_domain(P, sbm_psi(24, 40)), mu=_mu(), **_other(eq))
    with pytest.raises(NotImplementedError, match=f"{name} sensitivities support Euler and RK4"):
        fit.sensitivity_solve(None, eqn, Imex(), np.full((1, 24, 40), 0.5), [0.0, 1e-6], [(L.SENS_MU, 1)])


@pytest.mark.parametrize("eq", ["ac", "ch"])
def test_a_3d_domain_is_refused(eq):
    model = _model(eq, P.Euler)
    model.domain = P.Domain((8, 8, 8), ((0, 1),) * 3, "dimensionless")
    with pytest.raises(NotImplementedError, match=f"{SBM[eq].__name__} on a 3-D domain"):
        fit.reject_unsupported(model)


@pytest.mark.parametrize("eq", ["ac", "ch"])
@pytest.mark.parametrize("key", ["f", "kappa", "theta", "flux"])
def test_fixed_data_is_not_trainable(eq, key):
    value = {"f": DiffLeg(np.array([0.1, 0.2])), "kappa": 1.5, "theta": SBM_THETA, "flux": SBM_FLUX}[key]
    with pytest.raises(fit.NotTrainableError, match=f"{key}.*other_parameters"):
        fit.ParamMap.of({"mu": _mu(), key: value}, SBM[eq])
    other = _other(eq)
    other.pop(key, None)
    with pytest.raises(fit.NotTrainableError, match=key):
        _train(_model(eq, P.RK4), {"mu": _mu(), key: value}, other)


def test_mu_constant_is_active_for_allen_cahn_and_inert_for_cahn_hilliard():
    ac = fit.ParamMap.of({"mu": _mu(), "R": DiffLeg(np.array([0.1]))}, SBM["ac"])
    assert ac.active().tolist() == [True, True, True]
    assert ac.sens_params() == [(L.SENS_MU, 0), (L.SENS_MU, 1), (L.SENS_MOB, 0)]
    ch = fit.ParamMap.of({"mu": _mu(), "D": DiffLeg(np.array([0.1]))}, SBM["ch"])
    assert ch.active().tolist() == [False, True, True]
    assert ch.sens_params() == [(L.SENS_MU, 1), (L.SENS_MOB, 0)]


@pytest.mark.parametrize("eq", ["ac", "ch"])
def test_jit_closures_and_modules_stay_refused(eq):
    tanh = lambda c: np.tanh(c)  # noqa: E731  (outside the in-kernel family: compiled at run time)
    with pytest.raises(UnsupportedClosureError):
        _train(_model(eq, P.RK4), {"mu": ChemLeg(np.array([0.0, -2.0]), tanh)}, _other(eq))
    with pytest.raises(UnsupportedClosureError):  # check_equation looks at f too
        _train(_model(eq, P.RK4), {"mu": _mu()}, _other(eq, f=lambda c: np.cosh(c) - 0.9))
    torch = pytest.importorskip("torch")
    with pytest.raises((NotImplementedError, ValueError)):
        _train(_model(eq, P.RK4), {"mu": torch.nn.Linear(1, 1)}, _other(eq))


def test_the_supported_text_is_only_appended_to():
    # the wording the earlier sensitivity tests match as substrings
    assert fit._SUPPORTED.startswith("CahnHilliard2DPeriodic on a 2-D domain or CahnHilliard3DPeriodic on a 3-D domain, or "
                                     "AllenCahn2DPeriodic or a Butler-Volmer Allen-Cahn class on a 2-D domain")
    assert "AllenCahn2DSmoothedBoundary or CahnHilliard2DSmoothedBoundary on a 2-D domain" in fit._SUPPORTED
    model = _model("ac", P.Euler)
    model.equation_type = dict
    with pytest.raises(NotImplementedError, match="CahnHilliard2DPeriodic on a 2-D domain or CahnHilliard3DPeriodic on a 3-D domain"):
        fit.reject_unsupported(model)
