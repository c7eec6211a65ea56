"""Allen-Cahn forward-mode sensitivities on the CPU: the numpy tangent-linear reference (tests/sens_ref_ac.py) against
central differences of the oracle, ParamMap's "R" role and equation-dependent inert rule, and the refusals of
PDEModel.train."""
import numpy as np
import pytest

import pde_opt_amd as P
from oracle import np_oracle as O
from pde_opt_amd import _lib as L
from pde_opt_amd import fit
from pde_opt_amd.numerics.closures import EXP_WRAP, LEGENDRE, LOGIT_PRIOR, MIX_ENTROPY, POLY, ClosureDesc
from pde_opt_amd.numerics.closures import UnsupportedClosureError
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg
import sens_ref_ac as S

N, H, KAPPA = 24, 1.0 / 24, 0.002


def _state(seed=0):
    rng = np.random.default_rng(seed)
    return np.clip(0.5 + 0.15 * rng.standard_normal((N, N)), 0.1, 0.9)


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# the closure classes of test_sens_cpu.py::test_tangent_rhs_matches_central_differences, with the second closure in the R
# role; mu's constant coefficient (deg0) moves the Allen-Cahn right-hand side
CASES = (
    [("legendre_mu_logit_deg%d" % d, ClosureDesc(LEGENDRE, LOGIT_PRIOR, tuple([0.1 * (i + 1) * (-1) ** i for i in range(d + 1)])),
      ClosureDesc(LEGENDRE, EXP_WRAP, (0.0,)), S.MU_ROLE, d) for d in range(6)]
    + [("mu_k0_of_3", ClosureDesc(LEGENDRE, LOGIT_PRIOR, (0.2, -3.0, 0.4)), ClosureDesc(LEGENDRE, EXP_WRAP, (-0.3, 0.2)), S.MU_ROLE, 0)]
    + [("exp_legendre_R_deg%d" % d, ClosureDesc(LEGENDRE, LOGIT_PRIOR, (0.0, -3.0)),
        ClosureDesc(LEGENDRE, EXP_WRAP, tuple([-0.5, 0.3, 0.2][: d + 1])), S.R_ROLE, d) for d in range(3)]
    + [("poly_mu", ClosureDesc(POLY, 0, (0.0, -1.0, 0.5, 1.0)), ClosureDesc(POLY, 0, (1.0, 0.2, 0.3)), S.MU_ROLE, 3),
       ("poly_mu_k0", ClosureDesc(POLY, 0, (0.1, -1.0, 0.5, 1.0)), ClosureDesc(POLY, 0, (1.0, 0.2, 0.3)), S.MU_ROLE, 0),
       ("poly_R", ClosureDesc(POLY, 0, (0.0, -1.0, 0.5, 1.0)), ClosureDesc(POLY, 0, (1.0, 0.2, 0.3)), S.R_ROLE, 2),
       ("mix_entropy", ClosureDesc(POLY, MIX_ENTROPY, (0.0, 2.0, -2.0)), ClosureDesc(POLY, 0, (1.0,)), S.MU_ROLE, 1)]
)


@pytest.mark.parametrize("name,mu,R,role,k", CASES, ids=[c[0] for c in CASES])
def test_tangent_rhs_matches_central_differences(name, mu, R, role, k):
    u = _state(1)
    du = 0.05 * np.random.default_rng(2).standard_normal(u.shape)
    got = S.tangent_rhs(u, du, H, H, KAPPA, mu, R, role, k)
    eps = 1e-5

    def f(e):
        m, r = S.perturbed(mu, R, role, k, e)
        return O.ac_rhs_fd(u + e * du, H, H, KAPPA, m, r)

    want = (f(eps) - f(-eps)) / (2 * eps)
    assert _rel(got, want) <= 1e-7


def test_reference_rhs_is_the_oracle():
    mu, R = ClosureDesc(LEGENDRE, LOGIT_PRIOR, (0.2, -3.0, 0.4)), ClosureDesc(LEGENDRE, EXP_WRAP, (-0.3, 0.2))
    u = _state(4)
    np.testing.assert_array_equal(S.ac_rhs(u, H, 2 * H, KAPPA, mu, R), O.ac_rhs_fd(u, H, 2 * H, KAPPA, mu, R))
    # the reference's RK4 step of the state alone is the oracle's (same tableau, to rounding of the accumulation order)
    f = lambda t, y: O.ac_rhs_fd(y, H, H, KAPPA, mu, R)
    got, _ = S.step(u, [], [], 1e-2, H, H, KAPPA, mu, R, "rk4")
    np.testing.assert_allclose(got, O.rk4_step(f, 0.0, u, 1e-2), rtol=0, atol=1e-14)
    got, _ = S.step(u, [], [], 1e-2, H, H, KAPPA, mu, R, "euler")
    np.testing.assert_array_equal(got, O.euler_step(f, 0.0, u, 1e-2))


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_tangent_steps_match_central_differences(integrator):
    mu = ClosureDesc(LEGENDRE, LOGIT_PRIOR, (0.2, -3.0, 0.2))
    R = ClosureDesc(LEGENDRE, EXP_WRAP, (-0.3, 0.1))
    params = [(S.MU_ROLE, 0), (S.MU_ROLE, 1), (S.MU_ROLE, 2), (S.R_ROLE, 0), (S.R_ROLE, 1)]
    dt, n = 1e-2, 20
    u0 = _state(3)
    _, dus = S.trajectory(u0, params, dt, n, H, H, KAPPA, mu, R, integrator)
    for (role, k), du in zip(params, dus):
        eps = 1e-5

        def end(e):
            m, r = S.perturbed(mu, R, role, k, e)
            u, _ = S.trajectory(u0, [], dt, n, H, H, KAPPA, m, r, integrator)
            return u

        want = (end(eps) - end(-eps)) / (2 * eps)
        assert np.linalg.norm(du) > 0
        assert _rel(du, want) <= 1e-7, (role, k)


# ---- ParamMap -------------------------------------------------------------------------------------------------------


def _mu():
    return ChemLeg(np.array([0.1, -2.0]), lambda c: np.log(c / (1 - c)))


def test_param_map_accepts_R_role():
    opt = {"mu": _mu(), "R": DiffLeg(np.array([0.1, 0.2]))}
    pm = fit.ParamMap.of(opt, P.AllenCahn2DPeriodic)
    assert pm.all_params() == [(L.SENS_MU, 0), (L.SENS_MU, 1), (L.SENS_MOB, 0), (L.SENS_MOB, 1)]
    back = pm.build(pm.flatten(opt))
    assert set(back) == {"mu", "R"} and isinstance(back["R"], DiffLeg) and isinstance(back["mu"], ChemLeg)
    np.testing.assert_array_equal(back["R"].expansion.params, [0.1, 0.2])
    assert back["mu"].prior_fn is opt["mu"].prior_fn


def test_mu_constant_is_active_for_allen_cahn_and_inert_for_cahn_hilliard():
    ac = fit.ParamMap.of({"mu": _mu(), "R": DiffLeg(np.array([0.1]))}, P.AllenCahn2DPeriodic)
    assert ac.active().tolist() == [True, True, True]
    assert ac.sens_params() == [(L.SENS_MU, 0), (L.SENS_MU, 1), (L.SENS_MOB, 0)]
    r, G = ac.expand(np.array([1.0, 2.0, 3.0]), np.arange(9.0).reshape(3, 3))
    np.testing.assert_array_equal(r, [1.0, 2.0, 3.0])
    np.testing.assert_array_equal(G, np.arange(9.0).reshape(3, 3))
    opt = {"mu": _mu(), "D": DiffLeg(np.array([0.1]))}
    for ch in (fit.ParamMap.of(opt), fit.ParamMap.of(opt, P.CahnHilliard2DPeriodic), fit.ParamMap.of(opt, P.CahnHilliard3DPeriodic)):
        assert ch.active().tolist() == [False, True, True]
        assert ch.sens_params() == [(L.SENS_MU, 1), (L.SENS_MOB, 0)]


# ---- refusals (before any device work) -----------------------------------------------------------------------------


def _model(equation, solver):
    return P.PDEModel(equation, P.Domain((64, 64), ((0, 1), (0, 1)), "dimensionless"), solver)


def _train(model, opt, other):
    data = {"ys": [np.full((64, 64), 0.5)] * 3, "ts": [0.0, 1e-6, 2e-6]}
    return model.train(data, [[0, 1, 2]], opt, other, {"A": 0.5} if model.solver_type is P.SemiImplicitFourierSpectral
                       else {}, {}, 0.0)


@pytest.mark.parametrize("solver", ["Euler", "RK4"])
def test_reject_unsupported_accepts_allen_cahn(solver):
    fit.reject_unsupported(_model(P.AllenCahn2DPeriodic, getattr(P, solver)))


def test_allen_cahn_rejects_tsit5():
    with pytest.raises(NotImplementedError, match="Euler and RK4"):
        _train(_model(P.AllenCahn2DPeriodic, P.Tsit5), {"mu": _mu()}, {"R": DiffLeg(np.array([0.0])), "kappa": KAPPA})


def test_allen_cahn_rejects_imex_at_the_solve():
    # the model itself cannot be built (Allen-Cahn publishes no fourier_symbol); the solve refuses the integrator too
    eq = P.AllenCahn2DPeriodic(P.Domain((64, 64), ((0, 1), (0, 1)), "dimensionless"), KAPPA, _mu(), DiffLeg(np.array([0.0])))

    class Imex:
        integrator = L.INT_IMEX

    with pytest.raises(NotImplementedError, match="Euler and RK4"):
        fit.sensitivity_solve(None, eq, Imex(), np.full((1, 64, 64), 0.5), [0.0, 1e-6], [(L.SENS_MU, 0)])


def test_allen_cahn_rejects_fourier_derivatives():
    with pytest.raises(NotImplementedError, match="fd"):
        _train(_model(P.AllenCahn2DPeriodic, P.Euler), {"mu": _mu()},
               {"R": DiffLeg(np.array([0.0])), "kappa": KAPPA, "derivs": "fourier"})


def test_allen_cahn_rejects_jit_closures():
    mu = ChemLeg(np.array([0.0, -2.0]), lambda c: np.tanh(c))  # a prior outside the family: compiled at run time
    with pytest.raises(UnsupportedClosureError):
        _train(_model(P.AllenCahn2DPeriodic, P.RK4), {"mu": mu}, {"R": DiffLeg(np.array([0.0])), "kappa": KAPPA})


def test_allen_cahn_rejects_kappa_and_3d_domain():
    with pytest.raises(ValueError, match="kappa"):
        _train(_model(P.AllenCahn2DPeriodic, P.Euler), {"mu": _mu(), "kappa": KAPPA}, {"R": DiffLeg(np.array([0.0]))})
    model = _model(P.AllenCahn2DPeriodic, P.Euler)
    model.domain = P.Domain((8, 8, 8), ((0, 1),) * 3, "dimensionless")
    with pytest.raises(NotImplementedError, match="AllenCahn2DPeriodic on a 3-D domain"):
        fit.reject_unsupported(model)


@pytest.mark.parametrize("solver", ["RK4", "Tsit5"])
def test_cahn_hilliard_still_rejects_rk4_and_tsit5(solver):
    with pytest.raises(NotImplementedError, match="SemiImplicitFourierSpectral"):
        _train(_model(P.CahnHilliard2DPeriodic, getattr(P, solver)), {"mu": _mu()}, {"D": DiffLeg(np.array([0.0])), "kappa": KAPPA})


def test_cahn_hilliard_refusals_unchanged():
    with pytest.raises(ValueError, match="kappa"):
        _train(_model(P.CahnHilliard2DPeriodic, P.SemiImplicitFourierSpectral), {"mu": _mu(), "kappa": KAPPA},
               {"D": DiffLeg(np.array([0.0]))})
    model = _model(P.CahnHilliard2DPeriodic, P.Euler)
    model.equation_type = dict  # any type outside the supported set
    with pytest.raises(NotImplementedError, match="CahnHilliard2DPeriodic on a 2-D domain or CahnHilliard3DPeriodic on a 3-D domain"):
        fit.reject_unsupported(model)
    with pytest.raises(NotImplementedError):
        _model(P.AllenCahn2DPeriodic, P.Euler).optimize()
