"""3-D forward-mode sensitivities on the CPU: the numpy tangent-linear reference (tests/sens_ref3d.py) against central
differences of the oracle's ch3d_rhs_fd and of short IMEX / Euler trajectories, and what PDEModel.train accepts and
refuses for CahnHilliard3DPeriodic.  The grid is not cubic and its spacings differ, so that an axis mix-up shows."""
import numpy as np
import pytest

import pde_opt_amd as P
from oracle import np_oracle as O
from pde_opt_amd import fit
from pde_opt_amd.numerics.closures import EXP_WRAP, LEGENDRE, LOGIT_PRIOR, MIX_ENTROPY, POLY, ClosureDesc
from pde_opt_amd.numerics.closures import UnsupportedClosureError
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg
import sens_ref3d as S3

SHAPE = (8, 10, 12)
BOX = ((0.0, 0.8), (0.0, 1.5), (0.0, 0.9))  # hx = 0.1, hy = 0.15, hz = 0.075
KAPPA = 0.002


def _dom(shape=SHAPE, box=BOX):
    return P.Domain(shape, box, "dimensionless")


H = _dom().dx


def _state(seed=0):
    rng = np.random.default_rng(seed)
    return np.clip(0.5 + 0.15 * rng.standard_normal(SHAPE), 0.1, 0.9)


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_grid_is_not_cubic():
    assert len(set(SHAPE)) == 3 and len(set(H)) == 3


CASES = (
    [("legendre_mu_logit_deg%d" % d, ClosureDesc(LEGENDRE, LOGIT_PRIOR, tuple([0.1 * (i + 1) * (-1) ** i for i in range(d + 1)])),
      ClosureDesc(LEGENDRE, EXP_WRAP, (0.0,)), S3.MU_ROLE, d) for d in range(6)]
    + [("exp_legendre_D_deg%d" % d, ClosureDesc(LEGENDRE, LOGIT_PRIOR, (0.0, -3.0)),
        ClosureDesc(LEGENDRE, EXP_WRAP, tuple([-0.5, 0.3, 0.2][: d + 1])), S3.MOB_ROLE, d) for d in range(3)]
    + [("poly_mu", ClosureDesc(POLY, 0, (0.0, -1.0, 0.5, 1.0)), ClosureDesc(POLY, 0, (1.0, 0.2, 0.3)), S3.MU_ROLE, 3),
       ("poly_D", ClosureDesc(POLY, 0, (0.0, -1.0, 0.5, 1.0)), ClosureDesc(POLY, 0, (1.0, 0.2, 0.3)), S3.MOB_ROLE, 2),
       ("mix_entropy", ClosureDesc(POLY, MIX_ENTROPY, (0.0, 2.0, -2.0)), ClosureDesc(POLY, 0, (1.0,)), S3.MU_ROLE, 1),
       ("mix_entropy_exp_D", ClosureDesc(POLY, MIX_ENTROPY, (0.0, 2.0, -2.0)), ClosureDesc(POLY, EXP_WRAP, (-0.2, 0.4)),
        S3.MOB_ROLE, 1)]
)


@pytest.mark.parametrize("name,mu,mob,role,k", CASES, ids=[c[0] for c in CASES])
def test_tangent_rhs_matches_central_differences(name, mu, mob, role, k):
    u = _state(1)
    du = 0.05 * np.random.default_rng(2).standard_normal(u.shape)
    got = S3.tangent_rhs(u, du, H, KAPPA, mu, mob, role, k)
    eps = 1e-5

    def f(e):
        m, d = S3.perturbed(mu, mob, role, k, e)
        return O.ch3d_rhs_fd(u + e * du, H[0], H[1], H[2], KAPPA, m, d)

    want = (f(eps) - f(-eps)) / (2 * eps)
    assert _rel(got, want) <= 1e-7


def test_base_rhs_is_the_oracle():
    mu, mob = ClosureDesc(LEGENDRE, LOGIT_PRIOR, (0.0, -3.0)), ClosureDesc(LEGENDRE, EXP_WRAP, (-0.3,))
    u = _state(4)
    np.testing.assert_array_equal(S3.ch_rhs(u, H, KAPPA, mu, mob), O.ch3d_rhs_fd(u, *H, KAPPA, mu, mob))


@pytest.mark.parametrize("integrator", ["imex", "euler"])
def test_tangent_steps_match_central_differences(integrator):
    mu = ClosureDesc(LEGENDRE, LOGIT_PRIOR, (0.0, -3.0, 0.2))
    mob = ClosureDesc(LEGENDRE, EXP_WRAP, (-0.3, 0.1))
    params = [(S3.MU_ROLE, 1), (S3.MU_ROLE, 2), (S3.MOB_ROLE, 0), (S3.MOB_ROLE, 1)]
    symbol = P.CahnHilliard3DPeriodic(_dom(), KAPPA, mu, mob).fourier_symbol
    dt, n = (1e-3, 20) if integrator == "imex" else (1e-5, 20)
    u0 = _state(3)
    _, dus = S3.trajectory(u0, params, dt, n, H, KAPPA, mu, mob, integrator, 0.5, symbol)
    for (role, k), du in zip(params, dus):
        eps = 1e-5

        def end(e):
            m, d = S3.perturbed(mu, mob, role, k, e)
            u, _ = S3.trajectory(u0, [], dt, n, H, KAPPA, m, d, integrator, 0.5, symbol)
            return u

        want = (end(eps) - end(-eps)) / (2 * eps)
        assert np.linalg.norm(want) > 0
        assert _rel(du, want) <= 1e-7


# ---- what train accepts and refuses in 3-D (before any device work) ---------------------------------------------------


def _model(solver=None, equation=None, shape=(8, 8, 8)):
    box = tuple((0.0, 1.0) for _ in shape)
    return P.PDEModel(equation or P.CahnHilliard3DPeriodic, P.Domain(shape, box, "dimensionless"),
                      solver or P.SemiImplicitFourierSpectral)


def _mu():
    return ChemLeg(np.array([0.0, -2.0]), lambda c: np.log(c / (1 - c)))


def _train(model, opt, other):
    data = {"ys": [np.full(model.domain.points, 0.5)] * 3, "ts": [0.0, 1e-6, 2e-6]}
    return model.train(data, [[0, 1, 2]], opt, other, {"A": 0.5} if model.solver_type is P.SemiImplicitFourierSpectral
                       else {}, {}, 0.0)


@pytest.mark.parametrize("solver", ["SemiImplicitFourierSpectral", "Euler"])
def test_reject_unsupported_accepts_3d(solver):
    fit.reject_unsupported(_model(getattr(P, solver)))


def test_reject_unsupported_refuses_dimension_mismatch():
    with pytest.raises(NotImplementedError, match="CahnHilliard3DPeriodic on a 3-D domain"):
        fit.reject_unsupported(_model(equation=P.CahnHilliard2DPeriodic))
    with pytest.raises(NotImplementedError, match="CahnHilliard2DPeriodic on a 2-D domain"):
        fit.reject_unsupported(_model(shape=(16, 16)))


@pytest.mark.parametrize("solver", ["RK4", "Tsit5"])
def test_train_3d_rejects_other_solvers(solver):
    with pytest.raises(NotImplementedError, match="SemiImplicitFourierSpectral"):
        _train(_model(getattr(P, solver)), {"mu": _mu()}, {"D": DiffLeg(np.array([0.0])), "kappa": KAPPA})


def test_train_3d_rejects_fourier_derivatives():
    with pytest.raises(NotImplementedError, match="fd"):
        _train(_model(), {"mu": _mu()}, {"D": DiffLeg(np.array([0.0])), "kappa": KAPPA, "derivs": "fourier"})


def test_train_3d_rejects_kappa():
    with pytest.raises(ValueError, match="kappa"):
        _train(_model(), {"mu": _mu(), "kappa": KAPPA}, {"D": DiffLeg(np.array([0.0]))})


def test_train_3d_rejects_jit_closures():
    mu = ChemLeg(np.array([0.0, -2.0]), lambda c: np.tanh(c))  # a prior outside the family: compiled at run time
    with pytest.raises(UnsupportedClosureError):
        _train(_model(), {"mu": mu}, {"D": DiffLeg(np.array([0.0])), "kappa": KAPPA})
