"""Forward-mode sensitivities and the fitting drivers on the CPU: the numpy tangent-linear reference against central
differences of the oracle, the Levenberg-Marquardt / BFGS drivers on a fake sensitivity provider, PDEModel.train's
data stacking and its refusals."""
import numpy as np
import pytest

import pde_opt_amd as P
from oracle import np_oracle as O
from pde_opt_amd import fit
from pde_opt_amd.numerics.closures import EXP_WRAP, LEGENDRE, LOGIT_PRIOR, MIX_ENTROPY, POLY, ClosureDesc
from pde_opt_amd.numerics.closures import UnsupportedClosureError
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg
from pde_opt_amd.pde_model import stack_training_data
import sens_ref as S

N, H, KAPPA = 24, 1.0 / 24, 0.002


def _state(seed=0):
    rng = np.random.default_rng(seed)
    return np.clip(0.5 + 0.15 * rng.standard_normal((N, N)), 0.1, 0.9)


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


CASES = (
    [("legendre_mu_logit_deg%d" % d, ClosureDesc(LEGENDRE, LOGIT_PRIOR, tuple([0.1 * (i + 1) * (-1) ** i for i in range(d + 1)])),
      ClosureDesc(LEGENDRE, EXP_WRAP, (0.0,)), S.MU_ROLE, d) for d in range(6)]
    + [("exp_legendre_D_deg%d" % d, ClosureDesc(LEGENDRE, LOGIT_PRIOR, (0.0, -3.0)),
        ClosureDesc(LEGENDRE, EXP_WRAP, tuple([-0.5, 0.3, 0.2][: d + 1])), S.MOB_ROLE, d) for d in range(3)]
    + [("poly_mu", ClosureDesc(POLY, 0, (0.0, -1.0, 0.5, 1.0)), ClosureDesc(POLY, 0, (1.0, 0.2, 0.3)), S.MU_ROLE, 3),
       ("poly_D", ClosureDesc(POLY, 0, (0.0, -1.0, 0.5, 1.0)), ClosureDesc(POLY, 0, (1.0, 0.2, 0.3)), S.MOB_ROLE, 2),
       ("mix_entropy", ClosureDesc(POLY, MIX_ENTROPY, (0.0, 2.0, -2.0)), ClosureDesc(POLY, 0, (1.0,)), S.MU_ROLE, 1)]
)


@pytest.mark.parametrize("name,mu,mob,role,k", CASES, ids=[c[0] for c in CASES])
def test_tangent_rhs_matches_central_differences(name, mu, mob, role, k):
    u = _state(1)
    du = 0.05 * np.random.default_rng(2).standard_normal(u.shape)
    got = S.tangent_rhs(u, du, H, H, KAPPA, mu, mob, role, k)
    eps = 1e-5

    def f(e):
        m, d = S.perturbed(mu, mob, role, k, e)
        return O.ch_rhs_fd(u + e * du, H, H, KAPPA, m, d)

    want = (f(eps) - f(-eps)) / (2 * eps)
    assert _rel(got, want) <= 1e-7


@pytest.mark.parametrize("shape", [(40, 72), (17, 33), (6, 10), (96, 80)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("closures", ["legendre16", "mix_entropy_exp_poly", "poly"])
def test_tangent_rhs_reference_on_ragged_anisotropic_grids(closures, shape):
    """the reference at the closure sets and grids the GPU kernels are held to in tests/test_gpu_sens_shapes.py:
    hx != hy, Legendre coefficients up to index 15, POLY under EXP_WRAP and with MIX_ENTROPY"""
    from test_gpu_sens_shapes import CLOSURES

    mu, mob, params = CLOSURES[closures]
    hx, hy = 1 / 64, 1 / 128
    rng = np.random.default_rng(5)
    u = np.clip(0.5 + 0.1 * rng.standard_normal(shape), 0.1, 0.9)
    du = 0.05 * rng.standard_normal(shape)
    eps = 1e-6
    for role, k in params:
        def f(e):
            m, d = S.perturbed(mu, mob, role, k, e)
            return O.ch_rhs_fd(u + e * du, hx, hy, KAPPA, m, d)

        want = (f(eps) - f(-eps)) / (2 * eps)
        assert _rel(S.tangent_rhs(u, du, hx, hy, KAPPA, mu, mob, role, k), want) <= 1e-8, (role, k)


@pytest.mark.parametrize("integrator", ["imex", "euler"])
def test_tangent_steps_match_central_differences(integrator):
    mu = ClosureDesc(LEGENDRE, LOGIT_PRIOR, (0.0, -3.0, 0.2))
    mob = ClosureDesc(LEGENDRE, EXP_WRAP, (-0.3, 0.1))
    params = [(S.MU_ROLE, 1), (S.MU_ROLE, 2), (S.MOB_ROLE, 0), (S.MOB_ROLE, 1)]
    symbol = O.ch_fourier_symbol(N, N, H, H, KAPPA)
    dt, n = (1e-4, 20) if integrator == "imex" else (2e-7, 20)
    u0 = _state(3)
    _, dus = S.trajectory(u0, params, dt, n, H, H, KAPPA, mu, mob, integrator, 0.5, symbol)
    for (role, k), du in zip(params, dus):
        eps = 1e-5

        def end(e):
            m, d = S.perturbed(mu, mob, role, k, e)
            u, _ = S.trajectory(u0, [], dt, n, H, H, KAPPA, m, d, integrator, 0.5, symbol)
            return u

        want = (end(eps) - end(-eps)) / (2 * eps)
        assert _rel(du, want) <= 1e-7


def test_closure_derivatives_of_legendre_recurrence():
    # the kernel's P'_{n+1} = P'_{n-1} + (2n + 1) P_n, against numpy's legder
    c = np.linspace(0.05, 0.95, 37)
    a = np.array([0.3, -1.0, 0.5, 0.25, -0.7, 0.1])
    x = 2 * c - 1
    pm, pc, dpm, dpc, d = np.ones_like(x), x, 0 * x, 1 + 0 * x, a[1] + 0 * x
    for k in range(1, len(a) - 1):
        pn = ((2 * k + 1) * x * pc - k * pm) / (k + 1)
        dpn = dpm + (2 * k + 1) * pc
        d = d + a[k + 1] * dpn
        pm, pc, dpm, dpc = pc, pn, dpc, dpn
    np.testing.assert_allclose(2 * d, S.closure_dc(ClosureDesc(LEGENDRE, 0, tuple(a)), c), rtol=1e-13, atol=1e-13)


# ---- optimisers on a fake sensitivity provider -----------------------------------------------------------------------


def _linear_objective(A, v, lam=0.0, w=None):
    """pred(p) = A p: dpred = A, r = v - A p"""
    def sums(p):
        r = v - A @ p
        return float(r @ r), A.T @ r, A.T @ A

    return fit.Objective(sums=sums, ssr=lambda p: sums(p)[0], M=len(v), lambda_reg=lam, w=w)


def test_levenberg_marquardt_linear_problem_converges_to_lstsq():
    rng = np.random.default_rng(0)
    A, v = rng.standard_normal((40, 5)), rng.standard_normal(40)
    p, hist = fit.levenberg_marquardt(_linear_objective(A, v), np.zeros(5))
    np.testing.assert_allclose(p, np.linalg.lstsq(A, v, rcond=None)[0], rtol=1e-7, atol=1e-9)
    assert hist[-1] <= hist[0]


def test_bfgs_linear_problem_converges_to_lstsq():
    rng = np.random.default_rng(1)
    A, v = rng.standard_normal((40, 4)), rng.standard_normal(40)
    p, _ = fit.bfgs(_linear_objective(A, v), np.zeros(4))
    np.testing.assert_allclose(p, np.linalg.lstsq(A, v, rcond=None)[0], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("method", [fit.levenberg_marquardt, fit.bfgs])
def test_zero_column_leaves_its_parameter_unchanged(method):
    rng = np.random.default_rng(2)
    A, v = rng.standard_normal((30, 3)), rng.standard_normal(30)
    A[:, 0] = 0.0  # mu's constant coefficient: grad of a constant is 0
    p, _ = method(_linear_objective(A, v), np.array([0.7, 0.0, 0.0]))
    assert p[0] == 0.7
    np.testing.assert_allclose(p[1:], np.linalg.lstsq(A[:, 1:], v, rcond=None)[0], rtol=1e-5, atol=1e-6)


def test_levenberg_marquardt_with_regularization_matches_normal_equations():
    # objective 1/2 (|v - A p|^2 + (lam sum w p^2)^2): check the gradient vanishes at the result
    rng = np.random.default_rng(3)
    A, v = rng.standard_normal((30, 3)), rng.standard_normal(30)
    lam, w = 0.1, np.array([1.0, 2.0, 0.5])
    p, _ = fit.levenberg_marquardt(_linear_objective(A, v, lam, w), np.zeros(3))
    reg = lam * np.sum(w * p * p)
    grad = -A.T @ (v - A @ p) + reg * 2 * lam * w * p
    assert np.max(np.abs(grad)) < 1e-7


def test_regularization_is_the_reference_formula():
    params = {"mu": ChemLeg(np.array([0.5, -2.0, 1.0]), lambda c: np.log(c / (1 - c))), "D": DiffLeg(np.array([0.3])),
              "kappa": 0.002}
    weights = {"mu": ChemLeg(np.array([1.0, 2.0, 3.0])), "D": DiffLeg(np.array([4.0])), "kappa": None}
    want = 7.0 * (1.0 * 0.25 + 2.0 * 4.0 + 3.0 * 1.0 + 4.0 * 0.09)
    assert abs(fit.regularization(params, weights, 7.0) - want) < 1e-12
    model = P.PDEModel(P.CahnHilliard2DPeriodic, P.Domain((8, 8), ((0, 1), (0, 1)), "dimensionless"),
                       P.SemiImplicitFourierSpectral)
    assert abs(model.regularization(params, weights, 7.0) - want) < 1e-12


def test_param_map_round_trip_keeps_class_and_prior():
    prior = lambda c: np.log(c / (1 - c)) + 3 * (1 - 2 * c)  # a polynomial part folded into the series
    opt = {"mu": ChemLeg(np.array([0.0, -2.0]), prior), "D": DiffLeg(np.array([0.1]))}
    pm = fit.ParamMap.of(opt)
    assert pm.all_params() == [(0, 0), (0, 1), (1, 0)]
    assert pm.sens_params() == [(0, 1), (1, 0)]  # mu's constant coefficient never moves the solution
    r, G = pm.expand(np.array([1.0, 2.0]), np.array([[3.0, 4.0], [4.0, 5.0]]))
    np.testing.assert_array_equal(r, [0.0, 1.0, 2.0])
    np.testing.assert_array_equal(G, [[0, 0, 0], [0, 3, 4], [0, 4, 5]])
    back = pm.build(pm.flatten(opt))
    assert isinstance(back["mu"], ChemLeg) and back["mu"].prior_fn is prior and isinstance(back["D"], DiffLeg)
    np.testing.assert_array_equal(back["mu"].expansion.params, [0.0, -2.0])
    # the kernel coefficients carry the folded prior on top of the trainable ones
    desc = back["mu"].closure_desc()
    assert desc.flags == LOGIT_PRIOR and desc.coef[1] == -2.0 + (-3.0)


def test_walk_save_points_follows_diffeqsolve():
    from fake_engine import OracleEngine
    from util import MOB, MU

    dom = P.Domain((16, 16), ((0, 1), (0, 1)), "dimensionless")
    eq = P.CahnHilliard2DPeriodic(dom, 0.002, MU["regsol"], MOB["one"])
    ts = [0.0, 0.4e-4, 1e-4, 2.5e-4, 2.7e-4, 3.3e-4]
    eng = OracleEngine()
    P.diffeqsolve(eq, P.Euler(), ts[0], ts[-1], 1e-4, _state()[:16, :16], saveat=P.SaveAt(ts=ts), engine=eng)
    want = [(c[2], c[3], c[4]) for c in eng.calls if c[0] == "advance"]
    got, thetas = [], []
    fit.walk_save_points(ts[0], ts[-1], 1e-4, ts, lambda dt, n, t: got.append((dt, n, t)), lambda: None,
                         lambda q, th: thetas.append(th))
    assert got == want
    assert thetas[0] is None and thetas[2] is None and len(thetas) == len(ts)
    assert abs(thetas[1] - 0.4) < 1e-12


def test_stack_training_data_from_inds():
    ys = [np.full((4, 4), float(i)) for i in range(100)]
    ts = np.linspace(0.0, 0.02, 100)
    y0s, values, rel = stack_training_data({"ys": ys, "ts": ts}, [[30, 40, 50], [50, 60, 70], [70, 80, 90]])
    assert y0s.shape == (3, 4, 4) and values.shape == (3, 2, 4, 4)
    assert [y[0, 0] for y in y0s] == [30.0, 50.0, 70.0]
    assert values[1, :, 0, 0].tolist() == [60.0, 70.0]
    np.testing.assert_allclose(rel, [0.0, ts[40] - ts[30], ts[50] - ts[30]], rtol=0, atol=0)


# ---- refusals (before any device work) -----------------------------------------------------------------------------


def _train(model, opt, other):
    data = {"ys": [np.full((64, 64), 0.5)] * 3, "ts": [0.0, 1e-6, 2e-6]}
    return model.train(data, [[0, 1, 2]], opt, other, {"A": 0.5} if model.solver_type is P.SemiImplicitFourierSpectral
                       else {}, {}, 0.0)


def _model(solver=None):
    return P.PDEModel(P.CahnHilliard2DPeriodic, P.Domain((64, 64), ((0, 1), (0, 1)), "dimensionless"),
                      solver or P.SemiImplicitFourierSpectral)


def _mu():
    return ChemLeg(np.array([0.0, -2.0]), lambda c: np.log(c / (1 - c)))


def test_train_rejects_kappa():
    with pytest.raises(ValueError, match="kappa"):
        _train(_model(), {"mu": _mu(), "kappa": 0.002}, {"D": DiffLeg(np.array([0.0]))})


def test_train_rejects_fourier_derivatives():
    with pytest.raises(NotImplementedError, match="fd"):
        _train(_model(), {"mu": _mu()}, {"D": DiffLeg(np.array([0.0])), "kappa": 0.002, "derivs": "fourier"})


@pytest.mark.parametrize("solver", ["RK4", "Tsit5"])
def test_train_rejects_other_solvers(solver):
    with pytest.raises(NotImplementedError, match="SemiImplicitFourierSpectral"):
        _train(_model(getattr(P, solver)), {"mu": _mu()}, {"D": DiffLeg(np.array([0.0])), "kappa": 0.002})


def test_train_rejects_strang():
    # StrangSplitting needs A_term, which Cahn-Hilliard lacks: the model refuses it at construction, as upstream
    with pytest.raises(ValueError):
        _model(P.StrangSplitting)
    model = _model()
    model.solver_type = P.StrangSplitting
    with pytest.raises(NotImplementedError, match="SemiImplicitFourierSpectral"):
        _train(model, {"mu": _mu()}, {"D": DiffLeg(np.array([0.0])), "kappa": 0.002})


def test_train_rejects_3d():
    model = _model()
    model.equation_type = P.CahnHilliard3DPeriodic
    with pytest.raises(NotImplementedError, match="CahnHilliard2DPeriodic"):
        _train(model, {"mu": _mu()}, {"D": DiffLeg(np.array([0.0])), "kappa": 0.002})


def test_train_rejects_jit_closures():
    mu = ChemLeg(np.array([0.0, -2.0]), lambda c: np.tanh(c))  # a prior outside the family: compiled at run time
    with pytest.raises(UnsupportedClosureError):
        _train(_model(), {"mu": mu}, {"D": DiffLeg(np.array([0.0])), "kappa": 0.002})


def test_optimize_still_unsupported():
    with pytest.raises(NotImplementedError):
        _model().optimize()


def test_accumulation_kernel_uses_no_atomics():
    """Guideline 12: the Gauss-Newton sums are a fixed-order slab reduction, so their ISA holds no atomic at all"""
    import os
    import re
    import subprocess

    from pde_opt_amd.csrc import build as B

    src = os.path.join(B.HERE, "sens.hip")
    isa = subprocess.run([B._hipcc(), *B.CXXFLAGS, "-I" + os.path.join(B.ROOT, "include"), "--cuda-device-only", "-S",
                          "-o", "-", src], capture_output=True, text=True, check=True).stdout
    bodies = re.findall(r"^(_Z\w*sens_gn\w*):.*?\n(.*?)s_endpgm", isa, flags=re.S | re.M)
    assert len(bodies) == 3  # the fp32 / fp64 partial-slab kernels and the final in-order sum
    for name, body in bodies:
        assert "atomic" not in body, name
