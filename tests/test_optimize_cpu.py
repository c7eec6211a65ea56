"""PDEModel.optimize on the CPU: the generic BFGS entry, the torch adapter, the gradient assembly with the numpy
tangent references in the engine's place (tests/optimize_ref.py), the refusals, and train(method="mse") unchanged by the
BFGS both share."""
import numpy as np
import pytest
import torch

import pde_opt_amd as P
from pde_opt_amd import fit
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg
import ac_fit_problem as F
import optimize_ref as R
import sens_ref as S
import sens_ref_ac as SA


# ---- the generic BFGS entry -----------------------------------------------------------------------------------------------


def _within_tolerances(p, want):
    return np.all(np.abs(p - want) <= 10 * (fit.ATOL + fit.RTOL * np.abs(want)))


def test_minimize_bfgs_convex_quadratic():
    A = np.array([[3.0, 0.5, 0.0], [0.5, 2.0, 0.3], [0.0, 0.3, 1.0]])
    b = np.array([1.0, -2.0, 0.5])
    f = lambda p: 0.5 * p @ A @ p - b @ p
    p, hist = fit.minimize_bfgs(lambda p: (f(p), A @ p - b), f, np.zeros(3))
    want = np.linalg.solve(A, b)
    # the iteration stops when a step is within ATOL + RTOL |p|; the superlinear tail leaves the iterate well inside 10 x
    assert _within_tolerances(p, want), (p, want)
    assert abs(hist[-1] - f(want)) <= fit.ATOL + fit.RTOL * abs(f(want))
    assert all(b <= a for a, b in zip(hist, hist[1:]))


def test_minimize_bfgs_rosenbrock():
    f = lambda p: (1 - p[0]) ** 2 + 100 * (p[1] - p[0] ** 2) ** 2
    g = lambda p: np.array([-2 * (1 - p[0]) - 400 * p[0] * (p[1] - p[0] ** 2), 200 * (p[1] - p[0] ** 2)])
    p, hist = fit.minimize_bfgs(lambda p: (f(p), g(p)), f, np.array([-1.2, 1.0]), max_steps=200)
    assert _within_tolerances(p, np.ones(2)), p
    assert hist[-1] <= fit.ATOL


def test_minimize_bfgs_never_moves_a_direction_without_gradient():
    f = lambda p: (p[0] - 1) ** 2 + 3 * (p[2] + 2) ** 2
    p, _ = fit.minimize_bfgs(lambda p: (f(p), np.array([2 * (p[0] - 1), 0.0, 6 * (p[2] + 2)])), f, np.array([0.0, 0.7, 0.0]))
    assert p[1] == 0.7 and _within_tolerances(p[[0, 2]], np.array([1.0, -2.0]))


def test_minimize_bfgs_backs_off_non_finite_trial_points():
    f = lambda p: float(p[0] - np.log(p[0])) if p[0] > 0 else float("nan")
    p, _ = fit.minimize_bfgs(lambda p: (f(p), np.array([1 - 1 / p[0]])), f, np.array([0.05]))
    assert _within_tolerances(p, np.ones(1))


# ---- the torch adapter ------------------------------------------------------------------------------------------------------


def test_torch_adapter_matches_hand_written_gradient():
    rng = np.random.default_rng(0)
    ys, target = rng.standard_normal((4, 6, 5)), rng.standard_normal((6, 5))
    tt = torch.tensor(target)
    obj = fit.as_objective(lambda y: torch.mean((y[-1] - tt) ** 2) + 0.1 * torch.mean(y[2] ** 2), ys)
    J, g = obj.value_and_grad(ys)
    want_g = np.zeros_like(ys)
    want_g[-1] = 2 * (ys[-1] - target) / 30
    want_g[2] = 0.2 * ys[2] / 30
    want_J = np.mean((ys[-1] - target) ** 2) + 0.1 * np.mean(ys[2] ** 2)
    assert isinstance(J, float) and g.dtype == np.float64 and g.shape == ys.shape
    assert abs(J - want_J) <= 4 * np.finfo(float).eps * abs(want_J)
    np.testing.assert_allclose(g, want_g, rtol=4 * np.finfo(float).eps, atol=0)
    assert abs(obj.value(ys) - want_J) <= 4 * np.finfo(float).eps * abs(want_J)
    # a float32 solution reaches the objective in float64
    assert fit.as_objective(lambda y: torch.sum(y) * (1.0 if y.dtype == torch.float64 else float("nan"))).value(ys.astype(np.float32)) == \
        pytest.approx(float(np.sum(ys.astype(np.float32).astype(np.float64))))


class _Recorder:
    def __init__(self, out):
        self.out, self.seen = out, None

    def __call__(self, cot):
        self.seen = cot
        return self.out


def test_frame_zero_cotangent_is_dropped_and_inert_entries_get_zero():
    rng = np.random.default_rng(1)
    ys = rng.standard_normal((4, 6, 5))
    obj = fit.as_objective(lambda y: torch.sum(y ** 2), ys)  # every frame has a cotangent, frame 0 included
    pmap = fit.ParamMap.of({"mu": ChemLeg(np.array([0.1, -2.0]), F.logit), "D": DiffLeg(np.array([0.3]))}, P.CahnHilliard2DPeriodic)
    rec = _Recorder(np.array([[1.5, -2.5]]))
    J, grad = fit.objective_gradient(obj, ys, 2, rec, pmap)
    assert rec.seen.shape == (3, 1, 6, 5) and rec.seen.flags.c_contiguous
    np.testing.assert_array_equal(rec.seen[:, 0], 2 * ys[1:])
    np.testing.assert_array_equal(grad, [0.0, 1.5, -2.5])  # mu's constant coefficient is inert for Cahn-Hilliard
    # batched: (T, B, *spatial) goes through as it is and the trajectories are summed
    ysb = rng.standard_normal((3, 2, 6, 5))
    rec = _Recorder(np.array([[1.0, 2.0], [10.0, 20.0]]))
    _, grad = fit.objective_gradient(fit.as_objective(lambda y: torch.sum(y ** 2)), ysb, 2, rec, pmap)
    np.testing.assert_array_equal(rec.seen, 2 * ysb[1:])
    np.testing.assert_array_equal(grad, [0.0, 11.0, 22.0])


# ---- gradient assembly against central differences of the numpy trajectory -----------------------------------------------


def _cases():
    n = 12
    dom = P.Domain((n, 10), ((-0.06, 0.06), (-0.05, 0.05)), "dimensionless")
    ch = R.ch_stepper_factory(dom, 0.002, 3)
    ch_pmap = fit.ParamMap.of({"mu": ChemLeg(np.zeros(3), F.logit), "D": DiffLeg(np.zeros(2))}, P.CahnHilliard2DPeriodic)
    ac = lambda p: R.ac_stepper(p, n=n, dt=1e-6)
    return {"ch2d_imex": (ch, ch_pmap, np.array([0.0, -3.0, 0.2, -1.0, 0.2]), (n, 10)),
            "ac2d_rk4": (ac, R.ac_pmap(), np.array(F.MU_TRUE + F.R_TRUE), (n, n))}


@pytest.mark.parametrize("name", ["ch2d_imex", "ac2d_rk4"])
def test_gradient_assembly_matches_central_differences(name):
    make, pmap, p, shape = _cases()[name]
    rng = np.random.default_rng(2)
    y0s = np.clip(0.5 + 0.05 * rng.standard_normal((2,) + shape), 0.1, 0.9)
    target = torch.tensor(0.5 + 0.05 * rng.standard_normal((2,) + shape))
    obj = fit.as_objective(lambda y: torch.mean((y[-1] - target) ** 2) + 0.1 * torch.mean(y[1] ** 2))
    vg, v = R.value_and_grad_fns(fit, obj, make, y0s, pmap.sens_params(), [15, 25], pmap)
    J, grad = vg(p)
    assert abs(J - v(p)) <= 1e-15 * abs(J)
    eps = 1e-5
    cd = np.array([(v(p + eps * e) - v(p - eps * e)) / (2 * eps) for e in np.eye(len(p))])
    assert np.max(np.abs(grad)) > 0
    assert np.max(np.abs(grad - cd)) <= 1e-7 * np.max(np.abs(grad))  # test_sens_ac_cpu.py's gate for tangent steps
    assert np.all(grad[~pmap.active()] == 0.0)


# ---- refusals -----------------------------------------------------------------------------------------------------------------


def _model(equation=P.AllenCahn2DPeriodic, solver=P.RK4):
    return P.PDEModel(equation, P.Domain((64, 64), ((0, 1), (0, 1)), "dimensionless"), solver)


def _mu():
    return ChemLeg(np.array([0.1, -2.0]), F.logit)


def _optimize(model, objective, opt, other):
    sp = {"A": 0.5} if model.solver_type is P.SemiImplicitFourierSpectral else {}
    return model.optimize(objective, np.full((64, 64), 0.5), [0.0, 1e-6], opt, other, sp, {}, 0.0)


_TORCH = lambda ys: torch.mean(ys[-1] ** 2)  # noqa: E731


def test_optimize_without_arguments_raises():
    with pytest.raises(NotImplementedError, match="torch-differentiable.*value_and_grad"):
        _model().optimize()


def test_numpy_only_callable_is_refused_naming_both_forms():
    with pytest.raises(NotImplementedError, match="torch-differentiable.*value_and_grad"):
        _optimize(_model(), lambda ys: np.mean(np.asarray(ys)[-1] ** 2), {"mu": _mu()}, {"R": DiffLeg(np.array([0.0])), "kappa": 0.002})
    with pytest.raises(NotImplementedError, match="torch-differentiable.*value_and_grad"):
        _optimize(_model(), lambda ys: 1.0, {"mu": _mu()}, {"R": DiffLeg(np.array([0.0])), "kappa": 0.002})
    with pytest.raises(NotImplementedError, match="torch-differentiable.*value_and_grad"):
        _optimize(_model(), 3.0, {"mu": _mu()}, {"R": DiffLeg(np.array([0.0])), "kappa": 0.002})


def test_unsupported_pairs_are_refused_as_by_train():
    with pytest.raises(NotImplementedError, match="Euler and RK4"):
        _optimize(_model(P.AllenCahn2DPeriodic, P.Tsit5), _TORCH, {"mu": _mu()}, {"R": DiffLeg(np.array([0.0])), "kappa": 0.002})
    with pytest.raises(NotImplementedError, match="SemiImplicitFourierSpectral"):
        _optimize(_model(P.CahnHilliard2DPeriodic, P.RK4), _TORCH, {"mu": _mu()}, {"D": DiffLeg(np.array([0.0])), "kappa": 0.002})
    with pytest.raises(NotImplementedError, match="fd"):
        _optimize(_model(P.AllenCahn2DPeriodic, P.Euler), _TORCH, {"mu": _mu()},
                  {"R": DiffLeg(np.array([0.0])), "kappa": 0.002, "derivs": "fourier"})
    with pytest.raises(ValueError, match="kappa"):
        _optimize(_model(P.CahnHilliard2DPeriodic, P.SemiImplicitFourierSpectral), _TORCH, {"mu": _mu(), "kappa": 0.002},
                  {"D": DiffLeg(np.array([0.0]))})
    model = _model(P.CahnHilliard2DPeriodic, P.Euler)
    model.equation_type = dict
    with pytest.raises(NotImplementedError, match="CahnHilliard2DPeriodic on a 2-D domain"):
        _optimize(model, _TORCH, {"mu": _mu()}, {})


# ---- train(method="mse") follows the numbers it did ---------------------------------------------------------------------

# fit.bfgs on the problem of tests/ac_fit_problem.py through the numpy tangents (optimize_ref.cpu_train_mse), recorded on
# the commit before bfgs and minimize_bfgs shared their loop: the fitted vector, the number of accepted steps + 1 and
# the final objective
PARENT_P = ["0x1.999999998feb0p-4", "-0x1.7fffffffff98ap+1", "0x1.333333332d90ep-2", "0x1.b999999999f8fp+2", "0x1.333333332bd9ap-2"]
PARENT_HIST = (21, "0x1.3ed4db4b1c71cp-92")


def test_train_mse_is_bit_identical_to_the_parent():
    p, hist = R.cpu_train_mse(fit)
    assert [float(x).hex() for x in p] == PARENT_P
    assert (len(hist), float(hist[-1]).hex()) == PARENT_HIST
