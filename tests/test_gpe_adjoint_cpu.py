"""CPU checks of the GPE control gradient's host side and of its reference (tests/gpe_adjoint_ref.py): the torch step
against the numpy oracle, its autograd gradient against central differences of the oracle, SpotMap, the refusals."""
import numpy as np
import pytest

import pde_opt_amd as P
from oracle import np_oracle as O
from pde_opt_amd import gpe_control
from pde_opt_amd.gpe_control import SpotMap
from pde_opt_amd.numerics.functions.lights import SPOT_NUMBERS, GaussianSpot, GaussianSpots
from pde_opt_amd.utils import prepare_solver_params

import gpe_adjoint_ref as R

K_GPE, E_GPE, TRAP = 1.3, 0.2, 0.7
SPOTS = np.array([[1.5, -0.8, 0.4, 0.9, -0.3, 0.5, 0.6], [-0.7, 0.4, -0.8, -0.6, 0.5, 0.3, 0.9]])


def make(points, kinetic, time_scale, p=SPOTS):
    dom = P.Domain(points, ((-2.0, 2.0), (-1.5, 1.5)), "dimensionless")
    spots = SpotMap(len(p)).build(np.asarray(p).reshape(-1))
    eq = P.GPE2DTSControl(dom, K_GPE, E_GPE, spots, trap_factor=TRAP, kinetic=kinetic)
    solver = P.StrangSplitting(**prepare_solver_params(P.StrangSplitting, {"time_scale": time_scale}, eq))
    return eq, solver


def state(points, seed=0, batch=None):
    rng = np.random.default_rng(seed)
    shape = (() if batch is None else (batch,)) + tuple(points) + (2,)
    return rng.standard_normal(shape)


def oracle_step(eq, solver, p, y, t0, dt):
    spots = SpotMap(len(p)).build(np.asarray(p).reshape(-1))
    b = lambda t, s: O.gpe_b_terms(s, eq.xmesh, eq.ymesh, eq.k, eq.e, eq.trap_factor, spots(t, eq.xmesh, eq.ymesh))
    return O.strang_step(b, t0, y, dt, np.asarray(solver.A_term), solver.dx, solver.time_scale)


@pytest.mark.parametrize("kinetic", [False, True])
@pytest.mark.parametrize("time_scale", [1.0, -1j])
def test_reference_step_equals_the_oracle(kinetic, time_scale):
    import torch

    eq, solver = make((12, 10), kinetic, time_scale)
    y = state((12, 10))
    case = R.Case.of(eq, solver)
    got = R.step(case, torch.as_tensor(y), torch.as_tensor(SPOTS), 0.3, 0.02).numpy()
    want = oracle_step(eq, solver, SPOTS, y, 0.3, 0.02)
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("time_scale", [1.0, 0.3 - 1j])
def test_reference_gradient_equals_central_differences_of_the_oracle(time_scale):
    eq, solver = make((12, 10), True, time_scale)
    y0 = state((12, 10), 1)
    w = state((12, 10), 2)
    t0, dt, n = 0.2, 0.02, 3

    def J(p):
        y = y0
        for i in range(n):
            y = oracle_step(eq, solver, p, y, t0 + i * dt, dt)
        return float(np.sum(w * y))

    ts = np.array([t0, t0 + n * dt])
    _, _, grad, _ = R.solve_grad(R.Case.of(eq, solver), y0, SPOTS, ts, dt, lambda ys: (ys[-1] * R.torch.as_tensor(w)).sum())
    h = 1e-4
    fd = np.zeros_like(SPOTS)
    for idx in np.ndindex(SPOTS.shape):
        d = np.zeros_like(SPOTS)
        d[idx] = h
        fd[idx] = (J(SPOTS + d) - J(SPOTS - d)) / (2 * h)
    # central differences with step h: truncation h^2 / 6 |J'''| + rounding eps |J| / h.  All numbers of the problem are
    # O(1) and the spots' widths are 0.6 and 0.9, so |J'''| and |J| are within two decades of the largest gradient
    # component: 100 (h^2 + eps / h) = 1e-6 of it
    tol = 100.0 * (h * h + np.finfo(float).eps / h)
    assert np.max(np.abs(grad - fd)) <= tol * np.max(np.abs(fd))
    assert np.all(np.abs(fd).max(axis=0) > 0)  # every one of the 7 numbers is exercised


def test_spot_map_round_trip_and_free():
    spots = GaussianSpots([GaussianSpot(*row) for row in SPOTS], free=("y0", "x0"))
    assert spots.free == ("x0", "y0")  # in the order of SPOT_NUMBERS
    m = SpotMap.of(spots)
    p = m.flatten(spots)
    assert p.shape == (14,) and m.size == 14
    np.testing.assert_array_equal(p.reshape(2, 7), SPOTS)
    back = m.build(p)
    assert back.free == spots.free and back.spots == spots.spots
    act = m.active()
    assert act.shape == (2, 7) and [n for n, a in zip(SPOT_NUMBERS, act[0]) if a] == ["x0", "y0"]
    assert SpotMap.of(GaussianSpots(spots.spots)).active().all()
    np.testing.assert_array_equal(m.weight_vector(2.0), np.full(14, 2.0))
    np.testing.assert_array_equal(m.weight_vector(np.arange(14.0).reshape(2, 7)), np.arange(14.0))
    with pytest.raises(ValueError):
        GaussianSpots(spots.spots, free=("radius",))
    with pytest.raises(ValueError):
        m.build(np.zeros(7))


def test_width_chain_rule_against_a_finite_difference():
    # the library differentiates with respect to inv_two_w2 = 1 / (2 w^2); the host turns that into d/dw
    spots = GaussianSpots([GaussianSpot(*row) for row in SPOTS])
    raw = np.zeros((2, 7))
    raw[:, 6] = [0.37, -1.2]  # dJ / d inv_two_w2
    got = SpotMap.user_gradient(spots, raw)[:, 6]
    h = 1e-6
    for s, w in enumerate(SPOTS[:, 6]):
        c = lambda v: GaussianSpot(0, 0, 0, 0, 0, 0, v).inv_two_w2
        fd = raw[s, 6] * (c(w + h) - c(w - h)) / (2 * h)
        assert abs(got[s] - fd) <= 1e-8 * abs(fd)  # h^2 of the third derivative + eps / h
    np.testing.assert_array_equal(SpotMap.user_gradient(spots, raw)[:, :6], 0.0)


def test_add_refuses_operands_that_disagree_on_free():
    a = GaussianSpots.single(1.0, 0.0, 0.0, 0.5)
    b = GaussianSpots([GaussianSpot(*SPOTS[0])], free=("x0",))
    with pytest.raises(ValueError, match="free"):
        a + b
    both = b + GaussianSpots([GaussianSpot(*SPOTS[1])], free=("x0",))
    assert both.free == ("x0",) and len(both.spots) == 2
    assert (a + a).free is None


def test_unsupported_cases_raise_before_any_engine(monkeypatch):
    import pde_opt_amd.engine as E

    def no_engine(self, *a, **k):
        raise AssertionError("an engine was created")

    monkeypatch.setattr(E.HipEngine, "__init__", no_engine)
    dom = P.Domain((16, 16), ((-2.0, 2.0), (-2.0, 2.0)), "dimensionless")
    y0 = np.ones((16, 16, 2))
    ts = [0.0, 0.1]
    spots = GaussianSpots.single(1.0, 0.0, 0.0, 0.5)

    class Obj:
        def value_and_grad(self, ys):
            return float(np.sum(ys)), np.ones_like(ys)

    model = P.PDEModel(P.GPE2DTSControl, dom, P.StrangSplitting)
    base = dict(k=1.0, e=0.0)
    with pytest.raises(NotImplementedError, match="GaussianSpots"):  # another lights callable
        model.control_gradient(Obj(), y0, ts, dict(base, lights=lambda t, x, y: 0.0 * x))
    with pytest.raises(NotImplementedError, match="GaussianSpots"):
        model.optimize(Obj(), y0, ts, {"lights": lambda t, x, y: 0.0 * x}, base)
    for name in ("k", "e", "trap_factor"):  # other optimisation variables
        other = {n: v for n, v in dict(base, trap_factor=1.0, lights=spots).items() if n != name}
        with pytest.raises(NotImplementedError, match="GaussianSpots"):
            model.optimize(Obj(), y0, ts, {name: 1.0}, other)
    with pytest.raises(NotImplementedError, match="time_dependent"):
        model.control_gradient(Obj(), y0, ts, dict(base, lights=spots, time_dependent=False))
    with pytest.raises(NotImplementedError):  # optimize keeps refusing a missing objective first
        model.optimize(None, y0, ts, {"lights": spots}, base)
    with pytest.raises(NotImplementedError, match="StrangSplitting"):  # any solver but Strang
        gpe_control.reject_unsupported(P.GPE2DTSControl, P.RK4)
    with pytest.raises(NotImplementedError, match="GaussianSpots"):  # another equation
        gpe_control.reject_unsupported(P.CahnHilliard2DPeriodic, P.StrangSplitting)
