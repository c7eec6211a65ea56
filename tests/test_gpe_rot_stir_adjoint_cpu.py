"""CPU checks of the stirred rotating-frame GPE's gradient entries and of their reference
(tests/gpe_rot_stir_adjoint_ref.py): the torch step against the independent numpy step of tests/gpe_rot_stir_ref.py,
its autograd gradient against central differences of that numpy step, the new ABI symbol, and the refusals and the
flat-vector bookkeeping of ``stirring_gradient`` / ``optimize_stirring`` (no engine, no GPU)."""
import os
import re

import numpy as np
import pytest
import torch

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd.numerics.functions.lights import GaussianSpot, GaussianSpots

import gpe_rot_ref as RR
import gpe_rot_stir_adjoint_ref as A
import gpe_rot_stir_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
BOX = ((-2.0, 2.0), (-1.5, 1.5))
POINTS, DT, T0 = (48, 40), 0.02, 0.3
P4 = np.array([50.0, 0.1, 0.5, 0.9])  # k, e, omega, rate
# two moving spots in the library's order: amp0, amp_rate, x0, x_rate, y0, y_rate, inv_two_w2
SPOTS = np.array([[3.0, 0.5, -0.6, 0.8, 0.3, -0.4, 1.0 / (2 * 0.35**2)], [-2.0, 1.0, 0.7, -0.5, -0.45, 0.6, 1.0 / (2 * 0.25**2)]])


def lights_of(rows):
    """the light field of (S, 7) rows as a plain callable, written out here: not the library's GaussianSpots"""
    def lights(t, x, y):
        return sum((a0 + a1 * t) * np.exp(-((x - x0 - x1 * t) ** 2 + (y - y0 - y1 * t) ** 2) * c) for a0, a1, x0, x1, y0, y1, c in rows)
    return lights


def numpy_step(dom, p, rows, time_scale, psi, t0=T0):
    return S.StirCase(dom, p[0], p[1], p[2], time_scale, True, lights_of(rows), p[3]).step(psi, DT, t0)


@pytest.mark.parametrize("time_scale", [1.0, -1j, 0.3 - 1j])
def test_torch_step_equals_the_numpy_step(time_scale):
    dom = P.Domain(POINTS, BOX, "dimensionless")
    y0 = np.random.default_rng(7).standard_normal((1,) + POINTS + (2,))
    out = A.step(A.Case(dom, time_scale), torch.as_tensor(y0), torch.as_tensor(P4[None]), torch.as_tensor(SPOTS[None]), DT, T0)
    want = numpy_step(dom, P4, SPOTS, time_scale, RR.from_pairs(y0[0]))
    err = np.max(np.abs(RR.from_pairs(out.numpy()[0]) - want)) / np.max(np.abs(want))
    print(f"torch step against numpy step, ts={time_scale}: {err:.3e}")
    assert err <= 1e-12


def test_reference_gradient_against_a_difference_quotient():
    """autograd of the torch step over the 4 scalars and the 14 spot numbers against central differences of the numpy
    step.  The difference step 1e-5 is the one that minimises the mismatch on this case (measured over 1e-3 .. 1e-7:
    truncation takes over above it, cancellation below); every quantity within 1e-6 of its block's largest entry."""
    dom = P.Domain(POINTS, BOX, "dimensionless")
    rng = np.random.default_rng(3)
    y0, lam1 = rng.standard_normal((1,) + POINTS + (2,)), rng.standard_normal((1,) + POINTS + (2,))
    ts = 0.3 - 1j
    g, gs, _ = A.step_vjp(A.Case(dom, ts), y0, P4[None], SPOTS[None], DT, T0, lam1)
    psi = RR.from_pairs(y0[0])
    J = lambda p, rows: float(np.sum(RR.to_pairs(numpy_step(dom, p, rows, ts, psi)) * lam1[0]))
    H = 1e-5
    for j in range(4):
        h = np.zeros(4)
        h[j] = H
        fd = (J(P4 + h, SPOTS) - J(P4 - h, SPOTS)) / (2 * H)
        print(f"scalar {j}: autograd {g[0, j]:.9e} difference {fd:.9e}")
        assert abs(fd - g[0, j]) <= 1e-6 * np.max(np.abs(g)), (j, fd, g[0, j])
    for s in range(2):
        for j in range(7):
            h = np.zeros_like(SPOTS)
            h[s, j] = H
            fd = (J(P4, SPOTS + h) - J(P4, SPOTS - h)) / (2 * H)
            print(f"spot {s} number {j}: autograd {gs[0, s, j]:.9e} difference {fd:.9e}")
            assert abs(fd - gs[0, s, j]) <= 1e-6 * np.max(np.abs(gs)), (s, j, fd, gs[0, s, j])


# ---- ABI ----------------------------------------------------------------------------------------------------------------

def test_the_new_symbol_is_declared_and_bound():
    header = open(os.path.join(os.path.dirname(HERE), "include", "pdeopt_hip.h")).read()
    decl = re.search(r"int\s+pdeopt_gpe_rot_stir_adjoint_step\s*\(([^)]*)\)\s*;", header)
    assert decl and len(decl.group(1).split(",")) == 7
    assert len(L._SIGNATURES["pdeopt_gpe_rot_stir_adjoint_step"][1]) == 7
    assert hasattr(L.load_library(), "pdeopt_gpe_rot_stir_adjoint_step")
    assert callable(P.HipEngine.gpe_rot_stir_adjoint_step)


# ---- refusals -----------------------------------------------------------------------------------------------------------

DOM = P.Domain((16, 16), ((-2.0, 2.0), (-2.0, 2.0)), "dimensionless")
Y0 = np.zeros((16, 16, 2))
TS = [0.0, 0.1]
OBJ = lambda ys: ys.sum()
BASE = dict(k=1.0, e=0.0, omega=0.3)


def spots(free=None):
    return GaussianSpots([GaussianSpot(1.0, 0.5, 0.1, 0.2, -0.1, 0.3, 0.4), GaussianSpot(-1.0, 0.0, -0.3, 0.1, 0.2, 0.0, 0.5)], free=free)


def test_the_new_entries_refuse_another_equation_or_solver():
    m = P.PDEModel(P.GPE2DTSControl, DOM, P.StrangSplitting)
    params = dict(k=1.0, e=0.0, lights=spots())
    with pytest.raises(NotImplementedError, match="GPE2DTSRot with RotatingStrangSplitting"):
        m.stirring_gradient(OBJ, Y0, TS, params)
    with pytest.raises(NotImplementedError, match="GPE2DTSRot with RotatingStrangSplitting"):
        m.optimize_stirring(OBJ, Y0, TS, {"k": 1.0}, {"e": 0.0})
    ch = P.PDEModel(P.CahnHilliard2DPeriodic, DOM, P.RK4)
    with pytest.raises(NotImplementedError, match="CahnHilliard2DPeriodic"):
        ch.stirring_gradient(OBJ, np.zeros((16, 16)), TS, {})


def test_the_new_entries_refuse_unknown_names_adaptive_steps_and_other_lights():
    m = P.PDEModel(P.GPE2DTSRot, DOM, P.RotatingStrangSplitting)
    with pytest.raises(NotImplementedError, match=r"\['trap_factor'\].*subset of k, e, omega, omega_rate and lights"):
        m.optimize_stirring(OBJ, Y0, TS, {"trap_factor": 1.0}, BASE)
    with pytest.raises(NotImplementedError, match="subset of k, e, omega, omega_rate and lights"):
        m.optimize_stirring(OBJ, Y0, TS, {}, BASE)
    pid = P.PIDController(rtol=1e-3, atol=1e-6)
    with pytest.raises(NotImplementedError, match="PIDController.*ConstantStepSize"):
        m.stirring_gradient(OBJ, Y0, TS, dict(BASE, omega_rate=0.5), stepsize_controller=pid)
    with pytest.raises(NotImplementedError, match="PIDController.*ConstantStepSize"):
        m.optimize_stirring(OBJ, Y0, TS, {"omega_rate": 0.3}, BASE, stepsize_controller=pid)
    # a callable of time that is no GaussianSpots: the forward solve's ValueError stays, the gradient says what it covers
    moving = lambda t, x, y: t * x
    with pytest.raises(ValueError, match="time-dependent lights must be a GaussianSpots"):
        m.solve(dict(BASE, lights=moving), Y0, TS)
    with pytest.raises(NotImplementedError, match="time-dependent lights must be a GaussianSpots.*stirring_gradient"):
        m.stirring_gradient(OBJ, Y0, TS, dict(BASE, lights=moving))
    with pytest.raises(NotImplementedError, match="as an optimisation variable"):
        m.optimize_stirring(OBJ, Y0, TS, {"lights": lambda t, x, y: 0.0 * x}, BASE)


class ReachedTheEngine(Exception):
    pass


def no_engine(monkeypatch, m):
    def solve(*a, **k):
        raise ReachedTheEngine()
    monkeypatch.setattr(m, "solve", solve)


@pytest.mark.parametrize("extra", [dict(lights=None, omega_rate=0.0), dict(lights=spots(), omega_rate=0.5),
                                   dict(lights=lambda t, x, y: 0.1 * x * x)])
def test_supported_problems_are_accepted_up_to_the_engine(monkeypatch, extra):
    """spots, a ramp, a static callable, and neither of them: nothing refuses before the forward solve"""
    m = P.PDEModel(P.GPE2DTSRot, DOM, P.RotatingStrangSplitting)
    no_engine(monkeypatch, m)
    with pytest.raises(ReachedTheEngine):
        m.stirring_gradient(OBJ, Y0, TS, dict(BASE, **extra))
    with pytest.raises(ReachedTheEngine):
        m.optimize_stirring(OBJ, Y0, TS, {"omega": 0.3}, dict(k=1.0, e=0.0, **extra))


def test_the_older_entries_keep_refusing_a_stirred_problem():
    m = P.PDEModel(P.GPE2DTSRot, DOM, P.RotatingStrangSplitting)
    with pytest.raises(NotImplementedError, match="without lights and with omega_rate = 0"):
        m.rotation_gradient(OBJ, Y0, TS, dict(BASE, omega_rate=0.5))
    with pytest.raises(NotImplementedError, match="without lights and with omega_rate = 0.*stirring_gradient"):
        m.rotation_gradient(OBJ, Y0, TS, dict(BASE, lights=spots()))
    with pytest.raises(NotImplementedError, match="without lights and with omega_rate = 0"):
        m.optimize_rotation(OBJ, Y0, TS, {"omega": 0.3}, dict(k=1.0, e=0.0, lights=spots()))


def test_optimize_stirring_flat_vector_round_trip_and_free_mask(monkeypatch):
    """the flat vector is (e, omega_rate) in the library's order, then the spots' 14 numbers; entries that are not free
    get a zero gradient and come back unchanged.  The gradient is a stub: J = sum (p - target)^2 over the whole vector."""
    m = P.PDEModel(P.GPE2DTSRot, DOM, P.RotatingStrangSplitting)
    start = spots(free=("x_rate", "amp0"))
    flat0 = np.array([[getattr(s, n) for n in ("amp0", "amp_rate", "x0", "x_rate", "y0", "y_rate", "width")] for s in start.spots])
    target = dict(e=0.25, omega_rate=-0.4, lights=flat0 + 0.1)
    seen = []

    def residual(params):
        lights = np.array([[getattr(s, n) for n in ("amp0", "amp_rate", "x0", "x_rate", "y0", "y_rate", "width")]
                           for s in params["lights"].spots])
        return params["e"] - target["e"], params["omega_rate"] - target["omega_rate"], lights - target["lights"]

    def value_of(params):
        re, rr, rl = residual(params)
        return re * re + rr * rr + float(np.sum(rl * rl))

    def stirring_gradient(objective, y0, ts, params, solver_parameters=None, dt0=1e-6, **kw):
        seen.append(params)
        assert params["k"] == 1.0 and params["omega"] == 0.3 and params["lights"].free == ("amp0", "x_rate")
        re, rr, rl = residual(params)
        return value_of(params), {"k": 7.0, "e": 2 * re, "omega": 7.0, "omega_rate": 2 * rr, "lights": 2 * rl}, None

    class Obj:
        def value_and_grad(self, ys):
            raise AssertionError("the stub gradient never solves")

        def value(self, ys):
            return value_of(np.asarray(ys).item())  # `solve` below hands the parameters through (as a 0-d object array)

    monkeypatch.setattr(m, "stirring_gradient", stirring_gradient)
    monkeypatch.setattr(m, "solve", lambda params, *a, **k: params)
    out = m.optimize_stirring(Obj(), Y0, TS, {"omega_rate": 0.1, "lights": start, "e": 0.0}, dict(k=1.0, omega=0.3), max_steps=50)
    assert out["k"] == 1.0 and out["omega"] == 0.3
    assert abs(out["e"] - target["e"]) <= 1e-6 and abs(out["omega_rate"] - target["omega_rate"]) <= 1e-6
    got = np.array([[getattr(s, n) for n in ("amp0", "amp_rate", "x0", "x_rate", "y0", "y_rate", "width")] for s in out["lights"].spots])
    free = np.array([True, False, False, True, False, False, False])
    np.testing.assert_allclose(got[:, free], target["lights"][:, free], atol=1e-6)
    np.testing.assert_array_equal(got[:, ~free], flat0[:, ~free])  # the masked numbers never moved
    assert out["lights"].free == ("amp0", "x_rate")
    # the first point the gradient saw is the start, number for number
    assert seen[0]["e"] == 0.0 and seen[0]["omega_rate"] == 0.1
    assert [s for s in seen[0]["lights"].spots] == list(start.spots)
    assert m.last_optimize_history[-1] < m.last_optimize_history[0]
