"""The stirred, ramped rotating-frame GPE without a GPU: the numpy reference
(tests/gpe_rot_stir_ref.py) against the references it extends, the refusals (no engine may be created), what
``GPE2DTSRot`` uploads (on tests/fake_engine.py) and the new ABI symbol."""
import os
import re

import numpy as np
import pytest

import gpe_rot_ref as R
import gpe_rot_stir_ref as S
import pde_opt_amd as P
from fake_engine import OracleEngine
from oracle import np_oracle as O
from pde_opt_amd import _lib as L
from pde_opt_amd.numerics.functions.lights import GaussianSpot, GaussianSpots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOM = P.Domain((32, 24), ((-2.0, 2.0), (-1.5, 1.5)), "dimensionless")
SQ = P.Domain((32, 32), ((-5.0, 5.0), (-5.0, 5.0)), "dimensionless")
K, E = 50.0, 0.1
SPOTS = GaussianSpots([GaussianSpot(3.0, 0.5, -0.6, 0.8, 0.3, -0.4, 0.35), GaussianSpot(-2.0, 1.0, 0.7, -0.5, -0.45, 0.6, 0.25)])


# ---- the reference -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("double", [True, False])
@pytest.mark.parametrize("time_scale", [1.0, 0.3 - 1j])
def test_without_spots_and_ramp_the_reference_is_rotcase_exactly(double, time_scale):
    psi = R.smooth_state(DOM, 3)[0]
    old = R.RotCase(DOM, K, E, 0.7, time_scale, double)
    new = S.StirCase(DOM, K, E, 0.7, time_scale, double)
    a, b = psi, psi
    for s in range(3):
        a, b = old.step(a, 0.02), new.step(b, 0.02, 0.3 + s * 0.02)
    assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("time_scale", [1.0, -1j, 0.3 - 1j])
def test_omega_zero_with_spots_is_the_oracles_strang_step_with_the_kinetic_a_term(time_scale):
    psi = R.smooth_state(SQ, 3)[0]
    x, y = SQ.mesh()
    kx, ky = SQ.fft_mesh()
    a_term = 0.5j * ((2j * np.pi * kx) ** 2 + (2j * np.pi * ky) ** 2)
    b_terms = lambda t, s: O.gpe_b_terms(s, x, y, K, E, 1.0, SPOTS(t, x, y))
    case = S.StirCase(SQ, K, E, 0.0, time_scale, lights=SPOTS)
    got, want = psi, R.to_pairs(psi)
    for s in range(3):
        t = 0.3 + s * 0.01
        got = case.step(got, 0.01, t)
        want = O.strang_step(b_terms, t, want, 0.01, a_term, SQ.dx[0], time_scale)
    err = np.max(np.abs(got - R.from_pairs(want))) / np.max(np.abs(want))
    assert err <= 1e-13, err


def test_the_ramp_and_the_spots_change_the_step_and_single_precision_follows():
    psi = R.smooth_state(DOM, 3)[0]
    plain = S.StirCase(DOM, K, E, 0.7).advance(psi, 0.02, 3, 0.3)
    ramp = S.StirCase(DOM, K, E, 0.7, omega_rate=0.9).advance(psi, 0.02, 3, 0.3)
    lit = S.StirCase(DOM, K, E, 0.7, lights=SPOTS).advance(psi, 0.02, 3, 0.3)
    assert np.max(np.abs(ramp - plain)) > 1e-4 and np.max(np.abs(lit - plain)) > 1e-4
    # a ramp is the frozen step at Omega(t0), step by step
    by_hand = psi
    for s in range(3):
        by_hand = R.RotCase(DOM, K, E, 0.7 + 0.9 * (0.3 + s * 0.02)).step(by_hand, 0.02)
    assert np.max(np.abs(by_hand - ramp)) <= 1e-14
    both64 = S.StirCase(DOM, K, E, 0.7, lights=SPOTS, omega_rate=0.9).advance(psi, 0.02, 3, 0.3)
    both32 = S.StirCase(DOM, K, E, 0.7, double=False, lights=SPOTS, omega_rate=0.9).advance(psi, 0.02, 3, 0.3)
    assert both32.dtype == np.complex64 and 0 < np.max(np.abs(both32 - both64)) <= 1e-5


def test_solve_keeps_the_save_semantics_and_hands_every_step_its_time():
    psi = R.smooth_state(DOM, 3)[0]
    case = S.StirCase(DOM, K, E, 0.4, lights=SPOTS, omega_rate=0.9)
    ts = np.array([0.3, 0.32, 0.331, 0.35])  # a save on a step, one inside a step, a clipped last step
    out = S.solve(case, psi, ts, 0.02)
    one = case.step(psi, 0.02, 0.3)
    two = case.step(one, 0.02, 0.32)
    assert np.array_equal(out[0], psi) and np.array_equal(out[1], one)
    np.testing.assert_allclose(out[2], one + 0.55 * (two - one), rtol=0, atol=1e-12)
    np.testing.assert_allclose(out[3], case.step(two, 0.35 - 0.3 - 2 * 0.02, 0.3 + 2 * 0.02), rtol=0, atol=1e-12)


# ---- the equation class -----------------------------------------------------------------------------------------------------

def test_fields_defaults_and_host_terms():
    eq = P.GPE2DTSRot(DOM, K, E, 0.7)
    assert eq.lights is None and eq.omega_rate == 0.0 and isinstance(eq.omega, float)
    assert P.GPE2DTSRot._all_per_env_controls() == frozenset({"k", "e", "omega", "lights", "omega_rate"})
    lit = P.GPE2DTSRot(DOM, K, E, 0.7, SPOTS, 0.9)
    ax0, ay0 = eq.A_terms(None, 0.5)
    ax1, ay1 = lit.A_terms(None, 0.5)
    ref = P.GPE2DTSRot(DOM, K, E, 0.7 + 0.9 * 0.5).A_terms(None, 0.0)
    assert np.array_equal(ax1, ref[0]) and np.array_equal(ay1, ref[1]) and not np.array_equal(ax0, ax1)
    psi = R.smooth_state(DOM, 3)[0]
    x, y = DOM.mesh()
    np.testing.assert_allclose(lit.B_terms(psi, 0.5), eq.B_terms(psi, 0.5) - 1j * SPOTS(0.5, x, y), rtol=1e-14)
    np.testing.assert_allclose(lit.potential(0.5), eq.trap_potential() + SPOTS(0.5, x, y), rtol=1e-15)
    with pytest.raises(ValueError, match="callable"):
        P.GPE2DTSRot(DOM, K, E, 0.7, lights=3.0)


# ---- refusals, before any engine exists ----------------------------------------------------------------------------------------

@pytest.fixture
def no_engine(monkeypatch):
    import pde_opt_amd.engine as EN

    def refuse(self, *a, **k):
        raise AssertionError("an engine was created")

    monkeypatch.setattr(EN.HipEngine, "__init__", refuse)


Y0 = np.zeros(tuple(DOM.points) + (2,))
MOVING = lambda t, x, y: np.sin(t) * x


def test_a_host_sampled_lights_is_refused_and_names_the_spots(no_engine):
    m = P.PDEModel(P.GPE2DTSRot, DOM, P.RotatingStrangSplitting)
    with pytest.raises(ValueError, match="GaussianSpots"):
        m.solve(dict(k=K, e=E, omega=0.3, lights=MOVING), Y0, [0.0, 0.1], dt0=0.02)


def test_ground_state_refuses_a_ramp_and_moving_spots(no_engine):
    m = P.PDEModel(P.GPE2DTSRot, DOM, P.RotatingStrangSplitting)
    with pytest.raises(ValueError, match="omega_rate"):
        m.ground_state(dict(k=K, e=E, omega=0.3, omega_rate=0.5), Y0, 0.01)
    with pytest.raises(ValueError, match="pinning beam"):
        m.ground_state(dict(k=K, e=E, omega=0.3, lights=SPOTS), Y0, 0.01)
    with pytest.raises(ValueError, match="omega_rate"):
        m.ground_state([dict(k=K, e=E, omega=0.3), dict(k=K, e=E, omega=0.3, omega_rate=-0.1)], np.stack([Y0, Y0]), 0.01)


def test_rotation_gradients_refuse_lights_and_a_ramp(no_engine):
    m = P.PDEModel(P.GPE2DTSRot, DOM, P.RotatingStrangSplitting)
    J = lambda ys: ys.sum()
    pin = GaussianSpots.single(2.0, 0.1, 0.2, 0.3)
    for extra in (dict(lights=pin), dict(omega_rate=0.5)):
        with pytest.raises(NotImplementedError, match="without lights and with omega_rate = 0"):
            m.rotation_gradient(J, Y0, [0.0, 0.1], dict(k=K, e=E, omega=0.3, **extra), dt0=0.02)
        with pytest.raises(NotImplementedError, match="without lights and with omega_rate = 0"):
            m.optimize_rotation(J, Y0, [0.0, 0.1], {"omega": 0.3}, dict(k=K, e=E, **extra), dt0=0.02)


# ---- what the equation uploads -----------------------------------------------------------------------------------------------------

class RecordingEngine(OracleEngine):
    """the oracle-backed engine double plus the rotating frame's setters, every call recorded in order"""

    def __init__(self, batch):
        super().__init__()
        self.configure(L.EQ_GPE, np.float64, DOM.points[0], DOM.points[1], batch, DOM.dx[0], DOM.dx[1], gpe_k=K)
        self.log = []

    def set_gpe_spots(self, tables, x_first=0.0, y_first=0.0, env_first=0):
        self.log.append(("spots", None if tables is None else np.array(tables), x_first, y_first))
        super().set_gpe_spots(tables, x_first, y_first, env_first)

    def set_aux(self, which, field, per_env=False, key=None):
        self.log.append(("aux", which, np.array(field), bool(per_env)))
        super().set_aux(which, field, per_env, key)

    def set_env_gpe_k(self, env_first, k):
        self.log.append(("k", env_first, list(k)))

    def set_gpe_rotation(self, omega, x_first, y_first):
        self.log.append(("rotation", omega, x_first, y_first))

    def set_env_gpe_omega(self, env_first, omega):
        self.log.append(("omega", env_first, list(omega)))

    def set_env_gpe_omega_rate(self, env_first, rate):
        self.log.append(("rate", env_first, list(rate)))

    def set_aux_time_fn(self, *a, **k):
        raise AssertionError("the rotating step samples nothing on the host")


def names(eng):
    return [c[0] for c in eng.log]


CELL0 = (float(DOM.axes()[0][0]), float(DOM.axes()[1][0]))


def test_without_lights_and_ramp_the_calls_are_the_parents():
    eng = RecordingEngine(1)
    eq = P.GPE2DTSRot(DOM, K, E, 0.7)
    eq._engine_upload(eng, 0.0, 1.0)
    assert names(eng) == ["spots", "aux", "rotation"]
    assert eng.log[0][1] is None
    assert eng.log[1][1] == L.AUX_GPE_POTENTIAL and np.array_equal(eng.log[1][2], eq.trap_potential()) and not eng.log[1][3]
    assert eng.log[2][1:] == (0.7, *CELL0)
    eng = RecordingEngine(3)
    eqs = [P.GPE2DTSRot(DOM, K + b, E, 0.1 * b) for b in range(3)]
    P.GPE2DTSRot._engine_upload_batch(eng, eqs, 0.0, 1.0)
    assert names(eng) == ["spots", "k", "aux", "rotation", "omega"]
    assert eng.log[0][1] is None and eng.log[1][2] == [K, K + 1, K + 2] and not eng.log[2][3]
    assert eng.log[4][2] == [0.0, 0.1, 0.2]


def test_single_upload_sends_spots_rate_and_the_trap():
    eng = RecordingEngine(2)
    eq = P.GPE2DTSRot(DOM, K, E, 0.7, SPOTS, 0.9)
    eq._engine_upload(eng, 0.0, 1.0)
    assert names(eng) == ["spots", "aux", "rotation", "rate"]
    tab = eng.log[0][1]
    assert tab.shape == (2, 2, 7) and np.array_equal(tab[0], SPOTS.table(2)) and np.array_equal(tab[1], tab[0])
    assert eng.log[0][2:] == CELL0
    assert np.array_equal(eng.log[1][2], eq.trap_potential())  # the spots are NOT folded in
    assert eng.log[3][1:] == (0, [0.9, 0.9])
    # the rate comes after set_gpe_rotation, which resets the rates
    assert names(eng).index("rate") > names(eng).index("rotation")


def test_static_lights_are_folded_into_the_potential():
    x, y = DOM.mesh()
    pin = lambda t, xx, yy: 2.0 * np.exp(-(xx**2 + yy**2))
    eng = RecordingEngine(1)
    eq = P.GPE2DTSRot(DOM, K, E, 0.7, pin)
    eq._engine_upload(eng, 0.0, 1.0)
    assert names(eng) == ["spots", "aux", "rotation"] and eng.log[0][1] is None
    np.testing.assert_allclose(eng.log[1][2], eq.trap_potential() + pin(0.0, x, y), rtol=1e-15)
    # one potential (t_end None: a ground state, an evaluation): spots frozen at t are a static potential too
    eng = RecordingEngine(1)
    P.GPE2DTSRot(DOM, K, E, 0.7, SPOTS)._engine_upload(eng, 0.25, None)
    assert eng.log[0][1] is None
    np.testing.assert_allclose(eng.log[1][2], eq.trap_potential() + SPOTS(0.25, x, y), rtol=1e-15)
    with pytest.raises(ValueError, match="GaussianSpots"):
        P.GPE2DTSRot(DOM, K, E, 0.7, MOVING)._engine_upload(RecordingEngine(1), 0.0, 1.0)


def test_batch_upload_is_per_environment_and_padded():
    one = GaussianSpots.single((1.5, 0.2), (0.3, -0.1), (-0.2, 0.4), 0.3)
    eqs = [P.GPE2DTSRot(DOM, K, E, 0.1, SPOTS, 0.0), P.GPE2DTSRot(DOM, K + 1, E + 0.1, 0.2, one, -0.4),
           P.GPE2DTSRot(DOM, K + 2, E, 0.3, SPOTS, 0.6)]
    eng = RecordingEngine(3)
    P.GPE2DTSRot._engine_upload_batch(eng, eqs, 0.0, 1.0)
    assert names(eng) == ["spots", "k", "aux", "rotation", "omega", "rate"]
    tab = eng.log[0][1]
    assert tab.shape == (3, 2, 7)
    assert np.array_equal(tab[0], SPOTS.table(2)) and np.array_equal(tab[1], one.table(2)) and tab[1, 1, 0] == 0.0
    aux = eng.log[2]
    assert aux[3] and aux[2].shape == (3,) + tuple(DOM.points)
    for b, eq in enumerate(eqs):
        assert np.array_equal(aux[2][b], eq.trap_potential())
    assert eng.log[4][2] == [0.1, 0.2, 0.3] and eng.log[5][1:] == (0, [0.0, -0.4, 0.6])
    # only the rates differ: one shared trap, no spots, the parent's calls plus the rates
    eng = RecordingEngine(2)
    P.GPE2DTSRot._engine_upload_batch(eng, [P.GPE2DTSRot(DOM, K, E, 0.1, None, r) for r in (0.0, 0.5)], 0.0, 1.0)
    assert names(eng) == ["spots", "k", "aux", "rotation", "omega", "rate"] and eng.log[0][1] is None and not eng.log[2][3]


def test_observables_weights_take_the_time():
    from pde_opt_amd.gpe_observables import equation_weights

    eqs = [P.GPE2DTSRot(DOM, K, E, 0.1, None, 0.5), P.GPE2DTSRot(DOM, K, E, -0.2)]
    omega, kappa = equation_weights(eqs, 0.4)
    np.testing.assert_allclose(omega, [0.1 + 0.5 * 0.4, -0.2], rtol=1e-15)
    assert kappa == 1.0
    np.testing.assert_array_equal(equation_weights(eqs)[0], [0.1, -0.2])


# ---- ABI ---------------------------------------------------------------------------------------------------------------------

def test_the_new_symbol_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "pdeopt_hip.h")).read()
    decl = re.search(r"int\s+pdeopt_set_env_gpe_omega_rate\s*\(([^)]*)\)\s*;", header)
    assert decl and len(decl.group(1).split(",")) == 4 and "const double*" in decl.group(1)
    assert len(L._SIGNATURES["pdeopt_set_env_gpe_omega_rate"][1]) == 4
    assert hasattr(L.load_library(), "pdeopt_set_env_gpe_omega_rate")
    from pde_opt_amd.engine import HipEngine

    assert callable(HipEngine.set_env_gpe_omega_rate)
    assert not any(n for n, _ in L.Problem._fields_ if "omega" in n)
