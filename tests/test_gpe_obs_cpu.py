"""GPE observables and the ground-state solve, the part that needs no GPU: the numpy reference against analytic
states, the C ABI's declaration and binding, the refusals, and ``ground_state``'s stopping rule on a stub engine."""
import os
import re

import numpy as np
import pytest

import gpe_obs_ref as R
import gpe_rot_ref as RR
import pde_opt_amd as P
from pde_opt_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOM = P.Domain((64, 64), ((-8.0, 8.0), (-8.0, 8.0)), "dimensionless")


def normalised(psi):
    return psi / np.sqrt(np.sum(np.abs(psi) ** 2) * DOM.dx[0] * DOM.dx[1])


def test_reference_on_the_gaussian():
    x, y = DOM.mesh()
    v, _ = R.observables(DOM, normalised(np.exp(-(x**2 + y**2) / 2)), R.trap(DOM, 0.0), 0.0)
    for name, want in (("norm", 1.0), ("e_kin", 0.5), ("e_pot", 0.5), ("x2", 0.5), ("y2", 0.5), ("l_z", 0.0), ("e_int", 0.0)):
        assert abs(v[name] - want) <= 1e-12, name


def test_reference_on_the_first_vortex_state():
    x, y = DOM.mesh()
    v, _ = R.observables(DOM, normalised((x + 1j * y) * np.exp(-(x**2 + y**2) / 2)), R.trap(DOM, 0.0), 0.0)
    for name, want in (("e_kin", 1.0), ("e_pot", 1.0), ("l_z", 1.0)):
        assert abs(v[name] - want) <= 1e-12, name
    energy, mu = R.derived(v, omega=0.4)
    assert abs(energy - (2.0 - 0.4)) <= 1e-12 and abs(mu - energy) <= 1e-12


def test_reference_single_precision_variant_sums_in_fp64():
    psi = RR.smooth_state(DOM, 3)[0]
    v64, s = R.observables(DOM, psi, R.trap(DOM, 0.1), 50.0)
    v32, _ = R.observables(DOM, psi, R.trap(DOM, 0.1), 50.0, double=False)
    for name in R.NAMES:
        assert 0 < abs(v32[name] - v64[name]) <= 1e-6 * s[name], name


def test_imaginary_time_does_not_raise_the_energy():
    k, e, omega, dt = 50.0, 0.1, 0.5, 0.01
    case = RR.RotCase(DOM, k, e, omega, time_scale=-1j)
    x, y = DOM.mesh()
    psi = np.exp(-((x - 0.7) ** 2 + (y + 0.4) ** 2) / 3).astype(complex)
    prev = None
    for _ in range(200):
        psi = case.step(psi, dt)
        energy, _ = R.derived(R.observables(DOM, psi, case.V, k)[0], omega)
        assert prev is None or energy <= prev + 1e-12
        prev = energy


# ---- header and bindings ---------------------------------------------------------------------------------------------

def test_the_symbol_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "pdeopt_hip.h")).read()
    m = re.search(r"int pdeopt_gpe_observables\(([^)]*)\)", header)
    assert m and len(m.group(1).split(",")) == 7  # the coordinates of cell (0, 0) are arguments
    assert re.search(r"PDEOPT_GPE_OBS_COUNT\s*=\s*8\b", header) and L.GPE_OBS_COUNT == 8
    for i, name in enumerate(P.OBSERVABLE_NAMES):
        assert re.search(rf"PDEOPT_GPE_OBS_{name.upper()}\s*=\s*{i}\b", header), name
        assert getattr(L, "GPE_OBS_" + name.upper()) == i
    assert len(L._SIGNATURES["pdeopt_gpe_observables"][1]) == 7
    assert hasattr(L.load_library(), "pdeopt_gpe_observables")
    assert L.load_library().pdeopt_abi_version() == 1


def test_from_raw_folds_omega_and_kappa_in():
    raw = np.array([[2.0, 1.0, 3.0, 0.5, 0.25, 7.0, 9.0, 0.0], [1.0, 0.0, 1.0, 0.0, -1.0, 1.0, 1.0, 0.0]])
    o = P.GpeObservables.from_raw(raw, omega=[0.4, -0.5], kappa=1.0)
    np.testing.assert_allclose(o.energy, [(1.0 + 3.0 + 0.5 - 0.1) / 2.0, 1.0 - 0.5], rtol=1e-15)
    np.testing.assert_allclose(o.mu, [(1.0 + 3.0 + 1.0 - 0.1) / 2.0, 1.0 - 0.5], rtol=1e-15)
    np.testing.assert_array_equal(o.l_z, raw[:, 4])
    np.testing.assert_allclose(P.GpeObservables.from_raw(raw, kappa=0.0).energy, [3.5 / 2.0, 1.0], rtol=1e-15)
    assert o["x2"][0] == 7.0
    with pytest.raises(ValueError):
        P.GpeObservables.from_raw(raw[:, :7])


# ---- refusals, before any engine exists -------------------------------------------------------------------------------

@pytest.fixture
def no_engine(monkeypatch):
    import pde_opt_amd.engine as E

    def refuse(self, *a, **k):
        raise AssertionError("an engine was created")

    monkeypatch.setattr(E.HipEngine, "__init__", refuse)


def test_other_equations_are_refused(no_engine):
    dom = P.Domain((16, 16), ((0.0, 1.0), (0.0, 1.0)), "dimensionless")
    m = P.PDEModel(P.CahnHilliard2DPeriodic, dom, P.RK4)
    params = dict(kappa=0.1, mu=lambda c: c**3 - c, D=lambda c: 1.0)
    with pytest.raises(NotImplementedError, match="GPE2DTSControl"):
        m.observables(params, np.zeros((16, 16)))
    with pytest.raises(NotImplementedError, match="GPE2DTSControl"):
        m.ground_state(params, np.zeros((16, 16)), 0.01)


def test_real_time_ground_state_is_refused(no_engine):
    m = P.PDEModel(P.GPE2DTSRot, DOM, P.RotatingStrangSplitting)
    with pytest.raises(ValueError, match="time_scale"):
        m.ground_state(dict(k=1.0, e=0.0, omega=0.0), np.zeros((64, 64, 2)), 0.01, solver_parameters={"time_scale": 1.0})


ENV_KW = dict(end_time=1.0, step_dt=0.1, numeric_dt=0.01, state_to_observation_func=None, reward_function=None,
              reset_func=None, reset_control_value=0.0, update_control_value=None, update_control_parameter=None,
              action_space_config={}, static_equation_parameters=dict(k=1.0, e=0.0), control_equation_parameter_name="omega",
              solver_parameters={})


def test_unknown_gpe_rewards_are_refused(no_engine):
    for reward in (("gpe", "nonsense"), ("gpe",), ("observables", "l_z")):
        with pytest.raises(ValueError, match="unknown device reward"):
            P.VectorPDEEnv(2, P.GPE2DTSRot, DOM, P.RotatingStrangSplitting, device_reward=reward, **ENV_KW)
    with pytest.raises(NotImplementedError):
        P.VectorPDEEnv(2, P.CahnHilliard2DPeriodic, DOM, P.RK4, device_reward=("gpe", "energy"), **ENV_KW)


# ---- ground_state's loop on a stub engine --------------------------------------------------------------------------------

class ScriptedEngine:
    """the engine calls ``ground_state`` makes; ``gpe_observables`` returns norm 1 and e_pot = the next row of a scripted
    energy table (so energy = mu = that number)"""

    def __init__(self, energies):
        self.energies = np.asarray(energies, dtype=float)  # (checks, B)
        self.advances, self.checks = [], 0

    def configure(self, **kw):
        self.batch = kw["batch"]

    def set_gpe_spots(self, *a, **k): pass
    def set_aux(self, *a, **k): pass
    def set_env_gpe_k(self, *a, **k): pass
    def set_env_gpe_omega(self, *a, **k): pass
    def set_gpe_rotation(self, *a, **k): pass

    def set_integrator_params(self, **kw):
        self.time_scale = kw["time_scale"]

    def set_state(self, y):
        self.y = np.array(y)

    def get_state(self):
        return self.y.copy()

    def advance(self, integrator, dt, n, t0=0.0):
        self.advances.append((integrator, dt, n))

    def gpe_observables(self, t=0.0, env_first=0, env_count=None):
        raw = np.zeros((self.batch, 8))
        raw[:, L.GPE_OBS_NORM] = 1.0
        raw[:, L.GPE_OBS_E_POT] = self.energies[self.checks]
        self.checks += 1
        return raw


def run(energies, **kw):
    m = P.PDEModel(P.GPE2DTSRot, DOM, P.RotatingStrangSplitting)
    m._engine = eng = ScriptedEngine(energies)
    B = eng.energies.shape[1]
    params = [dict(k=1.0, e=0.0, omega=0.1 * b) for b in range(B)]
    return m.ground_state(params, np.ones((B, 64, 64, 2)), 0.1, **kw), eng


def test_ground_state_stops_when_every_environment_stands_still():
    # check_every dt = 1: the criterion is |dE| <= tol = 0.05.  Environment 0 meets it at check 3, environment 1 at 5
    table = [[9.0, 9.0], [5.0, 7.0], [4.96, 6.0], [4.959, 5.5], [4.959, 5.47], [0.0, 0.0]]
    gs, eng = run(table, tol=0.05, check_every=10, max_steps=1000)
    assert gs.converged.tolist() == [True, True]
    assert gs.steps.tolist() == [30, 50] and gs.steps.dtype.kind == "i"
    assert eng.checks == 5 and eng.advances == [(L.INT_STRANG_ROT, 0.1, 10)] * 5
    assert eng.time_scale == -1j
    assert gs.history.shape == (5, 2, 2)
    np.testing.assert_array_equal(gs.history[:, :, 0], np.asarray(table[:5]))
    np.testing.assert_array_equal(gs.observables.energy, [4.959, 5.47])
    assert gs.state.shape == (2, 64, 64, 2)


def test_ground_state_reports_the_environments_that_never_arrive():
    table = [[9.0, 9.0], [5.0, 9.0 - 1e-3], [4.0, 9.0 - 2e-3], [3.0, 8.0]]
    gs, eng = run(table, tol=0.01, check_every=10, max_steps=35)
    assert gs.converged.tolist() == [False, True]
    assert gs.steps.tolist() == [35, 20]
    assert [a[2] for a in eng.advances] == [10, 10, 10, 5]  # the last block is clipped to max_steps
    assert gs.history.shape == (4, 2, 2)


def test_a_single_state_comes_back_single():
    m = P.PDEModel(P.GPE2DTSRot, DOM, P.RotatingStrangSplitting)
    m._engine = ScriptedEngine([[2.0], [1.0], [1.0]])
    gs = m.ground_state(dict(k=1.0, e=0.0, omega=0.0), np.ones((64, 64, 2)), 0.1, tol=1e-8, check_every=2)
    assert gs.state.shape == (64, 64, 2) and gs.steps.tolist() == [6] and gs.converged.tolist() == [True]
