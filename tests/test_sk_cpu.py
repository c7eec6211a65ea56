"""The structure factor's definition on the numpy reference (tests/sk_ref.py), the host-side derivations of
pde_opt_amd.structure_factor and every Python refusal -- no GPU needed."""
import os
import re

import numpy as np
import pytest

import pde_opt_amd as P
import sk_ref as R
from pde_opt_amd import _lib as L
from pde_opt_amd import structure_factor as SK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def domain(points, lengths):
    return P.Domain(tuple(points), tuple((0.0, v) for v in lengths), "dimensionless")


# ---- the definition --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("points,lengths", R.GRIDS)
def test_half_spectrum_sums_equal_full_spectrum_sums(points, lengths):
    u = R.white_noise(points, 2, seed=sum(points))
    p, counts, _ = R.power(u, lengths)
    pf, counts_f = R.power_full(u, lengths)
    # two roundings per |u^|^2 and a sum of at most N terms either way: 1e-13 relative leaves two digits over N 2^-53
    assert np.all(np.abs(p - pf) <= 1e-13 * pf.max())
    assert np.array_equal(counts, counts_f)  # sums of 1 and 2: exact
    assert counts.sum() == np.prod(points) - 1
    assert counts[0] == 0 and np.all(counts[1:] > 0)  # shell 0 holds the zero mode alone; no other shell is empty here
    b, _, n_bins, _ = R.half_bins(points, lengths)
    assert b.max() < n_bins
    assert np.all(np.diff(b, axis=-1) >= 0)  # what the kernel's scan relies on: sorted shells along a row


@pytest.mark.parametrize("points,lengths", R.GRIDS)
def test_parseval(points, lengths):
    u = R.white_noise(points, 2, seed=1 + sum(points))
    p, counts, dk = R.power(u, lengths)
    d = R.derived(p, counts, int(np.prod(points)), dk)
    var = u.reshape(2, -1).var(axis=1)
    np.testing.assert_allclose(d["variance"], var, rtol=1e-13)


def test_a_plane_wave_sits_in_one_shell():
    u = R.plane_wave()
    p, counts, dk = R.power(u[None], (1.0, 1.0))
    peak = u.size**2 * 0.02
    assert abs(p[0, 5] - peak) <= 1e-12 * peak
    others = np.delete(p[0], 5)
    assert np.all(others < 1e-20 * peak)
    d = R.derived(p, counts, u.size, dk)
    np.testing.assert_allclose(d["length"], 1.0 / 5.0, rtol=1e-12)  # the wave length of (3, 4): 2 pi / (5 * 2 pi)


# ---- the module's tables and derived quantities --------------------------------------------------------------------

@pytest.mark.parametrize("points,lengths", R.GRIDS)
def test_shell_tables_are_the_reference_tables(points, lengths):
    tabs = SK.shell_tables(domain(points, lengths))
    ref_tabs, dk = R.tables(points, lengths)
    assert len(tabs.tables) == len(points) and all(np.array_equal(a, b) for a, b in zip(tabs.tables, ref_tabs))
    _, counts, _ = R.power(np.zeros((1,) + tuple(points)), lengths)
    assert tabs.n_bins == R.n_bins_of(ref_tabs) and tabs.dk == dk and tabs.n == np.prod(points)
    assert np.array_equal(tabs.counts, counts) and np.array_equal(tabs.k, np.arange(tabs.n_bins) * dk)
    assert SK.shell_tables(domain(points, lengths)) is tabs  # kept per grid


def test_derived_quantities_of_a_hand_written_spectrum():
    k = np.array([0.0, 2.0, 4.0, 6.0])
    counts = np.array([0.0, 4.0, 8.0, 3.0])
    n = 16
    power = np.array([[0.0, 64.0, 128.0, 0.0], [0.0, 0.0, 256.0, 96.0]])
    sf = P.StructureFactor.from_power(power, k, counts, n, dk=2.0)
    np.testing.assert_array_equal(sf.s, [[0.0, 1.0, 1.0, 0.0], [0.0, 0.0, 2.0, 2.0]])
    np.testing.assert_array_equal(sf.variance, [192.0 / 256.0, 352.0 / 256.0])
    np.testing.assert_array_equal(sf.k1, [3.0, 5.0])
    np.testing.assert_array_equal(sf.k2, [np.sqrt(10.0), np.sqrt(26.0)])
    np.testing.assert_array_equal(sf.length, [2.0 * np.pi / 3.0, 2.0 * np.pi / 5.0])
    assert sf.dk == 2.0 and sf["length"] is sf.length and SK.REWARD_NAMES == ("length", "k1", "k2", "variance")
    assert P.StructureFactor.from_power(np.stack([power, power, power]), k, counts, n, 2.0).length.shape == (3, 2)
    with pytest.raises(ValueError):
        P.StructureFactor.from_power(power[:, :3], k, counts, n, 2.0)
    with pytest.raises(KeyError):
        sf["power"]
    d = R.derived(power, counts, n, 2.0)
    for name in ("s", "variance", "k1", "k2", "length"):
        np.testing.assert_array_equal(getattr(sf, name), d[name])


def test_the_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "pdeopt_hip.h")).read()
    m = re.search(r"int pdeopt_sk_configure\(([^)]*)\)", header)
    assert m and len(m.group(1).split(",")) == 5
    m = re.search(r"int pdeopt_structure_factor\(([^)]*)\)", header)
    assert m and len(m.group(1).split(",")) == 4
    lib = L.load_library()
    assert hasattr(lib, "pdeopt_sk_configure") and hasattr(lib, "pdeopt_structure_factor")
    assert lib.pdeopt_abi_version() == 1


# ---- refusals, before any engine exists -----------------------------------------------------------------------------

@pytest.fixture
def no_engine(monkeypatch):
    import pde_opt_amd.engine as E

    def refuse(self, *a, **k):
        raise AssertionError("an engine was created")

    monkeypatch.setattr(E.HipEngine, "__init__", refuse)


DOM = domain((16, 16), (1.0, 1.0))
CUBIC = dict(kappa=0.1, mu=lambda c: c**3 - c, D=lambda c: 1.0)
U0 = np.full((16, 16), 0.5)


def test_other_equation_classes_are_refused(no_engine):
    pairs = ((P.CahnHilliard2DSmoothedBoundary, P.RK4), (P.AllenCahn2DSmoothedBoundary, P.RK4),
             (P.AllenCahn2DPeriodicButlerVolmer, P.RK4), (P.AllenCahn2DPeriodicButlerVolmerConstantCurrent, P.RK4),
             (P.AdvectionDiffusion2D, P.RK4), (P.GPE2DTSControl, P.StrangSplitting), (P.GPE2DTSRot, P.RotatingStrangSplitting))
    for eq, solver in pairs:
        m = P.PDEModel(eq, DOM, solver)
        with pytest.raises(NotImplementedError, match="no structure factor"):
            m.structure_factor(U0)
        with pytest.raises(NotImplementedError, match="no structure factor"):
            m.structure_factor_trace({}, U0, [0.0, 1.0])


def test_complex_states_and_wrong_shapes_are_refused(no_engine):
    m = P.PDEModel(P.CahnHilliard2DPeriodic, DOM, P.RK4)
    with pytest.raises(ValueError, match="complex"):
        m.structure_factor(U0 + 0j)
    with pytest.raises(ValueError, match="complex"):
        m.structure_factor_trace(CUBIC, U0.astype(np.complex64), [0.0, 1e-3], dt0=1e-4)
    for bad in (np.zeros((16, 15)), np.zeros((2, 3, 16, 16)), np.zeros(16)):
        with pytest.raises(ValueError, match="expected"):
            m.structure_factor(bad)
    with pytest.raises(ValueError, match="expected"):
        P.PDEModel(P.CahnHilliard3DPeriodic, domain((8, 8, 8), (1.0, 1.0, 1.0)), P.Euler).structure_factor(U0)


def test_a_save_point_inside_a_step_is_refused(no_engine):
    m = P.PDEModel(P.CahnHilliard2DPeriodic, DOM, P.SemiImplicitFourierSpectral)
    with pytest.raises(ValueError, match="inside a step"):
        m.structure_factor_trace(CUBIC, U0, [0.0, 2.5e-4, 1e-3], dt0=1e-4)
    with pytest.raises(NotImplementedError, match="Euler, RK4"):
        P.PDEModel(P.CahnHilliard2DPeriodic, DOM, P.Tsit5).structure_factor_trace(CUBIC, U0, [0.0, 1e-3], dt0=1e-4)
    with pytest.raises(ValueError, match="one parameter dict"):
        m.structure_factor_trace([CUBIC, CUBIC], np.stack([U0, U0]), [0.0, 1e-3], dt0=1e-4)


def test_too_many_shells_are_refused(no_engine):
    m = P.PDEModel(P.CahnHilliard2DPeriodic, domain((6000, 6000), (1.0, 1.0)), P.RK4)
    with pytest.raises(ValueError, match="at most 4096"):
        m.structure_factor(np.zeros((1, 1)))  # (the grid is looked at before the state)


ENV_KW = dict(end_time=1.0, step_dt=0.1, numeric_dt=0.01, state_to_observation_func=None, reward_function=None,
              reset_func=None, reset_control_value=0.0, update_control_value=None, update_control_parameter=None,
              action_space_config={}, solver_parameters={})


def test_unknown_structure_factor_rewards_are_refused(no_engine):
    ch = dict(static_equation_parameters=dict(mu=CUBIC["mu"], D=CUBIC["D"]), control_equation_parameter_name="kappa")
    for reward in (("structure_factor", "nonsense"), ("structure_factor",), ("structure_factor", "s"), ("structure_factor", "length", 1)):
        with pytest.raises(ValueError, match="unknown device reward"):
            P.VectorPDEEnv(2, P.CahnHilliard2DPeriodic, DOM, P.RK4, device_reward=reward, **ch, **ENV_KW)
    gpe = dict(static_equation_parameters=dict(k=1.0, e=0.0), control_equation_parameter_name="omega")
    with pytest.raises(NotImplementedError, match="no structure factor"):
        P.VectorPDEEnv(2, P.GPE2DTSRot, P.Domain((64, 64), ((-8.0, 8.0), (-8.0, 8.0)), "dimensionless"), P.RotatingStrangSplitting,
                       device_reward=("structure_factor", "length"), **gpe, **ENV_KW)
