"""The host path the device diagnostics share (pde_opt_amd.diagnostics) and the table of tuple device rewards: the batch of
states, the parameter sets, and every refusal with the exception type and the text it had before the three modules
shared this code -- no engine and no GPU needed."""
import numpy as np
import pytest

import pde_opt_amd as P
from pde_opt_amd import diagnostics as D
from pde_opt_amd import gpe_observables, phase_field_observables, structure_factor


def domain(points, lengths):
    return P.Domain(tuple(points), tuple((0.0, v) for v in lengths), "dimensionless")


@pytest.fixture(autouse=True)
def no_engine(monkeypatch):
    import pde_opt_amd.engine as E

    def refuse(self, *a, **k):
        raise AssertionError("an engine was created")

    monkeypatch.setattr(E.HipEngine, "__init__", refuse)


DOM = domain((16, 12), (1.0, 1.0))
GDOM = P.Domain((64, 64), ((-8.0, 8.0), (-8.0, 8.0)), "dimensionless")
MODEL = P.PDEModel(P.CahnHilliard2DPeriodic, DOM, P.SemiImplicitFourierSpectral)
CUBIC = dict(kappa=0.1, mu=lambda c: c**3 - c, D=lambda c: 1.0)
U0 = np.full((16, 12), 0.5)


# ---- batch_states -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("trailing", [(), (2,)])
def test_a_single_state_and_a_batch(trailing):
    one = np.arange(16 * 12 * int(np.prod(trailing, dtype=int)), dtype=np.float32).reshape((16, 12) + trailing)
    yb, single = D.batch_states(MODEL, one, trailing=trailing)
    assert single and yb.shape == (1, 16, 12) + trailing and yb.dtype == np.float32 and np.array_equal(yb[0], one)
    many = np.stack([one, 2 * one, 3 * one]).astype(np.float64)
    yb, single = D.batch_states(MODEL, many, trailing=trailing)
    assert not single and yb is many  # fp32 and fp64 pass through as they are


def test_other_dtypes_are_widened_to_fp64():
    half = np.linspace(0.0, 1.0, 16 * 12).reshape(16, 12).astype(np.float16)
    yb, single = D.batch_states(MODEL, half)
    assert single and yb.dtype == np.float64 and np.array_equal(yb[0], half.astype(np.float64))
    yb, _ = D.batch_states(MODEL, np.ones((2, 16, 12), dtype=np.int32))
    assert yb.dtype == np.float64 and yb.shape == (2, 16, 12)


def test_contiguous_is_a_request():
    strided = np.zeros((2, 16, 24))[:, :, ::2]
    assert not D.batch_states(MODEL, strided)[0].flags.c_contiguous
    yb, _ = D.batch_states(MODEL, strided, contiguous=True)
    assert yb.flags.c_contiguous and yb.shape == (2, 16, 12)


def test_a_wrong_shape_is_refused():
    cases = ((np.zeros((16, 11)), (), "state of shape (16, 11): expected (16, 12) or (B,) + that"),
             (np.zeros((2, 3, 16, 12)), (), "state of shape (2, 3, 16, 12): expected (16, 12) or (B,) + that"),
             (np.zeros(16), (), "state of shape (16,): expected (16, 12) or (B,) + that"),
             (np.zeros((16, 12)), (2,), "state of shape (16, 12): expected (16, 12, 2) or (B,) + that"),
             (np.zeros((16, 11, 2)), (2,), "state of shape (16, 11, 2): expected (16, 12, 2) or (B,) + that"))
    for bad, trailing, text in cases:
        with pytest.raises(ValueError) as e:
            D.batch_states(MODEL, bad, trailing=trailing)
        assert str(e.value) == text


def test_a_complex_state_with_and_without_a_message():
    for text in ("complex states are stored as (..., 2) real/imag pairs",
                 "the structure factor is that of a real field, got a complex state"):
        with pytest.raises(ValueError) as e:
            D.batch_states(MODEL, U0 + 0j, complex_message=text)
        assert str(e.value) == text
    # the callers' sentences, through the callers
    with pytest.raises(ValueError) as e:
        P.PDEModel(P.GPE2DTSRot, GDOM, P.RotatingStrangSplitting).observables({}, np.zeros((64, 64), dtype=complex))
    assert str(e.value) == "complex states are stored as (..., 2) real/imag pairs"
    with pytest.raises(ValueError) as e:
        MODEL.structure_factor(U0 + 0j)
    assert str(e.value) == "the structure factor is that of a real field, got a complex state"
    # without one (the phase field's free energy) the array is converted like any other dtype: numpy drops the
    # imaginary part and warns
    with pytest.warns(np.exceptions.ComplexWarning if hasattr(np, "exceptions") else np.ComplexWarning):
        yb, single = D.batch_states(MODEL, U0 + 1j)
    assert single and yb.dtype == np.float64 and np.array_equal(yb[0], U0)


# ---- parameter_sets ----------------------------------------------------------------------------------------------------

def test_parameter_sets_one_dict_or_one_per_state():
    p = dict(kappa=1.0)
    assert D.parameter_sets(p, 3) == [p] and D.parameter_sets(p, 3)[0] is p
    assert D.parameter_sets([p], 3) == [p]
    three = (dict(kappa=1.0), dict(kappa=2.0), dict(kappa=3.0))
    assert D.parameter_sets(three, 3) == list(three)
    for n in (2, 4):
        with pytest.raises(ValueError) as e:
            D.parameter_sets([p] * n, 3)
        assert str(e.value) == f"{n} parameter sets for 3 states: one dict, or one per state"
    with pytest.raises(ValueError) as e:
        MODEL.free_energy([CUBIC, CUBIC], np.stack([U0, U0, U0]))
    assert str(e.value) == "2 parameter sets for 3 states: one dict, or one per state"


# ---- the table of tuple device rewards -----------------------------------------------------------------------------

ENV_KW = dict(end_time=1.0, step_dt=0.1, numeric_dt=0.01, state_to_observation_func=None, reward_function=None,
              reset_func=None, reset_control_value=0.0, update_control_value=None, update_control_parameter=None,
              action_space_config={}, solver_parameters={})
CH_ENV = (P.CahnHilliard2DPeriodic, DOM, P.RK4,
          dict(static_equation_parameters=dict(mu=CUBIC["mu"], D=CUBIC["D"]), control_equation_parameter_name="kappa"))
GPE_ENV = (P.GPE2DTSRot, GDOM, P.RotatingStrangSplitting,
           dict(static_equation_parameters=dict(k=1.0, e=0.0), control_equation_parameter_name="omega"))

GPE_TAKES = ("(\"gpe\" takes one of ('norm', 'e_kin', 'e_pot', 'e_int', 'l_z', 'x2', 'y2', 'energy', 'mu'))")
PF_TAKES = ("(\"phase_field\" takes one of ('mass', 'u2', 'f_bulk', 'f_grad', 'mu', 'mu2', 'diss', 'nonfinite', 'free_energy', "
            "'mean', 'mu_mean', 'mu_variance', 'dissipation'))")
SK_TAKES = "(\"structure_factor\" takes one of ('length', 'k1', 'k2', 'variance'))"
GPE_CLASS = ("energy, chemical potential and L_z are observables of GPE2DTSControl and GPE2DTSRot; CahnHilliard2DPeriodic has "
             "none")
PF_CLASS = ('GPE2DTSRot has no free energy here: the free energy is summed for CahnHilliard2DPeriodic, AllenCahn2DPeriodic and '
            'CahnHilliard3DPeriodic with derivs="fd" and a mu that is a polynomial or a Legendre series, with or without the '
            'log(c / (1 - c)) prior (the smoothed-boundary, Butler-Volmer, advection-diffusion and GPE classes are not covered)')
SK_CLASS = ("GPE2DTSRot has no structure factor here: the structure factor is that of the real periodic phase-field classes "
            "CahnHilliard2DPeriodic, AllenCahn2DPeriodic and CahnHilliard3DPeriodic (the smoothed-boundary, Butler-Volmer, "
            "advection-diffusion and GPE classes are not covered)")


def make_env(setup, reward):
    eq, dom, solver, kw = setup
    return P.VectorPDEEnv(2, eq, dom, solver, device_reward=reward, **kw, **ENV_KW)


@pytest.mark.parametrize("kind,name,own,other,takes,refusal", [
    ("gpe", "energy", GPE_ENV, CH_ENV, GPE_TAKES, GPE_CLASS),
    ("phase_field", "free_energy", CH_ENV, GPE_ENV, PF_TAKES, PF_CLASS),
    ("structure_factor", "length", CH_ENV, GPE_ENV, SK_TAKES, SK_CLASS)])
def test_a_reward_kind_refuses_names_lengths_and_classes(kind, name, own, other, takes, refusal):
    for reward in ((kind, "nonsense"), (kind,), (kind, name, 1)):
        with pytest.raises(ValueError) as e:
            make_env(own, reward)
        assert str(e.value) == f"unknown device reward {reward!r} {takes}"
    with pytest.raises(NotImplementedError) as e:
        make_env(other, (kind, name))
    assert str(e.value) == refusal


def test_the_table_and_what_stays_outside_it():
    from pde_opt_amd.pde_env import _TUPLE_REWARDS

    assert set(_TUPLE_REWARDS) == {"gpe", "phase_field", "structure_factor"}
    assert _TUPLE_REWARDS["gpe"].names == gpe_observables.OBSERVABLE_NAMES + gpe_observables.DERIVED_NAMES
    assert _TUPLE_REWARDS["phase_field"].names == phase_field_observables.REWARD_NAMES
    assert _TUPLE_REWARDS["structure_factor"].names == structure_factor.REWARD_NAMES
    assert _TUPLE_REWARDS["phase_field"].precheck is phase_field_observables.check_equation
    assert _TUPLE_REWARDS["gpe"].precheck is None and _TUPLE_REWARDS["structure_factor"].precheck is None
    with pytest.raises(ValueError) as e:
        make_env(CH_ENV, ("nonsense", 1))
    assert str(e.value) == "unknown device reward 'nonsense'"


# ---- trace_on_step_edges, through its two callers -------------------------------------------------------------------

INSIDE = ("save point ts[1] = np.float64(0.00025) lies inside a step of dt0 = 0.0001 (at 0.5 of it): {}; put ts on step edges "
          "(ts[0] + k dt0, and ts[-1])")
TRACES = [("free_energy_trace", "the energy of a linear interpolation of states is not an interpolation of energies"),
          ("structure_factor_trace", "the spectrum of a linear interpolation of states is not the state's at that time")]


@pytest.mark.parametrize("name,why", TRACES)
def test_a_trace_refuses_before_an_engine_exists(name, why):
    with pytest.raises(ValueError) as e:
        getattr(MODEL, name)(CUBIC, U0, [0.0, 2.5e-4, 1e-3], dt0=1e-4)
    assert str(e.value) == INSIDE.format(why).replace("np.float64(0.00025)", repr(np.float64(2.5e-4)))
    with pytest.raises(NotImplementedError) as e:
        getattr(P.PDEModel(P.CahnHilliard2DPeriodic, DOM, P.Tsit5), name)(CUBIC, U0, [0.0, 1e-3], dt0=1e-4)
    assert str(e.value) == f"{name} steps with Euler, RK4 or SemiImplicitFourierSpectral (constant steps), not Tsit5"
    with pytest.raises(ValueError) as e:
        getattr(MODEL, name)([CUBIC, CUBIC], np.stack([U0, U0]), [0.0, 1e-3], dt0=1e-4)
    assert str(e.value) == f"{name} runs the solve of PDEModel.solve: one parameter dict for the batch"
    for ts in ([], [[0.0, 1e-3]]):
        with pytest.raises(ValueError) as e:
            getattr(MODEL, name)(CUBIC, U0, ts, dt0=1e-4)
        assert str(e.value) == "ts is a non-empty 1-D sequence of save times"


def test_each_trace_keeps_the_order_of_its_refusals():
    spectral = dict(CUBIC, derivs="fourier")
    # the free energy checks the equation before it looks at ts; S(k) takes any derivs and never builds it that early
    with pytest.raises(ValueError, match="finite-difference right-hand side"):
        MODEL.free_energy_trace(spectral, U0, [], dt0=1e-4)
    with pytest.raises(ValueError, match="non-empty 1-D"):
        MODEL.structure_factor_trace(spectral, U0, [], dt0=1e-4)
    # a parameter set no equation can be built from: S(k) refuses the save point first, the free energy the parameters
    with pytest.raises(ValueError, match="inside a step"):
        MODEL.structure_factor_trace(dict(nonsense=1), U0, [0.0, 2.5e-4, 1e-3], dt0=1e-4)
    with pytest.raises(TypeError):
        MODEL.free_energy_trace(dict(nonsense=1), U0, [0.0, 2.5e-4, 1e-3], dt0=1e-4)
