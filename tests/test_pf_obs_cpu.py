"""Phase-field observables, the part that needs no GPU: the numpy reference (tests/pf_obs_ref.py) against the two
identities it must satisfy and against the committed right-hand-side goldens, the antiderivatives, the C ABI's
declaration and binding, and every refusal -- raised before an engine exists."""
import os
import re

import numpy as np
import pytest

import pde_opt_amd as P
import pf_obs_ref as R
from pde_opt_amd import _lib as L
from pde_opt_amd import phase_field_observables as PFO
from pde_opt_amd.numerics import closures as CLS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS64 = np.finfo(np.float64).eps

MUS = {
    "poly": R.Closure("poly", (0.1, -1.0, 0.2, 1.0)),
    "legendre": R.Closure("legendre", (0.2, -0.8, 0.3, 0.5, -0.2)),
    "logit": R.Closure("poly", (3.0, -6.0), logit=True),
}
MOB = R.Closure("poly", (0.2, 1.0, -1.0))


def spec_for(eq, mu):
    h = (0.11, 0.07, 0.13)[: 3 if eq == "ch3d" else 2]
    return dict(eq=eq, h=h, kappa=0.004, mu=MUS[mu], mob=MOB)


def state_for(eq, seed=3):
    shape = (6, 5, 4) if eq == "ch3d" else (12, 10)
    return np.random.default_rng(seed).uniform(0.1, 0.9, shape)


CASES = [(eq, mu) for eq in ("ch", "ac", "ch3d") for mu in MUS]


@pytest.mark.parametrize("eq,mu", CASES)
def test_the_free_energy_gradient_is_h_mu(eq, mu):
    """central differences of F over single cells give h mu.  F is quadratic in u except for f_h, so the difference
    leaves eps^2 / 6 x h max|f_h'''| = eps^2 / 6 x h max|mu_h''|; forming it costs 2 eps64 x (h sum |term|) / (2 eps)
    of rounding in each F, doubled for the two of them and for the summation"""
    spec, u = spec_for(eq, mu), state_for(eq)
    h, eps = float(np.prod(spec["h"])), 1e-4
    want = h * R.chem_pot(u, spec)
    _, scale = R.observables(u, spec)
    tol = eps**2 / 6 * h * R.second_derivative_bound(spec["mu"], 0.1 - eps, 0.9 + eps) + 4 * EPS64 * (scale[2] + scale[3]) / eps
    worst = 0.0
    for idx in np.ndindex(u.shape):
        up, um = u.copy(), u.copy()
        up[idx] += eps
        um[idx] -= eps
        worst = max(worst, abs((R.free_energy(up, spec) - R.free_energy(um, spec)) / (2 * eps) - want[idx]))
    assert worst <= tol, (worst, tol)
    assert tol <= 1e-5 * np.abs(want).max()  # the check resolves h mu


@pytest.mark.parametrize("eq,mu", CASES)
def test_the_free_energy_decays_at_the_dissipation_rate(eq, mu):
    """(F(u + eps f) - F(u - eps f)) / 2 eps = -DISS with f = rhs_fd(u): exact by summation by parts up to the third
    derivative along f, eps^2 / 6 x h max|mu_h''| sum |f|^3, and the rounding of the two F as above"""
    spec, u = spec_for(eq, mu), state_for(eq)
    f = R.rhs_fd(u, spec)
    h, eps = float(np.prod(spec["h"])), 1e-5 / np.abs(f).max()
    assert np.all(u + eps * f > 0.09) and np.all(u + eps * f < 0.91)
    v, scale = R.observables(u, spec)
    got = (R.free_energy(u + eps * f, spec) - R.free_energy(u - eps * f, spec)) / (2 * eps)
    tol = (eps**2 / 6 * h * R.second_derivative_bound(spec["mu"], 0.09, 0.91) * np.sum(np.abs(f) ** 3)
           + 4 * EPS64 * (scale[2] + scale[3]) / eps)
    assert abs(got + v[6]) <= tol, (got, v[6], tol)
    assert v[6] > 0 and tol <= 1e-6 * v[6]


GOLD_MU = {"cubic": R.Closure("poly", (0.0, -1.0, 0.0, 1.0)), "regsol": R.Closure("poly", (3.0, -6.0), logit=True)}
GOLD_MOB = {"one": R.Closure("poly", (1.0,)), "c1mc": R.Closure("poly", (0.0, 1.0, -1.0)),
            "one_plus_sq": R.Closure("poly", (1.0, 0.0, 1.0)), "const015": R.Closure("poly", (0.15,))}


def _rhs_tolerance(u, spec):
    """the reference evaluates closures by Horner, the goldens' source term by term: mu differs by a few ulp of its
    largest term, dmu = 16 eps64 (max|mu| + kappa sum 4 / h^2 max|u|).  Allen-Cahn: max R x dmu.  Cahn-Hilliard: every
    face difference carries twice dmu, times D / h^2 per axis, two faces each"""
    m, d = R.chem_pot(u, spec), R.evaluate(spec["mob"], u)
    lapscale = sum(4.0 / (hh * hh) for hh in spec["h"]) * spec["kappa"] * np.abs(u).max()
    dmu = 16 * EPS64 * (np.abs(m).max() + lapscale)
    if spec["eq"] == "ac":
        return dmu * np.abs(d).max()
    return 4 * dmu * np.abs(d).max() * sum(1.0 / (hh * hh) for hh in spec["h"])


def test_the_reference_right_hand_sides_match_the_goldens(golden):
    z = golden("rhs_cases.npz")
    keys = sorted(k[: -len("/rhs")] for k in z.files if k.endswith("float64/rhs") and k.split("/")[0] in ("ch_fd", "ac_fd"))
    assert len(keys) >= 8
    for key in keys:
        kind, mu, mob, tag = key.split("/")
        nx, ny = (int(v) for v in tag.split("_")[0].split("x"))
        spec = dict(eq=kind[:2], h=(0.01 * nx / nx, 0.01 * ny / ny), kappa=0.002, mu=GOLD_MU[mu], mob=GOLD_MOB[mob])
        u = z[key + "/u"]
        tol = _rhs_tolerance(u, spec)
        err = np.abs(R.rhs_fd(u, spec) - z[key + "/rhs"]).max()
        assert err <= tol, (key, err, tol)
        assert tol <= 1e-9 * np.abs(z[key + "/rhs"]).max(), key


def test_the_3d_reference_right_hand_side_matches_the_goldens(golden):
    z = golden("ch3d_cases.npz")
    tags = sorted(k[: -len("/rhs")] for k in z.files if k.endswith("float64/rhs"))
    assert len(tags) == 3
    for tag in tags:
        spec = dict(eq="ch3d", h=(0.01, 0.01, 0.012), kappa=0.002, mu=GOLD_MU["regsol"], mob=GOLD_MOB["c1mc"])
        u = z[tag + "/u"]
        err = np.abs(R.rhs_fd(u, spec) - z[tag + "/rhs"]).max()
        assert err <= _rhs_tolerance(u, spec), (tag, err)


def test_the_single_precision_variant_sums_in_fp64():
    spec, u = spec_for("ch", "logit"), state_for("ch")
    v64, s = R.observables(u.astype(np.float32), spec)
    v32, _ = R.observables(u.astype(np.float32), spec, np.float32)
    assert v32.dtype == np.float64 and v32[0] == v64[0]  # the same fp32 values, summed in fp64: the mass is exact
    for i in range(1, 7):
        assert 0 < abs(v32[i] - v64[i]) <= 1e-4 * s[i], R.NAMES[i]


# ---- antiderivatives ---------------------------------------------------------------------------------------------------

def test_the_legendre_antiderivative_is_legint_after_the_change_of_variable():
    """int_0^c sum a_k P_k(2c' - 1) dc' = 1/2 [legint(a)(x) - legint(a)(-1)], x = 2c - 1"""
    a = np.array([0.3, -1.2, 0.7, 0.25, -0.4, 0.1])
    c = np.linspace(0.0, 1.0, 41)
    integ = np.polynomial.legendre.legint(a)
    want = 0.5 * (np.polynomial.legendre.legval(2 * c - 1, integ) - np.polynomial.legendre.legval(-1.0, integ))
    desc = CLS.ClosureDesc(CLS.LEGENDRE, 0, tuple(a))
    np.testing.assert_allclose(PFO.antiderivative(desc, c), want, rtol=0, atol=1e-14)
    np.testing.assert_allclose(R.antiderivative(R.Closure("legendre", tuple(a)), c), want, rtol=0, atol=1e-14)


def test_antiderivatives_of_the_other_forms():
    c = np.linspace(0.0, 1.0, 11)
    np.testing.assert_allclose(PFO.antiderivative(P.polynomial(1.0, 2.0, 3.0), c), c + c**2 + c**3, atol=1e-15)
    got = PFO.antiderivative(P.polynomial(0.0, logit_prior=True), c)
    assert got[0] == 0.0 and got[-1] == 0.0  # c ln c + (1 - c) ln(1 - c) is taken as 0 at the ends
    np.testing.assert_allclose(got[1:-1], c[1:-1] * np.log(c[1:-1]) + (1 - c[1:-1]) * np.log(1 - c[1:-1]), atol=1e-15)
    # f_h' = mu_h: a central difference of the antiderivative gives the closure back
    for cl in MUS.values():
        x, e = np.linspace(0.1, 0.9, 17), 1e-5
        d = (R.antiderivative(cl, x + e) - R.antiderivative(cl, x - e)) / (2 * e)
        np.testing.assert_allclose(d, R.evaluate(cl, x), atol=e * e / 6 * 2e4 + 1e-10)
        np.testing.assert_allclose(PFO.antiderivative(cl.desc(), x), R.antiderivative(cl, x), atol=1e-15)


# ---- header, bindings, derived entries ---------------------------------------------------------------------------------------

def test_the_symbol_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "pdeopt_hip.h")).read()
    m = re.search(r"int pdeopt_pf_observables\(([^)]*)\)", header)
    assert m and len(m.group(1).split(",")) == 4
    assert re.search(r"PDEOPT_PF_OBS_COUNT\s*=\s*8\b", header) and L.PF_OBS_COUNT == 8
    for i, name in enumerate(PFO.RAW_NAMES):
        assert re.search(rf"PDEOPT_PF_OBS_{name.upper()}\s*=\s*{i}\b", header), name
        assert getattr(L, "PF_OBS_" + name.upper()) == i
    assert PFO.RAW_NAMES == R.NAMES
    assert hasattr(L.load_library(), "pdeopt_pf_observables")
    assert L.load_library().pdeopt_abi_version() == 1


def test_from_raw_derives_the_six_entries():
    raw = np.array([[2.0, 1.5, 0.25, 0.5, 3.0, 6.0, 0.7, 0.0], [4.0, 9.0, -1.0, 0.25, -2.0, 5.0, 0.1, 3.0]])
    o = P.PhaseFieldObservables.from_raw(raw, volume=4.0)
    np.testing.assert_array_equal(o.free_energy, [0.75, -0.75])
    np.testing.assert_array_equal(o.mean, [0.5, 1.0])
    np.testing.assert_array_equal(o.mu_mean, [0.75, -0.5])
    np.testing.assert_array_equal(o.mu_variance, [6.0 / 4 - 0.75**2, 5.0 / 4 - 0.25])
    np.testing.assert_array_equal(o.dissipation, raw[:, 6])
    np.testing.assert_array_equal(o["nonfinite"], [0.0, 3.0])
    assert len(PFO.REWARD_NAMES) == 13 and len(set(PFO.REWARD_NAMES)) == 13  # eight raw, six derived, nonfinite is both
    assert P.PhaseFieldObservables.from_raw(np.stack([raw, raw]), 4.0).free_energy.shape == (2, 2)
    with pytest.raises(ValueError):
        P.PhaseFieldObservables.from_raw(raw[:, :7], 4.0)
    with pytest.raises(KeyError):
        o["energy"]


# ---- refusals, before any engine exists -----------------------------------------------------------------------------------

@pytest.fixture
def no_engine(monkeypatch):
    import pde_opt_amd.engine as E

    def refuse(self, *a, **k):
        raise AssertionError("an engine was created")

    monkeypatch.setattr(E.HipEngine, "__init__", refuse)


DOM = P.Domain((16, 16), ((0.0, 1.0), (0.0, 1.0)), "dimensionless")
CUBIC = dict(kappa=0.1, mu=lambda c: c**3 - c, D=lambda c: 1.0)
U0 = np.full((16, 16), 0.5)


def test_unsupported_closures_and_derivs_are_refused(no_engine):
    m = P.PDEModel(P.CahnHilliard2DPeriodic, DOM, P.RK4)
    entropy = CLS.ClosureDesc(CLS.POLY, CLS.MIX_ENTROPY, (0.0, 1.0))
    wrapped = CLS.ClosureDesc(CLS.POLY, CLS.EXP_WRAP, (0.0, 1.0))
    for mu, word in ((entropy, "mixing entropy"), (wrapped, "exp"), (lambda c: np.tanh(c), "compiled at run time")):
        with pytest.raises(ValueError, match=word):
            m.free_energy({**CUBIC, "mu": mu}, U0)
        with pytest.raises(ValueError, match=word):
            m.free_energy_trace({**CUBIC, "mu": mu}, U0, [0.0, 1e-3], dt0=1e-4)
    with pytest.raises(ValueError, match="compiled at run time"):
        m.free_energy({**CUBIC, "D": lambda c: np.tanh(c)}, U0)
    with pytest.raises(ValueError, match="fourier"):
        m.free_energy({**CUBIC, "derivs": "fourier"}, U0)
    # D may be any closure of the family: an exp-wrapped mobility passes the checks
    PFO.check_equation(P.CahnHilliard2DPeriodic(domain=DOM, kappa=0.1, mu=CUBIC["mu"], D=wrapped))


def test_a_network_as_mu_is_refused(no_engine):
    torch = pytest.importorskip("torch")
    m = P.PDEModel(P.CahnHilliard2DPeriodic, DOM, P.Euler)
    with pytest.raises(ValueError, match="torch.nn.Module"):
        m.free_energy({**CUBIC, "mu": torch.nn.Identity()}, U0)


def test_other_equation_classes_are_refused(no_engine):
    pairs = ((P.CahnHilliard2DSmoothedBoundary, P.RK4), (P.AllenCahn2DSmoothedBoundary, P.RK4),
             (P.AllenCahn2DPeriodicButlerVolmer, P.RK4), (P.AllenCahn2DPeriodicButlerVolmerConstantCurrent, P.RK4),
             (P.AdvectionDiffusion2D, P.RK4), (P.GPE2DTSControl, P.StrangSplitting), (P.GPE2DTSRot, P.RotatingStrangSplitting))
    for eq, solver in pairs:
        m = P.PDEModel(eq, DOM, solver)
        with pytest.raises(NotImplementedError, match="no free energy"):
            m.free_energy({}, U0)
        with pytest.raises(NotImplementedError, match="no free energy"):
            m.free_energy_trace({}, U0, [0.0, 1.0])


def test_a_save_point_inside_a_step_is_refused(no_engine):
    m = P.PDEModel(P.CahnHilliard2DPeriodic, DOM, P.SemiImplicitFourierSpectral)
    with pytest.raises(ValueError, match="inside a step"):
        m.free_energy_trace(CUBIC, U0, [0.0, 2.5e-4, 1e-3], dt0=1e-4)
    with pytest.raises(NotImplementedError, match="Euler, RK4"):
        P.PDEModel(P.CahnHilliard2DPeriodic, DOM, P.Tsit5).free_energy_trace(CUBIC, U0, [0.0, 1e-3], dt0=1e-4)
    with pytest.raises(ValueError, match="closures' structure"):
        m.free_energy([CUBIC, {**CUBIC, "mu": lambda c: c - 0.5}], np.stack([U0, U0]))


ENV_KW = dict(end_time=1.0, step_dt=0.1, numeric_dt=0.01, state_to_observation_func=None, reward_function=None,
              reset_func=None, reset_control_value=0.0, update_control_value=None, update_control_parameter=None,
              action_space_config={}, solver_parameters={})


def test_unknown_phase_field_rewards_are_refused(no_engine):
    ch = dict(static_equation_parameters=dict(mu=CUBIC["mu"], D=CUBIC["D"]), control_equation_parameter_name="kappa")
    for reward in (("phase_field", "nonsense"), ("phase_field",), ("phase_field", "energy"), ("phase_field", "free_energy", 1)):
        with pytest.raises(ValueError, match="unknown device reward"):
            P.VectorPDEEnv(2, P.CahnHilliard2DPeriodic, DOM, P.RK4, device_reward=reward, **ch, **ENV_KW)
    gpe = dict(static_equation_parameters=dict(k=1.0, e=0.0), control_equation_parameter_name="omega")
    with pytest.raises(NotImplementedError, match="no free energy"):
        P.VectorPDEEnv(2, P.GPE2DTSRot, P.Domain((64, 64), ((-8.0, 8.0), (-8.0, 8.0)), "dimensionless"), P.RotatingStrangSplitting,
                       device_reward=("phase_field", "free_energy"), **gpe, **ENV_KW)
