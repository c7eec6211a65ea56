"""Butler-Volmer Allen-Cahn without a GPU: the reference's own invariants (tests/bv_ref.py), the SQRT_WRAP closure and
the class surface of the three equations."""
import dataclasses
import types

import numpy as np
import pytest

import bv_ref as R
import pde_opt_amd as P
from pde_opt_amd.numerics import closures as CL
from util import std_domain

KAPPA = 0.002


def _cases():
    rng = np.random.default_rng(3)
    h = 0.01
    yield "periodic", R.notebook_state(rng, (16, 12)), h, h, None
    yield "disc", R.notebook_state(rng, (24, 24)), h, h, R.disc_psi(24, 24)


CASES = list(_cases())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("C", [0.02, 0.0, -0.01])
def test_total_rate_is_the_current_for_alpha_one_half(case, C):
    _, u, hx, hy, psi = case
    k = R.rhs_current(u, hx, hy, KAPPA, 0.5, C, psi=psi)
    scale = R.current_scale(u, hx, hy, KAPPA, C, psi=psi)
    assert abs(R.total_rate(k, hx, hy, psi) - C) <= 1e-12 * scale


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_get_voltage_is_the_v_inside_rhs(case):
    _, u, hx, hy, psi = case
    for alpha, C in ((0.5, 0.02), (0.3, -0.01)):
        v = R.voltage(u, hx, hy, KAPPA, C, psi=psi)
        want = R.rate(u, R.mu_of(u, hx, hy, KAPPA, psi=psi), v, alpha)
        assert np.array_equal(R.rhs_current(u, hx, hy, KAPPA, alpha, C, psi=psi), want)
    if psi is None:  # the fixed-voltage class at that v is the constant-current class
        assert np.array_equal(R.rhs_voltage(u, hx, hy, KAPPA, 0.3, v), want)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_zero_current_has_zero_total_rate(case):
    _, u, hx, hy, psi = case
    k = R.rhs_current(u, hx, hy, KAPPA, 0.5, 0.0, psi=psi)
    assert abs(R.total_rate(k, hx, hy, psi)) <= 1e-12 * R.current_scale(u, hx, hy, KAPPA, 0.0, psi=psi)


# ---- the SQRT_WRAP closure ---------------------------------------------------------------------------------------------
def test_sqrt_of_a_polynomial_becomes_sqrt_wrap():
    d = CL.as_closure(lambda c: np.sqrt((1 - c) * c), sqrt_wrap=True)
    assert (d.kind, d.flags, d.coef) == (CL.POLY, CL.SQRT_WRAP, (0.0, 1.0, -1.0))
    c = np.linspace(0.05, 0.95, 7)
    assert np.allclose(d(c), np.sqrt((1 - c) * c), rtol=1e-15)
    d2 = CL.as_closure(lambda c: 2.0 * np.sqrt(1 + c**2), sqrt_wrap=True)  # a positive factor moves under the root
    assert d2.flags == CL.SQRT_WRAP and d2.coef == (4.0, 0.0, 4.0)
    assert CL.as_closure(R.MU, sqrt_wrap=True).flags == CL.LOGIT_PRIOR  # the notebook's mu stays polynomial + logit


def test_the_default_tracer_does_not_hand_out_sqrt_wrap():
    """every other equation traces without the flag: sqrt(polynomial) stays a run-time-compiled closure there"""
    assert CL.as_closure(lambda c: np.sqrt((1 - c) * c)).kind == CL.JIT


def test_sqrt_times_exp_stays_unsupported():
    fn = lambda c: np.sqrt(c) * np.exp(c)  # noqa: E731
    assert not CL.as_closure(fn, sqrt_wrap=True).flags & CL.SQRT_WRAP
    dom = std_domain(P, 8, 8)
    with pytest.raises(P.UnsupportedClosureError):
        P.AllenCahn2DPeriodicButlerVolmerConstantCurrent(dom, KAPPA, R.MU, fn, 0.5, 0.02)


def test_sqrt_wrap_is_the_exchange_currents_alone():
    """the kernels evaluate mu_h without the flag: a square root as mu is refused, traced or handed over as a descriptor"""
    dom = std_domain(P, 8, 8)
    desc = CL.ClosureDesc(CL.POLY, CL.SQRT_WRAP, (1.0, 1.0))
    for mu in (lambda c: np.sqrt(1.0 + c), desc):
        with pytest.raises(P.UnsupportedClosureError):
            P.AllenCahn2DPeriodicButlerVolmerConstantCurrent(dom, KAPPA, mu, R.J0, 0.5, 0.02)
        with pytest.raises(P.UnsupportedClosureError):
            P.AllenCahn2DPeriodicButlerVolmer(dom, KAPPA, mu, R.J0, 0.5)
    assert P.AllenCahn2DPeriodicButlerVolmer(dom, KAPPA, R.MU, desc, 0.5)._mob_desc is desc  # as j0 it is taken


def test_sqrt_wrap_on_another_equation_raises():
    dom = std_domain(P, 8, 8)
    desc = CL.ClosureDesc(CL.POLY, CL.SQRT_WRAP, (0.0, 1.0, -1.0))
    with pytest.raises(P.UnsupportedClosureError):
        P.AllenCahn2DPeriodic(dom, KAPPA, R.MU, desc)
    with pytest.raises(P.UnsupportedClosureError):
        P.CahnHilliard2DPeriodic(dom, KAPPA, R.MU, desc)


# ---- class surface -------------------------------------------------------------------------------------------------------
def _names(cls):
    return [f.name for f in dataclasses.fields(cls)]


def test_field_order_is_upstreams():
    assert _names(P.AllenCahn2DPeriodicButlerVolmer) == ["domain", "kappa", "mu", "j0", "alpha", "derivs", "v"]
    assert _names(P.AllenCahn2DPeriodicButlerVolmerConstantCurrent) == ["domain", "kappa", "mu", "j0", "alpha", "Crate", "derivs"]
    assert _names(P.AllenCahn2DSmoothedBoundaryButlerVolmerConstantCurrent) == ["domain", "kappa", "f", "mu", "j0", "alpha",
                                                                               "Crate", "derivs"]


def test_published_attributes_and_methods():
    dom = std_domain(P, 16, 12)
    for eq in (P.AllenCahn2DPeriodicButlerVolmer(dom, KAPPA, R.MU, R.J0, 0.5),
               P.AllenCahn2DPeriodicButlerVolmerConstantCurrent(dom, KAPPA, R.MU, R.J0, 0.5, 0.02)):
        for name in ("kx", "ky", "two_pi_i_kx", "two_pi_i_ky", "two_pi_i_kx_2", "two_pi_i_ky_2", "two_pi_i_k_2", "fft", "ifft"):
            assert hasattr(eq, name), name
        assert eq.kx.shape == (16, 12)
        assert eq.rhs.__func__ is type(eq).rhs_fd
        assert eq._mob_desc.flags == CL.SQRT_WRAP and eq._mu_desc.flags == CL.LOGIT_PRIOR
    psi = R.disc_psi(12, 12)
    sdom = P.Domain((12, 12), ((0.0, 12.0), (0.0, 12.0)), "dimensionless", geometry=types.SimpleNamespace(smooth=psi))
    eq = P.AllenCahn2DSmoothedBoundaryButlerVolmerConstantCurrent(sdom, KAPPA, lambda c: c, R.MU, R.J0, 0.5, 0.02)
    assert np.array_equal(eq.psi, psi) and eq.sqrt_kappa == np.sqrt(KAPPA) and (eq.hx, eq.hy) == tuple(sdom.dx)
    assert eq.norm_grad_psi.shape == psi.shape and eq.left_half.shape == psi.shape
    assert callable(eq.get_voltage)


def test_three_argument_rhs_fd_and_voltage_field():
    import inspect

    sig = inspect.signature(P.AllenCahn2DPeriodicButlerVolmer.rhs_fd)
    assert list(sig.parameters) == ["self", "state", "t", "v"]
    dom = std_domain(P, 8, 8)
    eq = P.AllenCahn2DPeriodicButlerVolmer(dom, KAPPA, R.MU, R.J0, 0.5)
    assert eq.v == 0.0 and not eq._time_dependent_rhs()
    ramp = P.AllenCahn2DPeriodicButlerVolmer(dom, KAPPA, R.MU, R.J0, 0.5, v=lambda t: 0.1 * t)
    assert ramp._time_dependent_rhs() and ramp._value() == 0.0


def test_per_environment_controls():
    assert P.AllenCahn2DPeriodicButlerVolmer._per_env_controls == {"kappa", "mu", "j0", "v"}
    for cls in (P.AllenCahn2DPeriodicButlerVolmerConstantCurrent, P.AllenCahn2DSmoothedBoundaryButlerVolmerConstantCurrent):
        assert cls._per_env_controls == {"kappa", "mu", "j0", "Crate"}


def test_fourier_and_fitting_are_refused():
    dom = std_domain(P, 8, 8)
    with pytest.raises(NotImplementedError):
        P.AllenCahn2DPeriodicButlerVolmerConstantCurrent(dom, KAPPA, R.MU, R.J0, 0.5, 0.02, derivs="fourier")
    with pytest.raises(ValueError):
        P.AllenCahn2DPeriodicButlerVolmerConstantCurrent(dom, KAPPA, R.MU, R.J0, 0.5, 0.02, derivs="spectral")
    model = P.PDEModel(P.AllenCahn2DPeriodicButlerVolmerConstantCurrent, dom, P.Euler)
    with pytest.raises(NotImplementedError):
        model.train({"ys": [], "ts": []}, [], {}, {}, {}, {}, 0.0)
    with pytest.raises(NotImplementedError):
        model.optimize(lambda ys: ys.sum(), np.zeros((8, 8)), [0.0, 1.0], {"mu": R.MU}, {})
    with pytest.raises(NotImplementedError):
        model.observables({}, np.zeros((8, 8, 2)))
