"""Device memory is owned by DeviceBuffer members (csrc/device_buffer.hpp): nothing leaks when the networks and engines
close, a block that survives a configure is never undersized, and the grow-only work blocks grow, never shrink and
never return stale rows.  32 x 32 grids, 64 x 64 where the GPE passes need a covered size; batch 2 - 3."""

import numpy as np
import pytest

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg
from pde_opt_amd.structure_factor import shell_tables
from pde_opt_amd.utils import prepare_solver_params

import bv_ref
import sens_ref

pytestmark = pytest.mark.gpu

MU = lambda c: np.log(c / (1 - c)) + 3 * (1 - 2 * c)  # noqa: E731
MOB = lambda c: c * (1 - c)  # noqa: E731
DT = 2e-7
GPE_BOX = ((-12.0, 12.0), (-9.0, 9.0))


def _domain(n):
    return P.Domain((n, n), ((-0.005 * n, 0.005 * n), (-0.005 * n, 0.005 * n)), "dimensionless")


def _ch(n):
    return P.CahnHilliard2DPeriodic(_domain(n), 0.002, MU, MOB)


def _problem(n, equation=L.EQ_CAHN_HILLIARD):
    prob = dict(_ch(n)._engine_problem())
    prob["equation"] = equation
    return prob


def _state(n, batch, seed):
    rng = np.random.default_rng(seed)
    return np.clip(0.5 + 0.05 * rng.standard_normal((batch, n, n)), 0.05, 0.95).astype(np.float32)


def _psi(dom, batch):
    X, Y = dom.mesh()
    out = []
    for b in range(batch):
        psi = np.exp(-(X**2 / (14.0 + b) + Y**2 / 10.0)) * np.exp(0.3j * X - 0.1j * b * Y)
        psi /= np.sqrt(np.sum(np.abs(psi) ** 2) * dom.dx[0] * dom.dx[1])
        out.append(np.stack([psi.real, psi.imag], axis=-1))
    return np.stack(out).astype(np.float32)


def _gpe_strang(eng, n, batch, steps=2):
    """configure the controlled GPE with its potential and multiplier, load a state, run a short Strang advance"""
    dom = P.Domain((n, n), GPE_BOX, "dimensionless")
    eq = P.GPE2DTSControl(dom, 500.0, 0.2, lambda t, x, y: 0.05 * x - 0.02 * y, trap_factor=1.0, kinetic=True)
    eng.configure(dtype=np.float32, batch=batch, **eq._engine_problem())
    eng.set_aux(L.AUX_GPE_POTENTIAL, eq.potential(0.0))
    P.StrangSplitting(eq.A_term, eq.dx, eq.fft, eq.ifft, 1.0).configure_engine(eng, eq)
    eng.set_state(_psi(dom, batch))
    eng.advance(L.INT_STRANG, 1e-3, steps)
    X, Y = dom.mesh()
    eng.gpe_origin = (float(X[0, 0]), float(Y[0, 0]))
    return dom


def _gpe_rot(eng, n, batch):
    """one rotating-frame split step and one step of its adjoint"""
    dom = P.Domain((n, n), ((-2.0, 2.0), (-1.5, 1.5)), "dimensionless")
    eqs = [P.GPE2DTSRot(dom, 1.3 + 0.2 * b, 0.2, 0.6 - 0.3 * b) for b in range(batch)]
    eng.configure(dtype=np.float32, batch=batch, **eqs[0]._engine_problem())
    P.GPE2DTSRot._engine_upload_batch(eng, eqs, 0.0, 0.02)
    P.RotatingStrangSplitting(**prepare_solver_params(P.RotatingStrangSplitting, {"time_scale": 1.0}, eqs[0])).configure_engine(eng, eqs[0])
    rng = np.random.default_rng(3)
    eng.set_state(rng.standard_normal((batch, n, n, 2)).astype(np.float32))
    eng.advance(L.INT_STRANG_ROT, 0.02, 1)
    lam = rng.standard_normal((batch, n, n, 2)).astype(np.float32)
    lam_dev = eng.buffer_alloc(lam.nbytes)
    eng.buffer_copy(lam_dev, lam, lam.nbytes, L.COPY_H2D)
    grad = np.zeros((batch, 3))
    eng.gpe_rot_adjoint_step(0.02, eng.state_device_ptr()[0], lam_dev, grad.ctypes.data)
    eng.sync()
    eng.buffer_free(lam_dev)
    assert np.all(np.isfinite(grad))


def _explicit_and_diagnostics(eng, n, batch):
    eng.configure(dtype=np.float32, batch=batch, **_problem(n))
    eng.set_state(_state(n, batch, 0))
    eng.advance(L.INT_RK4, DT, 2)
    eng.snapshot()
    eng.advance(L.INT_RK4, DT, 1)
    eng.get_interpolated(0.5)
    eng.tsit5_trial(0.0, DT, 1e-4, 1e-6)
    eng.tsit5_commit(True)
    eng.reduce(L.RED_MEAN)
    eng.reduce(L.RED_VAR)
    eng.pf_observables()
    tabs = shell_tables(_domain(n))
    eng.sk_configure(tabs.tables, tabs.n_bins)
    eng.structure_factor()


def _imex(eng, n, batch):
    eq = _ch(n)
    eng.configure(dtype=np.float32, batch=batch, **eq._engine_problem())
    P.SemiImplicitFourierSpectral(0.5, eq.fourier_symbol, eq.fft, eq.ifft).configure_engine(eng, eq)
    eng.set_state(_state(n, batch, 1))
    eng.advance(L.INT_IMEX, 1e-6, 2)


def _implicit(eng, n, batch):
    eng.configure(dtype=np.float32, batch=batch, **_problem(n))
    eng.set_state(_state(n, batch, 2))
    eng.implicit_configure(1e-6, 1e-9, restart=5)
    eng.implicit_advance(DT, 1)
    eng.implicit_set_precond("spectral")
    eng.implicit_advance(DT, 1)


def _sensitivities(eng, n, B):
    """a sensitivity solve of B trajectories and two parameters, then the Gauss-Newton sums of one frame"""
    params = [(sens_ref.MU_ROLE, 1), (sens_ref.MOB_ROLE, 0)]
    logit = lambda c: np.log(c / (1.0 - c))  # noqa: E731
    eq = P.CahnHilliard2DPeriodic(P.Domain((n, n), ((0.0, 1.0), (0.0, 1.0)), "dimensionless"), 0.002,
                                  ChemLeg(np.array([0.0, -3.0, 0.4]), logit), DiffLeg(np.array([-0.3, 0.2])))
    eng.configure(dtype=np.float64, batch=(1 + len(params)) * B, **eq._engine_problem())
    eq._engine_upload(eng, 0.0, 1.0)
    P.SemiImplicitFourierSpectral(0.5, eq.fourier_symbol, eq.fft, eq.ifft).configure_engine(eng, eq)
    eng.sens_configure(B, params)
    base = _state(n, B, 4).astype(np.float64)
    eng.set_state(np.concatenate([base, np.zeros((len(params) * B, n, n))]))
    eng.sens_advance(L.INT_IMEX, 1e-6, 2)
    eng.sens_set_data(base[None])
    assert np.all(np.isfinite(eng.sens_accumulate(0)))


def _butler_volmer(eng, n, batch):
    h = 0.01
    dom = P.Domain((n, n), ((-h * n / 2, h * n / 2), (-h * n / 2, h * n / 2)), "dimensionless")
    eqs = [P.AllenCahn2DPeriodicButlerVolmerConstantCurrent(dom, 0.002, bv_ref.MU, bv_ref.J0, 0.5, 0.02 - 0.01 * b) for b in range(batch)]
    eng.configure(dtype=np.float64, batch=batch, **eqs[0]._engine_problem())
    type(eqs[0])._engine_upload_batch(eng, eqs)
    eng.set_state(bv_ref.notebook_state(np.random.default_rng(5), (batch, n, n), np.float64))
    eng.advance(L.INT_RK4, 1e-6, 2)
    assert np.all(np.isfinite(eng.bv_voltage()))


def _network(eng, net):
    """one forward and one vjp of a native network on device fields of the configured problem; the handle stays open"""
    net.set_params(0.1 * np.random.default_rng(6).standard_normal(net.n_params))
    shape = (eng.batch,) + eng.state_shape
    host = [np.random.default_rng(s).standard_normal(shape).astype(eng.dtype) for s in (7, 8, 9, 10)]
    dev = [eng.buffer_alloc(a.nbytes) for a in host]
    for d, a in zip(dev, host):
        eng.buffer_copy(d, a, a.nbytes, L.COPY_H2D)
    u, mu, g, lam = dev
    net.forward(u, mu)
    net.vjp(u, g, lam)
    assert np.all(np.isfinite(net.grad_read(reset=True)))
    for d in dev:
        eng.buffer_free(d)


def test_everything_is_released():
    probe = P.HipEngine()  # never configured: holds nothing, reads the process-wide counter
    before = probe.device_bytes()
    eng = P.HipEngine()
    _explicit_and_diagnostics(eng, 32, 2)
    assert probe.device_bytes() > before
    _imex(eng, 32, 2)
    _gpe_strang(eng, 64, 2)
    eng.gpe_observables()
    eng.detect_vortices(0.01, 0.5, want_winding=False)
    _gpe_rot(eng, 64, 2)
    _sensitivities(eng, 32, 2)
    _butler_volmer(eng, 32, 2)
    _implicit(eng, 32, 2)
    # the networks on a second engine, while the first still holds the implicit workspace
    nets_eng = P.HipEngine()
    nets_eng.configure(dtype=np.float32, batch=2, **_problem(32))
    cnn = nets_eng.cnn((1, 16, 1), L.CNN_TANH)
    mixer = nets_eng.mixer(4, 8, 5, 7, 1, L.MIXER_RELU)
    _network(nets_eng, cnn)
    _network(nets_eng, mixer)
    held = probe.device_bytes()
    cnn.close()
    mixer.close()
    assert probe.device_bytes() < held
    nets_eng.close()
    eng.close()
    assert probe.device_bytes() == before
    probe.close()


def _configure(eng, kind, n, batch, seed):
    """(configure, set the state, a short advance) -> what is compared bit for bit with a fresh engine"""
    if kind == "gpe":
        _gpe_strang(eng, n, batch, steps=3)
        return (eng.get_state(),)
    eng.configure(dtype=np.float32, batch=batch, **_problem(n, L.EQ_ALLEN_CAHN if kind == "ac" else L.EQ_CAHN_HILLIARD))
    eng.set_state(_state(n, batch, seed))
    eng.advance(L.INT_RK4, DT, 3)
    return eng.reduce(L.RED_VAR), eng.get_state()


def test_reconfigure_matches_a_fresh_engine():
    """a block that survives a configure with the wrong size would show here: as PDEOPT_ESTATE, never as a fault"""
    eng = P.HipEngine()
    order = (("ch", 32, 2), ("gpe", 64, 3), ("ac", 32, 2), ("gpe", 64, 2), ("ch", 64, 3), ("gpe", 64, 3), ("ch", 32, 2))
    for step, (kind, n, batch) in enumerate(order):
        got = _configure(eng, kind, n, batch, step)
        fresh = P.HipEngine()
        want = _configure(fresh, kind, n, batch, step)
        fresh.close()
        for g, w in zip(got, want):
            assert np.all(np.isfinite(w)) and np.array_equal(g, w), (step, kind, n, batch)
    eng.close()


def test_grow_only_blocks_keep_their_size_and_their_rows():
    batch = 3
    tabs = shell_tables(_domain(32))

    def engine():
        e = P.HipEngine()
        e.configure(dtype=np.float32, batch=batch, **_problem(32))
        e.set_state(_state(32, batch, 7))
        e.sk_configure(tabs.tables, tabs.n_bins)
        return e

    calls = (lambda e, n: e.structure_factor(0, n), lambda e, n: e.pf_observables(0, n), lambda e, n: e.reduce(L.RED_VAR)[:n])
    ref = engine()  # the single-call values: one call each on an engine that has made no other
    full = [c(ref, batch) for c in calls]
    ref.close()
    eng = engine()
    one = [c(eng, 1) for c in calls]
    after_first = eng.device_bytes()
    whole = [c(eng, batch) for c in calls]  # grows the work blocks of the first call
    after_second = eng.device_bytes()
    assert after_second > after_first
    again = [c(eng, 1) for c in calls]
    assert eng.device_bytes() == after_second
    for f, o, w, a in zip(full, one, whole, again):
        assert np.array_equal(w, f) and np.array_equal(o, f[:1]) and np.array_equal(a, f[:1])
    eng.close()
