"""Device memory is owned by DeviceBuffer members (csrc/device_buffer.hpp): nothing leaks when the networks and engines
close, a block that survives a configure is never undersized, and the grow-only work blocks grow, never shrink and
never return stale rows.  32 x 32 grids, 64 x 64 where the GPE passes need a covered size; batch 2 - 3."""

import numpy as np
import pytest

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg
from pde_opt_amd.numerics.functions.lights import GaussianSpot, GaussianSpots
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


def _adjoint_call(eng, call, *grad_shapes):
    """one backward substep from the resident state: a white-noise cotangent on the device, host gradient blocks;
    `call(psi0_ptr, lam_ptr, *grad_ptrs)`.  Returns the new cotangent and the blocks."""
    shape = (eng.batch,) + eng.state_shape
    lam = np.random.default_rng(12).standard_normal(shape).astype(eng.dtype)
    lam_dev = eng.buffer_alloc(lam.nbytes)
    eng.buffer_copy(lam_dev, lam, lam.nbytes, L.COPY_H2D)
    grads = [np.zeros(s) for s in grad_shapes]
    call(eng.state_device_ptr()[0], lam_dev, *[g.ctypes.data for g in grads])
    eng.sync()
    eng.buffer_copy(lam, lam_dev, lam.nbytes, L.COPY_D2H)
    eng.buffer_free(lam_dev)
    assert all(np.all(np.isfinite(g)) for g in grads) and np.all(np.isfinite(lam))
    return (lam,) + tuple(grads)


def _gpe_strang_library_and_adjoint(eng, batch):
    """after _gpe_strang: one Strang step through rocFFT (the Spectral state), then one step of the Strang step's adjoint,
    which differentiates one light spot"""
    eng.set_kernel_path(1)
    eng.advance(L.INT_STRANG, 1e-3, 1)
    assert eng.last_kernel == "strang_rocfft_c2c"
    eng.set_kernel_path(0)
    tab = GaussianSpots([GaussianSpot(1.5, -0.8, 0.4, 0.9, -0.3, 0.5, 0.6)]).table(1)
    eng.set_gpe_spots(np.broadcast_to(tab, (batch,) + tab.shape), *eng.gpe_origin)
    _adjoint_call(eng, lambda psi0, lam, g: eng.gpe_adjoint_step(0.0, 1e-3, psi0, lam, g), (batch, 1, 7))
    assert eng.last_kernel == "strang_adjoint_rocfft_c2c"
    eng.set_gpe_spots(None)


def _gpe_rot_stirred_adjoint(eng, n, batch):
    """one step of the adjoint of the stirred, ramped rotating-frame split step (the set-up of
    test_gpu_gpe_rot_stir_adjoint.py: two moving spots and a rotation ramp per environment)"""
    dom = P.Domain((n, n), ((-2.0, 2.0), (-1.5, 1.5)), "dimensionless")
    spots = lambda b: GaussianSpots([GaussianSpot(3.0 + b, 0.5, -0.6 + 0.1 * b, 0.8, 0.3 - 0.07 * b, -0.4, 0.35),  # noqa: E731
                                     GaussianSpot(-2.0, 1.0 + b, 0.7, -0.5 - 0.2 * b, -0.45, 0.6 + 0.1 * b, 0.25 + 0.05 * b)])
    eqs = [P.GPE2DTSRot(dom, k=50.0 + 7.0 * b, e=0.1 + 0.05 * b, omega=0.5 - 0.3 * b, lights=spots(b), omega_rate=0.9 - 0.7 * b)
           for b in range(batch)]
    eng.configure(dtype=np.float32, batch=batch, **eqs[0]._engine_problem())
    P.GPE2DTSRot._engine_upload_batch(eng, eqs, 0.3, 1.3)
    P.RotatingStrangSplitting(**prepare_solver_params(P.RotatingStrangSplitting, {"time_scale": 1.0}, eqs[0])).configure_engine(eng, eqs[0])
    eng.set_state(np.random.default_rng(13).standard_normal((batch, n, n, 2)).astype(np.float32))
    _adjoint_call(eng, lambda psi0, lam, g, sg: eng.gpe_rot_stir_adjoint_step(0.3, 0.02, psi0, lam, g, sg), (batch, 4), (batch, 2, 7))
    assert eng.last_kernel == "strang_rot_stir_adjoint_rocfft_1d"


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


def _tour(eng):
    """after _explicit_and_diagnostics(eng, 32, 2): every feature state of the ctx (csrc/feature_slot.hpp) is created on
    the way; the engine ends on the 32 x 32 fp32 batch-2 Cahn-Hilliard shape, holding the implicit workspace"""
    _imex(eng, 32, 2)  # Spectral (32 is no size of the hand-written transforms)
    _gpe_strang(eng, 64, 2)  # StrangFused
    _gpe_strang_library_and_adjoint(eng, 2)  # Spectral, GpeAdjoint
    eng.gpe_observables()  # GpeObs
    eng.detect_vortices(0.01, 0.5, want_winding=False)
    _gpe_rot(eng, 64, 2)  # GpeRot, GpeRotAdjoint (frozen)
    _gpe_rot_stirred_adjoint(eng, 64, 2)  # GpeRotAdjoint (stirred)
    _sensitivities(eng, 32, 2)  # Sens
    _butler_volmer(eng, 32, 2)  # BvState
    _implicit(eng, 32, 2)  # Implicit


def test_everything_is_released():
    probe = P.HipEngine()  # never configured: holds nothing, reads the process-wide counter
    before = probe.device_bytes()
    eng = P.HipEngine()
    _explicit_and_diagnostics(eng, 32, 2)
    assert probe.device_bytes() > before
    _tour(eng)
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


def test_a_shape_change_drops_every_feature_state():
    """An engine that has held every feature state and one that never held any hold the same bytes once both run the plain
    32 x 32 fp32 batch-2 Cahn-Hilliard problem: a state some slot left behind would show as a byte difference.  Both end
    with _explicit_and_diagnostics, so the grow-only work blocks of its reductions and diagnostics (and its shell tables)
    have the same sizes on both; the tour grows none of them any further."""
    probe = P.HipEngine()
    base = probe.device_bytes()

    def life(tour):
        eng = P.HipEngine()
        if tour:
            _explicit_and_diagnostics(eng, 32, 2)
            _tour(eng)
            # the tour ends on the shape of the last part, which a configure keeps: one more shape change (fp64) that drops
            # the implicit workspace and leaves the Butler-Volmer state for the last configure to drop
            _butler_volmer(eng, 32, 2)
        _explicit_and_diagnostics(eng, 32, 2)  # configure, a state, RK4 steps, the diagnostics
        eng.set_state(_state(32, 2, 11))
        eng.advance(L.INT_RK4, DT, 2)
        state, held = eng.get_state(), probe.device_bytes() - base
        eng.close()
        assert probe.device_bytes() == base
        return state, held

    state_a, held_a = life(True)
    state_b, held_b = life(False)
    print(f"bytes held: after the tour {held_a}, fresh {held_b}")
    assert held_b > 0 and held_a == held_b
    assert np.all(np.isfinite(state_b)) and np.array_equal(state_a, state_b)
    probe.close()


def _gpe_control(n):
    dom = P.Domain((n, n), GPE_BOX, "dimensionless")
    return dom, P.GPE2DTSControl(dom, 500.0, 0.2, GaussianSpots([GaussianSpot(1.5, -0.8, 0.4, 0.9, -0.3, 0.5, 0.6)]),
                                 trap_factor=1.0, kinetic=True)


def _strang_case(kernel_path, kernel):
    """(set up with the A_term scaled by s, run from the starting state) of a Strang advance on one kernel path"""
    dom, eq = _gpe_control(64)

    def setup(eng, s):
        eng.set_kernel_path(kernel_path)
        eng.configure(dtype=np.float32, batch=2, **eq._engine_problem())
        eq._engine_upload(eng, 0.0, 1.0)
        eng.set_integrator_params(time_scale=1.0, strang_dx=float(eq.dx))
        eng.set_aux(L.AUX_GPE_A_TERM, s * np.asarray(eq.A_term))

    def run(eng):
        eng.set_state(_psi(dom, 2))
        eng.advance(L.INT_STRANG, 1e-3, 2)
        assert eng.last_kernel == kernel
        return (eng.get_state(),)

    return L.AUX_GPE_A_TERM, np.asarray(eq.A_term), setup, run


def _strang_adjoint_case():
    dom, eq = _gpe_control(64)

    def setup(eng, s):
        eng.configure(dtype=np.float32, batch=2, **eq._engine_problem())
        eq._engine_upload(eng, 0.0, 1.0)
        eng.set_integrator_params(time_scale=1.0, strang_dx=float(eq.dx))
        eng.set_aux(L.AUX_GPE_A_TERM, s * np.asarray(eq.A_term))

    def run(eng):
        eng.set_state(_psi(dom, 2))
        return _adjoint_call(eng, lambda psi0, lam, g: eng.gpe_adjoint_step(0.0, 1e-3, psi0, lam, g), (2, 1, 7))

    return L.AUX_GPE_A_TERM, np.asarray(eq.A_term), setup, run


def _imex_case(n, kernel_path, kernel):
    eq = _ch(n)
    symbol = np.asarray(eq.fourier_symbol)

    def setup(eng, s):
        eng.set_kernel_path(kernel_path)
        eng.configure(dtype=np.float32, batch=2, **eq._engine_problem())
        eng.set_integrator_params(imex_A=0.5)
        eng.set_aux(L.AUX_IMEX_SYMBOL, s * symbol)

    def run(eng):
        eng.set_state(_state(n, 2, 1))
        eng.advance(L.INT_IMEX, 1e-6, 2)
        assert eng.last_kernel.endswith(kernel)
        return (eng.get_state(),)

    return L.AUX_IMEX_SYMBOL, symbol, setup, run


AUX_CASES = {
    "strang_fused": lambda: _strang_case(0, "strang_fused_lds_fft"),  # StrangFused::mult_valid
    "strang_rocfft": lambda: _strang_case(1, "strang_rocfft_c2c"),  # Spectral::mult_kind
    # 64 x 64: the smallest grid the hand-written transforms cover (at 32 x 32 the step below would run instead)
    "imex_fused": lambda: _imex_case(64, 0, "+imex_fused_lds_fft"),  # StrangFused::imex_valid
    "imex_rocfft": lambda: _imex_case(32, 1, "+imex_rocfft_r2c"),  # Spectral::mult_kind
    "strang_adjoint": _strang_adjoint_case,  # GpeAdjoint::mult_valid
}


@pytest.mark.parametrize("case", sorted(AUX_CASES))
def test_set_aux_invalidates_every_cached_multiplier(case):
    """A state that caches a multiplier keys it on the step size and the integrator's parameters, not on the aux field it
    was built from: only pdeopt_set_aux's invalidation makes the second advance below, with the same dt, rebuild it.
    Engine A advances with the field V1, uploads V2 = 1.5 V1 and advances again from the same state; engine B sees only V2.

    The rotating-frame step and its two adjoints have no case: their cached tables (GpeRot, GpeRotAdjoint: kin_x / kin_y)
    are functions of dt, the time scale and the mesh alone, formed in-kernel from no aux field (upload_kinetic in
    gpe_rot.hip / gpe_rot_adjoint.hip); the potential, their only aux field, is read by the kernels directly."""
    which, v1, setup, run = AUX_CASES[case]()
    a = P.HipEngine()
    setup(a, 1.0)
    first = run(a)
    a.set_aux(which, 1.5 * v1)
    again = run(a)
    a.close()
    b = P.HipEngine()
    setup(b, 1.5)
    want = run(b)
    b.close()
    assert all(np.all(np.isfinite(w)) for w in want)
    assert not np.array_equal(first[0], want[0]), "V1 and V2 give the same result: the case shows nothing"
    for g, w in zip(again, want):
        assert np.array_equal(g, w)


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
