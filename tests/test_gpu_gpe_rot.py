"""The rotating-frame alternating-direction split step on the MI355X (csrc/gpe_rot.hip) against its numpy reference
(tests/gpe_rot_ref.py): every transform path, the library path, Omega = 0 against the existing Strang step, the bitwise
properties, save points, per-environment Omega, PDEEnv and the example."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd.engine import HipEngine

import gpe_rot_ref as R

pytestmark = pytest.mark.gpu

OMEGA, K, E, DT = 0.7, 50.0, 0.1, 2e-3
F32_SHAPES = [(64, 64), (128, 64), (512, 64), (1024, 64), (64, 1024), (48, 40)]
F64_SHAPES = [(64, 64), (1024, 64), (48, 40)]
TIME_SCALES = [1.0, -1j, 0.3 - 1j]


def domain(points):
    return P.Domain(tuple(points), ((-6.0, 6.0), (-6.0, 6.0)), "dimensionless")


def engine_for(eq, solver, y0, eng=None, batch_eqs=None):
    eng = eng or HipEngine(0)
    eng.configure(dtype=y0.dtype, batch=y0.shape[0], **eq._engine_problem())
    if batch_eqs is None:
        eq._engine_upload(eng, 0.0, 1.0)
    else:
        type(eq)._engine_upload_batch(eng, batch_eqs, 0.0, 1.0)
    solver.configure_engine(eng, eq)
    eng.set_state(y0)
    return eng


@functools.lru_cache(maxsize=None)
def reference(points, batch, time_scale, omega, double, nsteps):
    dom = domain(points)
    case = R.RotCase(dom, K, E, omega, time_scale, double)
    return np.stack([case.advance(psi, DT, nsteps) for psi in R.smooth_state(dom, 5, batch)]).astype(np.complex128)


def device(points, batch, time_scale, omega, dtype, calls):
    """the states after each of the advance calls in `calls` (numbers of steps)"""
    dom = domain(points)
    eq = P.GPE2DTSRot(dom, K, E, omega)
    solver = P.RotatingStrangSplitting(eq.dx, time_scale)
    eng = engine_for(eq, solver, R.to_pairs(R.smooth_state(dom, 5, batch)).astype(dtype))
    out = []
    for n in calls:
        eng.advance(solver.integrator, DT, n)
        out.append(R.from_pairs(eng.get_state().astype(np.float64)))
    return out, eng.last_kernel


def dist(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


CASES = [(s, b, ts) for s in F32_SHAPES for b, ts in ((1, 1.0), (3, -1j), (3, 0.3 - 1j))]


@pytest.mark.parametrize("points,batch,time_scale", [c for c in CASES if c[0] in F64_SHAPES])
def test_one_step_and_five_steps_fp64(points, batch, time_scale):
    (one, six), kernel = device(points, batch, time_scale, OMEGA, np.float64, (1, 4))
    d1 = dist(one, reference(points, batch, time_scale, OMEGA, True, 1))
    d5 = dist(six, reference(points, batch, time_scale, OMEGA, True, 5))
    print(f"fp64 {points} B={batch} ts={time_scale} {kernel}: 1 step {d1:.3e}, 5 steps {d5:.3e}")
    assert ("rocfft" in kernel) == (points == (48, 40))
    assert d1 <= 1e-10 and d5 <= 1e-10


@pytest.mark.parametrize("points,batch,time_scale", CASES)
def test_one_step_and_five_steps_fp32(points, batch, time_scale):
    (one, six), kernel = device(points, batch, time_scale, OMEGA, np.float32, (1, 4))
    out = []
    for got, n in ((one, 1), (six, 5)):
        ref = reference(points, batch, time_scale, OMEGA, True, n)
        own = dist(reference(points, batch, time_scale, OMEGA, False, n), ref)
        out.append((dist(got, ref), own))
    print(f"fp32 {points} B={batch} ts={time_scale} {kernel}: 1 step {out[0][0]:.3e} (complex64 reference {out[0][1]:.3e}), "
          f"5 steps {out[1][0]:.3e} (complex64 reference {out[1][1]:.3e})")
    # the gate is 8 x the distance of the reference at complex64 from itself at complex128 on the same case
    for got, own in out:
        assert got <= 8 * own


@pytest.mark.parametrize("points", [(64, 64), (128, 64)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_omega_zero_equals_the_existing_strang_step(points, dtype):
    dom = domain(points)
    y0 = R.to_pairs(R.smooth_state(dom, 5, 2)).astype(dtype)
    (rot,), _ = device(points, 2, 1.0, 0.0, dtype, (5,))
    eq = P.GPE2DTSControl(dom, K, E, lambda t, x, y: 0.0 * x, kinetic=True)
    solver = P.StrangSplitting(eq.A_term, eq.dx, time_scale=1.0)
    eng = engine_for(eq, solver, y0)
    eng.advance(solver.integrator, DT, 5)
    old = R.from_pairs(eng.get_state().astype(np.float64))
    d = dist(rot, old)
    print(f"Omega = 0 {points} {np.dtype(dtype).name}: rotating step against the Strang step {d:.3e}")
    if dtype == np.float64:
        assert d <= 1e-10
    else:
        ref = reference(points, 2, 1.0, 0.0, True, 5)
        assert d <= 8 * dist(reference(points, 2, 1.0, 0.0, False, 5), ref)


@pytest.mark.parametrize("points,dtype", [((64, 128), np.float32), ((1024, 64), np.float64), ((48, 40), np.float32)])
def test_advance_n_equals_n_single_advances_and_a_repeat_bitwise(points, dtype):
    (a,), _ = device(points, 2, 0.3 - 1j, OMEGA, dtype, (4,))
    (b,), _ = device(points, 2, 0.3 - 1j, OMEGA, dtype, (4,))
    singles, _ = device(points, 2, 0.3 - 1j, OMEGA, dtype, (1, 1, 1, 1))
    assert np.array_equal(a, b)
    assert np.array_equal(a, singles[-1])


def test_saveat_through_pdemodel_solve():
    points, dt0 = (64, 64), 2e-3
    dom = domain(points)
    ts = np.array([0.0, 0.002, 0.0031, 0.006, 0.0075])  # on steps, inside steps, and a clipped last step
    psi0 = R.smooth_state(dom, 5)[0]
    model = P.PDEModel(P.GPE2DTSRot, dom, P.RotatingStrangSplitting)
    ys = model.solve(dict(k=K, e=E, omega=OMEGA), R.to_pairs(psi0), ts, {"time_scale": 1.0}, dt0=dt0)
    ref = R.solve(R.RotCase(dom, K, E, OMEGA), psi0, ts, dt0)
    d = dist(R.from_pairs(ys), ref)
    print(f"SaveAt(ts) fp64: {d:.3e}")
    assert ys.shape == (len(ts), 64, 64, 2) and d <= 1e-10
    batched = P.diffeqsolve(P.GPE2DTSRot(dom, K, E, OMEGA), P.RotatingStrangSplitting(dom.dx[0]), t0=0.0, t1=0.0075, dt0=dt0,
                            y0=np.stack([R.to_pairs(psi0)] * 2), saveat=P.SaveAt(t0=True, t1=True))
    assert batched.ys.shape == (2, 2, 64, 64, 2) and dist(R.from_pairs(batched.ys[-1, 1]), ref[-1]) <= 1e-10


def test_per_environment_omega_equals_single_solves_bitwise():
    points, omegas = (64, 128), (0.0, 0.5, -0.5)
    dom = domain(points)
    y0 = R.to_pairs(R.smooth_state(dom, 5, 3)).astype(np.float32)
    eqs = [P.GPE2DTSRot(dom, K, E, om) for om in omegas]
    solver = P.RotatingStrangSplitting(dom.dx[0], -1j)
    eng = engine_for(eqs[0], solver, y0, batch_eqs=eqs)
    eng.advance(solver.integrator, DT, 3)
    batch = eng.get_state()
    for b, eq in enumerate(eqs):
        one = engine_for(eq, solver, y0[b:b + 1])
        one.advance(solver.integrator, DT, 3)
        assert np.array_equal(one.get_state()[0], batch[b]), b
    assert not np.array_equal(batch[1], batch[2])


def test_pde_env_with_omega_as_the_control():
    points = (64, 64)
    dom = domain(points)
    psi0 = R.smooth_state(dom, 5)[0]
    env = P.PDEEnv(
        equation_type=P.GPE2DTSRot, domain=dom, solver_type=P.RotatingStrangSplitting, end_time=1.0, step_dt=3 * DT,
        numeric_dt=DT, state_to_observation_func=lambda s: (s[..., 0] ** 2 + s[..., 1] ** 2)[None],
        reward_function=lambda s: 0.0, reset_func=lambda d, seed=0: R.to_pairs(psi0), reset_control_value=0.2,
        update_control_value=lambda offset, old: old + offset, update_control_parameter=lambda old, new: new,
        action_space_config={"type": "discrete", "num_actions": 2, "action_mapping": {0: 0.3, 1: -0.6}},
        static_equation_parameters=dict(k=K, e=E), control_equation_parameter_name="omega", solver_parameters={"time_scale": 1.0})
    env.reset(seed=0)
    env.step(0)
    env.step(1)
    ref = psi0
    for om in (0.5, -0.1):
        ref = R.RotCase(dom, K, E, om).advance(ref, DT, 3)
    d = dist(R.from_pairs(env._state), ref)
    env.close()
    print(f"PDEEnv, omega 0.5 then -0.1: {d:.3e}")
    assert d <= 1e-10


def test_vector_env_controls_and_wrong_equation():
    assert P.GPE2DTSRot._per_env_controls == frozenset({"k", "e", "omega"})
    eng = HipEngine(0)
    eng.configure(equation=L.EQ_ALLEN_CAHN, dtype=np.float32, nx=64, ny=64, batch=1, hx=0.1, hy=0.1, mu=P.as_closure(lambda c: c),
                  mob=P.as_closure(lambda c: 1.0 + 0 * c))
    with pytest.raises(ValueError, match="GPE"):
        eng.advance(L.INT_STRANG_ROT, 1e-3, 1)


def test_the_example_runs():
    """the vortex count is the CPU reference's on the same seeded case (tests/gpe_rot_ref.py, complex128 and complex64
    alike): the imprinted singularity stays, none joins it within the example's length"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "gpe_rotating_vortices.py")
    spec = importlib.util.spec_from_file_location("gpe_rotating_vortices", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    state, count = ex.main()
    assert np.isfinite(state).all()
    # normalised as the scheme normalises: between the half steps of every step, so that in imaginary time the state
    # at a step's end has the norm 1 + O(dt) of the CPU reference run of the same case (1.000858), not 1
    ref = R.RotCase(ex.dom, ex.K, ex.E, ex.OMEGA, -1j).advance(R.from_pairs(ex.initial_state().astype(np.float64)), ex.DT, ex.STEPS)
    h2 = ex.dom.dx[0] ** 2
    ref_norm = float(np.sum(np.abs(ref) ** 2) * h2)
    assert abs(ref_norm - 1.0) < 2e-3
    assert abs(float(np.sum(state.astype(np.float64) ** 2) * h2) - ref_norm) < 1e-4
    assert count == 1
