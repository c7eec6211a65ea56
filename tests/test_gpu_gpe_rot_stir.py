"""The stirred, ramped rotating-frame split step on the MI355X (csrc/gpe_rot.hip) against
its numpy reference (tests/gpe_rot_stir_ref.py): every transform path and the JOIN split, the library path, the bitwise
properties, environment groups, spots only / ramp only / neither, save points, PDEEnv, VectorPDEEnv and the
observables at Omega(t)."""
import functools

import numpy as np
import pytest

import pde_opt_amd as P
from pde_opt_amd.engine import HipEngine
from pde_opt_amd.numerics.functions.lights import GaussianSpot, GaussianSpots

import gpe_obs_ref as OR
import gpe_rot_ref as R
import gpe_rot_stir_ref as S

pytestmark = pytest.mark.gpu

K, E, OMEGA, RATE, DT, T0 = 50.0, 0.1, 0.5, 0.9, 0.02, 0.3
TIME_SCALES = [1.0, -1j, 0.3 - 1j]
# 64 x 128 / 128 x 64: x / y mix-ups of the spot coordinates and the JOIN's two Omega; 48 x 40: rocFFT; 1024 x 64:
# the fp64 JOIN runs as LAST + FIRST
SHAPES = [((64, 64), 1), ((64, 64), 3), ((64, 128), 2), ((128, 64), 2), ((48, 40), 3), ((1024, 64), 1)]


def domain(points):
    return P.Domain(tuple(points), ((-2.0, 2.0), (-1.5, 1.5)), "dimensionless")


def spots_of(b):
    """two moving spots of environment b: off-centre, placed and moving differently in x and y"""
    return GaussianSpots([GaussianSpot(3.0 + b, 0.5, -0.6 + 0.1 * b, 0.8, 0.3 - 0.07 * b, -0.4, 0.35),
                          GaussianSpot(-2.0, 1.0 + b, 0.7, -0.5 - 0.2 * b, -0.45, 0.6 + 0.1 * b, 0.25 + 0.05 * b)])


def params_of(b, variant="both"):
    """(k, e, omega, lights, omega_rate) of environment b: all of them differ between the environments of a batch"""
    lights = spots_of(b) if variant in ("both", "spots") else None
    rate = (RATE - 0.7 * b) if variant in ("both", "ramp") else 0.0
    return dict(k=K + 7.0 * b, e=E + 0.05 * b, omega=OMEGA - 0.3 * b, lights=lights, omega_rate=rate)


@functools.lru_cache(maxsize=None)
def reference(points, batch, time_scale, double, nsteps, variant="both"):
    dom = domain(points)
    out = []
    for b, psi in enumerate(R.smooth_state(dom, 5, batch)):
        p = params_of(b, variant)
        case = S.StirCase(dom, p["k"], p["e"], p["omega"], time_scale, double, p["lights"], p["omega_rate"])
        out.append(case.advance(psi, DT, nsteps, T0))
    return np.stack(out).astype(np.complex128)


def engine_for(points, batch, time_scale, dtype, variant="both", group=None):
    dom = domain(points)
    eqs = [P.GPE2DTSRot(dom, **params_of(b, variant)) for b in range(batch)]
    solver = P.RotatingStrangSplitting(eqs[0].dx, time_scale)
    y0 = R.to_pairs(R.smooth_state(dom, 5, batch)).astype(dtype)
    eng = HipEngine(0)
    eng.configure(dtype=y0.dtype, batch=batch, **eqs[0]._engine_problem())
    if batch == 1:
        eqs[0]._engine_upload(eng, T0, T0 + 1.0)
    else:
        P.GPE2DTSRot._engine_upload_batch(eng, eqs, T0, T0 + 1.0)
    solver.configure_engine(eng, eqs[0])
    if group is not None:
        eng.set_group_envs(group)
    eng.set_state(y0)
    return eng, solver.integrator, y0


def device(points, batch, time_scale, dtype, calls, variant="both", group=None):
    """the states after each list of advance calls in `calls`, every list from the start state; an entry is the number
    of steps of one ``advance``, which starts at the local time the steps before it ended at"""
    eng, integ, y0 = engine_for(points, batch, time_scale, dtype, variant, group)
    out = []
    for seq in calls:
        eng.set_state(y0)
        done = 0
        for n in seq:
            eng.advance(integ, DT, n, T0 + done * DT)
            done += n
        out.append(R.from_pairs(eng.get_state().astype(np.float64)))
    return out, eng.last_kernel


def dist(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def expected_kernel(points, variant="both"):
    lib = points == (48, 40)
    if variant == "none":
        return "strang_rot_rocfft_1d" if lib else "strang_rot_fused_lds_fft"
    return "strang_rot_stir_rocfft_1d" if lib else "strang_rot_stir_fused_lds_fft"


CASES = [(p, b, ts) for p, b in SHAPES for ts in TIME_SCALES]


@pytest.mark.parametrize("points,batch,time_scale", CASES)
def test_one_step_and_five_steps_fp64(points, batch, time_scale):
    (one, five), kernel = device(points, batch, time_scale, np.float64, ((1,), (5,)))
    d1 = dist(one, reference(points, batch, time_scale, True, 1))
    d5 = dist(five, reference(points, batch, time_scale, True, 5))
    print(f"fp64 {points} B={batch} ts={time_scale} {kernel}: 1 step {d1:.3e}, 5 steps {d5:.3e}")
    assert kernel == expected_kernel(points)
    assert d1 <= 1e-10 and d5 <= 1e-10


@pytest.mark.parametrize("points,batch,time_scale", CASES)
def test_one_step_and_five_steps_fp32(points, batch, time_scale):
    (one, five), kernel = device(points, batch, time_scale, np.float32, ((1,), (5,)))
    out = []
    for got, n in ((one, 1), (five, 5)):
        ref = reference(points, batch, time_scale, True, n)
        own = dist(reference(points, batch, time_scale, False, n), ref)
        out.append((dist(got, ref), own))
    print(f"fp32 {points} B={batch} ts={time_scale} {kernel}: 1 step {out[0][0]:.3e} (complex64 reference {out[0][1]:.3e}, "
          f"ratio {out[0][0] / out[0][1]:.2f}), 5 steps {out[1][0]:.3e} (complex64 reference {out[1][1]:.3e}, "
          f"ratio {out[1][0] / out[1][1]:.2f})")
    assert kernel == expected_kernel(points)
    # the gate is 8 x the distance of the reference at complex64 from itself at complex128 on the same case
    for got, own in out:
        assert got <= 8 * own


@pytest.mark.parametrize("points", [(64, 128), (48, 40)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_advance_n_equals_n_single_advances_and_a_repeat_bitwise(points, dtype):
    (a, b, singles), kernel = device(points, 2, 0.3 - 1j, dtype, ((5,), (5,), (1, 1, 1, 1, 1)))
    assert kernel == expected_kernel(points)
    assert np.array_equal(a, b)
    assert np.array_equal(a, singles)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_environment_groups_of_one_are_bitwise_the_ungrouped_run(dtype):
    (whole,), _ = device((64, 128), 3, 1.0, dtype, ((5,),))
    eng, integ, y0 = engine_for((64, 128), 3, 1.0, dtype, group=1)
    eng.advance(integ, DT, 5, T0)
    grouped = R.from_pairs(eng.get_state().astype(np.float64))
    assert eng.last_groups() == 3
    assert np.array_equal(whole, grouped)
    assert not np.array_equal(grouped[1], grouped[2])


@pytest.mark.parametrize("variant", ["spots", "ramp", "none"])
@pytest.mark.parametrize("points", [(64, 128), (48, 40)])
def test_spots_only_ramp_only_and_neither(points, variant):
    (five,), kernel = device(points, 3, 1.0, np.float64, ((5,),), variant)
    d = dist(five, reference(points, 3, 1.0, True, 5, variant))
    print(f"{variant} {points}: {kernel} {d:.3e}")
    assert kernel == expected_kernel(points, variant)
    assert d <= 1e-10
    # each of the two changes the solution
    assert dist(five, reference(points, 3, 1.0, True, 5, "both")) > 1e-6


def test_saveat_through_pdemodel_solve():
    points, dt0 = (48, 40), DT
    dom = domain(points)
    ts = np.array([0.3, 0.32, 0.331, 0.36, 0.395])  # on steps, inside a step, and a clipped last step
    psis = R.smooth_state(dom, 5, 2)
    p = params_of(1)
    model = P.PDEModel(P.GPE2DTSRot, dom, P.RotatingStrangSplitting)
    ys = model.solve(p, R.to_pairs(psis), ts, {"time_scale": 1.0}, dt0=dt0)
    assert ys.shape == (len(ts), 2, 48, 40, 2) and model._engine.last_kernel == "strang_rot_stir_rocfft_1d"
    case = S.StirCase(dom, p["k"], p["e"], p["omega"], 1.0, True, p["lights"], p["omega_rate"])
    for b in range(2):
        d = dist(R.from_pairs(ys[:, b]), S.solve(case, psis[b], ts, dt0))
        print(f"SaveAt(ts) fp64, state {b}: {d:.3e}")
        assert d <= 1e-10


ENV_KW = dict(domain=None, solver_type=P.RotatingStrangSplitting, end_time=1.0, step_dt=3 * DT, numeric_dt=DT,
              state_to_observation_func=lambda s: (s[..., 0] ** 2 + s[..., 1] ** 2)[None], reward_function=lambda s: 0.0,
              update_control_value=lambda offset, old: old + offset, solver_parameters={"time_scale": 1.0})


def test_pde_env_with_the_spot_position_as_the_control():
    dom = domain((64, 64))
    psi0 = R.smooth_state(dom, 5)[0]
    spoon = lambda old, new: GaussianSpots.moving(4.0, old, new, 3 * DT, 0.3)
    env = P.PDEEnv(**{**ENV_KW, "domain": dom}, equation_type=P.GPE2DTSRot, reset_func=lambda d, seed=0: R.to_pairs(psi0),
                   reset_control_value=np.array([-0.5, 0.2]), update_control_parameter=spoon,
                   action_space_config={"type": "discrete", "num_actions": 2,
                                        "action_mapping": {0: np.array([0.4, -0.1]), 1: np.array([-0.2, 0.5])}},
                   static_equation_parameters=dict(k=K, e=E, omega=OMEGA, omega_rate=RATE), control_equation_parameter_name="lights")
    env.reset(seed=0)
    env.step(0)
    env.step(1)
    kernel = env._engine.last_kernel
    ref, pos = psi0, np.array([-0.5, 0.2])
    for move in (np.array([0.4, -0.1]), np.array([-0.2, 0.5])):
        ref = S.StirCase(dom, K, E, OMEGA, lights=spoon(pos, pos + move), omega_rate=RATE).advance(ref, DT, 3, 0.0)
        pos = pos + move
    d = dist(R.from_pairs(env._state), ref)
    env.close()
    print(f"PDEEnv, the spoon as the control: {d:.3e}")
    assert kernel == "strang_rot_stir_fused_lds_fft" and d <= 1e-10


def test_pde_env_with_omega_rate_as_the_control():
    dom = domain((64, 64))
    psi0 = R.smooth_state(dom, 5)[0]
    env = P.PDEEnv(**{**ENV_KW, "domain": dom}, equation_type=P.GPE2DTSRot, reset_func=lambda d, seed=0: R.to_pairs(psi0),
                   reset_control_value=0.5, update_control_parameter=lambda old, new: new,
                   action_space_config={"type": "discrete", "num_actions": 2, "action_mapping": {0: 1.0, 1: -2.5}},
                   static_equation_parameters=dict(k=K, e=E, omega=OMEGA), control_equation_parameter_name="omega_rate")
    env.reset(seed=0)
    env.step(0)
    env.step(1)
    ref = psi0
    for rate in (1.5, -1.0):
        ref = S.StirCase(dom, K, E, OMEGA, omega_rate=rate).advance(ref, DT, 3, 0.0)
    d = dist(R.from_pairs(env._state), ref)
    env.close()
    print(f"PDEEnv, omega_rate 1.5 then -1.0: {d:.3e}")
    assert d <= 1e-10


def test_vector_env_with_one_spot_per_environment_equals_single_solves_bitwise():
    dom = domain((64, 128))
    y0 = R.to_pairs(R.smooth_state(dom, 5, 3)).astype(np.float32)
    spoon = lambda old, new: GaussianSpots.moving(4.0, old, new, 3 * DT, 0.3)
    moves = {0: np.array([0.4, -0.1]), 1: np.array([-0.2, 0.5]), 2: np.array([0.0, -0.3])}
    venv = P.VectorPDEEnv(3, **{**ENV_KW, "domain": dom}, equation_type=P.GPE2DTSRot,
                          reset_func=lambda d, seed=0: y0[seed], reset_control_value=np.array([-0.5, 0.2]),
                          update_control_parameter=spoon,
                          action_space_config={"type": "discrete", "num_actions": 3, "action_mapping": moves},
                          static_equation_parameters=dict(k=K, e=E, omega=OMEGA, omega_rate=RATE),
                          control_equation_parameter_name="lights", device_reward=("gpe", "energy"), fetch_observations=False)
    venv.reset(seed=0)
    _, rewards, *_ = venv.step([0, 1, 2])
    batch = venv.states
    venv.close()
    model = P.PDEModel(P.GPE2DTSRot, dom, P.RotatingStrangSplitting)
    start = np.array([-0.5, 0.2])
    for b in range(3):
        p = dict(k=K, e=E, omega=OMEGA, omega_rate=RATE, lights=spoon(start, start + moves[b]))
        one = model.solve(p, y0[b], [0.0, 3 * DT], {"time_scale": 1.0}, dt0=DT)[-1]
        assert np.array_equal(one, batch[b]), b
        # the reward is the energy in the frame of the step's end, Omega(step_dt), with the spoon where it ended
        want = model.observables(p, batch[b], 3 * DT).energy[0]
        assert abs(rewards[b] - want) <= 1e-6 * abs(want), b
    assert not np.array_equal(batch[0], batch[1])


def test_observables_of_a_ramped_stirred_state_use_omega_of_t():
    points, t = (64, 128), 0.37
    dom = domain(points)
    psis = R.smooth_state(dom, 5, 2)
    plist = [params_of(b) for b in range(2)]
    model = P.PDEModel(P.GPE2DTSRot, dom, P.RotatingStrangSplitting)
    obs = model.observables(plist, R.to_pairs(psis), t)
    x, y = dom.mesh()
    for b, p in enumerate(plist):
        V = OR.trap(dom, p["e"]) + p["lights"](t, x, y)
        vals, scales = OR.observables(dom, psis[b], V, p["k"])
        om_t = p["omega"] + p["omega_rate"] * t
        energy, mu = OR.derived(vals, om_t)
        for name in OR.NAMES:
            err = abs(obs[name][b] - vals[name]) / scales[name]
            print(f"observables at t, state {b} {name}: {err:.3e}")
            assert err <= 1e-12, name
        escale = (scales["e_kin"] + scales["e_pot"] + 2 * scales["e_int"] + abs(om_t) * scales["l_z"]) / vals["norm"]
        assert abs(obs.energy[b] - energy) <= 1e-12 * escale and abs(obs.mu[b] - mu) <= 1e-12 * escale
        assert abs(obs.omega[b] - om_t) <= 1e-15
        # Omega(0) would be off by rate * t * l_z
        assert abs(obs.energy[b] - OR.derived(vals, p["omega"])[0]) > 1e-6


def test_the_adjoint_step_refuses_a_ramp():
    eng, _, _ = engine_for((64, 64), 1, 1.0, np.float64, "ramp")
    lam, grad = np.zeros((1, 64, 64, 2)), np.zeros((1, 3))  # refused before any pointer is looked at
    with pytest.raises(ValueError, match="constant Omega"):
        eng.gpe_rot_adjoint_step(DT, eng.state_device_ptr()[0], lam.ctypes.data, grad.ctypes.data)
