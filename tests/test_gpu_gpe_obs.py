"""The GPE observables on the MI355X (csrc/gpe_obs.hip) against their numpy reference (tests/gpe_obs_ref.py): both
hand-written passes, mixed sizes, the library path, both equation classes, in-kernel spots, per-environment k / Omega /
potential; the bitwise properties; ``PDEModel.ground_state`` against the same loop in numpy; the device reward.

Gates (errors relative to an observable's scale = the sum of the absolute values of its terms): fp64 1e-12 (the
transforms agree with numpy to <= 3e-15, the sums are fp64), fp32 5e-6 (about 3 x the fp32 one-step error of the same
transforms)."""
import functools

import numpy as np
import pytest

import gpe_obs_ref as R
import gpe_rot_ref as RR
import pde_opt_amd as P
from pde_opt_amd.engine import HipEngine

pytestmark = pytest.mark.gpu

# the issue's grids; then the remaining transform sizes (row pass at 128, 256, 512; column pass at 256, 512, 1024:
# dif_split and the barrier form); then grids where ONE axis has a hand-written size: the pass of that axis runs only when the other axis
# divides into its workgroups (96 x 64 and 64 x 48: mixed; 48 x 64, 100 x 128: the library for both; 64 x 40: mixed in
# fp64, whose column pass takes 8 columns, the library in fp32, whose column pass takes 16)
GRIDS = [(64, 64), (128, 64), (64, 1024), (48, 40), (256, 512), (1024, 64), (512, 128), (128, 256), (96, 64), (64, 48), (48, 64), (64, 40), (100, 128)]
SIZES = (64, 128, 256, 512, 1024)


def expected_kernel(points, dtype):
    """the path csrc/gpe_obs.hip takes: per axis, hand-written when its length is covered and the other axis divides into
    the pass's workgroups (row: 256 / (ny / points per thread) lines; column: 16 (fp32) or 8 (fp64) columns, fewer
    when the workgroup would pass 512 / 256 threads)"""
    nx, ny = points
    tt = lambda n: n // (16 if n > 512 else 8)
    c, cap = (16, 512) if dtype == np.float32 else (8, 256)
    row = ny in SIZES and nx % (256 // tt(ny)) == 0
    col = nx in SIZES and ny % (cap // tt(nx) if c * tt(nx) > cap else c) == 0
    return "gpe_obs_fused_lds_fft" if row and col else "gpe_obs_mixed" if row or col else "gpe_obs_rocfft_1d"

KS, OMEGAS, E = (50.0, 20.0, 80.0), (0.7, 0.0, -0.4), 0.1
T_SPOTS = 0.3
SPOTS = P.GaussianSpots([P.GaussianSpot(3.0, 1.5, -1.0, 0.8, 0.5, -0.6, 0.9), P.GaussianSpot(-2.0, 0.7, 1.2, -0.5, -0.8, 0.4, 1.3)])
TOL = {np.float32: 5e-6, np.float64: 1e-12}
# (equation class, batch, kinetic, per-environment e)
CONFIGS = {"rot-b3": ("rot", 3, True, False), "rot-b1": ("rot", 1, True, False), "rot-b3-e": ("rot", 3, True, True),
           "control-b3-kinetic": ("control", 3, True, False), "control-b1": ("control", 1, False, False)}


def domain(points, half=6.0):
    return P.Domain(tuple(points), ((-half, half), (-half, half)), "dimensionless")


@pytest.fixture(scope="module")
def engine():
    eng = HipEngine(0)
    yield eng
    eng.close()


def model_for(kind, dom, engine):
    m = (P.PDEModel(P.GPE2DTSRot, dom, P.RotatingStrangSplitting) if kind == "rot"
         else P.PDEModel(P.GPE2DTSControl, dom, P.StrangSplitting))
    m._engine = engine
    return m


def case(config, dom):
    """(kind, parameter dicts, per environment (k, omega, V), kappa, t)"""
    kind, batch, kinetic, per_env_e = CONFIGS[config]
    es = [E + 0.15 * b if per_env_e else E for b in range(batch)]
    x, y = dom.mesh()
    if kind == "rot":
        params = [dict(k=KS[b], e=es[b], omega=OMEGAS[b]) for b in range(batch)]
        env = [(KS[b], OMEGAS[b], R.trap(dom, es[b])) for b in range(batch)]
        return kind, params, env, 1.0, 0.0
    params = [dict(k=KS[b], e=es[b], lights=SPOTS, kinetic=kinetic) for b in range(batch)]
    env = [(KS[b], 0.0, R.trap(dom, es[b]) + SPOTS(T_SPOTS, x, y)) for b in range(batch)]
    return kind, params, env, 1.0 if kinetic else 0.0, T_SPOTS


@functools.lru_cache(maxsize=None)
def states(points, batch):
    psi = RR.smooth_state(domain(points), 3, batch)
    psi.setflags(write=False)
    return psi


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("points", GRIDS)
def test_observables_against_the_reference(engine, points, dtype, config):
    dom = domain(points)
    kind, params, env, kappa, t = case(config, dom)
    psi = states(points, len(params))
    obs = model_for(kind, dom, engine).observables(params if len(params) > 1 else params[0], RR.to_pairs(psi).astype(dtype), t)
    kernel = engine.last_kernel
    assert kernel == expected_kernel(points, dtype)
    worst = {}
    for b, (k, omega, V) in enumerate(env):
        vals, scales = R.observables(dom, psi[b], V, k)
        for name in R.NAMES:
            worst[name] = max(worst.get(name, 0.0), abs(obs[name][b] - vals[name]) / scales[name])
        energy, mu = R.derived(vals, omega, kappa)
        total = (scales["e_kin"] + scales["e_pot"] + 2 * scales["e_int"] + abs(omega) * scales["l_z"]) / vals["norm"]
        worst["energy"] = max(worst.get("energy", 0.0), abs(obs.energy[b] - energy) / total)
        worst["mu"] = max(worst.get("mu", 0.0), abs(obs.mu[b] - mu) / total)
    print(f"{np.dtype(dtype).name} {points} {config} {kernel}: " + ", ".join(f"{n} {v:.2e}" for n, v in worst.items()))
    for name, v in worst.items():
        assert v <= (2 if name in ("energy", "mu") else 1) * TOL[dtype], name


@pytest.mark.parametrize("points,dtype", [((128, 64), np.float32), ((64, 64), np.float64), ((48, 40), np.float32),
                                          ((48, 64), np.float32), ((64, 40), np.float32), ((64, 40), np.float64),
                                          ((96, 64), np.float32)])
def test_state_untouched_repeat_and_sub_range_bitwise(engine, points, dtype):
    dom = domain(points)
    kind, params, _, _, _ = case("rot-b3", dom)
    y = RR.to_pairs(states(points, 3)).astype(dtype)
    model_for(kind, dom, engine).observables(params, y, 0.0)
    full = engine.gpe_observables()
    assert np.array_equal(engine.get_state(), y)
    assert np.array_equal(engine.gpe_observables(), full)
    assert np.array_equal(engine.gpe_observables(env_first=1, env_count=1), full[1:2])
    assert np.array_equal(engine.gpe_observables(env_first=2), full[2:])
    assert np.all(full[:, 7] == 0.0) and np.all(np.isfinite(full))
    with pytest.raises(ValueError):
        engine.gpe_observables(env_first=2, env_count=2)


def test_after_a_solve_the_resident_state_is_read_without_an_upload(engine):
    dom = domain((64, 64))
    m = model_for("control", dom, engine)
    params = dict(k=50.0, e=0.1, lights=lambda t, x, y: 0.3 * np.exp(-(x**2 + y**2)), kinetic=True)
    y0 = RR.to_pairs(states((64, 64), 1)[0])
    ys = m.solve(params, y0, [0.0, 0.02], dt0=2e-3)
    raw = engine.gpe_observables()
    x, y = dom.mesh()
    vals, scales = R.observables(dom, RR.from_pairs(ys[-1]), R.trap(dom, 0.1) + params["lights"](0.0, x, y), 50.0)
    for i, name in enumerate(R.NAMES):
        assert abs(raw[0, i] - vals[name]) <= 1e-12 * scales[name], name


def test_other_problems_are_refused(engine):
    engine.configure(equation=P._lib.EQ_ALLEN_CAHN, dtype=np.float32, nx=64, ny=64, batch=1, hx=0.1, hy=0.1)
    engine.gpe_origin = (0.0, 0.0)
    with pytest.raises(ValueError, match="GPE"):
        engine.gpe_observables()


# ---- ground state ------------------------------------------------------------------------------------------------------

GS_DOM = P.Domain((64, 64), ((-8.0, 8.0), (-8.0, 8.0)), "dimensionless")
GS_CASES = {"harmonic-rotating": (0.0, 0.3, 0.0), "interacting": (50.0, 0.0, 0.1)}  # (k, omega, e)
DT = 0.01


def gs_start():
    x, y = GS_DOM.mesh()
    return np.exp(-((x - 0.7) ** 2 + (y + 0.4) ** 2) / 3).astype(complex)


@functools.lru_cache(maxsize=None)
def numpy_ground_state(name):
    k, omega, e = GS_CASES[name]
    _, steps, conv, hist = R.ground_state_loop(RR.RotCase(GS_DOM, k, e, omega, time_scale=-1j), GS_DOM, gs_start(), k, omega, DT)
    assert conv
    return steps, hist


def check_against_numpy(name, steps, energy, mu):
    want_steps, hist = numpy_ground_state(name)
    assert abs(int(steps) - want_steps) <= 25, (steps, want_steps)  # the criterion sits on a threshold: one block
    e_ref, mu_ref = hist[-1]
    print(f"ground state {name}: {steps} steps (numpy {want_steps}), energy {energy:.10f} (numpy {e_ref:.10f}), "
          f"mu {mu:.10f} (numpy {mu_ref:.10f})")
    assert abs(energy - e_ref) <= 1e-8 and abs(mu - mu_ref) <= 1e-8


@pytest.mark.parametrize("name", list(GS_CASES))
def test_ground_state_converges_like_the_numpy_loop(engine, name):
    k, omega, e = GS_CASES[name]
    if name == "interacting":  # Omega = 0: the Strang step with the kinetic A_term
        m, params = model_for("control", GS_DOM, engine), dict(k=k, e=e, lights=lambda t, x, y: 0.0 * x, kinetic=True)
    else:
        m, params = model_for("rot", GS_DOM, engine), dict(k=k, e=e, omega=omega)
    gs = m.ground_state(params, RR.to_pairs(gs_start()), DT, tol=1e-8, check_every=25)
    assert gs.converged.tolist() == [True] and gs.state.shape == (64, 64, 2)
    assert gs.history.shape == (gs.steps[0] // 25, 1, 2)
    check_against_numpy(name, gs.steps[0], gs.observables.energy[0], gs.observables.mu[0])
    assert abs(gs.observables.norm[0] - 1.0) <= 0.2  # renormalised between the half steps: 1 + O(dt)


def test_ground_state_of_a_batch_counts_steps_per_environment(engine):
    params = [dict(k=k, e=e, omega=omega) for k, omega, e in GS_CASES.values()]
    y0 = np.stack([RR.to_pairs(gs_start())] * 2)
    gs = model_for("rot", GS_DOM, engine).ground_state(params, y0, DT, tol=1e-8, check_every=25)
    assert gs.converged.tolist() == [True, True] and gs.state.shape == (2, 64, 64, 2)
    assert gs.history.shape == (gs.steps.max() // 25, 2, 2)
    for b, name in enumerate(GS_CASES):
        row = gs.steps[b] // 25 - 1  # the check at which environment b arrived
        check_against_numpy(name, gs.steps[b], gs.history[row, b, 0], gs.history[row, b, 1])


# ---- device reward -----------------------------------------------------------------------------------------------------

def test_l_z_as_the_device_reward():
    dom = domain((64, 64))
    start = RR.to_pairs(states((64, 64), 3)).astype(np.float32)
    venv = P.VectorPDEEnv(
        3, P.GPE2DTSRot, dom, P.RotatingStrangSplitting, end_time=1.0, step_dt=0.01, numeric_dt=0.002,
        state_to_observation_func=lambda s: np.zeros((1, 64, 64), np.uint8), reward_function=None,
        reset_func=lambda d, seed=0: start[seed], reset_control_value=0.0, update_control_value=lambda off, old: old + off,
        update_control_parameter=lambda old, new: new, action_space_config={"shape": ()},
        static_equation_parameters=dict(k=50.0, e=E), control_equation_parameter_name="omega", solver_parameters={},
        device_reward=("gpe", "l_z"), fetch_observations=False)
    venv.reset(seed=0)
    obs, rewards, _, _, _ = venv.step(list(OMEGAS))
    assert obs is None and rewards.shape == (3,)
    got = venv.states
    for b in range(3):
        vals, scales = R.observables(dom, RR.from_pairs(got[b].astype(np.float64)), R.trap(dom, E), 50.0)
        print(f"l_z reward, environment {b}: {rewards[b]:.8f} (reference {vals['l_z']:.8f}, scale {scales['l_z']:.3f})")
        assert abs(rewards[b] - vals["l_z"]) <= 5e-6 * scales["l_z"]
    venv.close()
