"""The Butler-Volmer Allen-Cahn equations on the GPU (csrc/butler_volmer.hip) against tests/bv_ref.py.

States, closures and spacing are the notebook's (notebooks/run_butler_volmer_sbm.ipynb): clip(0.1 + 0.1 normal, 0.05, 1),
kappa = 0.002 on h = 0.01, mu = logit + 3 (1 - 2c), j0 = sqrt((1 - c) c).  Grids: 5 x 7 (one ragged workgroup whose ring
wraps onto its own tile), 33 x 20 (ragged in both axes), 64 x 96 (several workgroups: more than one partial per
environment), 100 x 100 (the notebook's).  Batches of 1 and of 3 with three currents (voltages) and two kappas.

fp64 gates: 1e-11 of max|rhs| and 1e-11 absolute on v -- a fixed-order fp64 sum of <= 1e4 positive terms is good to
about 1e-12 and the rate's sensitivity to eta is of order one.  fp32: the kernel's distance to the fp64 reference is held
to twice the worst ratio measured against the distance of the SAME reference evaluated in float32 (FP32_RATIO below; the
margin covers the exp / log differences between the device library and numpy).  For v, a single number per environment,
the reference's float32 distance is floored at eps32 (|v| + 1) before the ratio is taken: the recorded 3.16 is a ratio
to that floored distance."""
import types

import numpy as np
import pytest

import bv_ref as R
import pde_opt_amd as P
from pde_opt_amd import _lib as L

pytestmark = pytest.mark.gpu

H = 0.01
KAPPA = 0.002
GRIDS = [(5, 7), (33, 20), (64, 96), (100, 100)]
ALPHAS = [0.5, 0.3]
CS = [0.02, 0.0, -0.01]
KAPPAS3 = [0.002, 0.003, 0.002]
F_SBM = lambda c: c * np.log(c) + (1.0 - c) * np.log(1.0 - c) + 3.0 * c * (1.0 - c) + 0.059  # noqa: E731
# worst measured (kernel - ref64) / (ref32 - ref64) over every fp32 case below, on an MI355X: see DESIGN.md section 4.15
FP32_RATIO = {"rhs": 6.82, "v": 3.16}  # (sbm 64 x 96, alpha 0.5, kappa 0.003; current 5 x 7, C = 0)
ADAPTIVE_SEED = 0  # chosen on the CPU: no error ratio of the reference loop within 0.1 of the accept threshold


def domain(nx, ny, psi=None):
    geo = None if psi is None else types.SimpleNamespace(smooth=psi)
    return P.Domain((nx, ny), ((-H * nx / 2, H * nx / 2), (-H * ny / 2, H * ny / 2)), "dimensionless", geo)


def make_eq(kind, nx, ny, alpha, value, kappa=KAPPA):
    if kind == "voltage":
        return P.AllenCahn2DPeriodicButlerVolmer(domain(nx, ny), kappa, R.MU, R.J0, alpha, v=value)
    if kind == "current":
        return P.AllenCahn2DPeriodicButlerVolmerConstantCurrent(domain(nx, ny), kappa, R.MU, R.J0, alpha, value)
    return P.AllenCahn2DSmoothedBoundaryButlerVolmerConstantCurrent(domain(nx, ny, R.disc_psi(nx, ny)), kappa, F_SBM, R.MU, R.J0,
                                                                    alpha, value)


def ref_rhs(kind, u, alpha, value, kappa=KAPPA):
    u = np.asarray(u)
    if kind == "voltage":
        return R.rhs_voltage(u, H, H, kappa, alpha, value)
    psi = R.disc_psi(*u.shape).astype(u.dtype) if kind == "sbm" else None
    return R.rhs_current(u, H, H, kappa, alpha, value, psi=psi)


def ref_v(kind, u, value, kappa=KAPPA):
    u = np.asarray(u)
    psi = R.disc_psi(*u.shape).astype(u.dtype) if kind == "sbm" else None
    return R.voltage(u, H, H, kappa, value, psi=psi)


def kernel_name(kind):
    return {"voltage": "bv_rate<voltage>", "current": "bv_mu_sums+bv_rate", "sbm": "bv_mu_sums<SBM>+bv_rate"}[kind]


@pytest.fixture(scope="module")
def eng():
    e = P.HipEngine()
    yield e
    e.close()


def load(eng, kind, states, alpha, values, kappas=None):
    """the batch ``states`` with one value (C or v) and one kappa per environment on ``eng``"""
    states = np.asarray(states)
    B, nx, ny = states.shape
    values = np.broadcast_to(np.asarray(values, dtype=np.float64), (B,))
    kappas = np.broadcast_to(np.asarray(KAPPA if kappas is None else kappas, dtype=np.float64), (B,))
    eqs = [make_eq(kind, nx, ny, alpha, float(values[b]), float(kappas[b])) for b in range(B)]
    eng.configure(dtype=states.dtype, batch=B, **eqs[0]._engine_problem())
    eng.set_env_params(0, kappa=kappas)
    type(eqs[0])._engine_upload_batch(eng, eqs)
    eng.set_state(states)
    return eqs


def states_of(nx, ny, B, dtype=np.float64, seed=0):
    return R.notebook_state(np.random.default_rng(seed + 7 * nx + ny), (B, nx, ny), dtype)


KINDS = ["voltage", "current", "sbm"]


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("kind", KINDS)
def test_rhs_and_voltage_fp64(eng, kind, grid):
    nx, ny = grid
    for alpha in ALPHAS:
        for B in (1, 3):
            u = states_of(nx, ny, B)
            values = CS[:B] if kind != "voltage" else [0.05, 0.0, -0.1][:B]
            kappas = KAPPAS3[:B]
            load(eng, kind, u, alpha, values, kappas)
            got = eng.rhs()
            assert eng.last_kernel == kernel_name(kind)
            v_used = eng.bv_voltage(last=True)
            for b in range(B):
                want = ref_rhs(kind, u[b], alpha, values[b], kappas[b])
                err = np.max(np.abs(got[b] - want)) / np.max(np.abs(want))
                print(f"{kind} {nx}x{ny} alpha={alpha} B={B} env {b}: rhs err {err:.2e}")
                assert err <= 1e-11
                if kind != "voltage":
                    vw = ref_v(kind, u[b], values[b], kappas[b])
                    gv = eng.bv_voltage(b, 1)[0]
                    print(f"    v err {abs(gv - vw):.2e}")
                    assert abs(gv - vw) <= 1e-11 and abs(v_used[b] - vw) <= 1e-11
                else:
                    assert v_used[b] == values[b]


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("kind", KINDS)
def test_rhs_and_voltage_fp32(eng, kind, grid):
    nx, ny = grid
    for alpha in ALPHAS:
        u = states_of(nx, ny, 3, np.float32)
        values = CS if kind != "voltage" else [0.05, 0.0, -0.1]
        load(eng, kind, u, alpha, values, KAPPAS3)
        got = eng.rhs().astype(np.float64)
        assert eng.last_kernel == kernel_name(kind)
        for b in range(3):
            want = ref_rhs(kind, u[b].astype(np.float64), alpha, values[b], KAPPAS3[b])
            ref32 = ref_rhs(kind, u[b], np.float32(alpha), np.float32(values[b]), np.float32(KAPPAS3[b])).astype(np.float64)
            d_kernel, d_ref = np.max(np.abs(got[b] - want)), np.max(np.abs(ref32 - want))
            print(f"{kind} {nx}x{ny} alpha={alpha} env {b}: fp32 rhs ratio {d_kernel / d_ref:.3f} (kernel {d_kernel:.2e}, numpy fp32 {d_ref:.2e})")
            assert d_kernel <= 2.0 * FP32_RATIO["rhs"] * d_ref
            if kind != "voltage":
                vw = ref_v(kind, u[b].astype(np.float64), values[b], KAPPAS3[b])
                v32 = float(ref_v(kind, u[b], np.float32(values[b]), np.float32(KAPPAS3[b])))
                gv = eng.bv_voltage(b, 1)[0]
                # v is ONE number: the float32 reference's own distance can be tiny by luck, so it is floored at one float32
                # rounding of |v| + 1 before the ratio is taken (the right-hand side's is a maximum over cells: no floor)
                dv_ref = max(abs(v32 - vw), np.finfo(np.float32).eps * (abs(vw) + 1.0))
                print(f"    fp32 v ratio {abs(gv - vw) / dv_ref:.3f}")
                assert abs(gv - vw) <= 2.0 * FP32_RATIO["v"] * dv_ref


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["current", "sbm"])
def test_bitwise_repeat_batch_and_voltage(eng, kind, dtype):
    nx, ny = 64, 96
    u = states_of(nx, ny, 3, dtype)
    load(eng, kind, u, 0.3, CS, KAPPAS3)
    a = eng.rhs()
    va = eng.bv_voltage(last=True)
    b = eng.rhs()
    assert np.array_equal(a, b) and np.array_equal(va, eng.bv_voltage(last=True))
    # pdeopt_bv_voltage: the same summation order as the right-hand side's second pass
    assert np.array_equal(eng.bv_voltage(), va)
    assert np.array_equal(eng.bv_voltage(1, 2), va[1:])
    # environments 1..2 alone
    load(eng, kind, u[1:], 0.3, CS[1:], KAPPAS3[1:])
    assert np.array_equal(eng.rhs(), a[1:])
    assert np.array_equal(eng.bv_voltage(last=True), va[1:])


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("kind", ["current", "sbm"])
def test_current_constraint_on_the_device(eng, kind, grid):
    nx, ny = grid
    u = states_of(nx, ny, 3)
    load(eng, kind, u, 0.5, CS)
    k = eng.rhs()
    psi = R.disc_psi(nx, ny) if kind == "sbm" else None
    for b, C in enumerate(CS):
        scale = R.current_scale(u[b], H, H, KAPPA, C, psi=psi)
        got = R.total_rate(k[b], H, H, psi)
        print(f"{kind} {nx}x{ny} C={C}: |total - C| / scale = {abs(got - C) / scale:.2e}")
        assert abs(got - C) <= 1e-11 * scale


@pytest.mark.parametrize("grid", [(33, 20), (100, 100)], ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("solver", ["euler", "rk4", "tsit5"])
def test_fixed_step_integrators_fp64(eng, solver, grid):
    nx, ny = grid
    dt, n = 1e-4, 10
    # from the notebook's state relaxed by the notebook's own adaptive solve: on the raw state (rates of 1e5) a fixed
    # step of 1e-4 turns the REFERENCE into NaN (bv_ref.relaxed_state)
    u0 = R.relaxed_state(3, nx, ny)
    eq = make_eq("sbm", nx, ny, 0.5, 0.02)
    S = {"euler": P.Euler, "rk4": P.RK4, "tsit5": P.Tsit5}[solver]
    sol = P.diffeqsolve(eq, S(), t0=0.0, t1=n * dt, dt0=dt, y0=u0, engine=eng)
    assert sol.stats["kernel"] == kernel_name("sbm")
    psi = R.disc_psi(nx, ny)
    want = R.steps(lambda t, y: R.rhs_current(y, H, H, KAPPA, 0.5, 0.02, psi=psi), u0, dt, n, solver)
    assert np.all(np.isfinite(want))
    err = np.max(np.abs(sol.ys[-1] - want)) / np.max(np.abs(want))
    print(f"{solver} {nx}x{ny}: {err:.2e}")
    assert err <= 1e-10


def smooth_state(nx, ny):
    """a smooth state with rates of order one: fixed steps of 1e-4 are well inside the stability limit"""
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return 0.2 + 0.05 * np.sin(2 * np.pi * i / nx) * np.cos(2 * np.pi * j / ny)


@pytest.mark.parametrize("solver", ["euler", "rk4", "tsit5"])
def test_voltage_protocol_is_sampled_at_the_stage_times(eng, solver):
    """the given-voltage class with a callable v(t): every stage of every substep sees v at its own time"""
    nx, ny = 33, 20
    dt, n = 1e-4, 10
    ramp = lambda t: 0.1 + 300.0 * t  # noqa: E731  (v moves by 0.3 over the solve: 0.03 per substep)
    u0 = smooth_state(nx, ny)
    eq = P.AllenCahn2DPeriodicButlerVolmer(domain(nx, ny), KAPPA, R.MU, R.J0, 0.3, v=ramp)
    S = {"euler": P.Euler, "rk4": P.RK4, "tsit5": P.Tsit5}[solver]
    sol = P.diffeqsolve(eq, S(), t0=0.0, t1=n * dt, dt0=dt, y0=u0, engine=eng)
    assert sol.stats["kernel"] == kernel_name("voltage")
    f = lambda t, y: R.rhs_voltage(y, H, H, KAPPA, 0.3, ramp(t))  # noqa: E731
    want = R.steps(f, u0, dt, n, solver)
    frozen = R.steps(lambda t, y: R.rhs_voltage(y, H, H, KAPPA, 0.3, ramp(0.0)), u0, dt, n, solver)
    assert np.all(np.isfinite(want)) and np.max(np.abs(want - frozen)) > 1e-6  # the ramp matters
    err = np.max(np.abs(sol.ys[-1] - want)) / np.max(np.abs(want))
    print(f"v(t) {solver}: {err:.2e}")
    assert err <= 1e-10
    # a number again afterwards: the protocol does not linger on the engine
    const = P.AllenCahn2DPeriodicButlerVolmer(domain(nx, ny), KAPPA, R.MU, R.J0, 0.3, v=0.1)
    got = P.diffeqsolve(const, S(), t0=0.0, t1=n * dt, dt0=dt, y0=u0, engine=eng).ys[-1]
    assert np.max(np.abs(got - frozen)) <= 1e-10 * np.max(np.abs(frozen))


def test_long_advance_replays_a_graph_and_follows_new_parameters(eng):
    """constant current has no time term: 64 Euler substeps run from a captured graph, and a new alpha / current after
    it is what the next advance uses"""
    nx, ny = 33, 20
    dt, n = 1e-5, 64
    u0 = smooth_state(nx, ny)
    for alpha, C in ((0.5, 0.02), (0.3, -0.01)):
        eq = make_eq("current", nx, ny, alpha, C)
        sol = P.diffeqsolve(eq, P.Euler(), t0=0.0, t1=n * dt, dt0=dt, y0=u0, engine=eng)
        assert sol.stats["kernel"] == kernel_name("current") + "+hipGraph"
        want = R.steps(lambda t, y: R.rhs_current(y, H, H, KAPPA, alpha, C), u0, dt, n, "euler")
        err = np.max(np.abs(sol.ys[-1] - want)) / np.max(np.abs(want))
        print(f"graph alpha={alpha} C={C}: {err:.2e}")
        assert err <= 1e-10


def test_adaptive_solve_first_trial_steps(eng):
    """the first 40 trial steps of the notebook's solve: the accept / reject sequence and two saved states"""
    from pde_opt_amd.integrate import _clip_dt, _pid_update

    nx = ny = 100
    c = P.PIDController(rtol=1e-4, atol=1e-6)
    u0 = R.notebook_state(np.random.default_rng(ADAPTIVE_SEED), (nx, ny))
    psi = R.disc_psi(nx, ny)
    f = lambda t, y: R.rhs_current(y, H, H, KAPPA, 0.5, 0.02, psi=psi)  # noqa: E731
    n_trials, t1 = 40, 10.0
    acc0, _, _, t_end = R.adaptive(f, u0, 0.0, t1, 1e-6, c, n_trials)
    save_ts = [0.4 * t_end, 0.8 * t_end]  # two save times inside the prefix
    accepts, errs, saves, _ = R.adaptive(f, u0, 0.0, t1, 1e-6, c, n_trials, save_ts)
    assert accepts == acc0 and len(saves) == 2
    close = [e for e in errs if abs(e - 1.0) <= 1e-6]
    if close:
        pytest.skip(f"the reference loop has a step whose error ratio {close[0]!r} lies within 1e-6 of the accept threshold")
    eq = make_eq("sbm", nx, ny, 0.5, 0.02)
    eng.configure(dtype=np.float64, batch=1, **eq._engine_problem())
    eq._engine_upload(eng, 0.0, t1)
    eng.set_state(u0)
    assert not eng.tsit5_solve_small_supported()  # host-driven trial / commit loop
    t, dt, prev, pprev, qi = 0.0, 1e-6, 1.0, 1.0, 0
    got_accepts, got_saves = [], []
    for _ in range(n_trials):
        h = min(dt, t1 - t)
        en = float(np.max(eng.tsit5_trial(t, h, c.rtol, c.atol)))
        assert eng.last_kernel == kernel_name("sbm")
        keep, fac, inv = _pid_update(c, en, prev, pprev)
        got_accepts.append(keep)
        if keep:
            while qi < 2 and save_ts[qi] <= (t + h) + 1e-14 * max(1.0, abs(t + h)):
                got_saves.append(eng.tsit5_dense(min(1.0, max(0.0, (save_ts[qi] - t) / h)), h)[0])
                qi += 1
        eng.tsit5_commit(keep)
        if keep:
            t, pprev, prev = t + h, prev, inv
        dt = _clip_dt(c, h * fac)
    assert got_accepts == accepts
    assert len(got_saves) == 2
    for g, w in zip(got_saves, saves):
        print(f"adaptive save: {np.max(np.abs(g - w)):.2e}")
        assert np.max(np.abs(g - w)) <= 1e-9


def test_large_batch_does_not_take_the_one_cu_kernel(eng):
    u = states_of(64, 64, 256, np.float32)
    eq = make_eq("current", 64, 64, 0.5, 0.02)
    sol = P.diffeqsolve(eq, P.RK4(), t0=0.0, t1=4e-8, dt0=1e-8, y0=u, engine=eng)  # (rates of 1e5 on the raw state)
    assert sol.stats["kernel"] == kernel_name("current")
    assert np.all(np.isfinite(sol.ys[-1]))


def test_refusals(eng):
    eq = make_eq("current", 16, 16, 0.5, 0.02)
    prob = eq._engine_problem()
    with pytest.raises(ValueError, match="finite-difference"):
        eng.configure(dtype=np.float64, batch=1, **{**prob, "derivs": L.DERIVS_FOURIER})
    eng.set_halo_layout(4)
    try:
        with pytest.raises(ValueError, match="periodic layout"):
            eng.configure(dtype=np.float64, batch=1, **prob)
    finally:
        eng.set_halo_layout(0)
    eng.configure(dtype=np.float64, batch=1, **prob)
    with pytest.raises(L.PdeoptError, match="pdeopt_set_bv_params"):
        eng.rhs()  # parameters not set yet
    eq._engine_upload(eng)
    eng.set_state(states_of(16, 16, 1))
    for integ in (L.INT_IMEX, L.INT_STRANG):
        with pytest.raises(ValueError):
            eng.advance(integ, 1e-6, 1)
    # SQRT_WRAP is j0's: as mu the library refuses it for these equations too
    with pytest.raises(ValueError, match="SQRT_WRAP"):
        eng.configure(dtype=np.float64, batch=1, **{**prob, "mu": eq._mob_desc})
    # ... and it belongs to these kernels: Allen-Cahn refuses it in the library too
    ac = P.AllenCahn2DPeriodic(domain(16, 16), KAPPA, R.MU, lambda c: 1.0 + 0 * c)
    with pytest.raises(ValueError, match="SQRT_WRAP"):
        eng.configure(dtype=np.float64, batch=1, **{**ac._engine_problem(), "mob": eq._mob_desc})


def test_vector_env_with_per_environment_current():
    nx, ny = 33, 20
    dom = domain(nx, ny, R.disc_psi(nx, ny))
    reset = lambda d, seed=0: R.relaxed_state(seed, *d.points)  # noqa: E731  (fixed steps: see test_fixed_step_integrators_fp64)
    kw = dict(
        equation_type=P.AllenCahn2DSmoothedBoundaryButlerVolmerConstantCurrent, domain=dom, solver_type=P.RK4, end_time=3e-4,
        step_dt=1e-4, numeric_dt=2e-5, state_to_observation_func=lambda s: np.clip(s * 255, 0, 255).astype(np.uint8)[None],
        reward_function=lambda s: float(np.mean(s)), reset_func=reset, reset_control_value=0.01,
        update_control_value=lambda off, old: old + off, update_control_parameter=lambda old, new: new,
        action_space_config={"type": "discrete", "num_actions": 3, "action_mapping": {0: -0.02, 1: 0.0, 2: 0.01}},
        static_equation_parameters={"kappa": KAPPA, "f": F_SBM, "mu": R.MU, "j0": R.J0, "alpha": 0.5},
        control_equation_parameter_name="Crate", solver_parameters={})
    venv = P.VectorPDEEnv(3, **kw)
    venv.reset(seed=4)
    venv.step([0, 1, 2])
    states = venv.states
    psi = R.disc_psi(nx, ny)
    for b, C in enumerate((-0.01, 0.01, 0.02)):
        e = P.PDEEnv(**kw)
        e.reset(seed=4 + b)
        e.step(b)
        np.testing.assert_array_equal(states[b], e._state)  # one step equal to the single solve
        want = R.steps(lambda t, y, C=C: R.rhs_current(y, H, H, KAPPA, 0.5, C, psi=psi), reset(dom, 4 + b), 2e-5, 5, "rk4")
        assert np.max(np.abs(states[b] - want)) <= 1e-10 * np.max(np.abs(want))
        e.close()
    with pytest.raises(ValueError, match="cannot differ"):
        bad = P.VectorPDEEnv(2, **{**kw, "control_equation_parameter_name": "alpha", "reset_control_value": 0.5,
                                   "static_equation_parameters": {"kappa": KAPPA, "f": F_SBM, "mu": R.MU, "j0": R.J0, "Crate": 0.02}})
        bad.reset(seed=1)
        bad.step([0, 2])
    venv.close()
