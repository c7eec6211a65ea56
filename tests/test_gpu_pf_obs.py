"""The phase-field observables on the MI355X (csrc/pf_obs.hip) against their numpy reference (tests/pf_obs_ref.py).

Gates.  fp64: every entry within 1e-12 x h sum|term| of the reference (the worst-case fp64 summation bound N 2^-53 at
N <= 4096 plus a few ulp per term).  fp32: within 10 x the distance of the fp32-terms reference from the fp64 one, plus
the fp64 gate -- the summation-order bound, which holds whatever the state's dtype and is all that is left where the fp32
terms are exact (MASS).  Both references evaluate the problem the engine holds: an fp32 engine carries kappa and the
coefficients rounded to fp32.  The kernels form every term in fp64 from the stored fp32 values: with fp32 terms the
measured error was 1 to 8 x the reference's own distance, and that distance -- a signed sum of roundings -- falls to a
hundredth of its usual size now and then (MU2 on 8 x 8: 1e-11 beside 2e-9 in the neighbouring environments), which no
fp32 arithmetic can follow.  The measured ratios are recorded in DESIGN.md section 4.19."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import pde_opt_amd as P
import pf_obs_ref as R
from pde_opt_amd import _lib as L
from pde_opt_amd.engine import HipEngine

pytestmark = pytest.mark.gpu

MUS = {
    "poly": R.Closure("poly", (0.1, -1.0, 0.2, 1.0)),
    "legendre": R.Closure("legendre", (0.2, -0.8, 0.3, 0.5, -0.2)),
    "logit": R.Closure("poly", (3.0, -6.0), logit=True),
}
MOBS = {"quadratic": R.Closure("poly", (0.2, 1.0, -1.0)), "exp": R.Closure("poly", (-0.5, 0.8), exp=True)}
EQ_CODE = {"ch": L.EQ_CAHN_HILLIARD, "ac": L.EQ_ALLEN_CAHN, "ch3d": L.EQ_CAHN_HILLIARD_3D}
# 8 x 8: smaller than the 16 x 64 tile (the ring wraps onto the tile itself); 16 x 64: exactly one tile; 33 x 47: partial
# tiles, odd rows, hx != hy; 64 x 64: several tiles
SHAPES_2D = [(8, 8), (16, 64), (33, 47), (64, 64)]
SHAPES_3D = [(4, 6, 8), (9, 10, 11), (16, 16, 16)]


@pytest.fixture(scope="module")
def engine():
    eng = HipEngine(0)
    yield eng
    eng.close()


def spacings(shape):
    return (0.11, 0.07, 0.13)[: len(shape)]


def load(engine, eq, shape, dtype, mu, mob, states, kappa=0.004):
    h = spacings(shape)
    kw = dict(nz=shape[2], hz=h[2]) if len(shape) == 3 else {}
    engine.configure(equation=EQ_CODE[eq], dtype=dtype, nx=shape[0], ny=shape[1], batch=len(states), hx=h[0], hy=h[1],
                     kappa=kappa, mu=mu.desc(), mob=mob.desc(), **kw)
    engine.set_state(states.astype(dtype))
    if dtype == np.float32:  # the problem an fp32 engine holds: kappa and the coefficients rounded to fp32
        r32 = lambda cl: dataclasses.replace(cl, coef=tuple(float(np.float32(v)) for v in cl.coef))
        kappa, mu, mob = float(np.float32(kappa)), r32(mu), r32(mob)
    return dict(eq=eq, h=h, kappa=kappa, mu=mu, mob=mob)


def check_parity(engine, eq, shape, dtype, record=None):
    states = R.smooth_noise_states(shape, 3, seed=sum(shape))
    for mu_name, mu in MUS.items():
        for mob_name, mob in MOBS.items():
            spec = load(engine, eq, shape, dtype, mu, mob, states)
            got = engine.pf_observables()
            want, scale = R.observables(states.astype(dtype), spec)
            floor = 1e-12 * scale
            if dtype == np.float64:
                bound = floor
            else:
                own = np.abs(R.observables(states.astype(dtype), spec, np.float32)[0] - want)
                bound = 10 * own + floor
            err = np.abs(got - want)
            print(eq, shape, np.dtype(dtype).name, mu_name, mob_name, "err / bound per entry:", np.max(err[:, :7] / np.maximum(bound[:, :7], 1e-300), axis=0))
            assert np.all(err[:, :7] <= bound[:, :7]), (mu_name, mob_name, err[:, :7] / np.maximum(bound[:, :7], 1e-300))
            assert np.all(got[:, 7] == 0)
            assert engine.last_kernel.startswith("pf_obs<")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SHAPES_2D)
@pytest.mark.parametrize("eq", ["ch", "ac"])
def test_parity_2d(engine, eq, shape, dtype):
    check_parity(engine, eq, shape, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SHAPES_3D)
def test_parity_3d(engine, shape, dtype):
    check_parity(engine, "ch3d", shape, dtype)


@pytest.mark.parametrize("eq,shape", [("ch", (33, 47)), ("ac", (33, 47)), ("ch3d", (9, 10, 11))])
def test_nonfinite_count_and_bitwise_rows(engine, eq, shape):
    states = R.smooth_noise_states(shape, 3, seed=11)
    load(engine, eq, shape, np.float64, MUS["logit"], MOBS["quadratic"], states)
    full = engine.pf_observables()
    # determinism: a repeat and a sub-range give the same bits
    assert np.array_equal(engine.pf_observables(), full)
    assert np.array_equal(engine.pf_observables(env_first=1, env_count=2), full[1:3])
    assert np.array_equal(engine.pf_observables(env_first=2), full[2:])
    with pytest.raises(ValueError):
        engine.pf_observables(env_first=2, env_count=2)
    bad = states.copy()
    bad[(1,) + tuple(n // 2 for n in shape)] = np.nan
    engine.set_state(bad)
    got = engine.pf_observables()
    # one NaN cell: itself, and the cells whose mu reads it through the Laplacian (4 neighbours in 2-D, 6 in 3-D)
    assert got[1, 7] == 1 + 2 * len(shape) and np.isnan(got[1, 0])
    assert np.array_equal(got[[0, 2]], full[[0, 2]])


def test_per_environment_kappa_and_coefficients(engine):
    dom = P.Domain((33, 47), ((0.0, 33 * 0.11), (0.0, 47 * 0.07)), "dimensionless")
    m = P.PDEModel(P.CahnHilliard2DPeriodic, dom, P.RK4)
    m._engine = engine
    states = R.smooth_noise_states((33, 47), 3, seed=2)
    kappas, slopes = (0.004, 0.01, 0.0007), (-6.0, -5.0, -7.0)
    params = [dict(kappa=k, mu=R.Closure("poly", (3.0, s), logit=True).desc(), D=MOBS["quadratic"].desc()) for k, s in zip(kappas, slopes)]
    obs = m.free_energy(params, states)
    assert obs.free_energy.shape == (3,) and obs.volume == pytest.approx(33 * 0.11 * 47 * 0.07)
    for b, (k, s) in enumerate(zip(kappas, slopes)):
        spec = dict(eq="ch", h=tuple(dom.dx), kappa=k, mu=R.Closure("poly", (3.0, s), logit=True), mob=MOBS["quadratic"])
        want, scale = R.observables(states[b], spec)
        got = np.array([obs[n][b] for n in R.NAMES])
        assert np.all(np.abs(got - want) <= 1e-12 * scale), b
    one = m.free_energy(params[1], states[1])
    assert one.free_energy[0] == obs.free_energy[1] and one.dissipation[0] == obs.dissipation[1]
    with pytest.raises(NotImplementedError, match="GPE2DTSControl"):
        m.observables(params[0], states[0])


TRACE = {
    # (equation class, solver, numpy stepper, parameters, reference spec pieces, dt, state map)
    "imex": (P.CahnHilliard2DPeriodic, P.SemiImplicitFourierSpectral, R.imex_steps, "ch", MUS["logit"], R.Closure("poly", (0.0, 1.0, -1.0)), 5e-6,
             lambda s: s),
    "rk4": (P.AllenCahn2DPeriodic, P.RK4, R.rk4_steps, "ac", R.Closure("poly", (0.0, -1.0, 0.0, 1.0)), R.Closure("poly", (1.0, 0.0, 1.0)), 5e-3,
            lambda s: 2 * s - 1),
}


@pytest.mark.parametrize("which", ["imex", "rk4"])
def test_free_energy_trace(engine, which):
    """200 steps, 5 save points on step edges, 32 x 32, fp64.  ``solve`` issues the same advance calls for the same
    segments, so the rows equal ``free_energy`` of its frames bit for bit"""
    eq_type, solver, stepper, eq, mu, mob, dt, remap = TRACE[which]
    dom = P.Domain((32, 32), ((0.0, 1.0), (0.0, 1.0)), "dimensionless")
    y0 = remap(R.smooth_noise_states((32, 32), 3, seed=5, lo=0.3, hi=0.7))
    spec = dict(eq=eq, h=tuple(dom.dx), kappa=1e-3, mu=mu, mob=mob)
    # the step is small enough that the scheme itself, stepped in numpy, does not raise the free energy
    u, f_ref = y0.copy(), [R.free_energy(y0, spec)]
    for _ in range(4):
        u = stepper(u, spec, dt, 50)
        f_ref.append(R.free_energy(u, spec))
    assert np.all(np.diff(np.array(f_ref), axis=0) < 0)
    m = P.PDEModel(eq_type, dom, solver)
    m._engine = engine
    params = {"kappa": 1e-3, "mu": mu.desc(), ("R" if eq == "ac" else "D"): mob.desc()}
    ts = np.arange(5) * (50 * dt)
    sp = {"A": 0.5} if which == "imex" else {}
    trace = m.free_energy_trace(params, y0, ts, solver_parameters=sp, dt0=dt)
    assert trace.free_energy.shape == (5, 3) and np.all(trace.nonfinite == 0)
    frames = m.solve(params, y0, ts, solver_parameters=sp, dt0=dt)  # (5, 3, 32, 32)
    for q in range(5):
        at = m.free_energy(params, frames[q])
        for name in R.NAMES:
            assert np.array_equal(trace[name][q], at[name]), (q, name)
    assert np.all(np.diff(trace.free_energy, axis=0) < 0)
    np.testing.assert_allclose(trace.free_energy, np.array(f_ref), rtol=1e-9)
    if eq == "ch":  # Cahn-Hilliard conserves the mass
        np.testing.assert_allclose(trace.mass, np.broadcast_to(trace.mass[0], (5, 3)), rtol=1e-12)


def test_the_device_reward_is_the_free_energy(engine):
    dom = P.Domain((64, 64), ((0.0, 1.0), (0.0, 1.0)), "dimensionless")  # (a per-environment kappa under IMEX needs >= 64)
    mu, mob = MUS["logit"].desc(), R.Closure("poly", (0.0, 1.0, -1.0)).desc()
    y0 = R.smooth_noise_states((64, 64), 3, seed=5, lo=0.3, hi=0.7)
    env = P.VectorPDEEnv(3, P.CahnHilliard2DPeriodic, dom, P.SemiImplicitFourierSpectral, end_time=1.0, step_dt=2e-4, numeric_dt=5e-6,
                         state_to_observation_func=lambda s: s, reward_function=None,
                         reset_func=lambda d, seed=0: y0[seed % 3], reset_control_value=1e-3,
                         update_control_value=lambda a, v: v * (1.0 + 0.5 * float(np.ravel(a)[0])), update_control_parameter=lambda old, new: new,
                         action_space_config={"shape": (1,)}, static_equation_parameters=dict(mu=mu, D=mob),
                         control_equation_parameter_name="kappa", solver_parameters={"A": 0.5}, device_reward=("phase_field", "free_energy"),
                         fetch_observations=False, engine=engine)
    env.reset(seed=0)
    m = P.PDEModel(P.CahnHilliard2DPeriodic, dom, P.SemiImplicitFourierSpectral)  # (an engine of its own)
    kappas = np.full(3, 1e-3)
    for _ in range(2):
        actions = np.array([[0.0], [0.4], [-0.4]])
        _, rewards, *_ = env.step(actions)
        kappas = kappas * (1.0 + 0.5 * actions[:, 0])
        states = env.states  # fetched separately
        want = m.free_energy([dict(kappa=float(k), mu=mu, D=mob) for k in kappas], states).free_energy
        assert np.array_equal(np.asarray(rewards), want)
    assert len(set(np.asarray(rewards))) == 3  # every environment was rewarded with its own kappa
    with pytest.raises(NotImplementedError, match="GPE2DTSControl"):
        m.observables(dict(kappa=1e-3, mu=mu, D=mob), y0[0])


def test_the_c_call_refuses_what_it_does_not_cover(engine):
    lib, out = engine._lib, np.zeros((1, 8))
    call = lambda: lib.pdeopt_pf_observables(engine._h, 0, 1, out.ctypes.data_as(C.c_void_p))
    from pde_opt_amd.numerics import closures as CLS

    one = CLS.polynomial(1.0)
    # a smoothed-boundary problem
    engine.configure(equation=L.EQ_CAHN_HILLIARD_SBM, dtype=np.float64, nx=16, ny=16, batch=1, hx=0.1, hy=0.1, kappa=0.01,
                     mu=MUS["logit"].desc(), mob=one, fe=one)
    assert call() == L.EINVAL and b"smoothed-boundary" in lib.pdeopt_last_error(engine._h)
    # a mu with the mixing-entropy flag
    engine.configure(equation=L.EQ_CAHN_HILLIARD, dtype=np.float64, nx=16, ny=16, batch=1, hx=0.1, hy=0.1, kappa=0.01,
                     mu=CLS.ClosureDesc(CLS.POLY, CLS.MIX_ENTROPY, (0.0, 1.0)), mob=one)
    assert call() == L.EINVAL and b"mixing-entropy" in lib.pdeopt_last_error(engine._h)
    engine.configure(equation=L.EQ_CAHN_HILLIARD, dtype=np.float64, nx=16, ny=16, batch=1, hx=0.1, hy=0.1, kappa=0.01,
                     mu=MUS["logit"].desc(), mob=one, derivs=L.DERIVS_FOURIER)
    assert call() == L.EINVAL and b"finite-difference" in lib.pdeopt_last_error(engine._h)
    engine.configure(equation=L.EQ_CAHN_HILLIARD, dtype=np.float64, nx=16, ny=16, batch=1, hx=0.1, hy=0.1, kappa=0.01,
                     mu=MUS["logit"].desc(), mob=one)
    assert call() == L.OK


def test_state_error_before_configure():
    eng = HipEngine(0)
    try:
        out = np.zeros((1, 8))
        assert eng._lib.pdeopt_pf_observables(eng._h, 0, 1, out.ctypes.data_as(C.c_void_p)) == L.ESTATE
    finally:
        eng.close()
