"""ImplicitEuler's spectral preconditioner on the GPU (csrc/implicit.hip, pdeopt_implicit_set_precond) against the numpy
reference tests/implicit_precond_ref.py: the coefficient means, M^-1 v, exactness where the operator has constant
coefficients, one iteration on a linear problem, iteration counts, the implicit equation, mass, repeatability, batches
and refusals.  Problems and tolerances: tests/implicit_problems.py; grids and states: tests/implicit_precond_ref.py."""
import functools

import numpy as np
import pytest

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd.engine import HipEngine
from pde_opt_amd.numerics.closures import POLY, ClosureDesc

import implicit_problems as Q
import implicit_precond_ref as PR
import implicit_ref as R

pytestmark = pytest.mark.gpu

EQS = ("ch", "ac")
DTYPES = (np.float64, np.float32)
EPS32 = float(np.finfo(np.float32).eps)
# fp32 gates: the kernel's distance from the fp64 reference over the float32 numpy route's own distance from it, gated at
# twice the largest ratio measured over the cases of this file on an MI355X:
#   M^-1 v          96 cases, ratios 0.69 .. 1.91, median 1.21
#   A M^-1 v = v    96 cases, ratios 0.57 .. 1.50, median 0.97
#   mass            12 cases (every grid and closure set), ratios 0.28 .. 8.44, median 0.96.  The device's drift is
#                   5e-10 .. 3.0e-9 in every case (at most 0.03 eps max|y|), the reference route's own 6e-11 .. 3.4e-9: the
#                   ratio of two rounding walks, large where the reference's happens to end near zero (96x80)
FP32_MINV_RATIO_GATE = 2.0 * 1.91
FP32_EXACT_RATIO_GATE = 2.0 * 1.50
FP32_MASS_RATIO_GATE = 2.0 * 8.44
# fp32 coefficient means: the sums are fp64, the terms D mu_h' and D are formed from closures evaluated in fp32, each a few
# fp32 roundings off.  The roundings of the cells are independent, so the mean of 1e3 .. 1e4 terms is off by well under one
# eps of the mean term magnitude (measured: at most 0.25 eps for a, 0.02 eps for c), while a wrong closure term or a lost
# cell moves it by 1e-4 of that magnitude or more: gated at 2 eps
FP32_COEF_EPS = 2.0

ESTATE = 6  # PDEOPT_ESTATE (include/pdeopt_hip.h)
LINEAR_MU = ClosureDesc(POLY, 0, (0.1, 1.5))
CONST_D = ClosureDesc(POLY, 0, (0.7,))


@pytest.fixture(scope="module")
def eng():
    e = HipEngine()
    yield e
    e.close()


def _setup(eng, eq, points, closures, y, tol=None, precond="spectral", **kw):
    e = Q.equation(eq, points, closures)
    y = np.asarray(y)
    yb = y[None] if y.ndim == 2 else y
    eng.configure(dtype=yb.dtype, batch=yb.shape[0], **e._engine_problem())
    e._engine_upload(eng, 0.0, 1.0)
    rtol, atol = tol or Q.TOL[yb.dtype.type]
    eng.implicit_configure(rtol, atol, **kw)
    if precond is not None:
        eng.implicit_set_precond(precond)
    eng.set_state(yb)
    return e


def _states(points, batch, dtype):
    """unequal environments: uniform noise in [0.2, 0.8], the noise state, the stripe state"""
    ys = [Q.state(points, 3, dtype), PR.STATES["noise"](points, dtype), PR.STATES["stripe"](points, dtype)]
    return np.stack(ys[:batch])


def _grid_cases():
    """every grid with both batch sizes, spread over the closure sets (every closure set meets every grid)"""
    return [(g, b) for g in PR.GRIDS for b in (1, 3)]


# ---- 1. coefficients ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("closures", list(Q.CLOSURES))
@pytest.mark.parametrize("grid,batch", _grid_cases())
@pytest.mark.parametrize("eq", EQS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_coefficients_match_the_numpy_means(eng, dtype, eq, grid, batch, closures):
    points = PR.GRIDS[grid]
    mu, mob = Q.CLOSURES[closures]
    y = _states(points, batch, dtype)
    _setup(eng, eq, points, closures, y)
    got = eng.implicit_precond_coefs()
    for b in range(batch):
        a, c = PR.coefs(y[b], mu, mob)
        raw, _ = PR.coefs(y[b], mu, mob, clamp=False)
        if dtype == np.float64:
            print(f"coefs f64 {eq} {grid} {closures} env {b}: a {got[b, 0]:.16e} / {a:.16e} (unclamped {raw:.3e}), c {got[b, 1]:.16e} / {c:.16e}")
            assert abs(got[b, 0] - a) <= 1e-13 * abs(a) and abs(got[b, 1] - c) <= 1e-13 * abs(c)
        else:
            u64 = y[b].astype(np.float64)
            D = np.asarray(mob(u64)) * np.ones_like(u64)
            mag_a = float(np.mean(np.abs(D * R.S.closure_dc(mu, u64))))
            print(f"coefs f32 {eq} {grid} {closures} env {b}: |a - ref| / (eps mean|D mu'|) = {abs(got[b, 0] - a) / (EPS32 * mag_a):.3f}, "
                  f"|c - ref| / (eps c) = {abs(got[b, 1] - c) / (EPS32 * c):.3f}")
            assert abs(got[b, 0] - a) <= FP32_COEF_EPS * EPS32 * mag_a
            assert abs(got[b, 1] - c) <= FP32_COEF_EPS * EPS32 * c


# ---- 2. M^-1 v --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("closures", list(Q.CLOSURES))
@pytest.mark.parametrize("grid,batch", _grid_cases())
@pytest.mark.parametrize("eq", EQS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_minv_matches_the_numpy_reference_on_white_noise(eng, dtype, eq, grid, batch, closures):
    points = PR.GRIDS[grid]
    mu, mob = Q.CLOSURES[closures]
    y = _states(points, batch, dtype)
    v = np.random.default_rng(11).standard_normal(y.shape).astype(dtype)
    dt = Q.step_size(eq, points, closures, y[0])
    _setup(eng, eq, points, closures, y)
    got = eng.implicit_precond_apply(dt, v)
    for b in range(batch):
        want = PR.minv(eq, y[b].astype(np.float64), v[b].astype(np.float64), dt, Q.H, Q.H, Q.KAPPA, mu, mob)
        err = float(np.max(np.abs(got[b] - want)))
        scale = float(np.max(np.abs(want)))
        if dtype == np.float64:
            print(f"minv f64 {eq} {grid} {closures} env {b}: err / max|out| = {err / scale:.3e}")
            assert err <= 1e-12 * scale
        else:
            ref32 = PR.minv(eq, y[b], v[b], dt, Q.H, Q.H, Q.KAPPA, mu, mob)
            own = float(np.max(np.abs(ref32.astype(np.float64) - want)))
            print(f"minv f32 {eq} {grid} {closures} env {b}: kernel {err / scale:.3e}, float32 reference {own / scale:.3e}, "
                  f"ratio {err / own:.3f}")
            assert err <= FP32_MINV_RATIO_GATE * own


# ---- 3. exactness at a constant state ---------------------------------------------------------------------------------------
def _constants(eq, closures, batch):
    """constant states at which M is the whole operator: mu_h' > 0 there (no clamp), and for Allen-Cahn with a state-dependent
    R the term -R'(c) mu_h(c) v of J, which M does not carry, has to vanish: c = 1 is a root of the polynomial mu_h"""
    if eq == "ac" and closures == "poly_mob":
        return [1.0] * batch
    return [0.8, 0.7, 0.65][:batch]


@pytest.mark.parametrize("closures", list(Q.CLOSURES))
@pytest.mark.parametrize("grid,batch", _grid_cases())
@pytest.mark.parametrize("eq", EQS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_operator_times_minv_is_the_identity_at_a_constant_state(eng, dtype, eq, grid, batch, closures):
    points = PR.GRIDS[grid]
    mu, mob = Q.CLOSURES[closures]
    y = np.stack([np.full(points, c, dtype) for c in _constants(eq, closures, batch)])
    v = np.random.default_rng(12).standard_normal(y.shape).astype(dtype)
    dt = Q.step_size(eq, points, closures, y[0])
    _setup(eng, eq, points, closures, y)
    back = eng.implicit_apply(dt, eng.implicit_precond_apply(dt, v))
    for b in range(batch):
        assert PR.coefs(y[b], mu, mob, clamp=False)[0] > 0.0  # a condition on the input
        err = float(np.max(np.abs(back[b].astype(np.float64) - v[b])))
        scale = float(np.max(np.abs(v[b])))
        if dtype == np.float64:
            print(f"exact f64 {eq} {grid} {closures} env {b}: err / max|v| = {err / scale:.3e}")
            assert err <= 1e-10 * scale
        else:
            z32 = PR.minv(eq, y[b], v[b], dt, Q.H, Q.H, Q.KAPPA, mu, mob)
            own = float(np.max(np.abs(R.apply_op(eq, y[b], z32, dt, Q.H, Q.H, Q.KAPPA, mu, mob).astype(np.float64) - v[b])))
            print(f"exact f32 {eq} {grid} {closures} env {b}: kernel {err / scale:.3e}, float32 reference {own / scale:.3e}, "
                  f"ratio {err / own:.3f}")
            assert err <= FP32_EXACT_RATIO_GATE * own


# ---- 4. one iteration on a linear problem -----------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,batch", _grid_cases())
@pytest.mark.parametrize("eq", EQS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_problem_takes_one_iteration_per_solve(eng, dtype, eq, grid, batch):
    points = PR.GRIDS[grid]
    cls = P.CahnHilliard2DPeriodic if eq == "ch" else P.AllenCahn2DPeriodic
    e = cls(Q.domain(points), Q.KAPPA, LINEAR_MU, CONST_D)
    y = _states(points, batch, dtype)
    dt = Q.STEP_FACTOR * R.euler_limit(eq, y[0].astype(np.float64), Q.H, Q.H, Q.KAPPA, LINEAR_MU, CONST_D)
    eng.configure(dtype=dtype, batch=batch, **e._engine_problem())
    e._engine_upload(eng, 0.0, 1.0)
    eng.implicit_configure(*Q.TOL[dtype])
    eng.implicit_set_precond("spectral")
    eng.set_state(y)
    st = eng.implicit_advance(dt, 2)
    apps = eng.implicit_precond_count()
    print(f"linear {np.dtype(dtype).name} {eq} {grid} batch {batch}: stats {st.tolist()}, applications {apps.tolist()}")
    for b in range(batch):
        assert st[b, 0] >= 2 and st[b, 1] == st[b, 0]  # exactly one Krylov iteration in every linear solve
        assert apps[b] == st[b, 1] + st[b, 0]  # ... and one cycle: krylov_iterations + cycles


# ---- 5. iteration counts ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference_counts(eq, grid, state, closures, dtype_name):
    dtype = np.dtype(dtype_name).type
    points, mu, mob, y, dt = PR.count_problem(eq, grid, state, closures)
    rtol, atol = Q.TOL[dtype]
    return PR.newton_counts(eq, y.astype(dtype), dt, Q.H, Q.H, Q.KAPPA, mu, mob, rtol, atol, True)[2]


@pytest.mark.parametrize("state", list(PR.STATES))
@pytest.mark.parametrize("closures", list(Q.CLOSURES))
@pytest.mark.parametrize("grid", list(PR.GRIDS))
@pytest.mark.parametrize("eq", EQS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_iteration_counts_at_50x_the_euler_limit(eng, dtype, eq, grid, closures, state):
    points, mu, mob, y, dt = PR.count_problem(eq, grid, state, closures)
    ref = _reference_counts(eq, grid, state, closures, np.dtype(dtype).name)
    y = y.astype(dtype)
    _setup(eng, eq, points, closures, y)
    pre = eng.implicit_advance(dt, 1)[0]
    _setup(eng, eq, points, closures, y, precond=None)
    plain = eng.implicit_advance(dt, 1)[0]
    # as many Newton iterates as the reference, and its Krylov count plus 2 per Newton iterate (CGS2 against MGS, fp32 rounding)
    bound = sum(ref) + 2 * len(ref)
    print(f"counts {np.dtype(dtype).name} {eq} {grid} {closures} {state}: preconditioned {pre.tolist()}, reference {list(ref)}, "
          f"bound {bound}, unpreconditioned {plain.tolist()}")
    assert pre[0] <= len(ref)
    assert pre[1] <= bound
    assert pre[1] < plain[1]


# ---- 6. the implicit equation holds -----------------------------------------------------------------------------------------
def _equation_residual_check(dtype, eq, closures, y0, y1, dt, tag):
    """the criterion of tests/test_gpu_implicit.py"""
    rtol, atol = Q.TOL[dtype]
    mu, mob = Q.CLOSURES[closures]
    y0, y1 = y0.astype(np.float64), y1.astype(np.float64)
    f64 = R.rhs(eq, y1, Q.H, Q.H, Q.KAPPA, mu, mob)
    res = R.rms(y1 - y0 - dt * f64)
    thr = 2.0 * (atol + rtol * R.rms(y1))
    if dtype == np.float32:
        f32 = R.rhs(eq, y1.astype(np.float32), Q.H, Q.H, Q.KAPPA, mu, mob).astype(np.float64)
        extra = 4.0 * R.rms(dt * (f32 - f64))
        print(f"equation f32 {tag}: rms {res:.3e}, threshold {thr:.3e} + {extra:.3e}, ratio {res / (thr + extra):.3f}")
        thr += extra
    else:
        print(f"equation f64 {tag}: rms {res:.3e}, threshold {thr:.3e}")
    assert np.isfinite(y1).all()
    assert res <= thr


@pytest.mark.parametrize("closures", list(Q.CLOSURES))
@pytest.mark.parametrize("grid", list(PR.GRIDS))
@pytest.mark.parametrize("eq", EQS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_implicit_equation_holds_one_and_three_steps(eng, dtype, eq, grid, closures):
    points = PR.GRIDS[grid]
    y = Q.state(points, 1, dtype)
    dt = Q.step_size(eq, points, closures, y)
    _setup(eng, eq, points, closures, y)
    first = None
    for step in range(3):
        y0 = eng.get_state()[0]
        st = eng.implicit_advance(dt, 1, step * dt)
        y1 = eng.get_state()[0]
        first = y1 if first is None else first
        _equation_residual_check(dtype, eq, closures, y0, y1, dt, f"{eq} {grid} {closures} step {step} stats {st[0].tolist()}")
        assert st[0, 0] >= 1 and st[0, 1] >= st[0, 0] and st[0, 3] == st[0, 0] + 1
    if dtype == np.float64:
        rtol, atol = Q.TOL[dtype]
        _setup(eng, eq, points, closures, y, precond=None)
        eng.implicit_advance(dt, 1)
        plain = eng.get_state()[0]
        dist, thr = R.rms(first - plain), 10.0 * (atol + rtol * R.rms(plain))
        print(f"preconditioned - unpreconditioned y1 {eq} {grid} {closures}: rms {dist:.3e}, threshold {thr:.3e}")
        assert dist <= thr


# ---- 7. mass ----------------------------------------------------------------------------------------------------------------
def _drift(y0, yn):
    return abs(float(np.mean(yn.astype(np.float64))) - float(np.mean(y0.astype(np.float64))))


@pytest.mark.parametrize("closures", list(Q.CLOSURES))
@pytest.mark.parametrize("grid", list(PR.GRIDS))
def test_cahn_hilliard_mass_over_20_steps_fp64(eng, grid, closures):
    points = PR.GRIDS[grid]
    y = Q.state(points, 2)
    dt = Q.step_size("ch", points, closures, y)
    _setup(eng, "ch", points, closures, y, krylov_rtol=1e-1)
    eng.implicit_advance(dt, 20)
    yn = eng.get_state()[0]
    drift, gate = _drift(y, yn), 1e-13 * float(np.max(np.abs(yn)))
    print(f"mass f64 {grid} {closures}: drift {drift:.3e}, gate {gate:.3e}")
    assert drift <= gate


@pytest.mark.parametrize("closures", list(Q.CLOSURES))
@pytest.mark.parametrize("grid", list(PR.GRIDS))
def test_cahn_hilliard_mass_over_20_steps_fp32(eng, grid, closures):
    points = PR.GRIDS[grid]
    mu, mob = Q.CLOSURES[closures]
    y = Q.state(points, 2, np.float32)
    dt = Q.step_size("ch", points, closures, y)
    rtol, atol = Q.TOL[np.float32]
    yr = y.copy()
    for _ in range(20):
        yr = PR.newton_counts("ch", yr, dt, Q.H, Q.H, Q.KAPPA, mu, mob, rtol, atol, True, krylov_rtol=1e-1)[0]
    own = _drift(y, yr)
    _setup(eng, "ch", points, closures, y, krylov_rtol=1e-1)
    eng.implicit_advance(dt, 20)
    drift = _drift(y, eng.get_state()[0])
    print(f"mass f32 {grid} {closures}: drift {drift:.3e}, float32 reference route {own:.3e}, ratio {drift / own:.3f}")
    assert drift <= FP32_MASS_RATIO_GATE * own


# ---- 8. determinism and batching --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eq", EQS)
def test_repeat_is_bitwise_and_frames_are_the_step_states(eng, eq):
    points, closures = PR.GRIDS["45x33"], "poly_mob"
    y = np.stack([Q.state(points, 1, np.float32), Q.state(points, 2, np.float32)])
    dt = Q.step_size(eq, points, closures, y[0])
    e = Q.equation(eq, points, closures)
    solver = P.ImplicitEuler(*Q.TOL[np.float32], precond="spectral")
    ts = [dt, 2 * dt, 3 * dt]
    a = P.diffeqsolve(e, solver, t0=0.0, t1=3 * dt, dt0=dt, y0=y, saveat=P.SaveAt(ts=ts), engine=eng)
    b = P.diffeqsolve(e, solver, t0=0.0, t1=3 * dt, dt0=dt, y0=y, saveat=P.SaveAt(ts=ts), engine=eng)
    assert np.array_equal(a.ys, b.ys)
    assert a.stats["krylov_iterations"] == b.stats["krylov_iterations"]
    apps = a.stats["preconditioner_applications"]
    assert apps == b.stats["preconditioner_applications"] and len(apps) == 2
    assert all(n > k for n, k in zip(apps, a.stats["krylov_iterations"]))
    _setup(eng, eq, points, closures, y)
    for k in range(3):
        eng.implicit_advance(dt, 1, k * dt)
        assert np.array_equal(eng.get_state(), a.ys[k]), k
    plain = P.diffeqsolve(e, P.ImplicitEuler(*Q.TOL[np.float32]), t0=0.0, t1=dt, dt0=dt, y0=y, engine=eng)
    assert "preconditioner_applications" not in plain.stats


@pytest.mark.parametrize("grid", ["24x40", "96x80"])
@pytest.mark.parametrize("eq", EQS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_three_unequal_environments_each_satisfy_their_equation(eng, dtype, eq, grid):
    points, closures = PR.GRIDS[grid], "poly_mob"
    y = _states(points, 3, dtype)
    dt = Q.step_size(eq, points, closures, y[0])
    _setup(eng, eq, points, closures, y, restart=5)
    st = eng.implicit_advance(dt, 1)
    out = eng.get_state()
    print(f"per-environment stats {eq} {np.dtype(dtype).name} {grid}: {st.tolist()}, applications {eng.implicit_precond_count().tolist()}")
    for b in range(3):
        _equation_residual_check(dtype, eq, closures, y[b], out[b], dt, f"{eq} {grid} env {b}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_constant_environment_is_left_alone_and_counts_nothing(eng, dtype):
    points = PR.GRIDS["45x33"]
    y = np.stack([Q.state(points, 1, dtype), np.full(points, 0.5, dtype), Q.state(points, 2, dtype)])
    dt = Q.step_size("ch", points, "legendre_logit", y[0])
    _setup(eng, "ch", points, "legendre_logit", y)
    st = eng.implicit_advance(dt, 1)
    out = eng.get_state()
    apps = eng.implicit_precond_count()
    assert st[1].tolist() == [0, 0, 0, 1] and apps[1] == 0
    assert np.array_equal(out[1], y[1])
    assert np.isfinite(out).all() and apps[0] > 0 and apps[2] > 0


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------
def test_set_precond_refuses_what_it_does_not_cover(eng):
    points = PR.GRIDS["24x40"]
    e = Q.equation("ch", points, "poly")
    eng.configure(dtype=np.float64, batch=1, **e._engine_problem())
    with pytest.raises(L.PdeoptError, match="pdeopt_implicit_configure has not been called") as err:
        eng.implicit_set_precond("spectral")
    assert err.value.code == ESTATE
    eng.implicit_configure(1e-10, 1e-12)
    with pytest.raises(ValueError, match="spectral"):
        eng.implicit_set_precond("jacobi")
    with pytest.raises(L.PdeoptError, match="pdeopt_implicit_set_precond"):
        eng.implicit_precond_coefs()  # switched off: nothing to report
    dom3 = P.Domain((8, 8, 8), ((0.0, 1.0),) * 3, "dimensionless")
    e3 = P.CahnHilliard3DPeriodic(dom3, Q.KAPPA, *Q.CLOSURES["poly"])
    eng.configure(dtype=np.float64, batch=1, **e3._engine_problem())
    with pytest.raises(ValueError, match="periodic 2-D Cahn-Hilliard and Allen-Cahn"):
        eng.implicit_set_precond("spectral")
    # a smoothed-boundary problem: the equation code alone decides, before any field of it is needed
    eng.configure(dtype=np.float64, batch=1, **{**e._engine_problem(), "equation": L.EQ_CAHN_HILLIARD_SBM})
    with pytest.raises(ValueError, match="smoothed-boundary"):
        eng.implicit_set_precond("spectral")


def test_a_spent_krylov_budget_raises_and_keeps_the_state(eng):
    points = PR.GRIDS["24x40"]
    y = PR.STATES["stripe"](points)
    dt = 10.0 * Q.step_size("ch", points, "poly_mob", y)
    _setup(eng, "ch", points, "poly_mob", y, max_krylov=1)
    with pytest.raises(P.ImplicitSolveError, match=r"environment 0, step 0.*GMRES"):
        eng.implicit_advance(dt, 1)
    assert np.array_equal(eng.get_state()[0], y)
