"""Allen-Cahn forward-mode sensitivities on the MI355X: the tangent-linear right-hand side and Euler / RK4 tangent
trajectories against the numpy reference (tests/sens_ref_ac.py) and against central differences of GPU forward solves,
the base field against PDEModel.solve, the Gauss-Newton sums, the launch count, and PDEModel.train on synthetic data."""
import numpy as np
import pytest

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd import fit
from pde_opt_amd.engine import HipEngine
from pde_opt_amd.numerics.closures import EXP_WRAP, LEGENDRE, LOGIT_PRIOR, POLY, ClosureDesc
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg
import ac_fit_problem as F
import sens_ref_ac as S

pytestmark = pytest.mark.gpu

KAPPA = 0.002
PARAMS = [(S.MU_ROLE, 0), (S.MU_ROLE, 2), (S.R_ROLE, 0), (S.R_ROLE, 1)]
CLOSURES = {
    # Legendre series under the logit prior, exp-wrapped Legendre rate
    "legendre_logit_exp": (ClosureDesc(LEGENDRE, LOGIT_PRIOR, (0.2, -3.0, 0.4)), ClosureDesc(LEGENDRE, EXP_WRAP, (-0.3, 0.2))),
    # plain polynomials
    "poly": (ClosureDesc(POLY, 0, (0.1, -1.0, 0.5, 1.0)), ClosureDesc(POLY, 0, (1.0, 0.2, 0.3))),
}
# the tangent kernel's tile is 16 x 32
SHAPES = {
    "8x8": ((8, 8), ((0.0, 1.0), (0.0, 1.0))),        # smaller than a tile both ways: the wrap takes the modulo path
    "16x32": ((16, 32), ((0.0, 1.0), (0.0, 1.0))),    # exactly one tile: the ring wraps onto the tile itself
    "33x47": ((33, 47), ((0.0, 1.0), (0.0, 1.0))),    # partial tiles, a wrap that crosses a tile edge, odd row length
    "64x64": ((64, 64), ((0.0, 1.0), (0.0, 2.0))),    # several full tiles (the 16-byte row loads), hx != hy
}


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def _state(shape, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return np.clip(0.5 + 0.1 * rng.standard_normal(shape), 0.1, 0.9).astype(dtype)


def _sens_engine(eq, base, tangents, params):
    eng = HipEngine()
    B = base.shape[0]
    eng.configure(dtype=base.dtype, batch=(1 + len(params)) * B, **eq._engine_problem())
    eq._engine_upload(eng, 0.0, 1.0)
    eng.sens_configure(B, params)
    eng.set_state(np.concatenate([base, tangents]))
    return eng


@pytest.mark.parametrize("closures", list(CLOSURES))
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-11), (np.float32, 1e-4)])  # test_gpu_sens.py's, per dtype
def test_tangent_rhs_matches_numpy_reference(dtype, tol, shape, closures):
    points, box = SHAPES[shape]
    mu, R = CLOSURES[closures]
    dom = P.Domain(points, box, "dimensionless")
    hx, hy = dom.dx
    eq = P.AllenCahn2DPeriodic(dom, KAPPA, mu, R)
    B = 2
    base = np.stack([_state(points, 1 + b, dtype) for b in range(B)])
    tang = (0.05 * np.random.default_rng(7).standard_normal((len(PARAMS) * B,) + points)).astype(dtype)
    eng = _sens_engine(eq, base, tang, PARAMS)
    k = eng.sens_rhs()
    for b in range(B):
        u = base[b].astype(np.float64)
        assert _rel(k[b], S.ac_rhs(u, hx, hy, KAPPA, mu, R)) <= max(tol, 1e-12)
        for j, (role, kc) in enumerate(PARAMS):
            du = tang[j * B + b].astype(np.float64)
            want = S.tangent_rhs(u, du, hx, hy, KAPPA, mu, R, role, kc)
            assert _rel(k[B + j * B + b], want) <= tol, (b, j)


MU3, R2 = (0.1, -3.0, 0.4), (-0.3, 0.2)
TRAJ_PARAMS = [(S.MU_ROLE, 0), (S.MU_ROLE, 1), (S.MU_ROLE, 2), (S.R_ROLE, 0), (S.R_ROLE, 1)]


def _domain(n):
    return P.Domain((n, n), ((0.0, 1.0), (0.0, 1.0)), "dimensionless")


def _equation(n, mu=MU3, R=R2):
    return P.AllenCahn2DPeriodic(_domain(n), KAPPA, ChemLeg(np.array(mu), F.logit), DiffLeg(np.array(R)))


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_tangent_trajectories_200_substeps(integrator):
    n, dt = 64, 1e-3
    eq = _equation(n)
    h = 1.0 / n
    u0 = F.smooth_state(n, 3)
    code = L.INT_EULER if integrator == "euler" else L.INT_RK4
    Pn = len(TRAJ_PARAMS)
    eng = _sens_engine(eq, u0[None], np.zeros((Pn, n, n)), TRAJ_PARAMS)
    eng.sens_advance(code, dt, 200)
    got = eng.get_state()
    u_ref, dus = S.trajectory(u0, TRAJ_PARAMS, dt, 200, h, h, KAPPA, eq._mu_desc, eq._mob_desc, integrator)
    assert _rel(got[0], u_ref) <= 1e-12
    for j in range(Pn):
        assert _rel(got[1 + j], dus[j]) <= 1e-10, j
    # central differences of GPU forward solves: 2 P environments with their own coefficients +- eps
    eps = 1e-4
    fwd = HipEngine()
    fwd.configure(dtype=np.float64, batch=2 * Pn, **eq._engine_problem())
    eq._engine_upload(fwd, 0.0, 1.0)
    mu_c = np.tile(np.array(eq._mu_desc.coef), (2 * Pn, 1))
    R_c = np.tile(np.array(eq._mob_desc.coef), (2 * Pn, 1))
    for j, (role, kc) in enumerate(TRAJ_PARAMS):
        arr = mu_c if role == S.MU_ROLE else R_c
        arr[2 * j, kc] += eps
        arr[2 * j + 1, kc] -= eps
    fwd.set_env_params(0, mu_coef=mu_c, mob_coef=R_c)
    fwd.set_state(np.stack([u0] * (2 * Pn)))
    fwd.advance(code, dt, 200)
    ends = fwd.get_state()
    for j in range(Pn):
        cd = (ends[2 * j] - ends[2 * j + 1]) / (2 * eps)
        assert _rel(got[1 + j], cd) <= 1e-6, j


@pytest.mark.parametrize("solver", ["Euler", "RK4"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_base_field_equals_solve_bitwise(dtype, solver):
    n = 64
    solver_type = getattr(P, solver)
    model = P.PDEModel(P.AllenCahn2DPeriodic, _domain(n), solver_type)
    params = {"mu": ChemLeg(np.array([0.1, -3.0, 0.2]), F.logit), "R": DiffLeg(np.array([-0.2, 0.1])), "kappa": KAPPA}
    y0s = np.stack([F.smooth_state(n, s).astype(dtype) for s in (1, 2)])
    ts = np.array([0.0, 3.3e-2, 1.0e-1, 1.37e-1])  # save points inside steps and a remainder step (dt0 = 1e-2)
    want = model.solve(params, y0s, ts, {}, dt0=1e-2)
    eq = P.AllenCahn2DPeriodic(_domain(n), **params)
    pm = fit.ParamMap.of({"mu": params["mu"], "R": params["R"]}, P.AllenCahn2DPeriodic)
    _, fields = fit.sensitivity_solve(HipEngine(), eq, solver_type(), y0s, ts, pm.sens_params(), dt0=1e-2, fields=True)
    assert fields.dtype == want.dtype
    np.testing.assert_array_equal(fields[:, :2], want)


@pytest.mark.parametrize("solver", ["Euler", "RK4"])
def test_residuals_mse_and_bitwise_sums(solver):
    n = 64
    solver_type = getattr(P, solver)
    model = P.PDEModel(P.AllenCahn2DPeriodic, _domain(n), solver_type)
    truth = {"mu": ChemLeg(np.array([0.1, -3.0]), F.logit), "R": DiffLeg(np.array([5.0])), "kappa": KAPPA}
    y0s = np.stack([F.smooth_state(n, s) for s in (4, 5)])
    ts = np.array([0.0, 2.5e-5, 6e-5])
    values = np.swapaxes(model.solve(truth, y0s, ts, {}, dt0=1e-5), 0, 1)[:, 1:]
    guess = {"mu": ChemLeg(np.array([0.2, -2.5]), F.logit), "R": DiffLeg(np.array([5.2])), "kappa": KAPPA}
    weights = {"mu": ChemLeg(np.array([1.0, 1.0])), "R": DiffLeg(np.array([2.0]))}
    r, reg = model.residuals(guess, (y0s, values), {}, ts, weights, 0.5)
    pred = model.solve(guess, y0s, ts, {})
    np.testing.assert_array_equal(r, values - np.swapaxes(pred, 0, 1)[:, 1:])
    assert abs(reg - 0.5 * (0.04 + 6.25 + 2 * 27.04)) < 1e-12
    m = model.mse(guess, (y0s, values), {}, ts, weights, 0.5)
    assert abs(m - (np.mean(r ** 2) + reg)) <= 1e-12 * abs(m)
    # the Gauss-Newton sums against sums over the fetched fields, and bitwise-equal on a repeat
    eq = P.AllenCahn2DPeriodic(_domain(n), **guess)
    pm = fit.ParamMap.of({"mu": guess["mu"], "R": guess["R"]}, P.AllenCahn2DPeriodic)
    frames = np.ascontiguousarray(np.swapaxes(values, 0, 1))
    eng = HipEngine()
    s1, fields = fit.sensitivity_solve(eng, eq, solver_type(), y0s, ts, pm.sens_params(), dt0=1e-5, fields=True, frames=frames)
    s2, _ = fit.sensitivity_solve(eng, eq, solver_type(), y0s, ts, pm.sens_params(), dt0=1e-5, frames=frames)
    assert s1.tobytes() == s2.tobytes()
    assert eng.sens_accumulate(1).tobytes() == eng.sens_accumulate(1).tobytes()  # pdeopt_sens_accumulate twice
    B, Pn = 2, len(pm.sens_params())
    assert Pn == 3  # mu's constant coefficient has a tangent
    rr = frames - fields[1:, :B]
    tang = [fields[1:, B + j * B: B + (j + 1) * B] for j in range(Pn)]
    ssr, rdp, G = fit.unpack_sums(s1, Pn)
    assert abs(ssr - np.sum(rr ** 2)) <= 1e-10 * ssr
    # the residuals assembled from solve give the same sum of squares
    assert abs(ssr - np.sum((values - np.swapaxes(model.solve(guess, y0s, ts, {}, dt0=1e-5), 0, 1)[:, 1:]) ** 2)) <= 1e-10 * ssr
    for i in range(Pn):
        assert np.sum(tang[i] ** 2) > 0
        assert abs(rdp[i] - np.sum(rr * tang[i])) <= 1e-10 * np.sqrt(ssr * np.sum(tang[i] ** 2))
        for j in range(Pn):
            assert abs(G[i, j] - np.sum(tang[i] * tang[j])) <= 1e-10 * np.sqrt(np.sum(tang[i] ** 2) * np.sum(tang[j] ** 2))


@pytest.mark.parametrize("integrator,per_substep", [("euler", 3), ("rk4", 12)])
def test_launches_per_substep_do_not_depend_on_P(integrator, per_substep):
    n, B = 128, 2
    code = L.INT_EULER if integrator == "euler" else L.INT_RK4
    counts = []
    for params in (TRAJ_PARAMS[:1], TRAJ_PARAMS + [(S.MU_ROLE, 1), (S.R_ROLE, 0)]):
        eq = _equation(n)
        base = np.stack([_state((n, n), b) for b in range(B)])
        eng = _sens_engine(eq, base, np.zeros((len(params) * B, n, n)), params)
        before = eng.stage_launches()
        eng.sens_advance(code, 1e-3, 10)
        counts.append(eng.stage_launches() - before)
    assert counts[0] == counts[1] == 10 * per_substep  # base slope, tangent slope, update: per substep / per RK4 stage


# The same fit on the CPU (fp64 numpy tangents under the same optimisers: `python tests/ac_fit_problem.py`) ends at
#   least_squares: max |p - p_true| = 4.974e-14, ssr / M = 2.291e-32   (11 solves)
#   mse:           max |p - p_true| = 1.671e-12, ssr / M = 2.515e-28   (49 solves)
# and the GPU fit is gated at 10 x those values.
CPU_FIT = {"least_squares": (4.974e-14, 2.291e-32), "mse": (1.671e-12, 2.515e-28)}


@pytest.mark.parametrize("method", ["least_squares", "mse"])
def test_fit_recovers_coefficients(method):
    model = P.PDEModel(P.AllenCahn2DPeriodic, _domain(F.N), P.RK4)
    truth = {"mu": ChemLeg(np.array(F.MU_TRUE), F.logit), "R": DiffLeg(np.array(F.R_TRUE)), "kappa": F.KAPPA}
    y0s = F.y0s()
    sol = model.solve(truth, y0s, F.TS, {})  # (T, B, n, n): noise-free synthetic data
    B, T = len(y0s), len(F.TS)
    data = {"ys": [sol[q, b] for b in range(B) for q in range(T)], "ts": np.tile(F.TS, B)}
    inds = [[b * T + q for q in range(T)] for b in range(B)]
    init = {"mu": ChemLeg(np.array(F.MU_INIT), F.logit), "R": DiffLeg(np.array(F.R_INIT))}
    res = model.train(data, inds, init, {"kappa": F.KAPPA}, {}, {}, 0.0, method=method, max_steps=100)
    p = np.concatenate([res["mu"].expansion.params, res["R"].expansion.params])
    p_true = np.array(F.MU_TRUE + F.R_TRUE)
    err = float(np.max(np.abs(p - p_true)))
    values = np.swapaxes(sol, 0, 1)[:, 1:]
    final = model.mse(res, (y0s, values), {}, F.TS, {}, 0.0)
    print(f"{method}: max |p - p_true| = {err:.3e}, ssr / M = {final:.3e}")
    cpu_err, cpu_final = CPU_FIT[method]
    assert isinstance(res["mu"], ChemLeg) and res["mu"].prior_fn is F.logit and isinstance(res["R"], DiffLeg)
    # mu's constant coefficient moves toward its true value: Allen-Cahn's right-hand side holds mu itself
    assert abs(p[0] - F.MU_TRUE[0]) < 0.1 * abs(F.MU_INIT[0] - F.MU_TRUE[0])
    assert err <= 10 * cpu_err
    assert final <= 10 * cpu_final
