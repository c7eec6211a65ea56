"""Smoothed-boundary forward-mode sensitivities on the MI355X (csrc/sens_sbm.hip): the tangent-linear right-hand sides and
Euler / RK4 tangent trajectories of AllenCahn2DSmoothedBoundary / CahnHilliard2DSmoothedBoundary against the numpy reference
(tests/sbm_sens_ref.py) and against central differences of GPU forward solves, the base block against the forward engine
bit for bit, the stage times, the launch count, the save-point sums and PDEModel.residuals / mse."""
import functools

import numpy as np
import pytest

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd import fit
from pde_opt_amd.engine import HipEngine
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg
import sbm_sens_problem as Q
import sbm_sens_ref as S
from util import SBM_F, SBM_FLUX, SBM_THETA, TOL

pytestmark = pytest.mark.gpu

T_EVAL = 0.17  # theta(0.17) = 0.80, flux(0.17) = 0.030
B = 2
# fp64 gate of the tangent right-hand sides: the forward smoothed-boundary kernels meet util.TOL (1e-11) against the
# oracle on these inputs (asserted below for the base block), so the tangents are held to the same 1e-11, as
# test_gpu_sens_ac.py does.
TOL64 = TOL[np.dtype(np.float64)]


def _sens_engine(eq, base, tangents, params, t_const=None):
    eng = HipEngine()
    eng.configure(dtype=base.dtype, batch=(1 + len(params)) * base.shape[0], **eq._engine_problem())
    eq._engine_upload(eng, 0.0, 1.0)
    if t_const is not None:  # the time terms of one evaluation time, as constants (pdeopt_sens_rhs passes no time)
        eng.set_time_terms(None, constant=eq._time_terms(t_const))
    eng.sens_configure(base.shape[0], params)
    eng.set_state(np.concatenate([base, tangents]))
    return eng


def _fwd_engine(eq, states, t_const=None):
    eng = HipEngine()
    eng.configure(dtype=states.dtype, batch=states.shape[0], **eq._engine_problem())
    eq._engine_upload(eng, 0.0, 1.0)
    if t_const is not None:
        eng.set_time_terms(None, constant=eq._time_terms(t_const))
    eng.set_state(states)
    return eng


@functools.lru_cache(maxsize=None)
def _rhs_reference(eq, shape, mob):
    """fp64 reference slopes of one case, and the reference's own single-precision error: the same functions evaluated
    on float32 inputs against themselves in float64 (computed once, shared by the fp64 and fp32 tests)"""
    p = Q.problem(eq, shape, mob)
    points = p.psi.shape
    base = np.stack([Q.state(points, 1 + b) for b in range(B)])
    tang = 0.05 * np.random.default_rng(7).standard_normal((len(Q.PARAMS) * B,) + points)
    b32, t32, p32 = base.astype(np.float32), tang.astype(np.float32), p.astype(np.float32)
    want, want32, own32 = {}, {}, 0.0
    for b in range(B):
        want[b] = S.rhs(p, base[b], T_EVAL)
        for j, (role, kc) in enumerate(Q.PARAMS):
            want[b, j] = S.tangent_rhs(p, base[b], tang[j * B + b], T_EVAL, role, kc)
            # the fp32 kernels read fp32 inputs: compare against the fp64 reference of those same values
            want32[b, j] = S.tangent_rhs(p, b32[b].astype(np.float64), t32[j * B + b].astype(np.float64), T_EVAL, role, kc)
            own32 = max(own32, Q.rel(S.tangent_rhs(p32, b32[b], t32[j * B + b], T_EVAL, role, kc), want32[b, j]))
    return p, base, tang, want, want32, own32


CASES = [(eq, shape, mob) for eq in ("ac", "ch") for shape in Q.SHAPES_OF[eq] for mob in Q.MOBS]


@pytest.mark.parametrize("eq,shape,mob", CASES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_tangent_rhs_matches_numpy_reference(dtype, eq, shape, mob):
    p, base, tang, want, want32, own32 = _rhs_reference(eq, shape, mob)
    assert np.all(p.f(base) > 0)
    equation = Q.equation(P, p)
    base, tang = base.astype(dtype), tang.astype(dtype)
    eng = _sens_engine(equation, base, tang, Q.PARAMS, T_EVAL)
    k = eng.sens_rhs()
    # the base block is the forward engine's own right-hand side, bit for bit
    fwd = _fwd_engine(equation, base, T_EVAL)
    np.testing.assert_array_equal(k[:B], fwd.rhs(0.0))
    if dtype == np.float64:
        tol = TOL64
        fwd_err = max(Q.rel(k[b], want[b]) for b in range(B))
        print(f"{eq} {shape} {mob}: forward kernel vs oracle {fwd_err:.2e}")
        assert fwd_err <= TOL64
    else:
        # 8 x the reference's own single-precision error (the project's margin for fp32), not below 1e-4
        tol = max(8 * own32, 1e-4)
        want = want32
    worst = 0.0
    for b in range(B):
        for j, (role, kc) in enumerate(Q.PARAMS):
            err = Q.rel(k[B + j * B + b], want[b, j])
            worst = max(worst, err)
            assert err <= tol, (b, j, err, tol)
    print(f"{eq} {shape} {mob} {np.dtype(dtype).name}: worst tangent error {worst:.2e} (gate {tol:.2e}, own fp32 error {own32:.2e})")


def test_missing_aux_is_refused():
    p = Q.problem("ac", "16x32")
    eq = Q.equation(P, p)
    eng = HipEngine()
    eng.configure(dtype=np.float64, batch=2, **eq._engine_problem())
    with pytest.raises(P.PdeoptError, match="SBM_PSI"):
        eng.sens_configure(1, [(S.MU_ROLE, 0)])


# ---- trajectories ----------------------------------------------------------------------------------------------------------

N = 64
MU3, MOB2 = (0.1, -3.0, 0.4), (0.8, 0.2)
TRAJ_PARAMS = {"ac": [(S.MU_ROLE, 0), (S.MU_ROLE, 1), (S.MU_ROLE, 2), (S.MOB_ROLE, 0), (S.MOB_ROLE, 1)],
               "ch": [(S.MU_ROLE, 1), (S.MU_ROLE, 2), (S.MOB_ROLE, 0), (S.MOB_ROLE, 1)]}
logit = lambda c: np.log(c / (1 - c))  # noqa: E731


def _traj_problem(eq):
    equation0 = Q.equation(P, Q.problem(eq, ((N, N), (1.0, 1.0))), mu=ChemLeg(np.array(MU3), logit), mob=DiffLeg(np.array(MOB2)))
    p = Q.problem(eq, ((N, N), (1.0, 1.0)), mob=equation0._mob_desc, mu=equation0._mu_desc)
    return p, equation0


@functools.lru_cache(maxsize=None)
def _traj_reference(eq, integrator):
    p, _ = _traj_problem(eq)
    u0 = Q.smooth_state((N, N), 3)
    return (u0,) + S.trajectory(p, u0, TRAJ_PARAMS[eq], Q.TRAJ_DT[eq], 200, integrator, Q.TRAJ_T0)


@pytest.mark.parametrize("eq", ["ac", "ch"])
@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_tangent_trajectories_200_substeps(eq, integrator):
    p, equation = _traj_problem(eq)
    params, dt, t0 = TRAJ_PARAMS[eq], Q.TRAJ_DT[eq], Q.TRAJ_T0
    Pn = len(params)
    u0, u_ref, dus = _traj_reference(eq, integrator)
    code = L.INT_EULER if integrator == "euler" else L.INT_RK4
    zeros = np.zeros((Pn, N, N))
    eng = _sens_engine(equation, u0[None], zeros, params)
    eng.sens_advance(code, dt, 200, t0)
    got = eng.get_state()
    assert "sens_sbm_" + eq in eng.last_kernel
    assert Q.rel(got[0], u_ref) <= 1e-12
    for j in range(Pn):
        assert Q.rel(got[1 + j], dus[j]) <= 1e-10, j
    # the base trajectory is the forward engine's, bit for bit -- on its stage-by-stage path, the launches the base block
    # issues (at this size the forward engine would otherwise pick its one-launch kernel, which has its own rounding)
    fwd = _fwd_engine(equation, u0[None])
    fwd.set_small_persist(-1)
    fwd.advance(code, dt, 200, t0)
    np.testing.assert_array_equal(got[0], fwd.get_state()[0])
    # a repeat gives identical bits; a split call with the right start time too; a wrong start time does not
    def run(parts):
        e = _sens_engine(equation, u0[None], zeros, params)
        for n, t in parts:
            e.sens_advance(code, dt, n, t)
        return e.get_state()
    assert run([(200, t0)]).tobytes() == got.tobytes()
    assert run([(120, t0), (80, t0 + 120 * dt)]).tobytes() == got.tobytes()
    wrong = run([(120, t0), (80, t0)])
    assert Q.rel(wrong[1], got[1]) > 1e-6 and Q.rel(wrong[0], got[0]) > 1e-8
    # central differences of GPU forward solves: 2 P environments with their own coefficients +- eps.  The truncation
    # of a central difference is eps^2 / 6 |d^3 u / dp^3| and its rounding ~1e-16 |u| / (eps |du/dp|).  Allen-Cahn's tangents
    # grow to O(1) - O(10) over these 200 steps (the equation is not conservative) and the third derivative with them: eps =
    # 1e-5 keeps the truncation below 1e-7 and, the tangents being large, the rounding at 1e-12.  Cahn-Hilliard's tangents
    # stay O(1e-2): eps = 1e-4 balances the two (both ~1e-8).
    eps = 1e-5 if eq == "ac" else 1e-4
    mu_c = np.tile(np.array(equation._mu_desc.coef), (2 * Pn, 1))
    mob_c = np.tile(np.array(equation._mob_desc.coef), (2 * Pn, 1))
    for j, (role, kc) in enumerate(params):
        arr = mu_c if role == S.MU_ROLE else mob_c
        arr[2 * j, kc] += eps
        arr[2 * j + 1, kc] -= eps
    fwd2 = _fwd_engine(equation, np.stack([u0] * (2 * Pn)))
    fwd2.set_env_params(0, mu_coef=mu_c, mob_coef=mob_c)
    fwd2.advance(code, dt, 200, t0)
    ends = fwd2.get_state()
    for j in range(Pn):
        assert Q.rel(got[1 + j], (ends[2 * j] - ends[2 * j + 1]) / (2 * eps)) <= 1e-6, j


@pytest.mark.parametrize("eq", ["ac", "ch"])
@pytest.mark.parametrize("integrator,per_substep", [("euler", 3), ("rk4", 12)])
def test_launches_per_substep_do_not_depend_on_P(eq, integrator, per_substep):
    _, equation = _traj_problem(eq)
    code = L.INT_EULER if integrator == "euler" else L.INT_RK4
    counts = []
    for params in (TRAJ_PARAMS[eq][:1], TRAJ_PARAMS[eq] + [(S.MU_ROLE, 1), (S.MOB_ROLE, 0), (S.MOB_ROLE, 1)][:7 - len(TRAJ_PARAMS[eq])]):
        base = np.stack([Q.state((N, N), b) for b in range(B)])
        eng = _sens_engine(equation, base, np.zeros((len(params) * B, N, N)), params)
        before = eng.stage_launches()
        eng.sens_advance(code, Q.TRAJ_DT[eq], 10, Q.TRAJ_T0)
        counts.append(eng.stage_launches() - before)
    assert counts[0] == counts[1] == 10 * per_substep  # base slope, tangent slope, update: per substep / per RK4 stage


# ---- save points: sums, contraction, residuals, mse ----------------------------------------------------------------------------

KINDS = {"ac": (P.AllenCahn2DSmoothedBoundary, "R"), "ch": (P.CahnHilliard2DSmoothedBoundary, "D")}


def _params(eq, mu, mob):
    cls, key = KINDS[eq]
    o = {"mu": ChemLeg(np.array(mu), logit), key: DiffLeg(np.array(mob)), "kappa": Q.KAPPA, "f": SBM_F, "theta": SBM_THETA}
    if eq == "ch":
        o["flux"] = SBM_FLUX
    return o


@pytest.mark.parametrize("eq", ["ac", "ch"])
@pytest.mark.parametrize("solver", ["Euler", "RK4"])
def test_residuals_mse_sums_and_contraction(eq, solver):
    cls, key = KINDS[eq]
    solver_type = getattr(P, solver)
    p = Q.problem(eq, "24x120" if eq == "ac" else "67x40")
    points = p.psi.shape
    model = P.PDEModel(cls, Q.domain(P, p), solver_type)
    truth, guess = _params(eq, (0.1, -3.0), (0.8, 0.2)), _params(eq, (0.2, -2.5), (0.9, 0.1))
    y0s = np.stack([Q.smooth_state(points, s) for s in (4, 5)])
    dt0 = Q.TRAJ_DT[eq]
    ts = np.array([0.0, 2.5 * dt0, 6 * dt0])  # a save point inside a step and one on an edge
    values = np.swapaxes(model.solve(truth, y0s, ts, {}, dt0=dt0), 0, 1)[:, 1:]
    weights = {"mu": ChemLeg(np.array([1.0, 1.0])), key: DiffLeg(np.array([2.0, 0.0]))}
    # residuals / mse use the default step of solve: compare with the host-side formulas on the same solve
    r, reg = model.residuals(guess, (y0s, values), {}, ts, weights, 0.5)
    pred = model.solve(guess, y0s, ts, {})
    np.testing.assert_array_equal(r, values - np.swapaxes(pred, 0, 1)[:, 1:])
    assert abs(reg - 0.5 * (0.04 + 6.25 + 2 * 0.81)) < 1e-12
    m = model.mse(guess, (y0s, values), {}, ts, weights, 0.5)
    assert abs(m - (np.mean(r ** 2) + reg)) <= 1e-12 * abs(m)
    # the Gauss-Newton sums and the contraction against sums over the reference's fields
    equation = cls(domain=Q.domain(P, p), **guess)
    pm = fit.ParamMap.of({"mu": guess["mu"], key: guess[key]}, cls)
    sp = pm.sens_params()
    assert len(sp) == (4 if eq == "ac" else 3)  # mu's constant coefficient: active for Allen-Cahn, inert for Cahn-Hilliard
    frames = np.ascontiguousarray(np.swapaxes(values, 0, 1))
    eng = HipEngine()
    s1, fields = fit.sensitivity_solve(eng, equation, solver_type(), y0s, ts, sp, dt0=dt0, fields=True, frames=frames)
    s2, _ = fit.sensitivity_solve(eng, equation, solver_type(), y0s, ts, sp, dt0=dt0, frames=frames)
    assert s1.tobytes() == s2.tobytes()
    np.testing.assert_array_equal(fields[:, :B], model.solve(guess, y0s, ts, {}, dt0=dt0))  # the base follows solve
    # reference fields at the save points: 2 steps + half a step (linear dense output), 6 steps
    pr = Q.problem(eq, (points, (1.0, 1.0)), mu=equation._mu_desc, mob=equation._mob_desc)
    integ = solver.lower()
    ref = []
    for b in range(B):
        u2, d2 = S.trajectory(pr, y0s[b], sp, dt0, 2, integ)
        u3, d3 = S.step(pr, u2, d2, sp, 2 * dt0, dt0, integ)
        u6, d6 = u3, d3
        for s in range(3, 6):
            u6, d6 = S.step(pr, u6, d6, sp, s * dt0, dt0, integ)
        ref.append([[0.5 * (a + c) for a, c in zip([u2] + d2, [u3] + d3)], [u6] + d6])
    Pn = len(sp)
    rr = np.array([[frames[q, b] - ref[b][q][0] for b in range(B)] for q in range(2)])
    tang = [np.array([[ref[b][q][1 + j] for b in range(B)] for q in range(2)]) for j in range(Pn)]
    ssr, rdp, G = fit.unpack_sums(s1, Pn)
    # the GPU fields follow the reference to 1e-10 (the trajectory gate); a residual is a small difference of fields, so
    # its relative error is that times |field| / |residual|
    tol_r = 1e-10 + 4e-10 * np.linalg.norm(fields[1:, :B]) / np.linalg.norm(rr)
    assert abs(ssr - np.sum(rr ** 2)) <= tol_r * ssr
    for i in range(Pn):
        assert abs(rdp[i] - np.sum(rr * tang[i])) <= tol_r * np.sqrt(ssr * np.sum(tang[i] ** 2))
        for j in range(Pn):
            assert abs(G[i, j] - np.sum(tang[i] * tang[j])) <= 1e-9 * np.sqrt(np.sum(tang[i] ** 2) * np.sum(tang[j] ** 2))
    cot = np.random.default_rng(3).standard_normal(frames.shape)
    c, _ = fit.sensitivity_solve(eng, equation, solver_type(), y0s, ts, sp, dt0=dt0, cotangents=cot)
    for b in range(B):
        for j in range(Pn):
            want = np.sum(cot[:, b] * tang[j][:, b])
            assert abs(c[b, j] - want) <= 1e-9 * np.sqrt(np.sum(cot[:, b] ** 2) * np.sum(tang[j][:, b] ** 2))
