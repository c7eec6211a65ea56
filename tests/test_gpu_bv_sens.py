"""Forward-mode sensitivities of the Butler-Volmer Allen-Cahn equations on the MI355X (csrc/butler_volmer.hip, the bvsens
kernels) against the numpy tangent reference tests/bv_sens_ref.py: the tangent right-hand side (constant current, given
voltage, smoothed boundary; fp64 and fp32), the voltage tangents, Euler / RK4 tangent trajectories, central differences of
GPU forward solves, the base block against PDEModel.solve, bitwise repeats and the Gauss-Newton sums with the voltage terms.

Shapes around the 16 x 64 workgroup tile: 16 x 64 (one workgroup, one partial), 20 x 70 (2 x 2 ragged tiles), 33 x 130
(3 x 3 tiles, odd ny).  B = 2 with a current per trajectory, P = 5 (3 mu + 2 j0 coefficients), and the notebook's
sqrt((1 - c) c) as a fixed j0 (P = 3).

Gates: 1e-11 relative L2 for the fp64 right-hand side and the voltage tangents, 1e-10 for 40-step trajectories and the
Gauss-Newton sums (tests/test_gpu_sens_ac.py), 10 x bv_sens_ref.CD_MEASURED for central differences (measured in
tests/test_bv_sens_cpu.py).  fp32: the kernel's relative L2 distance from the fp64 reference is held to 2 x the distance of
the SAME reference evaluated in float32 on the same inputs."""
import types

import numpy as np
import pytest

import bv_ref as R
import bv_sens_ref as S
import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd import fit
from pde_opt_amd.engine import HipEngine
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg

pytestmark = pytest.mark.gpu

SHAPES = [(16, 64), (20, 70), (33, 130)]
KINDS = ["current", "voltage", "sbm"]
VOLTS = (0.05, -0.1)  # the given-voltage class: one voltage per trajectory
B = 2
F_SBM = lambda c: c * np.log(c) + (1.0 - c) * np.log(1.0 - c) + 3.0 * c * (1.0 - c) + 0.059  # noqa: E731


def logit(c):
    return np.log(c / (1.0 - c))


def domain(nx, ny, psi=None):
    geo = None if psi is None else types.SimpleNamespace(smooth=psi)
    return P.Domain((nx, ny), ((0.0, S.H * nx), (0.0, S.H * ny)), "dimensionless", geo)


def make_eq(kind, nx, ny, value, mu=S.MU_DESC, j0=S.J0_DESC):
    if kind == "voltage":
        return P.AllenCahn2DPeriodicButlerVolmer(domain(nx, ny), S.KAPPA, mu, j0, S.ALPHA, v=value)
    if kind == "current":
        return P.AllenCahn2DPeriodicButlerVolmerConstantCurrent(domain(nx, ny), S.KAPPA, mu, j0, S.ALPHA, value)
    return P.AllenCahn2DSmoothedBoundaryButlerVolmerConstantCurrent(domain(nx, ny, R.disc_psi(nx, ny)), S.KAPPA, F_SBM, mu, j0,
                                                                    S.ALPHA, value)


def values_of(kind):
    return VOLTS if kind == "voltage" else S.CRATES


def sens_engine(eng, kind, base, tangents, params, j0=S.J0_DESC):
    """``eng`` configured for the (1 + P) B batch of ``base`` (B, nx, ny) and ``tangents`` (P B, nx, ny)"""
    nb, nx, ny = base.shape
    vals = values_of(kind)[:nb]
    eq = make_eq(kind, nx, ny, vals[0], j0=j0)
    eng.configure(dtype=base.dtype, batch=(1 + len(params)) * nb, **eq._engine_problem())
    eq._engine_upload(eng, 0.0, 1.0)
    eng.set_bv_params(S.ALPHA, eq._mode, list(vals))  # the trajectories' numbers; the tangent environments read none
    eng.sens_configure(nb, params)
    eng.set_state(np.concatenate([base, tangents]))
    return eq


def ref_slopes(kind, u, dus, params, value, j0desc=S.J0_DESC):
    """the reference in the dtype of ``u``"""
    t = u.dtype.type
    mu, j0 = S.Closure(S.MU_DESC), S.Closure(j0desc)
    if kind == "voltage":
        return S.slopes_voltage(u, dus, params, S.H, S.H, t(S.KAPPA), t(S.ALPHA), t(value), mu, j0)
    psi = R.disc_psi(*u.shape).astype(u.dtype) if kind == "sbm" else None
    return S.slopes_current(u, dus, params, S.H, S.H, t(S.KAPPA), t(S.ALPHA), t(value), mu, j0, psi)


@pytest.fixture(scope="module")
def eng():
    e = HipEngine()
    yield e
    e.close()


def inputs(nx, ny, n_params, dtype=np.float64):
    rng = np.random.default_rng(100 * nx + ny)
    base = R.notebook_state(rng, (B, nx, ny), dtype)
    assert 0.05 <= base.min() and base.max() < 0.95  # sqrt, logit and their derivatives are finite
    tang = (0.05 * rng.standard_normal((n_params * B, nx, ny))).astype(dtype)
    return base, tang


CASES = [(k, S.J0_DESC, S.PARAMS) for k in KINDS] + [("current", S.J0_SQRT_DESC, S.PARAMS[:3])]
CASE_IDS = KINDS + ["current-sqrt-j0"]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_tangent_rhs_fp64(eng, case, shape):
    kind, j0desc, params = case
    base, tang = inputs(*shape, len(params))
    sens_engine(eng, kind, base, tang, params, j0desc)
    k = eng.sens_rhs()
    for b in range(B):
        f, dfs = ref_slopes(kind, base[b], [tang[j * B + b] for j in range(len(params))], params, values_of(kind)[b], j0desc)
        assert S.rel(k[b], f) <= 1e-11
        for j in range(len(params)):
            err = S.rel(k[B + j * B + b], dfs[j])
            print(f"{CASE_IDS[CASES.index(case)]} {shape} b={b} j={j}: {err:.2e}")
            assert err <= 1e-11, (b, j)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", KINDS)
def test_tangent_rhs_fp32(eng, kind, shape):
    """The distance is the relative L2 norm over the tangent block of pdeopt_sens_rhs's output (all P B tangent slopes of the
    case), for the kernel and for the float32 numpy evaluation alike.  Per single tangent field the two distances are both a
    few float32 roundings and their ratio scatters (numpy's can be small by luck): it is printed, not gated.  Measured on an
    MI355X: DESIGN.md section 4.16."""
    base, tang = inputs(*shape, len(S.PARAMS), np.float32)
    sens_engine(eng, kind, base, tang, S.PARAMS)
    k = eng.sens_rhs().astype(np.float64)
    Pn = len(S.PARAMS)
    want_all, ref_all = np.empty((Pn * B,) + shape), np.empty((Pn * B,) + shape)
    for b in range(B):
        dus32 = [tang[j * B + b] for j in range(Pn)]
        _, want = ref_slopes(kind, base[b].astype(np.float64), [d.astype(np.float64) for d in dus32], S.PARAMS, values_of(kind)[b])
        _, ref32 = ref_slopes(kind, base[b], dus32, S.PARAMS, values_of(kind)[b])
        for j in range(Pn):
            want_all[j * B + b], ref_all[j * B + b] = want[j], ref32[j]
            d_kernel, d_ref = S.rel(k[B + j * B + b], want[j]), S.rel(ref32[j], want[j])
            print(f"{kind} {shape} b={b} j={j}: fp32 ratio {d_kernel / d_ref:.3f} (kernel {d_kernel:.2e}, numpy fp32 {d_ref:.2e})")
    d_kernel, d_ref = S.rel(k[B:], want_all), S.rel(ref_all, want_all)
    print(f"{kind} {shape}: fp32 ratio of the tangent block {d_kernel / d_ref:.3f} (kernel {d_kernel:.2e}, numpy fp32 {d_ref:.2e})")
    assert d_kernel <= 2.0 * d_ref


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["current", "sbm"])
def test_voltage_tangents(eng, kind, shape):
    base, tang = inputs(*shape, len(S.PARAMS))
    sens_engine(eng, kind, base, tang, S.PARAMS)
    got = eng.sens_bv_voltage()
    assert got[:, 0].tobytes() == eng.bv_voltage(0, B).tobytes()  # bitwise the v of pdeopt_bv_voltage
    mu, j0 = S.Closure(S.MU_DESC), S.Closure(S.J0_DESC)
    psi = R.disc_psi(*shape) if kind == "sbm" else None
    for b in range(B):
        v, dvs, _, _ = S.voltage_tangents(base[b], [tang[j * B + b] for j in range(len(S.PARAMS))], S.PARAMS, S.H, S.H, S.KAPPA,
                                          S.CRATES[b], mu, j0, psi)
        assert abs(got[b, 0] - v) <= 1e-11
        for j, dv in enumerate(dvs):
            print(f"{kind} {shape} b={b} dv[{j}]: {got[b, 1 + j]:.12e} vs {dv:.12e}")
            assert abs(got[b, 1 + j] - dv) <= 1e-11 * max(1.0, abs(dv)), (b, j)


def test_given_voltage_mode_has_no_voltage_tangent(eng):
    base, tang = inputs(16, 64, len(S.PARAMS))
    sens_engine(eng, "voltage", base, tang, S.PARAMS)
    with pytest.raises(Exception, match="mode 1"):
        eng.sens_bv_voltage()


# ---- trajectories --------------------------------------------------------------------------------------------------------
TNX, TNY = 20, 70
_cache = {}


def traj_states():
    if "u0" not in _cache:
        _cache["u0"] = np.stack([R.relaxed_state(3 + b, TNX, TNY) for b in range(B)])
        assert 0.05 < _cache["u0"].min() and _cache["u0"].max() < 0.95
    return _cache["u0"]


def ref_trajectory(integrator):
    """the reference's state, tangents and (v, dv) after TRAJ_STEPS steps, per trajectory; computed once"""
    if integrator not in _cache:
        mu, j0 = S.Closure(S.MU_DESC), S.Closure(S.J0_DESC)
        out = []
        for b in range(B):
            f = S.current_rhs(S.PARAMS, S.H, S.H, S.KAPPA, S.ALPHA, S.CRATES[b], mu, j0)
            u, dus = S.trajectory(f, traj_states()[b], len(S.PARAMS), S.TRAJ_DT, S.TRAJ_STEPS, integrator)
            v, dvs, _, _ = S.voltage_tangents(u, dus, S.PARAMS, S.H, S.H, S.KAPPA, S.CRATES[b], mu, j0)
            out.append((u, dus, v, dvs))
        _cache[integrator] = out
    return _cache[integrator]


@pytest.mark.parametrize("integrator", ["rk4", "euler"])
def test_tangent_trajectories_40_steps(eng, integrator):
    u0 = traj_states()
    Pn = len(S.PARAMS)
    code = L.INT_EULER if integrator == "euler" else L.INT_RK4
    sens_engine(eng, "current", u0, np.zeros((Pn * B, TNX, TNY)), S.PARAMS)
    eng.sens_advance(code, S.TRAJ_DT, S.TRAJ_STEPS)
    assert eng.last_kernel == "bvsens_tangent_rhs+" + integrator
    got = eng.get_state()
    vd = eng.sens_bv_voltage()
    for b, (u, dus, v, dvs) in enumerate(ref_trajectory(integrator)):
        assert S.rel(got[b], u) <= 1e-12
        scale = np.linalg.norm(dus[1])
        # mu's constant coefficient at constant current: v absorbs it, the state tangent is zero up to rounding
        assert np.linalg.norm(got[B + b]) <= 1e-10 * scale
        for j in range(1, Pn):
            err = S.rel(got[B + j * B + b], dus[j])
            print(f"{integrator} b={b} j={j}: {err:.2e}")
            assert err <= 1e-10, (b, j)
        assert abs(vd[b, 0] - v) <= 1e-10
        assert abs(vd[b, 1] + 1.0) <= 1e-10  # dv / d mu_0 = -1
        for j in range(Pn):
            assert abs(vd[b, 1 + j] - dvs[j]) <= 1e-10 * max(1.0, abs(dvs[j])), (b, j)


@pytest.mark.parametrize("integrator", ["rk4", "euler"])
def test_tangents_match_central_differences_of_gpu_forward_solves(eng, integrator):
    u0 = traj_states()[:1]
    Pn = len(S.PARAMS)
    code = L.INT_EULER if integrator == "euler" else L.INT_RK4
    # (one trajectory: B = 1 in this engine)
    eq = make_eq("current", TNX, TNY, S.CRATES[0])
    eng.configure(dtype=np.float64, batch=1 + Pn, **eq._engine_problem())
    eq._engine_upload(eng, 0.0, 1.0)
    eng.sens_configure(1, S.PARAMS)
    eng.set_state(np.concatenate([u0, np.zeros((Pn, TNX, TNY))]))
    eng.sens_advance(code, S.TRAJ_DT, S.TRAJ_STEPS)
    got = eng.get_state()
    fwd = HipEngine()
    fwd.configure(dtype=np.float64, batch=2 * Pn, **eq._engine_problem())
    eq._engine_upload(fwd, 0.0, 1.0)
    mu_c = np.tile(np.array(S.MU_COEF), (2 * Pn, 1))
    j0_c = np.tile(np.array(S.J0_COEF), (2 * Pn, 1))
    for j, (role, kc) in enumerate(S.PARAMS):
        arr = mu_c if role == S.MU_ROLE else j0_c
        arr[2 * j, kc] += S.CD_EPS
        arr[2 * j + 1, kc] -= S.CD_EPS
    fwd.set_env_params(0, mu_coef=mu_c, mob_coef=j0_c)
    fwd.set_state(np.concatenate([u0] * (2 * Pn)))
    fwd.advance(code, S.TRAJ_DT, S.TRAJ_STEPS)
    ends = fwd.get_state()
    fwd.close()
    scale = np.linalg.norm(got[2])
    for j in range(Pn):
        cd = (ends[2 * j] - ends[2 * j + 1]) / (2 * S.CD_EPS)
        if j == 0:  # exactly zero in exact arithmetic
            assert np.linalg.norm(got[1]) <= 1e-10 * scale and np.linalg.norm(cd) <= 10 * S.CD_MEASURED * scale
            continue
        err = S.rel(got[1 + j], cd)
        print(f"{integrator} j={j}: tangent vs central difference {err:.2e}")
        assert err <= 10 * S.CD_MEASURED, j


def model_params(crate=S.CRATES[0]):
    return {"mu": ChemLeg(np.array(S.MU_COEF), logit), "j0": DiffLeg(np.array(S.J0_COEF)), "kappa": S.KAPPA, "alpha": S.ALPHA,
            "Crate": crate}


CURRENT = P.AllenCahn2DPeriodicButlerVolmerConstantCurrent


@pytest.mark.parametrize("solver", ["Euler", "RK4"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_base_block_equals_solve_bitwise(dtype, solver):
    solver_type = getattr(P, solver)
    model = P.PDEModel(CURRENT, domain(TNX, TNY), solver_type)
    params = model_params()
    y0s = traj_states().astype(dtype)
    ts = np.array([0.0, 3.3e-4, 1.0e-3, 1.37e-3])  # save points inside steps and a remainder step (dt0 = 1e-4)
    want = model.solve(params, y0s, ts, {}, dt0=1e-4)
    eq = CURRENT(domain(TNX, TNY), **params)
    pm = fit.ParamMap.of({"mu": params["mu"], "j0": params["j0"]}, CURRENT)
    e = HipEngine()
    _, fields = fit.sensitivity_solve(e, eq, solver_type(), y0s, ts, pm.sens_params(), dt0=1e-4, fields=True)
    e.close()
    assert fields.dtype == want.dtype
    np.testing.assert_array_equal(fields[:, :B], want)


@pytest.mark.parametrize("kind", ["current", "voltage", "sbm"])
def test_repeated_calls_give_identical_bits(eng, kind):
    base, tang = inputs(33, 130, len(S.PARAMS))
    outs = []
    for _ in range(2):
        sens_engine(eng, kind, base, tang, S.PARAMS)
        k = eng.sens_rhs()
        vd = eng.sens_bv_voltage() if kind != "voltage" else np.zeros(1)
        vd2 = eng.sens_bv_voltage() if kind != "voltage" else np.zeros(1)
        eng.sens_advance(L.INT_RK4, 1e-8, 3)  # (the raw notebook state: rates of 1e5)
        eng.sens_advance(L.INT_EULER, 1e-8, 3)
        outs.append((k.tobytes(), vd.tobytes(), vd2.tobytes(), eng.get_state().tobytes()))
    assert outs[0] == outs[1] and outs[0][1] == outs[0][2]
    assert np.all(np.isfinite(np.frombuffer(outs[0][3])))


def test_gauss_newton_sums_with_and_without_voltages():
    model = P.PDEModel(CURRENT, domain(TNX, TNY), P.RK4)
    truth = model_params()
    guess = {**truth, "mu": ChemLeg(np.array([0.15, -2.8, 0.25]), logit), "j0": DiffLeg(np.array([-0.8, 0.1]))}
    opt = {"mu": guess["mu"], "j0": guess["j0"]}
    other = {"kappa": S.KAPPA, "alpha": S.ALPHA, "Crate": S.CRATES[0]}
    y0s = traj_states()
    dt0 = 1e-4
    ts = np.array([0.0, 4e-4, 1e-3])
    sol = model.solve(truth, y0s, ts, {}, dt0=dt0)
    frames = np.ascontiguousarray(sol[1:])  # (T - 1, B, nx, ny)
    eq_true = CURRENT(domain(TNX, TNY), **truth)
    v_obs = np.stack([eq_true.get_voltage(sol[q]) for q in range(1, len(ts))])  # (T - 1, B)
    eq = CURRENT(domain(TNX, TNY), **guess)
    pm = fit.ParamMap.of(opt, CURRENT)
    Pn = len(pm.sens_params())
    assert Pn == 5
    e = HipEngine()
    volt = []
    s1, fields = fit.sensitivity_solve(e, eq, P.RK4(), y0s, ts, pm.sens_params(), dt0=dt0, fields=True, frames=frames, voltages=volt)
    s2, _ = fit.sensitivity_solve(e, eq, P.RK4(), y0s, ts, pm.sens_params(), dt0=dt0, frames=frames)
    e.close()
    assert s1.tobytes() == s2.tobytes()
    V, dV = model.voltage_sensitivities(opt, other, y0s, ts, dt0=dt0)
    assert V.shape == (3, B) and dV.shape == (3, B, 5)
    vd = np.stack(volt)
    assert V.tobytes() == vd[..., 0].tobytes() and dV.tobytes() == vd[..., 1:].tobytes()
    # the voltages of the base block are those of the forward solve's states
    pred = model.solve(guess, y0s, ts, {}, dt0=dt0)
    np.testing.assert_allclose(V, np.stack([eq.get_voltage(pred[q]) for q in range(len(ts))]), rtol=0, atol=1e-12)
    # host sums from the fetched fields
    rr = frames - fields[1:, :B]
    tang = [fields[1:, B + j * B: B + (j + 1) * B] for j in range(Pn)]
    J = np.stack([t.reshape(-1) for t in tang], axis=1)
    r = rr.reshape(-1)
    for with_vs in (False, True):
        ssr, rdp, G = fit.unpack_sums(s1, Pn)
        h_ssr, h_rdp, h_G = r @ r, J.T @ r, J.T @ J
        if with_vs:
            w = 0.5 * frames.size / v_obs.size
            ssr, rdp, G = fit.add_voltage_sums(ssr, rdp, G, v_obs - V[1:], dV[1:], w)
            rv, Jv = (v_obs - V[1:]).reshape(-1), dV[1:].reshape(-1, Pn)
            h_ssr, h_rdp, h_G = h_ssr + w * (rv @ rv), h_rdp + w * (Jv.T @ rv), h_G + w * (Jv.T @ Jv)
        norms = np.sqrt(np.diag(h_G))
        assert abs(ssr - h_ssr) <= 1e-10 * h_ssr
        for i in range(Pn):
            if not with_vs and i == 0:  # mu's constant coefficient without voltages: a column of rounding noise
                assert abs(G[0, 0]) <= 1e-18 * G[1, 1]
                continue
            assert abs(rdp[i] - h_rdp[i]) <= 1e-10 * np.sqrt(h_ssr) * norms[i], i
            for j in range(Pn):
                if not with_vs and j == 0:
                    continue
                assert abs(G[i, j] - h_G[i, j]) <= 1e-10 * norms[i] * norms[j], (i, j)


def test_c_level_refusals(eng):
    base, tang = inputs(16, 64, len(S.PARAMS))
    eq = make_eq("current", 16, 64, 0.02)
    fresh = HipEngine()  # (a re-configure of the same shape keeps the parameters of the last one)
    fresh.configure(dtype=np.float64, batch=6 * B, **eq._engine_problem())
    with pytest.raises(Exception, match="pdeopt_set_bv_params"):
        fresh.sens_configure(B, S.PARAMS)  # the parameters come first
    fresh.close()
    sens_engine(eng, "current", base, tang, S.PARAMS)
    with pytest.raises(Exception, match="Euler and RK4"):
        eng.sens_advance(L.INT_IMEX, 1e-6, 1)
