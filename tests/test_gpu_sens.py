"""Forward-mode sensitivities on the MI355X: the tangent-linear right-hand side and tangent trajectories against the
numpy reference (tests/sens_ref.py) and against central differences of GPU forward solves, the base field against
PDEModel.solve, the Gauss-Newton sums, and PDEModel.train on the reference notebooks' fitting problems."""
import numpy as np
import pytest

import pde_opt_amd as P
from oracle import np_oracle as O
from pde_opt_amd import _lib as L
from pde_opt_amd import fit
from pde_opt_amd.engine import HipEngine
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg
import sens_ref as S

pytestmark = pytest.mark.gpu

KAPPA = 0.002


def _logit(c):
    return np.log(c / (1.0 - c))


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def _domain(n):
    return P.Domain((n, n), ((0.0, 1.0), (0.0, 1.0)), "dimensionless")


def _state(n, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return np.clip(0.5 + 0.1 * rng.standard_normal((n, n)), 0.1, 0.9).astype(dtype)


def _smooth_state(n, seed, dtype=np.float64):
    """a smooth random field around 0.5 (a few Fourier modes)"""
    rng = np.random.default_rng(seed)
    x = np.arange(n) / n
    u = 0.5 + np.zeros((n, n))
    for _ in range(6):
        kx, ky = rng.integers(1, 4, 2)
        u += 0.03 * rng.standard_normal() * np.cos(2 * np.pi * (kx * x[:, None] + ky * x[None, :]) + rng.uniform(0, 6))
    return u.astype(dtype)


MU3 = (0.0, -3.0, 0.4)
D2 = (-0.3, 0.2)
PARAMS = [(S.MU_ROLE, 1), (S.MU_ROLE, 2), (S.MOB_ROLE, 0), (S.MOB_ROLE, 1)]


def _equation(n, mu=MU3, D=D2):
    return P.CahnHilliard2DPeriodic(_domain(n), KAPPA, ChemLeg(np.array(mu), _logit), DiffLeg(np.array(D)))


def _sens_engine(eq, solver, base, tangents, params):
    eng = HipEngine()
    B = base.shape[0]
    eng.configure(dtype=base.dtype, batch=(1 + len(params)) * B, **eq._engine_problem())
    eq._engine_upload(eng, 0.0, 1.0)
    if solver is not None:
        solver.configure_engine(eng, eq)
    eng.sens_configure(B, params)
    eng.set_state(np.concatenate([base, tangents]))
    return eng


@pytest.mark.parametrize("n", [64, 128])
@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-11), (np.float32, 1e-4)])
def test_tangent_rhs_matches_numpy_reference(n, dtype, tol):
    eq = _equation(n)
    B = 2
    base = np.stack([_state(n, 1 + b, dtype) for b in range(B)])
    rng = np.random.default_rng(7)
    tang = (0.05 * rng.standard_normal((len(PARAMS) * B, n, n))).astype(dtype)
    eng = _sens_engine(eq, None, base, tang, PARAMS)
    k = eng.sens_rhs()
    h = 1.0 / n
    mu, mob = eq._mu_desc, eq._mob_desc
    for b in range(B):
        u = base[b].astype(np.float64)
        assert _rel(k[b], S.ch_rhs(u, h, h, KAPPA, mu, mob)) <= max(tol, 1e-12)
        for j, (role, kc) in enumerate(PARAMS):
            du = tang[B + j * B + b - B].astype(np.float64)
            want = S.tangent_rhs(u, du, h, h, KAPPA, mu, mob, role, kc)
            assert _rel(k[B + j * B + b], want) <= tol, (b, j)


@pytest.mark.parametrize("integrator", ["imex", "euler"])
def test_tangent_trajectories_200_substeps(integrator):
    n = 64
    eq = _equation(n)
    h = 1.0 / n
    symbol = O.ch_fourier_symbol(n, n, h, h, KAPPA)
    u0 = _smooth_state(n, 3)
    dt = 2e-6 if integrator == "imex" else 2e-7
    code = L.INT_IMEX if integrator == "imex" else L.INT_EULER
    solver = P.SemiImplicitFourierSpectral(A=0.5, fourier_symbol=eq.fourier_symbol) if integrator == "imex" else None
    eng = _sens_engine(eq, solver, u0[None], np.zeros((len(PARAMS), n, n)), PARAMS)
    eng.sens_advance(code, dt, 200)
    got = eng.get_state()
    u_ref, dus = S.trajectory(u0, PARAMS, dt, 200, h, h, KAPPA, eq._mu_desc, eq._mob_desc, integrator, 0.5, symbol)
    assert _rel(got[0], u_ref) <= 1e-12
    for j in range(len(PARAMS)):
        assert _rel(got[1 + j], dus[j]) <= 1e-10, j
    # central differences of GPU forward solves: 2 P environments with their own coefficients +- eps
    eps = 1e-4
    fwd = HipEngine()
    fwd.configure(dtype=np.float64, batch=2 * len(PARAMS), **eq._engine_problem())
    eq._engine_upload(fwd, 0.0, 1.0)
    if solver is not None:
        solver.configure_engine(fwd, eq)
    mu_c = np.tile(np.array(eq._mu_desc.coef), (2 * len(PARAMS), 1))
    mob_c = np.tile(np.array(eq._mob_desc.coef), (2 * len(PARAMS), 1))
    for j, (role, kc) in enumerate(PARAMS):
        arr = mu_c if role == S.MU_ROLE else mob_c
        arr[2 * j, kc] += eps
        arr[2 * j + 1, kc] -= eps
    fwd.set_env_params(0, mu_coef=mu_c, mob_coef=mob_c)
    fwd.set_state(np.stack([u0] * (2 * len(PARAMS))))
    fwd.advance(code, dt, 200)
    ends = fwd.get_state()
    for j in range(len(PARAMS)):
        cd = (ends[2 * j] - ends[2 * j + 1]) / (2 * eps)
        assert _rel(got[1 + j], cd) <= 1e-6, j


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-12), (np.float32, 1e-5)])
def test_base_field_matches_solve(dtype, tol):
    n = 64
    model = P.PDEModel(P.CahnHilliard2DPeriodic, _domain(n), P.SemiImplicitFourierSpectral)
    params = {"mu": ChemLeg(np.array([0.0, -3.0, 0.2]), _logit), "D": DiffLeg(np.array([-0.2])), "kappa": KAPPA}
    y0s = np.stack([_smooth_state(n, s, dtype) for s in (1, 2)])
    ts = np.array([0.0, 3.3e-5, 1.0e-4, 1.37e-4])  # save points inside steps and a remainder step (dt0 = 1e-5)
    want = model.solve(params, y0s, ts, {"A": 0.5}, dt0=1e-5)
    eq = P.CahnHilliard2DPeriodic(_domain(n), **params)
    solver = P.SemiImplicitFourierSpectral(A=0.5, fourier_symbol=eq.fourier_symbol)
    pm = fit.ParamMap.of({"mu": params["mu"], "D": params["D"]})
    _, fields = fit.sensitivity_solve(HipEngine(), eq, solver, y0s, ts, pm.sens_params(), dt0=1e-5, fields=True)
    assert _rel(fields[:, :2], want.astype(np.float64)) <= tol


def test_residuals_mse_and_bitwise_sums():
    n = 64
    model = P.PDEModel(P.CahnHilliard2DPeriodic, _domain(n), P.SemiImplicitFourierSpectral)
    truth = {"mu": ChemLeg(np.array([0.0, -3.0]), _logit), "D": DiffLeg(np.array([0.0])), "kappa": KAPPA}
    y0s = np.stack([_smooth_state(n, s) for s in (4, 5)])
    ts = np.array([0.0, 2.5e-5, 6e-5])
    values = np.swapaxes(model.solve(truth, y0s, ts, {"A": 0.5}, dt0=1e-5), 0, 1)[:, 1:]
    guess = {"mu": ChemLeg(np.array([0.1, -2.5]), _logit), "D": DiffLeg(np.array([0.2])), "kappa": KAPPA}
    weights = {"mu": ChemLeg(np.array([1.0, 1.0])), "D": DiffLeg(np.array([2.0]))}
    r, reg = model.residuals(guess, (y0s, values), {"A": 0.5}, ts, weights, 0.5)
    pred = model.solve(guess, y0s, ts, {"A": 0.5})
    np.testing.assert_array_equal(r, values - np.swapaxes(pred, 0, 1)[:, 1:])
    assert abs(reg - 0.5 * (0.01 + 6.25 + 2 * 0.04)) < 1e-12
    m = model.mse(guess, (y0s, values), {"A": 0.5}, ts, weights, 0.5)
    assert abs(m - (np.mean(r ** 2) + reg)) <= 1e-12 * abs(m)
    # the Gauss-Newton sums against sums over the fetched fields, and bitwise-equal on a repeat
    eq = P.CahnHilliard2DPeriodic(_domain(n), **guess)
    solver = P.SemiImplicitFourierSpectral(A=0.5, fourier_symbol=eq.fourier_symbol)
    pm = fit.ParamMap.of({"mu": guess["mu"], "D": guess["D"]})
    frames = np.ascontiguousarray(np.swapaxes(values, 0, 1))
    eng = HipEngine()
    s1, fields = fit.sensitivity_solve(eng, eq, solver, y0s, ts, pm.sens_params(), dt0=1e-5, fields=True, frames=frames)
    s2, _ = fit.sensitivity_solve(eng, eq, solver, y0s, ts, pm.sens_params(), dt0=1e-5, frames=frames)
    assert s1.tobytes() == s2.tobytes()
    B, Pn = 2, len(pm.sens_params())
    rr = frames - fields[1:, :B]
    tang = [fields[1:, B + j * B: B + (j + 1) * B] for j in range(Pn)]
    ssr, rdp, G = fit.unpack_sums(s1, Pn)
    assert abs(ssr - np.sum(rr ** 2)) <= 1e-10 * ssr
    for i in range(Pn):
        assert abs(rdp[i] - np.sum(rr * tang[i])) <= 1e-10 * np.sqrt(ssr * np.sum(tang[i] ** 2))
        for j in range(Pn):
            assert abs(G[i, j] - np.sum(tang[i] * tang[j])) <= 1e-10 * np.sqrt(np.sum(tang[i] ** 2) * np.sum(tang[j] ** 2))


def test_launches_per_substep():
    n = 128
    for params in (PARAMS[:3], [(S.MU_ROLE, 0), (S.MU_ROLE, 1), (S.MU_ROLE, 2), (S.MOB_ROLE, 0), (S.MOB_ROLE, 1),
                                (S.MU_ROLE, 1), (S.MOB_ROLE, 0)]):
        eq = _equation(n)
        solver = P.SemiImplicitFourierSpectral(A=0.5, fourier_symbol=eq.fourier_symbol)
        B = 2
        base = np.stack([_state(n, b) for b in range(B)])
        eng = _sens_engine(eq, solver, base, np.zeros((len(params) * B, n, n)), params)
        before = eng.stage_launches()
        eng.sens_advance(L.INT_IMEX, 1e-6, 10)
        assert eng.stage_launches() - before <= 10 * 5


def _notebook_data(n, dtype, mu_true, D_true):
    model = P.PDEModel(P.CahnHilliard2DPeriodic, _domain(n), P.SemiImplicitFourierSpectral)
    y0 = _smooth_state(n, 11, dtype)
    ts = np.linspace(0.0, 0.02, 100)
    truth = {"mu": ChemLeg(np.array(mu_true), _logit), "D": DiffLeg(np.array(D_true)), "kappa": KAPPA}
    sol = model.solve(truth, y0, ts, {"A": 0.5})
    return model, {"ys": list(sol), "ts": ts}


INDS = [[30, 40, 50], [50, 60, 70], [70, 80, 90]]


def test_notebook_least_squares_fp64():
    model, data = _notebook_data(128, np.float64, [0.0, -3.0], [0.0])
    init = {"mu": ChemLeg(np.array([0.0, -2.0]), _logit), "D": DiffLeg(np.array([0.0]))}
    weights = {"mu": ChemLeg(np.array([0.0, 0.0])), "D": DiffLeg(np.array([0.0]))}
    res = model.train(data, INDS, init, {"kappa": KAPPA}, {"A": 0.5}, weights, 1000.0)
    hist = model.last_train_history
    assert isinstance(res["mu"], ChemLeg) and res["mu"].prior_fn is _logit and isinstance(res["D"], DiffLeg)
    assert abs(res["mu"].expansion.params[1] + 3.0) <= 1e-6
    assert res["mu"].expansion.params[0] == 0.0
    assert hist[-1] <= 1e-12 * hist[0]
    assert res["kappa"] == KAPPA


def test_notebook_least_squares_fp32():
    model, data = _notebook_data(128, np.float32, [0.0, -3.0], [0.0])
    init = {"mu": ChemLeg(np.array([0.0, -2.0]), _logit), "D": DiffLeg(np.array([0.0]))}
    res = model.train(data, INDS, init, {"kappa": KAPPA}, {"A": 0.5}, {}, 0.0)
    assert abs(res["mu"].expansion.params[1] + 3.0) <= 1e-2


@pytest.mark.parametrize("method", ["least_squares", "mse"])
def test_seven_parameter_fit(method):
    n = 64
    model, data = _notebook_data(n, np.float64, [0.0, -3.0, 0.0, 0.0, 0.0, 0.0], [np.log(0.15)])
    init = {"mu": ChemLeg(np.zeros(6), _logit), "D": DiffLeg(np.array([np.log(0.05)]))}
    weights = {"mu": ChemLeg(np.array([0.0, 2, 6, 12, 20, 30])), "D": DiffLeg(np.array([0.0]))}
    res = model.train(data, INDS, init, {"kappa": KAPPA}, {"A": 0.5}, weights, 0.0, method=method, max_steps=100)
    np.testing.assert_allclose(res["mu"].expansion.params, [0.0, -3.0, 0.0, 0.0, 0.0, 0.0], rtol=0, atol=1e-4)
    np.testing.assert_allclose(res["D"].expansion.params, [np.log(0.15)], rtol=0, atol=1e-4)
    ys = model.solve(res, data["ys"][30], data["ts"][30:41] - data["ts"][30], {"A": 0.5})
    assert np.all(np.isfinite(ys))
