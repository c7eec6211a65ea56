"""kappa as a trainable scalar, on the CPU: the numpy tangent reference (tests/sens_kappa_ref.py) against central
differences in kappa of the oracle's trajectory, ParamMap's scalar entries, and PDEModel.train's host logic on a test
double of the engine (tests/fake_engine.py plus the sensitivity calls, backed by the same reference)."""
import math

import numpy as np
import pytest

import pde_opt_amd as P
from fake_engine import OracleEngine
from pde_opt_amd import _lib as L
from pde_opt_amd import fit
from pde_opt_amd.numerics.closures import EXP_WRAP, LEGENDRE, LOGIT_PRIOR, ClosureDesc
from pde_opt_amd.numerics.functions import TrainableScalar
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg
import sens_kappa_ref as K

KAPPA = 0.002
MU = ClosureDesc(LEGENDRE, LOGIT_PRIOR, (0.1, -3.0, 0.2))
MOB = ClosureDesc(LEGENDRE, EXP_WRAP, (-0.3, 0.1))
RATE = ClosureDesc(LEGENDRE, EXP_WRAP, (6.9, 0.3))  # Allen-Cahn's R ~ 1000: the state moves in 20 steps of 1e-6


def _state(shape, seed):
    rng = np.random.default_rng(seed)
    return np.clip(0.5 + 0.15 * rng.standard_normal(shape), 0.1, 0.9)


# (eq, shape, spacings, mob, integrator, dt).  The kappa step of the central difference, eps = 1e-4 kappa: its truncation
# error is (eps / kappa)^2 = 1e-8 times a factor of order one (the third derivative along log kappa over the first; at
# 1e-3 kappa the IMEX case measures 1.7e-6), its rounding error 1e-16 |u| / (eps |du/dkappa|) ~ 1e-10: both below the gate.
CASES = {
    "ch_imex": ("ch2d", (24, 20), (1 / 24, 1 / 20), MOB, "imex", 1e-4),
    "ch_euler": ("ch2d", (24, 20), (1 / 24, 1 / 20), MOB, "euler", 2e-7),
    "ac_rk4": ("ac2d", (24, 20), (1 / 24, 1 / 20), RATE, "rk4", 1e-6),
    "ch3d_imex": ("ch3d", (10, 8, 6), (1 / 10, 1 / 8, 1 / 6), MOB, "imex", 1e-4),
}


@pytest.mark.parametrize("case", list(CASES))
def test_kappa_tangent_matches_central_differences_of_the_oracle(case):
    eq, shape, h, mob, integrator, dt = CASES[case]
    u0 = _state(shape, 3)
    n = 20
    params = [(K.MU_ROLE, 1), (K.KAPPA_ROLE, 0), (K.MOB_ROLE, 0)]
    u, dus = K.trajectory(eq, u0, params, dt, n, h, KAPPA, MU, mob, integrator, 0.5, K.symbol_of(shape, h, KAPPA))
    # the base of the reference is the oracle's trajectory
    assert np.max(np.abs(u - K.end_state(eq, u0, dt, n, h, KAPPA, MU, mob, integrator))) <= 1e-13
    eps = 1e-4 * KAPPA
    want = (K.end_state(eq, u0, dt, n, h, KAPPA + eps, MU, mob, integrator)
            - K.end_state(eq, u0, dt, n, h, KAPPA - eps, MU, mob, integrator)) / (2 * eps)
    err = float(np.max(np.abs(dus[1] - want)) / np.max(np.abs(want)))
    print(f"{case}: max |d - cd| / max |cd| = {err:.3e}")
    assert err <= 1e-6
    # the closure tangents next to it are the ones tests/sens_ref*.py give (kappa changes nothing for them)
    _, alone = K.trajectory(eq, u0, [params[0], params[2]], dt, n, h, KAPPA, MU, mob, integrator, 0.5, K.symbol_of(shape, h, KAPPA))
    assert np.array_equal(alone[0], dus[0]) and np.array_equal(alone[1], dus[2])


def test_imex_kappa_tangent_needs_the_operator_term():
    """without -dt Re ifftn(A dt (symbol / kappa) fftn(f) / L^2) the tangent is wrong by far more than the gate"""
    eq, shape, h, mob, _, dt = CASES["ch_imex"]
    u0 = _state(shape, 3)
    sym = K.symbol_of(shape, h, KAPPA)
    _, (with_term,) = K.trajectory(eq, u0, [(K.KAPPA_ROLE, 0)], dt, 20, h, KAPPA, MU, mob, "imex", 0.5, sym)
    u, du = u0, np.zeros_like(u0)
    for _ in range(20):  # the same solve applied to the linearised slope only
        f = K.rhs(eq, u, h, KAPPA, MU, mob)
        df = K.tangent_rhs(eq, u, du, h, KAPPA, MU, mob, K.KAPPA_ROLE, 0)
        solve = lambda g: np.fft.ifftn(np.fft.fftn(g) / (1 + 0.5 * dt * sym)).real
        u, du = u + dt * solve(f), du + dt * solve(df)
    assert np.max(np.abs(du - with_term)) > 1e-3 * np.max(np.abs(with_term))


# ---- ParamMap with a TrainableScalar ---------------------------------------------------------------------------------


def _logit(c):
    return np.log(c / (1 - c))


def _opt(kappa):
    return {"mu": ChemLeg(np.array([0.0, -2.0]), _logit), "kappa": kappa, "D": DiffLeg(np.array([0.1, 0.2]))}


def test_trainable_scalar_is_a_number():
    x = TrainableScalar(0.002)
    assert float(x) == 0.002 and x.value == 0.002 and x.positive
    assert x.variable() == math.log(0.002) and x.column_factor() == 0.002
    y = x.with_variable(math.log(0.004))
    assert isinstance(y, TrainableScalar) and abs(y.value - 0.004) < 1e-17 and y.positive  # exp(log(x)): an ulp
    z = TrainableScalar(-1.5, positive=False)
    assert z.variable() == -1.5 and z.column_factor() == 1.0 and z.with_variable(2.0).value == 2.0
    with pytest.raises(ValueError):
        TrainableScalar(0.0)
    with pytest.raises(ValueError):
        TrainableScalar(float("nan"), positive=False)
    from pde_opt_amd.numerics.functions.scalar import TrainableScalar as T2

    assert T2 is TrainableScalar


def test_param_map_orders_scalar_entries_with_the_closures():
    pm = fit.ParamMap.of(_opt(TrainableScalar(0.002)), P.CahnHilliard2DPeriodic)
    assert pm.keys == ["mu", "kappa", "D"] and pm.sizes == [2, 1, 2] and pm.size == 5
    assert pm.all_params() == [(L.SENS_MU, 0), (L.SENS_MU, 1), (L.SENS_KAPPA, 0), (L.SENS_MOB, 0), (L.SENS_MOB, 1)]
    assert L.SENS_KAPPA == 2
    # Cahn-Hilliard: mu's constant coefficient is inert, kappa is active
    assert pm.active().tolist() == [False, True, True, True, True]
    assert pm.sens_params() == [(L.SENS_MU, 1), (L.SENS_KAPPA, 0), (L.SENS_MOB, 0), (L.SENS_MOB, 1)]
    ac = fit.ParamMap.of({"kappa": TrainableScalar(0.002), "R": DiffLeg(np.array([0.1]))}, P.AllenCahn2DPeriodic)
    assert ac.active().tolist() == [True, True] and ac.sens_params() == [(L.SENS_KAPPA, 0), (L.SENS_MOB, 0)]
    alone = fit.ParamMap.of({"kappa": TrainableScalar(0.002)}, P.CahnHilliard3DPeriodic)
    assert alone.sens_params() == [(L.SENS_KAPPA, 0)]


@pytest.mark.parametrize("positive", [True, False])
def test_param_map_variable_column_factor_and_round_trip(positive):
    opt = _opt(TrainableScalar(0.002, positive=positive))
    pm = fit.ParamMap.of(opt, P.CahnHilliard2DPeriodic)
    p = pm.flatten(opt)
    assert p.tolist() == [0.0, -2.0, math.log(0.002) if positive else 0.002, 0.1, 0.2]
    np.testing.assert_allclose(pm.column_factors(p), [1.0, 1.0, 0.002 if positive else 1.0, 1.0, 1.0], rtol=1e-15, atol=0)
    back = pm.build(p)
    assert isinstance(back["kappa"], TrainableScalar) and back["kappa"].positive is positive
    assert abs(back["kappa"].value - 0.002) <= 1e-17
    assert isinstance(back["mu"], ChemLeg) and back["mu"].prior_fn is _logit and isinstance(back["D"], DiffLeg)
    np.testing.assert_allclose(pm.flatten(back), p, rtol=1e-15, atol=0)
    assert fit.plain(back)["kappa"] == back["kappa"].value and fit.plain(back)["mu"] is back["mu"]
    # a moved variable
    q = p.copy()
    q[2] = math.log(0.005) if positive else 0.005
    assert abs(pm.build(q)["kappa"].value - 0.005) <= 1e-17
    assert abs(pm.column_factors(q)[2] - (0.005 if positive else 1.0)) <= 1e-17
    # the sums of the value-derivatives become sums of the variable-derivatives
    rdp, G = pm.scale_sums(q, np.arange(1.0, 6.0), np.ones((5, 5)))
    s = pm.column_factors(q)
    np.testing.assert_array_equal(rdp, np.arange(1.0, 6.0) * s)
    np.testing.assert_array_equal(G, np.outer(s, s))
    # feasibility: only a positive=False scalar can leave the domain of the equation
    q[2] = -0.001
    assert pm.feasible(q) is positive and pm.feasible(p)
    if positive:
        assert pm.build(q)["kappa"].value > 0.0


def test_weights_of_a_scalar_weigh_the_optimisers_variable():
    opt = _opt(TrainableScalar(0.002))
    pm = fit.ParamMap.of(opt, P.CahnHilliard2DPeriodic)
    np.testing.assert_array_equal(fit.weight_vector(pm, {"kappa": 3.0}), [0, 0, 3.0, 0, 0])
    np.testing.assert_array_equal(fit.weight_vector(pm, {"kappa": None, "D": DiffLeg(np.array([1.0, 2.0]))}), [0, 0, 0, 1.0, 2.0])
    np.testing.assert_array_equal(fit.weight_vector(pm, {}), np.zeros(5))
    q = math.log(0.002)
    assert abs(fit.regularization(opt, {"kappa": 3.0}, 0.5) - 0.5 * 3.0 * q * q) <= 1e-12
    assert fit.regularization(opt, {"kappa": None}, 0.5) == 0.0 and fit.regularization(opt, {}, 0.5) == 0.0
    # the Objective's regulariser is the same number and its gradient is with respect to the variable
    obj = fit.Objective(sums=None, ssr=None, M=1, lambda_reg=0.5, w=fit.weight_vector(pm, {"kappa": 3.0}))
    p = pm.flatten(opt)
    assert abs(obj.reg(p) - 0.5 * 3.0 * q * q) <= 1e-12 and abs(obj.reg_grad(p)[2] - 2 * 0.5 * 3.0 * q) <= 1e-12


# ---- refusals ------------------------------------------------------------------------------------------------------


def test_a_plain_float_is_still_refused():
    with pytest.raises(fit.NotTrainableError, match="kappa"):
        fit.ParamMap.of({"mu": ChemLeg(np.array([0.0, -2.0]), _logit), "kappa": 0.002}, P.CahnHilliard2DPeriodic)
    with pytest.raises(ValueError, match="kappa"):
        fit.ParamMap.of({"kappa": 0.002}, P.AllenCahn2DPeriodic)
    with pytest.raises(fit.NotTrainableError):  # a TrainableScalar is kappa's: no other key takes one
        fit.ParamMap.of({"alpha": TrainableScalar(0.5)}, P.CahnHilliard2DPeriodic)


@pytest.mark.parametrize("cls", ["AllenCahn2DSmoothedBoundary", "CahnHilliard2DSmoothedBoundary", "AllenCahn2DPeriodicButlerVolmer",
                                 "AllenCahn2DPeriodicButlerVolmerConstantCurrent",
                                 "AllenCahn2DSmoothedBoundaryButlerVolmerConstantCurrent"])
def test_smoothed_boundary_and_butler_volmer_refuse_a_trainable_kappa(cls):
    with pytest.raises(fit.NotTrainableError, match="kappa"):
        fit.ParamMap.of({"mu": ChemLeg(np.array([0.0, -2.0]), _logit), "kappa": TrainableScalar(0.002)}, getattr(P, cls))


# ---- PDEModel.train on a test double of the engine --------------------------------------------------------------------


class SensOracleEngine(OracleEngine):
    """OracleEngine with the sensitivity calls fit.sensitivity_solve makes, backed by tests/sens_kappa_ref.py.  It
    records the kappa of every configure: what reached the engine."""

    def __init__(self):
        super().__init__()
        self.kappas = []

    def configure(self, **kw):
        self.kappas.append(float(kw.get("kappa", 0.0)))
        super().configure(**kw)

    def sens_configure(self, n_traj, params):
        self.sens_shape, self.sens_params = (int(n_traj), len(params)), list(params)

    def sens_set_data(self, frames):
        self.frames = np.asarray(frames, dtype=np.float64)

    def sens_advance(self, integrator, dt, n, t0=0.0):
        B, Pn = self.sens_shape
        eq = "ch2d" if self.eq == L.EQ_CAHN_HILLIARD else "ac2d"
        name = {L.INT_EULER: "euler", L.INT_RK4: "rk4", L.INT_IMEX: "imex"}[integrator]
        for b in range(B):
            u, dus = self.y[b], [self.y[B + j * B + b] for j in range(Pn)]
            for _ in range(int(n)):
                u, dus = K.step(eq, u, dus, self.sens_params, dt, (self.hx, self.hy), self.kappa, self.mu, self.mob, name,
                                self.imex_A, self.symbol)
            self.y[b] = u
            for j in range(Pn):
                self.y[B + j * B + b] = dus[j]

    def sens_accumulate(self, frame, theta=1.0, interp=False):
        B, Pn = self.sens_shape
        y = self.snap + theta * (self.y - self.snap) if interp else self.y
        out = np.zeros((B, 1 + Pn + Pn * (Pn + 1) // 2))
        for b in range(B):
            rows = [self.frames[frame, b] - y[b]] + [y[B + j * B + b] for j in range(Pn)]
            out[b, :1 + Pn] = [np.sum(rows[0] * r) for r in rows]
            out[b, 1 + Pn:] = [np.sum(rows[1 + i] * rows[1 + j]) for i in range(Pn) for j in range(i, Pn)]
        return out


N = 12
TS = np.array([0.0, 2e-5, 4e-5])
TRUE = {"mu": ChemLeg(np.array([0.0, -3.0]), _logit), "D": DiffLeg(np.array([0.0])), "kappa": 0.002}


def _fit_problem():
    model = P.PDEModel(P.CahnHilliard2DPeriodic, P.Domain((N, N), ((0.0, 1.0), (0.0, 1.0)), "dimensionless"), P.Euler)
    model._engine, model._sens_eng = OracleEngine(), SensOracleEngine()
    x = np.arange(N) / N
    y0s = np.stack([0.5 + 0.1 * np.cos(2 * np.pi * (x[:, None] + s * x[None, :]) + s) for s in (1, 2)])
    return model, y0s


def _data(model, y0s, dt0):
    orig = model.solve
    model.solve = lambda *a, **k: orig(*a, **{**k, "dt0": dt0})  # the explicit step of a 12 x 12 grid; train's is fixed
    sol = model.solve(TRUE, y0s, TS, {})
    T = len(TS)
    data = {"ys": [sol[q, b] for b in range(2) for q in range(T)], "ts": np.tile(TS, 2)}
    return data, [[b * T + q for q in range(T)] for b in range(2)]


def test_solve_unwraps_a_trainable_scalar():
    model, y0s = _fit_problem()
    a = model.solve(TRUE, y0s, TS, {}, dt0=2e-7)
    b = model.solve({**TRUE, "kappa": TrainableScalar(0.002)}, y0s, TS, {}, dt0=2e-7)
    assert np.array_equal(a, b)
    # residuals and mse take the same dict
    values = np.swapaxes(a, 0, 1)[:, 1:]
    orig = model.solve
    model.solve = lambda *x, **k: orig(*x, **{**k, "dt0": 2e-7})
    assert model.mse({**TRUE, "kappa": TrainableScalar(0.002)}, (y0s, values), {}, TS, {}, 0.0) == 0.0


def _capture_objective(monkeypatch, model, data, inds, opt, other, method="least_squares"):
    """PDEModel.train's Objective and starting point, handed to the optimiser"""
    seen = {}

    def grab(obj, p0, max_steps=100, **kw):
        seen["obj"], seen["p0"] = obj, np.array(p0)
        return np.array(p0), [0.0]

    monkeypatch.setattr(fit, "levenberg_marquardt" if method == "least_squares" else "bfgs", grab)
    monkeypatch.setattr(fit, "sensitivity_solve", _with_dt0(fit.sensitivity_solve, 2e-7))
    res = model.train(data, inds, opt, other, {}, {}, 0.0, method=method)
    return seen["obj"], seen["p0"], res


def _with_dt0(fn, dt0):
    return lambda *a, **k: fn(*a, **{**k, "dt0": dt0})


@pytest.mark.parametrize("positive", [True, False])
def test_train_scales_the_kappa_column_by_kappa(monkeypatch, positive):
    model, y0s = _fit_problem()
    data, inds = _data(model, y0s, 2e-7)
    opt = {"mu": ChemLeg(np.array([0.0, -2.5]), _logit), "kappa": TrainableScalar(0.003, positive=positive)}
    obj, p0, res = _capture_objective(monkeypatch, model, data, inds, opt, {"D": TRUE["D"]})
    assert isinstance(res["kappa"], TrainableScalar) and abs(res["kappa"].value - 0.003) < 1e-15 and res["D"] is TRUE["D"]
    ssr, rdp, G = obj.sums(p0)
    assert model._sens_eng.sens_params == [(L.SENS_MU, 1), (L.SENS_KAPPA, 0)] and abs(model._sens_eng.kappas[-1] - 0.003) < 1e-17
    # central differences of the forward objective in the optimiser's variable: d(ssr / 2)/dp = -rdp
    for j in (1, 2):
        e = np.zeros(3)
        e[j] = 1e-6 * max(1.0, abs(p0[j])) if positive or j == 1 else 1e-9
        cd = (obj.ssr(p0 + e) - obj.ssr(p0 - e)) / (2 * e[j])
        assert abs(-2 * rdp[j] - cd) <= 1e-5 * abs(cd), (j, rdp[j], cd)
    assert rdp[0] == 0.0 and G[0, 0] == 0.0 and G[2, 2] > 0.0
    assert abs(obj.ssr(p0) - ssr) <= 1e-12 * ssr


@pytest.mark.parametrize("method", ["least_squares", "mse"])
def test_a_trial_with_kappa_not_positive_never_reaches_the_engine(monkeypatch, method):
    model, y0s = _fit_problem()
    data, inds = _data(model, y0s, 2e-7)
    opt = {"kappa": TrainableScalar(0.003, positive=False)}
    obj, p0, _ = _capture_objective(monkeypatch, model, data, inds, opt, {"mu": TRUE["mu"], "D": TRUE["D"]}, method)
    sens, fwd = model._sens_eng, model._engine
    n_sens, n_fwd = len(sens.kappas), len(fwd.calls)
    for bad in (-0.001, 0.0, float("nan")):
        s = obj.sums(np.array([bad]))
        assert s[0] == math.inf and s[1].shape == (1,) and s[2].shape == (1, 1)
        assert obj.ssr(np.array([bad])) == math.inf
    assert len(sens.kappas) == n_sens and len(fwd.calls) == n_fwd  # nothing was configured, nothing advanced
    assert math.isfinite(obj.sums(p0)[0]) and len(sens.kappas) == n_sens + 1 and all(k > 0 for k in sens.kappas)


def test_optimisers_treat_an_infeasible_trial_as_a_rejected_step():
    """f(p) = (p - 1)^2 / 2 on p > 0 from a start whose first Gauss-Newton step overshoots below zero: the drivers must
    come back with p > 0 without ever evaluating the model there"""
    asked = []

    def sums(p):
        asked.append(float(p[0]))
        if p[0] <= 0:
            return math.inf, np.zeros(1), np.zeros((1, 1))
        r = np.array([1.0 - p[0] ** 3])  # pred = p^3: a Gauss-Newton step from 0.05 jumps far
        J = np.array([3 * p[0] ** 2])
        return float(r @ r), J * r, np.outer(J, J)

    obj = fit.Objective(sums=sums, ssr=lambda p: sums(p)[0], M=1)
    for method in (fit.levenberg_marquardt, fit.bfgs):
        p, hist = method(obj, np.array([3.0]), max_steps=200)
        assert p[0] > 0 and abs(p[0] - 1.0) < 1e-4 and all(math.isfinite(h) for h in hist)


def test_train_fits_kappa_and_mu_on_the_test_double(monkeypatch):
    """end to end through Levenberg-Marquardt with the reference's tangents: kappa comes back from 0.003 to 0.002"""
    model, y0s = _fit_problem()
    data, inds = _data(model, y0s, 2e-7)
    monkeypatch.setattr(fit, "sensitivity_solve", _with_dt0(fit.sensitivity_solve, 2e-7))
    opt = {"kappa": TrainableScalar(0.003), "mu": ChemLeg(np.array([0.0, -2.6]), _logit)}
    res = model.train(data, inds, opt, {"D": TRUE["D"]}, {}, {}, 0.0, max_steps=30)
    assert list(res)[:2] == ["kappa", "mu"] and isinstance(res["kappa"], TrainableScalar)
    assert abs(res["kappa"].value - 0.002) <= 1e-6 * 0.002 and abs(res["mu"].expansion.params[1] + 3.0) <= 1e-6
    # solve takes train's return value as it is
    assert model.solve(res, y0s, TS, {}).shape == (3, 2, N, N)
