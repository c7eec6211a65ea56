"""kappa as a trainable scalar on the MI355X: the kappa slope and tangent trajectories of the three periodic equations
against the numpy reference (tests/sens_kappa_ref.py), the bits of the base and of the other tangents with and without a
kappa tangent, pdeopt_sens_configure's refusals, and PDEModel.train / optimize with a TrainableScalar."""
import numpy as np
import pytest

import kappa_fit_problem as F
import pde_opt_amd as P
import sens_kappa_ref as K
from pde_opt_amd import _lib as L
from pde_opt_amd import fit
from pde_opt_amd.engine import HipEngine
from pde_opt_amd.numerics.functions import TrainableScalar
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg

pytestmark = pytest.mark.gpu

KAPPA = 0.002
MU3 = (0.1, -3.0, 0.4)
SECOND = (-0.3, 0.2)  # D of Cahn-Hilliard, R of Allen-Cahn: exp of a Legendre series
KR = (K.KAPPA_ROLE, 0)
# kappa alone; first, in the middle and last among mu and D / R entries
ROLE_LISTS = {
    "alone": [KR],
    "first": [KR, (K.MU_ROLE, 1), (K.MOB_ROLE, 0)],
    "middle": [(K.MU_ROLE, 1), KR, (K.MOB_ROLE, 1)],
    "last": [(K.MU_ROLE, 2), (K.MOB_ROLE, 0), KR],
}
# the 2-D tangent kernels' tile is 16 x 32
SHAPES2 = {
    "8x8": ((8, 8), ((0.0, 1.0), (0.0, 1.0))),        # one partial tile
    "16x32": ((16, 32), ((0.0, 1.0), (0.0, 1.0))),    # exactly one tile
    "33x47": ((33, 47), ((0.0, 1.0), (0.0, 1.0))),    # ragged, several tiles, odd ny: Allen-Cahn's single-cell stores and loads
    "64x64": ((64, 64), ((0.0, 1.0), (0.0, 2.0))),    # hx != hy; a grid the hand-written FFT passes would take
}
SHAPES3 = {
    "8x8x8": ((8, 8, 8), ((0.0, 1.0),) * 3),
    "12x10x6": ((12, 10, 6), ((0.0, 1.2), (0.0, 0.8), (0.0, 0.9))),
}
EQS = {"ch2d": SHAPES2, "ac2d": SHAPES2, "ch3d": SHAPES3}
CASES = [(e, s) for e, shapes in EQS.items() for s in shapes]
# the gates tests/test_gpu_sens.py, test_gpu_sens_ac.py and test_gpu_sens3d.py hold the same kernels' other slopes to
RHS_TOL = {"ch2d": {np.float64: 1e-11, np.float32: 1e-4}, "ac2d": {np.float64: 1e-11, np.float32: 1e-4},
           "ch3d": {np.float64: 1e-12, np.float32: 1e-4}}
BASE_TOL, TRAJ_TOL = 1e-12, 1e-10  # those files' fp64 trajectory gates: the base block, every tangent


def _logit(c):
    return np.log(c / (1.0 - c))


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def _equation(eq, shape):
    points, box = EQS[eq][shape]
    dom = P.Domain(points, box, "dimensionless")
    cls = {"ch2d": P.CahnHilliard2DPeriodic, "ac2d": P.AllenCahn2DPeriodic, "ch3d": P.CahnHilliard3DPeriodic}[eq]
    return cls(dom, KAPPA, ChemLeg(np.array(MU3), _logit), DiffLeg(np.array(SECOND))), tuple(float(d) for d in dom.dx)


def _state(points, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return np.clip(0.5 + 0.1 * rng.standard_normal(points), 0.1, 0.9).astype(dtype)


def _smooth(points, seed):
    rng = np.random.default_rng(seed)
    x = [np.arange(n) / n for n in points]
    u = 0.5 + np.zeros(points)
    for _ in range(6):
        k = rng.integers(1, 3, len(points))
        ph = sum(k[a] * x[a].reshape([-1 if i == a else 1 for i in range(len(points))]) for a in range(len(points)))
        u += 0.04 * rng.standard_normal() * np.cos(2 * np.pi * ph + rng.uniform(0, 6))
    return u


def _load(eng, eq, solver, base, tangents, params):
    """``eng`` configured for the (1 + P) B batch of ``base`` (B, *points) and ``tangents`` (P B, *points)"""
    B = base.shape[0]
    eng.configure(dtype=base.dtype, batch=(1 + len(params)) * B, **eq._engine_problem())
    eq._engine_upload(eng, 0.0, 1.0)
    if solver is not None:
        solver.configure_engine(eng, eq)
    eng.sens_configure(B, params)
    eng.set_state(np.concatenate([base, tangents]))


@pytest.fixture(scope="module")
def eng():
    e = HipEngine()
    yield e
    e.close()


@pytest.mark.parametrize("eq,shape", CASES, ids=["%s-%s" % c for c in CASES])
def test_kappa_slope_matches_numpy_reference(eng, eq, shape):
    equation, h = _equation(eq, shape)
    points = EQS[eq][shape][0]
    mu, mob = equation._mu_desc, equation._mob_desc
    for dtype in (np.float64, np.float32):
        tol = RHS_TOL[eq][dtype]
        for B, name in ((1, "alone"), (3, "first"), (1, "middle"), (3, "last"), (3, "alone"), (1, "last")):
            params = ROLE_LISTS[name]
            base = np.stack([_state(points, 1 + b, dtype) for b in range(B)])
            tang = (0.05 * np.random.default_rng(7).standard_normal((len(params) * B,) + points)).astype(dtype)
            _load(eng, equation, None, base, tang, params)
            k = eng.sens_rhs()
            for b in range(B):
                u = base[b].astype(np.float64)
                assert _rel(k[b], K.rhs(eq, u, h, KAPPA, mu, mob)) <= max(tol, 1e-12), (dtype, B, name, b)
                for j, (role, kc) in enumerate(params):
                    du = tang[j * B + b].astype(np.float64)
                    want = K.tangent_rhs(eq, u, du, h, KAPPA, mu, mob, role, kc)
                    assert _rel(k[B + j * B + b], want) <= tol, (dtype, B, name, b, j)


INTEGRATORS = {"ch2d": ("imex", "euler"), "ac2d": ("euler", "rk4"), "ch3d": ("imex", "euler")}
DT = {("ch2d", "imex"): 1e-5, ("ch2d", "euler"): 2e-7, ("ac2d", "euler"): 1e-3, ("ac2d", "rk4"): 1e-3,
      ("ch3d", "imex"): 1e-5, ("ch3d", "euler"): 2e-7}
CODE = {"imex": L.INT_IMEX, "euler": L.INT_EULER, "rk4": L.INT_RK4}
TRAJ_CASES = [(e, i, s) for e, s in CASES for i in INTEGRATORS[e]]
N_SUB = 40


@pytest.mark.parametrize("eq,integrator,shape", TRAJ_CASES, ids=["%s-%s-%s" % c for c in TRAJ_CASES])
def test_tangent_trajectories_40_substeps(eng, eq, integrator, shape):
    equation, h = _equation(eq, shape)
    points = EQS[eq][shape][0]
    mu, mob = equation._mu_desc, equation._mob_desc
    dt = DT[(eq, integrator)]
    sym = np.asarray(equation.fourier_symbol) if integrator == "imex" else None
    solver = P.SemiImplicitFourierSpectral(A=0.5, fourier_symbol=equation.fourier_symbol) if integrator == "imex" else None
    if sym is not None:  # the class publishes kappa K2^2: what the kappa tangent of the operator takes for granted
        assert np.max(np.abs(sym - K.symbol_of(points, h, KAPPA))) <= 1e-12 * np.max(np.abs(sym))
    for B, name in ((1, "alone"), (3, "middle"), (1, "first"), (3, "last")):
        params = ROLE_LISTS[name]
        jk = params.index(KR)
        u0s = np.stack([_smooth(points, 3 + b) for b in range(B)])
        refs = [K.trajectory(eq, u0, params, dt, N_SUB, h, KAPPA, mu, mob, integrator, 0.5, sym) for u0 in u0s]
        _load(eng, equation, solver, u0s, np.zeros((len(params) * B,) + points), params)
        eng.sens_advance(CODE[integrator], dt, N_SUB)
        got = eng.get_state()
        kernel = eng.last_kernel
        assert ("imex_rocfft_r2c_kappa" in kernel) == (integrator == "imex"), kernel  # every grid, 64 x 64 included
        for b, (u_ref, dus) in enumerate(refs):
            assert _rel(got[b], u_ref) <= BASE_TOL, (B, name, b)
            for j in range(len(params)):
                assert _rel(got[B + j * B + b], dus[j]) <= TRAJ_TOL, (B, name, b, j)
        # fp32, the kappa column: the reference's own float32-versus-float64 distance, times 10
        refs32 = [K.trajectory(eq, u0.astype(np.float32), params, dt, N_SUB, h, KAPPA, mu, mob, integrator, 0.5, sym) for u0 in u0s]
        _load(eng, equation, solver, u0s.astype(np.float32), np.zeros((len(params) * B,) + points, np.float32), params)
        eng.sens_advance(CODE[integrator], dt, N_SUB)
        got32 = eng.get_state()
        for b in range(B):
            assert refs32[b][1][jk].dtype == np.float32
            cpu = _rel(refs32[b][1][jk], refs[b][1][jk])
            gpu = _rel(got32[B + jk * B + b], refs[b][1][jk])
            print(f"{eq} {integrator} {shape} B={B} {name} b={b}: fp32 kappa column, reference {cpu:.3e}, GPU {gpu:.3e}")
            assert gpu <= 10 * cpu, (B, name, b, gpu, cpu)


@pytest.mark.parametrize("eq,shape", [("ch2d", "33x47"), ("ch3d", "12x10x6")])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_base_and_other_tangents_keep_their_bits_next_to_a_kappa_tangent(eng, eq, shape, dtype):
    """roles [mu_1, kappa] against [mu_1, mu_2] under IMEX: the same batch, so the same rocFFT plans; the multiply of the
    kappa run must give the base block and the mu_1 tangent the bits of spectral_mul_kernel"""
    equation, _ = _equation(eq, shape)
    points = EQS[eq][shape][0]
    solver = P.SemiImplicitFourierSpectral(A=0.5, fourier_symbol=equation.fourier_symbol)
    B = 2
    u0s = np.stack([_smooth(points, 3 + b) for b in range(B)]).astype(dtype)

    def run(params):
        _load(eng, equation, solver, u0s, np.zeros((len(params) * B,) + points, dtype), params)
        eng.sens_advance(L.INT_IMEX, 1e-5, N_SUB)
        return eng.get_state()

    with_kappa = run([(K.MU_ROLE, 1), KR])
    without = run([(K.MU_ROLE, 1), (K.MU_ROLE, 2)])
    again = run([(K.MU_ROLE, 1), KR])
    assert with_kappa[:2 * B].tobytes() == without[:2 * B].tobytes()
    assert again.tobytes() == with_kappa.tobytes()
    assert np.all(np.isfinite(with_kappa)) and np.any(with_kappa[2 * B:] != 0)


def test_configure_refusals(eng):
    equation, _ = _equation("ch2d", "16x32")
    points = (16, 32)
    base = np.stack([_state(points, 1), _state(points, 2)])
    with pytest.raises(Exception, match="coef_index"):
        _load(eng, equation, None, base, np.zeros((2,) + points), [(L.SENS_KAPPA, 1)])
    with pytest.raises(Exception, match="twice"):
        _load(eng, equation, None, base, np.zeros((4,) + points), [KR, KR])
    # base environments with different kappa: the derivative is of one shared scalar
    eng.configure(dtype=np.float64, batch=4, **equation._engine_problem())
    equation._engine_upload(eng, 0.0, 1.0)
    eng.set_env_params(0, kappa=[0.002, 0.003, 0.002, 0.002])
    with pytest.raises(Exception, match="shared"):
        eng.sens_configure(2, [KR])
    eng.sens_configure(2, [(K.MU_ROLE, 1)])  # the closure roles do not mind
    eng.set_env_params(0, kappa=[0.003, 0.003, 0.1, 0.2])  # the tangent environments' kappa is never read
    eng.sens_configure(2, [KR])


def test_smoothed_boundary_and_butler_volmer_contexts_refuse_the_kappa_role():
    import bv_sens_ref as BS
    import sbm_sens_problem as SP
    from test_gpu_bv_sens import make_eq, values_of

    for name in ("ac", "ch"):
        p = SP.problem(name, "16x32")
        eq = SP.equation(P, p)
        e = HipEngine()
        e.configure(dtype=np.float64, batch=2, **eq._engine_problem())
        eq._engine_upload(e, 0.0, 1.0)
        with pytest.raises(Exception, match="PDEOPT_SENS_KAPPA"):
            e.sens_configure(1, [KR])
        e.sens_configure(1, [(K.MU_ROLE, 1)])
        e.close()
    for kind in ("voltage", "current"):
        eq = make_eq(kind, 16, 32, values_of(kind)[0])
        e = HipEngine()
        e.configure(dtype=np.float64, batch=2, **eq._engine_problem())
        eq._engine_upload(e, 0.0, 1.0)
        e.set_bv_params(BS.ALPHA, eq._mode, [values_of(kind)[0]])
        with pytest.raises(Exception, match="PDEOPT_SENS_KAPPA"):
            e.sens_configure(1, [KR])
        e.close()


# ---- end to end -----------------------------------------------------------------------------------------------------

# The same fits on the CPU (fp64 numpy tangents under the same Levenberg-Marquardt: `python tests/kappa_fit_problem.py`):
#   ch_imex: kappa = 2.000000000000e-03, ssr = 8.679e-28   (8 solves)
#   ac_rk4:  kappa = 1.999999999980e-03, ssr = 1.802e-23   (10 solves)
# and the GPU fit's final ssr is gated at 10 x those values.
CPU_SSR = {"ch_imex": 8.679e-28, "ac_rk4": 1.802e-23}


@pytest.mark.parametrize("name", ["ch_imex", "ac_rk4"])
def test_train_recovers_kappa_and_mu(name):
    _, _, mu_true, mu_init, second = F.CASES[name]
    dom = P.Domain(F.SHAPE, F.BOX, "dimensionless")
    if name == "ch_imex":
        model, sp, key = P.PDEModel(P.CahnHilliard2DPeriodic, dom, P.SemiImplicitFourierSpectral), {"A": 0.5}, "D"
    else:
        model, sp, key = P.PDEModel(P.AllenCahn2DPeriodic, dom, P.RK4), {}, "R"
    fixed = {key: DiffLeg(np.array(second))}
    truth = {"mu": ChemLeg(np.array(mu_true), F.logit), "kappa": F.KAPPA_TRUE, **fixed}
    y0s = F.y0s()
    sol = model.solve(truth, y0s, F.TS, sp)  # (T, B, nx, ny): noise-free synthetic data
    B, T = len(y0s), len(F.TS)
    data = {"ys": [sol[q, b] for b in range(B) for q in range(T)], "ts": np.tile(F.TS, B)}
    inds = [[b * T + q for q in range(T)] for b in range(B)]
    init = {"kappa": TrainableScalar(F.KAPPA_INIT), "mu": ChemLeg(np.array(mu_init), F.logit)}
    res = model.train(data, inds, init, fixed, sp, {}, 0.0, method="least_squares", max_steps=100)
    assert isinstance(res["kappa"], TrainableScalar) and isinstance(res["mu"], ChemLeg) and res["mu"].prior_fn is F.logit
    values = np.swapaxes(sol, 0, 1)[:, 1:]
    r, _ = model.residuals(res, (y0s, values), sp, F.TS, {}, 0.0)  # train's return value as it is
    ssr = float(np.sum(np.asarray(r, dtype=np.float64) ** 2))
    print(f"{name}: kappa = {res['kappa'].value:.12e}, mu = {res['mu'].expansion.params}, ssr = {ssr:.3e}, "
          f"{len(model.last_train_history)} accepted steps")
    assert abs(res["kappa"].value - F.KAPPA_TRUE) < 1e-3 * abs(F.KAPPA_INIT - F.KAPPA_TRUE)
    assert ssr <= 10 * CPU_SSR[name]


def test_optimize_gradient_with_kappa_alone():
    """PDEModel.optimize's gradient over log(kappa), kappa the only parameter, against the reference's tangents contracted
    with the same cotangents, at tests/test_gpu_optimize.py's fp64 gate"""
    import torch

    points = (16, 32)
    dom = P.Domain(points, ((-0.08, 0.08), (-0.16, 0.16)), "dimensionless")
    model = P.PDEModel(P.CahnHilliard2DPeriodic, dom, P.SemiImplicitFourierSpectral)
    other = {"mu": ChemLeg(np.array([0.0, -3.0, 0.2]), _logit), "D": DiffLeg(np.array([-1.0, 0.2]))}
    opt = {"kappa": TrainableScalar(KAPPA)}
    eq = P.CahnHilliard2DPeriodic(dom, KAPPA, **other)
    h, sym = tuple(float(d) for d in dom.dx), np.asarray(eq.fourier_symbol)
    y0 = np.stack([_smooth(points, s) for s in (1, 2)])
    ts = np.array([0.0, 0.6e-4, 1e-4])  # dt0 = 1e-6: both save points on step edges (60, 100)
    target = torch.tensor(np.stack([_smooth(points, s) for s in (7, 8)]))

    def objective(ys):
        return torch.mean((ys[-1] - target) ** 2) + 0.1 * torch.mean(ys[1] ** 2)

    vg, v, pmap = model._objective_functions(objective, y0, ts, opt, other, {"A": 0.5}, {}, 0.0)
    p = pmap.flatten(opt)
    assert p.tolist() == [np.log(KAPPA)]
    J, grad = vg(p)
    assert abs(J - v(p)) <= 1e-15 * abs(J)
    ys = model.solve({**opt, **other}, y0, ts, {"A": 0.5})
    g = fit.torch_objective(objective).value_and_grad(ys)[1]
    want = 0.0
    for b in range(2):
        u, dus = y0[b], [np.zeros(points)]
        for q, n in ((1, 60), (2, 40)):
            for _ in range(n):
                u, dus = K.step("ch2d", u, dus, [KR], 1e-6, h, KAPPA, eq._mu_desc, eq._mob_desc, "imex", 0.5, sym)
            want += np.sum(g[q, b] * dus[0])
    want *= KAPPA  # d / d log(kappa)
    print("optimize: dJ/dlog(kappa) =", grad[0], "reference", want, "rel", abs(grad[0] - want) / abs(want))
    assert abs(grad[0] - want) <= 1e-10 * abs(grad[0])
    eps = 1e-5
    cd = (v(p + eps) - v(p - eps)) / (2 * eps)
    assert abs(grad[0] - cd) <= 1e-6 * abs(grad[0])
    res = model.optimize(objective, y0, ts, opt, other, {"A": 0.5}, max_steps=2)
    assert isinstance(res["kappa"], TrainableScalar) and res["kappa"].value > 0 and res["mu"] is other["mu"]
    assert model.last_optimize_history[-1] <= model.last_optimize_history[0]
