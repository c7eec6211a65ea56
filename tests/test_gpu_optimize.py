"""PDEModel.optimize on the MI355X: the contraction kernel (pdeopt_sens_contract) against fp64 sums of the fields read
back, its determinism, its agreement with the Gauss-Newton kernel, the gradient of an objective against the numpy
tangent references and against central differences of PDEModel.solve, and an optimisation end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pde_opt_amd as P
from pde_opt_amd import fit
from pde_opt_amd.engine import HipEngine
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg
import ac_fit_problem as F
import optimize_ref as R
import sens_ref as S
import sens_ref3d as S3
import sens_ref_ac as SA

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAPPA = 0.002
MU, D = (0.1, -3.0, 0.4, 0.2), (-0.3, 0.2)
ALL_PARAMS = [(S.MU_ROLE, 1), (S.MOB_ROLE, 0), (S.MU_ROLE, 2), (S.MOB_ROLE, 1), (S.MU_ROLE, 3)]
# a block of the contraction covers 2048 cells
SHAPES = {
    "8x8": (8, 8),              # far below a block
    "33x47": (33, 47),          # one partial block
    "47x45": (47, 45),          # a full block plus 67 cells
    "64x64": (64, 64),          # exactly two blocks
    "12x10x9": (12, 10, 9),     # 3-D, one partial block
    "16x16x9": (16, 16, 9),     # 3-D, 2048 + 256
}


def _equation(shape):
    dom = P.Domain(shape, ((0.0, 1.0),) * len(shape), "dimensionless")
    cls = P.CahnHilliard2DPeriodic if len(shape) == 2 else P.CahnHilliard3DPeriodic
    return cls(dom, KAPPA, ChemLeg(np.array(MU), F.logit), DiffLeg(np.array(D)))


def _loaded_engine(shape, B, Pn, dtype, seed):
    """an engine whose snapshot and state are two different random batches, and cotangents g (2, B, *shape) with sign
    changes; save point 1 of g is the one the tests contract"""
    rng = np.random.default_rng(seed)
    eq = _equation(shape)
    eng = HipEngine()
    eng.configure(dtype=dtype, batch=(1 + Pn) * B, **eq._engine_problem())
    eq._engine_upload(eng, 0.0, 1.0)
    eng.sens_configure(B, ALL_PARAMS[:Pn])
    eng.set_state(rng.standard_normal(((1 + Pn) * B,) + shape).astype(dtype))
    eng.snapshot()
    eng.set_state(rng.standard_normal(((1 + Pn) * B,) + shape).astype(dtype))
    g = rng.standard_normal((2, B) + shape).astype(dtype)
    eng.sens_set_data(g)
    return eng, g


def _check_contraction(got, g, fields, B, Pn):
    """per entry within cells 2^-53 sum |g dpred|: the worst case of an fp64 sum of that length (the products of two
    fp32 values are exact in fp64, those of fp64 values add one rounding each, inside the same bound's first order)"""
    cells = g[0].size
    for b in range(B):
        for j in range(Pn):
            prod = g[b].astype(np.float64) * fields[B + j * B + b].astype(np.float64)
            assert abs(got[b, j] - np.sum(prod)) <= cells * 2.0 ** -53 * np.sum(np.abs(prod)), (b, j)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("Pn", [1, 5])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_contraction_matches_fp64_sums_of_the_fields(shape, B, Pn, dtype):
    eng, g = _loaded_engine(SHAPES[shape], B, Pn, dtype, 11)
    edge = eng.sens_contract(1)
    assert edge.shape == (B, Pn) and edge.dtype == np.float64
    _check_contraction(edge, g[1], eng.get_state(), B, Pn)
    inside = eng.sens_contract(1, 0.37, True)
    _check_contraction(inside, g[1], eng.get_interpolated(0.37), B, Pn)
    assert np.all(edge != inside)
    # no atomics: repeated calls give identical bits
    assert eng.sens_contract(1).tobytes() == edge.tobytes()
    assert eng.sens_contract(1, 0.37, True).tobytes() == inside.tobytes()


def test_contract_errors():
    eng, _ = _loaded_engine((8, 8), 1, 1, np.float64, 3)
    with pytest.raises(Exception, match="frame 2 of 2"):
        eng.sens_contract(2)
    fresh = HipEngine()
    eq = _equation((8, 8))
    fresh.configure(dtype=np.float64, batch=2, **eq._engine_problem())
    fresh.sens_configure(1, ALL_PARAMS[:1])
    fresh.set_state(np.zeros((2, 8, 8)))
    fresh.sens_set_data(np.zeros((1, 1, 8, 8)))
    with pytest.raises(Exception, match="snapshot"):
        fresh.sens_contract(0, 0.5, True)


@pytest.mark.parametrize("interp", [False, True])
@pytest.mark.parametrize("shape", ["47x45", "16x16x9"])
def test_contraction_equals_the_gauss_newton_kernels_r_dpred(shape, interp):
    B, Pn = 3, 5
    eng, data = _loaded_engine(SHAPES[shape], B, Pn, np.float64, 5)
    theta = 0.37 if interp else 1.0
    sums = eng.sens_accumulate(1, theta, interp)
    fields = eng.get_interpolated(theta) if interp else eng.get_state()
    r = data[1] - fields[:B]  # fp64: the residual the kernel forms, bit for bit
    eng.sens_set_data(np.stack([data[0], r]))
    got = eng.sens_contract(1, theta, interp)
    cells = r[0].size
    for b in range(B):
        for j in range(Pn):
            bound = cells * 2.0 ** -53 * np.sum(np.abs(r[b] * fields[B + j * B + b]))
            assert abs(got[b, j] - sums[b, 1 + j]) <= bound, (b, j)


# ---- the gradient of an objective ---------------------------------------------------------------------------------------

TS = np.array([0.0, 0.7535e-4, 2e-4])  # dt0 = 1e-6: 200 substeps, the middle point 0.35 into step 76


def _smooth(shape, seed):
    rng = np.random.default_rng(seed)
    x = [np.arange(n) / n for n in shape]
    u = 0.5 + np.zeros(shape)
    for _ in range(6):
        k = rng.integers(1, 3, len(shape))
        ph = sum(k[a] * x[a].reshape([-1 if i == a else 1 for i in range(len(shape))]) for a in range(len(shape)))
        u += 0.04 * rng.standard_normal() * np.cos(2 * np.pi * ph + rng.uniform(0, 6))
    return u


def _case(name):
    """(model, opt, other, solver_parameters, y0 (B, *shape), stepper of the numpy reference)"""
    if name == "ac2d_rk4":
        shape, opt = (16, 32), {"mu": ChemLeg(np.array([0.1, -3.0, 0.3]), F.logit), "R": DiffLeg(np.array([6.9, 0.3]))}
        dom = P.Domain(shape, ((0.0, 1.0), (0.0, 1.0)), "dimensionless")
        model, sp = P.PDEModel(P.AllenCahn2DPeriodic, dom, P.RK4), {}
        eq = P.AllenCahn2DPeriodic(dom, KAPPA, **opt)
        hx, hy = dom.dx
        step = lambda u, dus, params: SA.step(u, dus, params, 1e-6, hx, hy, KAPPA, eq._mu_desc, eq._mob_desc, "rk4")
    else:
        shape = (16, 32) if name == "ch2d_imex" else (12, 12, 12)
        opt = {"mu": ChemLeg(np.array([0.0, -3.0, 0.2]), F.logit), "D": DiffLeg(np.array([-1.0, 0.2]))}
        dom = P.Domain(shape, tuple((-0.005 * n, 0.005 * n) for n in shape), "dimensionless")
        cls = P.CahnHilliard2DPeriodic if len(shape) == 2 else P.CahnHilliard3DPeriodic
        model, sp = P.PDEModel(cls, dom, P.SemiImplicitFourierSpectral), {"A": 0.5}
        eq = cls(dom, KAPPA, **opt)
        sym = np.asarray(eq.fourier_symbol)
        if len(shape) == 2:
            hx, hy = dom.dx
            step = lambda u, dus, params: S.step(u, dus, params, 1e-6, hx, hy, KAPPA, eq._mu_desc, eq._mob_desc, "imex", 0.5, sym)
        else:
            step = lambda u, dus, params: S3.step(u, dus, params, 1e-6, dom.dx, KAPPA, eq._mu_desc, eq._mob_desc, "imex", 0.5, sym)
    y0 = np.stack([_smooth(shape, s) for s in (1, 2)])
    return model, opt, {"kappa": KAPPA}, sp, y0, step


@pytest.mark.parametrize("name", ["ch2d_imex", "ac2d_rk4", "ch3d_imex"])
def test_objective_gradient(name):
    model, opt, other, sp, y0, step = _case(name)
    target = torch.tensor(np.stack([_smooth(y0.shape[1:], s) for s in (7, 8)]))

    def objective(ys):
        return torch.mean((ys[-1] - target) ** 2) + 0.1 * torch.mean(ys[1] ** 2)

    vg, v, pmap = model._objective_functions(objective, y0, TS, opt, other, sp, {}, 0.0)
    p = pmap.flatten(opt)
    J, grad = vg(p)
    assert abs(J - v(p)) <= 1e-15 * abs(J)
    act = np.nonzero(pmap.active())[0]
    assert np.all(grad[~pmap.active()] == 0.0) and np.all(grad[act] != 0.0)
    scale = np.max(np.abs(grad))
    # the numpy references: tangents at steps 75, 76 (interpolated at 0.35) and 200, contracted with the same cotangents
    ys = model.solve({**opt, **other}, y0, TS, sp)
    g = fit.torch_objective(objective).value_and_grad(ys)[1]
    params = pmap.sens_params()
    want = np.zeros(len(params))
    for b in range(len(y0)):
        (_, d75), (_, d76), (_, d200) = R.frames_of(step, y0[b], params, [75, 1, 124])
        for j in range(len(params)):
            want[j] += np.sum(g[1, b] * (d75[j] + 0.35 * (d76[j] - d75[j]))) + np.sum(g[2, b] * d200[j])
    print(name, "grad", grad, "vs reference", np.max(np.abs(grad[act] - want)) / scale)
    assert np.max(np.abs(grad[act] - want)) <= 1e-10 * scale  # test_gpu_sens_ac.py's gate of tangents against the reference
    # central differences of PDEModel.solve under the objective
    eps = 1e-4
    cd = np.array([(v(p + eps * e) - v(p - eps * e)) / (2 * eps) for e in np.eye(len(p))])
    print(name, "vs central differences", np.max(np.abs(grad - cd)) / scale)
    assert np.max(np.abs(grad - cd)) <= 1e-6 * scale  # that file's gate of tangents against central differences


# The same optimisation on the CPU (fp64 numpy tangents under the same BFGS: `python tests/optimize_ref.py`) ends at
#   max |p - p_true| = 2.725e-11, J = 6.901e-25   (48 BFGS steps from J = 8.731e-04)
# The final frame alone identifies all five coefficients there, so the objective needs no intermediate frame.  The GPU
# run is gated at 10 x those values.
CPU_OPTIMIZE = (2.725e-11, 6.901e-25)


def test_optimize_recovers_coefficients_from_the_final_frame():
    dom = P.Domain((F.N, F.N), ((0.0, 1.0), (0.0, 1.0)), "dimensionless")
    model = P.PDEModel(P.AllenCahn2DPeriodic, dom, P.RK4)
    truth = {"mu": ChemLeg(np.array(F.MU_TRUE), F.logit), "R": DiffLeg(np.array(F.R_TRUE)), "kappa": F.KAPPA}
    y0s = F.y0s()
    target = torch.tensor(model.solve(truth, y0s, R.E2E_TS, {})[-1])

    def objective(ys):
        return torch.mean((ys[-1] - target) ** 2)

    init = {"mu": ChemLeg(np.array(F.MU_INIT), F.logit), "R": DiffLeg(np.array(F.R_INIT))}
    res = model.optimize(objective, y0s, R.E2E_TS, init, {"kappa": F.KAPPA}, {}, {}, 0.0, max_steps=100)
    p = np.concatenate([res["mu"].expansion.params, res["R"].expansion.params])
    err = float(np.max(np.abs(p - np.array(F.MU_TRUE + F.R_TRUE))))
    final = float(objective(torch.tensor(model.solve(res, y0s, R.E2E_TS, {}))))
    hist = model.last_optimize_history
    print(f"optimize: max |p - p_true| = {err:.3e}, J = {final:.3e}, {len(hist) - 1} steps from J = {hist[0]:.3e}")
    assert isinstance(res["mu"], ChemLeg) and res["mu"].prior_fn is F.logit and isinstance(res["R"], DiffLeg)
    assert res["kappa"] == F.KAPPA
    assert err <= 10 * CPU_OPTIMIZE[0]
    assert final <= 10 * CPU_OPTIMIZE[1]


def test_optimize_objective_example_runs():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "optimize_objective.py"), "--quick"], env=env,
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
