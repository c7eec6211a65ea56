"""A torch.nn.Module as mu on the MI355X: the field-mu right-hand side against the numpy oracle, the adjoint kernel
against the autograd VJP of the torch reference (tests/fieldmu_ref.py) and, by duality, against the forward-mode tangent
kernel; the module path of PDEModel.solve against the in-kernel closure; the gradient of mse_backward against the CPU
autograd reference and central differences of PDEModel.mse, its independence of the chunking and its determinism; and
train(method="mse") of a PeriodicCNN end to end."""
import numpy as np
import pytest
import torch

import pde_opt_amd as P
from oracle import np_oracle as O
from pde_opt_amd import _lib as L
from pde_opt_amd import fieldmu
from pde_opt_amd.engine import HipEngine
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg
import fieldmu_ref as R
import sens_ref as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _logit(c):
    return np.log(c / (1.0 - c))


def _domain(shape, box=R.BOX):
    return P.Domain(tuple(shape), box, "dimensionless")


def _mu_h(u):
    return O.chem_potential_legendre(R.MU_TRUE, u, _logit)


def _engine(shape, B, dtype, mu=None):
    """an engine on a torch stream, configured for B trajectories of the grid (mu: the closure the tangent kernel reads)"""
    stream = torch.cuda.Stream(DEV)
    eng = HipEngine(0, stream=stream.cuda_stream)
    eq = P.CahnHilliard2DPeriodic(_domain(shape), R.KAPPA, mu if mu is not None else 0.0, DiffLeg(np.array(R.D_COEF)))
    eng.configure(dtype=dtype, batch=B, **eq._engine_problem())
    return eng, stream, eq


def _dev(a, stream):
    with torch.cuda.stream(stream):
        return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-11), (np.float32, 1e-4)])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", list(R.GRIDS))
def test_rhs_matches_the_numpy_oracle(shape, B, dtype, tol):
    """the gates of tests/test_gpu_sens.py::test_tangent_rhs_matches_numpy_reference for the base slope"""
    shape = R.GRIDS[shape]
    hx, hy = R.spacing(shape)
    u = R.rough_state(shape, B, 1, dtype)
    muh = _mu_h(u.astype(np.float64)).astype(dtype)
    eng, stream, _ = _engine(shape, B, dtype)
    eng.set_state(u)
    mu_d, out = _dev(muh, stream), _dev(np.zeros_like(u), stream)
    eng.fieldmu_rhs(mu_d.data_ptr(), out.data_ptr())
    eng.sync()
    got = out.cpu().numpy()
    for b in range(B):
        want = O.ch_rhs_fd(u[b].astype(np.float64), hx, hy, R.KAPPA, lambda c: muh[b].astype(np.float64),
                           lambda c: O.diffusion_legendre(R.D_COEF, c))
        rel = np.linalg.norm(got[b].astype(np.float64) - want) / np.linalg.norm(want)
        print(shape, B, np.dtype(dtype).name, "rhs rel", rel)
        assert rel <= max(tol, 1e-12)


def _adjoint_outputs(shape, B, dtype):
    """(g_u, g_mu) of pdeopt_fieldmu_adjoint_step with S = I and dt = 1 (lambda_f = lambda), and the inputs"""
    u, muh, lam = R.vjp_inputs(shape, B, dtype)
    eng, stream, _ = _engine(shape, B, dtype)
    u_d, mu_d, lam_d, g_d = (_dev(a, stream) for a in (u, muh, lam, np.zeros_like(u)))
    eng.fieldmu_adjoint_step(L.INT_EULER, 1.0, u_d.data_ptr(), mu_d.data_ptr(), lam_d.data_ptr(), g_d.data_ptr())
    eng.sync()
    return (lam_d.cpu().numpy().astype(np.float64) - lam.astype(np.float64), g_d.cpu().numpy().astype(np.float64)), (u, muh, lam)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", list(R.GRIDS))
def test_adjoint_step_matches_the_autograd_vjp(shape, B, dtype):
    """g_u and g_mu per entry, relative to the field maximum.  fp64: 1e-12.  fp32: 10 x the reference's own fp32-vs-fp64
    distance on the same inputs (`python tests/fieldmu_ref.py`: 0.9e-7 .. 1.8e-7 over the grids and batch sizes), which
    covers another summation order, not another formula.  (g_u is lambda_after - lambda_before: exact to an ulp of
    lambda_after, whose size g_u dominates.)"""
    shape = R.GRIDS[shape]
    hx, hy = R.spacing(shape)
    got, (u, muh, lam) = _adjoint_outputs(shape, B, dtype)
    t = lambda a: torch.as_tensor(a.astype(np.float64))
    want = R.vjp_rhs(t(u), t(muh), t(lam), hx, hy, R.KAPPA, R.diffusion_legendre(R.D_COEF))
    gate = 1e-12 if dtype == np.float64 else 10 * R.fp32_vjp_distance(shape, B)
    for name, g, w in zip(("g_u", "g_mu"), got, want):
        err = float(np.max(np.abs(g - w.numpy())) / np.max(np.abs(w.numpy())))
        print(shape, B, np.dtype(dtype).name, name, "err", err, "gate", gate)
        assert err <= gate, name


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", list(R.GRIDS))
def test_adjoint_is_dual_to_the_tangent_kernel(shape, B):
    """<lambda, tangent slope of pdeopt_sens_rhs> = <g_u + mu_h' g_mu, du> + <g_mu, dmu_h/dp> for the pointwise Legendre
    mu, within the fp64 rounding of the three sums (the bound form of tests/test_gpu_optimize.py's contraction check)"""
    shape = R.GRIDS[shape]
    (g_u, g_mu), (u, muh, lam) = _adjoint_outputs(shape, B, np.float64)
    params = [(S.MU_ROLE, 1), (S.MU_ROLE, 2)]
    du = 0.05 * np.random.default_rng(33).standard_normal((len(params) * B,) + shape)
    eng = HipEngine()
    eq = P.CahnHilliard2DPeriodic(_domain(shape), R.KAPPA, ChemLeg(np.array(R.MU_TRUE), _logit), DiffLeg(np.array(R.D_COEF)))
    eng.configure(dtype=np.float64, batch=(1 + len(params)) * B, **eq._engine_problem())
    eng.sens_configure(B, params)
    eng.set_state(np.concatenate([u, du]))
    slopes = eng.sens_rhs()
    ut = torch.as_tensor(u).requires_grad_(True)
    mod = R.PointwiseLegendreMu(R.MU_TRUE)
    (mu1,) = torch.autograd.grad(mod(ut).sum(), ut)
    cells = u[0].size
    for j, (_, k) in enumerate(params):
        basis = np.polynomial.legendre.legval(2 * u - 1, np.eye(k + 1)[k])  # dmu_h/dp_k = P_k(2u - 1)
        for b in range(B):
            d = du[j * B + b]
            lhs = lam[b] * slopes[B + j * B + b]
            rhs1 = (g_u[b] + mu1[b].numpy() * g_mu[b]) * d
            rhs2 = g_mu[b] * basis[b]
            bound = cells * 2.0 ** -53 * (np.sum(np.abs(lhs)) + np.sum(np.abs(rhs1)) + np.sum(np.abs(rhs2)))
            gap = abs(np.sum(lhs) - np.sum(rhs1) - np.sum(rhs2))
            print(shape, B, j, b, "duality gap", gap, "bound", bound)
            assert gap <= bound, (j, b)


def _pointwise_model(shape, solver=P.SemiImplicitFourierSpectral, box=R.BOX):
    return P.PDEModel(P.CahnHilliard2DPeriodic, _domain(shape, box), solver)


@pytest.mark.parametrize("shape", ["16x32", "33x47"])
def test_solve_with_the_pointwise_module_matches_the_closure(shape):
    """200 IMEX substeps (rocFFT on both grids).  torch evaluates mu_h, so the match is not bitwise: gated at 10 x the
    distance between the CPU reference with the torch-evaluated mu_h and np_oracle (`python tests/fieldmu_ref.py`:
    1.6e-17 at 16 x 32, 3.3e-17 at 33 x 47, relative L2 of the final state)."""
    shape = R.GRIDS[shape]
    model = _pointwise_model(shape)
    y0 = R.smooth_state(shape, 1, 3)[0]
    ts = np.array([0.0, 2e-4])
    D = DiffLeg(np.array(R.D_COEF))
    want = model.solve({"kappa": R.KAPPA, "mu": ChemLeg(np.array(R.MU_TRUE), _logit), "D": D}, y0, ts, {"A": 0.5})
    mod = R.PointwiseLegendreMu(R.MU_TRUE).to(DEV)
    got = model.solve({"kappa": R.KAPPA, "mu": mod, "D": D}, y0, ts, {"A": 0.5})
    assert got.shape == want.shape and got.dtype == want.dtype
    rel = float(np.linalg.norm(got[-1] - want[-1]) / np.linalg.norm(want[-1]))
    gate = 10 * R.solve_distance(shape)
    print(shape, "module vs closure", rel, "gate", gate)
    assert rel <= gate


def _grad_case(integrator):
    solver = P.SemiImplicitFourierSpectral if integrator == "imex" else P.Euler
    model = _pointwise_model(R.GRAD_SHAPE, solver)
    sp = {"A": 0.5} if integrator == "imex" else {}
    y0s, values = R.grad_problem()
    return model, sp, y0s, values


def _gpu_grad(model, sp, y0s, values, seed=7, hidden=(4,), chunk_bytes=None):
    m = R.seeded_cnn(hidden, seed).to(DEV)
    model.fieldmu_solver().chunk_bytes = chunk_bytes
    params = {"kappa": R.KAPPA, "mu": m, "D": DiffLeg(np.array(R.D_COEF))}
    loss = model.mse_backward(params, (y0s, values), sp, R.GRAD_TS, {}, 0.0)
    return loss, fieldmu.flatten_grads(m), m, params


@pytest.mark.parametrize("integrator", ["imex", "euler"])
def test_mse_gradient(integrator):
    """two trajectories, 40 substeps, the middle save inside a substep, PeriodicCNN(1, (4,), 1): against the CPU autograd
    reference (1e-10 of max |grad|) and against central differences of PDEModel.mse on 5 seeded parameters (1e-6): the
    project's gates for forward-mode gradients"""
    model, sp, y0s, values = _grad_case(integrator)
    loss, grad, m, params = _gpu_grad(model, sp, y0s, values)
    hx, hy = R.spacing(R.GRAD_SHAPE)
    ref = R.seeded_cnn((4,), 7)
    J, want = R.mse_and_grad(ref, y0s, values, R.GRAD_TS, 1e-6, hx, hy, R.KAPPA, R.diffusion_legendre(R.D_COEF), integrator, 0.5,
                             R.symbol_of(R.GRAD_SHAPE))
    scale = np.max(np.abs(want))
    print(integrator, "loss", loss, "ref", J, "grad err", np.max(np.abs(grad - want)) / scale)
    assert abs(loss - J) <= 1e-12 * J
    assert abs(loss - model.mse(params, (y0s, values), sp, R.GRAD_TS, {}, 0.0)) <= 1e-12 * J
    assert np.max(np.abs(grad - want)) <= 1e-10 * scale
    p = fieldmu.flatten_params(m)
    eps = 1e-4
    for j in np.random.default_rng(0).choice(len(p), 5, replace=False):
        f = []
        for sgn in (1, -1):
            q = p.copy()
            q[j] += sgn * eps
            fieldmu.unflatten_params(m, q)
            f.append(model.mse(params, (y0s, values), sp, R.GRAD_TS, {}, 0.0))
        cd = (f[0] - f[1]) / (2 * eps)
        print(integrator, "parameter", j, "grad", grad[j], "cd", cd, (grad[j] - cd) / scale)
        assert abs(grad[j] - cd) <= 1e-6 * scale, j


def test_gradient_bits_do_not_depend_on_chunking_or_on_the_run():
    model, sp, y0s, values = _grad_case("imex")
    whole = _gpu_grad(model, sp, y0s, values)
    assert model.fieldmu_solver().last_chunks == 1
    again = _gpu_grad(model, sp, y0s, values)
    assert whole[0] == again[0] and whole[1].tobytes() == again[1].tobytes()
    # 5 states per chunk: the segments between the save points (17.5 and 22.5 substeps) take >= 3 chunks each
    chunked = _gpu_grad(model, sp, y0s, values, chunk_bytes=5 * y0s.nbytes)
    assert model.fieldmu_solver().last_chunks == 8
    assert whole[0] == chunked[0] and whole[1].tobytes() == chunked[1].tobytes()


def test_fp32_and_a_single_field_module():
    """fp32 end of the path, and a module written for one (nx, ny) field through the adapter: the gradient against the
    fp64 one within fp32 rounding of a 40-substep solve (1e-3 of max |grad|)"""

    class OneField(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, x):
            assert x.dim() == 2
            return self.inner(x[None, None])[0, 0]

    model, sp, y0s, values = _grad_case("imex")
    _, want, _, _ = _gpu_grad(model, sp, y0s, values)
    m = OneField(R.seeded_cnn((4,), 7, dtype=torch.float32)).to(DEV)
    params = {"kappa": R.KAPPA, "mu": m, "D": DiffLeg(np.array(R.D_COEF))}
    ys = model.solve(params, y0s.astype(np.float32), R.GRAD_TS, sp)
    assert ys.dtype == np.float32 and ys.shape == (3,) + y0s.shape
    model.mse_backward(params, (y0s.astype(np.float32), values.astype(np.float32)), sp, R.GRAD_TS, {}, 0.0)
    got = fieldmu.flatten_grads(m)
    print("fp32 gradient vs fp64", np.max(np.abs(got - want)) / np.max(np.abs(want)))
    assert np.max(np.abs(got - want)) <= 1e-3 * np.max(np.abs(want))


def test_caller_stream_is_ordered_against_the_solver():
    """the documented loop `mse_backward(...); opt.step()` with the caller on the default stream and on a stream of its
    own, against the same loop with a device synchronise after every call: identical losses, bit for bit.  (The solver
    waits for the caller's stream on entry and the caller's stream for the solver on exit; a missing wait is a race
    the other tests cannot see, this one only when the race is lost.)"""
    model, sp, y0s, values = _grad_case("imex")
    fm = model.fieldmu_solver()
    fm.chunk_bytes = None

    def loop(caller, sync):
        with torch.cuda.stream(caller):
            m = R.seeded_cnn((4,), 7).to(DEV)
            params = {"kappa": R.KAPPA, "mu": m, "D": DiffLeg(np.array(R.D_COEF))}
            opt = torch.optim.Adam(m.parameters(), lr=1e-2)
            out = []
            for _ in range(4):
                out.append(model.mse_backward(params, (y0s, values), sp, R.GRAD_TS, {}, 0.0))
                if sync:
                    torch.cuda.synchronize()
                opt.step()
                if sync:
                    torch.cuda.synchronize()
            return out, fieldmu.flatten_params(m)

    want, p_want = loop(torch.cuda.default_stream(DEV), True)
    assert want[-1] < want[0]
    for caller in (torch.cuda.default_stream(DEV), torch.cuda.Stream(DEV), fm.stream):
        got, p = loop(caller, False)
        assert got == want and p.tobytes() == p_want.tobytes()


def test_adjoint_step_refuses_overlapping_fields():
    shape = (8, 8)
    eng, stream, _ = _engine(shape, 2, np.float64)
    big = _dev(np.zeros((5, 2) + shape), stream)
    u, mu, lam, g = (big[k] for k in range(4))
    eng.fieldmu_adjoint_step(L.INT_EULER, 1.0, u.data_ptr(), mu.data_ptr(), lam.data_ptr(), g.data_ptr())
    half = big.reshape(10, 8, 8)
    for bad in ((u, mu, lam, lam), (u, mu, lam, half[5:7]), (u, mu, half[1:3], g), (u, mu, half[3:5], g)):  # equal, or one environment shared
        with pytest.raises(ValueError, match="overlap"):
            eng.fieldmu_adjoint_step(L.INT_EULER, 1.0, *(t.data_ptr() for t in bad))
    with pytest.raises(ValueError, match="field pointer"):
        eng.fieldmu_adjoint_step(L.INT_EULER, 1.0, u.data_ptr(), 0, lam.data_ptr(), g.data_ptr())
    with pytest.raises(ValueError, match="field pointer"):
        eng.fieldmu_adjoint_step(L.INT_EULER, 1.0, u.data_ptr(), mu.data_ptr() + 4, lam.data_ptr(), g.data_ptr())
    eng.sync()


# The same 30 BFGS steps on the CPU through the autograd reference (fieldmu_ref.train_reference, re-derived by
# tests/test_fieldmu_cpu.py) take the mse from 8.845e-06 to 3.060e-07: more than 10 x, so the gate below is not vacuous
CPU_TRAIN = R.CPU_TRAIN


def test_train_a_periodic_cnn_end_to_end():
    assert CPU_TRAIN[1] <= CPU_TRAIN[0] / 10
    model = _pointwise_model(R.GRAD_SHAPE, box=R.E2E_BOX)
    y0s, values = R.e2e_problem()
    ts = R.GRAD_TS
    data = {"ys": [y0s[0], values[0, 0], values[0, 1], y0s[1], values[1, 0], values[1, 1]], "ts": list(ts) + list(ts)}
    m = R.seeded_cnn(R.E2E_HIDDEN, R.E2E_SEED).to(DEV)
    other = {"kappa": R.KAPPA, "D": DiffLeg(np.array(R.D_COEF))}
    res = model.train(data, [[0, 1, 2], [3, 4, 5]], {"mu": m}, other, {"A": 0.5}, {}, 0.0, method="mse", max_steps=R.E2E_STEPS)
    hist = model.last_train_history
    final = model.mse(res, (y0s, values), {"A": 0.5}, ts, {}, 0.0)
    print(f"train: mse {hist[0]:.6e} -> {final:.6e} in {len(hist) - 1} BFGS steps")
    assert res["mu"] is m and res["kappa"] == R.KAPPA
    assert abs(hist[0] - CPU_TRAIN[0]) <= 1e-3 * CPU_TRAIN[0]
    assert final <= 10 * CPU_TRAIN[1]
