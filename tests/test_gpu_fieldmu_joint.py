"""Training the mobility D together with a torch.nn.Module as mu on the MI355X: the coefficient gradient of one adjoint
step against autograd of the torch reference (tests/fieldmu_joint_ref.py), the D gradient of mse_backward against the CPU
reference, central differences of PDEModel.mse and the forward-mode tangents, its determinism, the regularisation share,
and train(method="mse") over {"mu", "D"} end to end."""
import numpy as np
import pytest
import torch

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd import fieldmu, fit
from pde_opt_amd.engine import HipEngine
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg
import fieldmu_joint_ref as J
import fieldmu_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _logit(c):
    return np.log(c / (1.0 - c))


def _domain(shape, box=R.BOX):
    return P.Domain(tuple(shape), box, "dimensionless")


def _dev(a, stream):
    with torch.cuda.stream(stream):
        return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


# ---- one adjoint step ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", J.N_COEFS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", J.STEP_GRIDS)
def test_adjoint_step_coefficient_gradient_matches_autograd(shape, B, n, dtype):
    """S = I, dt = 1: the sums read back against d <lam, ch_rhs(u, mu_h; D(coef))> / d coef, relative to max |grad|.
    fp64: 1e-12.  fp32: 10 x the reference's own fp32-vs-fp64 distance on the same inputs (`python
    tests/fieldmu_joint_ref.py`: 0.5e-8 .. 1.9e-7 over the grids, batch sizes and coefficient counts), which covers
    another summation order, not another formula.  lam and g_mu are those of pdeopt_fieldmu_adjoint_step, bit for bit;
    a second step doubles the sums and a read with reset empties them."""
    shape = R.GRIDS[shape]
    hx, hy = R.spacing(shape)
    coef = J.d_coefs(n)
    u, muh, lam = R.vjp_inputs(shape, B, dtype)
    stream = torch.cuda.Stream(DEV)
    eng = HipEngine(0, stream=stream.cuda_stream)
    eq = P.CahnHilliard2DPeriodic(_domain(shape), R.KAPPA, 0.0, DiffLeg(coef))
    eng.configure(dtype=dtype, batch=B, **eq._engine_problem())
    out = []
    for step in (eng.fieldmu_adjoint_step, eng.fieldmu_adjoint_step_coef, eng.fieldmu_adjoint_step_coef):
        u_d, mu_d, lam_d, g_d = (_dev(a, stream) for a in (u, muh, lam, np.zeros_like(u)))
        step(L.INT_EULER, 1.0, u_d.data_ptr(), mu_d.data_ptr(), lam_d.data_ptr(), g_d.data_ptr())
        eng.sync()
        out.append((lam_d.cpu().numpy(), g_d.cpu().numpy()))
    twice = eng.fieldmu_coef_grad_read(n, reset=False)
    again = eng.fieldmu_coef_grad_read(n, reset=True)
    empty = eng.fieldmu_coef_grad_read(n)
    for k in (1, 2):
        assert out[k][0].tobytes() == out[0][0].tobytes() and out[k][1].tobytes() == out[0][1].tobytes()
    assert twice.tobytes() == again.tobytes() and not empty.any()
    got = 0.5 * twice  # the same step twice: each slot holds s + s, exactly
    want = J.coef_vjp(u, muh, lam, coef, hx, hy)
    gate = 1e-12 if dtype == np.float64 else 10 * J.fp32_coef_distance(shape, B, n)
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print(shape, B, n, np.dtype(dtype).name, "coefficient gradient err", err, "gate", gate)
    assert err <= gate


def test_coefficient_gradient_is_zeroed_by_configure_and_refuses_what_it_cannot_name():
    shape = R.GRIDS["8x8"]
    u, muh, lam = R.vjp_inputs(shape, 2, np.float64)
    stream = torch.cuda.Stream(DEV)
    eng = HipEngine(0, stream=stream.cuda_stream)
    eq = P.CahnHilliard2DPeriodic(_domain(shape), R.KAPPA, 0.0, DiffLeg(J.d_coefs(2)))
    eng.configure(dtype=np.float64, batch=2, **eq._engine_problem())
    u_d, mu_d, lam_d, g_d = (_dev(a, stream) for a in (u, muh, lam, np.zeros_like(u)))
    eng.fieldmu_adjoint_step_coef(L.INT_EULER, 1.0, u_d.data_ptr(), mu_d.data_ptr(), lam_d.data_ptr(), g_d.data_ptr())
    assert eng.fieldmu_coef_grad_read(2, reset=False).any()
    with pytest.raises(ValueError, match="2 coefficients"):
        eng.fieldmu_coef_grad_read(3)
    eng.configure(dtype=np.float64, batch=2, **eq._engine_problem())
    assert not eng.fieldmu_coef_grad_read(2).any()
    with pytest.raises(ValueError, match="overlap"):
        eng.fieldmu_adjoint_step_coef(L.INT_EULER, 1.0, u_d.data_ptr(), mu_d.data_ptr(), lam_d.data_ptr(), lam_d.data_ptr())
    eng.sync()


# ---- the whole solve ----------------------------------------------------------------------------------------------------


def _model(integrator="imex", box=R.BOX):
    solver = P.SemiImplicitFourierSpectral if integrator == "imex" else P.Euler
    return P.PDEModel(P.CahnHilliard2DPeriodic, _domain(R.GRAD_SHAPE, box), solver), ({"A": 0.5} if integrator == "imex" else {})


_PROBLEM = []


def _problem():
    if not _PROBLEM:
        _PROBLEM.append(R.grad_problem())
    return _PROBLEM[0]


def _joint_grad(model, sp, native=False, joint=True, chunk_bytes=None, coef=R.D_COEF, weights=None, lambda_reg=0.0, module=None):
    """(loss, flat module gradient, D gradient or None, module, params) of mse_backward on grad_problem()"""
    y0s, values = _problem()
    m = module if module is not None else R.seeded_cnn((4,), 7).to(DEV)
    fm = model.fieldmu_solver()
    fm.chunk_bytes, fm.native_cnn = chunk_bytes, native
    params = {"kappa": R.KAPPA, "mu": m, "D": DiffLeg(np.array(coef))}
    grads = {} if joint else None
    loss = model.mse_backward(params, (y0s, values), sp, R.GRAD_TS, weights or {}, lambda_reg, closure_grads=grads)
    return loss, fieldmu.flatten_grads(m), (grads["D"] if joint else None), m, params


@pytest.mark.parametrize("native", [False, True], ids=["autograd", "native_cnn"])
@pytest.mark.parametrize("integrator", ["imex", "euler"])
def test_D_gradient_of_the_whole_solve(integrator, native):
    """two trajectories, 40 substeps, the middle save inside a substep, PeriodicCNN(1, (4,), 1): the D gradient against the
    CPU autograd reference (1e-10 of its maximum) and against central differences of PDEModel.mse over each coefficient
    (1e-6), the gates of test_mse_gradient; the module's gradient is the one mse_backward gives without closure_grads,
    bit for bit"""
    model, sp = _model(integrator)
    y0s, values = _problem()
    loss, g_mu, g_D, m, params = _joint_grad(model, sp, native)
    plain = _joint_grad(model, sp, native, joint=False)
    assert loss == plain[0] and g_mu.tobytes() == plain[1].tobytes()
    assert g_D.dtype == np.float64 and g_D.shape == (2,)
    hx, hy = R.spacing(R.GRAD_SHAPE)
    Jref, _, want = J.mse_and_grads(R.seeded_cnn((4,), 7), R.D_COEF, y0s, values, R.GRAD_TS, 1e-6, hx, hy, integrator,
                                    R.symbol_of(R.GRAD_SHAPE))
    scale = np.max(np.abs(want))
    print(integrator, native, "loss", loss, "ref", Jref, "D grad", g_D, "ref", want, "err", np.max(np.abs(g_D - want)) / scale)
    assert abs(loss - Jref) <= 1e-12 * Jref
    assert np.max(np.abs(g_D - want)) <= 1e-10 * scale
    eps = 1e-4
    for k in range(2):
        f = []
        for sgn in (1, -1):
            c = np.array(R.D_COEF)
            c[k] += sgn * eps
            f.append(model.mse({**params, "D": DiffLeg(c)}, (y0s, values), sp, R.GRAD_TS, {}, 0.0))
        cd = (f[0] - f[1]) / (2 * eps)
        print(integrator, native, "coefficient", k, "grad", g_D[k], "cd", cd, (g_D[k] - cd) / scale)
        assert abs(g_D[k] - cd) <= 1e-6 * scale, k


# `python tests/fieldmu_joint_ref.py`: the two CPU references (autograd of the torch solve, numpy tangents of tests/sens_ref.py)
# differ by 2.243e-14 of max |grad| on this problem
CPU_FORWARD_VS_REVERSE = 2.243e-14


def test_reverse_mode_D_gradient_equals_forward_mode():
    """mu as fieldmu_ref.PointwiseLegendreMu through the module path, and the same function as a
    ChemicalPotentialLegendrePolynomials closure through fit.sensitivity_solve over the D coefficients: the reverse-mode D
    gradient against -2 / M rdp, gated at 10 x the distance between the two CPU references (2.243e-14 of max |grad|).  The
    one check whose reference side does not go through torch."""
    model, sp = _model("imex")
    y0s, values = _problem()
    m = R.PointwiseLegendreMu(J.FWD_MU).to(DEV)
    _, _, rev, _, _ = _joint_grad(model, sp, coef=J.FWD_D, module=m)
    D = DiffLeg(np.array(J.FWD_D))
    eq = P.CahnHilliard2DPeriodic(_domain(R.GRAD_SHAPE), R.KAPPA, ChemLeg(np.array(J.FWD_MU), _logit), D)
    solver = P.SemiImplicitFourierSpectral(**P.utils.prepare_solver_params(P.SemiImplicitFourierSpectral, sp, eq))
    pmap = fit.ParamMap.of({"D": D}, P.CahnHilliard2DPeriodic)
    s, _ = fit.sensitivity_solve(HipEngine(), eq, solver, y0s, R.GRAD_TS, pmap.sens_params(),
                                 frames=np.ascontiguousarray(np.swapaxes(values, 0, 1)))
    _, rdp, _ = fit.unpack_sums(s, 2)
    fwd = -2.0 / values.size * rdp
    err = float(np.max(np.abs(rev - fwd)) / np.max(np.abs(fwd)))
    print("reverse", rev, "forward", fwd, "err", err, "gate", 10 * CPU_FORWARD_VS_REVERSE)
    assert err <= 10 * CPU_FORWARD_VS_REVERSE


def test_bits_do_not_depend_on_the_run_the_chunking_or_an_abandoned_sweep():
    model, sp = _model("imex")
    y0s, _ = _problem()
    whole = _joint_grad(model, sp)
    assert model.fieldmu_solver().last_chunks == 1
    again = _joint_grad(model, sp)
    chunked = _joint_grad(model, sp, chunk_bytes=5 * y0s.nbytes)
    assert model.fieldmu_solver().last_chunks == 8
    for other in (again, chunked):
        assert whole[0] == other[0] and whole[1].tobytes() == other[1].tobytes() and whole[2].tobytes() == other[2].tobytes()

    class Fails(torch.nn.Module):
        """the network, until its forward has been called `left` times"""

        def __init__(self, inner, left):
            super().__init__()
            self.inner, self.left = inner, left

        def forward(self, x):
            self.left -= 1
            if self.left < 0:
                raise RuntimeError("abandoned")
            return self.inner(x)

    # the probe, 40 forward substeps, 39 of the chunk's re-run, then 20 of the 40 backward substeps
    with pytest.raises(RuntimeError, match="abandoned"):
        _joint_grad(model, sp, module=Fails(R.seeded_cnn((4,), 7), 1 + 40 + 39 + 20).to(DEV))
    assert model.fieldmu_solver()._coef_pending
    after = _joint_grad(model, sp)
    fresh = _joint_grad(_model("imex")[0], sp)
    for other in (after, fresh):
        assert whole[0] == other[0] and whole[1].tobytes() == other[1].tobytes() and whole[2].tobytes() == other[2].tobytes()


def test_regularisation_share():
    model, sp = _model("imex")
    lam, w_D = 0.1, np.array([0.0, 2.0])
    plain = _joint_grad(model, sp)
    reg = _joint_grad(model, sp, weights={"mu": 1.0, "D": [0.0, 2.0]}, lambda_reg=lam)
    p_mu, p_D = fieldmu.flatten_params(plain[3]), np.array(R.D_COEF)
    assert reg[0] == plain[0] + float(lam * np.sum(p_mu * p_mu)) + float(lam * np.sum(w_D * p_D * p_D))
    np.testing.assert_array_equal(reg[2], plain[2] + 2.0 * lam * w_D * p_D)
    np.testing.assert_allclose(reg[1], plain[1] + 2.0 * lam * p_mu, rtol=0, atol=1e-15 * np.max(np.abs(reg[1])))
    y0s, values = _problem()
    assert abs(model.mse(reg[4], (y0s, values), sp, R.GRAD_TS, {"mu": 1.0, "D": w_D}, lam) - reg[0]) <= 1e-12 * reg[0]


def test_what_the_joint_gradient_refuses():
    model, sp = _model("imex")
    y0s, values = _problem()
    m = R.seeded_cnn((4,), 7).to(DEV)
    with pytest.raises(NotImplementedError, match="DiffusionLegendrePolynomials"):
        model.mse_backward({"kappa": R.KAPPA, "mu": m, "D": lambda c: c * (1 - c)}, (y0s, values), sp, R.GRAD_TS, {}, 0.0, closure_grads={})


def test_train_mu_and_D_end_to_end():
    """fieldmu_ref's 16 x 32 end-to-end problem with a PeriodicCNN(1, (4,), 1) and a two-coefficient D started at (0, 0),
    8 BFGS steps.  The same BFGS on the CPU through the autograd reference (fieldmu_joint_ref.train_reference) takes the
    mse from 7.346666e-05 to 4.373277e-06; the GPU run is gated at 10 x that final value, the factor of
    test_train_a_periodic_cnn_end_to_end."""
    assert J.CPU_TRAIN[1] <= J.CPU_TRAIN[0] / 10
    model, sp = _model("imex", box=R.E2E_BOX)
    model.fieldmu_solver().native_cnn = True
    y0s, values = R.e2e_problem()
    ts = R.GRAD_TS
    data = {"ys": [y0s[0], values[0, 0], values[0, 1], y0s[1], values[1, 0], values[1, 1]], "ts": list(ts) + list(ts)}
    m = R.seeded_cnn(J.E2E_HIDDEN, J.E2E_SEED).to(DEV)
    res = model.train(data, [[0, 1, 2], [3, 4, 5]], {"mu": m, "D": DiffLeg(np.array(J.E2E_D_START))}, {"kappa": R.KAPPA}, sp, {}, 0.0,
                      method="mse", max_steps=J.E2E_STEPS)
    hist = model.last_train_history
    final = model.mse(res, (y0s, values), sp, ts, {}, 0.0)
    print(f"train: mse {hist[0]:.6e} -> {final:.6e} in {len(hist) - 1} BFGS steps, D = {res['D'].expansion.params}")
    assert res["mu"] is m and isinstance(res["D"], DiffLeg) and res["kappa"] == R.KAPPA
    assert all(b <= a for a, b in zip(hist, hist[1:]))
    assert abs(hist[0] - J.CPU_TRAIN[0]) <= 1e-3 * J.CPU_TRAIN[0]
    assert final <= 10 * J.CPU_TRAIN[1]
