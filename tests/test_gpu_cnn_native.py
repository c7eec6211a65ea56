"""The library's own PeriodicCNN (csrc/cnn.hip) on the MI355X against the same module evaluated by torch in fp64 on the
device and its autograd.grad: values and vector-Jacobian products in fp64 and fp32, determinism of the gradient sums, the
refusals, and mse_backward / solve with ``FieldMuSolver.native_cnn`` against the torch path of the same solver."""
import functools

import numpy as np
import pytest
import torch

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd import fieldmu
from pde_opt_amd.engine import HipEngine, NativeCNN
from pde_opt_amd.numerics.functions import cnn as C
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg
import fieldmu_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F = torch.nn.functional

GRIDS = [(4, 4), (16, 16), (20, 12), (33, 17)]  # every neighbour wraps; whole tiles; partial tiles; odd and ragged
BATCHES = [1, 3]
HIDDEN = [(16,), (8, 24), (32, 64, 64), (64, 64, 64, 64)]  # (8, 24): the padding path; (32, 64, 64): the notebook's
ACTS = {"gelu": F.gelu, "gelu_tanh": functools.partial(F.gelu, approximate="tanh"), "tanh": torch.tanh}
CASES = [(g, B, h, "gelu") for g in GRIDS for B in BATCHES for h in HIDDEN] + [((20, 12), 3, (8, 24), a) for a in ("gelu_tanh", "tanh")]
IDS = [f"{g[0]}x{g[1]}-B{B}-{'_'.join(map(str, h))}-{a}" for g, B, h, a in CASES]


def _module(hidden, act):
    """PeriodicCNN(1, hidden) in fp64 with seeded parameters of unit gain: weights N(0, 1 / (9 C_in)), biases 0.1 N(0, 1)"""
    m = C.PeriodicCNN(1, hidden, act=ACTS[act]).double()
    rng = np.random.default_rng(11)
    parts = [rng.standard_normal(q.numel()) * (0.1 if q.dim() == 1 else (9 * q.shape[1]) ** -0.5) for q in m.parameters()]
    fieldmu.unflatten_params(m, np.concatenate(parts))
    return m.to(DEV)


def _vjp(m, u, g):
    """(mu, N'(u)^T g, flat parameter gradient of <g, N(u)>) by torch, in the dtype of the module"""
    u = u.clone().requires_grad_(True)
    mu = m(u[:, None])[:, 0]
    grads = torch.autograd.grad((mu * g).sum(), [u] + list(m.parameters()))
    return mu.detach(), grads[0], torch.cat([q.reshape(-1) for q in grads[1:]])


@functools.lru_cache(maxsize=None)
def _reference(grid, B, hidden, act):
    """inputs (representable in fp32) and what torch gives for them in fp64 and in fp32; computed once per case"""
    rng = np.random.default_rng(5)
    u = (0.5 + 0.2 * rng.standard_normal((B,) + grid)).astype(np.float32).astype(np.float64)
    g = rng.standard_normal((B,) + grid).astype(np.float32).astype(np.float64)
    lam0 = (0.25 * rng.standard_normal((B,) + grid)).astype(np.float32).astype(np.float64)
    m = _module(hidden, act)
    ud, gd = torch.as_tensor(u).to(DEV), torch.as_tensor(g).to(DEV)
    ref = {"u": u, "g": g, "lam0": lam0, "params": fieldmu.flatten_params(m), "spec": C.native_spec(m)}
    prev = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        ref["f64"] = tuple(t.cpu().numpy() for t in _vjp(m, ud, gd))
        ref["f32"] = tuple(t.double().cpu().numpy() for t in _vjp(m.float(), ud.float(), gd.float()))
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = prev
    return ref


_engines = {}


def _engine(grid, B, dtype):
    """one engine per (grid, batch, dtype) on a stream of its own, configured as the field-mu path configures it"""
    key = (grid, B, np.dtype(dtype).name)
    if key not in _engines:
        stream = torch.cuda.Stream(DEV)
        eng = HipEngine(0, stream=stream.cuda_stream)
        eq = P.CahnHilliard2DPeriodic(P.Domain(grid, R.BOX, "dimensionless"), R.KAPPA, 0.0, DiffLeg(np.array(R.D_COEF)))
        eng.configure(dtype=dtype, batch=B, **eq._engine_problem())
        _engines[key] = (eng, stream)
    return _engines[key]


def _native(grid, B, hidden, act, dtype):
    """(mu, lam after one vjp from lam0, parameter gradient) of the library in ``dtype``, as fp64 arrays, and the handle"""
    ref = _reference(grid, B, hidden, act)
    eng, stream = _engine(grid, B, dtype)
    channels, name = ref["spec"]
    net = eng.cnn(channels, C.NATIVE_ACTIVATIONS.index(name))
    net.set_params(ref["params"])
    with torch.cuda.stream(stream):
        u, g, lam = (torch.as_tensor(ref[k].astype(dtype)).to(DEV) for k in ("u", "g", "lam0"))
        mu = torch.empty_like(u)
        net.forward(u.data_ptr(), mu.data_ptr())
        net.vjp(u.data_ptr(), g.data_ptr(), lam.data_ptr())
        grad = net.grad_read(reset=True)
        out = mu.double().cpu().numpy(), lam.double().cpu().numpy(), grad
    return out, net, (u, g, stream)


def _err(a, b):
    return float(np.max(np.abs(a - b)))


@pytest.mark.parametrize("grid, B, hidden, act", CASES, ids=IDS)
def test_fp64_matches_torch(grid, B, hidden, act):
    """values to 1e-12 of max |mu| (the value gate of test_gpu_fieldmu.py), the lam increment and the parameter gradient
    to 1e-10 of their maxima (the gate of test_mse_gradient)"""
    ref = _reference(grid, B, hidden, act)
    (mu, lam, grad), net, _ = _native(grid, B, hidden, act, np.float64)
    net.close()
    want_mu, want_gu, want_gp = ref["f64"]
    e = (_err(mu, want_mu) / np.max(np.abs(want_mu)), _err(lam, ref["lam0"] + want_gu) / np.max(np.abs(want_gu)),
         _err(grad, want_gp) / np.max(np.abs(want_gp)))
    print(grid, B, hidden, act, "fp64 rel err: mu %.3g, lam %.3g, grad %.3g" % e)
    assert e[0] <= 1e-12
    assert e[1] <= 1e-10
    assert e[2] <= 1e-10


@pytest.mark.parametrize("grid, B, hidden, act", CASES, ids=IDS)
def test_fp32_is_as_close_to_fp64_as_torch_fp32(grid, B, hidden, act):
    """the native fp32 error against torch fp64 is at most 4 x that of torch's own fp32 evaluation of the same inputs
    (another summation order over up to 576 terms per output, nothing else), with a floor of 1e-6 of the maximum"""
    ref = _reference(grid, B, hidden, act)
    (mu, lam, grad), net, _ = _native(grid, B, hidden, act, np.float32)
    net.close()
    lam0_32 = ref["lam0"].astype(np.float32)
    torch_lam = (lam0_32 + ref["f32"][1].astype(np.float32)).astype(np.float64)  # torch's own lam += u.grad in fp32
    got = (mu, lam, grad)
    theirs = (ref["f32"][0], torch_lam, ref["f32"][2])
    want = (ref["f64"][0], ref["lam0"] + ref["f64"][1], ref["f64"][2])
    scales = tuple(np.max(np.abs(ref["f64"][k])) for k in range(3))
    for name, a, t, w, s in zip(("mu", "lam", "grad"), got, theirs, want, scales):
        mine, torchs = _err(a, w) / s, _err(t, w) / s
        print(grid, B, hidden, act, name, "fp32 rel err: native %.3g, torch %.3g" % (mine, torchs))
        assert mine <= max(4 * torchs, 1e-6), name


@pytest.mark.parametrize("B", BATCHES)
def test_vjp_is_deterministic_and_accumulates_in_order(B):
    grid, hidden, act = (20, 12), (8, 24), "gelu"
    ref = _reference(grid, B, hidden, act)
    (_, lam1, g1), net, (u, g, stream) = _native(grid, B, hidden, act, np.float64)
    with torch.cuda.stream(stream):
        lam = torch.as_tensor(ref["lam0"]).to(DEV)
        net.vjp(u.data_ptr(), g.data_ptr(), lam.data_ptr())
        g2 = net.grad_read(reset=True)
        assert lam.cpu().numpy().tobytes() == lam1.tobytes() and g2.tobytes() == g1.tobytes()
        for _ in range(3):
            net.vjp(u.data_ptr(), g.data_ptr(), lam.data_ptr())
        g3 = net.grad_read(reset=True)
    assert g3.tobytes() == ((g1 + g1) + g1).tobytes()
    assert not net.grad_read().any()  # reset
    net.close()


def test_refusals():
    eng, stream = _engine((16, 16), 1, np.float64)
    net = eng.cnn((1, 16, 1), L.CNN_TANH)
    with torch.cuda.stream(stream):
        u, g = torch.zeros((1, 16, 16), dtype=torch.float64, device=DEV), torch.zeros((2, 16, 16), dtype=torch.float64, device=DEV)
        with pytest.raises(L.PdeoptError, match="set_params"):
            net.forward(u.data_ptr(), g.data_ptr())
        net.set_params(np.zeros(net.n_params))
        with pytest.raises(ValueError, match="overlap"):
            net.vjp(u.data_ptr(), g.data_ptr(), g.data_ptr())
        with pytest.raises(ValueError, match="overlap"):
            net.vjp(u.data_ptr(), g.data_ptr(), g[0, 8:].data_ptr())  # lam starts inside gmu
        with pytest.raises(ValueError, match="parameters"):
            net.set_params(np.zeros(net.n_params + 1))
    net.close()
    for channels, act in (((1, 65, 1), L.CNN_TANH), ((2, 16, 1), L.CNN_TANH), ((1, 16, 1), 3), ((1, 1), L.CNN_TANH)):
        with pytest.raises(ValueError):
            eng.cnn(channels, act)
    small, stream3 = _engine((3, 3), 1, np.float64)
    net = small.cnn((1, 16, 1), L.CNN_TANH)
    net.set_params(np.zeros(net.n_params))
    with torch.cuda.stream(stream3):
        u, mu = torch.zeros((1, 3, 3), dtype=torch.float64, device=DEV), torch.zeros((1, 3, 3), dtype=torch.float64, device=DEV)
        with pytest.raises(ValueError, match="4 x 4"):
            net.forward(u.data_ptr(), mu.data_ptr())
    net.close()


# ---- through FieldMuSolver -------------------------------------------------------------------------------------------


def _grad_case(integrator):
    solver = P.SemiImplicitFourierSpectral if integrator == "imex" else P.Euler
    model = P.PDEModel(P.CahnHilliard2DPeriodic, P.Domain(R.GRAD_SHAPE, R.BOX, "dimensionless"), solver)
    y0s, values = R.grad_problem()
    return model, ({"A": 0.5} if integrator == "imex" else {}), y0s, values


def _seeded(act=torch.tanh):
    m = C.PeriodicCNN(1, (16,), act=act).double()
    n = sum(q.numel() for q in m.parameters())
    fieldmu.unflatten_params(m, 0.3 * np.random.default_rng(7).standard_normal(n))
    return m.to(DEV)


def _mse_backward(model, sp, y0s, values, native, chunk_bytes=None):
    m = _seeded()
    fm = model.fieldmu_solver()
    fm.native_cnn, fm.chunk_bytes = native, chunk_bytes
    params = {"kappa": R.KAPPA, "mu": m, "D": DiffLeg(np.array(R.D_COEF))}
    try:
        loss = model.mse_backward(params, (y0s, values), sp, R.GRAD_TS, {}, 0.0)
    finally:
        fm.native_cnn, fm.chunk_bytes = False, None
    return loss, fieldmu.flatten_grads(m), params


@pytest.mark.parametrize("integrator", ["imex", "euler"])
def test_mse_backward_native_matches_the_torch_path(integrator):
    """the problem of test_gpu_fieldmu.py::test_mse_gradient with PeriodicCNN(1, (16,), act=tanh), fp64: loss to 1e-12 J,
    gradient to 1e-10 of its maximum, identical bits on a repeat and under chunking"""
    model, sp, y0s, values = _grad_case(integrator)
    made = NativeCNN.created
    J, want, _ = _mse_backward(model, sp, y0s, values, native=False)
    assert NativeCNN.created == made  # switch off: a supported module still runs in torch
    loss, grad, _ = _mse_backward(model, sp, y0s, values, native=True)
    assert NativeCNN.created == made + 1
    scale = np.max(np.abs(want))
    print(integrator, "loss", loss, "torch", J, "grad err", np.max(np.abs(grad - want)) / scale)
    assert abs(loss - J) <= 1e-12 * J
    assert np.max(np.abs(grad - want)) <= 1e-10 * scale
    chunked = _mse_backward(model, sp, y0s, values, native=True, chunk_bytes=5 * y0s.nbytes)
    assert model.fieldmu_solver().last_chunks == 8
    assert chunked[0] == loss and chunked[1].tobytes() == grad.tobytes()
    assert NativeCNN.created == made + 1  # the handle is kept between calls


def test_solve_native_matches_the_torch_path():
    model, sp, y0s, _ = _grad_case("imex")
    params = {"kappa": R.KAPPA, "mu": _seeded(), "D": DiffLeg(np.array(R.D_COEF))}
    fm = model.fieldmu_solver()
    want = model.solve(params, y0s[0], R.GRAD_TS, sp, dt0=1e-6)
    fm.native_cnn = True
    try:
        got = model.solve(params, y0s[0], R.GRAD_TS, sp, dt0=1e-6)
    finally:
        fm.native_cnn = False
    rel = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print("solve native vs torch", rel)
    assert got.shape == want.shape and rel <= 1e-12


def test_native_on_refuses_a_module_outside_the_family():
    model, sp, y0s, values = _grad_case("imex")
    m = C.PeriodicCNN(1, (4,), act=torch.relu).double().to(DEV)
    fm = model.fieldmu_solver()
    fm.native_cnn = True
    try:
        with pytest.raises(NotImplementedError, match="activation"):
            model.mse_backward({"kappa": R.KAPPA, "mu": m, "D": DiffLeg(np.array(R.D_COEF))}, (y0s, values), sp, R.GRAD_TS, {}, 0.0)
    finally:
        fm.native_cnn = False
