"""The library's own Mixer2d (csrc/mixer.hip) on the MI355X against the same module evaluated by torch in fp64 on the
device and its autograd.grad: values and vector-Jacobian products in fp64 and fp32, determinism of the gradient sums, the
refusals, and mse_backward / solve with ``FieldMuSolver.native_mixer`` against the torch path of the same solver."""
import functools

import numpy as np
import pytest
import torch

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd import fieldmu
from pde_opt_amd.engine import HipEngine, NativeMixer
from pde_opt_amd.numerics.functions import mixer as M
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg
import fieldmu_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F = torch.nn.functional
ACTS = {"relu": F.relu, "gelu": F.gelu, "gelu_tanh": functools.partial(F.gelu, approximate="tanh"), "tanh": torch.tanh}

# (grid, patch, hidden, (mix_patch, mix_hidden), blocks, batch, activation, seed).  Grids: one patch (the layer norm is over
# C numbers alone); a whole tile of patches; a ragged 3 x 5 patch grid, padding in P; an odd patch size; the grid of the
# field-mu gradient problem; patches that are pixels, several tiles.  The seeds of the relu cases are chosen so that the
# reference's hidden pre-activations keep clear of zero (test_relu_cases_keep_clear_of_the_kink).
CASES = [
    ((4, 4), 4, 8, (5, 7), 1, 1, "relu", 0),
    ((4, 4), 4, 16, (16, 16), 2, 3, "relu", 0),
    ((8, 8), 2, 16, (16, 16), 1, 1, "relu", 0),
    ((8, 8), 2, 8, (5, 7), 2, 3, "relu", 0),
    ((8, 8), 2, 64, (64, 32), 1, 1, "relu", 0),
    ((12, 20), 4, 8, (5, 7), 1, 1, "relu", 0),
    ((12, 20), 4, 24, (16, 16), 2, 3, "relu", 1),
    ((12, 20), 4, 16, (64, 32), 4, 1, "relu", 0),
    ((12, 20), 4, 64, (5, 7), 1, 3, "relu", 0),
    ((12, 20), 4, 24, (5, 7), 4, 1, "relu", 0),
    ((18, 6), 3, 8, (5, 7), 2, 1, "relu", 0),
    ((18, 6), 3, 24, (64, 32), 1, 3, "relu", 0),
    ((18, 6), 3, 16, (16, 16), 4, 1, "relu", 0),
    ((16, 32), 8, 8, (5, 7), 2, 1, "relu", 0),
    ((16, 32), 8, 8, (5, 7), 2, 3, "relu", 0),
    ((16, 32), 8, 24, (16, 16), 1, 1, "relu", 0),
    ((16, 32), 8, 64, (64, 32), 2, 3, "relu", 92),
    ((16, 16), 1, 8, (5, 7), 1, 1, "relu", 0),
    ((16, 16), 1, 16, (16, 16), 2, 3, "relu", 135),
    ((16, 16), 1, 24, (64, 32), 1, 1, "relu", 4),
    ((16, 16), 1, 64, (16, 16), 1, 3, "relu", 8),
    ((12, 20), 4, 24, (5, 7), 2, 3, "gelu", 0),
    ((12, 20), 4, 24, (5, 7), 2, 3, "gelu_tanh", 0),
    ((12, 20), 4, 24, (5, 7), 2, 3, "tanh", 0),
]
IDS = [f"{g[0]}x{g[1]}-p{p}-C{c}-m{m[0]}_{m[1]}-K{k}-B{b}-{a}" for g, p, c, m, k, b, a, _ in CASES]
RELU_CLEARANCE = 1e-5  # no hidden pre-activation of the reference within this fraction of its layer's largest


def build_module(case):
    """Mixer2d in fp64 on the CPU with seeded parameters of unit gain: weights N(0, 1 / fan_in), layer-norm weights
    1 + 0.1 N(0, 1), biases 0.1 N(0, 1)"""
    grid, p, c, (mp, mh), k, _, act, seed = case
    m = M.Mixer2d((1,) + grid, p, c, mp, mh, k, act=ACTS[act]).double()
    rng = np.random.default_rng(100 + seed)
    parts = []
    for name, q in m.named_parameters():
        g = rng.standard_normal(q.numel())
        if "norm" in name:
            parts.append(1.0 + 0.1 * g if name.endswith("weight") else 0.1 * g)
        elif q.dim() == 1:
            parts.append(0.1 * g)
        else:
            parts.append(g * (q[0].numel() if "conv_in" in name or q.dim() == 2 else q.shape[0]) ** -0.5)
    fieldmu.unflatten_params(m, np.concatenate(parts))
    return m


def inputs(case):
    """(u, gmu, lam0), representable in fp32"""
    grid, B = case[0], case[5]
    rng = np.random.default_rng(5)
    u = (0.5 + 0.2 * rng.standard_normal((B,) + grid)).astype(np.float32).astype(np.float64)
    g = rng.standard_normal((B,) + grid).astype(np.float32).astype(np.float64)
    lam0 = (0.25 * rng.standard_normal((B,) + grid)).astype(np.float32).astype(np.float64)
    return u, g, lam0


def relu_clearance(m, u):
    """the smallest |z| / max |z| over the hidden layers of ``m`` evaluated on the batch ``u (B, H, W)``"""
    seen = []
    hooks = [mlp.layers[0].register_forward_hook(lambda mod, args, out: seen.append(float(out.abs().min() / out.abs().max())))
             for blk in m.blocks for mlp in (blk.patch_mixer, blk.hidden_mixer)]
    try:
        with torch.no_grad():
            m(u[:, None])
    finally:
        for h in hooks:
            h.remove()
    return min(seen)


def _vjp(m, u, g):
    """(mu, N'(u)^T g, flat parameter gradient of <g, N(u)>) by torch, in the dtype of the module"""
    u = u.clone().requires_grad_(True)
    mu = m(u[:, None])[:, 0]
    grads = torch.autograd.grad((mu * g).sum(), [u] + list(m.parameters()))
    return mu.detach(), grads[0], torch.cat([q.reshape(-1) for q in grads[1:]])


@functools.lru_cache(maxsize=None)
def _reference(case):
    """inputs and what torch gives for them in fp64 and in fp32 on the device; computed once per case"""
    u, g, lam0 = inputs(case)
    m = build_module(case).to(DEV)
    ud, gd = torch.as_tensor(u).to(DEV), torch.as_tensor(g).to(DEV)
    ref = {"u": u, "g": g, "lam0": lam0, "params": fieldmu.flatten_params(m), "spec": M.native_spec(m)}
    ref["clearance"] = relu_clearance(m, ud)
    ref["f64"] = tuple(t.cpu().numpy() for t in _vjp(m, ud, gd))
    ref["f32"] = tuple(t.double().cpu().numpy() for t in _vjp(m.float(), ud.float(), gd.float()))
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


def _handle(eng, spec):
    return eng.mixer(*spec[1:6], M.NATIVE_ACTIVATIONS.index(spec[6]))


def _native(case, dtype):
    """(mu, lam after one vjp from lam0, parameter gradient) of the library in ``dtype``, as fp64 arrays, and the handle"""
    ref = _reference(case)
    eng, stream = _engine(case[0], case[5], dtype)
    net = _handle(eng, ref["spec"])
    assert net.n_params == ref["params"].size
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


@pytest.mark.parametrize("case", [c for c in CASES if c[6] == "relu"], ids=[i for i, c in zip(IDS, CASES) if c[6] == "relu"])
def test_relu_cases_keep_clear_of_the_kink(case):
    """relu's derivative jumps at zero: a pre-activation that changes sign between fp32 and fp64 moves the gradient by a
    whole weight.  A condition on the fp64 torch reference alone, not a measurement of the library"""
    c = _reference(case)["clearance"]
    print(case, "smallest |z| / max |z| of a hidden layer: %.3g" % c)
    assert c > RELU_CLEARANCE


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp64_matches_torch(case):
    """values to 1e-12 of max |mu|, the lam increment and the parameter gradient to 1e-10 of their maxima (the gates of
    test_gpu_cnn_native.py)"""
    ref = _reference(case)
    (mu, lam, grad), net, _ = _native(case, np.float64)
    net.close()
    want_mu, want_gu, want_gp = ref["f64"]
    e = (_err(mu, want_mu) / np.max(np.abs(want_mu)), _err(lam, ref["lam0"] + want_gu) / np.max(np.abs(want_gu)),
         _err(grad, want_gp) / np.max(np.abs(want_gp)))
    print(case, "fp64 rel err: mu %.3g, lam %.3g, grad %.3g" % e)
    assert e[0] <= 1e-12
    assert e[1] <= 1e-10
    assert e[2] <= 1e-10


FP32_MARGIN = 4.0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp32_is_as_close_to_fp64_as_torch_fp32(case):
    """the native fp32 error against torch fp64 is at most 4 x that of torch's own fp32 evaluation of the same inputs
    (another summation order, fp64 layer-norm statistics), with a floor of 1e-6 of the maximum"""
    ref = _reference(case)
    (mu, lam, grad), net, _ = _native(case, np.float32)
    net.close()
    lam0_32 = ref["lam0"].astype(np.float32)
    torch_lam = (lam0_32 + ref["f32"][1].astype(np.float32)).astype(np.float64)  # torch's own lam += u.grad in fp32
    got = (mu, lam, grad)
    theirs = (ref["f32"][0], torch_lam, ref["f32"][2])
    want = (ref["f64"][0], ref["lam0"] + ref["f64"][1], ref["f64"][2])
    scales = tuple(np.max(np.abs(ref["f64"][k])) for k in range(3))
    report = []
    for name, a, t, w, s in zip(("mu", "lam", "grad"), got, theirs, want, scales):
        mine, torchs = _err(a, w) / s, _err(t, w) / s
        report.append((name, mine, torchs))
        print(case, name, "fp32 rel err: native %.3g, torch %.3g, ratio %.3g" % (mine, torchs, mine / max(torchs, 1e-30)))
    for name, mine, torchs in report:
        assert mine <= max(FP32_MARGIN * torchs, 1e-6), name


@pytest.mark.parametrize("B", [1, 3])
def test_vjp_is_deterministic_and_accumulates_in_order(B):
    case = next(c for c in CASES if c[:2] == ((12, 20), 4) and c[2] == (8 if B == 1 else 24) and c[5] == B)
    ref = _reference(case)
    (_, lam1, g1), net, (u, g, stream) = _native(case, np.float64)
    with torch.cuda.stream(stream):
        lam = torch.as_tensor(ref["lam0"]).to(DEV)
        net.vjp(u.data_ptr(), g.data_ptr(), lam.data_ptr())
        g2 = net.grad_read(reset=True)
        assert lam.cpu().numpy().tobytes() == lam1.tobytes() and g2.tobytes() == g1.tobytes()
        for _ in range(3):
            net.vjp(u.data_ptr(), g.data_ptr(), lam.data_ptr())
        g3 = net.grad_read(reset=True)
    assert g1.any()
    assert g3.tobytes() == ((g1 + g1) + g1).tobytes()
    assert not net.grad_read().any()  # reset
    net.close()


def test_refusals():
    eng, stream = _engine((16, 16), 1, np.float64)
    net = eng.mixer(4, 8, 5, 7, 1, L.MIXER_RELU)
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
    # patch, hidden, mix_patch, mix_hidden, blocks, activation outside the family; 16 x 16 pixels as patches of 1 are
    # 256 patches, and no grid here exceeds 4096
    for sizes in ((0, 8, 5, 7, 1, 3), (8, 65, 5, 7, 1, 3), (8, 8, 257, 7, 1, 3), (8, 8, 5, 0, 1, 3), (8, 8, 5, 7, 9, 3), (8, 8, 5, 7, 1, 4)):
        with pytest.raises(ValueError):
            eng.mixer(*sizes)
    ragged, _ = _engine((12, 20), 1, np.float64)
    with pytest.raises(ValueError, match="divide"):
        ragged.mixer(8, 8, 5, 7, 1, L.MIXER_RELU)
    with pytest.raises(ValueError, match="patch size 17"):
        ragged.mixer(17, 8, 5, 7, 1, L.MIXER_RELU)


# ---- through FieldMuSolver -------------------------------------------------------------------------------------------


def _grad_case(integrator):
    solver = P.SemiImplicitFourierSpectral if integrator == "imex" else P.Euler
    model = P.PDEModel(P.CahnHilliard2DPeriodic, P.Domain(R.GRAD_SHAPE, R.BOX, "dimensionless"), solver)
    y0s, values = R.grad_problem()
    return model, ({"A": 0.5} if integrator == "imex" else {}), y0s, values


def _seeded():
    m = M.Mixer2d((1,) + R.GRAD_SHAPE, 8, 8, 5, 7, 2).double()
    n = sum(q.numel() for q in m.parameters())
    fieldmu.unflatten_params(m, 0.3 * np.random.default_rng(7).standard_normal(n))
    return m.to(DEV)


def _mse_backward(model, sp, y0s, values, native, chunk_bytes=None):
    m = _seeded()
    fm = model.fieldmu_solver()
    fm.native_mixer, fm.chunk_bytes = native, chunk_bytes
    params = {"kappa": R.KAPPA, "mu": m, "D": DiffLeg(np.array(R.D_COEF))}
    try:
        loss = model.mse_backward(params, (y0s, values), sp, R.GRAD_TS, {}, 0.0)
    finally:
        fm.native_mixer, fm.chunk_bytes = False, None
    return loss, fieldmu.flatten_grads(m), params


@pytest.mark.parametrize("integrator", ["imex", "euler"])
def test_mse_backward_native_matches_the_torch_path(integrator):
    """the problem of test_gpu_fieldmu.py::test_mse_gradient with Mixer2d((1, 16, 32), 8, 8, 5, 7, 2), fp64: loss to 1e-12 J,
    gradient to 1e-10 of its maximum, identical bits under chunking"""
    model, sp, y0s, values = _grad_case(integrator)
    made = NativeMixer.created
    J, want, _ = _mse_backward(model, sp, y0s, values, native=False)
    assert NativeMixer.created == made  # switch off: a supported module still runs in torch
    loss, grad, _ = _mse_backward(model, sp, y0s, values, native=True)
    assert NativeMixer.created == made + 1
    scale = np.max(np.abs(want))
    print(integrator, "loss", loss, "torch", J, "grad err", np.max(np.abs(grad - want)) / scale)
    assert abs(loss - J) <= 1e-12 * J
    assert np.max(np.abs(grad - want)) <= 1e-10 * scale
    chunked = _mse_backward(model, sp, y0s, values, native=True, chunk_bytes=5 * y0s.nbytes)
    assert model.fieldmu_solver().last_chunks == 8
    assert chunked[0] == loss and chunked[1].tobytes() == grad.tobytes()
    assert NativeMixer.created == made + 1  # the handle is kept between calls


def test_solve_native_matches_the_torch_path():
    model, sp, y0s, _ = _grad_case("imex")
    params = {"kappa": R.KAPPA, "mu": _seeded(), "D": DiffLeg(np.array(R.D_COEF))}
    fm = model.fieldmu_solver()
    want = model.solve(params, y0s[0], R.GRAD_TS, sp, dt0=1e-6)
    fm.native_mixer = True
    try:
        got = model.solve(params, y0s[0], R.GRAD_TS, sp, dt0=1e-6)
    finally:
        fm.native_mixer = False
    rel = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print("solve native vs torch", rel)
    assert got.shape == want.shape and rel <= 1e-12


def test_native_on_refuses_a_module_outside_the_family():
    from pde_opt_amd.numerics.functions.cnn import PeriodicCNN

    model, sp, y0s, values = _grad_case("imex")
    m = PeriodicCNN(1, (4,)).double().to(DEV)
    fm = model.fieldmu_solver()
    made = NativeMixer.created
    fm.native_mixer = True
    try:
        with pytest.raises(NotImplementedError, match="not a Mixer2d"):
            model.mse_backward({"kappa": R.KAPPA, "mu": m, "D": DiffLeg(np.array(R.D_COEF))}, (y0s, values), sp, R.GRAD_TS, {}, 0.0)
    finally:
        fm.native_mixer = False
    assert NativeMixer.created == made
