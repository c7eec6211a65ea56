"""The handle lifecycle the library's own networks share (csrc/nn_host.hpp), once for both families: parameters are packed
again after ``set_params`` and after a change of the problem dtype, the workspace follows the problem's batch and grid,
the gradient buffer accumulates, reads and resets, a closed or refused handle owns nothing, and a call launches what its
launch sequence says.  Everything is compared bit for bit with a fresh engine and handle of the same build; accuracy
against torch is tests/test_gpu_cnn_native.py and tests/test_gpu_mixer_native.py.

Grid 8 x 12 (no multiple of the CNN's 8 x 16 tile; patch 4 divides it), batch 2 and 3.  CNN (1, 16, 1) and (1, 5, 20, 1)
(padded widths 16 and 32: two N tiles, two layers of scratch), mixer (patch 4, hidden 8, mix 5 and 7, 1 block)."""
import functools

import numpy as np
import pytest
import torch

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd.engine import HipEngine
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg
import fieldmu_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

GRID, BATCH = (8, 12), 2
FAMILIES = {"cnn-1_16_1": ("cnn", (1, 16, 1)), "cnn-1_5_20_1": ("cnn", (1, 5, 20, 1)), "mixer-p4_C8_m5_7_K1": ("mixer", (4, 8, 5, 7, 1))}
CNNS = [f for f, (kind, _) in FAMILIES.items() if kind == "cnn"]
DTYPES = [np.float64, np.float32]
per_family = pytest.mark.parametrize("family", list(FAMILIES))
per_dtype = pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])


class Engine:
    """an engine on a stream of its own, configured as the field-mu path configures it; ``configure`` again re-keys"""

    def __init__(self, grid, batch, dtype):
        self.stream = torch.cuda.Stream(DEV)
        self.eng = HipEngine(0, stream=self.stream.cuda_stream)
        self.configure(grid, batch, dtype)

    def configure(self, grid, batch, dtype):
        eq = P.CahnHilliard2DPeriodic(P.Domain(grid, R.BOX, "dimensionless"), R.KAPPA, 0.0, DiffLeg(np.array(R.D_COEF)))
        self.eng.configure(dtype=dtype, batch=batch, **eq._engine_problem())
        self.grid, self.batch, self.dtype = grid, batch, dtype

    def open(self, family):
        kind, sizes = FAMILIES[family]
        return self.eng.cnn(sizes, L.CNN_GELU) if kind == "cnn" else self.eng.mixer(*sizes, L.MIXER_GELU)

    def fields(self):
        """device fields (u, gmu, lam0) of the configured shape and dtype, the same numbers for every engine"""
        rng = np.random.default_rng(5)
        shape = (self.batch,) + self.grid
        host = 0.5 + 0.2 * rng.standard_normal(shape), rng.standard_normal(shape), 0.25 * rng.standard_normal(shape)
        with torch.cuda.stream(self.stream):
            return tuple(torch.as_tensor(a.astype(self.dtype)).to(DEV) for a in host)

    def forward(self, net):
        u, _, _ = self.fields()
        with torch.cuda.stream(self.stream):
            mu = torch.empty_like(u)
            net.forward(u.data_ptr(), mu.data_ptr())
            return mu.cpu().numpy()

    def vjp(self, net, times=1):
        """lam after ``times`` vjp calls from lam0 (the parameter gradient stays in the handle)"""
        u, g, lam = self.fields()
        with torch.cuda.stream(self.stream):
            for _ in range(times):
                net.vjp(u.data_ptr(), g.data_ptr(), lam.data_ptr())
            return lam.cpu().numpy()

    def close(self):
        self.eng.close()


def _params(net, seed):
    return 0.3 * np.random.default_rng(seed).standard_normal(net.n_params)


@functools.lru_cache(maxsize=None)
def _fresh(family, grid, batch, dtype, seed):
    """(mu, lam after one vjp, parameter gradient) of a fresh engine and handle with the parameters of ``seed``; computed
    once per case and read-only"""
    e = Engine(grid, batch, dtype)
    net = e.open(family)
    net.set_params(_params(net, seed))
    out = e.forward(net), e.vjp(net), net.grad_read(reset=True)
    net.close()
    e.close()
    for a in out:
        a.setflags(write=False)
    assert all(np.all(np.isfinite(a)) and a.any() for a in out)
    return out


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@per_family
@per_dtype
def test_set_params_packs_again(family, dtype):
    e = Engine(GRID, BATCH, dtype)
    net = e.open(family)
    net.set_params(_params(net, 1))
    first = e.forward(net)
    assert _same(first, _fresh(family, GRID, BATCH, dtype, 1)[0])
    net.set_params(_params(net, 2))
    second = e.forward(net)
    assert not _same(second, first)
    assert _same(second, _fresh(family, GRID, BATCH, dtype, 2)[0])
    net.close()
    e.close()


@per_family
@pytest.mark.parametrize("before, after", [(np.float64, np.float32), (np.float32, np.float64)], ids=["fp64-fp32", "fp32-fp64"])
def test_another_dtype_packs_again(family, before, after):
    """the packed block is in the problem dtype: the same handle after a configure in the other dtype, no set_params between"""
    e = Engine(GRID, BATCH, before)
    net = e.open(family)
    net.set_params(_params(net, 1))
    assert _same(e.forward(net), _fresh(family, GRID, BATCH, before, 1)[0])
    e.configure(GRID, BATCH, after)
    want = _fresh(family, GRID, BATCH, after, 1)
    assert _same(e.forward(net), want[0])
    assert _same(e.vjp(net), want[1]) and _same(net.grad_read(reset=True), want[2])
    net.close()
    e.close()


def _rekeyed(family, dtype, grid, batch):
    """(mu, lam, gradient) of a handle that ran forward and vjp at GRID x BATCH before the engine was configured again"""
    e = Engine(GRID, BATCH, dtype)
    net = e.open(family)
    net.set_params(_params(net, 1))
    e.forward(net)
    e.vjp(net)
    net.grad_read(reset=True)
    e.configure(grid, batch, dtype)
    try:
        return e.forward(net), e.vjp(net), net.grad_read(reset=True)
    finally:
        net.close()
        e.close()


@per_family
@per_dtype
def test_workspace_follows_the_batch(family, dtype):
    got, want = _rekeyed(family, dtype, GRID, 3), _fresh(family, GRID, 3, dtype, 1)
    for name, g, w in zip(("mu", "lam", "grad"), got, want):
        assert _same(g, w), name


@pytest.mark.parametrize("family", CNNS)
@per_dtype
def test_cnn_workspace_follows_the_grid(family, dtype):
    got, want = _rekeyed(family, dtype, (12, 8), BATCH), _fresh(family, (12, 8), BATCH, dtype, 1)
    for name, g, w in zip(("mu", "lam", "grad"), got, want):
        assert _same(g, w), name


@per_dtype
def test_mixer_refuses_another_grid(dtype):
    with pytest.raises(ValueError, match="the mixer was created for a 8 x 12 grid, the problem is now 12 x 8"):
        _rekeyed("mixer-p4_C8_m5_7_K1", dtype, (12, 8), BATCH)


@per_family
@per_dtype
def test_gradient_buffer_accumulates_reads_and_resets(family, dtype):
    e = Engine(GRID, BATCH, dtype)
    net = e.open(family)
    net.set_params(_params(net, 1))
    rounds = []
    for _ in range(2):
        lam = e.vjp(net, times=2)
        kept = net.grad_read(reset=False)
        again = net.grad_read(reset=True)
        assert kept.any() and _same(again, kept)
        assert not net.grad_read(reset=True).any()
        rounds.append((lam, kept))
    assert _same(rounds[0][0], rounds[1][0]) and _same(rounds[0][1], rounds[1][1])
    once = _fresh(family, GRID, BATCH, dtype, 1)[2]
    assert _same(rounds[0][1], once + once)  # two calls accumulate in order
    net.close()
    e.close()


@per_family
@per_dtype
def test_a_closed_handle_and_a_refused_create_own_nothing(family, dtype):
    e = Engine(GRID, BATCH, dtype)
    before = e.eng.device_bytes()
    net = e.open(family)
    assert e.eng.device_bytes() > before  # the gradient buffer
    net.set_params(_params(net, 1))
    e.forward(net)
    e.vjp(net)
    assert e.eng.device_bytes() > before + net.n_params * 8  # the packed parameters and the workspace
    net.close()
    assert e.eng.device_bytes() == before
    kind, sizes = FAMILIES[family]
    with pytest.raises(ValueError, match="activation 99"):
        e.eng.cnn(sizes, 99) if kind == "cnn" else e.eng.mixer(*sizes, 99)
    assert e.eng.device_bytes() == before
    e.close()


def _launches(family):
    """(forward, vjp) launches, read off the launch sequences of csrc/cnn.hip and csrc/mixer.hip"""
    kind, sizes = FAMILIES[family]
    if kind == "cnn":
        n_conv = len(sizes) - 1  # L
        # forward: one convolution per layer.  vjp: the hidden layers again (L - 1), then per layer the weight gradient,
        # its reduction and the backward-data convolution (3 L)
        return n_conv, (n_conv - 1) + 3 * n_conv
    K = sizes[4]
    # forward: conv_in (1); per block statistics, two products, statistics, two products (6 K); the final statistics (1);
    # conv_out (1).  backward: the output bias sum, conv_out's weight gradient and backward-data product, the final
    # norm's two kernels (5); per block and per product a weight gradient and a backward-data product (4 x 2) and per norm
    # two kernels (2 x 2) (12 K); conv_in's weight gradient and backward-data product (2)
    forward, backward = 1 + 6 * K + 1 + 1, 5 + 12 * K + 2
    return forward, (forward - 1) + backward  # vjp: the forward pass without conv_out, then backward


@per_family
@per_dtype
def test_launch_counts(family, dtype):
    e = Engine(GRID, BATCH, dtype)
    net = e.open(family)
    net.set_params(_params(net, 1))
    counts = []
    for call in (e.forward, e.vjp):
        start = e.eng.stage_launches()
        call(net)
        counts.append(e.eng.stage_launches() - start)
    net.close()
    e.close()
    assert tuple(counts) == _launches(family)
