"""The torch mirror of the reference's Mixer2d against a numpy restatement of its definition (tests/mixer_ref.py), its
flat parameter order, the two call shapes, and the host side of the library's own mixer (csrc/mixer.hip): which modules
``native_spec`` takes and refuses, and the packed layouts.  No GPU needed."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from torch import nn  # noqa: E402

import mixer_ref  # noqa: E402
from pde_opt_amd import _lib as L  # noqa: E402
from pde_opt_amd import fieldmu  # noqa: E402
from pde_opt_amd.numerics.functions import mixer as M  # noqa: E402

F = nn.functional


def _seeded(grid, p, C, mp, mh, blocks, act=F.relu, seed=3):
    m = M.Mixer2d((1,) + tuple(grid), p, C, mp, mh, blocks, act=act).double()
    n = sum(q.numel() for q in m.parameters())
    fieldmu.unflatten_params(m, 0.4 * np.random.default_rng(seed).standard_normal(n))
    return m


# a non-square grid, an odd patch size, one patch
CASES = [((8, 12), 4, 6, 5, 7, 2), ((9, 15), 3, 5, 4, 3, 1), ((4, 4), 4, 8, 3, 5, 2)]


@pytest.mark.parametrize("grid, p, C, mp, mh, blocks", CASES)
@pytest.mark.parametrize("act, name", [(F.relu, "relu"), (torch.tanh, "tanh")])
def test_mirror_matches_the_numpy_restatement(grid, p, C, mp, mh, blocks, act, name):
    m = _seeded(grid, p, C, mp, mh, blocks, act)
    u = 0.5 + 0.2 * np.random.default_rng(4).standard_normal(grid)
    want = mixer_ref.forward(fieldmu.flatten_params(m), u, p, C, mp, mh, blocks, name)
    with torch.no_grad():
        got = m(torch.as_tensor(u)).numpy()
    assert got.shape == want.shape == tuple(grid)
    assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))


@pytest.mark.parametrize("grid, p, C, mp, mh, blocks", CASES)
def test_parameter_count_and_flat_order(grid, p, C, mp, mh, blocks):
    m = _seeded(grid, p, C, mp, mh, blocks)
    P = (grid[0] // p) * (grid[1] // p)
    block = [(mp, P), (mp,), (P, mp), (P,), (mh, C), (mh,), (C, mh), (C,), (C, P), (C, P), (P, C), (P, C)]
    want = [(C, 1, p, p), (C,), (C, 1, p, p), (1,)] + block * blocks + [(C, P), (C, P)]
    assert [tuple(q.shape) for q in m.parameters()] == want
    names = [k for k, _ in m.named_parameters()]
    assert names[:4] == ["conv_in.weight", "conv_in.bias", "conv_out.weight", "conv_out.bias"]
    assert names[4:8] == ["blocks.0.patch_mixer.layers.0.weight", "blocks.0.patch_mixer.layers.0.bias",
                          "blocks.0.patch_mixer.layers.1.weight", "blocks.0.patch_mixer.layers.1.bias"]
    assert names[12:16] == ["blocks.0.norm1.weight", "blocks.0.norm1.bias", "blocks.0.norm2.weight", "blocks.0.norm2.bias"]
    assert names[-2:] == ["norm.weight", "norm.bias"]
    assert M.n_params(grid, p, C, mp, mh, blocks) == len(fieldmu.flatten_params(m)) == sum(int(np.prod(s)) for s in want)


def test_single_field_and_batched_calls_agree():
    grid = (8, 12)
    m = _seeded(grid, 4, 6, 5, 7, 2)
    u = torch.as_tensor(0.5 + 0.2 * np.random.default_rng(5).standard_normal((3,) + grid))
    with torch.no_grad():
        batched = m(u[:, None])
        assert batched.shape == (3, 1) + grid
        for b in range(3):
            one = m(u[b])
            assert one.shape == grid
            assert torch.max(torch.abs(one - batched[b, 0])) <= 1e-13 * torch.max(torch.abs(one))


def test_as_field_call_accepts_the_mirror():
    grid = (8, 12)
    m = _seeded(grid, 4, 6, 5, 7, 1)
    u = torch.as_tensor(0.5 + 0.2 * np.random.default_rng(6).standard_normal((2,) + grid))
    with torch.no_grad():
        out = fieldmu.as_field_call(m, u)(u)
        assert out.numel() == u.numel()
        assert torch.equal(out.reshape(u.shape), m(u[:, None])[:, 0])


def test_rejects_an_indivisible_image():
    with pytest.raises(ValueError, match="divide"):
        M.Mixer2d((1, 10, 12), 4, 6, 5, 7, 1)


# ---- the native family -----------------------------------------------------------------------------------------------


def test_native_spec_takes_the_family():
    m = M.Mixer2d((1, 16, 32), 8, 8, 5, 7, 2)
    assert M.native_spec(m) == ((16, 32), 8, 8, 5, 7, 2, "relu")
    assert M.native_refusal(m) is None
    edge = M.Mixer2d((1, 64, 64), 1, 64, 256, 256, 1)  # the upper bounds of the sizes: 4096 patches
    assert M.native_spec(edge) == ((64, 64), 1, 64, 256, 256, 1, "relu") and M.native_refusal(edge) is None
    assert M.native_spec(M.Mixer2d((1, 16, 16), 16, 1, 1, 1, 8)) == ((16, 16), 16, 1, 1, 1, 8, "relu")


@pytest.mark.parametrize("act, name", [
    (F.relu, "relu"), (torch.relu, "relu"), (nn.ReLU(), "relu"), (F.gelu, "gelu"), (nn.GELU(approximate="tanh"), "gelu_tanh"),
    (functools.partial(F.gelu, approximate="tanh"), "gelu_tanh"), (torch.tanh, "tanh"), (nn.Tanh(), "tanh"),
])
def test_native_spec_recognises_the_activation_spellings(act, name):
    assert M.native_spec(M.Mixer2d((1, 8, 8), 2, 8, 5, 7, 1, act=act))[-1] == name


def test_activation_names_are_the_c_enum():
    assert M.NATIVE_ACTIVATIONS == ("gelu", "gelu_tanh", "tanh", "relu")
    assert (L.MIXER_GELU, L.MIXER_GELU_TANH, L.MIXER_TANH, L.MIXER_RELU) == (0, 1, 2, 3)


class _Overridden(M.Mixer2d):
    def forward(self, x):
        return super().forward(x) + 1.0


class _OtherBlock(M.MixerBlock):
    def forward(self, y):
        return y


def _with_other_block():
    m = M.Mixer2d((1, 8, 8), 2, 8, 5, 7, 2)
    m.blocks[1] = _OtherBlock(16, 8, 5, 7)
    return m


def _with_mixed_activations():
    m = M.Mixer2d((1, 8, 8), 2, 8, 5, 7, 2)
    m.blocks[1].hidden_mixer.activation = torch.tanh
    return m


@pytest.mark.parametrize("make, word", [
    (lambda: nn.Conv2d(1, 1, 3), "not a Mixer2d"),
    (lambda: _Overridden((1, 8, 8), 2, 8, 5, 7, 1), "overrides"),
    (_with_other_block, "not a plain MixerBlock"),
    (lambda: M.Mixer2d((2, 8, 8), 2, 8, 5, 7, 1), "in_channels = 2"),
    (lambda: M.Mixer2d((1, 34, 34), 17, 8, 5, 7, 1), "patch_size 17"),
    (lambda: M.Mixer2d((1, 8, 8), 2, 65, 5, 7, 1), "hidden_size 65"),
    (lambda: M.Mixer2d((1, 8, 8), 2, 8, 257, 7, 1), "mix sizes 257 and 7"),
    (lambda: M.Mixer2d((1, 8, 8), 2, 8, 5, 257, 1), "mix sizes 5 and 257"),
    (lambda: M.Mixer2d((1, 65, 64), 1, 2, 2, 2, 1), "4160 patches"),
    (lambda: M.Mixer2d((1, 8, 8), 2, 8, 5, 7, 0), "0 blocks"),
    (lambda: M.Mixer2d((1, 8, 8), 2, 8, 5, 7, 9), "9 blocks"),
    (lambda: M.Mixer2d((1, 8, 8), 2, 8, 5, 7, 1, act=torch.sigmoid), "activation"),
    (_with_mixed_activations, "different activations"),
])
def test_native_spec_refuses_with_a_reason(make, word):
    m = make()
    assert M.native_spec(m) is None
    assert word in M.native_refusal(m)


def test_native_cnn_still_refuses_a_mixer():
    from pde_opt_amd.numerics.functions import cnn as C

    m = M.Mixer2d((1, 8, 8), 2, 8, 5, 7, 1)
    assert C.native_spec(m) is None and "not a PeriodicCNN" in C.native_refusal(m)


# ---- the packed layouts ------------------------------------------------------------------------------------------------

pad16 = lambda c: -(-c // 16) * 16


@pytest.mark.parametrize("O, I", [(24, 8), (1, 17), (16, 33)])
def test_packed_linear_is_the_right_hand_operand(O, I):
    rng = np.random.default_rng(7)
    w, x, d = rng.standard_normal((O, I)), rng.standard_normal((5, I)), rng.standard_normal((5, O))
    f, r = M.pack_linear(w), M.pack_linear(w, backward=True)
    assert f.shape == (pad16(I), pad16(O)) and r.shape == (pad16(O), pad16(I))
    xp, dp = np.zeros((5, pad16(I))), np.zeros((5, pad16(O)))
    xp[:, :I], dp[:, :O] = x, d
    z, g = xp @ f, dp @ r
    np.testing.assert_allclose(z[:, :O], x @ w.T, rtol=0, atol=1e-13)
    np.testing.assert_allclose(g[:, :I], d @ w, rtol=0, atol=1e-13)
    assert not z[:, O:].any() and not g[:, I:].any()  # the padding stays zero
    assert np.array_equal(M.pack_linear(w.T.copy(), stored_io=True), f)


@pytest.mark.parametrize("grid, p", [((8, 12), 4), ((9, 15), 3), ((4, 6), 1)])
def test_patch_matrix_and_packed_convolutions_match_torch(grid, p):
    C = 5
    rng = np.random.default_rng(8)
    u = rng.standard_normal(grid)
    P, Q = (grid[0] // p) * (grid[1] // p), p * p
    up = M.patch_matrix(u, p)
    assert up.shape == (P, Q)
    cin, cout = nn.Conv2d(1, C, p, stride=p).double(), nn.ConvTranspose2d(C, 1, p, stride=p).double()
    with torch.no_grad():
        want = cin(torch.as_tensor(u)[None, None])[0].reshape(C, P).numpy()
        upp = np.zeros((P, pad16(Q)))
        upp[:, :Q] = up
        got = upp @ M.pack_linear(cin.weight.numpy().reshape(C, Q)) + np.pad(cin.bias.numpy(), (0, pad16(C) - C))
        np.testing.assert_allclose(got[:, :C].T, want, rtol=0, atol=1e-13)
        # conv_out: its weight (C, 1, p, p) reads as the map from C channels to p p pixels, stored (I, O)
        y = rng.standard_normal((C, P))
        want = cout(torch.as_tensor(y).reshape(1, C, grid[0] // p, grid[1] // p))[0, 0].numpy()
        yp = np.zeros((P, pad16(C)))
        yp[:, :C] = y.T
        got = yp @ M.pack_linear(cout.weight.numpy().reshape(C, Q), stored_io=True) + cout.bias.numpy()[0]
        np.testing.assert_allclose(got[:, :Q], M.patch_matrix(want, p), rtol=0, atol=1e-13)
