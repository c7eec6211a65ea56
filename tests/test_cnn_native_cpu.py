"""Host side of the library's own PeriodicCNN (csrc/cnn.hip): which modules ``native_spec`` takes and refuses, and the
packed weight layouts against a direct numpy convolution.  No GPU needed."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from torch import nn  # noqa: E402

from pde_opt_amd import _lib as L  # noqa: E402
from pde_opt_amd.numerics.functions import cnn as C  # noqa: E402

F = nn.functional


def test_native_spec_takes_the_notebook_cnn():
    m = C.PeriodicCNN(1, (32, 64, 64))
    assert C.native_spec(m) == ((1, 32, 64, 64, 1), "gelu")
    assert C.native_refusal(m) is None


@pytest.mark.parametrize("act, name", [
    (F.gelu, "gelu"), (nn.GELU(), "gelu"), (nn.GELU(approximate="tanh"), "gelu_tanh"),
    (functools.partial(F.gelu, approximate="tanh"), "gelu_tanh"), (torch.tanh, "tanh"), (F.tanh, "tanh"), (nn.Tanh(), "tanh"),
])
def test_native_spec_recognises_the_activation_spellings(act, name):
    assert C.native_spec(C.PeriodicCNN(1, (8, 24), act=act)) == ((1, 8, 24, 1), name)


def test_activation_names_are_the_c_enum():
    assert C.NATIVE_ACTIVATIONS == ("gelu", "gelu_tanh", "tanh")
    assert (L.CNN_GELU, L.CNN_GELU_TANH, L.CNN_TANH) == (0, 1, 2)


class _Overridden(C.PeriodicCNN):
    def forward(self, x):
        return super().forward(x) + 1.0


@pytest.mark.parametrize("make, word", [
    (lambda: C.PeriodicCNN(1, (16,), kernel_size=5), "kernel_size"),
    (lambda: C.PeriodicCNN(1, (65,)), "width 65"),
    (lambda: C.PeriodicCNN(2, (16,)), "in_channels = 2"),
    (lambda: C.PeriodicCNN(1, (16,), act=torch.relu), "activation"),
    (lambda: C.PeriodicCNN(1, (16,), act=functools.partial(F.gelu, approximate="sigmoid")), "activation"),
    (lambda: _Overridden(1, (16,)), "overrides"),
    (lambda: C.PeriodicCNN(1, ()), "hidden layers"),
    (lambda: C.PeriodicCNN(1, (8,) * 7), "hidden layers"),
    (lambda: nn.Conv2d(1, 1, 3), "not a PeriodicCNN"),
])
def test_native_spec_refuses_with_a_reason(make, word):
    m = make()
    assert C.native_spec(m) is None
    assert word in C.native_refusal(m)


# ---- the packed layouts ----------------------------------------------------------------------------------------------

NX, NY = 5, 4


def _conv_direct(w, a):
    """z[o, x, y] = sum_{i, ky, kx} w[o, i, ky, kx] a[i, x + ky - 1, y + kx - 1], periodic (torch's Conv2d, circular)"""
    O, I = w.shape[:2]
    z = np.zeros((O, NX, NY))
    for ky in range(3):
        for kx in range(3):
            shifted = np.roll(a, (-(ky - 1), -(kx - 1)), axis=(1, 2))
            z += np.einsum("oi,ixy->oxy", w[:, :, ky, kx], shifted)
    return z


def _conv_packed(packed, a_cl):
    """what the kernel computes from a packed block (9, Cin_p, Cout_p) and a channels-last field (NX, NY, Cin_p)"""
    out = np.zeros(a_cl.shape[:2] + (packed.shape[2],))
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        out += np.roll(a_cl, (-(ky - 1), -(kx - 1)), axis=(0, 1)) @ packed[tap]
    return out


def _channels_last(a, cp):
    out = np.zeros((NX, NY, cp))
    out[:, :, :a.shape[0]] = np.moveaxis(a, 0, -1)
    return out


@pytest.mark.parametrize("O, I", [(24, 8), (1, 17), (16, 1)])
def test_packed_weights_match_a_direct_convolution(O, I):
    rng = np.random.default_rng(3)
    w = rng.standard_normal((O, I, 3, 3))
    a = rng.standard_normal((I, NX, NY))
    p = C.pack_conv3x3(w)
    pad = lambda c: -(-c // 16) * 16
    assert p.shape == (9, pad(I), pad(O))
    z = _conv_packed(p, _channels_last(a, pad(I)))
    np.testing.assert_allclose(np.moveaxis(z[:, :, :O], -1, 0), _conv_direct(w, a), rtol=0, atol=1e-13)
    assert not z[:, :, O:].any()  # the padding stays zero


@pytest.mark.parametrize("O, I", [(24, 8), (1, 17), (16, 1)])
def test_backward_packed_weights_are_the_transpose(O, I):
    """<d, conv(w, a)> = <conv(backward pack, d), a> for all a, d: the backward-data pass is the adjoint map"""
    rng = np.random.default_rng(4)
    w = rng.standard_normal((O, I, 3, 3))
    a = rng.standard_normal((I, NX, NY))
    d = rng.standard_normal((O, NX, NY))
    pb = C.pack_conv3x3(w, backward=True)
    pad = lambda c: -(-c // 16) * 16
    assert pb.shape == (9, pad(O), pad(I))
    ga = _conv_packed(pb, _channels_last(d, pad(O)))
    assert not ga[:, :, I:].any()
    lhs = float((d * _conv_direct(w, a)).sum())
    rhs = float((np.moveaxis(ga[:, :, :I], -1, 0) * a).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    # and entry by entry against torch's own gradient of the circular convolution
    conv = nn.Conv2d(I, O, 3, padding=1, padding_mode="circular", bias=False).double()
    with torch.no_grad():
        conv.weight.copy_(torch.as_tensor(w))
    at = torch.as_tensor(a)[None].requires_grad_(True)
    (conv(at) * torch.as_tensor(d)[None]).sum().backward()
    np.testing.assert_allclose(np.moveaxis(ga[:, :, :I], -1, 0), at.grad[0].numpy(), rtol=0, atol=1e-12)


def test_pack_refuses_other_kernel_sizes():
    with pytest.raises(ValueError):
        C.pack_conv3x3(np.zeros((4, 4, 5, 5)))
