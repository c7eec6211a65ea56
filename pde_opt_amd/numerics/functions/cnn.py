"""A periodic CNN as a closure (the reference's pde_opt/numerics/functions/cnn.py:13-102), as a ``torch.nn.Module``.

``PeriodicCNN(in_channels, hidden_channels, out_channels, kernel_size, act)`` keeps the reference's constructor
arguments: a stack of ``Conv2d -> act`` blocks and a final ``Conv2d`` without activation, all with circular "same"
padding and stride 1, so the map is translation-equivariant on the torus.  It is not pointwise: as ``mu`` of
``CahnHilliard2DPeriodic`` it runs in torch on the GPU next to the HIP kernels, which see the field it returns
(``pde_opt_amd.fieldmu``).  Input ``(B, C, H, W)`` or ``(C, H, W)``; the output has the same spatial size.

The library can also evaluate and differentiate such a network itself (csrc/cnn.hip, ``FieldMuSolver.native_cnn``):
``native_spec`` says whether a module is of the family its kernels cover, ``pack_conv3x3`` is the weight layout they read.

Importing this module imports torch (the package itself does not)."""

from __future__ import annotations

import functools
from typing import Callable, Optional, Sequence

import numpy as np
import torch
from torch import nn


class PeriodicConvBlock(nn.Module):
    """``Conv2d -> act`` with periodic padding (cnn.py:13-43)"""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int = 3, act: Callable = nn.functional.gelu):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=1, padding=kernel_size // 2,
                              padding_mode="circular", bias=True)
        self.act = act

    def forward(self, x):
        return self.act(self.conv(x))


class PeriodicCNN(nn.Module):
    """Stack of periodic conv blocks; the final conv returns ``out_channels`` (``in_channels`` when None), cnn.py:46-102"""

    def __init__(self, in_channels: int, hidden_channels: Sequence[int] = (32, 64, 64), out_channels: Optional[int] = None,
                 kernel_size: int = 3, act: Callable = nn.functional.gelu):
        super().__init__()
        if kernel_size % 2 != 1:
            raise ValueError("use odd kernels to avoid off-by-one alignment")
        out_channels = in_channels if out_channels is None else out_channels
        blocks, c_prev = [], in_channels
        for c_next in hidden_channels:
            blocks.append(PeriodicConvBlock(c_prev, c_next, kernel_size, act))
            c_prev = c_next
        blocks.append(nn.Conv2d(c_prev, out_channels, kernel_size, stride=1, padding=kernel_size // 2,
                                padding_mode="circular", bias=True))
        self.layers = nn.ModuleList(blocks)

    def forward(self, x):
        single = x.dim() == 3
        y = x[None] if single else x
        for layer in self.layers:
            y = layer(y)
        return y[0] if single else y


# ---- the family the library's own kernels cover (csrc/cnn.hip) ---------------------------------------------------------

NATIVE_ACTIVATIONS = ("gelu", "gelu_tanh", "tanh")  # index = pdeopt_cnn_activation
NATIVE_MAX_HIDDEN, NATIVE_MAX_WIDTH = 6, 64


def _activation_name(act) -> Optional[str]:
    """``gelu`` (erf form), ``gelu_tanh`` or ``tanh`` for the spellings of these three that torch offers, else None"""
    F = nn.functional
    if act is F.gelu or act is torch.tanh or act is F.tanh:
        return "gelu" if act is F.gelu else "tanh"
    if isinstance(act, nn.Tanh):
        return "tanh"
    approx = None
    if isinstance(act, nn.GELU):
        approx = act.approximate
    elif isinstance(act, functools.partial) and act.func is F.gelu and not act.args and set(act.keywords) <= {"approximate"}:
        approx = act.keywords.get("approximate", "none")
    return {"none": "gelu", "tanh": "gelu_tanh"}.get(approx)


def _inspect(module):
    """``((channels, activation), None)`` or ``(None, reason)``"""
    if not isinstance(module, PeriodicCNN):
        return None, f"a {type(module).__name__} is not a PeriodicCNN"
    if type(module).forward is not PeriodicCNN.forward:
        return None, f"{type(module).__name__} overrides PeriodicCNN.forward"
    layers = list(module.layers)
    if not layers or not isinstance(layers[-1], nn.Conv2d):
        return None, "the last layer is not a Conv2d"
    blocks, convs, acts = layers[:-1], [], []
    for blk in blocks:
        if not isinstance(blk, PeriodicConvBlock) or type(blk).forward is not PeriodicConvBlock.forward:
            return None, f"hidden layer {type(blk).__name__} is not a plain PeriodicConvBlock"
        convs.append(blk.conv)
        acts.append(_activation_name(blk.act))
        if acts[-1] is None:
            return None, f"activation {blk.act!r} is not one of gelu (erf or tanh form) and tanh"
    if not 1 <= len(blocks) <= NATIVE_MAX_HIDDEN:
        return None, f"{len(blocks)} hidden layers: supported are 1 to {NATIVE_MAX_HIDDEN}"
    if len(set(acts)) != 1:
        return None, f"the hidden layers use different activations {sorted(set(acts))}"
    convs.append(layers[-1])
    for k, conv in enumerate(convs):
        if type(conv) is not nn.Conv2d:
            return None, f"layer {k} is a {type(conv).__name__}, not a Conv2d"
        if tuple(conv.kernel_size) != (3, 3):
            return None, f"kernel_size {tuple(conv.kernel_size)}: supported is 3"
        if (tuple(conv.stride), tuple(conv.dilation), conv.groups) != ((1, 1), (1, 1), 1):
            return None, f"layer {k} has a stride, dilation or groups other than 1"
        if conv.padding_mode != "circular" or tuple(conv.padding) != (1, 1):
            return None, f'layer {k} does not use circular "same" padding'
        if conv.bias is None:
            return None, f"layer {k} has no bias"
    channels = (convs[0].in_channels,) + tuple(c.out_channels for c in convs)
    if any(a.in_channels != c for a, c in zip(convs, channels)):
        return None, "the layers' channel counts do not chain"
    if channels[0] != 1 or channels[-1] != 1:
        return None, f"in_channels = {channels[0]}, out_channels = {channels[-1]}: supported is one channel in, one out"
    if max(channels) > NATIVE_MAX_WIDTH:
        return None, f"hidden width {max(channels)}: supported are 1 to {NATIVE_MAX_WIDTH}"
    return (channels, acts[0]), None


def native_spec(module):
    """``(channels, activation)`` -- ``(1, hidden..., 1)`` and a name of ``NATIVE_ACTIVATIONS`` -- when ``module`` is
    exactly a ``PeriodicCNN`` of the family csrc/cnn.hip evaluates; None otherwise (``native_refusal`` says why)"""
    return _inspect(module)[0]


def native_refusal(module) -> Optional[str]:
    """why ``native_spec(module)`` is None, or None"""
    return _inspect(module)[1]


def pack_conv3x3(weight, backward: bool = False) -> np.ndarray:
    """The layout csrc/cnn.hip reads a torch weight ``(O, I, 3, 3)`` in: ``(9, pad16(I), pad16(O))`` with
    ``packed[3 ky + kx, i, o] = weight[o, i, ky, kx]`` and zeros in the padding.  ``backward``: the weights of the
    backward-data pass, the same convolution run from the output's cotangent to the input's,
    ``(9, pad16(O), pad16(I))`` with ``packed[3 ky + kx, o, i] = weight[o, i, 2 - ky, 2 - kx]`` (transposed, flipped)."""
    w = np.asarray(weight)
    O, I = w.shape[:2]
    if w.shape != (O, I, 3, 3):
        raise ValueError(f"weight of shape {w.shape}: expected (O, I, 3, 3)")
    pad = lambda c: -(-c // 16) * 16
    taps = w.reshape(O, I, 9)
    if backward:
        out = np.zeros((9, pad(O), pad(I)), dtype=w.dtype)
        out[:, :O, :I] = np.transpose(taps[:, :, ::-1], (2, 0, 1))
    else:
        out = np.zeros((9, pad(I), pad(O)), dtype=w.dtype)
        out[:, :I, :O] = np.transpose(taps, (2, 1, 0))
    return out
