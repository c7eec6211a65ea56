"""An MLP-mixer as a closure (the reference's pde_opt/numerics/functions/mixer_mlp.py:13-86), as a ``torch.nn.Module``.

``Mixer2d(img_size, patch_size, hidden_size, mix_patch_size, mix_hidden_size, num_blocks)`` keeps the reference's
constructor arguments and attribute names (``conv_in``, ``conv_out``, ``blocks``, ``norm``; per block ``patch_mixer``,
``hidden_mixer``, ``norm1``, ``norm2``).  For one field ``u (H, W)``, ``C = hidden_size`` and ``P = (H / p)(W / p)``:

* ``conv_in``: a ``p x p`` convolution of stride ``p`` to ``C`` channels, flattened to ``y (C, P)`` (patches row-major);
* per block ``y += patch_mixer(norm1(y))`` (an MLP ``P -> mix_patch_size -> P`` on every channel row), then across the
  transpose ``y += hidden_mixer(norm2(y))`` (``C -> mix_hidden_size -> C`` on every patch row);
* the layer norms run over the whole ``(C, P)`` array: one mean and one biased variance per field, ``eps = 1e-5``, an
  elementwise weight and bias of the full shape;
* ``conv_out``: a transposed ``p x p`` convolution of stride ``p`` back to ``(H, W)``.

The hidden activation is that of equinox's ``MLP``, relu by default; ``act`` overrides it.  The map is global and its
parameter shapes depend on ``P``: a module is bound to one grid.  ``forward`` takes one field ``(H, W)`` -- the
reference's call -- or a batch ``(B, 1, H, W)`` and returns the same shape.

The library can also evaluate and differentiate such a network itself (csrc/mixer.hip, ``FieldMuSolver.native_mixer``):
``native_spec`` says whether a module is of the family its kernels cover, ``pack_linear`` and ``patch_matrix`` are the
layouts they read.  Flat parameter order, ``module.parameters()``: ``conv_in.weight (C, 1, p, p)``, ``conv_in.bias (C)``,
``conv_out.weight (C, 1, p, p)``, ``conv_out.bias (1)``; per block the patch mixer's ``W1 (Mp, P)``, ``b1``, ``W2 (P, Mp)``,
``b2``, the hidden mixer's ``W3 (Mh, C)``, ``b3``, ``W4 (C, Mh)``, ``b4``, ``norm1.weight``, ``norm1.bias`` ``(C, P)``,
``norm2.weight``, ``norm2.bias`` ``(P, C)``; then ``norm.weight``, ``norm.bias`` ``(C, P)``.

Importing this module imports torch (the package itself does not)."""

from __future__ import annotations

from typing import Callable, Optional

import numpy as np
import torch
from torch import nn

from .cnn import _activation_name as _cnn_activation_name

LN_EPS = 1e-5


class MLP(nn.Module):
    """equinox.nn.MLP with ``depth=1``: ``Linear -> activation -> Linear`` on the last axis"""

    def __init__(self, in_size: int, out_size: int, width_size: int, activation: Callable = nn.functional.relu):
        super().__init__()
        self.layers = nn.ModuleList([nn.Linear(in_size, width_size), nn.Linear(width_size, out_size)])
        self.activation = activation

    def forward(self, x):
        return self.layers[1](self.activation(self.layers[0](x)))


class MixerBlock(nn.Module):
    """mixer_mlp.py:13-37 on ``y (..., C, P)``"""

    def __init__(self, num_patches: int, hidden_size: int, mix_patch_size: int, mix_hidden_size: int,
                 act: Callable = nn.functional.relu):
        super().__init__()
        self.patch_mixer = MLP(num_patches, num_patches, mix_patch_size, act)
        self.hidden_mixer = MLP(hidden_size, hidden_size, mix_hidden_size, act)
        self.norm1 = nn.LayerNorm((hidden_size, num_patches), eps=LN_EPS)
        self.norm2 = nn.LayerNorm((num_patches, hidden_size), eps=LN_EPS)

    def forward(self, y):
        y = y + self.patch_mixer(self.norm1(y))
        y = y.transpose(-1, -2)
        y = y + self.hidden_mixer(self.norm2(y))
        return y.transpose(-1, -2)


class Mixer2d(nn.Module):
    """mixer_mlp.py:40-86; ``img_size = (channels, H, W)``"""

    def __init__(self, img_size, patch_size: int, hidden_size: int, mix_patch_size: int, mix_hidden_size: int, num_blocks: int,
                 act: Callable = nn.functional.relu):
        super().__init__()
        input_size, height, width = (int(v) for v in img_size)
        if height % patch_size or width % patch_size:
            raise ValueError(f"patch_size {patch_size} does not divide the image {height} x {width}")
        num_patches = (height // patch_size) * (width // patch_size)
        self.img_size, self.patch_size, self.num_patches = (input_size, height, width), int(patch_size), num_patches
        self.conv_in = nn.Conv2d(input_size, hidden_size, patch_size, stride=patch_size)
        self.conv_out = nn.ConvTranspose2d(hidden_size, input_size, patch_size, stride=patch_size)
        self.blocks = nn.ModuleList([MixerBlock(num_patches, hidden_size, mix_patch_size, mix_hidden_size, act)
                                     for _ in range(num_blocks)])
        self.norm = nn.LayerNorm((hidden_size, num_patches), eps=LN_EPS)

    def forward(self, x):
        single = x.dim() == 2
        y = x[None, None] if single else x
        y = self.conv_in(y)
        B, C, h, w = y.shape
        y = y.reshape(B, C, h * w)
        for block in self.blocks:
            y = block(y)
        y = self.conv_out(self.norm(y).reshape(B, C, h, w))
        return y[0, 0] if single else y


# ---- the family the library's own kernels cover (csrc/mixer.hip) -------------------------------------------------------

NATIVE_ACTIVATIONS = ("gelu", "gelu_tanh", "tanh", "relu")  # index = pdeopt_mixer_activation
NATIVE_MAX_PATCH, NATIVE_MAX_HIDDEN, NATIVE_MAX_MIX, NATIVE_MAX_PATCHES, NATIVE_MAX_BLOCKS = 16, 64, 256, 4096, 8


def _activation_name(act) -> Optional[str]:
    F = nn.functional
    if act is F.relu or act is torch.relu or isinstance(act, nn.ReLU):
        return "relu"
    return _cnn_activation_name(act)


def _plain_mlp(mlp, n_in):
    """``(width, None)`` when ``mlp`` is ``Linear(n_in, width) -> act -> Linear(width, n_in)`` with biases, else ``(None, reason)``"""
    if type(mlp) is not MLP:
        return None, f"a {type(mlp).__name__} is not a plain MLP"
    layers = list(mlp.layers)
    if len(layers) != 2 or any(type(l) is not nn.Linear for l in layers):
        return None, "an MLP is not two Linear layers"
    if any(l.bias is None for l in layers):
        return None, "a Linear layer has no bias"
    width = layers[0].out_features
    if (layers[0].in_features, layers[1].in_features, layers[1].out_features) != (n_in, width, n_in):
        return None, "an MLP's layer sizes do not chain"
    return width, None


def _plain_norm(norm, shape):
    if type(norm) is not nn.LayerNorm or tuple(norm.normalized_shape) != tuple(shape):
        return f"a layer norm is not a LayerNorm over {tuple(shape)}"
    if norm.weight is None or norm.bias is None or norm.eps != LN_EPS:
        return f"a layer norm lacks its weight or bias, or its eps is not {LN_EPS}"
    return None


def _inspect(module):
    """``(spec, None)`` or ``(None, reason)``"""
    if not isinstance(module, Mixer2d):
        return None, f"a {type(module).__name__} is not a Mixer2d"
    if type(module).forward is not Mixer2d.forward:
        return None, f"{type(module).__name__} overrides Mixer2d.forward"
    cin, cout = module.conv_in, module.conv_out
    if type(cin) is not nn.Conv2d or type(cout) is not nn.ConvTranspose2d:
        return None, "conv_in is not a Conv2d or conv_out is not a ConvTranspose2d"
    channels, H, W = module.img_size
    if (cin.in_channels, cout.out_channels, channels) != (1, 1, 1):
        return None, f"in_channels = {cin.in_channels}, out_channels = {cout.out_channels}: supported is one channel in, one out"
    p, C = module.patch_size, cin.out_channels
    for conv in (cin, cout):
        if (tuple(conv.kernel_size), tuple(conv.stride), tuple(conv.padding), tuple(conv.dilation), conv.groups) != ((p, p), (p, p), (0, 0), (1, 1), 1):
            return None, f"a patch convolution is not {p} x {p} of stride {p} without padding, dilation or groups"
        if conv.bias is None:
            return None, "a patch convolution has no bias"
    if tuple(cout.output_padding) != (0, 0) or cout.in_channels != C:
        return None, "conv_out does not mirror conv_in"
    if not 1 <= p <= NATIVE_MAX_PATCH:
        return None, f"patch_size {p}: supported are 1 to {NATIVE_MAX_PATCH}"
    if H % p or W % p:
        return None, f"patch_size {p} does not divide the grid {H} x {W}"
    P = (H // p) * (W // p)
    if not 1 <= C <= NATIVE_MAX_HIDDEN:
        return None, f"hidden_size {C}: supported are 1 to {NATIVE_MAX_HIDDEN}"
    if not 1 <= P <= NATIVE_MAX_PATCHES:
        return None, f"{P} patches: supported are 1 to {NATIVE_MAX_PATCHES}"
    blocks = list(module.blocks)
    if not 1 <= len(blocks) <= NATIVE_MAX_BLOCKS:
        return None, f"{len(blocks)} blocks: supported are 1 to {NATIVE_MAX_BLOCKS}"
    sizes, acts = set(), set()
    for blk in blocks:
        if type(blk) is not MixerBlock:
            return None, f"block {type(blk).__name__} is not a plain MixerBlock"
        (mp, why_p), (mh, why_h) = _plain_mlp(blk.patch_mixer, P), _plain_mlp(blk.hidden_mixer, C)
        why = why_p or why_h or _plain_norm(blk.norm1, (C, P)) or _plain_norm(blk.norm2, (P, C))
        if why:
            return None, why
        sizes.add((mp, mh))
        for mlp in (blk.patch_mixer, blk.hidden_mixer):
            name = _activation_name(mlp.activation)
            if name is None:
                return None, f"activation {mlp.activation!r} is not one of relu, gelu (erf or tanh form) and tanh"
            acts.add(name)
    if len(sizes) != 1:
        return None, f"the blocks use different mix sizes {sorted(sizes)}"
    if len(acts) != 1:
        return None, f"the MLPs use different activations {sorted(acts)}"
    mp, mh = next(iter(sizes))
    if not (1 <= mp <= NATIVE_MAX_MIX and 1 <= mh <= NATIVE_MAX_MIX):
        return None, f"mix sizes {mp} and {mh}: supported are 1 to {NATIVE_MAX_MIX}"
    why = _plain_norm(module.norm, (C, P))
    if why:
        return None, why
    return ((H, W), p, C, mp, mh, len(blocks), next(iter(acts))), None


def native_spec(module):
    """``((H, W), patch_size, hidden_size, mix_patch_size, mix_hidden_size, num_blocks, activation)`` -- the activation a
    name of ``NATIVE_ACTIVATIONS`` -- when ``module`` is exactly a ``Mixer2d`` of the family csrc/mixer.hip evaluates; None
    otherwise (``native_refusal`` says why)"""
    return _inspect(module)[0]


def native_refusal(module) -> Optional[str]:
    """why ``native_spec(module)`` is None, or None"""
    return _inspect(module)[1]


def n_params(grid, patch_size, hidden_size, mix_patch_size, mix_hidden_size, num_blocks) -> int:
    """the length of the flat parameter vector"""
    p, C, mp, mh = patch_size, hidden_size, mix_patch_size, mix_hidden_size
    P = (grid[0] // p) * (grid[1] // p)
    block = (mp * P + mp + P * mp + P) + (mh * C + mh + C * mh + C) + 4 * C * P
    return 2 * C * p * p + C + 1 + num_blocks * block + 2 * C * P


def pack_linear(weight, backward: bool = False, stored_io: bool = False) -> np.ndarray:
    """The layout csrc/mixer.hip reads the weight of a map from ``I`` inputs to ``O`` outputs in, given as torch stores a
    ``Linear``'s, ``(O, I)`` (``stored_io``: as ``(I, O)``, which is how a ``ConvTranspose2d`` weight ``(C, 1, p, p)`` reads
    as the map from ``C`` channels to ``p p`` pixels): ``(pad16(I), pad16(O))`` with ``packed[i, o] = W[o, i]`` and zeros
    in the padding -- the right-hand operand of ``x @ W^T``.  ``backward``: the backward-data product's,
    ``(pad16(O), pad16(I))`` with ``packed[o, i] = W[o, i]``."""
    w = np.asarray(weight)
    if w.ndim != 2:
        raise ValueError(f"weight of shape {w.shape}: expected two axes")
    w = w.T if stored_io else w
    O, I = w.shape
    pad = lambda c: -(-c // 16) * 16
    out = np.zeros((pad(O), pad(I)) if backward else (pad(I), pad(O)), dtype=w.dtype)
    if backward:
        out[:O, :I] = w
    else:
        out[:I, :O] = w.T
    return out


def patch_matrix(field, patch_size: int) -> np.ndarray:
    """a field ``(H, W)`` as the kernels read and write it: ``(P, p p)`` with row ``(H-block, W-block)`` row-major over the
    patch grid and column ``(row, column)`` inside the patch"""
    a = np.asarray(field)
    H, W = a.shape
    p = int(patch_size)
    return a.reshape(H // p, p, W // p, p).transpose(0, 2, 1, 3).reshape((H // p) * (W // p), p * p)
