"""A periodic CNN as a closure (the reference's pde_opt/numerics/functions/cnn.py:13-102), as a ``torch.nn.Module``.

``PeriodicCNN(in_channels, hidden_channels, out_channels, kernel_size, act)`` keeps the reference's constructor
arguments: a stack of ``Conv2d -> act`` blocks and a final ``Conv2d`` without activation, all with circular "same"
padding and stride 1, so the map is translation-equivariant on the torus.  It is not pointwise: as ``mu`` of
``CahnHilliard2DPeriodic`` it runs in torch on the GPU next to the HIP kernels, which see the field it returns
(``pde_opt_amd.fieldmu``).  Input ``(B, C, H, W)`` or ``(C, H, W)``; the output has the same spatial size.

Importing this module imports torch (the package itself does not)."""

from __future__ import annotations

from typing import Callable, Optional, Sequence

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
