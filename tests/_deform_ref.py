"""mmcv ``DeformConv2d`` restated from its published algorithm (mmcv/ops/csrc/common/*deform_conv*: deformable_im2col_bilinear),
for 3x3 kernels, stride 1, one deformable group, no bias -- the only form TransRef uses (RefPA/PA.py).  Unpinned: mmcv cannot be
installed here.  Offset channel 2k is dy and 2k + 1 is dx of tap k = 3 ky + kx; the sample point of output (oy, ox) is
(oy - pad + ky + dy, ox - pad + kx + dx).  Outside (h <= -1, h >= H, w <= -1 or w >= W) the sample is 0; inside it is bilinear and
every corner outside the image reads 0.  Runs in the dtype of its inputs (float64 for goldens and tests)."""
from __future__ import annotations

import torch
import torch.nn as nn


def deform_im2col(x, offset, pad=1):
    """x [B,C,H,W], offset [B,18,H,W] -> cols [B, 9, C, H, W] (the bilinear samples of every tap)."""
    B, C, H, W = x.shape
    dt = x.dtype
    oy = torch.arange(H, dtype=dt).view(1, H, 1)
    ox = torch.arange(W, dtype=dt).view(1, 1, W)
    cols = []
    flat = x.reshape(B, C, H * W)
    for k in range(9):
        ky, kx = divmod(k, 3)
        h = (oy - pad + ky) + offset[:, 2 * k]
        w = (ox - pad + kx) + offset[:, 2 * k + 1]
        inside = (h > -1) & (w > -1) & (h < H) & (w < W)
        hl, wl = torch.floor(h), torch.floor(w)
        lh, lw = h - hl, w - wl
        hh, hw = 1 - lh, 1 - lw
        hl, wl = hl.long(), wl.long()
        val = torch.zeros((B, C, H, W), dtype=dt)
        for dy, dx, wgt in ((0, 0, hh * hw), (0, 1, hh * lw), (1, 0, lh * hw), (1, 1, lh * lw)):
            yy, xx = hl + dy, wl + dx
            ok = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
            idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).view(B, 1, H * W).expand(B, C, H * W)
            v = torch.gather(flat, 2, idx).view(B, C, H, W)
            val = val + torch.where(ok.unsqueeze(1), wgt.unsqueeze(1) * v, torch.zeros((), dtype=dt))
        cols.append(val)
    return torch.stack(cols, 1)


def deform_conv2d(x, offset, weight, pad=1):
    """x [B,C,H,W], offset [B,18,H,W], weight [Cout, C, 3, 3] -> [B, Cout, H, W]."""
    cols = deform_im2col(x, offset, pad)
    w = weight.reshape(weight.shape[0], weight.shape[1], 9)
    return torch.einsum("bkchw,ock->bohw", cols, w)


class DeformConv2d(nn.Module):
    """Stand-in for ``mmcv.ops.deform_conv.DeformConv2d`` with the reference's construction arguments (same parameter names)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, dilation=1, groups=1, deform_groups=1, bias=False):
        super().__init__()
        assert kernel_size == 3 and stride == 1 and dilation == 1 and groups == 1 and deform_groups == 1 and not bias
        self.padding = padding
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 3, 3))
        nn.init.kaiming_uniform_(self.weight)

    def forward(self, x, offset):
        return deform_conv2d(x, offset.to(x.dtype), self.weight.to(x.dtype), self.padding)
