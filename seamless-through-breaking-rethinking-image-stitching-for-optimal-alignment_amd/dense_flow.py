"""Weight-free residual flow: the dense displacement FlowFormer++ predicts after the homography, computed from the pixels themselves --
a coarse-to-fine, zero-mean Lucas-Kanade on integer pyramids (``ops.dense_flow``; README.md, dense_flow).

    lk = stitch_amd.DenseFlow()
    flow = lk.flow(a, warp2, mask2=warp_mask)          # fp32 [B,2,H,W], 1 -> 2: what FlowHomoAdpater.predict_flow returns

``cfg.flow_source = "dense_lk"`` makes the model use it in place of the network (configs/last_config_classical.py).  Where a window has
too few valid pixels, or no texture, the pixel keeps what the coarser levels and the median gave it, decided on the device: the host
learns nothing and the launch sequence never changes, so the call captures into a hipGraph like the network it stands in for.  It sees
only what the coarsest level can see: a residual of a few pixels per level, not large parallax (README.md)."""
from __future__ import annotations

import torch

from . import ops


class DenseFlow:
    def __init__(self, levels=ops.DENSE_FLOW_DEFAULTS["levels"], iters=ops.DENSE_FLOW_DEFAULTS["iters"], radius=ops.DENSE_FLOW_DEFAULTS["radius"],
                 damping=ops.DENSE_FLOW_DEFAULTS["damping"]):
        self.levels, self.iters, self.radius, self.damping = int(levels), int(iters), int(radius), int(damping)
        self._ws = {}              # (device, stream, B, H, W) -> workspace of the eager calls
        self.last_support = None   # uint8 [B,1,H,W] of the latest call, on the device (ops.dense_flow)

    def workspace(self, dev, B, H, W):
        """this object's workspace for a shape on the current stream of ``dev`` (calls on several streams must not share one).  While a
        hipGraph is being captured the workspace is allocated from that graph's own pool instead: every capture runs on the same capture
        stream, and graphs captured from one model replay side by side on several streams (evaluate.EvalPipeline's slots)."""
        nbytes = ops.dense_flow_workspace_bytes(B, H, W, self.levels)
        if torch.cuda.is_current_stream_capturing():
            return torch.empty(nbytes, dtype=torch.uint8, device=dev)
        key = (str(dev), torch.cuda.current_stream(dev).cuda_stream, B, H, W)
        if key not in self._ws:
            self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return self._ws[key]

    def flow_and_support(self, image1, image2, mask1=None, mask2=None):
        """(flow [B,2,H,W], support [B,1,H,W]) of ``ops.dense_flow`` with this object's parameters and workspace"""
        image1, image2 = image1.float().contiguous(), image2.float().contiguous()
        B, _, H, W = image1.shape
        out = ops.dense_flow(image1, image2, mask1, mask2, levels=self.levels, iters=self.iters, radius=self.radius, damping=self.damping,
                             workspace=self.workspace(image1.device, B, H, W))
        self.last_support = out[1]
        return out

    def flow(self, image1, image2, mask1=None, mask2=None):
        return self.flow_and_support(image1, image2, mask1, mask2)[0]

    def flow_pair(self, image1, image2, mask2):
        """(flow 1 -> 2, flow 2 -> 1) from one batch of 2B: ``mask2`` is image 2's validity in both directions"""
        B = image1.shape[0]
        image1, image2, mask2 = image1.float(), image2.float(), mask2.float()
        if mask2.shape[1] != 1:
            mask2 = mask2[:, 0:1]
        ones = torch.ones_like(mask2)
        both = self.flow(torch.cat([image1, image2]), torch.cat([image2, image1]), torch.cat([ones, mask2]), torch.cat([mask2, ones]))
        return both[:B], both[B:]
