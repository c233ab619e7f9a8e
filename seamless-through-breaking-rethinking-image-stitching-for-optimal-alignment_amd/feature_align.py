"""Weight-free alignment: the four corner offsets the homography network regresses, computed from the pixels themselves -- Harris
corners, upright BRIEF-256, mutual nearest neighbours, RANSAC (``ops.feature_homography``; README.md, feature_align).

    aligner = stitch_amd.FeatureAligner()
    motion = aligner.motion(a, b)          # fp32 [B,4,2]: what FlowHomoAdpater.predict_homo returns

``cfg.homo_source = "features"`` makes the model use it in place of the network (configs/last_config_features.py).  A pair without a
valid model -- too few keypoints, matches or inliers -- gets zero motion, i.e. the identity, decided on the device: the host learns
nothing and the launch sequence never changes, so the call captures into a hipGraph like the network it stands in for.  The descriptor
is upright and single-scale: it is not invariant to rotation or scale beyond what the tests measure (README.md).
``FeatureAligner(multiscale=True)`` (``cfg.feature_align = dict(multiscale=True)``, configs/last_config_classical_ms.py) takes the
oriented, multi-scale front end instead (``ops.feature_homography_ms``; README.md, feature_align_ms): quarter turns, any roll and about
one octave of zoom, at several times the cost."""
from __future__ import annotations

import torch

from . import ops


class FeatureAligner:
    def __init__(self, max_hyp=2048, thr=3.0, min_inliers=12, seed=1, multiscale=False, levels=6, oriented=True):
        self.max_hyp, self.thr, self.min_inliers, self.seed = int(max_hyp), float(thr), int(min_inliers), int(seed)
        self.multiscale, self.levels, self.oriented = bool(multiscale), int(levels), bool(oriented)
        self._ws = {}              # (device, stream, B, H, W) -> workspace of the eager calls
        self.last_info = None      # int32 [B,8] of the latest call, on the device (ops.feature_homography)

    def workspace(self, dev, B, H, W):
        """this object's workspace for a shape on the current stream of ``dev`` (calls on several streams must not share one).  While a
        hipGraph is being captured the workspace is allocated from that graph's own pool instead: every capture runs on the same capture
        stream, and graphs captured from one model replay side by side on several streams (evaluate.EvalPipeline's slots)."""
        if self.multiscale:
            nbytes = ops.feature_ms_workspace_bytes(B, H, W, self.levels, self.max_hyp)
        else:
            nbytes = ops.feature_workspace_bytes(B, H, W, self.max_hyp)
        if torch.cuda.is_current_stream_capturing():
            return torch.empty(nbytes, dtype=torch.uint8, device=dev)
        key = (str(dev), torch.cuda.current_stream(dev).cuda_stream, B, H, W)
        if key not in self._ws:
            self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return self._ws[key]

    def homography(self, image1, image2):
        """(motion [B,4,2], H [B,3,3], info [B,8]) of ``ops.feature_homography`` (``ops.feature_homography_ms`` with ``multiscale``) with this
        object's parameters and workspace"""
        image1, image2 = image1.float().contiguous(), image2.float().contiguous()
        B, _, H, W = image1.shape
        kw = dict(max_hyp=self.max_hyp, thr=self.thr, min_inliers=self.min_inliers, seed=self.seed, workspace=self.workspace(image1.device, B, H, W))
        if self.multiscale:
            out = ops.feature_homography_ms(image1, image2, levels=self.levels, oriented=self.oriented, **kw)
        else:
            out = ops.feature_homography(image1, image2, **kw)
        self.last_info = out[2]
        return out

    def motion(self, image1, image2):
        return self.homography(image1, image2)[0]
