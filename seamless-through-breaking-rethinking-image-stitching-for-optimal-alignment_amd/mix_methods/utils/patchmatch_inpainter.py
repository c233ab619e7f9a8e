"""`patchmatch_inpainter`: exemplar-based hole filling on the GPU, no weights -- PatchMatch (Barnes et al. 2009) inside the coarse-to-fine
vote / search loop of Wexler et al. 2007 (README.md, "patchmatch_inpainter").  No counterpart in the reference and pinned against no
library: the contract is this project's own (tests/_patchmatch_ref.py).  The protocol, the preprocessing and the result type are
`cv_inpainter`'s; the fill itself is `ops.inpaint_patchmatch`, which copies image content into the hole where Telea diffuses the border
colours.  Selected by `TPS_PIPELINE_CONFIG.inpainter = "patchmatch_inpainter"` (inf_configs/*_pm.py)."""
from __future__ import annotations

import torch

from ... import ops


class Inpainter:
    def __init__(self, levels=None, iters=4, seed=1):
        self.name = "patchmatch_inpainter"
        self.levels, self.iters, self.seed = levels, iters, seed

    @torch.no_grad()
    def inpaint(self, init_image_tensor, mask_image_tensor, control_image_tensor=None, prompt="", resize_to_area_limit_before_inpaint=False):
        """init [B,3,H,W], mask [B,1 or 3,H,W] -> uint8 [1,3,H,W] on the input's device.  Batch element 0 only (B > 1 raises).
        The preprocessing is `cv_inpainter`'s (`ops.inpaint_prep`): nonzero mask = fill.  `control_image_tensor` and
        `resize_to_area_limit_before_inpaint` are ignored.  Nothing is read back: where there is nothing to fill, or no hole-free 7x7
        patch to fill it from, the image comes back as it is."""
        img, mask = init_image_tensor, mask_image_tensor
        if img.dim() != 4 or img.shape[1] != 3 or mask.dim() != 4 or mask.shape[1] not in (1, 3) or mask.shape[2:] != img.shape[2:]:
            raise ValueError(f"[B,3,H,W] image and [B,1|3,H,W] mask expected, got {tuple(img.shape)} and {tuple(mask.shape)}")
        if img.shape[0] != 1 or mask.shape[0] != 1:
            raise ValueError(f"patchmatch_inpainter handles one image (batch element 0), got batches {img.shape[0]} and {mask.shape[0]}")
        dev = img.device
        img3 = img[0].to(device="cuda" if dev.type == "cpu" else dev, dtype=torch.float32).contiguous()
        mask3 = mask[0].to(device=img3.device, dtype=torch.float32).contiguous()
        img_hwc, mask_u8 = ops.inpaint_prep(img3, mask3)
        out, _ = ops.inpaint_patchmatch(img_hwc, mask_u8, levels=self.levels, iters=self.iters, seed=self.seed)
        return out.permute(2, 0, 1).unsqueeze(0).contiguous().to(dev)


inpainter = Inpainter()
