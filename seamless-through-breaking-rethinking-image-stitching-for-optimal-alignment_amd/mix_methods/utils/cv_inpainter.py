"""`cv_inpainter` (reference: core/inference/mix_methods/utils/cv_inpainter.py, `inpaint_cv`: OpenCV's Telea fast-marching
inpainting, cv2.inpaint(img, mask, 64, cv2.INPAINT_TELEA), no weights) on the GPU: the same preprocessing and result type, the
fill itself is `ops.inpaint_telea`, Telea 2004 restated ring by ring (README.md, "cv_inpainter").  Not pinned against OpenCV:
its sequential heap order is not reproduced.  Selected by `TPS_PIPELINE_CONFIG.inpainter = "cv_inpainter"`
(inf_configs/*_cv.py)."""
from __future__ import annotations

import torch

from ... import ops


class Inpainter:
    def __init__(self, radius=64):
        self.name = "cv_inpainter"
        self.radius = radius

    @torch.no_grad()
    def inpaint(self, init_image_tensor, mask_image_tensor, control_image_tensor=None, prompt="", resize_to_area_limit_before_inpaint=False):
        """init [B,3,H,W], mask [B,1 or 3,H,W] -> uint8 [1,3,H,W] on the input's device.  Batch element 0 only (B > 1 raises).
        The image is clamped to 0..255 and truncated (to(torch.uint8)); the mask repeated to 3 channels, x255 + clamped when
        its max is <= 1.1, truncated and reduced with PIL's integer luma: nonzero = fill.  `control_image_tensor` and
        `resize_to_area_limit_before_inpaint` are ignored, as in the reference."""
        img, mask = init_image_tensor, mask_image_tensor
        if img.dim() != 4 or img.shape[1] != 3 or mask.dim() != 4 or mask.shape[1] not in (1, 3) or mask.shape[2:] != img.shape[2:]:
            raise ValueError(f"[B,3,H,W] image and [B,1|3,H,W] mask expected, got {tuple(img.shape)} and {tuple(mask.shape)}")
        if img.shape[0] != 1 or mask.shape[0] != 1:
            raise ValueError(f"cv_inpainter handles one image (batch element 0), got batches {img.shape[0]} and {mask.shape[0]}")
        dev = img.device
        img3 = img[0].to(device="cuda" if dev.type == "cpu" else dev, dtype=torch.float32).contiguous()
        mask3 = mask[0].to(device=img3.device, dtype=torch.float32).contiguous()
        img_hwc, mask_u8 = ops.inpaint_prep(img3, mask3)
        out = ops.inpaint_telea(img_hwc, mask_u8, self.radius)
        return out.permute(2, 0, 1).unsqueeze(0).contiguous().to(dev)


inpainter = Inpainter()
