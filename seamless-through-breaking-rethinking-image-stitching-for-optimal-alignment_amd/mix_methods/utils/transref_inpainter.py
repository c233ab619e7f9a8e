"""`transref_inpainter` (reference: core/inference/mix_methods/utils/transref_inpainter.py, TransRef/models/TransRef.py): the TransRef
inpainting network on the GPU (`stitch_amd.transref`).  As in the reference, importing this module builds `inpainter` from
`TransRef/400_Trans.pth` next to this file (`{'net': state_dict}`, loaded strict=False; missing / unexpected key counts reported).
Without that file the import raises `transref.CheckpointMissing` (an ImportError): `out.load_inpainter` then keeps its pass-through
stand-in.  `Inpainter(state_dict=None, seed=None, device=...)` builds one from any state dict or from seeded weights."""
from __future__ import annotations

import os

from ...transref import CheckpointMissing, Inpainter, load_checkpoint

CHECKPOINT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "TransRef", "400_Trans.pth")

__all__ = ["CHECKPOINT", "Inpainter", "inpainter"]

if not os.path.exists(CHECKPOINT):
    raise CheckpointMissing(f"transref_inpainter: no checkpoint at {CHECKPOINT} (the reference's 400_Trans.pth, format "
                            f"{{'net': state_dict}}); build an Inpainter(state_dict=..., seed=...) from stitch_amd.transref instead")
_sd, _missing, _unexpected = load_checkpoint(CHECKPOINT)
print(f"[transref_inpainter] loaded {CHECKPOINT}: {len(_missing)} missing, {len(_unexpected)} unexpected keys")
inpainter = Inpainter(state_dict=_sd)
