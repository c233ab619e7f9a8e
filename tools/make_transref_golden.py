"""Golden vectors of the TransRef inpainter from the REFERENCE's own code (build container only; writes tests/golden/transref_*.{json,npz}).

    python tools/make_transref_golden.py

Imports the reference's TransRef/models/TransRef.py, base_networks.py and RefPA/*.py by path, with third-party stand-ins:
oracle.ref_harness.stubs.install() (timm; imported, not edited) and, local to this tool, torchvision.transforms.ToTensor /
Normalize / Compose, util.util, models.loss, models.base_model and mmcv's DeformConv2d (tests/_deform_ref.py, unpinned).  The
weights are stitch_amd.transref.seeded_state_dict(SEED), loaded strict into TransRef_Base.

The wrapper runs through the reference's own TransRef.set_input / forward on a TransRef object whose constructor is bypassed (it
builds VGG16 and moves everything to CUDA), and through Inpainter.inpaint of transref_inpainter.py, executed from the reference file
without its module-level ``inpainter = Inpainter()`` line and its relative sys.path edits (the checkpoint load and the device moves
are what those lines do); the Inpainter object is made without __init__ and given the model, the transforms and device "cpu".

Two runs: the reference as is (fp32), and the same wrapper with the network in float64 (input cast up, output float64, so the
final blend, resize and rounding run in float64 too).  Stored (inputs at a non-512 origin size, thin-border mask as mix_fn makes it):
the network output of the fp64 run on a stride-8 grid (float32), the fp32 run's spread against it (max and p99 over the whole
512 x 512 x 3 output), the Tenc stage-4 and Tdec outputs (fp64 run), the wrapper's uint8 result of both runs and the output bytes whose fp64 value before rounding lies within NEAR of a .5 boundary
(flat index into [3, H, W] and that distance).
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 2024
ORIGIN_HW = (172, 150)
GRID = 8
NEAR = 0.01                                         # bytes whose fp64 value lies this close to a .5 boundary are listed


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _ToTensor:
    """torchvision ToTensor on a PIL uint8 RGB image: HWC -> CHW, float32 / 255."""

    def __call__(self, pic):
        a = torch.from_numpy(np.array(pic, dtype=np.uint8, copy=True))
        return a.permute(2, 0, 1).contiguous().to(torch.float32).div(255)


class _Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, t):
        mean = torch.as_tensor(self.mean, dtype=t.dtype).view(-1, 1, 1)
        std = torch.as_tensor(self.std, dtype=t.dtype).view(-1, 1, 1)
        return t.sub(mean).div(std)


class _Compose:
    def __init__(self, ts):
        self.ts = ts

    def __call__(self, x):
        for t in self.ts:
            x = t(x)
        return x


def _install():
    from oracle.ref_harness import stubs
    import _deform_ref
    stubs.install()
    import PIL.Image  # noqa: F401  (the wrapper calls PIL.Image.fromarray after a bare `import PIL`)
    tr_dir = os.path.join(stubs.REF_ROOT, "core", "inference", "mix_methods", "utils", "TransRef")
    if tr_dir not in sys.path:
        sys.path.insert(0, tr_dir)
    tv = sys.modules["torchvision"]
    tv.transforms.ToTensor, tv.transforms.Normalize, tv.transforms.Compose = _ToTensor, _Normalize, _Compose
    _mod("util")
    _mod("util.util", showpatch=lambda *a, **k: None)
    _mod("models.loss", VGG16=nn.Module, PerceptualLoss=nn.Module, StyleLoss=nn.Module)
    _mod("models.base_model", BaseModel=object)
    _mod("mmcv")
    _mod("mmcv.ops")
    _mod("mmcv.ops.deform_conv", DeformConv2d=_deform_ref.DeformConv2d)
    return tr_dir


def build_reference():
    """TransRef_Base from the reference's own module (CPU, float32, eval)."""
    _install()
    from models.TransRef import TransRef_Base
    return TransRef_Base().eval()


def reference_wrapper(net):
    """(Inpainter object of transref_inpainter.py, TransRef object of TransRef.py) around ``net`` on the CPU."""
    tr_dir = _install()
    from models.TransRef import TransRef
    path = os.path.join(os.path.dirname(tr_dir), "transref_inpainter.py")
    src = open(path).read()
    keep = [l for l in src.splitlines() if not l.startswith("sys.path.") and l.strip() != "inpainter = Inpainter()"]
    ns = {"__name__": "ref_transref_inpainter", "__file__": path}
    exec(compile("\n".join(keep), path, "exec"), ns)
    model = TransRef.__new__(TransRef)
    model.device = torch.device("cpu")
    model.model = net
    inp = ns["Inpainter"].__new__(ns["Inpainter"])
    inp.name, inp.device, inp.model = "transref_inpainter", "cpu", model
    inp.img_transform = _Compose([_ToTensor(), _Normalize((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))])
    return inp, model


class _Float64(nn.Module):
    """the network in float64 behind the reference's float32 wrapper"""

    def __init__(self, net):
        super().__init__()
        self.net = net.double()

    def forward(self, x, ref):
        return self.net(x.double(), ref.double())


def synthetic_inputs(h, w, seed=5):
    """init / control uint8-valued images [1,3,h,w] (smooth texture + noise) and a thin-border 3-plane mask [1,3,h,w]."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    base = torch.stack([120 + 80 * torch.sin(6 * xx + 2 * yy), 100 + 70 * torch.cos(5 * yy - 3 * xx), 90 + 60 * torch.sin(9 * xx * yy)])
    init = (base + 12 * torch.rand((3, h, w), generator=g)).clamp(0, 255).floor()
    ctl = (base.flip(2) + 12 * torch.rand((3, h, w), generator=g)).clamp(0, 255).floor()
    # border band of irregular width (2..9 px) on every side, as dilate_thin_area leaves it around a warped canvas
    band = torch.zeros((h, w), dtype=torch.bool)
    top = 2 + (7 * torch.rand(w, generator=g)).long()
    left = 2 + (7 * torch.rand(h, generator=g)).long()
    for j in range(w):
        band[: top[j], j] = True
        band[h - top[(j * 7) % w]:, j] = True
    for i in range(h):
        band[i, : left[i]] = True
        band[i, w - left[(i * 5) % h]:] = True
    mask = band.to(torch.float32).expand(3, h, w).clone()
    return init[None], ctl[None], mask[None]


def run_reference(net32, init, ctl, mask):
    """wrapper result uint8, the network output and the pre-rounding float value of the reference run around ``net32``."""
    inp, model = reference_wrapper(net32)
    captured = {}
    h = model.model.register_forward_hook(lambda m, a, o: captured.__setitem__("out", o.detach().clone()))
    hooks = [h]
    tenc = getattr(model.model, "net", model.model).Tenc
    tdec = getattr(model.model, "net", model.model).Tdec
    hooks.append(tenc.register_forward_hook(lambda m, a, o: captured.__setitem__("tenc4", o[3].detach().clone())))
    hooks.append(tdec.register_forward_hook(lambda m, a, o: captured.__setitem__("tdec", o[0].detach().clone())))
    orig_round = torch.Tensor.round

    def spy_round(t, *a, **k):
        captured["pre_round"] = t.detach().clone()
        return orig_round(t, *a, **k)

    torch.Tensor.round = spy_round
    try:
        with torch.no_grad():
            out = inp.inpaint(init, mask, control_image_tensor=ctl)
    finally:
        torch.Tensor.round = orig_round
        for h in hooks:
            h.remove()
    return out, captured


def main():
    import stitch_amd.transref as tr
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = tr.seeded_state_dict(SEED)
    net = build_reference()
    net.load_state_dict(sd, strict=True)
    keys = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    with open(os.path.join(GOLDEN, "transref_state_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    init, ctl, mask = synthetic_inputs(*ORIGIN_HW)
    u8_32, c32 = run_reference(net, init, ctl, mask)
    net64 = build_reference()
    net64.load_state_dict(sd, strict=True)
    u8_64, c64 = run_reference(_Float64(net64), init, ctl, mask)
    o32, o64 = c32["out"].double(), c64["out"]
    d = (o32 - o64).abs().flatten()
    spread_max, spread_p99 = float(d.max()), float(torch.quantile(d[:: 7], 0.99))
    pre = c64["pre_round"][0]
    dist = (pre - torch.floor(pre) - 0.5).abs()
    np.savez_compressed(
        os.path.join(GOLDEN, "transref_512.npz"),
        seed=np.int64(SEED), grid=np.int64(GRID),
        init=init[0].numpy().astype(np.uint8), control=ctl[0].numpy().astype(np.uint8), mask=mask[0, 0].numpy().astype(np.uint8),
        net_out64=o64[0, :, GRID // 2::GRID, GRID // 2::GRID].float().numpy(),
        spread_max=np.float64(spread_max), spread_p99=np.float64(spread_p99),
        tenc4=c64["tenc4"][0].float().numpy(), tdec=c64["tdec"][0].float().numpy(),
        u8_64=u8_64[0].numpy(), u8_32=u8_32[0].numpy(), near_half_idx=np.flatnonzero(dist.numpy() < NEAR).astype(np.int32),
        near_half_dist=dist.numpy().ravel()[dist.numpy().ravel() < NEAR].astype(np.float32))
    print(f"keys {len(keys)}, elements {sum(int(np.prod(s)) for _, s in keys)}; fp32 spread max {spread_max:.3e} p99 {spread_p99:.3e}; "
          f"u8 fp32 vs fp64 differ at {int((u8_32 != u8_64).sum())} bytes; out range [{float(o64.min()):.3f}, {float(o64.max()):.3f}]")


if __name__ == "__main__":
    main()
