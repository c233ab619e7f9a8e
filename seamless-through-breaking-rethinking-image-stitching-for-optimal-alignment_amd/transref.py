"""TransRef inpainting network (reference: core/inference/mix_methods/utils/TransRef/models/TransRef.py ``TransRef_Base``,
base_networks.py, RefPA/*.py) on the HIP kernels, at its fixed 512 x 512 input.

``transref_spec()`` enumerates the reference's state-dict surface (565 tensors, 45.1 M elements, BN running statistics and the
modules the forward never reaches -- ``mini_patch_embed4{,_ref}``, ``convtail.conv_output`` -- included), ``TransRefModule`` holds it
as a ``ParamTree`` so a ``400_Trans.pth`` drops in, ``seeded_state_dict`` makes deterministic stand-in weights and ``pack`` re-lays
them for the kernels.  ``TransRefNet.forward(x6, ref3)`` is one fixed launch sequence without host synchronisation on channels-last
device tensors: implicit-GEMM convolutions and Linears (``ops.conv_gemm``), LayerNorm, max-pool, flash attention
(``ops.tr_attention``: every Block, Block_Ref, Block_dec and non-local block), mmcv's DeformConv2d as a bilinear im2col plus a GEMM,
transposed convolutions as four output-phase GEMMs plus an interleave, depthwise 3x3 + GELU.  There is no CPU path.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import torch

from . import ops
from .checkpoint import ParamTree

EMBED = (64, 128, 320, 512)
HEADS = (1, 2, 4, 4)
SR = (4, 2, 2, 1)
SIZE = 512


def _lin(d, n, cin, cout, bias=True):
    d[n + ".weight"] = (cout, cin)
    if bias:
        d[n + ".bias"] = (cout,)


def _conv(d, n, cin, cout, k, bias=True, groups=1):
    d[n + ".weight"] = (cout, cin // groups, k, k)
    if bias:
        d[n + ".bias"] = (cout,)


def _convT(d, n, cin, cout, k):
    d[n + ".weight"] = (cin, cout, k, k)
    d[n + ".bias"] = (cout,)


def _ln(d, n, c):
    d[n + ".weight"] = (c,)
    d[n + ".bias"] = (c,)


def _bn(d, n, c):
    _ln(d, n, c)
    d[n + ".running_mean"] = (c,)
    d[n + ".running_var"] = (c,)
    d[n + ".num_batches_tracked"] = ()


def _pe(d, n, cin, cout, k):
    _conv(d, n + ".proj", cin, cout, k)
    _ln(d, n + ".norm", cout)


def _attn(d, n, dim, sr, ref=False):
    _lin(d, n + ".q", dim, dim)
    _lin(d, n + ".kv", dim, 2 * dim)
    _lin(d, n + ".proj", dim, dim)
    if sr > 1:
        _conv(d, n + ".sr", dim, dim, sr)
        _ln(d, n + ".norm", dim)


def _block(d, n, dim, sr, mlp, ref=False):
    _ln(d, n + ".norm1", dim)
    if ref:
        _ln(d, n + ".norm1_Ref", dim)
    _attn(d, n + ".attn", dim, sr)
    _ln(d, n + ".norm2", dim)
    _lin(d, n + ".mlp.fc1", dim, dim * mlp)
    _conv(d, n + ".mlp.dwconv.dwconv", dim * mlp, dim * mlp, 3, groups=dim * mlp)
    _lin(d, n + ".mlp.fc2", dim * mlp, dim)


def _nonlocal(d, n, c=64, inter=32):
    _conv(d, n + ".g.0", c, inter, 1)
    _conv(d, n + ".W.0", inter, c, 1)
    _bn(d, n + ".W.1", c)
    _conv(d, n + ".theta", c, inter, 1)
    _conv(d, n + ".phi.0", c, inter, 1)


def _refpa(d, n, c):
    oe = n + ".PA.offset_estimator"
    _conv(d, oe + ".downblock1.0", 2 * c, 64, 3)
    _conv(d, oe + ".downblock2.0", 64, 64, 3)
    _conv(d, oe + ".downblock3.0", 64, 64, 3)
    for i in (1, 2, 3):
        _nonlocal(d, oe + f".attentionblock{i}")
    for i in (1, 2, 3):
        _convT(d, oe + f".upblock{i}.0", 64, 64, 3)
    _conv(d, oe + ".channelscaling_block", 64, c, 3)
    _conv(d, n + ".PA.offset_conv", c, 18, 3, bias=False)
    d[n + ".PA.deformconv.weight"] = (c, c, 3, 3)
    _conv(d, n + ".PH.fc.0", 2 * c, c // 8, 1)
    _conv(d, n + ".PH.fc.2", c // 8, 2 * c, 1)
    _conv(d, n + ".PH.reduc.0", 2 * c, c, 1)


def transref_spec():
    """{key: shape} of ``TransRef_Base().state_dict()`` in registration order."""
    d = OrderedDict()
    e = EMBED
    t = "Tenc."
    _pe(d, t + "patch_embed1", 6, e[0], 7)
    for i in (1, 2, 3):
        _pe(d, t + f"patch_embed{i + 1}", e[i - 1], e[i], 3)
    _pe(d, t + "patch_embed1_ref", 3, e[0], 7)
    for i in (1, 2, 3):
        _pe(d, t + f"patch_embed{i + 1}_ref", e[i - 1], e[i], 3)
    _pe(d, t + "mini_patch_embed1", e[0], e[1], 3)
    _pe(d, t + "mini_patch_embed1_ref", e[0], e[1], 3)
    _pe(d, t + "mini_patch_embed2", e[1], e[2], 3)
    _pe(d, t + "mini_patch_embed3", e[2], e[3], 3)
    _pe(d, t + "mini_patch_embed4", e[0], e[3], 3)
    _pe(d, t + "mini_patch_embed2_ref", e[1], e[2], 3)
    _pe(d, t + "mini_patch_embed3_ref", e[2], e[3], 3)
    _pe(d, t + "mini_patch_embed4_ref", e[0], e[3], 3)
    for i in (1, 2, 3):
        _refpa(d, t + f"RefPA{i}", e[i - 1])
    for s in range(4):
        for b in range(2):
            _block(d, t + f"block{s + 1}.{b}", e[s], SR[s], 2)
        _ln(d, t + f"norm{s + 1}", e[s])
        if s < 3:
            _block(d, t + f"patch_block{s + 1}.0", e[s + 1], SR[s], 2, ref=True)
            _ln(d, t + f"pnorm{s + 1}", e[s + 1])
    _pe(d, "Tdec.patch_embed1", 512, 512, 3)
    for b in range(3):
        _block(d, f"Tdec.block1.{b}", 512, 1, 4)
    _ln(d, "Tdec.norm1", 512)
    c = "convtail."
    for name, ci, co, res in (("convd32x", 512, 512, None), ("convd16x", 512, 320, "dense_4"), ("convd8x", 320, 128, "dense_3"),
                              ("convd4x", 128, 64, "dense_2"), ("convd2x", 64, 16, "dense_1"), ("convd1x", 16, 8, None)):
        _convT(d, c + name + ".conv2d", ci, co, 4)
        if res:
            _conv(d, c + res + ".0.conv1.conv2d", co, co, 3)
            _conv(d, c + res + ".0.conv2.conv2d", co, co, 3)
    _conv(d, c + "conv_output.conv2d", 8, 3, 3)
    _conv(d, "clean.conv2d", 8, 3, 3)
    return d


class TransRefModule(ParamTree):
    """The reference's state-dict surface; ``generation`` changes on every ``load_state_dict`` (holders re-pack)."""

    def __init__(self):
        super().__init__(transref_spec())
        self.generation = 0

    def load_state_dict(self, state_dict, strict=True, assign=False):
        r = super().load_state_dict(state_dict, strict=strict)
        self.generation += 1
        return r


def seeded_state_dict(seed=0):
    """Deterministic stand-in weights (CPU, float32), every tensor nonzero: weights N(0, 1 / fan_in) (transposed convolutions: the
    fan-in of one output phase, Cin k^2 / 4), biases N(0, 0.05^2), LayerNorm / BatchNorm scales 1 + N(0, 0.1^2), BN running means
    N(0, 0.05^2), running variances U(0.8, 1.2), ``num_batches_tracked`` 1.  The reference zero-initialises the non-local blocks' BN
    affine (a no-op block) and every bias; these do not."""
    g = torch.Generator().manual_seed(int(seed))
    out = OrderedDict()
    for key, shape in transref_spec().items():
        leaf = key.rsplit(".", 1)[1]
        if leaf == "num_batches_tracked":
            out[key] = torch.ones((), dtype=torch.int64)
        elif leaf == "running_var":
            out[key] = 0.8 + 0.4 * torch.rand(shape, generator=g)
        elif leaf in ("bias", "running_mean"):
            out[key] = 0.05 * torch.randn(shape, generator=g)
        elif len(shape) == 1:
            out[key] = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            fan_in = math.prod(shape[1:])
            if key.endswith(".conv2d.weight") and "convd" in key or ".upblock" in key:
                fan_in = shape[0] * shape[2] * shape[3] / 4
            out[key] = torch.randn(shape, generator=g) * (1.0 / fan_in) ** 0.5
    return out


def _phase_taps(k, pad, p):
    """taps of output phase p of a stride-2 transposed convolution along one axis: (first input offset, [kernel index per tap])"""
    taps = sorted(((p + pad - ky) // 2, ky) for ky in range(k) if (p + pad - ky) % 2 == 0)
    d0 = taps[0][0]
    assert [t[0] - d0 for t in taps] == list(range(len(taps)))
    return d0, [t[1] for t in taps]


def pack(sd, device):
    """Kernel operands from a state dict: GEMM weights [N, (ky, kx, cin)], transposed convolutions as four phase weights, depthwise
    weights [9, C], non-local W convolutions with their eval BatchNorm folded in (fp64), ResidualBlock conv2 biases pre-scaled by 0.1."""
    P = {}
    sd = {k: v.detach().to(torch.float64) for k, v in sd.items() if not k.endswith("num_batches_tracked")}

    def put(k, t):
        P[k] = t.to(device=device, dtype=torch.float32).contiguous()

    for k, v in sd.items():
        if v.dim() == 1:
            put(k, v)
        elif v.dim() == 2:
            put(k, v)
        elif ".dwconv.dwconv." in k:
            put(k, v.reshape(v.shape[0], 9).t())
        elif ".conv2d." in k and "convd" in k or ".upblock" in k:
            pass                                       # transposed: below
        else:
            put(k, v.permute(0, 2, 3, 1).reshape(v.shape[0], -1))
    for k, v in sd.items():
        if v.dim() == 4 and (".conv2d." in k and "convd" in k or ".upblock" in k):
            kk = v.shape[2]
            pad = 1
            phases = []
            for py in (0, 1):
                dy, kys = _phase_taps(kk, pad, py)
                for px in (0, 1):
                    dx, kxs = _phase_taps(kk, pad, px)
                    w = v[:, :, kys][:, :, :, kxs]                       # [cin, cout, th, tw]
                    phases.append((w.permute(1, 2, 3, 0).reshape(v.shape[1], -1).to(device=device, dtype=torch.float32).contiguous(),
                                   len(kys), len(kxs), -dy, -dx))
            P[k[: -len(".weight")] + ".phases"] = phases
    for k in list(sd):
        if k.endswith(".W.1.weight"):
            n = k[: -len(".W.1.weight")]
            s = sd[n + ".W.1.weight"] / torch.sqrt(sd[n + ".W.1.running_var"] + 1e-5)
            put(n + ".W.fold.weight", sd[n + ".W.0.weight"].reshape(64, 32) * s[:, None])
            put(n + ".W.fold.bias", (sd[n + ".W.0.bias"] - sd[n + ".W.1.running_mean"]) * s + sd[n + ".W.1.bias"])
        if ".conv2.conv2d.bias" in k:
            put(k + ".x0.1", sd[k] * 0.1)
    return P


class TransRefNet:
    """``TransRef_Base.forward`` on packed weights ``P`` (``pack``): x6 [512^2, 6], ref3 [512^2, 3] channels-last fp32 on the GPU ->
    [512^2, 3].  ``taps``: optional dict that receives the Tenc stage outputs and the Tdec output (channels-last)."""

    def __init__(self, P, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("TransRefNet runs on the GPU only (HIP kernels, no CPU fallback)")
        self.P, self.dev = P, device

    def _e(self, rows, c):
        return torch.empty((rows, c), device=self.dev, dtype=torch.float32)

    def lin(self, x, n, out=None, **kw):
        w = self.P[n + ".weight"]
        out = self._e(x.shape[0], w.shape[0]) if out is None else out
        return ops.conv_gemm(x, w, out, bias=self.P.get(n + ".bias"), **kw)

    def conv(self, x, n, H, W, k, s, p, out=None, bias=True, **kw):
        w = self.P[n + ".weight"]
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        out = self._e(Ho * Wo, w.shape[0]) if out is None else out
        ops.conv_gemm(x, w, out, geom=(1, H, W, k, k, s, s, p, p), bias=self.P.get(n + ".bias") if bias else None, **kw)
        return out, Ho, Wo

    def ln(self, x, n, eps, out=None):
        out = self._e(*x.shape) if out is None else out
        return ops.layernorm(x, self.P[n + ".weight"], self.P[n + ".bias"], out, eps)

    def convT(self, x, n, H, W, act="none", res=None):
        ph = self.P[n + ".phases"]
        cout = ph[0][0].shape[0]
        buf = torch.empty((4, H * W, cout), device=self.dev, dtype=torch.float32)
        for i, (w, kh, kw, py, px) in enumerate(ph):
            ops.conv_gemm(x, w, buf[i], geom=(1, H, W, kh, kw, 1, 1, py, px, H, W), bias=self.P[n + ".bias"], act=act)
        out = self._e(4 * H * W, cout)
        return ops.tr_phase_interleave(buf, out, H, W, res=res)

    def patch_embed(self, x, n, H, W, k, s):
        y, Ho, Wo = self.conv(x, n + ".proj", H, W, k, s, k // 2)
        return self.ln(y, n + ".norm", 1e-5), Ho, Wo

    def attention(self, q, k, v, heads, scale):
        out = self._e(q.shape[0], q.shape[1])
        return ops.tr_attention(q, k, v, out, heads, q.shape[1] // heads, scale)

    def block(self, x, n, H, W, heads, sr, ref=None):
        """Block / Block_Ref / Block_dec: x + proj(attn(LN x)), then x + fc2(GELU(dwconv(fc1(LN x))))"""
        C = x.shape[1]
        t = self.ln(x, n + ".norm1", 1e-6)
        q = self.lin(t, n + ".attn.q")
        src = t if ref is None else self.ln(ref, n + ".norm1_Ref", 1e-6)
        if sr > 1:
            src, _, _ = self.conv(src, n + ".attn.sr", H, W, sr, sr, 0)
            src = self.ln(src, n + ".attn.norm", 1e-5)
        kv = self.lin(src, n + ".attn.kv")
        a = self.attention(q, kv[:, :C], kv[:, C:], heads, (C // heads) ** -0.5)
        x = self.lin(a, n + ".attn.proj", epi="add", aux1=x)
        t = self.ln(x, n + ".norm2", 1e-6)
        h = self.lin(t, n + ".mlp.fc1")
        g = ops.tr_dwconv3x3_gelu(h, self.P[n + ".mlp.dwconv.dwconv.weight"], self.P[n + ".mlp.dwconv.dwconv.bias"], torch.empty_like(h), H, W)
        return self.lin(g, n + ".mlp.fc2", epi="add", aux1=x)

    def nonlocal_block(self, x, n, H, W, extra):
        """NONLocalBlock2D(x) + extra: W(BN)(softmax(theta phi^T) g) + x + extra (phi, g max-pooled 2x2; no 1/sqrt(d) scale)"""
        theta = self.lin(x, n + ".theta")
        Hp, Wp = H // 2, W // 2
        phi = ops.maxpool(self.lin(x, n + ".phi.0"), self._e(Hp * Wp, 32), 1, H, W, 32, 2, 2, 0)
        g = ops.maxpool(self.lin(x, n + ".g.0"), self._e(Hp * Wp, 32), 1, H, W, 32, 2, 2, 0)
        y = self.attention(theta, phi, g, 1, 1.0)
        return self.lin(y, n + ".W.fold", aux0=x, epi="add", aux1=extra)

    def refpa(self, inp, ref, n, H, W):
        """RefPA: PA (offset estimator, offset conv, deformable conv of ref) then PH."""
        C = inp.shape[1]
        cat = self._e(H * W, 2 * C)
        ops.copy2d(inp, cat[:, :C])
        ops.copy2d(ref, cat[:, C:])
        oe = n + ".PA.offset_estimator"
        d1, H1, W1 = self.conv(cat, oe + ".downblock1.0", H, W, 3, 2, 1, act="lrelu")
        d2, H2, W2 = self.conv(d1, oe + ".downblock2.0", H1, W1, 3, 2, 1, act="lrelu")
        d3, H3, W3 = self.conv(d2, oe + ".downblock3.0", H2, W2, 3, 2, 1, act="lrelu")
        u = self.nonlocal_block(d3, oe + ".attentionblock1", H3, W3, d3)
        u = self.convT(u, oe + ".upblock1.0", H3, W3, act="lrelu")
        u = self.nonlocal_block(u, oe + ".attentionblock2", H2, W2, d2)
        u = self.convT(u, oe + ".upblock2.0", H2, W2, act="lrelu")
        u = self.nonlocal_block(u, oe + ".attentionblock3", H1, W1, d1)
        u = self.convT(u, oe + ".upblock3.0", H1, W1, act="lrelu")
        feat, _, _ = self.conv(u, oe + ".channelscaling_block", H, W, 3, 1, 1)
        off, _, _ = self.conv(feat, n + ".PA.offset_conv", H, W, 3, 1, 1, bias=False)
        cols = ops.tr_deform_im2col(ref, off, self._e(H * W, 9 * C), H, W)
        cat2 = self._e(H * W, 2 * C)
        ops.copy2d(inp, cat2[:, :C])
        ops.conv_gemm(cols, self.P[n + ".PA.deformconv.weight"], cat2[:, C:])
        y = self.lin(cat2, n + ".PH.fc.0", act="gelu")
        y = self.lin(y, n + ".PH.fc.2", act="gelu", epi="mul", aux1=cat2)
        return self.lin(y, n + ".PH.reduc.0", act="gelu")

    def resblock(self, x, n, H, W, skip=None):
        """ResidualBlock (conv2(relu(conv1 x)) * 0.1 + x) [+ skip]"""
        h, _, _ = self.conv(x, n + ".conv1.conv2d", H, W, 3, 1, 1, act="relu")
        out = self._e(*x.shape)
        ops.conv_gemm(h, self.P[n + ".conv2.conv2d.weight"], out, geom=(1, H, W, 3, 3, 1, 1, 1, 1), bias=self.P[n + ".conv2.conv2d.bias.x0.1"],
                      alpha=0.1, aux0=x, epi="add" if skip is not None else "store", aux1=skip)
        return out

    def forward(self, x6, ref3, taps=None):
        e, t = EMBED, "Tenc."
        outs = []
        x1, H1, W1 = self.patch_embed(x6, t + "patch_embed1", SIZE, SIZE, 7, 4)
        xr, Hr, Wr = self.patch_embed(ref3, t + "patch_embed1_ref", SIZE, SIZE, 7, 4)
        x2 = x2r = None
        for s in range(4):
            if s > 0:
                x1, H1, W1 = self.patch_embed(outs[-1], t + f"patch_embed{s + 1}", H1, W1, 3, 2)
                x1 = ops.tr_add(x1, x2, x1)
                if s < 3:
                    xr, Hr, Wr = self.patch_embed(xr, t + f"patch_embed{s + 1}_ref", Hr, Wr, 3, 2)
            if s < 3:
                a = self.refpa(x1, xr, t + f"RefPA{s + 1}", H1, W1)
                x2r, H2, W2 = self.patch_embed(xr, t + f"mini_patch_embed{s + 1}_ref", Hr, Wr, 3, 2)
                x2, _, _ = self.patch_embed(a, t + f"mini_patch_embed{s + 1}", H1, W1, 3, 2)
            for b in range(2):
                x1 = self.block(x1, t + f"block{s + 1}.{b}", H1, W1, HEADS[s], SR[s])
            outs.append(self.ln(x1, t + f"norm{s + 1}", 1e-6))
            if s < 3:
                x2 = self.block(x2, t + f"patch_block{s + 1}.0", H2, W2, HEADS[min(s, 1)], SR[s], ref=x2r)
                x2 = self.ln(x2, t + f"pnorm{s + 1}", 1e-6)
        y, Hd, Wd = self.patch_embed(outs[3], "Tdec.patch_embed1", H1, W1, 3, 2)
        for b in range(3):
            y = self.block(y, f"Tdec.block1.{b}", Hd, Wd, 8, 1)
        y = self.ln(y, "Tdec.norm1", 1e-6)
        if taps is not None:
            taps.update(tenc=outs, tdec=y)
        c = "convtail."
        r = self.convT(y, c + "convd32x.conv2d", Hd, Wd, res=outs[3])
        H = 2 * Hd
        for conv, res, skip in (("convd16x", "dense_4", outs[2]), ("convd8x", "dense_3", outs[1]), ("convd4x", "dense_2", outs[0]),
                                ("convd2x", "dense_1", None)):
            r = self.convT(r, c + conv + ".conv2d", H, H)
            H *= 2
            r = self.resblock(r, c + res + ".0", H, H, skip)
        r = self.convT(r, c + "convd1x.conv2d", H, H)
        out, _, _ = self.conv(r, "clean.conv2d", 2 * H, 2 * H, 3, 1, 1, act="tanh")
        return out


class CheckpointMissing(ImportError):
    """``400_Trans.pth`` is not where the reference keeps it: the plug-in module cannot build its ``inpainter``."""


def load_checkpoint(path):
    """The reference's checkpoint format: ``{'net': state_dict}``, loaded strict=False -> (state dict, missing, unexpected)."""
    ck = torch.load(path, map_location="cpu")
    sd = ck["net"] if isinstance(ck, dict) and "net" in ck else ck
    m = TransRefModule()
    r = m.load_state_dict(sd, strict=False)
    return m.state_dict(), list(r.missing_keys), list(r.unexpected_keys)


class Inpainter:
    """``transref_inpainter.Inpainter`` (transref_inpainter.py:14-70) on the GPU: ``.name``, ``.inpaint(init, mask, control, ...)``.

    Weights: ``state_dict`` (the reference's key set, e.g. ``load_checkpoint(...)[0]``), else ``seeded_state_dict(seed or 0)``.  The
    network is captured once per device into a hipGraph on a side stream with its own split-K workspace and replayed (``graph=False``:
    eager launches); ``module.load_state_dict`` re-packs the weights and drops the graph."""

    def __init__(self, state_dict=None, seed=None, device="cuda", graph=True):
        self.name = "transref_inpainter"
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("transref_inpainter runs on the GPU only (HIP kernels, no CPU fallback)")
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self.module = TransRefModule()
        self.module.load_state_dict(state_dict if state_dict is not None else seeded_state_dict(0 if seed is None else seed), strict=True)
        self.graph = graph
        self._packed = None
        self._graph = None

    def _net(self):
        if self._packed is None or self._packed[0] != self.module.generation:
            self._packed = (self.module.generation, TransRefNet(pack(self.module.state_dict(), self.device), self.device))
            self._graph = None
        return self._packed[1]

    def forward_eager(self, x6, ref3, taps=None):
        with torch.cuda.device(self.device):
            return self._net().forward(x6, ref3, taps)

    def forward_graph(self, x6, ref3):
        """replay of the captured network; the result lives in the graph's static buffer (consume it before the next call)"""
        net = self._net()
        with torch.cuda.device(self.device):
            if self._graph is None:
                sx, sr = x6.clone(), ref3.clone()
                ws = ops.new_workspace(self.device)
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side), ops.workspace_scope(ws):
                    net.forward(sx, sr)                  # warm-up: LDS attributes, allocator pool
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g), ops.workspace_scope(ws):
                    out = net.forward(sx, sr)
                self._graph = (g, sx, sr, out, ws)
            g, sx, sr, out, _ = self._graph
            sx.copy_(x6)
            sr.copy_(ref3)
            g.replay()
            return out

    def prepare(self, init_image_tensor, mask_image_tensor, control_image_tensor):
        """steps 1-6 of the wrapper -> (x6 [512^2, 6], ref3 [512^2, 3], detail3 [3, 512^2], resized mask [planes, 512, 512], (H, W))"""
        img, mask, ctl = init_image_tensor, mask_image_tensor, control_image_tensor
        if ctl is None:
            raise ValueError("transref_inpainter needs control_image_tensor (the reference image)")
        if img.dim() != 4 or img.shape[1] != 3 or ctl.shape != img.shape or mask.dim() != 4 or mask.shape[1] not in (1, 3) or \
                mask.shape[2:] != img.shape[2:]:
            raise ValueError(f"[B,3,H,W] image and control and [B,1|3,H,W] mask expected, got {tuple(img.shape)}, {tuple(ctl.shape)}, "
                             f"{tuple(mask.shape)}")
        if img.shape[0] != 1 or mask.shape[0] != 1 or ctl.shape[0] != 1:
            raise ValueError(f"transref_inpainter handles one image (batch element 0), got batches {img.shape[0]}, {ctl.shape[0]}, {mask.shape[0]}")
        H, W = img.shape[2:]
        dev = self.device
        f = lambda t: t[0].to(device=dev, dtype=torch.float32).contiguous()
        img3, ctl3, m = f(img), f(ctl), f(mask)
        n = SIZE * SIZE
        planes6 = ops.tr_prep(img3, ctl3, torch.empty((6, H, W), device=dev, dtype=torch.float32))
        rs6 = ops.resize_bilinear(planes6[None], SIZE, SIZE, False)[0]
        mrs = ops.resize_bilinear(m[None], SIZE, SIZE, False)[0]
        x6 = torch.empty((n, 6), device=dev, dtype=torch.float32)
        ref3 = torch.empty((n, 3), device=dev, dtype=torch.float32)
        detail3 = torch.empty((3, n), device=dev, dtype=torch.float32)
        ops.tr_pack(rs6, mrs[0], x6, ref3, detail3)
        return x6, ref3, detail3, mrs, (H, W)

    def finish(self, out3, detail3, mrs, hw):
        """steps 7-8: blend, resize back, round -> uint8 [1, 3, H, W]"""
        fake = ops.tr_blend(out3, detail3, mrs.reshape(mrs.shape[0], -1), torch.empty_like(detail3))
        back = ops.resize_bilinear(fake.view(1, 3, SIZE, SIZE), hw[0], hw[1], False)
        return ops.tr_to_u8(back, torch.empty(back.shape, device=back.device, dtype=torch.uint8))

    @torch.no_grad()
    def inpaint(self, init_image_tensor, mask_image_tensor, control_image_tensor=None, prompt="", resize_to_area_limit_before_inpaint=False):
        """init / control [1,3,H,W] (0..255 floats), mask [1,1|3,H,W] -> uint8 [1,3,H,W] on the input's device.  B > 1 raises.
        ``prompt`` and ``resize_to_area_limit_before_inpaint`` are ignored, as in the reference."""
        with torch.cuda.device(self.device):
            x6, ref3, detail3, mrs, hw = self.prepare(init_image_tensor, mask_image_tensor, control_image_tensor)
            out3 = self.forward_graph(x6, ref3) if self.graph else self.forward_eager(x6, ref3)
            u8 = self.finish(out3, detail3, mrs, hw)
        return u8.to(init_image_tensor.device)
