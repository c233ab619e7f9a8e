"""Thin host wrappers over the C-ABI: torch tensors are only device memory here -- every call
passes raw device pointers + sizes to libstitch_gfx950.so on torch's current HIP stream."""
from __future__ import annotations

import ctypes as C
import warnings

import torch

from ._lib import ChainDesc, GemmDesc, JpegDecParams, JpegEncParams, MlpDesc, check, lib
from .jpeg_probe import JpegInfo, probe as _jpeg_probe
from ._lib import StitchError as StitchErrorBase

ACT = dict(none=0, relu=1, gelu=2, sigmoid=3, tanh=4, lrelu=5)
EPI = dict(store=0, add=1, mul=2, gru=3, axpy=4, zr=5)

assert lib.st_abi_gemm_desc_size() == C.sizeof(GemmDesc), "st_gemm_desc ABI mismatch between header and binding"
assert lib.st_abi_chain_desc_size() == C.sizeof(ChainDesc), "st_chain_desc ABI mismatch between header and binding"
assert lib.st_abi_mlp_desc_size() == C.sizeof(MlpDesc), "st_mlp_desc ABI mismatch between header and binding"
assert lib.st_abi_jpeg_dec_params_size() == C.sizeof(JpegDecParams), "st_jpeg_dec_params ABI mismatch between header and binding"
assert lib.st_abi_jpeg_enc_params_size() == C.sizeof(JpegEncParams), "st_jpeg_enc_params ABI mismatch between header and binding"


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    assert t.is_cuda, "device tensor expected (no CPU fallback)"
    return C.c_void_p(t.data_ptr())


def _pc(t):
    """pointer to a tensor the kernel reads as dense row-major"""
    if t is not None and not t.is_contiguous():
        raise ValueError(f"contiguous tensor expected, got shape {tuple(t.shape)} strides {t.stride()}")
    return _p(t)


def _ld(t):
    """row stride of a 2-D row-major view (last dim contiguous)."""
    assert t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1), (t.shape, t.stride())
    return t.stride(0)


class _Stub:
    """shape-only stand-in for an operand that conv_gemm addresses through Planes"""

    def __init__(self, shape):
        self.shape = tuple(shape)

    def dim(self):
        return len(self.shape)

    def stride(self, i):
        return self.shape[1] if i == 0 else 1

    def data_ptr(self):
        return 0


class Planes:
    """Three blocked bf16 planes (hi, mid, lo; x == hi + mid + lo exactly) of a channels-last fp32 tensor [rows, C], C % 32 == 0: the operand
    format of the exact-split contraction (``st_gemm_desc.split3``, csrc/gemm_split3.h).  Storage ``t`` = [3, C / 32, rows, 32] bf16.
    ``cols(c0, c1)`` is a column slice (whole 32-channel chunks) sharing the storage -- concatenation stays a column offset."""

    def __init__(self, rows, C, dev, t=None, c0=0, ncols=None):
        assert C % 32 == 0, C
        self.rows, self.C = rows, C
        self.t = t if t is not None else torch.empty((3, C // 32, rows, 32), device=dev, dtype=torch.bfloat16)
        self.c0, self.ncols = c0, (C if ncols is None else ncols)

    def cols(self, c0, c1):
        assert c0 % 32 == 0 and 0 <= c0 < c1 <= self.ncols, (c0, c1, self.ncols)
        return Planes(self.rows, self.C, None, t=self.t, c0=self.c0 + c0, ncols=c1 - c0)

    @property
    def pstride(self):
        return self.t.stride(0)

    def ptr(self):
        """address of (plane 0, first chunk of this slice)"""
        return self.t.data_ptr() + (self.c0 // 32) * self.rows * 64


def split3_pack(x, out=None, chunk_rows=None):
    """fp32 rows [rows, C] (row stride >= C) -> Planes (st_split3_pack): weights at pack time, activations no split3-emitting kernel produced."""
    rows, Cc = x.shape
    if out is None:
        out = Planes(chunk_rows or rows, Cc, x.device)
    assert out.ncols == Cc and out.rows >= rows
    check(lib.st_split3_pack(_p(x), C.c_void_p(out.ptr()), rows, Cc, _ld(x), out.pstride, out.rows, _stream()), "st_split3_pack")
    return out


_WS = {}
_WS_OVERRIDE = []


def _workspace(dev):
    """split-K slab buffer (64 MiB): one per (device, HIP stream) so concurrent streams never share
    slabs; an execution context that is replayed on arbitrary streams (a captured hipGraph) brings its
    own through ``workspace_scope``."""
    if _WS_OVERRIDE:
        return _WS_OVERRIDE[-1]
    k = (dev.type, dev.index, torch.cuda.current_stream().cuda_stream)
    if k not in _WS:
        _WS[k] = new_workspace(dev)
    return _WS[k]


def new_workspace(dev):
    return torch.empty((16 * 1024 * 1024,), device=dev, dtype=torch.float32)


class workspace_scope:
    """``with ops.workspace_scope(ws):`` -- every split-K GEMM launched inside uses ``ws``."""

    def __init__(self, ws):
        self.ws = ws

    def __enter__(self):
        _WS_OVERRIDE.append(self.ws)
        return self.ws

    def __exit__(self, *exc):
        _WS_OVERRIDE.pop()
        return False


def conv_gemm(x, w, out, *, geom=None, bias=None, act="none", alpha=1.0, aux0=None, row_div=0, row_mod=0,
              epi="store", aux1=None, aux2=None, scale_ptr=None, batch=1, bsa=0, bsw=0, bsc=0, bsx1=0, dil=(1, 1), M=None, tile=0, split_k=0, out2=None,
              ln_eps=None, a2=None, a2_channels=0, _desc_only=False, out_planes=None, plane_row0=0, plane_batch_rows=0, no_f32=False, N=None):
    """out[M,N] = epilogue(alpha * conv(x) @ w^T + bias).

    _desc_only=True returns the filled descriptor without launching (``conv_gemm_pair``).
    a2 / a2_channels: input channels below a2_channels are read from ``a2`` (same shape and row stride as x) instead of x.

    ln_eps: the rows of x are layer-normalised (no affine: fold gamma / beta into w / bias, ``fold_layernorm``) inside
    the kernel before the product (row-streaming kernel only: plain matrix, K = 64 / 128).

    x: 2-D view [rows, Cin] of a channels-last activation; geom=(B,H,W,kh,kw,sh,sw,ph,pw) or None (1x1).
    w: [N, kh*kw*Cin] view.  out/aux*: 2-D views (column slices of wider buffers are fine).

    Exact-split operands (``st_gemm_desc.split3``): x, w (and a2) given as ``Planes`` -- x a column slice of the activation's planes, w the
    ``split3_pack`` image of the [N, K] weight matrix.  out_planes (a ``Planes`` column slice, any kernel of the family): the result also
    leaves as planes, rows plane_row0 + batch * plane_batch_rows + m; no_f32 skips the fp32 store of that output."""
    d = GemmDesc()
    split3 = isinstance(x, Planes)
    if split3:
        assert isinstance(w, Planes) and (a2 is None or isinstance(a2, Planes))
        xp, wp, a2p = x, w, a2
        Cin = xp.ncols
        d.split3 = 1
        d.a_plane_stride, d.a_rows = xp.pstride, xp.rows
        d.w_plane_stride, d.w_rows = wp.pstride, wp.rows
        # stand-ins with the shapes the fp32 path reads below (pointers are replaced afterwards)
        x = _Stub((xp.rows, Cin))
        w = _Stub((wp.rows, wp.ncols))
        a2 = None
    Cin = x.shape[1]
    if geom is None:
        rows = x.shape[0] if M is None else M
        B, H, W, kh, kw, sh, sw, ph, pw = 1, 1, rows, 1, 1, 1, 1, 0, 0
        Ho, Wo = 1, rows
    else:
        B, H, W, kh, kw, sh, sw, ph, pw = geom[:9]
        Ho = (H + 2 * ph - dil[0] * (kh - 1) - 1) // sh + 1
        Wo = (W + 2 * pw - dil[1] * (kw - 1) - 1) // sw + 1
        if len(geom) == 11:            # explicit output size (asymmetric zero padding on the right/bottom)
            Ho, Wo = geom[9], geom[10]
    d.a, d.w, d.c = x.data_ptr(), w.data_ptr(), out.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.aux0 = aux0.data_ptr() if aux0 is not None else None
    d.aux1 = aux1.data_ptr() if aux1 is not None else None
    d.aux2 = aux2.data_ptr() if aux2 is not None else None
    d.scale_ptr = scale_ptr.data_ptr() if scale_ptr is not None else None
    d.M, d.N, d.K = B * Ho * Wo, (w.shape[0] if N is None else N), kh * kw * Cin          # (N: batched W planes hold every batch's rows)
    assert w.shape[1] == d.K, (tuple(w.shape), d.K)
    d.H, d.W, d.Cin, d.ldx = H, W, Cin, _ld(x)
    d.kh, d.kw, d.sh, d.sw, d.ph, d.pw, d.Ho, d.Wo = kh, kw, sh, sw, ph, pw, Ho, Wo
    d.ldw, d.ldc = _ld(w), _ld(out)
    d.ld_aux0 = _ld(aux0) if aux0 is not None else 0
    d.ld_aux1 = _ld(aux1) if aux1 is not None else 0
    d.ld_aux2 = _ld(aux2) if aux2 is not None else 0
    d.aux0_row_div, d.aux0_row_mod = row_div, row_mod
    d.act, d.epi, d.alpha = ACT[act], EPI[epi], alpha
    d.batch, d.batch_stride_a, d.batch_stride_w, d.batch_stride_c = batch, bsa, bsw, bsc
    d.batch_stride_aux1 = bsx1
    d.dh, d.dw = dil
    d.tile_cfg = tile
    d.split_k = split_k
    if ln_eps is not None:
        d.a_ln, d.a_ln_eps = 1, float(ln_eps)
    if a2 is not None:
        assert a2.shape == x.shape and _ld(a2) == _ld(x), "second A source: same geometry and row stride as x"
        d.a2, d.a2_channels = a2.data_ptr(), int(a2_channels)
    if split3:
        d.a, d.w = xp.ptr(), wp.ptr()
        d.ldx, d.ldw = Cin, d.K
        if a2p is not None:
            assert a2p.pstride == xp.pstride and a2p.rows == xp.rows, "second A source: planes of the same geometry"
            d.a2, d.a2_channels = a2p.ptr(), int(a2_channels)
    if out_planes is not None:
        d.c_planes, d.c_plane_stride, d.c_plane_rows = out_planes.t.data_ptr(), out_planes.pstride, out_planes.rows
        d.c_plane_col0, d.c_plane_row0, d.c_plane_batch_rows = out_planes.c0, int(plane_row0), int(plane_batch_rows)
        d.c_no_f32 = 1 if no_f32 else 0
    if out2 is not None:
        d.c2, d.ldc2 = out2.data_ptr(), _ld(out2)
    if _desc_only:
        return d
    _add_workspace(d, out.device)
    check(lib.st_conv_gemm(C.byref(d), _stream()), "st_conv_gemm")
    return out


def _add_workspace(d, dev):
    """the split-K slabs of a single conv_gemm (pair members never split)"""
    if d.batch <= 1 and d.split_k != 1:
        ws = _workspace(dev)
        d.workspace, d.workspace_floats = ws.data_ptr(), ws.numel()


def gemm_last_plan():
    """[kernel family, tile_cfg, split_k, walk / pair flag] of this thread's last st_conv_gemm (st_gemm_last_plan, include/stitch_gfx950.h)"""
    p = (C.c_int32 * 4)()
    check(lib.st_gemm_last_plan(p), "st_gemm_last_plan")
    return list(p)


def gemm_plan(x, w, out, pair_with=None, **kwargs):
    """What ``gemm_last_plan()`` reports after ``conv_gemm(x, w, out, **kwargs)`` -- or, with pair_with = (x, w, out, kwargs), after
    ``conv_gemm_pair((x, w, out, kwargs), pair_with)`` -- without launching anything (st_gemm_plan); StitchError for a rejected descriptor."""
    d = conv_gemm(x, w, out, _desc_only=True, **kwargs)
    d1 = None
    if pair_with is None:
        _add_workspace(d, out.device)
    else:
        d1 = C.byref(conv_gemm(pair_with[0], pair_with[1], pair_with[2], _desc_only=True, **pair_with[3]))
    p = (C.c_int32 * 4)()
    check(lib.st_gemm_plan(C.byref(d), d1, p), "st_gemm_plan")
    return list(p)


def conv_gemm_pair(call0, call1):
    """Two independent conv_gemm calls as ONE launch (st_conv_gemm_pair): each argument is (x, w, out, kwargs)."""
    d0 = conv_gemm(call0[0], call0[1], call0[2], _desc_only=True, **call0[3])
    d1 = conv_gemm(call1[0], call1[1], call1[2], _desc_only=True, **call1[3])
    check(lib.st_conv_gemm_pair(C.byref(d0), C.byref(d1), _stream()), "st_conv_gemm_pair")


def fold_layernorm(gamma, beta, w, bias=None):
    """Weights of ``Linear(LayerNorm(x))`` with the affine folded in, so that the GEMM can normalise its A rows in
    registers (``ln_eps=``): W' = W * gamma (per input column), b' = b + W @ beta.  Weight-only constant folding at
    load time, fp64 on the host."""
    dev = w.device
    w64, g64, b64 = w.detach().double().cpu(), gamma.detach().double().cpu(), beta.detach().double().cpu()
    wf = (w64 * g64[None, :]).float().contiguous().to(dev)
    bf = w64 @ b64
    if bias is not None:
        bf = bf + bias.detach().double().cpu()
    return wf, bf.float().contiguous().to(dev)


def linear_chain128(a, out, layers):
    """out = chain of up to 3 Linear(128 -> 128) layers over the rows of ``a`` without intermediate round trips (st_linear_chain128).
    layers: dicts with w [128,128], bias [128] or None, act (name), ln_eps (None = no LayerNorm of the layer's input; the affine is
    folded into w / bias: ``fold_layernorm``), res: None | a [M, >=128] tensor added to the layer's output | int l = the input of layer l."""
    d = ChainDesc()
    d.a, d.out, d.lda, d.ldo, d.M, d.nlayers = a.data_ptr(), out.data_ptr(), _ld(a), _ld(out), a.shape[0], len(layers)
    for i, y in enumerate(layers):
        ly = d.layer[i]
        w = y["w"]
        assert w.shape == (128, 128) and w.is_contiguous()
        ly.w, ly.bias = w.data_ptr(), (y["bias"].data_ptr() if y.get("bias") is not None else None)
        ly.act = ACT[y.get("act", "none")]
        ly.ln, ly.ln_eps = (1, float(y["ln_eps"])) if y.get("ln_eps") is not None else (0, 0.0)
        r = y.get("res")
        if r is None:
            ly.res = 0
        elif isinstance(r, int):
            ly.res, ly.res_layer = 2, r
        else:
            ly.res, ly.res_ptr, ly.ld_res = 1, r.data_ptr(), _ld(r)
    check(lib.st_linear_chain128(C.byref(d), _stream()), "st_linear_chain128")
    return out


def rowlin128_split3_pack(w, b):
    """weights of a Linear(128 -> N) -> the image st_rowlin128_split3 streams (uint8 tensor; pack once per weight load)"""
    N = w.shape[0]
    assert w.shape == (N, 128) and w.is_contiguous() and (b is None or b.shape == (N,))
    nb = C.c_int64(0)
    check(lib.st_rowlin128_split3_image_bytes(N, C.byref(nb)), "st_rowlin128_split3_image_bytes")
    img = torch.empty(nb.value, dtype=torch.uint8, device=w.device)
    check(lib.st_rowlin128_split3_pack(_p(w), _p(b), N, C.c_void_p(img.data_ptr()), nb.value, _stream()), "st_rowlin128_split3_pack")
    return img


def rowlin128_split3(a, out, image, ln_eps=None, aux=None, row_div=1):
    """out = LayerNorm(a) @ w^T + b [+ aux[row // row_div]] (ln_eps None: no LayerNorm) over 128-wide rows with the weights of `image` (rowlin128_split3_pack)"""
    assert a.shape[1] == 128 and out.shape[0] == a.shape[0] and out.shape[1] % 32 == 0
    if aux is not None:
        assert aux.shape[1] == out.shape[1] and aux.shape[0] * row_div >= a.shape[0]
    check(lib.st_rowlin128_split3(_p(a), _ld(a), _p(out), _ld(out), a.shape[0], out.shape[1], 1 if ln_eps is not None else 0,
                                  float(ln_eps or 0.0), C.c_void_p(image.data_ptr()), image.numel(), _p(aux), _ld(aux) if aux is not None else 0, row_div,
                                  _stream()), "st_rowlin128_split3")
    return out


def latent_self_attn_split3_pack(w, b):
    """q | k | v weights [384, 128] (+ bias [384] or None) of a latent self-attention layer -> the image st_latent_self_attn_split3 streams (uint8 tensor)"""
    assert w.shape == (384, 128) and w.is_contiguous() and (b is None or b.shape == (384,))
    nb = C.c_int64(0)
    check(lib.st_latent_self_attn_split3_image_bytes(C.byref(nb)), "st_latent_self_attn_split3_image_bytes")
    img = torch.empty(nb.value, dtype=torch.uint8, device=w.device)
    check(lib.st_latent_self_attn_split3_pack(_p(w), _p(b), C.c_void_p(img.data_ptr()), nb.value, _stream()), "st_latent_self_attn_split3_pack")
    return img


def latent_self_attn_split3(a, out, image, ln_eps=None, scale=16 ** -0.5):
    """out[M * 8, 128] = the 8-latent, 8-head, D = 16 self-attention of every 8 consecutive rows of q | k | v = LayerNorm(a) @ w^T + b, one launch
    (ln_eps None: no LayerNorm); the weights of `image` (latent_self_attn_split3_pack).  Same bits as rowlin128_split3 -> attention_small."""
    assert a.shape[1] == 128 and out.shape == (a.shape[0], 128)
    check(lib.st_latent_self_attn_split3(_p(a), _ld(a), _p(out), _ld(out), a.shape[0], 1 if ln_eps is not None else 0, float(ln_eps or 0.0), float(scale),
                                         C.c_void_p(image.data_ptr()), image.numel(), _stream()), "st_latent_self_attn_split3")
    return out


def mlp128_split3_pack(w1, b1, w2, proj=None):
    """weights of one st_mlp128 -> the image st_mlp128_split3 streams (uint8 tensor; pack once per weight load).  proj = (wp, bp or None)."""
    hidden = w1.shape[0]
    assert w1.shape == (hidden, 128) and w2.shape == (128, hidden) and w1.is_contiguous() and w2.is_contiguous() and b1.shape == (hidden,)
    nb = C.c_int64(0)
    check(lib.st_mlp128_split3_image_bytes(hidden, 1 if proj is not None else 0, C.byref(nb)), "st_mlp128_split3_image_bytes")
    img = torch.empty(nb.value, dtype=torch.uint8, device=w1.device)
    wp, bp = proj if proj is not None else (None, None)
    if wp is not None:
        assert wp.shape == (128, 128) and wp.is_contiguous()
    check(lib.st_mlp128_split3_pack(_p(w1), _p(b1), _p(w2), _p(wp) if wp is not None else None, _p(bp) if bp is not None else None, hidden,
                                    C.c_void_p(img.data_ptr()), nb.value, _stream()), "st_mlp128_split3_pack")
    return img


def mlp128(a, out, w1, b1, w2, b2, ln_eps=None, res=None, proj=None, image=None):
    """out = x + (GELU(LN(x) @ w1^T + b1) @ w2^T + b2) [+ res] over 128-wide rows in one launch (st_mlp128: the hidden activations stay
    on the CU).  x = a, or with proj = (wp [128,128], bp or None, res0 or None): x = a @ wp^T + bp + res0 (the Block's attention output
    projection + residual in the same launch).  ln_eps None = no LayerNorm (otherwise without affine: fold gamma / beta into w1 / b1)."""
    hidden = w1.shape[0]
    assert w1.shape == (hidden, 128) and w2.shape == (128, hidden) and w1.is_contiguous() and w2.is_contiguous()
    assert b1.shape == (hidden,) and b2.shape == (128,) and a.shape[1] == 128 and out.shape == a.shape
    d = MlpDesc()
    d.a, d.out, d.lda, d.ldo, d.M, d.hidden = a.data_ptr(), out.data_ptr(), _ld(a), _ld(out), a.shape[0], hidden
    d.w1, d.b1, d.w2, d.b2 = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
    d.ln, d.ln_eps = (1, float(ln_eps)) if ln_eps is not None else (0, 0.0)
    if res is not None:
        assert res.shape == a.shape
        d.res, d.ld_res = res.data_ptr(), _ld(res)
    if proj is not None:
        wp, bp, res0 = proj
        assert wp.shape == (128, 128) and wp.is_contiguous()
        d.wp = wp.data_ptr()
        if bp is not None:
            d.bp = bp.data_ptr()
        if res0 is not None:
            assert res0.shape == a.shape
            d.res0, d.ld_res0 = res0.data_ptr(), _ld(res0)
    if image is not None:                                       # the exact-split kernel on the packed image (mlp128_split3_pack)
        check(lib.st_mlp128_split3(C.byref(d), C.c_void_p(image.data_ptr()), image.numel(), _stream()), "st_mlp128_split3")
        return out
    check(lib.st_mlp128(C.byref(d), _stream()), "st_mlp128")
    return out


def corr_volume(f1, f2, out):
    B, N1, Cc = f1.shape
    N2 = f2.shape[1]
    check(lib.st_corr_volume(_p(f1), _p(f2), _p(out), B, N1, N2, Cc, _stream()), "st_corr_volume")
    return out


def corr_volume_split3(f1p, f2p, out12, out21, B, N, Cc):
    """all-pairs volume(s) from the feature planes (st_corr_volume_split3): f1p / f2p = split3_pack of the [B*N, C] feature rows; out21 may be None."""
    assert f1p.pstride == f2p.pstride and f1p.rows == f2p.rows
    check(lib.st_corr_volume_split3(C.c_void_p(f1p.ptr()), C.c_void_p(f2p.ptr()), f1p.pstride, f1p.rows, _pc(out12), _pc(out21) if out21 is not None else None,
                                    B, N, Cc, _stream()), "st_corr_volume_split3")
    return out12


def corr_volume_both(f1, f2, out12, out21):
    """out12 = f1 . f2^T and out21 = f2 . f1^T (= out12^T) from one launch."""
    B, N, Cc = f1.shape
    check(lib.st_corr_volume_both(_p(f1), _p(f2), _pc(out12), _pc(out21), B, N, Cc, _stream()), "st_corr_volume_both")
    return out12, out21


def layernorm(x, w, b, out, eps):
    check(lib.st_layernorm(_p(x), _ld(x), _p(w), _p(b), _p(out), _ld(out), x.shape[0], x.shape[1], eps, _stream()),
          "st_layernorm")
    return out


def softmax_rows(x):
    check(lib.st_softmax_rows(_p(x), _ld(x), x.shape[0], x.shape[1], _stream()), "st_softmax_rows")
    return x


def l2norm_rows(x, out):
    check(lib.st_l2norm_rows(_p(x), _p(out), x.shape[0], x.shape[1], _stream()), "st_l2norm_rows")
    return out


def maxpool(x, out, B, H, W, Cc, k, s, p):
    check(lib.st_maxpool_nhwc(_p(x), _p(out), B, H, W, Cc, k, s, p, _stream()), "st_maxpool_nhwc")
    return out


def dwconv3x3_residual(x, w9c, bias, out, B, H, W, Cc):
    check(lib.st_dwconv3x3_residual(_p(x), _p(w9c), _p(bias), _p(out), B, H, W, Cc, _stream()), "st_dwconv3x3_residual")
    return out


def sine_pe(out, dim, *, coords=None, Wg=0, ws=0, period=0, cscale=1.0, coff=0.0, accumulate=False):
    check(lib.st_sine_pe(_p(out), _ld(out), out.shape[0], dim, _p(coords), _ld(coords) if coords is not None else 0,
                         Wg, ws, period, cscale, coff, int(accumulate), _stream()), "st_sine_pe")       # accumulate: False / True / first added column
    return out


def attention_small(q, qs, k, ks, v, vs, out, os_, B, heads, Nq, Nk, D, scale):
    check(lib.st_attention_small(_p(q), qs[0], qs[1], _p(k), ks[0], ks[1], _p(v), vs[0], vs[1], _p(out), os_[0], os_[1],
                                 B, heads, Nq, Nk, D, scale, _stream()), "st_attention_small")
    return out


def latent_pool(scores, tokens, z, pixels, P):
    check(lib.st_latent_pool(_p(scores), _ld(scores), _p(tokens), _ld(tokens), _pc(z), pixels, P, _stream()), "st_latent_pool")
    return z


def attention_kvlds(q, qs, k, ks, v, vs, out, os_, B, heads, Nq, Nk, D, scale):
    check(lib.st_attention_kvlds(_p(q), qs[0], qs[1], _p(k), ks[0], ks[1], _p(v), vs[0], vs[1], _p(out), os_[0], os_[1],
                                 B, heads, Nq, Nk, D, scale, _stream()), "st_attention_kvlds")
    return out


def window_attention(q, k, v, bs, ts, qpad, kpad, vpad, out, o_bs, o_ts, B, H, W, heads, D, ws, scale):
    check(lib.st_window_attention(_p(q), _p(k), _p(v), bs, ts, _p(qpad), _p(kpad), _p(vpad), _p(out), o_bs, o_ts, B, H, W,
                                  heads, D, ws, scale, _stream()), "st_window_attention")
    return out


def ccl_softargmax(G, out, B, h, w):
    check(lib.st_ccl_softargmax(_p(G), _p(out), _ld(out), B, h, w, _stream()), "st_ccl_softargmax")
    return out


def patch_conv1(maps, w36x16, bias, out, M, H, W, Ho, Wo):
    check(lib.st_patch_conv1(_pc(maps), _pc(w36x16), _pc(bias), _p(out), M, H, W, Ho, Wo, _stream()), "st_patch_conv1")
    return out


def copy2d(src, dst):
    check(lib.st_copy2d(_p(src), _ld(src), _p(dst), _ld(dst), src.shape[0], src.shape[1], _stream()), "st_copy2d")
    return dst


def prep_image(src, dst, ldo, mul, div, sub):
    B, Cc, H, W = src.shape
    check(lib.st_prep_image(_pc(src), _p(dst), B, Cc, H, W, ldo, mul, div, sub, _stream()), "st_prep_image")
    return dst


def coords_grid(out, B, H, W, init=None):
    """rows [B*H*W, 2] = the pixel grid; with ``init`` (NCHW [B,2,H,W] fp32, low-res pixels) grid + init, the decoder's warm start."""
    if init is None:
        check(lib.st_coords_grid(_p(out), B, H, W, _stream()), "st_coords_grid")
        return
    if tuple(init.shape) != (B, 2, H, W) or init.dtype != torch.float32 or not init.is_contiguous() or init.device != out.device:
        raise ValueError(f"flow_init must be a contiguous float32 [{B}, 2, {H}, {W}] tensor on {out.device}")
    check(lib.st_coords_grid_init(_p(out), _p(init), B, H, W, _stream()), "st_coords_grid_init")


def forward_interpolate(flow, out=None, *, coords_rows=None):
    """The next frame's flow_init from this frame's low-resolution flow (core/utils/utils.py:32-60 as one kernel; contract in
    include/stitch_gfx950.h).  ``flow``: NCHW [B,2,H1,W1]; or, with ``coords_rows=(B, H1, W1)``, the decoder's coords1 rows
    [B*H1*W1, 2] (the grid is subtracted in the kernel).  Returns ``out`` (NCHW [B,2,H1,W1], allocated when None)."""
    if coords_rows is None:
        B, two, H, W = flow.shape
        ok = two == 2
    else:
        B, H, W = coords_rows
        ok = tuple(flow.shape) == (B * H * W, 2)
    if not ok or flow.dtype != torch.float32 or not flow.is_contiguous() or not flow.is_cuda:
        raise ValueError("forward_interpolate takes a contiguous float32 cuda tensor [B,2,H1,W1], or coords1 rows [B*H1*W1,2]")
    if out is None:
        out = torch.empty((B, 2, H, W), device=flow.device)
    elif tuple(out.shape) != (B, 2, H, W) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != flow.device:
        raise ValueError(f"out must be a contiguous float32 [{B}, 2, {H}, {W}] tensor on {flow.device}")
    check(lib.st_flow_forward_interpolate(_p(flow), 0 if coords_rows is None else 1, _p(out), B, H, W, _stream()),
          "st_flow_forward_interpolate")
    return out


def flow_from_coords(coords1, flow4, dst2, B, H, W):
    check(lib.st_flow_from_coords(_p(coords1), _p(flow4), _ld(flow4) if flow4 is not None else 0, _p(dst2),
                                  _ld(dst2) if dst2 is not None else 0, B, H, W, _stream()), "st_flow_from_coords")


def flow_encode(coords1, w98, bias, out, flow2, B, H, W):
    """out[:, :Co] = relu(conv7x7(coords1 - grid)); flow2[:, :2] = the flow (gru.py:251,254, decoder.py:321)."""
    check(lib.st_flow_encode(_pc(coords1), _pc(w98), _pc(bias), _p(out), _ld(out), _p(flow2), _ld(flow2) if flow2 is not None else 0,
                             B, H, W, w98.shape[1], _stream()), "st_flow_encode")
    return out


def flow_encode_split3(coords1, w98, bias, out, flow2, B, H, W, out_planes, flow_planes):
    """flow_encode that also writes the planes a split3 consumer reads: out_planes = image of out[:, :Co]; flow_planes = the column slice
    of the GRU input's planes that starts at the flow's two channels' 32-channel chunk (its offset inside the chunk from flow2's column)."""
    fp, fcol = flow_planes
    check(lib.st_flow_encode_split3(_pc(coords1), _pc(w98), _pc(bias), _p(out), _ld(out), _p(flow2), _ld(flow2), B, H, W, w98.shape[1],
                                    C.c_void_p(out_planes.ptr()), out_planes.pstride, out_planes.rows,
                                    C.c_void_p(fp.t.data_ptr()), fp.pstride, fp.rows, int(fcol), _stream()), "st_flow_encode_split3")
    return out


def cost_lookup(maps, coords, out, Nq, H2, W2, r=4):
    check(lib.st_cost_lookup(_p(maps), _p(coords), _p(out), _ld(out), Nq, H2, W2, r, _stream()), "st_cost_lookup")
    return out


def decoder_token_chain(corr, coords1, kv, weights16, rows, ntok):
    """weights16: list of 16 contiguous device tensors (see include/stitch_gfx950.h)."""
    arr = (C.c_void_p * 16)(*[w.data_ptr() for w in weights16])
    check(lib.st_decoder_token_chain(_p(corr), _ld(corr), _pc(coords1), _p(kv), arr, rows, ntok, _stream()), "st_decoder_token_chain")
    return corr


# ---- operator-level entry points (csrc/operators.hip) -------------------------------------------
def _ws(dev):
    ws = _workspace(dev)
    return ws.data_ptr(), ws.numel()


def patch_conv12(maps, c0_w, c0_b, c2_w, c2_b, out, M, H=64, W=64):
    """ReLU(c2(ReLU(c0(map)))) per 64x64 cost map in one launch (st_patch_conv12): maps [M, 4096] -> out [M*256, 32]."""
    check(lib.st_patch_conv12(_pc(maps), _pc(c0_w), _pc(c0_b), _pc(c2_w), _pc(c2_b), _p(out), M, H, W, _stream()), "st_patch_conv12")
    return out


def patch_conv12_planes(maps, c0_w, c0_b, c2_w, c2_b, planes, M, H=64, W=64):
    """patch_conv12 whose result leaves as the bf16 planes of ``planes`` = Planes(rows >= M*256, 32) (st_patch_conv12_planes)"""
    check(lib.st_patch_conv12_planes(_pc(maps), _pc(c0_w), _pc(c0_b), _pc(c2_w), _pc(c2_b), C.c_void_p(planes.ptr()), planes.pstride, M, H, W, _stream()),
          "st_patch_conv12_planes")
    return planes


def cost_lookup9x9(maps, coords, out, Nq, H2, W2):
    check(lib.st_cost_lookup9x9(_p(maps), _pc(coords), _p(out), _ld(out), Nq, H2, W2, _stream()), "st_cost_lookup9x9")
    return out


def patch_embed(cost_maps, weights11, ld_f0, pe_bias, s1, s2, s3, s4, tokens, M, H, W):
    """s1 = None: the caller expects the fused c0 + c2 launch (64 x 64 maps).  Whether it fuses is the LIBRARY's decision (shape and operand
    alignment): if it declines (ST_EINVAL) the scratch is allocated here and the call repeated -- the two sides cannot
    disagree into a hard failure."""
    arr = (C.c_void_p * 11)(*[w.data_ptr() for w in weights11])

    def call(s1_):
        return lib.st_patch_embed(_pc(cost_maps), arr, ld_f0, _pc(pe_bias), _pc(s1_) if s1_ is not None else None, _pc(s2), _pc(s3), _pc(s4), _pc(tokens),
                                  M, H, W, *_ws(cost_maps.device), _stream())
    rc = call(s1)
    if rc == 1001 and s1 is None:
        Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
        rc = call(torch.empty((M * (Hp // 2) * (Wp // 2), 16), device=cost_maps.device, dtype=torch.float32))
    check(rc, "st_patch_embed")
    return tokens


def pe_tail_split3_pack(w_f0, w_f2):
    """ffn_with_coord.0's first 64 input columns [128, ld] + ffn_with_coord.2 [128, 128] -> the LDS image of st_pe_tail_split3 (uint8 tensor; pack once per weight load)"""
    assert w_f0.shape[0] == 128 and w_f0.shape[1] >= 64 and w_f0.stride(1) == 1 and w_f2.shape == (128, 128) and w_f2.is_contiguous()
    nb = C.c_int64(0)
    check(lib.st_pe_tail_split3_image_bytes(C.byref(nb)), "st_pe_tail_split3_image_bytes")
    img = torch.empty(nb.value, dtype=torch.uint8, device=w_f0.device)
    check(lib.st_pe_tail_split3_pack(_p(w_f0), w_f0.stride(0), _p(w_f2), C.c_void_p(img.data_ptr()), nb.value, _stream()), "st_pe_tail_split3_pack")
    return img


def pe_tail_split3(x, tab, image, b2, gamma, beta, out, eps=1e-5):
    """out[R,128] = LayerNorm(ReLU(x[R,64] @ w1^T + tab[r % P]) @ w2^T + b2) (st_pe_tail_split3)"""
    assert x.shape[1] == 64 and x.is_contiguous() and out.shape == (x.shape[0], 128) and out.is_contiguous() and tab.shape[1] == 128 and tab.is_contiguous()
    check(lib.st_pe_tail_split3(_p(x), _p(tab), tab.shape[0], C.c_void_p(image.data_ptr()), image.numel(), _p(b2), _p(gamma), _p(beta), float(eps), _p(out),
                                x.shape[0], _stream()), "st_pe_tail_split3")
    return out


def patch_embed_split3(cost_maps, weights11, ld_f0, pe_bias, s2_planes, c4_w_planes, s3, s4, tokens, M, H, W, tail_image=None):
    """patch_embed for 64 x 64 maps with the third convolution on exact-split operands (st_patch_embed_split3); s2_planes = Planes(M*256, 32);
    tail_image (pe_tail_split3_pack): the three launches behind it as one (s4 may then be None)."""
    arr = (C.c_void_p * 11)(*[w.data_ptr() for w in weights11])
    check(lib.st_patch_embed_split3(_pc(cost_maps), arr, ld_f0, _pc(pe_bias), C.c_void_p(s2_planes.ptr()), s2_planes.pstride, C.c_void_p(c4_w_planes.ptr()),
                                    c4_w_planes.pstride, _pc(s3), _pc(s4) if s4 is not None else None, _pc(tokens), M, H, W,
                                    C.c_void_p(tail_image.data_ptr()) if tail_image is not None else None, tail_image.numel() if tail_image is not None else 0,
                                    *_ws(cost_maps.device), _stream()), "st_patch_embed_split3")
    return tokens


def gma_attention(inp, w_qk, qk, attn, B, N):
    check(lib.st_gma_attention(_p(inp), _ld(inp), _pc(w_qk), _pc(qk), _pc(attn), B, N, *_ws(inp.device), _stream()),
          "st_gma_attention")
    return attn


def gma_aggregate(attn, mf, w_v, gamma, vT, out, B, N, out_planes=None):
    """out = mf + gamma * attn @ (mf . w_v^T) (st_gma_aggregate); out_planes (a Planes column slice): the result also leaves as planes
    (st_gma_aggregate_planes: the same two fp32-MFMA launches, the second one's epilogue emits them)."""
    if out_planes is not None:
        check(lib.st_gma_aggregate_planes(_pc(attn), _p(mf), _ld(mf), _pc(w_v), _p(gamma), _pc(vT), _p(out), _ld(out), C.c_void_p(out_planes.t.data_ptr()),
                                          out_planes.pstride, out_planes.rows, out_planes.c0, B, N, *_ws(mf.device), _stream()), "st_gma_aggregate_planes")
        return out
    check(lib.st_gma_aggregate(_pc(attn), _p(mf), _ld(mf), _pc(w_v), _p(gamma), _pc(vT), _p(out), _ld(out), B, N,
                               *_ws(mf.device), _stream()), "st_gma_aggregate")
    return out


def gma_aggregate_split3(attn_planes, mf, w_v, gamma, vT, vT_planes, out, out_planes, B, N):
    """gma_aggregate on planes: attn_planes = split3_pack(attn [B*N, N]); vT_planes scratch Planes(B*128, N); out also -> out_planes (column slice)."""
    check(lib.st_gma_aggregate_split3(C.c_void_p(attn_planes.ptr()), attn_planes.pstride, _p(mf), _ld(mf), _pc(w_v), _p(gamma), _pc(vT),
                                      C.c_void_p(vT_planes.ptr()), vT_planes.pstride, _p(out), _ld(out), C.c_void_p(out_planes.t.data_ptr()),
                                      out_planes.pstride, out_planes.rows, out_planes.c0, B, N, *_ws(mf.device), _stream()), "st_gma_aggregate_split3")
    return out


def sepconv_gru_split3(hxA, hxA_planes, hxB_planes, zbuf, tab1, tab2, w_zr1, w_q1, w_zr2, w_q2, B, H, W):
    """sepconv_gru on planes (st_sepconv_gru_split3): w_* are split3_pack images of the fp32 operator's weights."""
    assert hxA_planes.pstride == hxB_planes.pstride and hxA_planes.rows == hxB_planes.rows and hxA_planes.C == _ld(hxA)
    assert w_zr1.pstride == w_zr2.pstride and w_q1.pstride == w_q2.pstride
    check(lib.st_sepconv_gru_split3(_p(hxA), _ld(hxA), C.c_void_p(hxA_planes.t.data_ptr()), C.c_void_p(hxB_planes.t.data_ptr()),
                                    hxA_planes.pstride, hxA_planes.rows, _pc(zbuf), _p(tab1), _p(tab2), _ld(tab1),
                                    C.c_void_p(w_zr1.ptr()), C.c_void_p(w_q1.ptr()), C.c_void_p(w_zr2.ptr()), C.c_void_p(w_q2.ptr()),
                                    w_zr1.pstride, w_q1.pstride, B, H, W, *_ws(hxA.device), _stream()), "st_sepconv_gru_split3")
    return hxA


def sepconv_gru(hxA, hxB, zbuf, tab1, tab2, w_zr1, w_q1, w_zr2, w_q2, B, H, W):
    assert _ld(hxA) == _ld(hxB) and w_zr1.shape[1] == 5 * _ld(hxA)
    check(lib.st_sepconv_gru(_p(hxA), _p(hxB), _ld(hxA), _pc(zbuf), _p(tab1), _p(tab2), _ld(tab1), _pc(w_zr1), _pc(w_q1),
                             _pc(w_zr2), _pc(w_q2), B, H, W, *_ws(hxA.device), _stream()), "st_sepconv_gru")
    return hxA


def convex_upsample(coords1, mask, out, B, H, W):
    check(lib.st_convex_upsample(_p(coords1), _p(mask), _ld(mask), _p(out), B, H, W, _stream()), "st_convex_upsample")
    return out


# ---- geometric stage (NCHW) ------------------------------------------------------------------
def dlt4(src4x2, motion, H_out, B, mscale_x=1.0, mscale_y=1.0, div=1.0):
    check(lib.st_dlt4(_pc(src4x2), _pc(motion), _pc(H_out), B, mscale_x, mscale_y, div, _stream()), "st_dlt4")
    return H_out


def mat3_sandwich(L, X, R, out, invert=False):
    check(lib.st_mat3_sandwich(_pc(L), _pc(X), _pc(R), _pc(out), X.shape[0], int(invert), _stream()), "st_mat3_sandwich")
    return out


def homo_warp(U, theta, out_hw, n_ones=0, want_idx=False, want_out=True):
    """U [B,C,H,W] (or None with C=0) -> out [B,C+n_ones,oh,ow] (+ idx [B,oh,ow,4] int32)."""
    B = theta.shape[0]
    if U is not None:
        _, Cc, H, W = U.shape
    else:
        raise ValueError("U required (pass n_ones for the implicit mask channels)")
    oh, ow = int(out_hw[0]), int(out_hw[1])
    out = torch.empty((B, Cc + n_ones, oh, ow), device=theta.device, dtype=torch.float32) if want_out else None
    idx = torch.empty((B, oh, ow, 4), device=theta.device, dtype=torch.int32) if want_idx else None
    check(lib.st_homo_warp(_pc(U), _pc(theta), _p(out), _p(idx), B, Cc, n_ones, H, W, oh, ow, _stream()), "st_homo_warp")
    return (out, idx) if want_idx else out


def mesh_bounds(H, out4, width, height, gw=511, gh=511):
    check(lib.st_mesh_bounds(_pc(H), _p(out4), H.shape[0], float(width), float(height), gw, gh, _stream()), "st_mesh_bounds")
    return out4


def flow_warp(x, flow, mul=None):
    B, Cc, H, W = x.shape
    out = torch.empty_like(x)
    check(lib.st_grid_sample_blend(_pc(x), _pc(flow), _pc(mul), _p(out), B, Cc, H, W, _stream()), "st_grid_sample_blend")
    return out


def homo_flow_warp(image2, H8, flow, want_hi=True):
    """use_combine_h_flow tail: image2 [B,3,H,W], H8 [B,3,3], flow [B,2,H,W] -> (final [B,6,H,W], overlap [B,H,W], Hi [B,3,3] or None)."""
    B, Cc, H, W = image2.shape
    if Cc != 3 or tuple(flow.shape) != (B, 2, H, W) or tuple(H8.shape) != (B, 3, 3):
        raise ValueError(f"image2 [B,3,H,W], H8 [B,3,3], flow [B,2,H,W] expected: {tuple(image2.shape)} {tuple(H8.shape)} {tuple(flow.shape)}")
    dev = image2.device
    out = torch.empty((B, 6, H, W), device=dev, dtype=torch.float32)
    overlap = torch.empty((B, H, W), device=dev, dtype=torch.float32)
    hi = torch.empty((B, 3, 3), device=dev, dtype=torch.float32) if want_hi else None
    check(lib.st_homo_flow_warp(_pc(image2), _pc(H8), _pc(flow), _p(out), _p(overlap), _p(hi), B, H, W, _stream()), "st_homo_flow_warp")
    return out, overlap, hi


def resize_bilinear(x, oh, ow, align_corners, div=None):
    B, Cc, H, W = x.shape
    out = torch.empty((B, Cc, oh, ow), device=x.device, dtype=torch.float32)
    d0, d1, nd = (div[0], div[1], 2) if div is not None else (1.0, 1.0, 0)
    check(lib.st_resize_bilinear(_pc(x), _p(out), B * Cc, H, W, oh, ow, int(align_corners), d0, d1, nd, _stream()),
          "st_resize_bilinear")
    return out


def range_map(flow):
    B, _, H, W = flow.shape
    scratch = torch.empty((B * H * W,), device=flow.device, dtype=torch.int64)
    out = torch.empty((B, 1, H, W), device=flow.device, dtype=torch.float32)
    check(lib.st_range_map(_pc(flow), _p(scratch), _p(out), B, H, W, _stream()), "st_range_map")
    return out


def occlusion_from_range(rng, threshold):
    out = torch.empty_like(rng)
    check(lib.st_occlusion_from_range(_pc(rng), _p(out), rng.numel(), int(threshold), _stream()), "st_occlusion_from_range")
    return out


def morph_open(mask, ksz=19):
    B, Cc, H, W = mask.shape
    scratch = torch.empty((2 * B * Cc * H * W,), device=mask.device, dtype=torch.uint8)
    out = torch.empty_like(mask)
    if ksz == 19:
        check(lib.st_morph_open19(_pc(mask), _p(out), _p(scratch), B * Cc, H, W, _stream()), "st_morph_open19")
    else:
        check(lib.st_morph_open(_pc(mask), _p(out), _p(scratch), B * Cc, H, W, ksz, _stream()), "st_morph_open")
    return out


def eval_finish(final6, occ):
    B, _, H, W = final6.shape
    overlap = torch.empty((B, H, W), device=final6.device, dtype=torch.float32)
    check(lib.st_eval_finish(_pc(final6), _pc(occ), _p(overlap), B, H, W, _stream()), "st_eval_finish")
    return overlap


def blend(homo1, homo2, fin, occ):
    _, _, h, w = homo1.shape
    dev = homo1.device
    o2 = torch.empty((1, 3, h, w), device=dev)
    m1 = torch.empty((1, 3, h, w), device=dev)
    m2 = torch.empty((1, 3, h, w), device=dev)
    bl = torch.empty((1, 3, h, w), device=dev, dtype=torch.uint8)
    check(lib.st_blend(_pc(homo1), _pc(homo2), _pc(fin), _pc(occ), _p(o2), _p(m1), _p(m2), _p(bl), h, w, _stream()), "st_blend")
    return o2, m1, m2, bl


def blend_plain(homo1, homo2, fin):
    """test_out blend without the consistency mask: (output2, mask1, mask2, blend) as ``blend``, fin left as it is."""
    _, _, h, w = homo1.shape
    dev = homo1.device
    o2 = torch.empty((1, 3, h, w), device=dev)
    m1 = torch.empty((1, 3, h, w), device=dev)
    m2 = torch.empty((1, 3, h, w), device=dev)
    bl = torch.empty((1, 3, h, w), device=dev, dtype=torch.uint8)
    check(lib.st_blend_plain(_pc(homo1), _pc(homo2), _pc(fin), _p(o2), _p(m1), _p(m2), _p(bl), h, w, _stream()), "st_blend_plain")
    return o2, m1, m2, bl


def mean_threshold(x, thr):
    B, Cc, H, W = x.shape
    out = torch.empty((B, 1, H, W), device=x.device, dtype=torch.float32)
    check(lib.st_mean_threshold(_pc(x), _p(out), B, Cc, H, W, thr, _stream()), "st_mean_threshold")
    return out


def tps_transform(U, source, target, out_hw, want_idx=False):
    """UDIS2 TPS transformer: U [B,C,H,W], source/target [B,N,2] in [-1,1] -> [B,C,oh,ow] (+T, idx)."""
    B, Cc, H, W = U.shape
    N = source.shape[1]
    oh, ow = int(out_hw[0]), int(out_hw[1])
    dev = U.device
    work = torch.empty((B * (N + 3) * (N + 5),), device=dev, dtype=torch.float64)
    T = torch.empty((B, 2, N + 3), device=dev, dtype=torch.float32)
    out = torch.empty((B, Cc, oh, ow), device=dev, dtype=torch.float32)
    idx = torch.empty((B, oh, ow, 4), device=dev, dtype=torch.int32) if want_idx else None
    check(lib.st_tps_solve_grid(_p(U), _p(source.contiguous()), _p(target.contiguous()), _p(work), _p(T), _p(out), _p(idx),
                                B, Cc, H, W, N, oh, ow, _stream()), "st_tps_solve_grid")
    return (out, T, idx) if want_idx else (out, T)


# ---- evaluation metric --------------------------------------------------------------------------
def load_rgb8(src_u8_hwc, out=None):
    """core/datasets.py:383-386 / out.py:137-143 on the GPU: uint8 [B,H,W,3] (decoder layout) -> float32 [B,3,H,W]."""
    B, H, W, c = src_u8_hwc.shape
    if c != 3 or src_u8_hwc.dtype != torch.uint8:
        raise ValueError(f"uint8 [B,H,W,3] expected, got {src_u8_hwc.dtype} {tuple(src_u8_hwc.shape)}")
    if out is None:
        out = torch.empty((B, 3, H, W), device=src_u8_hwc.device, dtype=torch.float32)
    check(lib.st_load_rgb8(_pc(src_u8_hwc), _pc(out), B, H, W, _stream()), "st_load_rgb8")
    return out


_JPEG_SAMPLING = {None: (2, 2), 2: (2, 2), 1: (2, 1), 0: (1, 1)}        # Pillow's `subsampling` -> luma sampling factors


def _jpeg_enc_params(channels, quality, subsampling, optimize, W=0, restart_marker_blocks=None, restart_marker_rows=None):
    """The `JpegEncParams` of Pillow's `save` keywords, or None when every keyword is at its default (`st_jpeg_encode_u8`, which fills in
    Pillow's defaults itself).  The restart interval in MCUs (`reserved[0]`) is libjpeg's: with `restart_marker_rows` r > 0
    min(r * MCUs per row, 65535), rows win over blocks; otherwise `restart_marker_blocks`; 0: none."""
    for name, v, top in (("restart_marker_blocks", restart_marker_blocks, 65535), ("restart_marker_rows", restart_marker_rows, None)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 0 or (top is not None and v > top)):
            raise ValueError(f"{name} {v!r}: an integer 0..{top if top is not None else ''} expected")
    if quality is None and subsampling is None and not optimize and not restart_marker_blocks and not restart_marker_rows:
        return None
    if subsampling not in _JPEG_SAMPLING or isinstance(subsampling, bool):
        raise ValueError(f"subsampling {subsampling!r}: None, 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0) expected")
    if channels == 1 and subsampling is not None:
        raise ValueError("subsampling applies to RGB arrays only (an L file has one component)")
    q = 75 if quality is None else quality
    if isinstance(q, bool) or not isinstance(q, int) or not 1 <= q <= 100:
        raise ValueError(f"quality {quality!r}: an integer 1..100 expected")
    hs, vs = _JPEG_SAMPLING[subsampling] if channels == 3 else (1, 1)
    prm = JpegEncParams(q, hs, vs, 1 if optimize else 0)
    prm.reserved[0] = min(restart_marker_rows * -(-W // (8 * hs)), 65535) if restart_marker_rows else (restart_marker_blocks or 0)
    return prm


def jpeg_encode(u8, workspace=None, quality=None, subsampling=None, optimize=False, restart_marker_blocks=None, restart_marker_rows=None):
    """out.py:260-312 `Image.fromarray(arr).save(path)` on the GPU: uint8 [H,W,3] (RGB) or [H,W] (L) -> (buf, nbytes), the JPEG file Pillow
    writes, byte for byte.  buf: uint8 device tensor of the worst-case size, nbytes: device int32 [1], the file is buf[:nbytes].  Rows may be
    strided (a column slice of a wider canvas).  No host synchronisation; current stream.
    `quality` (1..100), `subsampling` (RGB only: 0 4:4:4, 1 4:2:2, 2 4:2:0) and `optimize` are Pillow's `save` keywords (`st_jpeg_encode_u8_ex`);
    with all three at their defaults the call goes to `st_jpeg_encode_u8`, the same encoder (csrc/jpeg.hip) at Pillow's defaults -- quality 75,
    4:2:0, the Annex K tables.  `restart_marker_blocks` (MCUs, 0..65535) and `restart_marker_rows` (MCU rows; wins) are Pillow's too: a DRI
    segment, FF D0..D7 between the intervals, DC predictions restarting (the jpegr_enc_* kernels of csrc/jpeg.hip); None or 0: no restart interval.
    `workspace`: a uint8 device tensor of at least `jpeg_workspace_bytes` (same keywords) to reuse (stream-ordered: same stream as its last use)."""
    if u8.dtype != torch.uint8 or not (u8.dim() == 2 or (u8.dim() == 3 and u8.shape[2] == 3)):
        raise ValueError(f"uint8 [H,W,3] or [H,W] expected, got {u8.dtype} {tuple(u8.shape)}")
    H, W = u8.shape[:2]
    ch = 3 if u8.dim() == 3 else 1
    prm = _jpeg_enc_params(ch, quality, subsampling, optimize, W, restart_marker_blocks, restart_marker_rows)
    if (W > 1 and u8.stride(1) != ch) or (ch == 3 and u8.stride(2) != 1) or (H > 1 and u8.stride(0) < W * ch):
        u8 = u8.contiguous()
    row_stride = u8.stride(0) if H > 1 else W * ch
    if prm is None:
        cap, need = lib.st_jpeg_max_bytes(H, W, ch), lib.st_jpeg_workspace_bytes(H, W, ch)
    else:
        cap, need = lib.st_jpeg_max_bytes_ex(H, W, ch, C.byref(prm)), lib.st_jpeg_workspace_bytes_ex(H, W, ch, C.byref(prm))
    if cap == 0:
        raise StitchErrorBase(f"st_jpeg_encode_u8: unsupported shape {tuple(u8.shape)} (sides 1..65535, H * W <= 2^24)")
    if workspace is None:
        workspace = torch.empty((need,), device=u8.device, dtype=torch.uint8)
    buf = torch.empty((cap,), device=u8.device, dtype=torch.uint8)
    nbytes = torch.empty((1,), device=u8.device, dtype=torch.int32)
    if prm is None:
        check(lib.st_jpeg_encode_u8(_p(u8), H, W, ch, row_stride, _p(buf), cap, _p(nbytes), _pc(workspace), workspace.numel() * workspace.element_size(),
                                    _stream()), "st_jpeg_encode_u8")
    else:
        check(lib.st_jpeg_encode_u8_ex(_p(u8), H, W, ch, row_stride, C.byref(prm), _p(buf), cap, _p(nbytes), _pc(workspace),
                                       workspace.numel() * workspace.element_size(), _stream()), "st_jpeg_encode_u8_ex")
    return buf, nbytes


def jpeg_workspace_bytes(H, W, channels, quality=None, subsampling=None, optimize=False, restart_marker_blocks=None, restart_marker_rows=None):
    prm = _jpeg_enc_params(channels, quality, subsampling, optimize, W, restart_marker_blocks, restart_marker_rows)
    if prm is None:
        return lib.st_jpeg_workspace_bytes(H, W, channels)
    return lib.st_jpeg_workspace_bytes_ex(H, W, channels, C.byref(prm))


def jpeg_bytes(buf, nbytes):
    """The file of `jpeg_encode` on the host: reads the count, then copies exactly that many bytes."""
    n = int(nbytes.item())
    return buf[:n].cpu().numpy().tobytes()


def jpeg_probe(data, restart=False):
    """Host-side marker parse of a JPEG file (bytes-like, or a CPU uint8 tensor): the `JpegInfo` `jpeg_decode` needs, or None when the file is
    outside the decoder's contract (progressive, restart intervals, other sampling factors, ...: jpeg_probe.py) and keeps the Pillow path.
    restart=True also takes a file with a restart interval whose markers are all there and in order (`JpegInfo.restart_interval` > 0:
    the jpegr_* kernels of csrc/jpeg_dec.hip decode its entropy-coded part)."""
    if isinstance(data, torch.Tensor):
        data = data.numpy().tobytes()
    return _jpeg_probe(data, restart=restart)


def _jpeg_dec_params(info):
    return JpegDecParams(info.H, info.W, info.ncomp, info.hs, info.vs, (C.c_int32 * 3)(*info.tq), (C.c_int32 * 3)(*info.td), (C.c_int32 * 3)(*info.ta),
                         (C.c_int32 * 2)(*info.q_off), (C.c_int32 * 2)(*info.dc_off), (C.c_int32 * 2)(*info.ac_off), info.scan_off, info.scan_len,
                         info.restart_interval, 0)


def jpeg_dec_workspace_bytes(info):
    if info.restart_interval:
        return lib.st_jpeg_dec_workspace_bytes_ex(C.byref(_jpeg_dec_params(info)))
    return lib.st_jpeg_dec_workspace_bytes(info.H, info.W, info.ncomp, info.hs, info.vs, info.scan_len)


def jpeg_decode(data, info=None, out=None, workspace=None, status=None):
    """evaluate.py / out.py `np.array(Image.open(path))` on the GPU: the file's bytes -> (uint8 [H,W,3] or [H,W,1] device tensor, status), the
    pixels Pillow returns on libjpeg-turbo, bit for bit (csrc/jpeg_dec.hip).  `data`: bytes or a CPU uint8 tensor (uploaded on the current
    stream; `info` defaults to `jpeg_probe(data, restart=True)`), or a device uint8 tensor (`info` required).  `out`: a uint8 [H,W,C] device view to decode
    into, rows may be strided.  status: device int32 [1] (or the given one-element int32 device view): 0, or nonzero when the scan ended
    before the frame's blocks or ran on after them (pixels then unspecified; with restart intervals: some interval's bytes did, and the MCUs of
    every other interval are still exact).  No host synchronisation; current stream.
    `workspace`: a uint8 device tensor of at least `jpeg_dec_workspace_bytes(info)` to reuse (stream-ordered)."""
    if isinstance(data, (bytes, bytearray, memoryview)):
        data = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    if data.dtype != torch.uint8 or data.dim() != 1:
        raise ValueError(f"uint8 [nbytes] expected, got {data.dtype} {tuple(data.shape)}")
    if not data.is_cuda:
        if info is None:
            info = jpeg_probe(data, restart=True)
            if info is None:
                raise StitchErrorBase("jpeg_decode: unsupported file (jpeg_probe returned None)")
        data = data.cuda()              # a blocking copy: the host tensor may be a temporary of this call
    if info is None:
        raise ValueError("jpeg_decode of a device tensor needs the JpegInfo of jpeg_probe")
    data = data.contiguous()
    H, W, ch = info.H, info.W, info.ncomp
    if out is None:
        out = torch.empty((H, W, ch), device=data.device, dtype=torch.uint8)
    if out.dtype != torch.uint8 or tuple(out.shape) != (H, W, ch) or (ch > 1 and out.stride(2) != 1) or (W > 1 and out.stride(1) != ch):
        raise ValueError(f"out: uint8 [{H},{W},{ch}] with dense pixels expected, got {out.dtype} {tuple(out.shape)} strides {out.stride()}")
    row_stride = out.stride(0) if H > 1 else W * ch
    need = jpeg_dec_workspace_bytes(info)
    if need == 0:
        raise StitchErrorBase(f"st_jpeg_decode_u8: unsupported frame {H}x{W}x{ch}, sampling {info.hs}x{info.vs}")
    if workspace is None:
        workspace = torch.empty((need,), device=data.device, dtype=torch.uint8)
    if status is None:
        status = torch.empty((1,), device=data.device, dtype=torch.int32)
    if status.dtype != torch.int32 or status.numel() != 1:
        raise ValueError("status: one int32 element expected")
    prm = _jpeg_dec_params(info)
    check(lib.st_jpeg_decode_u8(_p(data), data.numel(), C.byref(prm), _p(out), row_stride, _p(status), _pc(workspace),
                                workspace.numel() * workspace.element_size(), _stream()), "st_jpeg_decode_u8")
    return out, status


def masked_psnr_ssim(image1, final_warp_output, out=None):
    """evaluate.py:44-59 on the GPU: image1 [B,3,H,W], final_warp_output [B,6,H,W] -> fp64 [B,2] (psnr, ssim)."""
    B, _, H, W = image1.shape
    dev = image1.device
    valid = torch.empty((B, H, W), device=dev, dtype=torch.float32)
    mask = final_warp_output[:, 3:6]
    check(lib.st_channel_mean(_p(mask), final_warp_output.stride(0), _p(valid), B, 3, H, W, _stream()), "st_channel_mean")
    nblk = (3 * H * W + 255) // 256
    partial = torch.empty((2 * B * nblk,), device=dev, dtype=torch.float64)
    if out is None:
        out = torch.empty((B, 2), device=dev, dtype=torch.float64)
    assert out.dtype == torch.float64 and out.shape == (B, 2) and out.is_contiguous()
    check(lib.st_masked_psnr_ssim(_pc(image1), _p(final_warp_output), final_warp_output.stride(0), _p(valid), _p(partial), _p(out),
                                  B, H, W, _stream()), "st_masked_psnr_ssim")
    return out


# ---- composition stage (csrc/composition.hip) --------------------------------------------------
def resize_nearest_rows(x, out, B, H, W, Cc, oh, ow):
    check(lib.st_resize_nearest_rows(_p(x), _ld(x), _p(out), _ld(out), B, H, W, Cc, oh, ow, _stream()), "st_resize_nearest_rows")
    return out


def sub_rows(a, b, out):
    check(lib.st_sub_rows(_p(a), _ld(a), _p(b), _ld(b), _p(out), _ld(out), a.shape[0], a.shape[1], _stream()), "st_sub_rows")
    return out


def compose_blend(warp1, warp2, mask1, mask2, net_out, lm1, lm2, stitched):
    B, _, H, W = warp1.shape
    check(lib.st_compose_blend(_pc(warp1), _pc(warp2), _pc(mask1), _pc(mask2), _p(net_out), _ld(net_out), _pc(lm1), _pc(lm2),
                               _pc(stitched), B, H, W, _stream()), "st_compose_blend")
    return stitched


def compose_normalize(x, out):
    check(lib.st_compose_normalize(_pc(x), _pc(out), x.numel(), _stream()), "st_compose_normalize")
    return out


# ---- TPS post-pipeline (csrc/tps_pipeline.hip) ---------------------------------------------------
def flow_boxavg(flow, valid=None, k=11, negate=True):
    B, Cc, H, W = flow.shape
    out = torch.empty_like(flow)
    v = valid.float().contiguous() if valid is not None else None
    check(lib.st_flow_boxavg(_pc(flow), _p(v), _p(out), B, Cc, H, W, k, int(negate), _stream()), "st_flow_boxavg")
    return out


def sobel_magnitude(image):
    """image [1,C,H,W] -> [H,W]."""
    B, Cc, H, W = image.shape
    assert B == 1
    grad = torch.empty((H, W), device=image.device, dtype=torch.float32)
    check(lib.st_sobel_magnitude(_pc(image), _p(grad), Cc, H, W, _stream()), "st_sobel_magnitude")
    return grad


def range_argmax(grad, ranges):
    H, W = grad.shape
    out = torch.empty((ranges.shape[0],), device=grad.device, dtype=torch.int32)
    check(lib.st_range_argmax(_pc(grad), _pc(ranges), _p(out), ranges.shape[0], H, W, _stream()), "st_range_argmax")
    return out


def gather_points(planes, points_xy):
    """planes [P,H,W] fp32, points [n,2] int32 (x, y) -> [n,P]."""
    P, H, W = planes.shape
    n = points_xy.shape[0]
    out = torch.empty((n, P), device=planes.device, dtype=torch.float32)
    if n:
        check(lib.st_gather_points(_pc(planes), _pc(points_xy.contiguous()), _p(out), n, P, H, W, _stream()), "st_gather_points")
    return out


class SingularTPSError(StitchErrorBase):
    """the TPS system of the control points has no unique solution (the reference's torch.linalg.solve raises there)"""


def tps2_solve(sites, centers, values, mode=0):
    n = sites.shape[0]
    dev = sites.device
    work = torch.empty(((n + 3) * (n + 6),), device=dev, dtype=torch.float64)
    kw = torch.empty((n, 2), device=dev, dtype=torch.float32)
    aw = torch.empty((3, 2), device=dev, dtype=torch.float32)
    status = torch.zeros((1,), device=dev, dtype=torch.int32)
    check(lib.st_tps2_solve(_pc(sites), _pc(centers), _pc(values), _p(work), _p(kw), _p(aw), n, mode, _p(status), _stream()), "st_tps2_solve")
    if int(status.item()):                     # (the post-pipeline already round-trips to the host for its control points)
        raise SingularTPSError(f"singular TPS system: {n} control points with coincident or collinear sites")
    return kw, aw


def tps2_warp(img, points_a, points_b, kernel_scale=1.0, affine_scale=1.0, mode=0, align_corners=False, weights=None):
    """TPS warp of img [1,C,H,W] by the spline with f(points_a_i) = points_b_i.  mode 0 (kornia): (kw, aw) =
    get_tps_transform(points_a, points_b), kernel centres = points_b; mode 1 (pixel units): centres = points_a; mode 3: mode 1 on
    uint8-quantised data (taps truncated to 0..255 integers, result rounded and saturated: what cv2 sees in the reference)."""
    B, Cc, H, W = img.shape
    assert B == 1
    dev = img.device
    a, b = points_a.float().contiguous().to(dev), points_b.float().contiguous().to(dev)
    centers = b if (mode & 1) == 0 else a
    kw, aw = weights if weights is not None else tps2_solve(a, centers, b, mode & 1)
    out = torch.empty_like(img)
    check(lib.st_tps2_warp(_pc(img), _pc(centers), _pc(kw), _pc(aw), _p(out), Cc, H, W, b.shape[0], float(kernel_scale),
                           float(affine_scale), int(align_corners), mode, _stream()), "st_tps2_warp")
    return out


def rect_filter(x, k, is_max):
    """cv2.erode (is_max False) / cv2.dilate (True) with a k x k rectangle on [.., H, W] planes."""
    H, W = x.shape[-2:]
    planes = x.numel() // (H * W)
    tmp, out = torch.empty_like(x), torch.empty_like(x)
    check(lib.st_minmax_filter(_pc(x), _p(tmp), planes, H, W, k, int(is_max), 0, _stream()), "st_minmax_filter")
    check(lib.st_minmax_filter(_p(tmp), _p(out), planes, H, W, k, int(is_max), 1, _stream()), "st_minmax_filter")
    return out


def tps_mask_inv(warped_mask):
    B, Cc, H, W = warped_mask.shape
    assert B == 1
    inv = torch.empty((1, 1, H, W), device=warped_mask.device, dtype=torch.float32)
    check(lib.st_tps_mask_inv(_pc(warped_mask), _p(inv), Cc, H, W, _stream()), "st_tps_mask_inv")
    return inv


def tps_mix_blend(tps3, inv_clean, final_warp3, output1_3, mask1_3):
    _, _, H, W = tps3.shape
    dev = tps3.device
    tmask = torch.empty((1, 1, H, W), device=dev, dtype=torch.float32)
    mixmask = torch.empty((1, 1, H, W), device=dev, dtype=torch.float32)
    mix = torch.empty((1, 3, H, W), device=dev, dtype=torch.float32)
    blend = torch.empty((1, 3, H, W), device=dev, dtype=torch.uint8)
    check(lib.st_tps_mix_blend(_pc(tps3), _pc(inv_clean), _pc(final_warp3), _pc(output1_3), _pc(mask1_3), _p(tmask), _p(mix),
                               _p(mixmask), _p(blend), H, W, _stream()), "st_tps_mix_blend")
    return tmask, mix, mixmask, blend


# ---- mix_fn plug-ins (csrc/tps_pipeline.hip, second half) -----------------------------------------
def box_sum_cmp(plane, k, pad, out_hw, cmp):
    H, W = plane.shape[-2:]
    out = torch.empty((1, 1, out_hw[0], out_hw[1]), device=plane.device, dtype=torch.float32)
    check(lib.st_box_sum_cmp(_pc(plane), H, W, _p(out), out_hw[0], out_hw[1], k, pad, cmp, _stream()), "st_box_sum_cmp")
    return out


def dilate_thin_area_plane(mask0, dilation_kernel_size=8, thickening_kernel_size=8):
    """core/inference/utils.py:125-160 on one plane [1,1,H,W] -> (result [1,1,H,W], result >= 1 as float)."""
    H, W = mask0.shape[-2:]
    k, p = dilation_kernel_size, dilation_kernel_size // 2
    ho, wo = H + 2 * p - k + 1, W + 2 * p - k + 1
    er = box_sum_cmp(mask0, k, p, (ho, wo), 1)
    di = box_sum_cmp(er, k, p, (H, W), 2)
    thick, thin = torch.empty_like(mask0), torch.empty_like(mask0)
    check(lib.st_mix_plane_op(_pc(mask0), _pc(di), _p(thick), _p(thin), mask0.numel(), 0, 0.0, _stream()), "st_mix_plane_op")
    k2, p2 = thickening_kernel_size, thickening_kernel_size // 2
    dt = box_sum_cmp(thin, k2, p2, (H, W), 2)
    res, ge1 = torch.empty_like(mask0), torch.empty_like(mask0)
    check(lib.st_mix_plane_op(_pc(thick), _pc(dt), _p(res), _p(ge1), mask0.numel(), 1, 0.0, _stream()), "st_mix_plane_op")
    return res, ge1


def plane_threshold(a, thr):
    out = torch.empty_like(a)
    check(lib.st_mix_plane_op(_pc(a), None, _p(out), None, a.numel(), 2, float(thr), _stream()), "st_mix_plane_op")
    return out


def mix_stage_a(final_warp, occ, mask1, tps, tmask, method):
    _, _, H, W = final_warp.shape
    tfw, tfwm = torch.empty_like(final_warp), torch.empty_like(final_warp)
    iam0 = torch.empty((1, 1, H, W), device=final_warp.device, dtype=torch.float32)
    check(lib.st_mix_stage_a(_pc(final_warp), _pc(occ), _pc(mask1), _pc(tps), _pc(tmask), _p(tfw), _p(tfwm), _p(iam0), H, W, method,
                             _stream()), "st_mix_stage_a")
    return tfw, tfwm, iam0


def mix_stage_b(iam, dil, mask1, tfw, output1):
    _, _, H, W = tfw.shape
    only1 = torch.empty_like(tfw)
    other0 = torch.empty((1, 1, H, W), device=tfw.device, dtype=torch.float32)
    check(lib.st_mix_stage_b(_pc(iam), _pc(dil), _pc(mask1), _pc(tfw), _pc(output1), _p(only1), _p(other0), H, W, _stream()),
          "st_mix_stage_b")
    return only1, other0


def mix_mul_mask(img3, mask=None, invert=False, clip=False):
    _, _, H, W = img3.shape
    out = torch.empty_like(img3)
    check(lib.st_mix_mul_mask(_pc(img3), _pc(mask) if mask is not None else None, _p(out), H, W, int(invert), int(clip), _stream()),
          "st_mix_mul_mask")
    return out


def blend_pair(output1, mask1, output2, mask2):
    _, _, H, W = output1.shape
    blend = torch.empty((1, 3, H, W), device=output1.device, dtype=torch.uint8)
    check(lib.st_blend_pair(_pc(output1), _pc(mask1), _pc(output2), _pc(mask2), mask2.shape[1], _p(blend), H, W, _stream()), "st_blend_pair")
    return blend


# ---- Telea inpainting (cv_inpainter) ------------------------------------------------------------
INPAINT_MAX_RADIUS = 88


def inpaint_prep(img3, mask):
    """cv_inpainter's preprocessing on the GPU: img3 fp32 [3,H,W] -> uint8 [H,W,3] (clamped to 0..255, truncated); mask fp32
    [1 or 3,H,W] -> uint8 [H,W] nonzero where to fill (x255 + clamp when its max is <= 1.1, truncation, PIL's integer luma)."""
    if img3.dim() != 3 or img3.shape[0] != 3 or img3.dtype != torch.float32:
        raise ValueError(f"fp32 [3,H,W] image expected, got {img3.dtype} {tuple(img3.shape)}")
    _, H, W = img3.shape
    if mask.dim() != 3 or mask.shape[0] not in (1, 3) or tuple(mask.shape[1:]) != (H, W) or mask.dtype != torch.float32:
        raise ValueError(f"fp32 [1 or 3,{H},{W}] mask expected, got {mask.dtype} {tuple(mask.shape)}")
    dev = img3.device
    img_hwc = torch.empty((H, W, 3), device=dev, dtype=torch.uint8)
    mask_u8 = torch.empty((H, W), device=dev, dtype=torch.uint8)
    scratch = torch.empty((1,), device=dev, dtype=torch.int32)
    check(lib.st_inpaint_prep(_pc(img3), _pc(mask), mask.shape[0], _p(img_hwc), _p(mask_u8), _p(scratch), H, W, _stream()),
          "st_inpaint_prep")
    return img_hwc, mask_u8


def inpaint_telea(img, mask, radius=64, return_fields=False):
    """Telea inpainting (cv2.inpaint(img, mask, radius, cv2.INPAINT_TELEA) restated ring by ring: README.md, cv_inpainter):
    img uint8 [H,W,3], mask uint8 / bool [H,W] (nonzero = fill) -> uint8 [H,W,3].  One device -> host read (the ring sizes),
    then one launch per ring on the current stream.  return_fields: also the ring index d (int32 [H,W], 0 on the known set) and
    the arrival time T (fp32 [H,W]) -- None when no kernel filled anything (no hole, or no known pixel: image returned as is)."""
    if img.dim() != 3 or img.shape[2] != 3 or img.dtype != torch.uint8:
        raise ValueError(f"uint8 [H,W,3] image expected, got {img.dtype} {tuple(img.shape)}")
    H, W, _ = img.shape
    if mask.dtype == torch.bool:
        mask = mask.to(torch.uint8)
    if mask.dtype != torch.uint8 or tuple(mask.shape) != (H, W):
        raise ValueError(f"uint8 [{H},{W}] mask expected, got {mask.dtype} {tuple(mask.shape)}")
    if not 1 <= int(radius) <= INPAINT_MAX_RADIUS:
        raise ValueError(f"radius must be in 1..{INPAINT_MAX_RADIUS}, got {radius}")
    if mask.device != img.device:
        raise ValueError("image and mask must be on the same device")
    dev = img.device
    nbytes = C.c_int64()
    check(lib.st_inpaint_telea_workspace(H, W, int(radius), C.byref(nbytes)), "st_inpaint_telea_workspace")
    work = torch.empty((nbytes.value,), device=dev, dtype=torch.uint8)
    counts = torch.empty((H + W + 1,), device=dev, dtype=torch.int32)
    check(lib.st_inpaint_telea_rings(_pc(img), _pc(mask), H, W, int(radius), _p(work), nbytes.value, _p(counts), _stream()),
          "st_inpaint_telea_rings")
    host = counts.cpu()                                  # the one device -> host read: ring sizes
    nz = torch.nonzero(host).flatten()
    nrings = int(nz[-1]) if len(nz) else 0
    if int(host[0]) == 0 or nrings == 0:                 # no known pixel / nothing to fill: no fill kernel runs
        out = img.clone()
        return (out, None, None) if return_fields else out
    ring_counts = (C.c_int32 * (nrings + 1))(*host[:nrings + 1].tolist())
    out = torch.empty_like(img)
    d = torch.empty((H, W), device=dev, dtype=torch.int32) if return_fields else None
    T = torch.empty((H, W), device=dev, dtype=torch.float32) if return_fields else None
    check(lib.st_inpaint_telea_fill(ring_counts, nrings, H, W, int(radius), _p(work), nbytes.value, _p(out), _p(d), _p(T), _stream()),
          "st_inpaint_telea_fill")
    return (out, d, T) if return_fields else out


def inpaint_disc_size(radius=64):
    """number of offsets 0 < |r| <= radius one filled pixel gathers over"""
    from math import isqrt
    return sum(2 * isqrt(radius * radius - y * y) + 1 for y in range(-radius, radius + 1)) - 1


# ---- tps_method="other" (csrc/tps_other.hip) -----------------------------------------------------
REMAP_MAX_SIDE = 32760          # cv2.remap keeps tap coordinates in int16: a source side past this is not restated


def cubic_remap_table():
    """cv2.remap's INTER_CUBIC 8U coefficient table (OpenCV initInterTab2D(INTER_CUBIC, fixpt=true)), int16 [32*32, 16]: row
    fy*32 + fx, entry k1*4 + k2 = weight of tap (sy-1+k1, sx-1+k2) in units of 2^-15.  The one place the table is built: the
    device upload and the test restatement both call it.  Not checked against OpenCV itself (not importable here)."""
    import numpy as np
    f32 = np.float32
    A = f32(-0.75)
    t = (np.arange(32, dtype=f32) * f32(1.0 / 32)).astype(f32)
    one = f32(1)
    c0 = ((A * (t + one) - f32(5) * A) * (t + one) + f32(8) * A) * (t + one) - f32(4) * A
    c1 = ((A + f32(2)) * t - (A + f32(3))) * t * t + one
    c2 = ((A + f32(2)) * (one - t) - (A + f32(3))) * (one - t) * (one - t) + one
    c3 = one - c0 - c1 - c2
    c = np.stack([c0, c1, c2, c3], 1).astype(f32)                                  # [32 fractions, 4 taps]
    prod = (c[:, None, :, None] * c[None, :, None, :]).astype(f32)                # [fy, fx, k1, k2] = cy[k1] * cx[k2] in fp32
    # cvRound (half to even) saturated to int16: fraction (0, 0) has cy[1] * cx[1] = 1 -> 32767, and the correction below puts the
    # missing 1 on tap (2, 2) (a copy stays exact: 32767 v + v' + 2^14 >> 15 == v for |v' - v| <= 255)
    tab = np.clip(np.rint(prod * f32(32768)), -32768, 32767).astype(np.int32).reshape(32 * 32, 16)
    for row in tab:
        diff = int(row.sum()) - 32768
        if diff == 0:
            continue
        mk = Mk = 2 * 4 + 2                                                        # scan the centre 2 x 2 from (2, 2)
        for k1 in (2, 3):
            for k2 in (2, 3):
                k = k1 * 4 + k2
                if row[k] < row[mk]:
                    mk = k
                elif row[k] > row[Mk]:
                    Mk = k
        if diff < 0:
            row[Mk] -= diff
        else:
            row[mk] -= diff
    return tab.astype(np.int16)


_REMAP_TABLES = {}


def _remap_table(dev):
    """cubic_remap_table() uploaded once per device"""
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _REMAP_TABLES:
        _REMAP_TABLES[key] = torch.from_numpy(cubic_remap_table()).to(dev).contiguous()
    return _REMAP_TABLES[key]


def tps_other_solve(c_src, c_dst):
    """the two splines of tps_method="other": f(c_dst_i) = c_src_i - c_dst_i (float32 [n,2] each, normalised coordinates),
    U(r) = r^2 ln(r + 1e-6), solved in fp64 -> (kernel_w [n,2], affine_w [3,2]) float32.  Raises SingularTPSError."""
    n = c_dst.shape[0]
    dev = c_dst.device
    sites = c_dst.float().contiguous()
    delta = (c_src.float().to(dev) - sites).contiguous()                  # float32, as the reference subtracts
    work = torch.empty(((n + 3) * (n + 6),), device=dev, dtype=torch.float64)
    kw = torch.empty((n, 2), device=dev, dtype=torch.float32)
    aw = torch.empty((3, 2), device=dev, dtype=torch.float32)
    status = torch.zeros((1,), device=dev, dtype=torch.int32)
    check(lib.st_tps_other_solve(_pc(sites), _pc(delta), _p(work), _p(kw), _p(aw), n, _p(status), _stream()), "st_tps_other_solve")
    if int(status.item()):
        raise SingularTPSError(f"singular TPS system: {n} control points with collinear sites")
    return kw, aw


def tps_other_maps(points_src, points_dst, H, W, weights=None):
    """cv2.remap maps (mapx, mapy) float32 [H,W] of tps_method="other" (other_tps.py tps_theta_from_points / tps_grid /
    tps_grid_to_remap) for float32 normalised points [n,2] on the same device.  Coincident points_dst keep their first occurrence.
    weights: (kernel_w [n,2], affine_w [3,2]) to use instead of the fit (kernel_w[0] is replaced by the reduced form)."""
    dev = points_dst.device
    c_src, c_dst = points_src.float().to(dev), points_dst.float()
    if weights is None:
        import numpy as np
        _, first = np.unique(c_dst.cpu().numpy(), axis=0, return_index=True)
        if len(first) < c_dst.shape[0]:
            keep = torch.from_numpy(np.sort(first)).to(dev)
            c_src, c_dst = c_src[keep], c_dst[keep]
        if c_dst.shape[0] < 3:
            raise SingularTPSError(f"singular TPS system: {c_dst.shape[0]} distinct control points")
        weights = tps_other_solve(c_src, c_dst)
    kw, aw = (w.float().contiguous().to(dev) for w in weights)
    c_dst = c_dst.contiguous()
    mapx = torch.empty((H, W), device=dev, dtype=torch.float32)
    mapy = torch.empty((H, W), device=dev, dtype=torch.float32)
    check(lib.st_tps_other_maps(_pc(c_dst), _pc(kw), _pc(aw), c_dst.shape[0], H, W, _p(mapx), _p(mapy), _stream()), "st_tps_other_maps")
    return mapx, mapy


def remap_cubic(planes, mapx, mapy):
    """cv2.remap(INTER_CUBIC, BORDER_CONSTANT 0) of the uint8 image the planes truncate to: planes float32 [P,Hs,Ws] (or
    [1,P,Hs,Ws]), maps float32 [H,W] -> float32 [P,H,W] (or [1,P,H,W]) holding 0..255."""
    batched = planes.dim() == 4
    if batched:
        if planes.shape[0] != 1:
            raise ValueError(f"batch 1 expected, got {tuple(planes.shape)}")
        planes = planes[0]
    if planes.dim() != 3 or planes.dtype != torch.float32:
        raise ValueError(f"float32 [P,H,W] planes expected, got {planes.dtype} {tuple(planes.shape)}")
    if mapx.shape != mapy.shape or mapx.dim() != 2 or mapx.dtype != torch.float32 or mapy.dtype != torch.float32:
        raise ValueError(f"float32 [H,W] maps expected, got {tuple(mapx.shape)} / {tuple(mapy.shape)}")
    if mapx.device != planes.device or mapy.device != planes.device:
        raise ValueError("planes and maps must be on the same device")
    P, Hs, Ws = planes.shape
    H, W = mapx.shape
    out = torch.empty((P, H, W), device=planes.device, dtype=torch.float32)
    check(lib.st_remap_cubic_u8(_pc(planes), P, Hs, Ws, _pc(mapx), _pc(mapy), H, W, _p(_remap_table(planes.device)), _p(out), _stream()),
          "st_remap_cubic_u8")
    return out[None] if batched else out


# ---- TransRef inpainter (mix_methods/utils/transref_inpainter.py, stitch_amd/transref.py) --------------------------------------
TR_ATTENTION_D = (32, 64, 80, 128, 160, 256)


def tr_attention(q, k, v, out, heads, D, scale):
    """out[:, h D:(h+1) D] = softmax(scale q_h k_h^T) v_h for every head h (st_tr_attention): 2-D row-major views, last dim contiguous."""
    check(lib.st_tr_attention(_p(q), _ld(q), _p(k), _ld(k), _p(v), _ld(v), _p(out), _ld(out), heads, q.shape[0], k.shape[0], D,
                              float(scale), _stream()), "st_tr_attention")
    return out


def tr_deform_im2col(x, off, cols, H, W):
    """mmcv DeformConv2d (3x3, pad 1) sampling: x [H W, C] view, off [H W, >=18] view -> cols [H W, 9 C] dense."""
    Cc = x.shape[1]
    assert cols.shape == (H * W, 9 * Cc) and cols.is_contiguous()
    check(lib.st_tr_deform_im2col(_p(x), _ld(x), _p(off), _ld(off), _p(cols), H, W, Cc, _stream()), "st_tr_deform_im2col")
    return cols


def tr_phase_interleave(phases, out, H, W, res=None):
    """phases [4, H W, C] dense -> out [(2H)(2W), C] view (+ res, same geometry)."""
    Cc = phases.shape[-1]
    assert phases.is_contiguous() and phases.numel() == 4 * H * W * Cc
    check(lib.st_tr_phase_interleave(_p(phases), _p(out), _ld(out), _p(res), _ld(res) if res is not None else 0, H, W, Cc, _stream()),
          "st_tr_phase_interleave")
    return out


def tr_dwconv3x3_gelu(x, w9c, bias, out, H, W):
    check(lib.st_tr_dwconv3x3_gelu(_p(x), _ld(x), _pc(w9c), _pc(bias), _p(out), _ld(out), H, W, x.shape[1], _stream()),
          "st_tr_dwconv3x3_gelu")
    return out


def tr_add(a, b, out):
    check(lib.st_tr_add(_p(a), _ld(a), _p(b), _ld(b), _p(out), _ld(out), a.shape[0], a.shape[1], _stream()), "st_tr_add")
    return out


def tr_prep(img3, ctl3, out6):
    check(lib.st_tr_prep(_pc(img3), _pc(ctl3), _pc(out6), img3[0].numel(), _stream()), "st_tr_prep")
    return out6


def tr_pack(rs6, mask0, x6, ref3, detail3):
    check(lib.st_tr_pack(_pc(rs6), _pc(mask0), _pc(x6), _pc(ref3), _pc(detail3), mask0.numel(), _stream()), "st_tr_pack")


def tr_blend(out3, detail3, mask, fake3):
    check(lib.st_tr_blend(_pc(out3), _pc(detail3), _pc(mask), mask.shape[0], _pc(fake3), detail3[0].numel(), _stream()), "st_tr_blend")
    return fake3


def tr_to_u8(x, out):
    check(lib.st_tr_to_u8(_pc(x), _pc(out), x.numel(), _stream()), "st_tr_to_u8")
    return out


# ---- multiband_fusion: Laplacian-pyramid seam blend (csrc/multiband.hip; README.md, multiband_fusion) ------------------------------
MULTIBAND_MAX_SIDE = 4096
MULTIBAND_MAX_LEVELS = 16


def edt_sq(mask, border_is_site=True, return_index=False):
    """Exact squared Euclidean distance transform on the GPU: mask [H,W] (bool, or any dtype: nonzero = inside) -> int32 [H,W], the squared
    distance of every pixel to the nearest pixel with mask == 0; with ``border_is_site`` the one-pixel ring round the canvas counts as
    zero too.  Without any site the distance is INT32_MAX.  ``return_index``: also int32 [H,W], the lowest row-major index among the
    canvas pixels at that distance (-1 when there is none, or when only the ring is that near)."""
    if mask.dim() != 2:
        raise ValueError(f"mask [H,W] expected, got {tuple(mask.shape)}")
    H, W = mask.shape
    if not (1 <= H <= MULTIBAND_MAX_SIDE and 1 <= W <= MULTIBAND_MAX_SIDE):
        raise ValueError(f"sides must be in 1..{MULTIBAND_MAX_SIDE}, got {H} x {W}")
    m = (mask != 0).to(torch.uint8).contiguous()
    D = torch.empty((H, W), dtype=torch.int32, device=mask.device)
    idx = torch.empty((H, W), dtype=torch.int32, device=mask.device) if return_index else None
    check(lib.st_edt_sq_u8(_pc(m), H, W, int(bool(border_is_site)), _p(D), _p(idx), _stream()), "st_edt_sq_u8")
    return (D, idx) if return_index else D


def multiband_workspace_bytes(H, W, levels):
    """bytes of workspace `multiband_blend` needs for an H x W canvas; 0 for a shape or level count outside the contract"""
    return int(lib.st_multiband_workspace_bytes(int(H), int(W), int(levels)))


def multiband_blend(img1, img2, mask1, mask2, levels=5, workspace=None, seam=None):
    """Multi-band (Laplacian pyramid) blend of two warped images along the distance-transform seam of their masks (README.md,
    multiband_fusion): img1, img2 fp32 [1,3,H,W] (clamped to 0..255 and truncated, as the saver does), mask1, mask2 fp32 [1,1,H,W] or
    [1,3,H,W] (channel 0 > 0.5) -> fp32 [1,3,H,W], 0 outside the union.  ``levels`` = REDUCE steps (0 = hard seam).  ``workspace``: a
    uint8 device tensor of at least `multiband_workspace_bytes` bytes, 16-byte aligned (default: allocated here); all launches go to the
    current stream and nothing is read back.  ``seam``: the (side, info) pair of `seam_dp` on the same canvas: where info says the seam is
    valid, the overlap belongs to image 1 where side is set, instead of where image 1's border is the farther one (decided on the device)."""
    if img1.dim() != 4 or img1.shape[0] != 1 or img1.shape[1] != 3 or img2.shape != img1.shape:
        raise ValueError(f"img1, img2 [1,3,H,W] expected, got {tuple(img1.shape)} and {tuple(img2.shape)}")
    H, W = img1.shape[2:]
    if seam is not None:
        side, info = seam
        if side.dtype != torch.uint8 or tuple(side.shape) != (H, W) or info.dtype != torch.int32 or tuple(info.shape) != (4,):
            raise ValueError(f"seam = (side uint8 [{H},{W}], info int32 [4]) expected, got {side.dtype} {tuple(side.shape)}, {info.dtype} {tuple(info.shape)}")
    for m in (mask1, mask2):
        if m.dim() != 4 or m.shape[0] != 1 or m.shape[1] not in (1, 3) or tuple(m.shape[2:]) != (H, W):
            raise ValueError(f"mask [1,1,{H},{W}] or [1,3,{H},{W}] expected, got {tuple(m.shape)}")
    for t in (img1, img2, mask1, mask2):
        if t.dtype != torch.float32:
            raise ValueError(f"float32 tensors expected, got {t.dtype}")
    need = multiband_workspace_bytes(H, W, levels)
    if need == 0:
        raise ValueError(f"sides must be in 1..{MULTIBAND_MAX_SIDE} and levels in 0..{MULTIBAND_MAX_LEVELS}, got {H} x {W}, levels {levels}")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=img1.device)
    out = torch.empty_like(img1, memory_format=torch.contiguous_format)
    mask1, mask2 = mask1[:, :1].contiguous(), mask2[:, :1].contiguous()         # channel 0 (no copy unless the mask is a strided view)
    if seam is not None:
        check(lib.st_multiband_blend_seam(_pc(img1), _pc(img2), _pc(mask1), _pc(mask2), H, W, int(levels), _pc(seam[0]), _pc(seam[1]), _p(out),
                                          _p(workspace), workspace.numel() * workspace.element_size(), _stream()), "st_multiband_blend_seam")
        return out
    check(lib.st_multiband_blend(_pc(img1), _pc(img2), _pc(mask1), _pc(mask2), H, W, int(levels), _p(out), _p(workspace),
                                 workspace.numel() * workspace.element_size(), _stream()), "st_multiband_blend")
    return out


# ---- exposure compensation: overlap gains in front of multiband_blend (csrc/exposure.hip; README.md, exposure compensation) ---------
EXPOSURE_BLOCKS = (8, 16, 32, 64)
EXPOSURE_MODES = dict(gain=0, blocks=1)
EXPOSURE_MAX_SMOOTH = 8


def _exposure_operands(img1, img2, mask1, mask2, block):
    """the checks of `multiband_blend` on the shared operands; returns H, W and the masks' channel 0 as dense planes"""
    if img1.dim() != 4 or img1.shape[0] != 1 or img1.shape[1] != 3 or img2.shape != img1.shape:
        raise ValueError(f"img1, img2 [1,3,H,W] expected, got {tuple(img1.shape)} and {tuple(img2.shape)}")
    H, W = img1.shape[2:]
    masks = [m for m in (mask1, mask2) if m is not None]
    for m in masks:
        if m.dim() != 4 or m.shape[0] != 1 or m.shape[1] not in (1, 3) or tuple(m.shape[2:]) != (H, W):
            raise ValueError(f"mask [1,1,{H},{W}] or [1,3,{H},{W}] expected, got {tuple(m.shape)}")
    for t in [img1, img2] + masks:
        if t.dtype != torch.float32:
            raise ValueError(f"float32 tensors expected, got {t.dtype}")
    if block not in EXPOSURE_BLOCKS:
        raise ValueError(f"block must be one of {EXPOSURE_BLOCKS}, got {block}")
    if not (1 <= H <= MULTIBAND_MAX_SIDE and 1 <= W <= MULTIBAND_MAX_SIDE):
        raise ValueError(f"sides must be in 1..{MULTIBAND_MAX_SIDE}, got {H} x {W}")
    return H, W, [m[:, :1].contiguous() for m in masks]         # channel 0 (no copy unless the mask is a strided view)


def exposure_workspace_bytes(H, W, block=32):
    """bytes of workspace `exposure_compensate` needs for an H x W canvas; 0 for a shape or block outside the contract"""
    return int(lib.st_exposure_workspace_bytes(int(H), int(W), int(block)))


def exposure_stats(img1, img2, mask1, mask2, block=32):
    """The tile statistics of `exposure_compensate` alone: int32 [Th,Tw,9] = per `block` x `block` tile N, S1[R,G,B,Y], S2[R,G,B,Y] over
    the overlap (mask1 > 0.5 and mask2 > 0.5) of the truncated pixels; Y = (19595 R + 38470 G + 7471 B + 0x8000) >> 16."""
    H, W, (k1, k2) = _exposure_operands(img1, img2, mask1, mask2, block)
    rec = torch.empty((-(-H // block), -(-W // block), 9), dtype=torch.int32, device=img1.device)
    check(lib.st_exposure_stats(_pc(img1), _pc(img2), _pc(k1), _pc(k2), H, W, int(block), _p(rec), _stream()), "st_exposure_stats")
    return rec


def exposure_apply(img1, img2, tables, block=32, channels=False, out=None):
    """The apply step of `exposure_compensate` alone on caller-given gain tables: fp32 [1,2,Th,Tw] (``channels=False``) or [3,2,Th,Tw]
    (R, G, B), second axis = (image 1, image 2), any Th, Tw >= 1 (indices are clamped to the table) -> (out1, out2), fp32 [1,3,H,W],
    min(floor(p g + 0.5), 255) with g interpolated bilinearly between the tile centres.  ``out``: a pair of tensors to write (each may be
    its own input: in place)."""
    H, W, _ = _exposure_operands(img1, img2, None, None, block)
    sets = 3 if channels else 1
    if tables.dim() != 4 or tables.shape[0] != sets or tables.shape[1] != 2 or tables.dtype != torch.float32:
        raise ValueError(f"tables float32 [{sets},2,Th,Tw] expected, got {tables.dtype} {tuple(tables.shape)}")
    out1, out2 = out if out is not None else (torch.empty_like(img1, memory_format=torch.contiguous_format),
                                              torch.empty_like(img2, memory_format=torch.contiguous_format))
    check(lib.st_exposure_apply(_pc(img1), _pc(img2), _pc(tables), tables.shape[2], tables.shape[3], H, W, int(block), int(bool(channels)),
                                _pc(out1), _pc(out2), _stream()), "st_exposure_apply")
    return out1, out2


def exposure_compensate(img1, img2, mask1, mask2, mode="gain", block=32, channels=False, min_count=None, smooth=2, sigma_n=10.0, sigma_g=0.1,
                        workspace=None, return_gains=False, out=None):
    """Gain compensation of two warped images from their overlap (README.md, exposure compensation), for the operands of
    `multiband_blend`: img1, img2 fp32 [1,3,H,W] (clamped to 0..255 and truncated, as the saver does), mask1, mask2 fp32 [1,1,H,W] or
    [1,3,H,W] (channel 0 > 0.5) -> (out1, out2), fp32 [1,3,H,W], integer-valued, every pixel written.  ``mode``: "gain" = one pair of gains
    from the global overlap sums, "blocks" = a pair per ``block`` x ``block`` tile with the global pair as prior (tiles with fewer than
    ``min_count`` overlap pixels, default block^2 / 8, keep it), smoothed ``smooth`` times.  ``channels``: gains per R, G, B instead of
    one from the integer luma.  ``return_gains``: also the tables the apply step read, fp32 [sets,2,Th,Tw] ([sets,2,1,1] in "gain").
    ``workspace``: a uint8 device tensor of at least `exposure_workspace_bytes` bytes, 16-byte aligned (default: allocated here);
    ``out``: a pair of tensors to write (each may be its own input).  All launches go to the current stream and nothing is read back."""
    H, W, (k1, k2) = _exposure_operands(img1, img2, mask1, mask2, block)
    if mode not in EXPOSURE_MODES:
        raise ValueError(f"mode must be one of {tuple(EXPOSURE_MODES)}, got {mode!r}")
    if not 0 <= smooth <= EXPOSURE_MAX_SMOOTH:
        raise ValueError(f"smooth must be in 0..{EXPOSURE_MAX_SMOOTH}, got {smooth}")
    if min_count is None:
        min_count = block * block // 8
    if min_count < 0:
        raise ValueError(f"min_count must not be negative, got {min_count}")
    for name, v in (("sigma_n", sigma_n), ("sigma_g", sigma_g)):
        if not (v > 0 and v < float("inf")):
            raise ValueError(f"{name} must be positive and finite, got {v}")
    need = exposure_workspace_bytes(H, W, block)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=img1.device)
    out1, out2 = out if out is not None else (torch.empty_like(img1, memory_format=torch.contiguous_format),
                                              torch.empty_like(img2, memory_format=torch.contiguous_format))
    sets = 3 if channels else 1
    th, tw = (-(-H // block), -(-W // block)) if mode == "blocks" else (1, 1)
    gains = torch.empty((sets, 2, th, tw), dtype=torch.float32, device=img1.device) if return_gains else None
    check(lib.st_exposure_compensate(_pc(img1), _pc(img2), _pc(k1), _pc(k2), H, W, EXPOSURE_MODES[mode], int(block), int(bool(channels)), int(min_count),
                                     int(smooth), float(sigma_n), float(sigma_g), _pc(out1), _pc(out2), _p(gains), _p(workspace),
                                     workspace.numel() * workspace.element_size(), _stream()), "st_exposure_compensate")
    return (out1, out2, gains) if return_gains else (out1, out2)


# ---- seam_dp: a minimum-difference seam for the ownership of multiband_blend (csrc/seam.hip; README.md, seam_dp) ---------------------
SEAM_ORIENTATIONS = dict(auto=0, vertical=1, horizontal=2)
SEAM_FIRST = {"auto": 0, 1: 1, 2: 2}


def _seam_operands(img1, img2, mask1, mask2):
    """the checks of `multiband_blend` on the shared operands; returns H, W and the masks' channel 0 as dense planes"""
    if img1.dim() != 4 or img1.shape[0] != 1 or img1.shape[1] != 3 or img2.shape != img1.shape:
        raise ValueError(f"img1, img2 [1,3,H,W] expected, got {tuple(img1.shape)} and {tuple(img2.shape)}")
    H, W = img1.shape[2:]
    for m in (mask1, mask2):
        if m.dim() != 4 or m.shape[0] != 1 or m.shape[1] not in (1, 3) or tuple(m.shape[2:]) != (H, W):
            raise ValueError(f"mask [1,1,{H},{W}] or [1,3,{H},{W}] expected, got {tuple(m.shape)}")
    for t in (img1, img2, mask1, mask2):
        if t.dtype != torch.float32:
            raise ValueError(f"float32 tensors expected, got {t.dtype}")
    if not (1 <= H <= MULTIBAND_MAX_SIDE and 1 <= W <= MULTIBAND_MAX_SIDE):
        raise ValueError(f"sides must be in 1..{MULTIBAND_MAX_SIDE}, got {H} x {W}")
    return H, W, mask1[:, :1].contiguous(), mask2[:, :1].contiguous()         # channel 0 (no copy unless the mask is a strided view)


def seam_workspace_bytes(H, W):
    """bytes of workspace `seam_dp` needs for an H x W canvas; 0 for a shape outside the contract"""
    return int(lib.st_seam_workspace_bytes(int(H), int(W)))


def seam_cost(img1, img2, mask1, mask2):
    """The cost plane of `seam_dp` alone, int32 [H,W]: 1 + sum over R, G, B of |p1 - p2| of the truncated pixels inside the overlap, 1
    outside both masks, 2^18 where exactly one mask is set."""
    H, W, k1, k2 = _seam_operands(img1, img2, mask1, mask2)
    cost = torch.empty((H, W), dtype=torch.int32, device=img1.device)
    check(lib.st_seam_cost(_pc(img1), _pc(img2), _pc(k1), _pc(k2), H, W, _p(cost), _stream()), "st_seam_cost")
    return cost


def seam_dp(img1, img2, mask1, mask2, orientation="auto", first="auto", workspace=None, return_path=False):
    """A minimum-cost monotone seam through the overlap of two warped images (README.md, seam_dp), on the operands of `multiband_blend`
    -> (side, info[, path]).  side uint8 [H,W]: 1 where the pixel lies on image 1's side of the seam (every canvas pixel; all ones
    without a valid seam).  info int32 [4] on the device: valid, orientation (1 vertical: one column per row; 2 horizontal), first (the
    image that owns the low-coordinate side), path cost.  ``orientation`` "auto" / "vertical" / "horizontal" and ``first`` "auto" / 1 / 2:
    auto decides from the centroids of the two exclusive regions.  ``return_path``: also int32 [max(H,W)], the seam position per line, -1
    behind the last line.  ``workspace``: a uint8 device tensor of at least `seam_workspace_bytes` bytes, 16-byte aligned (default:
    allocated here).  All launches go to the current stream and nothing is read back; (side, info) is what `multiband_blend(seam=...)` takes."""
    H, W, k1, k2 = _seam_operands(img1, img2, mask1, mask2)
    if orientation not in SEAM_ORIENTATIONS:
        raise ValueError(f"orientation must be one of {tuple(SEAM_ORIENTATIONS)}, got {orientation!r}")
    if first not in SEAM_FIRST:
        raise ValueError(f"first must be one of {tuple(SEAM_FIRST)}, got {first!r}")
    if workspace is None:
        workspace = torch.empty(seam_workspace_bytes(H, W), dtype=torch.uint8, device=img1.device)
    side = torch.empty((H, W), dtype=torch.uint8, device=img1.device)
    info = torch.empty(4, dtype=torch.int32, device=img1.device)
    path = torch.empty(max(H, W), dtype=torch.int32, device=img1.device) if return_path else None
    check(lib.st_seam_dp(_pc(img1), _pc(img2), _pc(k1), _pc(k2), H, W, SEAM_ORIENTATIONS[orientation], SEAM_FIRST[first], _p(side), _p(path), _p(info),
                         _p(workspace), workspace.numel() * workspace.element_size(), _stream()), "st_seam_dp")
    return (side, info, path) if return_path else (side, info)


# ---- seam_gc: a minimum cut over the overlap for the same place (csrc/seam_gc.hip; README.md, seam_gc) --------------------------------
SEAM_GC_MAX_ROUNDS = 2048                    # at least 8 x the most rounds any measured scene needed (README.md, seam_gc; profiles/seam_gc_bench.json)
SEAM_GC_PUSH_SWEEPS = 32                     # push / gather sweeps per round (csrc/seam_gc.hip)


def seam_gc_workspace_bytes(H, W):
    """bytes of workspace `seam_gc` needs for an H x W canvas; 0 for a shape outside the contract"""
    return int(lib.st_seam_gc_workspace_bytes(int(H), int(W)))


def seam_gc(img1, img2, mask1, mask2, workspace=None, max_rounds=None, return_stats=False):
    """A minimum cut over the overlap of two warped images (README.md, seam_gc), on the operands of `multiband_blend` and `seam_dp`
    -> (side, info[, stats]).  side uint8 [H,W]: 0 on the overlap pixels that fall to image 2 -- those that can still reach the sink under
    a maximum flow, the smallest sink side among all minimum cuts -- and 1 at every other canvas pixel (all ones without a valid cut).  info
    int32 [4] on the device: valid, 3, cut >> 31, cut & (2^31 - 1).  (side, info) is what `multiband_blend(seam=...)` takes.
    ``workspace``: a uint8 device tensor of at least `seam_gc_workspace_bytes` bytes, 16-byte aligned (default: allocated here).
    The number of push-relabel rounds depends on the data: after every round the status record (32 bytes) is read back from the device,
    so unlike `seam_dp` the call synchronises with the host and cannot be captured into a hipGraph as a whole.  ``max_rounds`` (default
    `SEAM_GC_MAX_ROUNDS`; 0 is allowed) bounds the rounds; when they do not suffice a warning is issued and info says not valid, with side
    all ones, so the blend keeps its distance seam.  ``return_stats``: also a dict with `converged`, `rounds`, `sweeps` (push / gather
    sweeps), `label_launches` and `host_reads`."""
    H, W, k1, k2 = _seam_operands(img1, img2, mask1, mask2)
    max_rounds = SEAM_GC_MAX_ROUNDS if max_rounds is None else int(max_rounds)
    if max_rounds < 0:
        raise ValueError(f"max_rounds must be >= 0, got {max_rounds}")
    if workspace is None:
        workspace = torch.empty(seam_gc_workspace_bytes(H, W), dtype=torch.uint8, device=img1.device)
    nbytes = workspace.numel() * workspace.element_size()
    side = torch.empty((H, W), dtype=torch.uint8, device=img1.device)
    info = torch.empty(4, dtype=torch.int32, device=img1.device)
    check(lib.st_seam_gc_begin(_pc(img1), _pc(img2), _pc(k1), _pc(k2), H, W, _p(workspace), nbytes, _stream()), "st_seam_gc_begin")
    record = workspace.view(torch.uint8).reshape(-1)[:32].view(torch.int32)
    status = record.tolist()                                 # a device -> host read per round: the status record
    reads = 1
    while not status[3] and status[2] < max_rounds:
        if status[1]:                                        # the global relabel has not reached its fixpoint: only that goes on
            check(lib.st_seam_gc_relabel(H, W, _p(workspace), nbytes, _stream()), "st_seam_gc_relabel")
        else:
            check(lib.st_seam_gc_round(H, W, _p(workspace), nbytes, _stream()), "st_seam_gc_round")
        status = record.tolist()
        reads += 1
    check(lib.st_seam_gc_finish(H, W, _p(side), _p(info), _p(workspace), nbytes, _stream()), "st_seam_gc_finish")
    if not status[3]:
        warnings.warn(f"seam_gc: no minimum cut after {status[2]} rounds (max_rounds = {max_rounds}); the blend keeps the distance seam")
    if return_stats:
        return side, info, dict(converged=bool(status[3]), rounds=status[2], sweeps=status[6], label_launches=status[7], host_reads=reads)
    return side, info


# ---- inner_crop: the largest hole-free rectangle of the stitch (csrc/crop.hip; README.md, inner_crop) --------------------------------
def inner_rect_workspace_bytes(H, W):
    """bytes of workspace `inner_rect` needs for an H x W canvas; 0 for a shape outside the contract"""
    return int(lib.st_inner_rect_workspace_bytes(int(H), int(W)))


def inner_rect(mask1, mask2=None, workspace=None, return_runs=False):
    """The largest axis-aligned rectangle inside the union of the masks (README.md, inner_crop): mask1, mask2 (optional) fp32 [1,1,H,W] or
    [1,3,H,W] (channel 0 > 0.5), the mask operands of `multiband_blend` -> info int32 [6] on the device: valid, top, left, height, width,
    area (all zeros when the union is empty); among the rectangles of the largest area the lowest top, then the lowest left, then the
    smallest height.  ``return_runs``: also int16 [H,W], the set pixels of the union in a column ending at each row, the plane the rectangle
    is searched in.  ``workspace``: a uint8 device tensor of at least `inner_rect_workspace_bytes` bytes, 16-byte aligned (default: allocated
    here).  All launches go to the current stream and nothing is read back."""
    masks = [m for m in (mask1, mask2) if m is not None]
    if mask1 is None or mask1.dim() != 4:
        raise ValueError(f"mask1 [1,1,H,W] or [1,3,H,W] expected, got {None if mask1 is None else tuple(mask1.shape)}")
    H, W = mask1.shape[2:]
    for m in masks:
        if m.dim() != 4 or m.shape[0] != 1 or m.shape[1] not in (1, 3) or tuple(m.shape[2:]) != (H, W):
            raise ValueError(f"mask [1,1,{H},{W}] or [1,3,{H},{W}] expected, got {tuple(m.shape)}")
        if m.dtype != torch.float32:
            raise ValueError(f"float32 tensors expected, got {m.dtype}")
    if not (1 <= H <= MULTIBAND_MAX_SIDE and 1 <= W <= MULTIBAND_MAX_SIDE):
        raise ValueError(f"sides must be in 1..{MULTIBAND_MAX_SIDE}, got {H} x {W}")
    k1 = mask1[:, :1].contiguous()                                   # channel 0 (no copy unless the mask is a strided view)
    k2 = mask2[:, :1].contiguous() if mask2 is not None else None
    if workspace is None:
        workspace = torch.empty(inner_rect_workspace_bytes(H, W), dtype=torch.uint8, device=mask1.device)
    info = torch.empty(6, dtype=torch.int32, device=mask1.device)
    runs = torch.empty((H, W), dtype=torch.int16, device=mask1.device) if return_runs else None
    check(lib.st_inner_rect(_pc(k1), _pc(k2), H, W, _p(info), _p(runs), _p(workspace), workspace.numel() * workspace.element_size(), _stream()),
          "st_inner_rect")
    return (info, runs) if return_runs else info


# ---- patchmatch_inpainter: exemplar hole filling (csrc/patchmatch.hip; README.md, patchmatch_inpainter) -------------------------------
PATCHMATCH_MIN_SIDE, PATCHMATCH_MAX_SIDE, PATCHMATCH_MAX_LEVELS, PATCHMATCH_MAX_ITERS = 15, 4096, 8, 64


def _patchmatch_levels(levels):
    if levels is None:
        return 0
    if not 1 <= int(levels) <= PATCHMATCH_MAX_LEVELS:
        raise ValueError(f"levels must be None (auto) or in 1..{PATCHMATCH_MAX_LEVELS}, got {levels}")
    return int(levels)


def patchmatch_workspace_bytes(H, W, levels=None):
    """bytes of workspace `inpaint_patchmatch` needs for an H x W image; 0 for a shape outside the contract"""
    return int(lib.st_patchmatch_workspace_bytes(int(H), int(W), _patchmatch_levels(levels)))


def patchmatch_levels(H, W, levels=None):
    """the number of pyramid levels `inpaint_patchmatch` runs on; 0 for a shape outside the contract"""
    return int(lib.st_patchmatch_levels(int(H), int(W), _patchmatch_levels(levels)))


def inpaint_patchmatch(img, mask, levels=None, iters=4, seed=1, workspace=None, return_fields=False):
    """Exemplar hole filling (README.md, patchmatch_inpainter; this project's own contract, pinned against no library): img uint8 [H,W,3],
    mask uint8 / bool [H,W] (nonzero = fill), the operands `inpaint_prep` produces -> (out uint8 [H,W,3], info int32 [4] on the device:
    valid, start level, level-0 sources, level-0 targets).  Known pixels come back byte for byte; with an empty mask or without a source
    patch at level 0 the image comes back as it is and info[0] = 0.  ``levels`` None = auto, else at most that many; ``iters`` search sweeps
    per level; ``seed`` keys every random draw.  ``return_fields``: also the level-0 match of every target centre after the last sweep
    (int32 [H,W,2], -1 elsewhere) and its cost (int32 [H,W], -1 elsewhere and without a sweep).  ``workspace``: a uint8 device tensor of at
    least `patchmatch_workspace_bytes` bytes, 16-byte aligned (default: allocated here).  All launches go to the current stream and nothing
    is read back."""
    if img.dim() != 3 or img.shape[2] != 3 or img.dtype != torch.uint8:
        raise ValueError(f"uint8 [H,W,3] image expected, got {img.dtype} {tuple(img.shape)}")
    H, W, _ = img.shape
    if mask.dtype == torch.bool:
        mask = mask.to(torch.uint8)
    if mask.dtype != torch.uint8 or tuple(mask.shape) != (H, W):
        raise ValueError(f"uint8 [{H},{W}] mask expected, got {mask.dtype} {tuple(mask.shape)}")
    if mask.device != img.device:
        raise ValueError("image and mask must be on the same device")
    if not (PATCHMATCH_MIN_SIDE <= H <= PATCHMATCH_MAX_SIDE and PATCHMATCH_MIN_SIDE <= W <= PATCHMATCH_MAX_SIDE):
        raise ValueError(f"sides must be in {PATCHMATCH_MIN_SIDE}..{PATCHMATCH_MAX_SIDE}, got {H} x {W}")
    lv = _patchmatch_levels(levels)
    if not 0 <= int(iters) <= PATCHMATCH_MAX_ITERS:
        raise ValueError(f"iters must be in 0..{PATCHMATCH_MAX_ITERS}, got {iters}")
    seed = int(seed) & 0xFFFFFFFF
    dev = img.device
    if workspace is None:
        workspace = torch.empty(patchmatch_workspace_bytes(H, W, levels), dtype=torch.uint8, device=dev)
    out = torch.empty_like(img, memory_format=torch.contiguous_format)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    nnf = torch.empty((H, W, 2), dtype=torch.int32, device=dev) if return_fields else None
    sad = torch.empty((H, W), dtype=torch.int32, device=dev) if return_fields else None
    check(lib.st_patchmatch_fill(_pc(img), _pc(mask), H, W, lv, int(iters), seed - (1 << 32) if seed >= 1 << 31 else seed, _p(out), _p(info), _p(nnf), _p(sad),
                                 _p(workspace), workspace.numel() * workspace.element_size(), _stream()), "st_patchmatch_fill")
    return (out, info, nnf, sad) if return_fields else (out, info)


# ---- feature_align: corners, binary descriptors, matching, RANSAC homography (csrc/features.hip; README.md, feature_align) -------------------
FEATURE_MIN_SIDE, FEATURE_MAX_SIDE, FEATURE_MAX_BATCH, FEATURE_MAX_HYP = 64, 1024, 64, 65536
_FEATURE_REGIONS = ("box", "kp", "desc", "nn", "matches", "count", "mc", "scores", "mask", "total")


def _feature_image(img, name="img"):
    if img.dim() != 4 or img.shape[1] != 3 or img.dtype != torch.float32:
        raise ValueError(f"{name}: float32 [B,3,H,W] expected, got {img.dtype} {tuple(img.shape)}")
    B, _, H, W = img.shape
    _feature_shape(B, H, W)
    return B, H, W


def _feature_shape(B, H, W):
    if not 1 <= B <= FEATURE_MAX_BATCH:
        raise ValueError(f"batch must be in 1..{FEATURE_MAX_BATCH}, got {B}")
    if not (FEATURE_MIN_SIDE <= H <= FEATURE_MAX_SIDE and FEATURE_MIN_SIDE <= W <= FEATURE_MAX_SIDE):
        raise ValueError(f"sides must be in {FEATURE_MIN_SIDE}..{FEATURE_MAX_SIDE}, got {H} x {W}")


def _feature_operand(t, name, dtype, shape):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: {dtype} {tuple(shape)} expected, got {t.dtype} {tuple(t.shape)}")
    return t


def _feature_lists(B, N, **operands):
    """the per-slot operands of the match and ransac stages of both paths, by name: kp* int32 [B,N,2], desc* int32 [B,N,8], matches int32 [B,N,2], count int32 [B]"""
    for name, t in operands.items():
        _feature_operand(t, name, torch.int32, (B,) if name == "count" else (B, N, 8) if name.startswith("desc") else (B, N, 2))


def _feature_model(B, dev):
    """the uninitialised (motion fp32 [B,4,2], H fp32 [B,3,3], info int32 [B,8]) that the ransac and homography entries of both paths fill"""
    return (torch.empty((B, 4, 2), dtype=torch.float32, device=dev), torch.empty((B, 3, 3), dtype=torch.float32, device=dev),
            torch.empty((B, 8), dtype=torch.int32, device=dev))


def _feature_fields(workspace, L, B, N, more=()):
    """copies of the regions of a workspace with the byte offsets L: the fields that both paths return, and under its own name every (name, bytes,
    dtype, shape) of `more`"""
    raw = workspace.view(torch.uint8).reshape(-1)

    def region(name, nbytes, dtype, shape):
        return raw[L[name]:L[name] + nbytes].view(dtype).reshape(shape).clone()
    kp = region("kp", 16 * B * N, torch.int32, (2, B, N, 2))
    desc = region("desc", 64 * B * N, torch.int32, (2, B, N, 8))
    return dict(kp1=kp[0], kp2=kp[1], desc1=desc[0], desc2=desc[1], nn=region("nn", 24 * B * N, torch.int32, (2, B, N, 3)),
                matches=region("matches", 8 * B * N, torch.int32, (B, N, 2)), count=region("count", 4 * B, torch.int32, (B,)),
                mask=region("mask", B * N, torch.uint8, (B, N)), **{r[0]: region(*r) for r in more})


def _feature_seed(seed):
    seed = int(seed) & 0xFFFFFFFF
    return seed - (1 << 32) if seed >= 1 << 31 else seed


def _feature_params(max_hyp, thr, min_inliers):
    if not 1 <= int(max_hyp) <= FEATURE_MAX_HYP:
        raise ValueError(f"max_hyp must be in 1..{FEATURE_MAX_HYP}, got {max_hyp}")
    if not 0.0 < float(thr) < float("inf"):
        raise ValueError(f"thr must be finite and positive, got {thr}")
    if int(min_inliers) < 0:
        raise ValueError(f"min_inliers must be >= 0, got {min_inliers}")
    return int(max_hyp), float(thr), int(min_inliers)


def feature_slots(H, W):
    """N = 4 ceil(H/32) ceil(W/32), the keypoint slots of an H x W image; 0 for a side outside 64..1024"""
    return int(lib.st_feature_slots(int(H), int(W)))


def feature_brief_pattern():
    """the BRIEF-256 pattern, an int8 [256,4] CPU tensor: bit k of a descriptor is S(p + (ax, ay)) < S(p + (bx, by)) for row k = (ax, ay, bx, by)"""
    buf = (C.c_int8 * 1024)()
    check(lib.st_feature_brief_pattern(C.cast(buf, C.c_void_p)), "st_feature_brief_pattern")
    return torch.tensor(list(buf), dtype=torch.int8).reshape(256, 4)


def feature_workspace_bytes(B, H, W, max_hyp=2048):
    """bytes of workspace `feature_homography` needs; 0 for a shape or max_hyp outside the contract"""
    return int(lib.st_feature_workspace_bytes(int(B), int(H), int(W), int(max_hyp)))


def feature_workspace_layout(B, H, W, max_hyp=2048):
    """{region: byte offset} of that workspace (include/stitch_gfx950.h, st_feature_workspace_layout) and its "total" """
    off = (C.c_int64 * 10)()
    check(lib.st_feature_workspace_layout(int(B), int(H), int(W), int(max_hyp), C.cast(off, C.c_void_p)), "st_feature_workspace_layout")
    return dict(zip(_FEATURE_REGIONS, (int(v) for v in off)))


def feature_detect(img):
    """Stage 1 (README.md, feature_align): img fp32 [B,3,H,W] -> (kp int32 [B,N,2] = (x, y) per slot, (-1, -1) unused; box int16 [B,H,W] (values 0..6375), the
    5x5 box sum of the luma that `feature_describe` reads)."""
    B, H, W = _feature_image(img)
    N = feature_slots(H, W)
    kp = torch.empty((B, N, 2), dtype=torch.int32, device=img.device)
    box = torch.empty((B, H, W), dtype=torch.int16, device=img.device)
    check(lib.st_feature_detect(_pc(img), B, H, W, _p(kp), _p(box), _stream()), "st_feature_detect")
    return kp, box


def feature_describe(box, kp):
    """Stage 2: box int16 [B,H,W], kp int32 [B,N,2] -> desc uint32 [B,N,8] (as int32 bit patterns: torch has no uint32 arithmetic), zero
    for an unused slot."""
    B, H, W = box.shape
    _feature_shape(B, H, W)
    N = feature_slots(H, W)
    _feature_operand(box, "box", torch.int16, (B, H, W))
    _feature_operand(kp, "kp", torch.int32, (B, N, 2))
    desc = torch.empty((B, N, 8), dtype=torch.int32, device=box.device)
    check(lib.st_feature_describe(_pc(box), _pc(kp), B, H, W, _p(desc), _stream()), "st_feature_describe")
    return desc


def feature_match(kp1, desc1, kp2, desc2, H, W):
    """Stage 3: -> (nn int32 [2,B,N,3] = per direction and slot (best slot or -1, d1, d2); matches int32 [B,N,2] = (slot 1, slot 2) in slot
    order of image 1, (-1, -1) behind the last; count int32 [B])."""
    B = kp1.shape[0]
    _feature_shape(B, H, W)
    N = feature_slots(H, W)
    _feature_lists(B, N, kp1=kp1, desc1=desc1, kp2=kp2, desc2=desc2)
    dev = kp1.device
    nn = torch.empty((2, B, N, 3), dtype=torch.int32, device=dev)
    matches = torch.empty((B, N, 2), dtype=torch.int32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    check(lib.st_feature_match(_pc(kp1), _pc(desc1), _pc(kp2), _pc(desc2), B, H, W, _p(nn), _p(matches), _p(count), _stream()), "st_feature_match")
    return nn, matches, count


def feature_ransac(kp1, kp2, matches, count, H, W, *, max_hyp=2048, thr=3.0, min_inliers=12, seed=1):
    """Stage 4: -> (motion fp32 [B,4,2], H fp32 [B,3,3], info int32 [B,8], mask uint8 [B,N]: the inlier flag of every list entry)."""
    B = kp1.shape[0]
    _feature_shape(B, H, W)
    max_hyp, thr, min_inliers = _feature_params(max_hyp, thr, min_inliers)
    N = feature_slots(H, W)
    _feature_lists(B, N, kp1=kp1, kp2=kp2, matches=matches, count=count)
    dev = kp1.device
    motion, Hm, info = _feature_model(B, dev)
    mask = torch.empty((B, N), dtype=torch.uint8, device=dev)
    ws = torch.empty(32 * B * N + 4 * B * max_hyp, dtype=torch.uint8, device=dev)
    check(lib.st_feature_ransac(_pc(kp1), _pc(kp2), _pc(matches), _pc(count), B, H, W, max_hyp, thr, min_inliers, _feature_seed(seed), _p(motion), _p(Hm), _p(info),
                                _p(mask), _p(ws), ws.numel(), _stream()), "st_feature_ransac")
    return motion, Hm, info, mask


def feature_homography(img1, img2, *, max_hyp=2048, thr=3.0, min_inliers=12, seed=1, workspace=None, return_fields=False):
    """A homography from pixels, without weights (README.md, feature_align; this project's own contract, pinned against no library): img1,
    img2 fp32 [B,3,H,W] in 0..255 -> (motion fp32 [B,4,2], H fp32 [B,3,3], info int32 [B,8]), all on the device.  H maps image-1 pixels onto
    image-2 pixels (h33 = 1) -- the matrix `dlt4` gives for the corners (0,0), (W,0), (0,H), (W,H) moved by `motion`, the direction of the
    homography network's offsets.  info = (valid, keypoints 1, keypoints 2, matches, winning hypothesis or -1, inliers, 0, 0); without a
    valid model motion is zero and H the identity.  ``max_hyp`` RANSAC hypotheses, ``thr`` the inlier distance in pixels, ``min_inliers``
    what a valid model needs, ``seed`` keys every draw.  ``workspace``: a uint8 device tensor of at least `feature_workspace_bytes` bytes,
    16-byte aligned (default: allocated here).  ``return_fields``: also a dict of copies of the workspace's regions after the call: kp1, kp2
    int32 [B,N,2]; desc1, desc2 int32 [B,N,8]; nn int32 [2,B,N,3]; matches int32 [B,N,2]; count int32 [B]; mask uint8 [B,N].  All
    launches go to the current stream and nothing is read back."""
    B, H, W = _feature_image(img1, "img1")
    if img2.shape != img1.shape or img2.dtype != torch.float32 or img2.device != img1.device:
        raise ValueError(f"img2: float32 {tuple(img1.shape)} on {img1.device} expected, got {img2.dtype} {tuple(img2.shape)} on {img2.device}")
    max_hyp, thr, min_inliers = _feature_params(max_hyp, thr, min_inliers)
    dev = img1.device
    if workspace is None:
        workspace = torch.empty(feature_workspace_bytes(B, H, W, max_hyp), dtype=torch.uint8, device=dev)
    motion, Hm, info = _feature_model(B, dev)
    check(lib.st_feature_homography(_pc(img1), _pc(img2), B, H, W, max_hyp, thr, min_inliers, _feature_seed(seed), _p(motion), _p(Hm), _p(info), _p(workspace),
                                    workspace.numel() * workspace.element_size(), _stream()), "st_feature_homography")
    if not return_fields:
        return motion, Hm, info
    return motion, Hm, info, _feature_fields(workspace, feature_workspace_layout(B, H, W, max_hyp), B, feature_slots(H, W))


# ---- feature_align_ms: oriented, multi-scale keypoints in front of the same matching and RANSAC (csrc/features_ms.hip; README.md, feature_align_ms) ----
FEATURE_MS_MAX_LEVELS = 8
_FEATURE_MS_REGIONS = ("pyr", "box", "kp", "bins", "desc", "nn", "matches", "count", "xy", "mc", "scores", "mask", "total")


def _feature_ms_levels(levels):
    if int(levels) != levels or not 1 <= int(levels) <= FEATURE_MS_MAX_LEVELS:
        raise ValueError(f"levels must be an integer in 1..{FEATURE_MS_MAX_LEVELS}, got {levels}")
    return int(levels)


def feature_ms_level_sizes(H, W, levels=6):
    """[(H_l, W_l)] of the pyramid: level l+1 exists iff l+1 < levels and min(4 H_l div 5, 4 W_l div 5) >= 64; [] for a rejected argument"""
    buf = (C.c_int32 * 16)()
    n = int(lib.st_feature_ms_level_sizes(int(H), int(W), int(levels), C.cast(buf, C.c_void_p)))
    return [(int(buf[2 * l]), int(buf[2 * l + 1])) for l in range(n)]


def feature_ms_slots(H, W, levels=6):
    """N = the keypoint slots of all levels, level 0 first; 0 for a rejected argument"""
    return int(lib.st_feature_ms_slots(int(H), int(W), int(levels)))


def feature_ms_workspace_bytes(B, H, W, levels=6, max_hyp=2048):
    """bytes of workspace `feature_homography_ms` needs; 0 for an argument outside the contract"""
    return int(lib.st_feature_ms_workspace_bytes(int(B), int(H), int(W), int(levels), int(max_hyp)))


def feature_ms_workspace_layout(B, H, W, levels=6, max_hyp=2048):
    """{region: byte offset} of that workspace (include/stitch_gfx950.h, st_feature_ms_workspace_layout) and its "total" """
    off = (C.c_int64 * 13)()
    check(lib.st_feature_ms_workspace_layout(int(B), int(H), int(W), int(levels), int(max_hyp), C.cast(off, C.c_void_p)), "st_feature_ms_workspace_layout")
    return dict(zip(_FEATURE_MS_REGIONS, (int(v) for v in off)))


def _feature_ms_split(flat, n, sizes):
    """a flat level-major buffer of n planes per level -> [view [n,H_l,W_l]]"""
    out, at = [], 0
    for h, w in sizes:
        out.append(flat[at:at + n * h * w].view(n, h, w))
        at += n * h * w
    return out


def _feature_ms_join(planes, name, dtype, n, sizes):
    if len(planes) != len(sizes):
        raise ValueError(f"{name}: {len(sizes)} levels expected, got {len(planes)}")
    for p, (h, w) in zip(planes, sizes):
        _feature_operand(p, name, dtype, (n, h, w))
    return torch.cat([p.reshape(-1) for p in planes])


def feature_ms_pyramid(img, levels=6):
    """Stage 1 (README.md, feature_align_ms): img fp32 [B,3,H,W] -> [uint8 [B,H_l,W_l]]: the luma, then each level the centre-aligned x 5/4 resample of the one before"""
    B, H, W = _feature_image(img)
    sizes = feature_ms_level_sizes(H, W, _feature_ms_levels(levels))
    flat = torch.empty(B * sum(h * w for h, w in sizes), dtype=torch.uint8, device=img.device)
    check(lib.st_feature_ms_pyramid(_pc(img), B, H, W, int(levels), _p(flat), _stream()), "st_feature_ms_pyramid")
    return _feature_ms_split(flat, B, sizes)


def feature_ms_detect(pyr, levels=6, oriented=True):
    """Stage 2: the pyramid of `feature_ms_pyramid` -> (kp int32 [B,N,2] in each slot's level pixels, (-1, -1) unused; bins uint8 [B,N], the orientation
    bin 0..31 of every slot; box: [int16 [B,H_l,W_l]], the 5x5 box sums `feature_ms_describe` reads)"""
    B, H, W = pyr[0].shape
    _feature_shape(B, H, W)
    sizes = feature_ms_level_sizes(H, W, _feature_ms_levels(levels))
    flat = _feature_ms_join(pyr, "pyr", torch.uint8, B, sizes)
    N, dev = feature_ms_slots(H, W, levels), flat.device
    kp = torch.empty((B, N, 2), dtype=torch.int32, device=dev)
    bins = torch.empty((B, N), dtype=torch.uint8, device=dev)
    box = torch.empty(flat.numel(), dtype=torch.int16, device=dev)
    check(lib.st_feature_ms_detect(_pc(flat), B, H, W, int(levels), int(bool(oriented)), _p(kp), _p(bins), _p(box), _stream()), "st_feature_ms_detect")
    return kp, bins, _feature_ms_split(box, B, sizes)


def feature_ms_describe(box, kp, bins, levels=6):
    """Stage 3: -> desc uint32 [B,N,8] (as int32 bit patterns): the BRIEF pattern steered by each slot's bin, on its level's box sums"""
    B, H, W = box[0].shape
    _feature_shape(B, H, W)
    sizes = feature_ms_level_sizes(H, W, _feature_ms_levels(levels))
    flat = _feature_ms_join(box, "box", torch.int16, B, sizes)
    N = feature_ms_slots(H, W, levels)
    _feature_operand(kp, "kp", torch.int32, (B, N, 2))
    _feature_operand(bins, "bins", torch.uint8, (B, N))
    desc = torch.empty((B, N, 8), dtype=torch.int32, device=flat.device)
    check(lib.st_feature_ms_describe(_pc(flat), _pc(kp), _pc(bins), B, H, W, int(levels), _p(desc), _stream()), "st_feature_ms_describe")
    return desc


def feature_ms_match(kp1, desc1, kp2, desc2, H, W, levels=6):
    """Stage 4: `feature_match` over the slots of all levels -> (nn int32 [2,B,N,3], matches int32 [B,N,2], count int32 [B])"""
    B = kp1.shape[0]
    _feature_shape(B, H, W)
    N = feature_ms_slots(H, W, _feature_ms_levels(levels))
    _feature_lists(B, N, kp1=kp1, desc1=desc1, kp2=kp2, desc2=desc2)
    dev = kp1.device
    nn = torch.empty((2, B, N, 3), dtype=torch.int32, device=dev)
    matches = torch.empty((B, N, 2), dtype=torch.int32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    check(lib.st_feature_ms_match(_pc(kp1), _pc(desc1), _pc(kp2), _pc(desc2), B, H, W, int(levels), _p(nn), _p(matches), _p(count), _stream()), "st_feature_ms_match")
    return nn, matches, count


def feature_ms_ransac(kp1, kp2, matches, count, H, W, levels=6, *, max_hyp=2048, thr=3.0, min_inliers=12, seed=1):
    """Stage 5: `feature_ransac` on level-0 coordinates -> (motion fp32 [B,4,2], H fp32 [B,3,3], info int32 [B,8], mask uint8 [B,N], xy fp64 [2,B,N,2]:
    the level-0 position of every slot of both images, (-1, -1) unused)."""
    B = kp1.shape[0]
    _feature_shape(B, H, W)
    max_hyp, thr, min_inliers = _feature_params(max_hyp, thr, min_inliers)
    N = feature_ms_slots(H, W, _feature_ms_levels(levels))
    _feature_lists(B, N, kp1=kp1, kp2=kp2, matches=matches, count=count)
    dev = kp1.device
    motion, Hm, info = _feature_model(B, dev)
    mask = torch.empty((B, N), dtype=torch.uint8, device=dev)
    xy = torch.empty((2, B, N, 2), dtype=torch.float64, device=dev)
    ws = torch.empty(32 * B * N + 4 * B * max_hyp, dtype=torch.uint8, device=dev)
    check(lib.st_feature_ms_ransac(_pc(kp1), _pc(kp2), _pc(matches), _pc(count), B, H, W, int(levels), max_hyp, thr, min_inliers, _feature_seed(seed), _p(motion), _p(Hm),
                                   _p(info), _p(mask), _p(xy), _p(ws), ws.numel(), _stream()), "st_feature_ms_ransac")
    return motion, Hm, info, mask, xy


def feature_homography_ms(img1, img2, *, levels=6, oriented=True, max_hyp=2048, thr=3.0, min_inliers=12, seed=1, workspace=None, return_fields=False):
    """`feature_homography` for rotated and zoomed pairs (README.md, feature_align_ms; this project's own contract, pinned against no library):
    corners on ``levels`` levels of a 5/4 pyramid (capped by the size), a 32-bin orientation per corner (``oriented``) that steers the
    descriptor, then the same matching over all slots and the same RANSAC on level-0 coordinates.  Operands, results, ``max_hyp``, ``thr``,
    ``min_inliers``, ``seed`` and ``info`` as `feature_homography`; ``workspace`` at least `feature_ms_workspace_bytes` bytes, 16-byte
    aligned.  ``return_fields``: also a dict of copies of the workspace's regions after the call: what `feature_homography` returns (kp in
    each slot's level pixels) and pyr1, pyr2 [uint8 [B,H_l,W_l]], bins1, bins2 uint8 [B,N], xy fp64 [2,B,N,2] (level-0 coordinates).  All
    launches go to the current stream and nothing is read back."""
    B, H, W = _feature_image(img1, "img1")
    if img2.shape != img1.shape or img2.dtype != torch.float32 or img2.device != img1.device:
        raise ValueError(f"img2: float32 {tuple(img1.shape)} on {img1.device} expected, got {img2.dtype} {tuple(img2.shape)} on {img2.device}")
    levels = _feature_ms_levels(levels)
    max_hyp, thr, min_inliers = _feature_params(max_hyp, thr, min_inliers)
    dev = img1.device
    if workspace is None:
        workspace = torch.empty(feature_ms_workspace_bytes(B, H, W, levels, max_hyp), dtype=torch.uint8, device=dev)
    motion, Hm, info = _feature_model(B, dev)
    check(lib.st_feature_ms_homography(_pc(img1), _pc(img2), B, H, W, levels, int(bool(oriented)), max_hyp, thr, min_inliers, _feature_seed(seed), _p(motion), _p(Hm),
                                       _p(info), _p(workspace), workspace.numel() * workspace.element_size(), _stream()), "st_feature_ms_homography")
    if not return_fields:
        return motion, Hm, info
    N, sizes = feature_ms_slots(H, W, levels), feature_ms_level_sizes(H, W, levels)
    fields = _feature_fields(workspace, feature_ms_workspace_layout(B, H, W, levels, max_hyp), B, N,
                             (("bins", 2 * B * N, torch.uint8, (2, B, N)), ("pyr", 2 * B * sum(h * w for h, w in sizes), torch.uint8, (-1,)),
                              ("xy", 32 * B * N, torch.float64, (2, B, N, 2))))
    bins, pyr = fields.pop("bins"), _feature_ms_split(fields.pop("pyr"), 2 * B, sizes)
    fields.update(bins1=bins[0], bins2=bins[1], pyr1=[p[:B] for p in pyr], pyr2=[p[B:] for p in pyr])
    return motion, Hm, info, fields


# ---- dense_flow: coarse-to-fine, zero-mean Lucas-Kanade residual flow on integer pyramids (csrc/dense_flow.hip; README.md, dense_flow) ------
DENSE_FLOW_MIN_SIDE, DENSE_FLOW_MAX_SIDE, DENSE_FLOW_MAX_BATCH, DENSE_FLOW_MAX_LEVELS = 16, 1024, 64, 8
DENSE_FLOW_MAX_ITERS, DENSE_FLOW_MAX_RADIUS, DENSE_FLOW_MAX_DAMPING = 16, 7, 1 << 24
DENSE_FLOW_DEFAULTS = dict(levels=5, iters=4, radius=4, damping=65536)


def _dense_flow_shape(B, H, W):
    if not 1 <= B <= DENSE_FLOW_MAX_BATCH:
        raise ValueError(f"batch must be in 1..{DENSE_FLOW_MAX_BATCH}, got {B}")
    if not (DENSE_FLOW_MIN_SIDE <= H <= DENSE_FLOW_MAX_SIDE and DENSE_FLOW_MIN_SIDE <= W <= DENSE_FLOW_MAX_SIDE):
        raise ValueError(f"sides must be in {DENSE_FLOW_MIN_SIDE}..{DENSE_FLOW_MAX_SIDE}, got {H} x {W}")


def _dense_flow_params(levels, iters, radius, damping):
    for name, v, lo, hi in (("levels", levels, 1, DENSE_FLOW_MAX_LEVELS), ("iters", iters, 1, DENSE_FLOW_MAX_ITERS), ("radius", radius, 1, DENSE_FLOW_MAX_RADIUS),
                            ("damping", damping, 0, DENSE_FLOW_MAX_DAMPING)):
        if int(v) != v or not lo <= int(v) <= hi:
            raise ValueError(f"{name} must be an integer in {lo}..{hi}, got {v}")
    return int(levels), int(iters), int(radius), int(damping)


def _dense_flow_images(img1, img2):
    if img1.dim() != 4 or img1.shape[1] != 3 or img1.dtype != torch.float32:
        raise ValueError(f"img1: float32 [B,3,H,W] expected, got {img1.dtype} {tuple(img1.shape)}")
    if img2.shape != img1.shape or img2.dtype != torch.float32 or img2.device != img1.device:
        raise ValueError(f"img2: float32 {tuple(img1.shape)} on {img1.device} expected, got {img2.dtype} {tuple(img2.shape)} on {img2.device}")
    B, _, H, W = img1.shape
    _dense_flow_shape(B, H, W)
    return B, H, W


def _dense_flow_mask(mask, name, ref):
    """-> (dense tensor or None, channels per item)"""
    if mask is None:
        return None, 1
    B, _, H, W = ref.shape
    if mask.dim() != 4 or mask.dtype != torch.float32 or mask.device != ref.device or mask.shape[0] != B or mask.shape[1] not in (1, 3) or tuple(mask.shape[2:]) != (H, W):
        raise ValueError(f"{name}: float32 [{B},1 or 3,{H},{W}] on {ref.device} expected, got {mask.dtype} {tuple(mask.shape)} on {mask.device}")
    return mask.contiguous(), int(mask.shape[1])


def dense_flow_level_sizes(H, W, levels=5):
    """[(H_l, W_l)] of the pyramid: level l+1 exists iff l+1 < levels and min(H_l, W_l) >= 32, and is ceil(H_l/2) x ceil(W_l/2)"""
    sizes = [(int(H), int(W))]
    while len(sizes) < levels and min(sizes[-1]) >= 32:
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    return sizes


def dense_flow_workspace_bytes(B, H, W, levels=5):
    """bytes of workspace `dense_flow` needs; 0 for a shape or `levels` outside the contract"""
    n = C.c_int64(0)
    return int(n.value) if lib.st_dense_flow_workspace_bytes(int(B), int(H), int(W), int(levels), C.cast(C.byref(n), C.c_void_p)) == 0 else 0


def dense_flow_workspace_layout(B, H, W, levels=5):
    """the regions of that workspace (include/stitch_gfx950.h, st_dense_flow_workspace_layout): dict(levels=L, v=[...], m=[...], u=[...] byte
    offsets per level, tmp, sup, total)"""
    off = (C.c_int64 * 28)()
    check(lib.st_dense_flow_workspace_layout(int(B), int(H), int(W), int(levels), C.cast(off, C.c_void_p)), "st_dense_flow_workspace_layout")
    o = [int(v) for v in off]
    L = o[0]
    return dict(levels=L, v=o[1:1 + L], m=o[9:9 + L], u=o[17:17 + L], tmp=o[25], sup=o[26], total=o[27])


def _dense_flow_workspace(workspace, B, H, W, levels, dev):
    need = dense_flow_workspace_bytes(B, H, W, levels)
    if workspace is None:
        return torch.empty(need, dtype=torch.uint8, device=dev)
    if workspace.device != dev:
        raise ValueError(f"workspace on {dev} expected, got {workspace.device}")
    return workspace


def _dense_flow_pyramid_views(workspace, B, H, W, levels):
    """copies of the pyramid regions of a workspace: (v1, v2 lists of int16 [B,Hl,Wl], m1, m2 lists of uint8 [B,Hl,Wl], layout, sizes)"""
    P, raw = dense_flow_workspace_layout(B, H, W, levels), workspace.view(torch.uint8).reshape(-1)
    sizes = dense_flow_level_sizes(H, W, levels)
    v1, v2, m1, m2 = [], [], [], []
    for l, (h, w) in enumerate(sizes):
        v = raw[P["v"][l]:P["v"][l] + 4 * B * h * w].view(torch.int16).reshape(2, B, h, w).clone()
        m = raw[P["m"][l]:P["m"][l] + 2 * B * h * w].reshape(2, B, h, w).clone()
        v1.append(v[0]), v2.append(v[1]), m1.append(m[0]), m2.append(m[1])
    return v1, v2, m1, m2, P, sizes


def dense_flow_pyramid(img1, img2, mask1=None, mask2=None, *, levels=5, workspace=None):
    """Stage 1 (README.md, dense_flow): both pyramids.  -> dict(v1, v2: lists per level of int16 [B,Hl,Wl], V = 16 luma at level 0;
    m1, m2: lists of uint8 [B,Hl,Wl])."""
    B, H, W = _dense_flow_images(img1, img2)
    levels = _dense_flow_params(levels, 1, 1, 0)[0]
    img1, img2 = img1.contiguous(), img2.contiguous()
    mask1, c1 = _dense_flow_mask(mask1, "mask1", img1)
    mask2, c2 = _dense_flow_mask(mask2, "mask2", img1)
    workspace = _dense_flow_workspace(workspace, B, H, W, levels, img1.device)
    check(lib.st_dense_flow_pyramid(_pc(img1), _pc(img2), _pc(mask1), c1, _pc(mask2), c2, B, H, W, levels, _p(workspace), workspace.numel() * workspace.element_size(),
                                    _stream()), "st_dense_flow_pyramid")
    v1, v2, m1, m2, _, _ = _dense_flow_pyramid_views(workspace, B, H, W, levels)
    return dict(v1=v1, v2=v2, m1=m1, m2=m2)


def dense_flow_iterate(v1, v2, m1, m2, u, *, radius=4, damping=65536):
    """Stage 2: one iteration at one level.  v1, v2 int16 [B,H,W], m1, m2 uint8 [B,H,W], u int32 [B,2,H,W] (1/256 px) ->
    (u_out int32 [B,2,H,W]: the clamped Lucas-Kanade update, then the 3x3 median; support uint8 [B,H,W])."""
    if v1.dim() != 3 or v1.dtype != torch.int16:
        raise ValueError(f"v1: int16 [B,H,W] expected, got {v1.dtype} {tuple(v1.shape)}")
    B, H, W = v1.shape
    _dense_flow_shape(B, H, W)
    _, _, radius, damping = _dense_flow_params(1, 1, radius, damping)
    for t, name, dtype, shape in ((v2, "v2", torch.int16, (B, H, W)), (m1, "m1", torch.uint8, (B, H, W)), (m2, "m2", torch.uint8, (B, H, W)),
                                  (u, "u", torch.int32, (B, 2, H, W))):
        if t.dtype != dtype or tuple(t.shape) != shape or t.device != v1.device:
            raise ValueError(f"{name}: {dtype} {shape} on {v1.device} expected, got {t.dtype} {tuple(t.shape)} on {t.device}")
    dev = v1.device
    u_out = torch.empty((B, 2, H, W), dtype=torch.int32, device=dev)
    support = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    ws = torch.empty(8 * B * H * W, dtype=torch.uint8, device=dev)
    check(lib.st_dense_flow_iterate(_pc(v1), _pc(v2), _pc(m1), _pc(m2), _pc(u), B, H, W, radius, damping, _p(u_out), _p(support), _p(ws), ws.numel(), _stream()),
          "st_dense_flow_iterate")
    return u_out, support


def dense_flow(img1, img2, mask1=None, mask2=None, *, levels=5, iters=4, radius=4, damping=65536, workspace=None, return_fields=False):
    """A dense residual flow from pixels, without weights (README.md, dense_flow; this project's own contract, pinned against no library):
    img1, img2 fp32 [B,3,H,W] in 0..255 -> (flow fp32 [B,2,H,W], support uint8 [B,1,H,W]).  flow[:,0] = dx, flow[:,1] = dy in pixels,
    1 -> 2: img1(p) ~ img2(p + flow(p)), the flow `flow_warp(img2, flow)` consumes to bring image 2 onto image 1.  support: whether the
    last iteration at full resolution had enough valid window pixels and a positive determinant (elsewhere the flow is what the coarser
    levels and the median left).  mask1, mask2: fp32 [B,1,H,W] or [B,3,H,W] (channel 0), valid iff > 0.5, None = all valid.  ``levels``
    1..8 (capped by the size), ``iters`` 1..16 per level, ``radius`` 1..7 of the window, ``damping`` 0..2^24 on the diagonal.
    ``workspace``: a uint8 device tensor of at least `dense_flow_workspace_bytes` bytes, 16-byte aligned (default: allocated here).
    ``return_fields``: also a dict of copies of the workspace's regions after the call: v1, v2, m1, m2 (the pyramids, lists per level) and
    u (list per level of int32 [B,2,Hl,Wl], the final flow of each level in 1/256 px).  All launches go to the current stream and nothing
    is read back."""
    B, H, W = _dense_flow_images(img1, img2)
    levels, iters, radius, damping = _dense_flow_params(levels, iters, radius, damping)
    img1, img2 = img1.contiguous(), img2.contiguous()
    mask1, c1 = _dense_flow_mask(mask1, "mask1", img1)
    mask2, c2 = _dense_flow_mask(mask2, "mask2", img1)
    dev = img1.device
    workspace = _dense_flow_workspace(workspace, B, H, W, levels, dev)
    flow = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev)
    support = torch.empty((B, 1, H, W), dtype=torch.uint8, device=dev)
    check(lib.st_dense_flow(_pc(img1), _pc(img2), _pc(mask1), c1, _pc(mask2), c2, B, H, W, levels, iters, radius, damping, _p(flow), _p(support), _p(workspace),
                            workspace.numel() * workspace.element_size(), _stream()), "st_dense_flow")
    if not return_fields:
        return flow, support
    v1, v2, m1, m2, P, sizes = _dense_flow_pyramid_views(workspace, B, H, W, levels)
    raw = workspace.view(torch.uint8).reshape(-1)
    u = [raw[P["u"][l]:P["u"][l] + 8 * B * h * w].view(torch.int32).reshape(B, 2, h, w).clone() for l, (h, w) in enumerate(sizes)]
    return flow, support, dict(v1=v1, v2=v2, m1=m1, m2=m2, u=u)
