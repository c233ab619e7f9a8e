"""fp64 references, first-order worst-case elementwise error bounds, case tables and input generators for the kernels of csrc/transref.hip
and the wrapper steps around them, shared by tests/test_transref_bounds_cpu.py and tests/test_transref_matrix_gpu.py.  Every reference
states the operation in torch fp64 (or, for the steps the project declares bit-exact, in torch-CPU fp32 one rounding per operation) and knows
nothing of a kernel's tiling; every bound E is a sum of the roundings the kernel performs, each taken at its worst, to first order in
u = 2^-24.  No constant here comes from a GPU measurement: each is a count read from the kernel text, given below.

tr_attention_kernel   the softmax-pooling bound of tests/_nn_bounds.py (tau_j, E_d there) with a new row of its table:

    kernel                                         pre  n_sub  n_exp        n_acc          n_sum            nch = ceil(Nk / 32)
    tr_attention_kernel (MFMA, online softmax)      1     4     2 + 2 nch   33 nch         2 nch + 5

    score   S^T = K Q^T by D / 8 groups of four v_mfma_f32_32x32x2f32, each adding two products: a chain of D terms (the D of (D + pre) S_j);
            then s[r] * scale, one rounding (pre = 1).
    n_sub   p = expf(s - mn): the subtraction of the running maximum and the argument handling of ocml's expf, both relative to |s_j - mn| <=
            |s_j - m| (2, as for softmax_rows_kernel).  Every later key tile rescales o and lp by alpha = expf(m - mn); the arguments of these
            alphas telescope to mn(tile of j) - m <= |s_j - m| (the argument of the `kvlds` VALU row), so the two roundings count twice: 4.
    n_exp   ocml expf, 1 ulp <= 2u, for p; each of the at most nch alphas that follow adds 2u to the weights before it.
    n_acc   per key tile one product o *= alpha and 16 MFMAs of two products each into o: 33 roundings along the chain.
    n_sum   lp[r] = lp[r] * alpha + p without contraction: two roundings per tile; the pairwise fold over 16 registers is four sums deep and
            the lane pair adds one: 5.  The single IEEE division per output is inside the `+ 2` of the form.
    Keys past Nk score -inf, their weight is an exact 0 and their (clamped) V row is multiplied by it: they appear nowhere.

tr_deform_im2col_kernel   cols = w1 v1 + w2 v2 + w3 v3 + w4 v4, the corners outside the image reading 0, 0 outside (-1, H) x (-1, W)
    The sample coordinate is taken as the fp32 sum  h = fl(fl(oy - 1 + ky) + off)  the kernel forms (mmcv forms it in fp32 as well), so the
    branch decisions (inside / outside, floor, which corners exist) are the reference's own and only the weights and the sum carry
    roundings:  lh = h - floor(h) (exact for h >= 0; one rounding, <= u, for -1 < h < 0), hh = 1 - lh (u more: <= 2u), a weight w = a b
    (d(ab) = da b + a db + u a b), the four products w v (u w |v| each) and the three sums of a four-term chain without contraction
    (each <= u sum w |v|):
        E = sum_i |v_i| (dw_i + u w_i) + 3 u sum_i w_i |v_i|
    The reference is tests/_deform_ref.py in fp64, handed the offsets  h - (oy - 1 + ky)  (exact in fp64, asserted) so that it forms h itself.

tr_dwconv3x3_gelu_kernel   y = 0.5 v (1 + erf(v c)),  v = b + sum of 9 taps x w,  c = 2^-1/2
    9 fma and the bias sum, each rounding bounded by u A, A = |b| + sum |x| |w|:  dv = 10 u A.   t = v c: the rounded constant and the product,
    dt = c dv + 2 u |t|.   erff: derf = (2 / sqrt(pi)) exp(-t^2) dt + ERF_ULPS 2u |erf t|; the sum 1 + erf: u |1 + erf t|; the three products
    0.5 * v * (.): 3 u |y|.
        E = 0.5 |1 + erf t| dv + 0.5 |v| (derf + u |1 + erf t|) + 3 u |y|
    ERF_ULPS = 1.  No accuracy table of ocml ships with the ROCm installation (its headers and share/doc hold none for erff), so the figure
    is measured on the CPU instead: torch-CPU fp32 erf against fp64 over [-6, 6] (4 10^6 points) errs by at most 1.00 ulp;
    tests/test_transref_bounds_cpu.py repeats the measurement and asserts it stays <= ERF_ULPS.

Bit-exact steps (no bound; a reference in torch-CPU fp32, one rounding per operation; transref.hip is built without fp contraction)
    tr_phase_interleave   out[(2a + py) 2W + 2b + px] = phases[2 py + px][a W + b] (+ res: one fp32 sum)
    tr_add                a + b
    tr_prep               x.to(uint8).float().div(255).sub(0.5).div(0.5)          (to_pillow_fn, ToTensor, Normalize(0.5, 0.5))
    tr_pack               TransRef.set_input: byte = mask.byte(); input_DE = fill where byte != 0; mask channels 1 - byte.float()
    tr_blend              out * m + detail * (1 - m)
    tr_to_u8              (x * 127.5 + 127.5).round().clamp(0, 255)

Stage gate (STAGES; tools/make_transref_stage_golden.py, tests/test_transref_stage_gpu.py)   every TransRefNet host stage on its own, at the
    smallest shapes that reach its paths, against the reference's own submodule run on the CPU in fp64 on the same seeded fp32 input.  The
    bound is the control rule with the reference's fp32 run as the control: e_rms <= 2 max(e_rms(fp32), 2^-24), e_max <= 4 max(e_max(fp32),
    2^-24).  No committed file may exceed 1 MiB, so the fixture is two files: tests/golden/transref_stages.npz (fp32 inputs, fp64 outputs) and
    tests/golden/transref_stages_refpa.npz for the three RefPA stages, which need 16 x 16 positions (three stride-2 levels and the 2 x 2 pooling
    of the innermost non-local block) at up to 320 channels: their inputs sit on the 2^-4 grid and are stored as int8, their fp64 outputs as
    an fp32 value plus an int8 residual in units of 2^-8 ulp (pack64 / unpack64: exact to 2^-9 ulp of fp32, asserted by the tool)."""
import math
from collections import OrderedDict

import numpy as np

import torch
import torch.nn.functional as F

import _deform_ref
import _geom_bounds as gb
import _nn_bounds as nb
from _nn_bounds import U, Consts, gen, ratio  # noqa: F401

ERF_ULPS = 1.0
SIZE = 512
FILL = tuple(2 * v / 255.0 - 1.0 for v in (123.0, 104.0, 117.0))       # TransRef.set_input's python floats


def cyc(seq, i):
    return seq[i % len(seq)]


# ================================================================================================ st_tr_attention
ATT_D = (32, 64, 80, 128, 160, 256)
ATT_NK = (1, 31, 32, 33, 64, 65, 100)
ATT_NQ = (1, 31, 32, 33, 127, 128, 129, 300)
ATT_HEADS = (1, 2, 3, 8)
AMPS = (5.0, 20.0, 60.0)                                               # AMPS of tests/test_nn_matrix_gpu.py
ATT_KINDS = ("randn", "dominant", "equal", "rise", "fall")
ATT_LAYOUTS = ("contig", "slices", "kvhalf", "odd")
# (D, Nk, Nq, heads, amp, kind, layout): per D every Nq once and every Nk at least once; the other axes rotate
ATT_CASES = [(D, cyc(ATT_NK, i + a), Nq, cyc(ATT_HEADS, i + a), cyc(AMPS, i + 2 * a), cyc(ATT_KINDS, i + 3 * a), cyc(ATT_LAYOUTS, i + a + i // 4))
             for a, D in enumerate(ATT_D) for i, Nq in enumerate(ATT_NQ)]


def att_id(c):
    return f"d{c[0]}_nk{c[1]}_nq{c[2]}_h{c[3]}_a{int(c[4])}_{c[5]}_{c[6]}"


def consts_tr_attention(Nk):
    nch = -(-Nk // 32)
    return Consts(1, 4, 2 + 2 * nch, 33 * nch, 2 * nch + 5)


def tile_maxima(q, k, heads, D, scale):
    """fp64 row maxima of every 32-key tile: [heads, Nq, ntiles]"""
    qh, kh = (nb.split_heads(t[None].double(), heads, D)[0] for t in (q, k))
    s = scale * (qh @ kh.transpose(-1, -2))
    return torch.stack([s[..., j:j + 32].amax(-1) for j in range(0, s.shape[-1], 32)], -1)


def att_inputs(heads, Nq, Nk, D, amp, kind, seed):
    """fp32 CPU q [Nq, C], k, v [Nk, C], C = heads D, for scale = D^-1/2.  randn / dominant / equal: nb.attn_inputs.  rise / fall: a
    staircase -- every key of tile t scores 3 t (rise) or 3 (ntiles - 1 - t) (fall) plus noise well below 1 against every query, so each
    query's running maximum grows in every 32-key tile (alpha = e^-3 rescales o and lp at every step) or is set by the first tile."""
    if kind in ("randn", "dominant", "equal"):
        return tuple(t[0] for t in nb.attn_inputs(1, heads, Nq, Nk, D, amp, seed, kind))
    C, scale = heads * D, D ** -0.5
    q, k, v = (torch.randn(n, C, generator=gen(seed + i)) * s for i, (n, s) in enumerate(((Nq, 0.25), (Nk, 0.25), (Nk, 1.0))))
    tile = torch.arange(Nk) // 32
    step = 3.0 * (tile if kind == "rise" else tile.max() - tile).float()
    q.view(Nq, heads, D)[..., 0] = 4.0
    k.view(Nk, heads, D)[..., 0] = (step / (4.0 * scale))[:, None]
    tm = tile_maxima(q, k, heads, D, scale)
    d = tm[..., 1:] - tm[..., :-1]
    assert bool((d > 2).all() if kind == "rise" else (d < -2).all())
    return q, k, v


def att_bound(q, k, v, heads, D, scale):
    """-> fp64 (ref, E, max|s|) [Nq, heads D]; the reference is per head (nb.attention_bound)"""
    ref, E, smax = nb.attention_bound(q[None], k[None], v[None], heads, D, scale, consts_tr_attention(k.shape[0]))
    return ref[0], E[0], smax


def att32(q, k, v, heads, D, scale):
    """the control: torch CPU fp32, per head"""
    qh, kh, vh = (nb.split_heads(t.cpu()[None], heads, D) for t in (q, k, v))
    return nb.merge_heads(torch.softmax((qh @ kh.transpose(-1, -2)) * scale, -1) @ vh)[0]


# ================================================================================================ st_tr_deform_im2col
DEFORM_HWC = ((1, 1, 1), (1, 7, 3), (5, 1, 4), (6, 5, 64), (9, 11, 65))
DEFORM_FAMILIES = ("zero", "integer", "frac", "edge_h", "edge_w", "far")
EDGE_SHIFTS = 12


def edge_targets(n):
    """-1, 0, n - 1, n and their float neighbours on both sides: 12 fp32 values"""
    base = torch.tensor([-1.0, 0.0, float(n - 1), float(n)])
    lo, hi = torch.nextafter(base, torch.full_like(base, -1e9)), torch.nextafter(base, torch.full_like(base, 1e9))
    return torch.stack([lo, base, hi], 1).reshape(-1)


def deform_base(H, W):
    """fp32 (oy - 1 + ky, ox - 1 + kx) of every (pixel, tap): [H W, 9] each"""
    p, kk = torch.arange(H * W)[:, None], torch.arange(9)[None, :]
    return (p // W - 1 + kk // 3).float(), (p % W - 1 + kk % 3).float()


def deform_offsets(H, W, family, seed, shift=0):
    """[H W, 18] fp32 offsets (channel 2k = dy, 2k + 1 = dx of tap k).  edge_h / edge_w: the sample's h / w aims at edge_targets, target
    (pixel + tap + shift) % 12, the other coordinate a fraction around its tap; far: +-1e6 and +-3e9 (beyond int range) mixed with fractions"""
    g = gen(seed)
    bh, bw = deform_base(H, W)
    n = H * W
    frac = lambda: torch.randn(n, 9, generator=g)                       # noqa: E731
    if family == "zero":
        dy, dx = torch.zeros(n, 9), torch.zeros(n, 9)
    elif family == "integer":
        dy, dx = (torch.randint(-3, 4, (n, 9), generator=g).float() for _ in range(2))
    elif family == "frac":
        dy, dx = 2.5 * frac(), 2.5 * frac()
    elif family in ("edge_h", "edge_w"):
        idx = (torch.arange(n)[:, None] + torch.arange(9)[None, :] + shift) % 12
        if family == "edge_h":
            dy, dx = (edge_targets(H)[idx].double() - bh.double()).float(), 0.3 * frac()
        else:
            dy, dx = 0.3 * frac(), (edge_targets(W)[idx].double() - bw.double()).float()
    else:
        big = torch.tensor([1e6, -1e6, 3e9, -3e9, 0.0, 0.0])
        i1, i2 = (torch.randint(0, 6, (n, 9), generator=g) for _ in range(2))
        dy, dx = big[i1] + 0.7 * frac(), big[i2] + 0.7 * frac()
    return torch.stack([dy, dx], -1).reshape(n, 18).contiguous()


def deform_coords(off, H, W):
    """the fp32 sums the kernel forms: h, w [H W, 9]"""
    bh, bw = deform_base(H, W)
    o = off.view(H * W, 9, 2)
    return bh + o[..., 0], bw + o[..., 1]


def _cl_to_nchw(x, H, W):
    return x.reshape(H, W, -1).permute(2, 0, 1)[None]


def deform_cols(x, off, H, W, dtype=torch.float64):
    """x [H W, C], off [H W, 18] fp32 -> cols [H W, 9 C] in `dtype` from tests/_deform_ref.py.  fp64: on the fp32 coordinate sums (handed
    over as offsets that reproduce them exactly); fp32: on the offsets themselves, the sum then being the kernel's"""
    C = x.shape[1]
    if dtype == torch.float64:
        h, w = deform_coords(off, H, W)
        bh, bw = deform_base(H, W)
        oy, ox = h.double() - bh.double(), w.double() - bw.double()
        assert bool(((bh.double() + oy) == h.double()).all() and ((bw.double() + ox) == w.double()).all())
        off = torch.stack([oy, ox], -1).reshape(H * W, 18)
    cols = _deform_ref.deform_im2col(_cl_to_nchw(x.to(dtype), H, W), _cl_to_nchw(off.to(dtype), H, W))      # [1, 9, C, H, W]
    return cols[0].permute(2, 3, 0, 1).reshape(H * W, 9 * C)


def deform_bound(x, off, H, W):
    """-> fp64 (ref, E) [H W, 9 C]"""
    C = x.shape[1]
    ref = deform_cols(x, off, H, W)
    h, w = (t.double() for t in deform_coords(off, H, W))
    inside = (h > -1) & (w > -1) & (h < H) & (w < W)
    hl, wl = torch.floor(h), torch.floor(w)
    lh, lw = h - hl, w - wl
    xa = x.double().abs().reshape(H, W, C)
    E = torch.zeros(H * W, 9, C, dtype=torch.float64)
    T = torch.zeros_like(E)
    for dy, dx, a, da, b, db in ((0, 0, 1 - lh, 2 * U, 1 - lw, 2 * U), (0, 1, 1 - lh, 2 * U, lw, U), (1, 0, lh, U, 1 - lw, 2 * U), (1, 1, lh, U, lw, U)):
        yy, xx = (hl + dy).long(), (wl + dx).long()
        ok = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        v = xa[yy.clamp(0, H - 1), xx.clamp(0, W - 1)] * ok[..., None]
        wgt = (a * b)[..., None]
        E += v * ((da * b + a * db)[..., None] + 2 * U * wgt)
        T += wgt * v
    return ref, (E + 3 * U * T).reshape(H * W, 9 * C)


def im2col_zero_padded(x, H, W):
    """the plain 3x3 / pad 1 im2col, (ky, kx, c) order: what zero offsets must give bit for bit"""
    C = x.shape[1]
    P = F.pad(x.reshape(H, W, C), (0, 0, 1, 1, 1, 1))
    return torch.stack([P[ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], 2).reshape(H * W, 9 * C)


# ================================================================================================ st_tr_phase_interleave, st_tr_add
PHASE_HWC = ((1, 1, 1), (1, 5, 3), (4, 1, 2), (3, 5, 48), (7, 6, 65))


def phase_interleave(ph, H, W, res=None, transposed=False):
    """ph [4, H W, C] -> [(2H)(2W), C] by torch indexing; `transposed`: the planted defect (phase 2 px + py)"""
    C = ph.shape[-1]
    out = torch.empty(2 * H, 2 * W, C, dtype=ph.dtype, device=ph.device)
    for py in (0, 1):
        for px in (0, 1):
            out[py::2, px::2] = ph[2 * px + py if transposed else 2 * py + px].reshape(H, W, C)
    out = out.reshape(4 * H * W, C)
    return out if res is None else out + res


# ================================================================================================ st_tr_dwconv3x3_gelu
DW_HWC = ((1, 1, 1), (1, 9, 5), (7, 1, 64), (2, 2, 3), (5, 6, 130))
DW_AMPS = (1.0, 4.0, 12.0)                                             # v = b + sum x w has std ~ amp: 4 and 12 reach both GELU tails


def dw_inputs(H, W, C, amp, seed):
    """x [H W, C], w9c [9, C] (tap-major), bias [C]"""
    g = gen(seed)
    return amp * torch.randn(H * W, C, generator=g), torch.randn(9, C, generator=g) / 3, 0.1 * torch.randn(C, generator=g)


def dw_conv(x, w9c, b, H, W, dtype):
    C = x.shape[1]
    return F.conv2d(_cl_to_nchw(x.to(dtype), H, W), w9c.to(dtype).t().reshape(C, 1, 3, 3), b.to(dtype), padding=1, groups=C)


def dw_gelu(x, w9c, b, H, W, dtype=torch.float64):
    """-> [H W, C] in `dtype`: nn.GELU() of the depthwise convolution, as TransRef.py's Mlp runs it"""
    return F.gelu(dw_conv(x, w9c, b, H, W, dtype))[0].permute(1, 2, 0).reshape(H * W, -1)


def dw_bound(x, w9c, b, H, W):
    """-> fp64 (ref, E) [H W, C]"""
    cl = lambda t: t[0].permute(1, 2, 0).reshape(H * W, -1)             # noqa: E731
    v = cl(dw_conv(x, w9c, b, H, W, torch.float64))
    A = cl(dw_conv(x.abs(), w9c.abs(), b.abs(), H, W, torch.float64))
    c = math.sqrt(0.5)
    t = v * c
    erf = torch.erf(t)
    y = 0.5 * v * (1 + erf)
    dv = 10 * U * A
    dt = c * dv + 2 * U * t.abs()
    derf = 2 / math.sqrt(math.pi) * torch.exp(-t * t) * dt + ERF_ULPS * 2 * U * erf.abs()
    E = 0.5 * (1 + erf).abs() * dv + 0.5 * v.abs() * (derf + U * (1 + erf).abs()) + 3 * U * y.abs()
    return y, E


# ================================================================================================ wrapper steps (torch-CPU fp32, bit for bit)
def prep_ref(x, rounding=False):
    """to_pillow_fn, ToTensor, Normalize(0.5, 0.5); `rounding`: the planted defect (round instead of truncate)"""
    x = x.round() if rounding else x
    return x.to(torch.uint8).float().div(255).sub(0.5).div(0.5)


def prep_values():
    """every integer 0..255 with the fractions .0, .5 and .999, then -0.9 and 255.99: 770 fp32 values"""
    k = torch.arange(256, dtype=torch.float64)
    return torch.cat([(k[:, None] + torch.tensor([0.0, 0.5, 0.999], dtype=torch.float64)[None, :]).reshape(-1),
                      torch.tensor([-0.9, 255.99], dtype=torch.float64)]).float()


def prep_inputs(hw, seed):
    """img3, ctl3 [3, hw]: the values of prep_values in two different rotations"""
    vals = prep_values()
    idx = torch.arange(3 * hw)
    return vals[(idx + seed) % 770].reshape(3, hw).contiguous(), vals[(7 * idx + seed + 3) % 770].reshape(3, hw).contiguous()


def pack_masks(n, seed):
    """[n] fp32: values of [0, 1] (0, 1 and nextafter(1, 0) among them) and 1.5, 2.0, 255.0, 255.9, 256.0"""
    special = torch.tensor([0.0, 1.0, 1.0, 1.5, 2.0, 255.0, 255.9, 256.0, 0.5, 0.0])
    special[2] = torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))
    m = torch.rand(n, generator=gen(seed))
    idx = torch.arange(n)
    return torch.where(idx % 3 == 0, m, special[(idx // 3) % 10])


def pack_ref(rs6, mask):
    """rs6 [6, n], mask [n] -> x6 [n, 6], ref3 [n, 3], detail3 [3, n] as TransRef.set_input / forward build them (byte = mask.byte(),
    masked_fill_ of input_DE where the byte is nonzero, mask channels 1 - byte)"""
    byte = mask.to(torch.int64).remainder(256).to(torch.uint8)         # .byte() of a float: the integer part modulo 256
    detail = rs6[:3].clone()
    for c in range(3):
        detail[c].masked_fill_(byte.bool(), FILL[c])
    inv = torch.add(torch.neg(byte.float()), 1).float()
    x6 = torch.cat([detail, inv[None].expand(3, -1)], 0).t().contiguous()
    return x6, rs6[3:].t().contiguous(), detail


def blend_ref(out3, detail3, mask):
    """out3 [n, 3], detail3 [3, n], mask [1 or 3, n] -> [3, n]: out * m + detail * (1 - m), one fp32 rounding per operation"""
    return out3.t() * mask + detail3 * (1 - mask)


def to_u8_ref(x, half_away=False):
    """(x * 127.5 + 127.5).round().clamp(0, 255) as uint8; `half_away`: the planted defect (halves away from zero)"""
    y = x * 127.5 + 127.5
    y = torch.floor(y + 0.5) if half_away else y.round()
    return y.clamp(0, 255).to(torch.uint8)


def to_u8_inputs():
    """a dense sweep of [-1.2, 1.2], the fp32 preimage (k - 127) / 127.5 of every k + 0.5 with both float neighbours, -0.0 and +-1"""
    x = (torch.arange(-1, 257, dtype=torch.float64) - 127.0) / 127.5
    x = x.float()
    nxt = lambda t, d: torch.nextafter(t, torch.full_like(t, d))        # noqa: E731
    return torch.cat([torch.linspace(-1.2, 1.2, 20001), x, nxt(x, -9.0), nxt(x, 9.0), torch.tensor([-0.0, 1.0, -1.0])]).contiguous()


# ================================================================================================ Inpainter.prepare / finish
ORIGINS = ((1, 1), (3, 5), (172, 150), (512, 512), (600, 520))


def wrapper_inputs(H, W, seed):
    """init / control [1, 3, H, W] with fractions (to_pillow_fn truncates them) and a binary 3-plane mask [1, 3, H, W]: blobs and a border band"""
    g = gen(seed)
    init = gb.image(1, 3, H, W, seed) + 0.7 * torch.rand(1, 3, H, W, generator=g)
    ctl = gb.image(1, 3, H, W, seed + 1).flip(3) + 0.3
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    m = ((yy * 7 + xx * 3) % 23 < 6) | (yy < H // 9) | (xx >= W - W // 11) | (torch.rand(H, W, generator=g) < 0.03)
    return init.float().contiguous(), m.float()[None, None].expand(1, 3, H, W).contiguous(), ctl.float().contiguous()


def prepare_ref(init, mask, ctl):
    """-> (planes6 [6, H, W] torch-CPU fp32, exact;  hole [512, 512] bool from torch-CPU F.interpolate(mask).byte();  fp64 (ref, E) [6, 512,
    512] of the resize of planes6, tests/_geom_bounds.resize_bound, align_corners = False)"""
    planes6 = torch.cat([prep_ref(init[0]), prep_ref(ctl[0])], 0)
    mrs = F.interpolate(mask, size=[SIZE, SIZE], mode="bilinear")
    hole = mrs[0, 0].byte().bool()
    ref, E = gb.resize_bound(planes6[None], SIZE, SIZE, 0)
    return planes6, mrs[0], hole, ref[0], E[0]


def finish_ref(out3, detail3, mrs, hw):
    """out3 [n, 3], detail3 [3, n], mrs [planes, 512, 512] (CPU fp32) -> (torch-CPU fp32 bytes [3, H, W], fp64 pre-round value, 127.5 E_resize)"""
    fake = blend_ref(out3, detail3, mrs.reshape(mrs.shape[0], -1)).view(1, 3, SIZE, SIZE)
    back = F.interpolate(fake, size=list(hw), mode="bilinear")
    u8 = (back * 127.5 + 127.5).round().clamp(0, 255).to(torch.uint8)[0]
    ref, E = gb.resize_bound(fake, hw[0], hw[1], 0)
    return u8, ref[0] * 127.5 + 127.5, 127.5 * E[0]


# ================================================================================================ stage gate
STAGE_SEED = 2024
_OE = "Tenc.RefPA1.PA.offset_estimator."
# name -> kind, the reference's submodule, the TransRefNet parameter prefix, (H, W), input channel counts, arguments of the TransRefNet method
STAGES = OrderedDict([
    # Block of the four encoder stages (heads, sr): 9 x 6 at sr 4 -> 2 x 1 keys, 5 x 7 and 3 x 5 at sr 2 -> 2 x 3 and 1 x 2, 3 x 3 at sr 1
    ("block1", ("block", "Tenc.block1.0", "Tenc.block1.0", (9, 6), (64,), (1, 4))),
    ("block2", ("block", "Tenc.block2.0", "Tenc.block2.0", (5, 7), (128,), (2, 2))),
    ("block3", ("block", "Tenc.block3.0", "Tenc.block3.0", (3, 5), (320,), (4, 2))),
    ("block4", ("block", "Tenc.block4.0", "Tenc.block4.0", (3, 3), (512,), (4, 1))),
    ("patch_block1", ("block_ref", "Tenc.patch_block1.0", "Tenc.patch_block1.0", (5, 6), (128, 128), (1, 4))),
    ("patch_block2", ("block_ref", "Tenc.patch_block2.0", "Tenc.patch_block2.0", (3, 5), (320, 320), (2, 2))),
    ("patch_block3", ("block_ref", "Tenc.patch_block3.0", "Tenc.patch_block3.0", (3, 3), (512, 512), (2, 2))),
    ("dec_block", ("block", "Tdec.block1.0", "Tdec.block1.0", (3, 3), (512,), (8, 1))),
    ("nonlocal_even", ("nonlocal", _OE + "attentionblock1", _OE + "attentionblock1", (4, 6), (64, 64), ())),
    ("nonlocal_odd", ("nonlocal", _OE + "attentionblock2", _OE + "attentionblock2", (5, 7), (64, 64), ())),
    ("embed_k7s4", ("embed", "Tenc.patch_embed1", "Tenc.patch_embed1", (13, 10), (6,), (7, 4))),
    ("embed_k3s2", ("embed", "Tenc.patch_embed2", "Tenc.patch_embed2", (7, 5), (64,), (3, 2))),
    ("convT3_1x3", ("convT", _OE + "upblock1", _OE + "upblock1.0", (1, 3), (64,), ("lrelu",))),
    ("convT3_5x4", ("convT", _OE + "upblock1", _OE + "upblock1.0", (5, 4), (64,), ("lrelu",))),
    ("convT4_1x3", ("convT", "convtail.convd4x", "convtail.convd4x.conv2d", (1, 3), (128, 64), ("none",))),
    ("convT4_5x4", ("convT", "convtail.convd4x", "convtail.convd4x.conv2d", (5, 4), (128, 64), ("none",))),
    ("res_skip", ("res", "convtail.dense_2", "convtail.dense_2.0", (5, 4), (64, 64), ())),
    ("res_plain", ("res", "convtail.dense_1", "convtail.dense_1.0", (5, 4), (16,), ())),
    ("clean_tanh", ("clean", "clean", "clean.conv2d", (5, 7), (8,), ())),
    ("refpa1", ("refpa", "Tenc.RefPA1", "Tenc.RefPA1", (16, 16), (64, 64), ())),
    ("refpa2", ("refpa", "Tenc.RefPA2", "Tenc.RefPA2", (16, 16), (128, 128), ())),
    ("refpa3", ("refpa", "Tenc.RefPA3", "Tenc.RefPA3", (16, 16), (320, 320), ())),
])
STAGE_FILES = ("transref_stages.npz", "transref_stages_refpa.npz")
STAGE_FILE_CAP = 1 << 20


def stage_file(name):
    return STAGE_FILES[STAGES[name][0] == "refpa"]


def stage_inputs(name):
    """seeded fp32 channels-last inputs [rows, C]; the residual of a transposed convolution has 4 H W rows; RefPA's sit on the 2^-4 grid"""
    kind, _, _, (H, W), cin, _ = STAGES[name]
    out = []
    for j, c in enumerate(cin):
        rows = H * W * (4 if kind == "convT" and j == 1 else 1)
        x = torch.randn(rows, c, generator=gen(STAGE_SEED + 100 * list(STAGES).index(name) + j))
        out.append((x * 16).round().clamp(-127, 127) / 16 if kind == "refpa" else x)
    return out


def stage_out_shape(name):
    kind, _, _, (H, W), cin, args = STAGES[name]
    if kind == "embed":
        k, s = args
        return (((H + 2 * (k // 2) - k) // s + 1) * ((W + 2 * (k // 2) - k) // s + 1), {6: 64, 64: 128}[cin[0]])
    if kind == "convT":
        return (4 * H * W, 64)
    return (H * W, 3 if kind == "clean" else cin[0])


def pack64(x):
    """fp64 -> (fp32 hi, int8 lo) with x ~ hi + lo spacing(hi) / 256"""
    hi = x.float()
    ulp = torch.from_numpy(np.spacing(np.abs(hi.numpy()))).double()
    lo = ((x - hi.double()) / ulp * 256).round().clamp(-128, 127).to(torch.int8)
    return hi, lo


def unpack64(hi, lo):
    ulp = torch.from_numpy(np.spacing(np.abs(hi.numpy()))).double()
    return hi.double() + lo.double() * ulp / 256


def load_stage(gold, name):
    """gold: {file: the loaded npz} -> (fp32 inputs, fp64 output, (e_rms, e_max) of the reference's fp32 run)"""
    z = gold[stage_file(name)]
    n = len(STAGES[name][4])
    if STAGES[name][0] == "refpa":
        ins = [torch.from_numpy(z[f"{name}.in{j}"]).float() / 16 for j in range(n)]
        out = unpack64(torch.from_numpy(z[f"{name}.out_hi"]), torch.from_numpy(z[f"{name}.out_lo"]))
    else:
        ins = [torch.from_numpy(z[f"{name}.in{j}"]) for j in range(n)]
        out = torch.from_numpy(z[f"{name}.out64"])
    return ins, out, tuple(float(v) for v in z[f"{name}.e32"])


def stage_errs(x, ref):
    x, ref = x.double().reshape(-1), ref.reshape(-1)
    return ((x - ref).norm() / ref.norm()).item(), ((x - ref).abs().max() / ref.abs().max()).item()
