"""fp64 references and first-order worst-case elementwise error bounds for the kernels of csrc/nn.hip (attention in its three forms,
LayerNorm, row softmax, L2 normalisation, the latent pooling and the CCL soft-argmax), and the input generators that
tests/test_nn_bounds_cpu.py and tests/test_nn_matrix_gpu.py share.  Every reference states the operation's definition in torch fp64 and
knows nothing of a kernel's tiling; every bound E is a sum of the roundings the kernel performs, each taken at its worst, to first order in
u = 2^-24.  No constant here comes from a GPU measurement: each is a count read from the kernel text, given below.

Softmax pooling  y_d = sum_j p_j v_jd,  p = softmax(s)   (attention: s = scale q.k;  latent pooling: s given)
    A computed probability weight is  exp(s_j - m)(1 + e_j)  with |e_j| <= tau_j,

        tau_j = u ((D + pre) S_j + n_sub |s_j - m| + n_exp),        S_j = |scale| |q|.|k_j|  (fp64)

    (D + pre) S_j  the score: a D-term fma / MFMA chain (<= D roundings, each bounded by u S_j) and `pre` roundings of the scaled query or
                   of the scaled score; an absolute score error is a relative error of exp(s).
    n_sub |s - m|  roundings of the exponent's argument, each relative to |s_j - m|: the subtraction of the row maximum (the maximum is one
                   of the computed scores and softmax is invariant to the shift, so only the rounding of the difference counts) and, where
                   the exponential is exp2(x log2 e), that product and the rounding of the constant.
    n_exp          the exponential itself: v_exp_f32 is good to 1 ulp <= 2u.
    Normalising by the computed sum turns e_j into e_j - sum_k p_k e_k, and the two sums add their chains:

        E_d = sum_j p_j |v_jd| (tau_j + sum_k p_k tau_k)  +  u (n_acc + n_sum + 2) sum_j p_j |v_jd|  +  2^-125 sum_j |v_jd|

    n_acc / n_sum: roundings along the longest chain of the numerator / of the denominator; + 2: 1 / sum and the product with it.  The last
    term is the fp32 underflow floor: a weight below 2^-126 is flushed to zero (the same floor as the softmax rows below).

    kernel                                         pre  n_sub  n_exp        n_acc          n_sum
    attention_kv_mfma_kernel, window_attention      3     1     2           Nk/2 + 1       Nk/4 + 2
        Q is multiplied by sl = scale * log2e: the constant's rounding, the product scale * log2e, the product q * sl (pre = 3); the
        exponent is a bare v_exp_f32 of sc - mx (n_sub = 1); two accumulator chains (keys r even / odd) of two 4-deep MFMAs per key tile
        = Nk / 2 roundings each, + 1 for the fold; a lane adds its Nk / 4 weights, two shuffles finish the sum.  The window kernel runs
        this on a 64-row slab whatever ws is (masked keys add exact zeros): Nk = 64.
    attention_small_kernel                          1     3     2           Nk             Nk
        q * scale before the chain (pre = 1); s - mx, then __expf = v_exp_f32(x * log2e): difference, product, constant (n_sub = 3).
    attention_kvlds_kernel (VALU, online softmax)   1     6     2 + 2 nch   Nk + nch       Nk + nch        nch = ceil(Nk / 8)
        q * scale before the chain (pre = 1).  A chunk's weights are taken against the running maximum and every later chunk rescales the
        accumulators by corr = __expf(mx - nm): the arguments of the later corr's telescope to m - nm(chunk of j) <= |s_j - m|, so the three
        argument roundings count twice (n_sub = 6); each corr adds 2u to the weights before it (n_exp) and one rounding to each
        accumulator (n_acc, n_sum).
    latent_pool_kernel (no S term)                  -     3     2           P              P / 2 + 1
        __expf(a - mx); a lane adds P / 2 weights and one shuffle; P / 2 MFMAs of depth 2.

LayerNorm  y = (x - mu) r w + b,  r = (var + eps)^-1/2
    n_s = roundings along the longest summation chain: layernorm_kernel 16 per-lane adds + 6 shuffles = 22; layernorm128_kernel
    (x + y) + (z + w) = 2, + 5 shuffles = 7 (the product with 1/128 is exact).  With d = x - mu:
        dmu = u (n_s + 2) mean|x|                                      the sum and the division by C
        E = |w| r (dmu + u |d| + |d| (u (n_s + 6) + dmu sum|d| / (sum d^2 + C eps))) + 2u |y| + u |d r w|
    dmu + u|d|: the computed d;  u (n_s + 6): r -- squares, chain, division, + eps, square root, reciprocal, more than the half of the variance's
    relative error that reaches r;  dmu sum|d| / (sum d^2 + C eps): the shifted mean inside the variance (2 dmu sum|d| relative to C (var + eps),
    halved by the root);  2u|y| + u|d r w|: the two products and the final sum.

Softmax rows (softmax_rows_kernel; expf is ocml's, not the native form)  a = |x - m|
        E_j = u y_j (2 a_j + n_s + 6 + sum_k y_k (2 a_k + 2)) + 2^-125,      n_s = 16 per-thread adds + 6 shuffles + 2 across the waves = 24
    2 a_j covers the subtraction and the argument handling of expf, 6 >= 2 (exp, 1 ulp) + 1 (division) with slack; 2^-125: a term and a quotient
    flushed below 2^-126.

l2norm_rows   E = u |y| (n_s + 4) + 2^-125,  n_s = ceil(C / 64) + 6: a lane's fma chain and the shuffles (half of it reaches the norm), the root,
    the quotient.

ccl_softargmax   vol_q = 10 sum_9 G taps:  9 adds and the product, each bounded through Sg = sum of the 9 |n1|.|n2| (>= sum |G|):
        tau_q = u (100 Sg_q + 2 a_q + 2),   n_s = 4 per-thread adds + 6 shuffles + 2 across the waves = 12
        E = sum_q p_q |dx_q| (tau_q + sum_k p_k tau_k + u (2 n_s + 2)) + 2^-125 sum_q |dx_q|
    (2 n_s + 2: the chains of e and of e * dx, the product e * dx, the division).  The reference is the statement of network.py:147-199 --
    the 3x3 patches of n2 are the filters of a convolution over n1 -- not the kernel's sum over diagonals of G."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

U = 2.0 ** -24
FLOOR = 2.0 ** -125
LOG2E = 1.44269504088896340736

Consts = namedtuple("Consts", "pre n_sub n_exp n_acc n_sum")
LN_NS_GENERIC, LN_NS_128 = 22, 7
SOFTMAX_NS = 24
CCL_NS = 12


def consts_mfma(Nk):
    return Consts(3, 1, 2, Nk // 2 + 1, Nk // 4 + 2)


def consts_window():
    return consts_mfma(64)


def consts_small(Nk):
    return Consts(1, 3, 2, Nk, Nk)


def consts_kvlds_valu(Nk):
    nch = (Nk + 7) // 8
    return Consts(1, 6, 2 + 2 * nch, Nk + nch, Nk + nch)


def consts_latent_pool(P):
    return Consts(0, 3, 2, P, P // 2 + 1)


def ratio(out, ref, E):
    """max |out - ref| / E; 0 / 0 = 0; an element that is NaN (never written, or an overflow) or wrong where E = 0 gives inf"""
    err = (out.double() - ref).abs()
    r = torch.where(E > 0, err / E.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")))
    r = r.max().item() if r.numel() else 0.0
    return float("inf") if math.isnan(r) else r


# ------------------------------------------------------------------------------------------------ softmax pooling / attention
def pool_bound(s, S, v, c, D=0):
    """s [..., Nq, Nk] fp64 logits, S their absolute companion or None, v [..., Nk, Dv] fp64 -> (softmax(s) v, E)"""
    a = s.amax(-1, keepdim=True) - s
    p = torch.softmax(s, -1)
    tau = U * (c.n_sub * a + c.n_exp)
    if S is not None:
        tau = tau + U * (D + c.pre) * S
    tbar = (p * tau).sum(-1, keepdim=True)
    av = v.abs()
    E = (p * (tau + tbar)) @ av + U * (c.n_acc + c.n_sum + 2) * (p @ av) + FLOOR * av.sum(-2, keepdim=True)
    return p @ v, E


def split_heads(t, heads, D):
    """[B, N, heads * D] -> [B, heads, N, D]"""
    return t.reshape(t.shape[0], t.shape[1], heads, D).transpose(1, 2)


def merge_heads(t):
    """[B, heads, N, D] -> [B, N, heads * D]"""
    return t.transpose(1, 2).reshape(t.shape[0], t.shape[2], -1)


def attention_bound(q, k, v, heads, D, scale, c):
    """q [B or 1, Nq, heads D], k / v [B, Nk, heads D] (any float dtype, any device) -> fp64 (ref, E, max|s|), ref / E [B, Nq, heads D]"""
    q, k, v = (split_heads(t.double(), heads, D) for t in (q, k, v))
    s = scale * (q @ k.transpose(-1, -2))
    S = abs(scale) * (q.abs() @ k.abs().transpose(-1, -2))
    ref, E = pool_bound(s, S, v, c, D)
    return merge_heads(ref), merge_heads(E), s.abs().max().item()


def to_windows(t, pad, B, H, W, ws):
    """image tokens [B, H W, C] and the pad table [ws ws, C] -> [B nwh nww, ws ws, C]: the grid is padded on the bottom / right to whole
    windows and a padded token carries the table row of its window position (twins.py:587-600)"""
    C = t.shape[-1]
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    full = pad.reshape(1, 1, ws, 1, ws, C).expand(B, Hp // ws, ws, Wp // ws, ws, C).reshape(B, Hp, Wp, C).clone()
    full[:, :H, :W] = t.reshape(B, H, W, C)
    return full.reshape(B, Hp // ws, ws, Wp // ws, ws, C).transpose(2, 3).reshape(-1, ws * ws, C)


def from_windows(o, B, H, W, ws):
    """[B nwh nww, ws ws, C] -> the image tokens [B, H W, C]"""
    C = o.shape[-1]
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    return o.reshape(B, Hp // ws, Wp // ws, ws, ws, C).transpose(2, 3).reshape(B, Hp, Wp, C)[:, :H, :W].reshape(B, H * W, C)


def window_attention_bound(q, k, v, qpad, kpad, vpad, B, H, W, heads, D, ws, scale):
    """-> fp64 (ref, E) [B, H W, heads D]: attention inside each ws x ws window of the padded grid, every one of its ws ws tokens a key"""
    qw, kw, vw = (to_windows(t.double(), p.double(), B, H, W, ws) for t, p in ((q, qpad), (k, kpad), (v, vpad)))
    ref, E, _ = attention_bound(qw, kw, vw, heads, D, scale, consts_window())
    return from_windows(ref, B, H, W, ws), from_windows(E, B, H, W, ws)


def latent_pool_bound(scores, tokens, M, P):
    """scores [M P, 64], tokens [M P, 128] -> fp64 (ref, E) [M, 64, 128]: softmax over the P tokens of a pixel for each of the 64 rows"""
    s = scores.double().reshape(M, P, 64).transpose(1, 2)
    return pool_bound(s, None, tokens.double().reshape(M, P, 128), consts_latent_pool(P))


# ------------------------------------------------------------------------------------------------ row kernels
def layernorm_bound(x, w, b, eps, n_s):
    x, w, b = x.double(), w.double(), b.double()
    C = x.shape[-1]
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    sd2 = (d * d).sum(-1, keepdim=True)
    r = 1.0 / torch.sqrt(sd2 / C + eps)
    y = d * r * w + b
    dmu = U * (n_s + 2) * x.abs().mean(-1, keepdim=True)
    E = w.abs() * r * (dmu + U * d.abs() + d.abs() * (U * (n_s + 6) + dmu * d.abs().sum(-1, keepdim=True) / (sd2 + C * eps))) \
        + 2 * U * y.abs() + U * (d * r * w).abs()
    return y, E


def softmax_rows_bound(x):
    x = x.double()
    a = x.amax(-1, keepdim=True) - x
    y = torch.softmax(x, -1)
    E = U * y * (2 * a + SOFTMAX_NS + 6 + (y * (2 * a + 2)).sum(-1, keepdim=True)) + FLOOR
    return y, E


def l2norm_bound(x):
    x = x.double()
    y = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return y, U * y.abs() * (-(-x.shape[-1] // 64) + 6 + 4) + FLOOR


def ccl_volume(n1, n2, B, h, w, dtype=torch.float64):
    """[B, filter q, pixel p]: every 3x3 patch of the zero-padded n2 as a filter of a convolution over the zero-padded n1"""
    P, C = h * w, n1.shape[-1]
    a, b = (t.to(dtype).reshape(B, h, w, C).permute(0, 3, 1, 2) for t in (n1, n2))
    patches = F.pad(b, (1, 1, 1, 1)).unfold(2, 3, 1).unfold(3, 3, 1)                       # [B, C, h, w, 3, 3]
    filt = patches.permute(0, 2, 3, 1, 4, 5).reshape(B, P, C, 3, 3)
    return torch.cat([F.conv2d(a[i:i + 1], filt[i], padding=1) for i in range(B)]).reshape(B, P, P)


def ccl_displacements(h, w, device, dtype):
    """(dx, dy) [q, p]: the filter's position minus the pixel's"""
    idx = torch.arange(h * w, device=device)
    return tuple((f(idx)[:, None] - f(idx)[None, :]).to(dtype) for f in (lambda t: t % w, lambda t: t // w))


def ccl_forward(n1, n2, B, h, w, dtype=torch.float64):
    """n1, n2 [B, h w, C] -> [B, h w, 2] = (flow_w, flow_h): softmax over the filters at temperature 10, then the expected displacement"""
    p = torch.softmax(10.0 * ccl_volume(n1, n2, B, h, w, dtype), 1)
    return torch.stack([(p * d).sum(1) for d in ccl_displacements(h, w, n1.device, dtype)], -1)


def ccl_bound(n1, n2, B, h, w):
    """-> fp64 (ref, E) [B, h w, 2]"""
    s, Sg = 10.0 * ccl_volume(n1, n2, B, h, w), ccl_volume(n1.abs(), n2.abs(), B, h, w)
    p = torch.softmax(s, 1)
    a = s.amax(1, keepdim=True) - s
    tau = U * (100.0 * Sg + 2 * a + 2)
    tbar = (p * tau).sum(1, keepdim=True)
    E = [(p * d.abs() * (tau + tbar + U * (2 * CCL_NS + 2))).sum(1) + FLOOR * d.abs().sum(0) for d in ccl_displacements(h, w, n1.device, torch.float64)]
    return ccl_forward(n1, n2, B, h, w), torch.stack(E, -1)


# ------------------------------------------------------------------------------------------------ inputs
def gen(seed):
    return torch.Generator().manual_seed(seed)


def attn_inputs(B, heads, Nq, Nk, D, amp, seed, kind="randn", bq=False):
    """fp32 CPU q [B or 1, Nq, C], k, v [B, Nk, C], C = heads D, for scale = D^-1/2.
    randn: q scaled so that max|s| over the whole case is `amp`;  equal: the same with every key the first one;  qzero: q = 0;
    dominant: per (batch, head) one key (its index varies) whose score is ahead of every other by more than 100."""
    C, scale = heads * D, D ** -0.5
    q = torch.randn(1 if bq else B, Nq, C, generator=gen(seed))
    k, v = torch.randn(B, Nk, C, generator=gen(seed + 1)), torch.randn(B, Nk, C, generator=gen(seed + 2))
    if kind == "equal":
        k = k[:, :1].expand(-1, Nk, -1).clone()
    if kind == "qzero":
        q.zero_()
    elif kind == "dominant":
        q, k = 0.25 * q, 0.25 * k
        qh, kh = q.view(-1, Nq, heads, D), k.view(B, Nk, heads, D)
        qh[..., 0], kh[..., 0] = 8.0, 0.0
        for b in range(B):
            for h in range(heads):
                kh[b, (5 * b + 3 * h + Nk // 2) % Nk, h, 0] = 20.0 / scale                  # score 160 against |others| of a few
    else:
        s = scale * (split_heads(q, heads, D) @ split_heads(k, heads, D).transpose(-1, -2))
        q = q * (amp / s.abs().max().item())
    return q.contiguous(), k.contiguous(), v.contiguous()


def ln_inputs(rows, C, mean, seed, const_row=None):
    """unit-std rows around `mean`; `const_row`: that row holds one value throughout"""
    x = torch.randn(rows, C, generator=gen(seed)) + mean
    if const_row is not None:
        x[const_row] = x[const_row, 0].item()
    return x, torch.randn(C, generator=gen(seed + 1)), torch.randn(C, generator=gen(seed + 2))


def softmax_inputs(rows, C, amp, seed):
    return torch.randn(rows, C, generator=gen(seed)) * amp


def ccl_inputs(B, h, w, C, seed):
    """features on the 2^-6 grid, |.| <= 2: every product of two is a multiple of 2^-12 and a sum of C <= 64 of them is below 2^8, so the all-pairs
    product G is exact in fp32 (and in fp64) and the kernel, which takes G, sees the same numbers as the reference, which takes n1 and n2"""
    n = [(torch.randn(B, h * w, C, generator=gen(seed + i)) * 0.25 * 64).round().clamp(-128, 128) / 64 for i in range(2)]
    return n[0], n[1]
