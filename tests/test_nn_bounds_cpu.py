"""The bounds of tests/_nn_bounds.py, shown on the CPU to be neither wrong nor vacuous, and the argument guards of csrc/nn.hip.

1. A bound that fp32 itself breaks is wrong: every bound is held against fp32 evaluations of the same operation on the generators the GPU
   file uses -- torch's own fp32, and a restatement in the kernel's order (log2-domain attention with exp2 as the MFMA kernels run it, the
   chunked online softmax of the VALU kernel, the 64-row masked slab of the window kernel, two-pass LayerNorm).  err / E <= 1 elementwise.
2. A bound that a real defect meets is vacuous: five planted errors, each of which must give err / E > 1 on at least one case of every
   amplitude family of its generator.  `max_first_chunk` is the online form with the rescale dropped (a chunk is exponentiated against the
   running maximum, the accumulators stay on the first chunk's): one wrong shift applied to every key alike is invisible by construction,
   softmax being shift invariant, and would only show through an overflow.
3. The entry points reject what their kernels cannot take before any launch: host code only, no pointer is dereferenced."""
import pytest
import torch

import _nn_bounds as nb

AMPS = (5.0, 20.0, 60.0)
# (B, heads, Nq, Nk, D): MFMA-shaped, VALU-shaped and small-shaped cases of the GPU tables, cut down in Nq
ATTN_CASES = [(1, 3, 17, 16, 16), (2, 1, 33, 48, 32), (1, 2, 40, 112, 16), (1, 1, 24, 256, 32), (1, 2, 19, 7, 16), (1, 1, 21, 12, 32),
              (1, 1, 18, 100, 16), (1, 1, 9, 300, 32), (2, 3, 8, 8, 8), (1, 2, 1, 64, 8), (1, 1, 8, 200, 16), (1, 1, 5, 1000, 16)]


def f32(x):
    return torch.tensor(x, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ fp32 attention, three orders
def att_torch32(q, k, v, scale):
    return torch.softmax((q @ k.transpose(-1, -2)) * scale, -1) @ v


def att_log2(q, k, v, scale, mask_from=None):
    """the MFMA kernels' order: scale * log2e folded into q, scores in the log2 domain, exp2 of the difference to the row maximum, one
    division at the end; `mask_from`: keys from that index on are masked to -inf (the window kernel's slab)"""
    t = (q * (f32(scale) * f32(nb.LOG2E))) @ k.transpose(-1, -2)
    if mask_from is not None:
        t[..., mask_from:] = float("-inf")
    p = torch.exp2(t - t.amax(-1, keepdim=True))
    return (p @ v) / p.sum(-1, keepdim=True)


def att_online(q, k, v, scale, rescale=True):
    """the VALU kernel's order: q * scale, chunks of 8 keys against a running maximum, the accumulators rescaled chunk by chunk"""
    s = (q * f32(scale)) @ k.transpose(-1, -2)
    mx = torch.full(s.shape[:-1] + (1,), float("-inf"))
    acc, tot = torch.zeros(q.shape[:-1] + (v.shape[-1],)), torch.zeros(s.shape[:-1] + (1,))
    for j0 in range(0, s.shape[-1], 8):
        sc = s[..., j0:j0 + 8]
        nm = torch.maximum(mx, sc.amax(-1, keepdim=True))
        if rescale or j0 == 0:
            corr = torch.exp(mx - nm)
            acc, tot = acc * corr, tot * corr
        mx = nm
        p = torch.exp(sc - nm)
        acc, tot = acc + p @ v[..., j0:j0 + 8, :], tot + p.sum(-1, keepdim=True)
    return acc / tot


def heads_of(q, k, v, heads, D):
    return tuple(nb.split_heads(t, heads, D) for t in (q, k, v))


def attn_ratio(fn, q, k, v, heads, D, c, kq=None, **kw):
    """err / E of fn on the head-split fp32 inputs against the fp64 reference of (q, k, v); kq: the (k, v) that fn is handed instead"""
    ref, E, _ = nb.attention_bound(q, k, v, heads, D, D ** -0.5, c)
    qh, kh, vh = heads_of(q, *(kq or (k, v)), heads, D)
    return nb.ratio(nb.merge_heads(fn(qh, kh, vh, D ** -0.5, **kw)), ref, E)


@pytest.mark.parametrize("amp", AMPS)
@pytest.mark.parametrize("kind", ["randn", "equal"])
def test_attention_bounds_hold_for_fp32(amp, kind):
    for i, (B, heads, Nq, Nk, D) in enumerate(ATTN_CASES):
        q, k, v = nb.attn_inputs(B, heads, Nq, Nk, D, amp, 100 + i, kind)
        for name, c in (("mfma", nb.consts_mfma(Nk)), ("small", nb.consts_small(Nk)), ("valu", nb.consts_kvlds_valu(Nk))):
            for fn in (att_torch32, att_log2, att_online):
                r = attn_ratio(fn, q, k, v, heads, D, c)
                assert r <= 1.0, (name, fn.__name__, (B, heads, Nq, Nk, D), amp, r)


@pytest.mark.parametrize("kind", ["qzero", "dominant"])
def test_attention_bounds_hold_on_the_probes(kind):
    for i, (B, heads, Nq, Nk, D) in enumerate(ATTN_CASES):
        q, k, v = nb.attn_inputs(B, heads, Nq, Nk, D, 0.0, 200 + i, kind)
        ref, E, smax = nb.attention_bound(q, k, v, heads, D, D ** -0.5, nb.consts_mfma(Nk))
        if kind == "dominant":
            s = D ** -0.5 * (nb.split_heads(q.double(), heads, D) @ nb.split_heads(k.double(), heads, D).transpose(-1, -2))
            top = s.topk(2, -1).values
            assert Nk == 1 or (top[..., 0] - top[..., 1]).min() > 100
        for fn in (att_torch32, att_log2, att_online):
            assert attn_ratio(fn, q, k, v, heads, D, nb.consts_mfma(Nk)) <= 1.0, (kind, fn.__name__, Nk)


def window_case(H, W, heads, D, ws, amp, seed):
    B, C = 2, heads * D
    q, k, v = nb.attn_inputs(B, heads, H * W, H * W, D, amp, seed)
    pads = [3.0 * torch.randn(ws * ws, C, generator=nb.gen(seed + 10 + i)) + 2.0 for i in range(3)]
    return B, q, k, v, pads


def window_slab(qw, kw, vw):
    """the kernel's 64-row slab: rows past ws ws hold token 0 (finite filler)"""
    fill = 64 - kw.shape[-2]
    return (torch.cat([t, t[..., :1, :].expand(*t.shape[:-2], fill, t.shape[-1])], -2) for t in (qw, kw, vw))


WINDOW_CASES = [(9, 10, 3, 16, 7), (7, 7, 1, 32, 7), (5, 3, 5, 16, 4), (1, 1, 4, 16, 5), (8, 16, 8, 32, 8)]


@pytest.mark.parametrize("amp", AMPS)
def test_window_bound_holds_and_the_mask_is_seen(amp):
    """the slab restatement (64 rows, keys >= ws ws masked) meets the bound; masking one key too many (the last token is lost) or one too few
    (a filler row becomes a key) does not, in every amplitude family"""
    fired = {-1: False, 1: False}
    for i, (H, W, heads, D, ws) in enumerate(WINDOW_CASES):
        B, q, k, v, (qp, kp, vp) = window_case(H, W, heads, D, ws, amp, 300 + i)
        T = ws * ws
        qw, kw, vw = (nb.to_windows(t, p, B, H, W, ws) for t, p in ((q, qp), (k, kp), (v, vp)))
        ref, E, _ = nb.attention_bound(qw, kw, vw, heads, D, D ** -0.5, nb.consts_window())
        qs, ks, vs = window_slab(*heads_of(qw, kw, vw, heads, D))
        for off in (0, -1, 1):
            if T + off > 64 or T + off < 1:
                continue
            o = nb.merge_heads(att_log2(qs, ks, vs, D ** -0.5, mask_from=T + off)[..., :T, :])
            r = nb.ratio(o, ref, E)
            if off == 0:
                assert r <= 1.0, ((H, W, heads, D, ws), amp, r)
                assert nb.ratio(nb.merge_heads(att_torch32(*heads_of(qw, kw, vw, heads, D), D ** -0.5)), ref, E) <= 1.0
            else:
                fired[off] |= r > 1.0
    assert fired[-1] and fired[1], fired


@pytest.mark.parametrize("amp", AMPS)
def test_attention_mutations_break_the_bound(amp):
    fired = dict(drop_last_key=False, max_first_chunk=False)
    for i, (B, heads, Nq, Nk, D) in enumerate(ATTN_CASES):
        if Nk == 1:
            continue
        q, k, v = nb.attn_inputs(B, heads, Nq, Nk, D, amp, 100 + i)
        fired["drop_last_key"] |= attn_ratio(att_log2, q, k, v, heads, D, nb.consts_mfma(Nk), kq=(k[:, :-1], v[:, :-1])) > 1.0
        if Nk > 8:
            fired["max_first_chunk"] |= attn_ratio(att_online, q, k, v, heads, D, nb.consts_kvlds_valu(Nk), rescale=False) > 1.0
    assert all(fired.values()), fired


def test_latent_pool_bound():
    for P in (2, 4, 30, 62, 64):
        for amp in (1.0, 3.0, 20.0):
            M = 3
            S, T = amp * torch.randn(M * P, 64, generator=nb.gen(P)), torch.randn(M * P, 128, generator=nb.gen(P + 1))
            ref, E = nb.latent_pool_bound(S, T, M, P)
            s32 = S.view(M, P, 64).transpose(1, 2)
            o = torch.softmax(s32, -1) @ T.view(M, P, 128)
            assert nb.ratio(o, ref, E) <= 1.0, (P, amp)
            p = torch.exp2((s32 - s32.amax(-1, keepdim=True)) * f32(nb.LOG2E))
            assert nb.ratio(((p / p.sum(-1, keepdim=True)) @ T.view(M, P, 128)), ref, E) <= 1.0, (P, amp)
            if P > 2:
                o = torch.softmax(s32[..., :-1], -1) @ T.view(M, P, 128)[:, :-1]                # the last token dropped
                assert nb.ratio(o, ref, E) > 1.0, (P, amp)


# ------------------------------------------------------------------------------------------------ row kernels
def ln_two_pass(x, w, b, eps, drop=0):
    """the kernels' order: mean, then the centred squares; `drop`: the mean's sum misses that many trailing elements"""
    C = x.shape[-1]
    mean = x[..., :C - drop].sum(-1, keepdim=True) / C
    d = x - mean
    return d * (1.0 / torch.sqrt((d * d).sum(-1, keepdim=True) / C + eps)) * w + b


LN_C = (1, 7, 64, 127, 128, 129, 192, 1024)


@pytest.mark.parametrize("mean", [0.0, 1e3, 1e4])
def test_layernorm_bound_and_mutation(mean):
    fired = False
    for C in LN_C:
        x, w, b = nb.ln_inputs(33, C, mean, 400 + C, const_row=5)
        for n_s in (nb.LN_NS_GENERIC,) + ((nb.LN_NS_128,) if C == 128 else ()):
            ref, E = nb.layernorm_bound(x, w, b, 1e-5, n_s)
            assert nb.ratio(torch.nn.functional.layer_norm(x, (C,), w, b, 1e-5), ref, E) <= 1.0, (C, mean, n_s)
            assert nb.ratio(ln_two_pass(x, w, b, 1e-5), ref, E) <= 1.0, (C, mean, n_s)
            fired |= nb.ratio(ln_two_pass(x, w, b, 1e-5, drop=1), ref, E) > 1.0
    assert fired


SOFTMAX_C = (1, 100, 255, 256, 257, 4095, 4096)


@pytest.mark.parametrize("amp", [1.0, 10.0, 80.0])
def test_softmax_rows_bound_and_mutation(amp):
    fired = False
    for C in SOFTMAX_C:
        x = nb.softmax_inputs(9, C, amp, 500 + C)
        ref, E = nb.softmax_rows_bound(x)
        assert nb.ratio(torch.softmax(x, -1), ref, E) <= 1.0, (C, amp)
        e = torch.exp(x - x.amax(-1, keepdim=True))
        e = torch.where(e < 2.0 ** -126, torch.zeros(()), e)                                   # flush to zero, as the GPU does
        assert nb.ratio(e / e.sum(-1, keepdim=True), ref, E) <= 1.0, (C, amp)
        fired |= nb.ratio(e / e[..., :-1].sum(-1, keepdim=True), ref, E) > 1.0                 # the sum misses the last column
    assert fired


def test_l2norm_bound():
    for C in (1, 63, 64, 65, 1024):
        x = torch.randn(40, C, generator=nb.gen(600 + C))
        x[3] = 0.0
        ref, E = nb.l2norm_bound(x)
        assert nb.ratio(torch.nn.functional.normalize(x, dim=-1), ref, E) <= 1.0, C
        assert nb.ratio(x / torch.sqrt((x * x).sum(-1, keepdim=True)).clamp_min(1e-12), ref, E) <= 1.0, C
        assert bool((ref[3] == 0).all())
        if C > 1:
            assert nb.ratio(x / torch.sqrt((x * x)[:, :-1].sum(-1, keepdim=True)).clamp_min(1e-12), ref, E) > 1.0, C


def ccl_diagonals(G, h, w):
    """the kernel's formulation in fp32: vol[p, q] = 10 sum over the 9 offsets d of G[p + d, q + d], both in bounds -> (flow_w, flow_h)"""
    P = h * w
    Gp = torch.nn.functional.pad(G.view(-1, h, w, h, w), (1, 1, 1, 1, 1, 1, 1, 1))
    vol = sum(Gp[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    p = torch.softmax(10.0 * vol.reshape(-1, P, P), -1)
    idx = torch.arange(P)
    dxs, dys = ((f(idx)[None, :] - f(idx)[:, None]).float() for f in (lambda t: t % w, lambda t: t // w))
    return torch.stack([(p * dxs).sum(-1), (p * dys).sum(-1)], -1)


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (16, 16), (8, 32), (1, 40)])
def test_ccl_bound_and_the_two_formulations(h, w):
    B, C = 2, 8
    n1, n2 = nb.ccl_inputs(B, h, w, C, 700 + h + w)
    G64 = n1.double() @ n2.double().transpose(1, 2)
    assert torch.equal(G64.float().double(), G64)                                             # exact in fp32
    ref, E = nb.ccl_bound(n1, n2, B, h, w)
    o = ccl_diagonals(G64.float(), h, w)
    assert nb.ratio(o, ref, E) <= 1.0
    if h * w > 1:
        wrong = ccl_diagonals(G64.float().transpose(1, 2).contiguous(), h, w)                   # n1 and n2 exchanged
        assert nb.ratio(wrong, ref, E) > 1.0


# ------------------------------------------------------------------------------------------------ argument guards (host only)
EINVAL = 1001
P0 = 0x7f0000000000                                   # never dereferenced: every call below must return before a launch


def ptrs(n):
    return [P0 + (i << 28) for i in range(n)]


def test_attention_small_guard():
    from stitch_amd._lib import lib

    def call(q, k, v, o, st=(1024, 128) * 4, B=2, heads=8, Nq=8, Nk=8, D=16):
        return lib.st_attention_small(q, st[0], st[1], k, st[2], st[3], v, st[4], st[5], o, st[6], st[7], B, heads, Nq, Nk, D, 0.25, None)
    q, k, v, o = ptrs(4)
    for i in range(4):                                                                        # each pointer off by one float
        a = [q, k, v, o]
        a[i] += 4
        assert call(*a) == EINVAL, i
    for i in range(8):                                                                        # each stride not a multiple of 4 floats
        st = [1024, 128] * 4
        st[i] += 2
        assert call(q, k, v, o, st=tuple(st)) == EINVAL, i
    for kw in (dict(B=0), dict(heads=0), dict(Nq=0), dict(Nk=0), dict(B=-1), dict(heads=-3), dict(D=12), dict(D=64)):
        assert call(q, k, v, o, **kw) == EINVAL, kw


def test_attention_kvlds_guard():
    from stitch_amd._lib import lib

    def call(q, k, v, o, st=(1 << 20, 128) * 4, B=2, heads=8, Nq=100, Nk=100, D=16):
        return lib.st_attention_kvlds(q, st[0], st[1], k, st[2], st[3], v, st[4], st[5], o, st[6], st[7], B, heads, Nq, Nk, D, 0.25, None)
    q, k, v, o = ptrs(4)
    for Nk in (100, 256, 300):                                                                # the VALU kernel and the MFMA kernel alike
        for i in range(4):
            a = [q, k, v, o]
            a[i] += 8
            assert call(*a, Nk=Nk) == EINVAL, (Nk, i)
        for i in range(8):
            st = [1 << 20, 128] * 4
            st[i] += 1
            assert call(q, k, v, o, st=tuple(st), Nk=Nk) == EINVAL, (Nk, i)
    for kw in (dict(B=0), dict(heads=0), dict(Nq=0), dict(Nk=0), dict(D=8), dict(D=64), dict(D=8, Nk=256),
               dict(D=16, Nk=1281), dict(D=32, Nk=641)):                                      # one key past 160 KiB of K | V
        assert call(q, k, v, o, **kw) == EINVAL, kw


def test_window_attention_guard():
    from stitch_amd._lib import lib

    def call(p, st=(1 << 20, 384, 1 << 19, 128), B=2, H=9, W=10, heads=8, D=16, ws=7):
        return lib.st_window_attention(p[0], p[1], p[2], st[0], st[1], p[3], p[4], p[5], p[6], st[2], st[3], B, H, W, heads, D, ws, 0.25, None)
    base = ptrs(7)
    for i in range(7):                                                                        # q, k, v, the three pad tables, out
        p = list(base)
        p[i] += 4
        assert call(p) == EINVAL, i
    for i in range(4):
        st = [1 << 20, 384, 1 << 19, 128]
        st[i] += 3
        assert call(base, st=tuple(st)) == EINVAL, i
    for kw in (dict(B=0), dict(H=0), dict(W=0), dict(heads=0), dict(H=-7), dict(W=-1), dict(heads=-8), dict(D=8), dict(D=64), dict(ws=0), dict(ws=9)):
        assert call(base, **kw) == EINVAL, kw


def test_row_kernel_and_ccl_guards():
    from stitch_amd._lib import lib
    a, b, c, d = ptrs(4)
    for kw in (dict(B=0), dict(h=0), dict(w=0), dict(B=-1), dict(h=-4, w=-4), dict(h=33, w=32), dict(h=1 << 16, w=1 << 16), dict(ldo=1)):
        g = dict(dict(ldo=4, B=2, h=8, w=8), **kw)
        assert lib.st_ccl_softargmax(a, b, g["ldo"], g["B"], g["h"], g["w"], None) == EINVAL, kw
    assert lib.st_layernorm(a, 1025, b, c, d, 1025, 4, 1025, 1e-5, None) == EINVAL            # C beyond 16 columns per lane
    assert lib.st_layernorm(a, 0, b, c, d, 0, 4, 0, 1e-5, None) == EINVAL
    assert lib.st_softmax_rows(a, 4097, 4, 4097, None) == EINVAL                              # C beyond 16 columns per thread
    assert lib.st_softmax_rows(a, 0, 4, 0, None) == EINVAL
    assert lib.st_l2norm_rows(a, b, 0, 64, None) == EINVAL and lib.st_l2norm_rows(a, b, 4, 0, None) == EINVAL
    for P, ld_s, ld_t in ((3, 64, 128), (63, 64, 128), (66, 64, 128), (0, 64, 128), (8, 63, 128), (8, 64, 127)):
        assert lib.st_latent_pool(a, ld_s, b, ld_t, c, 4, P, None) == EINVAL, (P, ld_s, ld_t)
