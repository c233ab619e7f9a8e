"""The attention and row-reduction kernels of csrc/nn.hip over their dispatch paths, the strided layouts the product calls them with, their
edges and the numerics the first-generation tests in test_ops_gpu.py never reach (large logits, one dominant key, equal keys, Nk = 1,
|mean| >> std, underflowing softmax terms).  The references and the bounds are those of tests/_nn_bounds.py; tests/test_nn_bounds_cpu.py
shows on the CPU that fp32 meets them and that planted defects do not.

Three bars per case, none taken from a GPU measurement:

(a) elementwise: |out - ref| <= E, ref the fp64 statement of the operation, E the first-order worst-case bound derived in _nn_bounds.py from
    the roundings the kernel that the case lands on performs; recorded as max err / E through _measure.check.
(b) the control rule of tests/test_stage_fp64_gpu.py: with e_rms(X) = |X - ref|_2 / |ref|_2, e_max(X) = max|X - ref| / max|ref| and o32 =
    torch's CPU fp32 on the same inputs in the same run,  e_rms(HIP) <= 2 max(e_rms(o32), 2^-24)  and  e_max(HIP) <= 4 max(e_max(o32), 2^-24).
    Both ratios are recorded for every case.  They are not asserted -- bar (a) stands alone -- where the rule compares unlike things, each
    such case carrying its reason (CONTROL_OFF and the two rules next to it): fewer than MIN_ROWS independent softmax rows, a constant
    LayerNorm row, the generic LayerNorm kernel at |mean| >> std, and two attention cases listed by name.
(c) bit identities inside one kernel path: a query's output row does not depend on the other queries (a prefix run cut mid-tile gives the
    same bits; the first 1000 rows of an Nq = 8232 run, four tiles per wave, equal an Nq = 1000 run, two per wave); every strided layout
    flowformer.py uses gives the bits of the contiguous one; a B x heads launch equals the per-(b, h) launches; a window's output depends
    on its own tokens and pad rows only; the row kernels do not care about the order of the rows or about ld.

Every operand sits at an offset inside a NaN-filled buffer: an output buffer must be NaN outside the view afterwards, and a read outside an
input view would put a NaN into the result.  The attention entries do not report which kernel ran: `kvlds_path` restates the dispatcher of
st_attention_kvlds and `layernorm_path` that of st_layernorm, each case table names the path it is meant for, and every case asserts that
the predicate agrees -- a bit identity that held across a pair meant to straddle two paths would say the predicate is out of date."""
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import _nn_bounds as nb  # noqa: E402
from _measure import check  # noqa: E402
from test_split3_matrix_gpu import nan_wide, untouched  # noqa: E402

NAN = float("nan")
FLOOR = 2.0 ** -24
MARGIN = 8                                                        # floats of NaN in front of and behind every placed operand
AMPS = (5.0, 20.0, 60.0)


def cyc(seq, i):
    return seq[i % len(seq)]


# ================================================================================================ case tables
# ---- st_attention_kvlds: (path, D, Nk, Nq, heads, B, amp, layout)
def kvlds_path(Nq, Nk, D):
    """the dispatcher of st_attention_kvlds, restated (alignment is a precondition of both kernels, checked before)"""
    if D not in (16, 32):
        return "einval"
    if Nk % 16 == 0 and Nk <= 256:
        return "mfma_tpw4" if Nq >= 8192 else "mfma_tpw2"
    return "valu" if 2 * Nk * D * 4 <= 160 * 1024 else "einval"


def valu_nk_max(D):
    return 160 * 1024 // (2 * D * 4)                              # 1280 at D = 16, 640 at D = 32: 160 KiB of K | V


KV_LAYOUTS = ("contig", "kvhalf", "latent")
KV_MFMA_NK, KV_TPW2_NQ, KV_TPW4_NQ = (16, 48, 112, 240, 256), (1, 15, 16, 17, 1000, 8191), (8192, 8232)
KV_VALU_NK, KV_VALU_NQ = (1, 7, 8, 12, 100, 257, 300, "max"), (1, 17, 600, 1000)
KV_CASES = []                                                     # heads, B, amplitude and layout rotate with the indices of the other axes
_MFMA_NQ = [("mfma_tpw2", n) for n in KV_TPW2_NQ] + [("mfma_tpw4", n) for n in KV_TPW4_NQ]
for (_a, _D), (_b, _Nk), (_c, (_path, _Nq)) in itertools.product(enumerate((16, 32)), enumerate(KV_MFMA_NK), enumerate(_MFMA_NQ)):
    KV_CASES.append((_path, _D, _Nk, _Nq, cyc((1, 3, 8), _b + _c), cyc((1, 3), _a + _b + _c), cyc(AMPS, _a + _b + 2 * _c), cyc(KV_LAYOUTS, _a + _c)))
for (_a, _D), (_b, _Nk) in itertools.product(enumerate((16, 32)), enumerate(KV_VALU_NK)):
    KV_CASES.append(("valu", _D, valu_nk_max(_D) if _Nk == "max" else _Nk, cyc(KV_VALU_NQ, _a + _b), cyc((1, 3, 8), _a + _b), cyc((1, 3), _b),
                     cyc(AMPS, 2 * _a + _b), cyc(KV_LAYOUTS, _a + 2 * _b)))

# ---- st_attention_small: (D, Nk, Nq, B, heads, amp, layout); B heads Nq is never a multiple of 256
SMALL_CASES = []
for (_a, _D), (_b, _Nk), (_c, _Nq) in itertools.product(enumerate((8, 16, 32)), enumerate((1, 8, 64, 200)), enumerate((1, 8))):
    _B, _heads = cyc(((37, 3), (5, 8), (1, 1), (67, 5)), _a + _b + 2 * _c)
    _lay = "fused" if _Nq == _Nk else cyc(("contig", "bq", "bq_kvhalf", "kvhalf"), _a + _b + _c)
    SMALL_CASES.append((_D, _Nk, _Nq, _B, _heads, cyc(AMPS, _a + _b + _c), _lay))

# ---- st_window_attention: (D, heads, ws, grid kind, amp, layout), B = 2 (the "vertical" layout: the latent index is the batch)
WINDOW_GRIDS = dict(one_token=lambda ws: (1, 1), sub_window=lambda ws: (ws - 1, max(1, ws - 2)), one_window=lambda ws: (ws, ws),
                    multiple=lambda ws: (2 * ws, 3 * ws), ragged=lambda ws: (2 * ws + 1, 3 * ws - 2), ragged_w=lambda ws: (ws, ws + 1))
WINDOW_CASES = []                                                 # two grids per (D, heads, ws)
for (_a, _D), (_b, _heads), (_c, _ws), _j in itertools.product(enumerate((16, 32)), enumerate((1, 3, 4, 5, 8)), enumerate((4, 5, 7, 8)), (0, 1)):
    WINDOW_CASES.append((_D, _heads, _ws, cyc(tuple(WINDOW_GRIDS), _a + _b + _c + 3 * _j), cyc(AMPS, _b + _c + _j), cyc(("contig", "fused", "vertical"), _a + _c + 2 * _j)))

# ---- row kernels
LN_C, LN_ROWS, LN_MEANS = (1, 7, 64, 127, 128, 129, 192, 1024), (1, 31, 32, 33, 1000), (0.0, 1e3, 1e4)
SOFTMAX_C, SOFTMAX_AMPS = (1, 100, 255, 256, 257, 4095, 4096), (1.0, 10.0, 80.0)
L2_C = (1, 63, 64, 65, 1024)
POOL_P = (2, 4, 30, 62, 64)
CCL_HW, CCL_LDO = ((1, 1), (3, 5), (16, 16), (8, 32), (32, 32), (1, 40)), (2, 4)


def layernorm_path(C, ldx, ldo, ptrs):
    """the dispatcher of st_layernorm, restated"""
    return "ln128" if C == 128 and ldx % 4 == 0 and ldo % 4 == 0 and all(p % 16 == 0 for p in ptrs) else "generic"


def test_the_tables_cover_the_axes():
    kv = set(KV_CASES)
    for path, nqs, nks in (("mfma_tpw2", KV_TPW2_NQ, KV_MFMA_NK), ("mfma_tpw4", KV_TPW4_NQ, KV_MFMA_NK)):
        assert {(c[1], c[2], c[3]) for c in kv if c[0] == path} == set(itertools.product((16, 32), nks, nqs))
        for ax, vals in ((4, (1, 3, 8)), (5, (1, 3)), (6, AMPS), (7, KV_LAYOUTS)):
            assert {c[ax] for c in kv if c[0] == path} == set(vals), (path, ax)
    valu = [c for c in kv if c[0] == "valu"]
    assert {c[2] for c in valu} == {1, 7, 8, 12, 100, 257, 300, 640, 1280} and {c[6] for c in valu} == set(AMPS) and {c[7] for c in valu} == set(KV_LAYOUTS)
    for c in KV_CASES:
        assert kvlds_path(c[3], c[2], c[1]) == c[0], c
    assert kvlds_path(600, 1281, 16) == kvlds_path(600, 641, 32) == "einval" and kvlds_path(600, 1280, 16) == kvlds_path(600, 640, 32) == "valu"
    assert all((c[3] * c[4] * c[2]) % 256 for c in SMALL_CASES) and {c[6] for c in SMALL_CASES} == {"contig", "bq", "bq_kvhalf", "kvhalf", "fused"}
    assert {c[3] for c in WINDOW_CASES} == set(WINDOW_GRIDS) and {c[5] for c in WINDOW_CASES} == {"contig", "fused", "vertical"}
    assert {(c[0], c[1], c[2]) for c in WINDOW_CASES} == set(itertools.product((16, 32), (1, 3, 4, 5, 8), (4, 5, 7, 8)))


# ================================================================================================ plumbing
@pytest.fixture(scope="module")
def ops():
    import stitch_amd
    assert torch.cuda.is_available()
    return stitch_amd.ops


# ---- where bar (b) is not asserted.  The multiples stay 2 and 4 everywhere else.
# An attention output row carries the error of ONE softmax row (all D outputs of a (batch, head, query) share its weights), so e_rms over n such
# rows is an estimate from n draws with a relative scatter of 1 / sqrt(2 n); the rule compares two of them.  For a factor of 2 (ln 2 = 0.69) to lie
# three standard deviations out the two estimates need n >= 2 (3 / 0.69)^2 / 2 = 19 rows each even when HIP and the control err alike, and HIP may
# legitimately err up to twice as much: the rule is asserted from 64 rows on.  (The smaller cases are there for the tile edges: Nq = 1, one token.)
MIN_ROWS = 64
CONTROL_OFF = {
    "kvlds_valu_d16_nk1280_nq1000_h3_b3_a20_latent":
        "the VALU kernel adds 1280 weights and products along ONE chain per thread (1440 roundings with the rescales); torch's GEMM and softmax "
        "sum in blocks, so the control's accumulation error is that of a much shorter chain",
    "window_d32_h1_ws4_ragged_a20_contig":
        "both errors are a few u (control 2.7 u rms): 16 keys, one head.  At that level v_exp_f32's 1 ulp against torch's correctly rounded exp "
        "is the difference; the same order of operations with an accurate exp2 on the CPU is at 1.06 of the control",
}


def errs(x, ref):
    x, ref = x.double().reshape(-1), ref.reshape(-1)
    if not bool(ref.any()):                                   # an exactly zero answer: only an exact zero is right
        e = 0.0 if not bool(x.any()) else float("inf")
        return e, e
    return ((x - ref).norm() / ref.norm()).item(), ((x - ref).abs().max() / ref.abs().max()).item()


def bars(name, out, ref, E, o32, control=True, rows=None, ctl_rows=None):
    """bar (a) and bar (b); every figure is recorded before any is asserted.  Bar (b) is recorded but not asserted when `control` is off (the
    caller says why), when the case has fewer than MIN_ROWS softmax `rows`, or when CONTROL_OFF names it; `ctl_rows`: the rows bar (b) is taken over"""
    assert out.shape == ref.shape == E.shape, (out.shape, ref.shape, E.shape)
    todo = [(f"nn_{name}_err_over_E", nb.ratio(out, ref, E), 1.0, "|out - ref| <= E elementwise, fp64 reference (tests/_nn_bounds.py)")]
    control = control and name not in CONTROL_OFF and (rows is None or rows >= MIN_ROWS)
    o32 = o32.to(ref.device)
    if ctl_rows is not None:
        out, ref, o32 = out[ctl_rows], ref[ctl_rows], o32[ctl_rows]
    hr, hm = errs(out, ref)
    cr, cm = errs(o32, ref)
    note = "torch CPU fp32 on the same inputs; multiples of tests/test_stage_fp64_gpu.py bar (a)" + ("" if control else "; recorded, not asserted")
    todo += [(f"nn_{name}_rms_over_ctl", hr / max(cr, FLOOR), 2.0 if control else float("inf"), note),
             (f"nn_{name}_max_over_ctl", hm / max(cm, FLOOR), 4.0 if control else float("inf"), note)]
    failed = []
    for nm, val, bound, nt in todo:
        try:
            check(nm, val, bound, inclusive=True, note=nt)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "; ".join(failed)


def place(spec, shapes, tensors):
    """spec: operand -> (buffer, offset, batch stride, token stride) in floats; shapes: operand -> (B, N, C).  Every buffer is NaN; each operand
    of `tensors` is copied to its strided view.  -> (buffers, views)"""
    size = {}
    for name, (buf, off, bs, ts) in spec.items():
        Bn, N, C = shapes[name]
        size[buf] = max(size.get(buf, 0), MARGIN + off + (Bn - 1) * bs + (N - 1) * ts + C + MARGIN)
    bufs = {b: torch.full((n,), NAN, device="cuda") for b, n in size.items()}
    views = {name: bufs[buf].as_strided(shapes[name], (bs, ts, 1), MARGIN + off) for name, (buf, off, bs, ts) in spec.items()}
    for name, t in tensors.items():
        views[name].copy_(t)
    return bufs, views


def take_output(bufs, views, spec):
    """the output view's content; the rest of its buffer must still be NaN"""
    torch.cuda.synchronize()
    out = views["o"].clone()
    views["o"].fill_(NAN)
    assert bool(torch.isnan(bufs[spec["o"][0]]).all()), "a write outside the output view"
    return out


def attn_layout(lay, B, Nq, Nk, C):
    """the q / k / v / out addressing of an attention call: contiguous, or as flowformer.py hands the operands over"""
    sp = dict(q=("q", 0, Nq * C, C), k=("k", 0, Nk * C, C), v=("v", 0, Nk * C, C), o=("o", 0, Nq * C, C))
    if lay in ("kvhalf", "bq_kvhalf"):                        # k | v halves of one [B Nk, 2C] buffer (flowformer.py:378, 443)
        sp.update(k=("kv", 0, Nk * 2 * C, 2 * C), v=("kv", C, Nk * 2 * C, 2 * C))
    if lay in ("bq", "bq_kvhalf"):                            # one q for every batch (flowformer.py:443)
        sp.update(q=("q", 0, 0, C))
    if lay == "fused":                                        # q | k | v thirds of one [B N, 3C] buffer (flowformer.py:464)
        assert Nq == Nk
        sp.update(q=("qkv", 0, Nq * 3 * C, 3 * C), k=("qkv", C, Nq * 3 * C, 3 * C), v=("qkv", 2 * C, Nq * 3 * C, 3 * C))
    if lay == "latent":                                       # the batch is the latent index: q / out rows (token, latent), k | v rows [latent][image][Nk]
        sp.update(q=("q", 0, C, B * C), o=("o", 0, C, B * C),  # of two images, this launch taking the second (flowformer.py:550)
                  k=("kv", Nk * 2 * C, 2 * Nk * 2 * C, 2 * C), v=("kv", Nk * 2 * C + C, 2 * Nk * 2 * C, 2 * C))
    return sp


def run_attention(ops, entry, lay, q, k, v, B, heads, Nq, Nk, D):
    C = heads * D
    sp = attn_layout(lay, B, Nq, Nk, C)
    assert B == 1 or (q.shape[0] == 1) == (sp["q"][2] == 0)
    bufs, vw = place(sp, dict(q=tuple(q.shape), k=(B, Nk, C), v=(B, Nk, C), o=(B, Nq, C)), dict(q=q, k=k, v=v))
    st = lambda n: (sp[n][2], sp[n][3])                        # noqa: E731
    getattr(ops, entry)(vw["q"], st("q"), vw["k"], st("k"), vw["v"], st("v"), vw["o"], st("o"), B, heads, Nq, Nk, D, D ** -0.5)
    return take_output(bufs, vw, sp)


def att32(q, k, v, heads, D):
    """the control: torch CPU fp32"""
    qh, kh, vh = (nb.split_heads(t.cpu(), heads, D) for t in (q, k, v))
    return nb.merge_heads(torch.softmax((qh @ kh.transpose(-1, -2)) * D ** -0.5, -1) @ vh)


def attention_case(ops, entry, name, consts, lay, B, heads, Nq, Nk, D, amp, seed, kind="randn"):
    bq = lay.startswith("bq")
    q, k, v = nb.attn_inputs(B, heads, Nq, Nk, D, amp, seed, kind, bq=bq)
    out = run_attention(ops, entry, lay, q, k, v, B, heads, Nq, Nk, D)
    ref, E, smax = nb.attention_bound(q.cuda(), k.cuda(), v.cuda(), heads, D, D ** -0.5, consts)
    if kind in ("randn", "equal"):
        assert abs(smax - amp) < 1e-3 * amp, (smax, amp)
    bars(name, out, ref, E, att32(q, k, v, heads, D), rows=B * heads * Nq)
    return q, k, v, out


# ================================================================================================ st_attention_kvlds
def kv_id(c):
    return f"{c[0]}_d{c[1]}_nk{c[2]}_nq{c[3]}_h{c[4]}_b{c[5]}_a{int(c[6])}_{c[7]}"


@pytest.mark.parametrize("case", KV_CASES, ids=kv_id)
def test_kvlds_matrix(ops, case):
    path, D, Nk, Nq, heads, B, amp, lay = case
    assert kvlds_path(Nq, Nk, D) == path
    consts = nb.consts_kvlds_valu(Nk) if path == "valu" else nb.consts_mfma(Nk)
    attention_case(ops, "attention_kvlds", "kvlds_" + kv_id(case), consts, lay, B, heads, Nq, Nk, D, amp, 1000 + KV_CASES.index(case))


@pytest.mark.parametrize("D,Nk", [(16, 48), (32, 256), (16, 100), (32, 300)])
def test_kvlds_queries_are_independent(ops, D, Nk):
    """a prefix run whose Nq' ends inside a 16-query tile (MFMA) / inside a 512-query workgroup (VALU) gives the bits of the full run; on the
    MFMA path the same holds between four tiles per wave (Nq = 8232, a prefix of 8200) and two (Nq = 1000)"""
    B, heads = 2, 3
    mfma = Nk % 16 == 0
    Nq = 8232 if mfma else 1000
    q, k, v = nb.attn_inputs(B, heads, Nq, Nk, D, 20.0, 2000 + Nk)
    full = run_attention(ops, "attention_kvlds", "contig", q, k, v, B, heads, Nq, Nk, D)
    for n in ((8200, 1000, 777, 9) if mfma else (777, 300, 9)):
        assert kvlds_path(n, Nk, D) == (("mfma_tpw4" if n >= 8192 else "mfma_tpw2") if mfma else "valu")
        part = run_attention(ops, "attention_kvlds", "contig", q[:, :n].contiguous(), k, v, B, heads, n, Nk, D)
        assert torch.equal(part, full[:, :n]), (D, Nk, n, (part != full[:, :n]).sum().item())


@pytest.mark.parametrize("D,Nk,Nq", [(16, 112, 1000), (32, 240, 8232), (16, 12, 600), (32, 257, 600)])
def test_kvlds_layouts_and_launch_shapes_same_bits(ops, D, Nk, Nq):
    """every strided layout of the product gives the bits of the contiguous one, and a B x heads launch those of its per-(b, h) launches"""
    B, heads = 3, 3
    q, k, v = nb.attn_inputs(B, heads, Nq, Nk, D, 20.0, 2100 + Nk)
    base = run_attention(ops, "attention_kvlds", "contig", q, k, v, B, heads, Nq, Nk, D)
    for lay in ("kvhalf", "latent"):
        assert torch.equal(run_attention(ops, "attention_kvlds", lay, q, k, v, B, heads, Nq, Nk, D), base), lay
    for b in range(B):
        for h in range(heads):
            sl = slice(h * D, (h + 1) * D)
            one = run_attention(ops, "attention_kvlds", "contig", *(t[b:b + 1, :, sl].contiguous() for t in (q, k, v)), 1, 1, Nq, Nk, D)
            assert torch.equal(one, base[b:b + 1, :, sl]), (b, h)


PROBE_ENTRIES = [("attention_kvlds", 16, 48, 1000), ("attention_kvlds", 32, 256, 8200), ("attention_kvlds", 16, 100, 600),
                 ("attention_kvlds", 32, 300, 17), ("attention_small", 8, 64, 8), ("attention_small", 32, 200, 8)]


def probe_consts(entry, Nq, Nk, D):
    if entry == "attention_small":
        return nb.consts_small(Nk)
    return nb.consts_kvlds_valu(Nk) if kvlds_path(Nq, Nk, D) == "valu" else nb.consts_mfma(Nk)


@pytest.mark.parametrize("entry,D,Nk,Nq", PROBE_ENTRIES)
def test_exact_probes(ops, entry, D, Nk, Nq):
    """all keys equal and q = 0: the mean of V within bar (a); one key more than 100 ahead in score: that V row, bit for bit (every other weight
    underflows to an exact zero, the sum is 1)"""
    B, heads = 2, 3
    c = probe_consts(entry, Nq, Nk, D)
    for kind in ("equal", "qzero"):
        q, k, v, out = attention_case(ops, entry, f"probe_{entry}_d{D}_nk{Nk}_{kind}", c, "contig", B, heads, Nq, Nk, D, 20.0, 2200 + Nk, kind)
        mean = v.double().mean(1, keepdim=True).expand(-1, Nq, -1).cuda()
        assert (out.double() - mean).abs().max().item() < 1e-4          # the reference of these two kinds IS the mean of V
    q, k, v, out = attention_case(ops, entry, f"probe_{entry}_d{D}_nk{Nk}_dominant", c, "contig", B, heads, Nq, Nk, D, 0.0, 2300 + Nk, "dominant")
    s = D ** -0.5 * (nb.split_heads(q.double(), heads, D) @ nb.split_heads(k.double(), heads, D).transpose(-1, -2))
    top = s.topk(2, -1)
    assert (top.values[..., 0] - top.values[..., 1]).min() > 100
    want = torch.gather(nb.split_heads(v, heads, D), 2, top.indices[..., :1].expand(-1, -1, -1, D))
    assert torch.equal(out.cpu(), nb.merge_heads(want))


@pytest.mark.parametrize("entry,D", [("attention_kvlds", 16), ("attention_kvlds", 32), ("attention_small", 8), ("attention_small", 16), ("attention_small", 32)])
def test_one_key_returns_v(ops, entry, D):
    B, heads, Nq = 3, 5, 1000 if entry == "attention_kvlds" else 8
    q, k, v = nb.attn_inputs(B, heads, Nq, 1, D, 60.0, 2400 + D)
    out = run_attention(ops, entry, "contig", q, k, v, B, heads, Nq, 1, D)
    assert torch.equal(out.cpu(), v.expand(-1, Nq, -1))


# ================================================================================================ st_attention_small
def small_id(c):
    return f"d{c[0]}_nk{c[1]}_nq{c[2]}_b{c[3]}_h{c[4]}_a{int(c[5])}_{c[6]}"


@pytest.mark.parametrize("case", SMALL_CASES, ids=small_id)
def test_small_matrix(ops, case):
    D, Nk, Nq, B, heads, amp, lay = case
    assert (B * heads * Nq) % 256
    attention_case(ops, "attention_small", "small_" + small_id(case), nb.consts_small(Nk), lay, B, heads, Nq, Nk, D, amp, 3000 + SMALL_CASES.index(case))


@pytest.mark.parametrize("D", [8, 16, 32])
def test_small_layouts_and_launch_shapes_same_bits(ops, D):
    B, heads, N = 37, 3, 8                                    # 888 threads: three full workgroups and a ragged fourth
    q, k, v = nb.attn_inputs(B, heads, N, N, D, 20.0, 3100 + D)
    base = run_attention(ops, "attention_small", "contig", q, k, v, B, heads, N, N, D)
    for lay in ("kvhalf", "fused"):
        assert torch.equal(run_attention(ops, "attention_small", lay, q, k, v, B, heads, N, N, D), base), lay
    part = run_attention(ops, "attention_small", "contig", q[:, :5].contiguous(), k, v, B, heads, 5, N, D)
    assert torch.equal(part, base[:, :5])
    q1 = q[:1].contiguous()                                   # the broadcast q against its expanded copy
    bq = run_attention(ops, "attention_small", "bq", q1, k, v, B, heads, N, N, D)
    assert torch.equal(bq, run_attention(ops, "attention_small", "contig", q1.expand(B, -1, -1).contiguous(), k, v, B, heads, N, N, D))
    assert torch.equal(bq, run_attention(ops, "attention_small", "bq_kvhalf", q1, k, v, B, heads, N, N, D))
    for b in (0, 17, 36):
        for h in range(heads):
            sl = slice(h * D, (h + 1) * D)
            one = run_attention(ops, "attention_small", "contig", *(t[b:b + 1, :, sl].contiguous() for t in (q, k, v)), 1, 1, N, N, D)
            assert torch.equal(one, base[b:b + 1, :, sl]), (b, h)


# ================================================================================================ st_window_attention
def window_layout(lay, B, N, C):
    sp = dict(q=("q", 0, N * C, C), k=("k", 0, N * C, C), v=("v", 0, N * C, C), o=("o", 0, N * C, C))
    if lay == "fused":                                        # q | k | v thirds of the fused rows (flowformer.py:359)
        sp.update(q=("qkv", 0, N * 3 * C, 3 * C), k=("qkv", C, N * 3 * C, 3 * C), v=("qkv", 2 * C, N * 3 * C, 3 * C))
    if lay == "vertical":                                     # rows (pixel, latent) and the latent is the batch (flowformer.py:510)
        sp.update(q=("qkv", 0, 3 * C, B * 3 * C), k=("qkv", C, 3 * C, B * 3 * C), v=("qkv", 2 * C, 3 * C, B * 3 * C), o=("o", 0, C, B * C))
    return sp


def run_window(ops, lay, q, k, v, pads, B, H, W, heads, D, ws):
    C, N = heads * D, H * W
    sp = window_layout(lay, B, N, C)
    bufs, vw = place(sp, {n: (B, N, C) for n in "qkvo"}, dict(q=q, k=k, v=v))
    assert sp["q"][2:] == sp["k"][2:] == sp["v"][2:]
    pw = [nan_wide(ws * ws + 2, C, off=0, pad=0)[0] for _ in range(3)]       # pad tables as row slices of NaN buffers (their stride is heads D by contract)
    for t, p in zip(pw, pads):
        t[1:-1] = p.cuda()
    ops.window_attention(vw["q"], vw["k"], vw["v"], sp["q"][2], sp["q"][3], pw[0][1:-1], pw[1][1:-1], pw[2][1:-1], vw["o"], sp["o"][2], sp["o"][3],
                         B, H, W, heads, D, ws, D ** -0.5)
    return take_output(bufs, vw, sp)


def window_inputs(B, H, W, heads, D, ws, amp, seed):
    """pad tables unlike the data: offset by 2 and three times as wide"""
    q, k, v = nb.attn_inputs(B, heads, H * W, H * W, D, amp, seed)
    pads = [3.0 * torch.randn(ws * ws, heads * D, generator=nb.gen(seed + 10 + i)) + 2.0 for i in range(3)]
    return q, k, v, pads


def window32(q, k, v, pads, B, H, W, heads, D, ws):
    qw, kw, vw = (nb.to_windows(t, p, B, H, W, ws) for t, p in zip((q, k, v), pads))
    return nb.from_windows(att32(qw, kw, vw, heads, D), B, H, W, ws)


def window_id(c):
    return f"d{c[0]}_h{c[1]}_ws{c[2]}_{c[3]}_a{int(c[4])}_{c[5]}"


@pytest.mark.parametrize("case", WINDOW_CASES, ids=window_id)
def test_window_matrix(ops, case):
    D, heads, ws, grid, amp, lay = case
    B, (H, W) = 2, WINDOW_GRIDS[grid](ws)
    q, k, v, pads = window_inputs(B, H, W, heads, D, ws, amp, 4000 + WINDOW_CASES.index(case))
    out = run_window(ops, lay, q, k, v, pads, B, H, W, heads, D, ws)
    ref, E = nb.window_attention_bound(q.cuda(), k.cuda(), v.cuda(), *(p.cuda() for p in pads), B, H, W, heads, D, ws, D ** -0.5)
    bars("window_" + window_id(case), out, ref, E, window32(q, k, v, pads, B, H, W, heads, D, ws), rows=B * heads * H * W)


@pytest.mark.parametrize("D,heads", [(16, 8), (32, 5)])
def test_window_depends_on_its_own_tokens_only(ops, D, heads):
    """a 14 x 21 grid of 2 x 3 windows: every layout and the per-batch launches give the same bits; the content of window (1, 2) run as a one-window
    7 x 7 grid, and moved to window (0, 0) of a grid whose other tokens are different, gives that window's bits; a ragged window (grid cut to
    12 x 19, pad rows in use) likewise against its own one-window run on a 5 x 5 grid"""
    B, ws, H, W = 2, 7, 14, 21
    C = heads * D
    q, k, v, pads = window_inputs(B, H, W, heads, D, ws, 20.0, 4200 + D)
    base = run_window(ops, "contig", q, k, v, pads, B, H, W, heads, D, ws)
    for lay in ("fused", "vertical"):
        assert torch.equal(run_window(ops, lay, q, k, v, pads, B, H, W, heads, D, ws), base), lay
    for b in range(B):
        assert torch.equal(run_window(ops, "contig", q[b:b + 1], k[b:b + 1], v[b:b + 1], pads, 1, H, W, heads, D, ws), base[b:b + 1])
    g = lambda t: t.view(B, H, W, C)                           # noqa: E731
    win = lambda t: g(t)[:, 7:14, 14:21].reshape(B, 49, C).contiguous()      # noqa: E731
    one = run_window(ops, "contig", win(q), win(k), win(v), pads, B, 7, 7, heads, D, ws)
    assert torch.equal(one, win(base))
    q2, k2, v2, _ = window_inputs(B, H, W, heads, D, ws, 20.0, 4300 + D)
    for t2, t in ((q2, q), (k2, k), (v2, v)):
        g(t2)[:, 0:7, 0:7] = g(t)[:, 7:14, 14:21]
    moved = run_window(ops, "contig", q2, k2, v2, pads, B, H, W, heads, D, ws)
    assert torch.equal(g(moved)[:, 0:7, 0:7].reshape(B, 49, C), win(base))
    Hc, Wc = 12, 19                                           # the bottom-right window keeps 5 x 5 tokens
    cut = lambda t: g(t)[:, :Hc, :Wc].reshape(B, Hc * Wc, C).contiguous()    # noqa: E731
    rag = run_window(ops, "contig", cut(q), cut(k), cut(v), pads, B, Hc, Wc, heads, D, ws)
    corner = lambda t: g(t)[:, 7:12, 14:19].reshape(B, 25, C).contiguous()   # noqa: E731
    one = run_window(ops, "contig", corner(q), corner(k), corner(v), pads, B, 5, 5, heads, D, ws)
    assert torch.equal(one, rag.view(B, Hc, Wc, C)[:, 7:12, 14:19].reshape(B, 25, C))


def test_window_of_one_token_returns_v(ops):
    """ws = 1: every token is its own window and its own only key"""
    B, H, W, heads, D = 2, 5, 9, 5, 16
    q, k, v, pads = window_inputs(B, H, W, heads, D, 1, 60.0, 4400)
    assert torch.equal(run_window(ops, "fused", q, k, v, pads, B, H, W, heads, D, 1).cpu(), v)


# ================================================================================================ row kernels
def placed_rows(x, ld_extra, off=1):
    """x [rows, C] as a column slice at column `off` of a NaN buffer with ld = C + off + ld_extra"""
    wide, view = nan_wide(x.shape[0], x.shape[1], off=off, pad=ld_extra)
    view.copy_(x)
    return wide, view


def ln_run(ops, x, w, b, eps, off, pad, want_path):
    """LayerNorm into a NaN-framed slice; x, out at column `off` of buffers with ld = C + off + pad"""
    rows, C = x.shape
    _, xv = placed_rows(x, pad, off)
    wide, out = nan_wide(rows, C, off=off, pad=pad)
    wd, bd = w.cuda(), b.cuda()
    assert layernorm_path(C, xv.stride(0), out.stride(0), [t.data_ptr() for t in (xv, out, wd, bd)]) == want_path
    ops.layernorm(xv, wd, bd, out, eps)
    torch.cuda.synchronize()
    assert untouched(wide, off, C)
    return out.clone()


@pytest.mark.parametrize("C", LN_C)
@pytest.mark.parametrize("mean", LN_MEANS)
def test_layernorm_matrix(ops, C, mean):
    """every C at every row count; C = 128 on the fast path (off = 4, ld = 136) and, forced by an offset view (off = 1) and by ld (off = 4,
    ld = 133), on the generic one.  Row 0 is constant where there is more than one row.
    Bar (b) leaves the constant row out: the right answer is b, torch's mean of equal numbers is exact and so is layernorm128_kernel's (its
    pairwise sums only double), while the 16-term per-lane chain of layernorm_kernel is off by a few u |x|, which r = eps^-1/2 = 316 multiplies --
    inside bar (a), whose dmu term is this very error.  And it is not asserted for layernorm_kernel at mean 1e3 and 1e4: torch's LayerNorm takes
    its moments by Welford updates over chunks, a different algorithm whose mean is far closer than a plain 22-deep fp32 sum when |mean| >> std;
    there the kernel is held to bar (a) alone.  The product's LayerNorm inputs have |mean| of the order of std."""
    eps = 1e-5
    for i, rows in enumerate(LN_ROWS):
        x, w, b = nb.ln_inputs(rows, C, mean, 5000 + 10 * C + i, const_row=0 if rows > 1 else None)
        variants = [("ln128", 4, 4), ("generic", 1, 2), ("generic", 4, 1)] if C == 128 else [("generic", 1, 2)]
        for path, off, pad in variants:
            out = ln_run(ops, x, w, b, eps, off, pad, path)
            ref, E = nb.layernorm_bound(x.cuda(), w.cuda(), b.cuda(), eps, nb.LN_NS_128 if path == "ln128" else nb.LN_NS_GENERIC)
            bars(f"layernorm_{path}_c{C}_r{rows}_m{int(mean)}_off{off}", out, ref, E, F.layer_norm(x, (C,), w, b, eps),
                 control=path == "ln128" or mean == 0.0, ctl_rows=slice(1, None) if rows > 1 else None)


@pytest.mark.parametrize("C,path,off,pad", [(128, "ln128", 4, 4), (128, "generic", 1, 2), (129, "generic", 1, 2), (1024, "generic", 4, 4)])
def test_layernorm_row_order_and_ld(ops, C, path, off, pad):
    rows = 1000
    x, w, b = nb.ln_inputs(rows, C, 1e3, 5900 + C)
    base = ln_run(ops, x, w, b, 1e-5, off, pad, path)
    perm = torch.randperm(rows, generator=nb.gen(1))
    assert torch.equal(ln_run(ops, x[perm], w, b, 1e-5, off, pad, path), base[perm.cuda()])
    assert torch.equal(ln_run(ops, x, w, b, 1e-5, off, pad + 8, path), base)
    assert torch.equal(ln_run(ops, x[:33], w, b, 1e-5, off, pad, path), base[:33])


@pytest.mark.parametrize("C", SOFTMAX_C)
@pytest.mark.parametrize("amp", SOFTMAX_AMPS)
def test_softmax_rows_matrix(ops, C, amp):
    """in place on a column slice (ld = C + 4); at amplitude 80 most terms of a row underflow"""
    for rows in (1, 7, 300):
        x = nb.softmax_inputs(rows, C, amp, 6000 + C + rows)
        wide, view = placed_rows(x, 3)
        ops.softmax_rows(view)
        torch.cuda.synchronize()
        assert untouched(wide, 1, C)
        ref, E = nb.softmax_rows_bound(x.cuda())
        bars(f"softmax_c{C}_r{rows}_a{int(amp)}", view, ref, E, torch.softmax(x, -1))
        if rows == 300:
            perm = torch.randperm(rows, generator=nb.gen(2))
            wide2, view2 = placed_rows(x[perm], 11)
            ops.softmax_rows(view2)
            assert torch.equal(view2, view[perm.cuda()]) and untouched(wide2, 1, C)


@pytest.mark.parametrize("C", L2_C)
def test_l2norm_rows_matrix(ops, C):
    """dense rows by contract (the entry takes no ld): the output is a row slice of a NaN buffer; row 3 is zero"""
    for rows in (5, 1000):
        x = torch.randn(rows, C, generator=nb.gen(6500 + C + rows))
        x[3] = 0.0
        wide = torch.full((rows + 2, C), NAN, device="cuda")
        ops.l2norm_rows(x.cuda(), wide[1:-1])
        torch.cuda.synchronize()
        assert bool(torch.isnan(wide[0]).all() and torch.isnan(wide[-1]).all())
        ref, E = nb.l2norm_bound(x.cuda())
        bars(f"l2norm_c{C}_r{rows}", wide[1:-1], ref, E, F.normalize(x, dim=-1))
        assert bool((wide[4] == 0).all())
        if rows == 1000:
            perm = torch.randperm(rows, generator=nb.gen(3))
            o2 = torch.empty(rows, C, device="cuda")
            ops.l2norm_rows(x[perm].cuda(), o2)
            assert torch.equal(o2, wide[1:-1][perm.cuda()])


@pytest.mark.parametrize("P", POOL_P)
@pytest.mark.parametrize("amp", [1.0, 3.0, 20.0])
def test_latent_pool_matrix(ops, P, amp):
    """scores a column slice with ld_s = 72, tokens one with ld_t = 140, z a row slice of a NaN buffer; the pixels' outputs do not depend on
    one another (a run on the pixels in another order gives the same bits)"""
    M = 37
    S, T = amp * torch.randn(M * P, 64, generator=nb.gen(7000 + P)), torch.randn(M * P, 128, generator=nb.gen(7001 + P))

    def run(order):
        rows = (order[:, None] * P + torch.arange(P)[None, :]).reshape(-1)
        _, sv = placed_rows(S[rows], 4, off=4)
        _, tv = placed_rows(T[rows], 8, off=4)
        z = torch.full((M * 64 + 2, 128), NAN, device="cuda")
        ops.latent_pool(sv, tv, z[1:-1], M, P)
        torch.cuda.synchronize()
        assert bool(torch.isnan(z[0]).all() and torch.isnan(z[-1]).all())
        return z[1:-1].view(M, 64, 128).clone()
    out = run(torch.arange(M))
    ref, E = nb.latent_pool_bound(S.cuda(), T.cuda(), M, P)
    o32 = torch.softmax(S.view(M, P, 64).transpose(1, 2), -1) @ T.view(M, P, 128)
    bars(f"latent_pool_p{P}_a{int(amp)}", out, ref, E, o32)
    perm = torch.randperm(M, generator=nb.gen(4))
    assert torch.equal(run(perm), out[perm.cuda()])


@pytest.mark.parametrize("h,w", CCL_HW)
@pytest.mark.parametrize("ldo", CCL_LDO)
def test_ccl_softargmax_matrix(ops, h, w, ldo):
    """the kernel takes G = n1 . n2^T and sums its diagonals; the reference takes n1 and n2 and runs the 3x3 patches of n2 as filters over n1.
    The features sit on a grid that makes G exact in fp32, so both see the same numbers.  Columns 2.. of the output are zero by contract."""
    B, C, P = 2, 8, h * w
    n1, n2 = nb.ccl_inputs(B, h, w, C, 8000 + 40 * h + w)
    G64 = n1.double().cuda() @ n2.double().cuda().transpose(1, 2)
    G = G64.float()
    assert torch.equal(G.double(), G64)
    wide = torch.full((B * P + 2, ldo), NAN, device="cuda")
    ops.ccl_softargmax(G.contiguous(), wide[1:-1], B, h, w)
    torch.cuda.synchronize()
    assert bool(torch.isnan(wide[0]).all() and torch.isnan(wide[-1]).all())
    assert bool((wide[1:-1, 2:] == 0).all())
    ref, E = nb.ccl_bound(n1.cuda(), n2.cuda(), B, h, w)
    bars(f"ccl_{h}x{w}_ldo{ldo}", wide[1:-1, :2].reshape(B, P, 2), ref, E, nb.ccl_forward(n1, n2, B, h, w, torch.float32))


# ================================================================================================ rejected arguments (no launch)
def test_rejections_on_device_tensors(ops):
    """what the kernels cannot take comes back as an error from the host, on real device tensors too: an unsupported D, K | V beyond 160 KiB
    of LDS, C beyond the row kernels' registers, an odd P.  (Misaligned and mis-strided operands: tests/test_nn_bounds_cpu.py, where no GPU
    is needed; such a call is never launched to see what happens.)"""
    z = torch.zeros(1 << 21, device="cuda")
    Err = ops.StitchErrorBase
    for D in (8, 12, 64):
        with pytest.raises(Err):
            ops.attention_kvlds(z, (1024, 128), z, (1024, 128), z, (1024, 128), z, (1024, 128), 2, 2, 8, 8, D, 0.25)
    for D in (4, 12, 64):
        with pytest.raises(Err):
            ops.attention_small(z, (1024, 128), z, (1024, 128), z, (1024, 128), z, (1024, 128), 2, 2, 8, 8, D, 0.25)
        with pytest.raises(Err):
            ops.window_attention(z, z, z, 4096, 128, z, z, z, z, 4096, 128, 1, 4, 4, 2, D, 4, 0.25)
    for D in (16, 32):
        with pytest.raises(Err):
            ops.attention_kvlds(z, (0, D), z, (0, D), z, (0, D), z, (0, D), 1, 1, 8, valu_nk_max(D) + 1, D, 0.25)
    with pytest.raises(Err):
        ops.window_attention(z, z, z, 4096, 128, z, z, z, z, 4096, 128, 1, 4, 4, 2, 16, 9, 0.25)
    with pytest.raises(Err):
        ops.layernorm(z[:4 * 1025].view(4, 1025), z, z, z[8192:8192 + 4 * 1025].view(4, 1025), 1e-5)
    with pytest.raises(Err):
        ops.softmax_rows(z[:4 * 4097].view(4, 4097))
    for P in (3, 66):
        with pytest.raises(Err):
            ops.latent_pool(z[:4 * P * 64].view(4 * P, 64), z[:4 * P * 128].view(4 * P, 128), z[1 << 20:(1 << 20) + 4 * 64 * 128].view(256, 128), 4, P)
    with pytest.raises(Err):
        ops.ccl_softargmax(z, z[:4096].view(1024, 4), 1, 33, 32)
    torch.cuda.synchronize()
