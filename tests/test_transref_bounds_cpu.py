"""The bounds and references of tests/_transref_bounds.py, shown on the CPU to be neither wrong nor vacuous, the coverage of the case tables
and the argument guards of csrc/transref.hip.

1. A bound that fp32 itself breaks is wrong: every bound is held against fp32 evaluations of the same operation on every case of the tables
   the GPU file runs -- torch's own fp32 and a restatement in the kernel's order (attention: the 32-key tile walk with the running maximum,
   alpha and one partial sum per register, folded pairwise; the deform sampler in fp32 on the fp32 coordinate sums).
2. A bound that a real defect meets is vacuous: nine planted errors, in the models, never in the kernels, each of which must give
   err / E > 1 (a mismatch, where the step is bit-exact) on at least one case of the tables.
3. The claims the GPU file leans on: 1 - byte on torch, fl(fl(1 - l) + l) = 1, the erf figure, the stability of the reference's hole set.
4. st_tr_attention and st_tr_blend reject what their kernels cannot take before any launch: host code only, no pointer is dereferenced."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _transref_bounds as tb
from _nn_bounds import ratio

NEG = float("-inf")
SLOT_HALF = (torch.arange(32) >> 2) & 1                                # the lane half that holds key slot (r & 3) + 8 (r >> 2) + 4 hf
SLOT_OF = [[(r & 3) + 8 * (r >> 2) + 4 * hf for r in range(16)] for hf in (0, 1)]


# ------------------------------------------------------------------------------------------------ attention: the kernel's walk in fp32
def att_head(q, k, v, scale, defect=None):
    """one head, fp32: 32 keys at a time; `m` and `alpha` per lane half (equal unless the exchange is dropped); lp per key slot = per
    (half, register); o[d] lives in half (d >> 2) & 1.  defects: lp_not_rescaled, mask_last (the last valid key scores -inf),
    clamped_weight (a key row past Nk keeps the clamped row's score), no_exchange (the running maximum of each lane half on its own)"""
    Nq, D = q.shape
    Nk = k.shape[0]
    d_half = (torch.arange(D) >> 2) & 1
    sc = torch.tensor(scale, dtype=torch.float32)
    o, lp, m = torch.zeros(Nq, D), torch.zeros(Nq, 32), torch.full((Nq, 2), NEG)
    for k0 in range(0, Nk, 32):
        key = k0 + torch.arange(32)
        rows = key.clamp(max=Nk - 1)
        s = (q @ k[rows].t()) * sc
        if defect != "clamped_weight":
            s = torch.where(key < (Nk - 1 if defect == "mask_last" else Nk), s, torch.full_like(s, NEG))
        mx = torch.stack([s[:, SLOT_HALF == h].amax(-1) for h in (0, 1)], -1)
        if defect != "no_exchange":
            mx = mx.amax(-1, keepdim=True).expand(-1, 2)
        mn = torch.maximum(m, mx)
        alpha = torch.exp(m - mn)
        m = mn
        p = torch.exp(s - mn[:, SLOT_HALF])
        lp = (lp if defect == "lp_not_rescaled" else lp * alpha[:, SLOT_HALF]) + p
        o = o * alpha[:, d_half] + p @ v[rows]
    halves = []
    for hf in (0, 1):
        regs = lp[:, SLOT_OF[hf]]
        for w in (8, 4, 2, 1):
            regs = regs[:, :w] + regs[:, w:2 * w]
        halves.append(regs)
    return o / (halves[0] + halves[1])


def att_tiles(q, k, v, heads, D, scale, defect=None):
    return torch.cat([att_head(*(t[:, h * D:(h + 1) * D] for t in (q, k, v)), scale, defect) for h in range(heads)], 1)


ATT_DEFECTS = ("lp_not_rescaled", "mask_last", "clamped_weight", "no_exchange")


def test_attention_bound_holds_for_fp32_and_the_defects_break_it():
    fired = dict.fromkeys(ATT_DEFECTS, False)
    for i, (D, Nk, Nq, heads, amp, kind, _lay) in enumerate(tb.ATT_CASES):
        q, k, v = tb.att_inputs(heads, Nq, Nk, D, amp, kind, 1000 + i)
        scale = D ** -0.5
        ref, E, smax = tb.att_bound(q, k, v, heads, D, scale)
        if kind in ("randn", "equal"):
            assert abs(smax - amp) < 1e-3 * amp
        for name, o in (("torch32", tb.att32(q, k, v, heads, D, scale)), ("tiles", att_tiles(q, k, v, heads, D, scale))):
            assert ratio(o, ref, E) <= 1.0, (name, tb.att_id(tb.ATT_CASES[i]), ratio(o, ref, E))
        for d in ATT_DEFECTS:
            fired[d] |= ratio(att_tiles(q, k, v, heads, D, scale, d), ref, E) > 1.0
    assert all(fired.values()), fired


def test_attention_probes():
    """the dominant key's V row comes back bit for bit and equal keys give the mean of V, in the kernel's order too"""
    for D, Nk in ((32, 33), (80, 100), (256, 65)):
        q, k, v = tb.att_inputs(2, 40, Nk, D, 0.0, "dominant", 7 + D)
        s = D ** -0.5 * (q.double().view(40, 2, D).transpose(0, 1) @ k.double().view(Nk, 2, D).permute(1, 2, 0))
        top = s.topk(2, -1)
        assert (top.values[..., 0] - top.values[..., 1]).min() > 100
        want = torch.cat([v[:, h * D:(h + 1) * D][top.indices[h, :, 0]] for h in range(2)], 1)
        assert torch.equal(att_tiles(q, k, v, 2, D, D ** -0.5), want)
        q, k, v = tb.att_inputs(2, 40, Nk, D, 20.0, "equal", 9 + D)
        assert (att_tiles(q, k, v, 2, D, D ** -0.5).double() - v.double().mean(0, keepdim=True)).abs().max() < 1e-4


def test_the_attention_table_covers_the_axes():
    cases = tb.ATT_CASES
    assert len(set(cases)) == len(cases) == 48
    assert {(c[0], c[1]) for c in cases} == {(D, Nk) for D in tb.ATT_D for Nk in tb.ATT_NK}
    assert {(c[0], c[2]) for c in cases} == {(D, Nq) for D in tb.ATT_D for Nq in tb.ATT_NQ}
    for ax, vals in ((3, tb.ATT_HEADS), (4, tb.AMPS), (5, tb.ATT_KINDS), (6, tb.ATT_LAYOUTS)):
        assert {c[ax] for c in cases} == set(vals), ax
        for D in tb.ATT_D:
            assert len({c[ax] for c in cases if c[0] == D}) >= min(3, len(vals)), (D, ax)
    for kind in ("rise", "fall"):                                        # the staircases meet more than one key tile at D % 32 == 0 and != 0
        assert {c[0] % 32 == 0 for c in cases if c[5] == kind and c[1] > 32} == {True, False}, kind
    assert {c[6] for c in cases if c[0] in (80, 160)} == set(tb.ATT_LAYOUTS)
    assert tb.consts_tr_attention(100) == tb.Consts(1, 4, 10, 132, 13)


# ------------------------------------------------------------------------------------------------ deform im2col
def deform_model(x, off, H, W, clamp_corner=False):
    """the kernel's arithmetic in fp32 on the fp32 coordinate sums; clamp_corner: a corner outside the image is read at the clamped index"""
    C = x.shape[1]
    h, w = tb.deform_coords(off, H, W)
    inside = (h > -1) & (w > -1) & (h < H) & (w < W)
    hl, wl = torch.floor(h), torch.floor(w)
    lh, lw = h - hl, w - wl
    hh, hw = 1 - lh, 1 - lw
    xg = x.reshape(H, W, C)
    val = None
    for dy, dx, wgt in ((0, 0, hh * hw), (0, 1, hh * lw), (1, 0, lh * hw), (1, 1, lh * lw)):
        yy, xx = (hl + dy).long(), (wl + dx).long()
        ok = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        v = xg[yy.clamp(0, H - 1), xx.clamp(0, W - 1)] * (ok | clamp_corner)[..., None]
        val = wgt[..., None] * v if val is None else val + wgt[..., None] * v
    return (val * inside[..., None]).reshape(H * W, 9 * C)


def deform_cases():
    for i, (H, W, C) in enumerate(tb.DEFORM_HWC):
        x = torch.randn(H * W, C, generator=tb.gen(300 + i)) + 0.5
        for fam in tb.DEFORM_FAMILIES:
            for shift in range(tb.EDGE_SHIFTS if fam.startswith("edge") else 1):
                yield (H, W, C), fam, shift, x, tb.deform_offsets(H, W, fam, 310 + i, shift)


def test_deform_bound_families_and_the_clamped_corner():
    fired = False
    hit_h, hit_w = {}, {}
    for (H, W, C), fam, shift, x, off in deform_cases():
        ref, E = tb.deform_bound(x, off, H, W)
        for name, o in (("ref32", tb.deform_cols(x, off, H, W, torch.float32)), ("model", deform_model(x, off, H, W))):
            assert ratio(o, ref, E) <= 1.0, (name, (H, W, C), fam, shift, ratio(o, ref, E))
        fired |= ratio(deform_model(x, off, H, W, clamp_corner=True), ref, E) > 1.0
        if fam == "zero":
            assert torch.equal(deform_model(x, off, H, W), tb.im2col_zero_padded(x, H, W)) and torch.equal(ref.float(), tb.im2col_zero_padded(x, H, W))
        if fam == "integer":
            assert torch.equal(deform_model(x, off, H, W).double(), ref)
        if fam == "far":
            h, w = tb.deform_coords(off, H, W)
            assert bool((h.abs() > 2.0 ** 31).any() and (w.abs() > 2.0 ** 31).any())
        h, w = tb.deform_coords(off, H, W)
        if fam == "edge_h":
            hit_h.setdefault((H, W, C), set()).update(h.reshape(-1).tolist())
        if fam == "edge_w":
            hit_w.setdefault((H, W, C), set()).update(w.reshape(-1).tolist())
    assert fired
    for (H, W, C) in tb.DEFORM_HWC:                                      # every edge value and both float neighbours are sampled, exactly
        assert set(tb.edge_targets(H).tolist()) <= hit_h[(H, W, C)], (H, W, C)
        assert set(tb.edge_targets(W).tolist()) <= hit_w[(H, W, C)], (H, W, C)


# ------------------------------------------------------------------------------------------------ phase interleave, dwconv + GELU
def test_phase_interleave_statement_and_the_transposed_phase():
    """the indexing statement equals F.conv_transpose2d's own placement (a 1x1-tap check: each phase weight alone), and transposing the
    phase index does not"""
    fired = False
    for i, (H, W, C) in enumerate(tb.PHASE_HWC):
        ph = torch.randn(4, H * W, C, generator=tb.gen(400 + i))
        out = tb.phase_interleave(ph, H, W).reshape(2 * H, 2 * W, C)
        for py in (0, 1):
            for px in (0, 1):
                w = torch.zeros(1, 1, 2, 2)
                w[0, 0, py, px] = 1.0
                up = F.conv_transpose2d(ph[2 * py + px].t().reshape(C, 1, H, W), w, stride=2)      # places the plane at (2a + py, 2b + px)
                assert torch.equal(up[:, 0, py::2, px::2], out[py::2, px::2].permute(2, 0, 1))
        res = torch.randn(4 * H * W, C, generator=tb.gen(450 + i))
        assert torch.equal(tb.phase_interleave(ph, H, W, res), out.reshape(-1, C) + res)
        fired |= not torch.equal(tb.phase_interleave(ph, H, W, transposed=True), out.reshape(-1, C))
    assert fired


def dw_model(x, w, b, H, W, tanh_form=False):
    """the kernel's arithmetic in fp32: 0.5 v (1 + erf(v 2^-1/2)) on torch's erf (F.gelu's vectorised CPU form is not this expression and errs
    by several u in the negative tail); tanh_form: the planted defect, GELU's tanh approximation"""
    v = tb.dw_conv(x, w, b, H, W, torch.float32)[0].permute(1, 2, 0).reshape(H * W, -1)
    if tanh_form:
        return 0.5 * v * (1.0 + torch.tanh(0.7978845608028654 * (v + 0.044715 * v * v * v)))
    return 0.5 * v * (1.0 + torch.erf(v * torch.tensor(0.70710678118654752440)))


def test_dwconv_gelu_bound_and_the_tanh_form():
    fired = False
    tails = [False, False]
    for i, (H, W, C) in enumerate(tb.DW_HWC):
        for j, amp in enumerate(tb.DW_AMPS):
            x, w, b = tb.dw_inputs(H, W, C, amp, 500 + 10 * i + j)
            ref, E = tb.dw_bound(x, w, b, H, W)
            assert ratio(dw_model(x, w, b, H, W), ref, E) <= 1.0, ((H, W, C), amp, ratio(dw_model(x, w, b, H, W), ref, E))
            assert (ref - tb.dw_gelu(x, w, b, H, W)).abs().max() < 1e-13                       # the bound's reference is nn.GELU() in fp64
            fired |= ratio(dw_model(x, w, b, H, W, tanh_form=True), ref, E) > 1.0
            v = tb.dw_conv(x, w, b, H, W, torch.float64)
            tails[0] |= bool((v < -5).any())
            tails[1] |= bool((v > 5).any())
    assert fired and all(tails)


def test_erf_figure():
    """torch-CPU fp32 erf against fp64 on [-6, 6]: at most ERF_ULPS ulp (the figure of the dwconv bound; see _transref_bounds.py)"""
    x = torch.linspace(-6, 6, 1_000_001)
    e64 = torch.erf(x.double())
    ulp = torch.from_numpy(np.spacing(np.abs(e64.float().numpy()))).double()
    assert ((torch.erf(x).double() - e64).abs() / ulp).max().item() <= tb.ERF_ULPS


# ------------------------------------------------------------------------------------------------ wrapper steps
def test_prep_values_and_the_rounding_defect():
    vals = tb.prep_values()
    assert vals.numel() == 770 and vals[-2] == torch.tensor(-0.9) and vals[-1] == torch.tensor(255.99)
    assert torch.equal(tb.prep_ref(vals[:768].reshape(256, 3)), tb.prep_ref(torch.arange(256.0))[:, None].expand(-1, 3))     # truncation
    assert tb.prep_ref(vals[-2:]).tolist() == [-1.0, 1.0]
    for hw in (1, 770):
        img, ctl = tb.prep_inputs(hw, 3)
        assert img.shape == ctl.shape == (3, hw)
        assert not torch.equal(tb.prep_ref(img, rounding=True), tb.prep_ref(img)) or hw == 1
    assert 770 % 256 and set(tb.prep_inputs(770, 3)[0].reshape(-1).tolist()) == set(vals.tolist())


def test_to_u8_inputs_and_the_half_away_defect():
    x = tb.to_u8_inputs()
    y = x * 127.5 + 127.5
    assert bool((y == torch.floor(y) + 0.5).sum() >= 200)                 # the preimages do land on the ties in fp32
    assert not torch.equal(tb.to_u8_ref(x, half_away=True), tb.to_u8_ref(x))
    assert tb.to_u8_ref(torch.tensor([-1.2, -1.0, -0.0, 1.0, 1.2])).tolist() == [0, 0, 128, 255, 255]


def test_one_minus_byte_on_torch():
    """TransRef.set_input's mask channels are 1 - mask.byte(): 1 and 0 for a 0 / 1 mask, -254 for a 0 / 255 one, and the byte of a float is
    its integer part modulo 256 whatever the tensor's length (the vectorised conversion included)"""
    for n in (30, 257, 4099):
        m = tb.pack_masks(n, n)
        byte = m.byte()
        assert torch.equal(byte, m.to(torch.int64).remainder(256).to(torch.uint8))
        x6, ref3, detail = tb.pack_ref(torch.randn(6, n, generator=tb.gen(n)), m)
        assert torch.equal(x6[:, 3], 1 - byte.float()) and torch.equal(x6[:, 4], x6[:, 3]) and torch.equal(x6[:, 5], x6[:, 3])
        for val, want in ((0.0, 1.0), (1.0, 0.0), (1.5, 0.0), (2.0, -1.0), (255.0, -254.0), (255.9, -254.0), (256.0, 1.0), (0.5, 1.0)):
            assert bool((x6[m == val, 3] == want).all()) and bool((m == val).any()), val
        below = torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))
        assert bool((x6[m == below, 3] == 1.0).all()) and bool((m == below).any())
        assert bool((detail[0][byte != 0] == torch.tensor(tb.FILL[0], dtype=torch.float32)).all())


def test_a_bilinear_mix_of_ones_is_one():
    """fl(fl(1 - l) + l) = 1 for every fp32 l of a dense sweep of [0, 1] (and of the small end, where 1 - l rounds to 1): the reference's
    resized binary mask is exactly 1.0 wherever all four taps are 1, so its hole set (byte != 0) is stable"""
    l = torch.cat([torch.linspace(0, 1, 2_000_001), torch.logspace(-45, 0, 200_001, base=10.0), torch.rand(1_000_000, generator=tb.gen(1))])
    assert bool((((1 - l) + l) == 1).all())
    w0, w1 = 1 - l, l
    assert bool(((w0 * 1.0 + w1 * 1.0) == 1).all())


@pytest.mark.parametrize("H,W", tb.ORIGINS)
def test_reference_hole_set_is_stable(H, W):
    """the byte of the resized binary mask is the same in torch-CPU fp32 and in fp64: nonzero exactly where the fp64 value is 1"""
    _, mask, _ = tb.wrapper_inputs(H, W, 60 + H)
    m32 = F.interpolate(mask, size=[512, 512], mode="bilinear")
    m64 = F.interpolate(mask.double(), size=[512, 512], mode="bilinear")
    assert torch.equal(m32.byte(), m64.byte()) and torch.equal(m32.byte().bool(), m64 == 1.0)
    assert H * W == 1 or 0 < int(m32.byte().sum()) < m32.numel()


# ------------------------------------------------------------------------------------------------ argument guards (host only)
EINVAL = 1001
P0 = 0x7f0000000000                                   # never dereferenced: every call below must return before a launch


def test_tr_attention_guard():
    from stitch_amd._lib import lib

    def call(p, ld=(256, 256, 256, 256), heads=2, Nq=40, Nk=40, D=64):
        return lib.st_tr_attention(p[0], ld[0], p[1], ld[1], p[2], ld[2], p[3], ld[3], heads, Nq, Nk, D, 0.125, None)
    base = [P0 + (i << 28) for i in range(4)]
    for i in (0, 1):                                                     # q, k one float off 16-byte alignment
        for off in (4, 8, 12):
            p = list(base)
            p[i] += off
            assert call(p) == EINVAL, (i, off)
    for i in (0, 1):                                                     # ldq, ldk not a multiple of 4 floats
        for d in (1, 2, 3):
            ld = [256] * 4
            ld[i] += d
            assert call(base, ld=tuple(ld)) == EINVAL, (i, d)
    for i in range(4):                                                   # any ld below heads D
        ld = [256] * 4
        ld[i] = 124
        assert call(base, ld=tuple(ld)) == EINVAL, i
    for kw in (dict(heads=0), dict(heads=-1), dict(Nq=0), dict(Nk=0), dict(D=48), dict(D=16), dict(D=96), dict(D=512)):
        assert call(base, **kw) == EINVAL, kw
    for i in range(4):
        p = list(base)
        p[i] = None
        assert call(p) == EINVAL, i


def test_tr_blend_and_shape_guards():
    from stitch_amd._lib import lib
    a, b, c, d = (P0 + (i << 28) for i in range(4))
    for planes in (0, 2, 4, -1):
        assert lib.st_tr_blend(a, b, c, planes, d, 100, None) == EINVAL, planes
    assert lib.st_tr_blend(a, b, c, 1, d, 0, None) == EINVAL
    assert lib.st_tr_deform_im2col(a, 3, b, 18, c, 4, 4, 4, None) == EINVAL            # ldx < C
    assert lib.st_tr_deform_im2col(a, 4, b, 17, c, 4, 4, 4, None) == EINVAL            # ldoff < 18
    assert lib.st_tr_phase_interleave(a, b, 3, None, 0, 2, 2, 4, None) == EINVAL       # ldo < C
    assert lib.st_tr_phase_interleave(a, b, 4, c, 3, 2, 2, 4, None) == EINVAL          # ldr < C
    assert lib.st_tr_dwconv3x3_gelu(a, 3, b, c, d, 4, 2, 2, 4, None) == EINVAL
    assert lib.st_tr_add(a, 4, b, 4, c, 3, 2, 4, None) == EINVAL
    for H, W, C in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
        assert lib.st_tr_dwconv3x3_gelu(a, 4, b, c, d, 4, H, W, C, None) == EINVAL
        assert lib.st_tr_deform_im2col(a, 4, b, 18, c, H, W, C, None) == EINVAL
        assert lib.st_tr_phase_interleave(a, b, 4, None, 0, H, W, C, None) == EINVAL


# ------------------------------------------------------------------------------------------------ the stage fixture
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_stage_fixture_keys_shapes_and_size():
    gold = {f: np.load(os.path.join(GOLDEN, f)) for f in tb.STAGE_FILES}
    want = {f: set() for f in tb.STAGE_FILES}
    for name, (kind, _, _, (H, W), cin, _) in tb.STAGES.items():
        ins, out, e32 = tb.load_stage(gold, name)
        assert [tuple(t.shape) for t in ins] == [tuple(t.shape) for t in tb.stage_inputs(name)] and all(t.dtype == torch.float32 for t in ins)
        assert all(torch.equal(a, b) for a, b in zip(ins, tb.stage_inputs(name))), name               # the stored input is the seeded one
        assert tuple(out.shape) == tb.stage_out_shape(name) and out.dtype == torch.float64 and bool(torch.isfinite(out).all())
        assert 0 < e32[0] < 1e-5 and 0 < e32[1] < 1e-5, (name, e32)                                  # an fp32 run's distance from fp64
        want[tb.stage_file(name)] |= {f"{name}.in{j}" for j in range(len(cin))} | {f"{name}.e32"} | \
            ({f"{name}.out_hi", f"{name}.out_lo"} if kind == "refpa" else {f"{name}.out64"})
    total = 0
    for f in tb.STAGE_FILES:
        assert set(gold[f].files) == want[f], f
        size = os.path.getsize(os.path.join(GOLDEN, f))
        assert size <= tb.STAGE_FILE_CAP, (f, size)
        total += size
    assert total < 2_000_000
    # what the table is meant to reach: ragged key counts, odd sizes, both transposed convolutions at H = 1
    kinds = [s[0] for s in tb.STAGES.values()]
    assert kinds.count("block") == 5 and kinds.count("block_ref") == 3 and kinds.count("refpa") == 3 and kinds.count("nonlocal") == 2
    for name in ("block1", "block2", "block3"):
        (H, W), sr = tb.STAGES[name][3], tb.STAGES[name][5][1]
        assert H % sr or W % sr
    x = torch.randn(7, 5, dtype=torch.float64)
    hi, lo = tb.pack64(x)
    assert (tb.unpack64(hi, lo) - x).abs().max() <= 2.0 ** -9 * 2.0 ** -23 * x.abs().max()


def test_the_tool_reproduces_the_stage_fixture():
    """where the reference tree is present: its submodules, run again by the tool (in a process of its own: the tool installs stand-ins for
    third-party modules), give the stored inputs, outputs and controls"""
    import subprocess
    import sys
    from oracle.ref_harness import stubs
    if not os.path.isdir(os.path.join(stubs.REF_ROOT, "core", "inference", "mix_methods", "utils", "TransRef")):
        pytest.skip("the reference tree is not on this machine")
    tool = os.path.join(os.path.dirname(os.path.dirname(GOLDEN)), "tools", "make_transref_stage_golden.py")
    r = subprocess.run([sys.executable, tool, "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
