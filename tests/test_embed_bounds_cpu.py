"""The bounds of tests/_embed_bounds.py shown on the CPU to be neither wrong nor vacuous, the case tables of tests/test_embed_matrix_gpu.py shown to
reach what they claim, and the C entries of PatchEmbed, the token chain and the small NHWC kernels shown to reject bad arguments before a launch.

1. Sound.  A float32 torch restatement of each operator (the split3 products as six fp32 products of the operands' bf16 parts) lies within E of
   the fp64 reference on every case of the tables.
2. Sharp.  Planted defects in those restatements each leave the bound (ratio > 1), or break a bit-equality, on at least one case; the largest
   ratio per defect is printed (pytest -s).
3. Coverage.  st_patch_conv1's dispatch predicate restated from csrc/nn.hip: the conv1 table reaches the MFMA kernel below and above 48 KiB of LDS
   and the scalar kernel for each of its three reasons; the token-chain rows straddle the 16-row tile and the 64-row workgroup.
4. Rejections.  ST_EINVAL from every entry for every bad size or leading dimension, on a machine without a GPU: nothing was launched."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import _embed_bounds as eb
from test_rows_bounds_cpu import f32_gelu, mm_s3

EINVAL = 1001


# ------------------------------------------------------------------------------------------------ float32 restatements (with the planted defects)
def conv1_32(maps, w36x16, b, Ho, Wo, defect=None):
    M, H, W = maps.shape
    x = F.pad(maps[:, None], (2, 2 * Wo - W + 2, 2, 2 * Ho - H + 2))
    if defect == "halo":                                    # a halo that was never zeroed
        x[:, :, :2], x[:, :, :, :2] = 1e-3, 1e-3
    if defect == "pad1":                                    # one zero row / column behind the image where the taps reach two: the second holds the neighbour
        x[:, :, -1], x[:, :, :, -1] = x[:, :, -3], x[:, :, :, -3]
    w = eb.conv1_w(w36x16)
    if defect == "transposed":
        w = w.transpose(2, 3)
    y = F.conv2d(x, w, b, stride=2)
    return eb.rows_of(y if defect == "no_relu" else y.clamp_min(0))


def conv12_32(maps, wt, defect=None):
    s1 = conv1_32(maps, wt["c0"].reshape(16, 36).t(), wt["b0"], 32, 32, defect).reshape(-1, 32, 32, 16).permute(0, 3, 1, 2)
    return eb.rows_of(F.conv2d(s1, wt["c2"], wt["b2"], stride=2, padding=2).clamp_min(0))


def conv12_halves32(maps, wt, seam_shift=0):
    """patch_c0c2_kernel's work split: a unit is half a map, its 20 rows of s1 come from the 44 map rows [32 h - 6, 32 h + 38) and are zero outside
    the feature map.  seam_shift: the first map row of the lower half off by that much (the defect)."""
    M = maps.shape[0]
    xp = F.pad(maps[:, None], (2, 2, 8, 8))                                            # map row y at 8 + y
    out = torch.empty(M, 32, 16, 16)
    for h in (0, 1):
        y0 = 32 * h - 6 + (seam_shift if h else 0)
        img = xp[:, :, 8 + y0:8 + y0 + 44]                                             # 44 rows, zero halo columns
        s1 = F.conv2d(img, wt["c0"], wt["b0"], stride=2).clamp_min(0)                  # rows r = 0 .. 19 = s1 rows 16 h - 2 + r
        r = torch.arange(20) + 16 * h - 2
        s1 = s1 * ((r >= 0) & (r < 32)).float().reshape(1, 1, 20, 1)
        s1 = F.pad(s1, (2, 2, 0, 0))
        out[:, :, 8 * h:8 * h + 8] = F.conv2d(s1, wt["c2"], wt["b2"], stride=2).clamp_min(0)
    return eb.rows_of(out)


def ln32(x, w, b, eps=1e-5):
    d = x - x.mean(-1, keepdim=True)
    return d * (1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)) * w + b


def embed32(maps, wt, pe_bias, route="fp32", defect=None):
    M, H, W = maps.shape
    Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    x = F.pad(maps[:, None], (0, Wp - W, 0, Hp - H))
    s1 = F.conv2d(x, wt["c0"], wt["b0"], stride=2, padding=2).clamp_min(0)
    s2 = F.conv2d(s1, wt["c2"], wt["b2"], stride=2, padding=2)
    s2 = s2 if defect == "no_relu_c2" else s2.clamp_min(0)
    P = (Hp // 8) * (Wp // 8)
    tab = pe_bias[(torch.arange(M * P) + (1 if defect == "table_row_plus_1" else 0)) % P]
    mm = mm_s3 if route == "split3_tail" else (lambda a, w: a @ w.t())
    if route == "fp32":
        s3 = eb.rows_of(F.conv2d(s2, wt["c4"], wt["b4"], stride=2, padding=2))
    else:
        cols = F.unfold(s2, 6, padding=2, stride=2).transpose(1, 2).reshape(M * P, -1)            # (c, ky, kx) order, as the weight's reshape
        s3 = mm_s3(cols, wt["c4"].reshape(64, -1)) + wt["b4"]
    v = torch.relu(mm(s3, wt["f0"][:, :64]) + tab)
    return ln32(mm(v, wt["f2"]) + wt["fb2"], wt["lw"], wt["lb"])


def pe32(coords, dim=64, band_shift=0):
    """sin / cos of the fp32 argument, correctly rounded (fp64 function, one rounding): inside any n_sin >= 1"""
    a = eb.sine_args32(coords, dim)
    if band_shift:
        f = torch.arange(dim // 4, dtype=torch.float32) + band_shift
        a = torch.stack([((torch.tensor(3.14) * coords[:, i:i + 1]) * f) * torch.tensor(0.005) for i in (0, 1)], 1)
    a = a.double()
    return torch.cat([torch.sin(a[:, 0]), torch.cos(a[:, 0]), torch.sin(a[:, 1]), torch.cos(a[:, 1])], -1).float()


def tc32(d, ntok, defect=None):
    w, x = d["w"], d["x"]
    R = x.shape[0]
    g = (lambda t: F.gelu(t, approximate="tanh")) if defect == "tanh_gelu" else f32_gelu
    query = g(x @ w["w0"].t() + w["b0"]) @ w["w2"].t() + w["b2"]
    y = ln32(query, w["n1w"], w["n1b"], 0.0 if defect == "no_eps" else 1e-5) + pe32(d["coords"], 64, 1 if defect == "band_plus_1" else 0)
    q = y @ w["wq"].t() + w["bq"]
    kv = d["kv"].reshape(R, ntok, 128)
    if defect == "mask_le" and ntok < 8:                     # slot ntok holds the clamped last token
        kv = torch.cat([kv, kv[:, -1:]], 1)
    k, v = (t.reshape(R, -1, 8, 8).transpose(1, 2) for t in (kv[..., :64], kv[..., 64:]))
    if defect == "heads_shift":
        k, v = k.roll(-1, 1), v.roll(-1, 1)
    scale = 0.125 if defect == "scale_eighth" else 8 ** -0.5
    p = torch.softmax((q.reshape(R, 8, 1, 8) @ k.transpose(-1, -2)) * scale, -1)
    proj = (p @ v).reshape(R, 64) @ w["wp"].t() + w["bp"]
    xx = proj if defect == "no_shortcut" else query + proj
    return xx + (g(ln32(xx, w["n2w"], w["n2b"]) @ w["wf0"].t() + w["bf0"]) @ w["wf3"].t() + w["bf3"])


def dwconv32(x, w9c, b):
    C_ = x.shape[-1]
    xn = x.permute(0, 3, 1, 2)
    return ((F.conv2d(xn, w9c.t().reshape(C_, 1, 3, 3), None, padding=1, groups=C_) + b.reshape(1, C_, 1, 1)) + xn).permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------ 1. sound
@pytest.mark.parametrize("case", eb.CONV1_CASES)
def test_conv1_fp32_within_bound_and_impulses_exact(case):
    M, H, W, Ho, Wo, _ = case
    maps, w, b = eb.conv1_inputs(M, H, W, 10 + H)
    ref, E = eb.conv1_bound(maps, w, b, Ho, Wo)
    assert eb.ratio(conv1_32(maps, w, b, Ho, Wo), ref, E) <= 1.0
    assert (ref == 0).float().mean() > 0.2                                       # the ReLU clips
    imp, pos = eb.impulse_maps(H, W)
    out = conv1_32(imp, w, b, Ho, Wo).reshape(len(pos), Ho, Wo, 16)
    for i, p in enumerate(pos):
        assert torch.equal(out[i], eb.conv1_impulse_expected(p, w, b, Ho, Wo)), (case, p)


@pytest.mark.parametrize("kind", eb.CONV12_KINDS)
def test_conv12_fp32_within_bound(kind):
    maps, wt = eb.conv12_inputs(kind, 3, 20)
    ref, E = eb.conv12_bound(maps, wt)
    assert eb.ratio(conv12_32(maps, wt), ref, E) <= 1.0
    assert eb.ratio(conv12_halves32(maps, wt), ref, E) <= 1.0
    if kind == "b0_neg":
        assert torch.equal(ref.float(), wt["b2"].clamp_min(0).expand(ref.shape[0], 32)) and (E <= eb.U * eb.n_gemm(576) * wt["b2"].abs().max()).all()
    if kind == "ones":                                                           # s1 == 1 inside, 0 in the halo: s2 = relu(b2 + the in-range taps of c2)
        ones = F.conv2d(torch.ones(1, 16, 32, 32, dtype=torch.float64), wt["c2"].double(), wt["b2"].double(), stride=2, padding=2).clamp_min(0)
        assert torch.equal(ref[:256], eb.rows_of(ones))


@pytest.mark.parametrize("shape", eb.EMBED_SHAPES)
def test_embed_fp32_within_bound(shape):
    M, H, W = shape
    maps, wt = torch.randn(M, H, W, generator=eb.gen(30 + H)) * 3, eb.embed_weights(31)
    P = ((H + 7) // 8) * ((W + 7) // 8)
    tab = eb.embed_table(P, 32)
    for route in ("fp32",) + (("split3", "split3_tail") if (H, W) == (64, 64) else ()):
        ref, E = eb.embed_bound(maps, wt, tab, route)
        assert eb.ratio(embed32(maps, wt, tab, route), ref, E) <= 1.0, route
        assert E.max() < 0.02 * ref.abs().max(), (route, E.max().item())                   # the bound says something
        for defect in ("no_relu_c2",) + (("table_row_plus_1",) if P > 1 else ()):
            assert planted("embed_" + defect, embed32(maps, wt, tab, route, defect), ref, E) > 1.0, (route, defect)
    dense = eb.embed_weights(31, dense=True)                                               # sound there too, but loose: see embed_weights
    ref, E = eb.embed_bound(maps, dense, tab)
    assert eb.ratio(embed32(maps, dense, tab), ref, E) <= 1.0


def test_split3_parts_are_exact():
    x = torch.randn(4096, generator=eb.gen(40)) * torch.logspace(-6, 6, 4096)
    hi, mid, lo = eb.split3_parts(x)
    assert torch.equal((hi.double() + mid.double() + lo.double()).float(), x)
    hi, mid, lo = eb.split3_parts(x, "mid_from_x")
    assert not torch.equal((hi.double() + mid.double() + lo.double()).float(), x)              # the defect breaks the bit-equality


@pytest.mark.parametrize("case", eb.TC_CASES)
def test_token_chain_fp32_within_bound(case):
    rows, ntok = case
    for kind in eb.TC_KINDS:
        d = eb.tc_inputs(kind, rows, ntok, 50 + rows)
        ref, E = eb.tc_bound(d["x"], d["coords"], d["kv"], ntok, d["w"], n_sin=1.0)
        r = eb.ratio(tc32(d, ntok), ref, E)
        assert r <= 1.0, (case, kind, r)
        assert torch.isfinite(E).all()
        if kind in eb.TC_SHARP_KINDS:                         # the bound says something (const_ln amplifies by eps^-1/2, dense by 8 per layer)
            assert E.max() < 0.1, (case, kind, E.max().item())


@pytest.mark.parametrize("shape", eb.DWCONV_SHAPES)
def test_dwconv_fp32_within_bound(shape):
    B, H, W, C_ = shape
    x, w, b = torch.randn(B, H, W, C_, generator=eb.gen(60)), torch.randn(9, C_, generator=eb.gen(61)), torch.randn(C_, generator=eb.gen(62))
    ref, E = eb.dwconv_bound(x, w, b)
    assert eb.ratio(dwconv32(x, w, b), ref, E) <= 1.0


@pytest.mark.parametrize("mode", list(eb.SINE_MODES))
def test_sine_pe_fp32_within_bound(mode):
    for dim in eb.SINE_DIMS:
        xy = eb.sine_xy(mode, eb.SINE_ROWS[mode], 70)
        ref, E = eb.sine_pe_bound(xy, dim, n_sin=1.0)
        assert eb.ratio(pe32(xy, dim), ref, E) <= 1.0
    if mode == "grid_period":
        assert torch.equal(xy[:15], xy[15:30]) and torch.equal(xy[:15], xy[30:]) and len(xy) == 45      # three periods


def test_blend_and_normalize_restatements_are_the_oracle(monkeypatch):
    from oracle import composition as oc
    g = eb.gen(80)
    w1, w2 = (torch.rand(2, 3, 16, 17, generator=g) * 2 - 1 for _ in range(2))
    m1, m2, o = torch.rand(2, 3, 16, 17, generator=g), torch.rand(2, 3, 16, 17, generator=g), torch.rand(2, 1, 16, 17, generator=g)
    monkeypatch.setattr(oc, "network", lambda sd, a, b: o)
    want = oc.build_model(None, w1, w2, m1, m2)
    l1, l2, st = eb.blend32(w1, w2, m1, m2, o)
    assert torch.equal(l1, want["learned_mask1"]) and torch.equal(l2, want["learned_mask2"]) and torch.equal(st, want["stitched_image"])
    x = torch.randn(1, 3, 512, 512, generator=g) * 150 + 100
    assert torch.equal(eb.normalize32(x), oc.preprocess(x, False))
    # the two production scalings of prep_image: the product with mul is exact, so a contracted mul * q - sub rounds once, like q' - sub
    for mul, div, sub in eb.PREP_SCALINGS:
        q = (torch.rand(4096, generator=g) * 255) / div
        assert torch.equal((mul * q).double(), mul * q.double())
        assert torch.equal(mul * q - sub, (mul * q.double() - sub).float())


# ------------------------------------------------------------------------------------------------ 2. sharp
CAUGHT = {}


def planted(name, out, ref, E):
    r = eb.ratio(out, ref, E)
    CAUGHT[name] = max(CAUGHT.get(name, 0.0), r)
    return r


CONV_DEFECTS = ("transposed", "pad1", "halo", "no_relu", "seam_row")
TC_DEFECTS = ("band_plus_1", "no_eps", "scale_eighth", "mask_le", "heads_shift", "no_shortcut", "tanh_gelu")


def test_conv_defects_leave_the_bound():
    for case in eb.CONV1_CASES:
        M, H, W, Ho, Wo, _ = case
        maps, w, b = eb.conv1_inputs(M, H, W, 10 + H)
        ref, E = eb.conv1_bound(maps, w, b, Ho, Wo)
        for defect in ("transposed", "pad1", "halo", "no_relu"):
            planted("conv1_" + defect, conv1_32(maps, w, b, Ho, Wo, defect), ref, E)
    for kind in eb.CONV12_KINDS:
        maps, wt = eb.conv12_inputs(kind, 3, 20)
        ref, E = eb.conv12_bound(maps, wt)
        for defect in ("transposed", "pad1", "halo", "no_relu"):
            planted(f"conv12_{defect}", conv12_32(maps, wt, defect), ref, E)
            planted(f"conv12_{defect}@{kind}", conv12_32(maps, wt, defect), ref, E)
        planted("conv12_seam_row", conv12_halves32(maps, wt, 1), ref, E)
        planted(f"conv12_seam_row@{kind}", conv12_halves32(maps, wt, 1), ref, E)
    for d in ("transposed", "pad1", "halo", "no_relu"):
        assert CAUGHT["conv1_" + d] > 1.0 and CAUGHT["conv12_" + d] > 1.0, (d, CAUGHT)
    assert CAUGHT["conv12_seam_row"] > 1.0
    # the localising probes do what they are for: the frame maps see the halo and the pad, the seam rows see the seam, the all-ones s1 sees a dirty
    # halo of y1 (here: of the image) at the border only
    assert CAUGHT["conv12_halo@frame"] > 1.0 and CAUGHT["conv12_pad1@frame"] > 1.0 and CAUGHT["conv12_seam_row@seam"] > 1.0
    assert CAUGHT["conv12_no_relu@dense"] > 1.0


def test_token_chain_defects_leave_the_bound():
    for rows, ntok in eb.TC_CASES:
        for kind in eb.TC_KINDS:
            d = eb.tc_inputs(kind, rows, ntok, 50 + rows)
            ref, E = eb.tc_bound(d["x"], d["coords"], d["kv"], ntok, d["w"])
            for defect in TC_DEFECTS:
                planted("tc_" + defect, tc32(d, ntok, defect), ref, E)
    for defect in TC_DEFECTS:
        assert CAUGHT["tc_" + defect] > 1.0, (defect, CAUGHT["tc_" + defect])


def test_every_defect_was_caught():
    if not any(k.startswith("tc_") for k in CAUGHT):
        test_token_chain_defects_leave_the_bound()
    if not any(k.startswith("conv1_") for k in CAUGHT):
        test_conv_defects_leave_the_bound()
    want = {f"{p}_{d}" for p in ("conv1", "conv12") for d in CONV_DEFECTS if (p, d) != ("conv1", "seam_row")} | {"tc_" + d for d in TC_DEFECTS}
    assert want <= set(CAUGHT) and all(CAUGHT[k] > 1.0 for k in want)
    for k in sorted(want):
        print(f"largest max(err / E) of {k}: {CAUGHT[k]:.3g}")


# ------------------------------------------------------------------------------------------------ 3. coverage
def conv1_path(H, W, Ho, Wo, misaligned):
    """st_patch_conv1's dispatch (csrc/nn.hip) -> ("mfma", lds > 48 KiB) or ("scalar", the reasons)"""
    Hl, Wl = 2 * Ho + 4, 2 * ((Wo + 15) // 16 * 16) + 4
    lds = Hl * Wl * 4
    reasons = [n for n, bad in (("frame", not (H + 2 <= Hl and W + 2 <= Wl)), ("lds", lds > 64 * 1024), ("width", W % 4 != 0), ("align", misaligned)) if bad]
    return ("scalar", tuple(reasons), lds) if reasons else ("mfma", lds > 48 * 1024, lds)


def test_the_tables_cover_the_axes():
    got = {c: conv1_path(c[1], c[2], c[3], c[4], c[5] % 4 != 0) for c in eb.CONV1_CASES}
    assert [g[:2] for g in got.values()] == [("mfma", False)] * 4 + [("mfma", True), ("scalar", ("width",)), ("scalar", ("align",)), ("scalar", ("lds",))]
    assert got[(1, 112, 128, 56, 64, 0)][2] == 61248 and got[(1, 128, 128, 64, 64, 0)][2] == 69696
    # every case is a map whose output grid is the padded map's: 2 Ho x 2 Wo is H x W rounded up to a multiple of 8 (4 for the 60-row one)
    assert all(2 * c[3] >= c[1] and 2 * c[4] >= c[2] for c in eb.CONV1_CASES)
    assert any(c[4] % 16 for c in eb.CONV1_CASES) and any(c[4] > 16 for c in eb.CONV1_CASES)          # a ragged last tile, more than one tile per row
    # the fused kernel: fewer units than workgroup slots, odd counts, and 514 units on 512 slots
    assert eb.CONV12_M == (1, 2, 3, 257) and 2 * 257 > 512
    # st_patch_embed: the fused route, the unfused MFMA route, the scalar conv1 (13 x 21 -> 16 x 24), P = 1
    assert (3, 64, 64) in eb.EMBED_SHAPES and (2, 13, 21) in eb.EMBED_SHAPES and (3, 8, 8) in eb.EMBED_SHAPES
    assert conv1_path(13, 21, 8, 12, False)[0] == "scalar" and conv1_path(60, 64, 32, 32, False)[0] == "mfma"
    # the token chain: rows below, at and above the 16-row tile and the 64-row workgroup, two workgroups and one row; ntok 1, 2, some, 8
    rows = [r for r, _ in eb.TC_CASES]
    assert {1, 15, 16, 17, 63, 64, 65, 129} == set(rows) and {n for _, n in eb.TC_CASES} >= {1, 2, 5, 8}
    assert set(eb.TC_LD) == {148, 152, 160} and all(ld % 4 == 0 for ld in eb.TC_LD)
    assert {-(-r // 64) for r in rows} == {1, 2, 3}
    # the small kernels
    assert eb.MAXPOOL_KSP == ((2, 2, 0), (3, 2, 1)) and set(eb.MAXPOOL_C) == {1, 3, 32} and set(eb.SINE_DIMS) == {4, 64, 192}
    assert {(h == 1, w == 1) for _, h, w, _ in eb.DWCONV_SHAPES} == {(True, True), (True, False), (False, True), (False, False)}
    assert any(b * h * w * c // 4 > 256 for b, h, w, c in eb.DWCONV_SHAPES)                               # more than one block


def test_counts_follow_the_kernel_text():
    assert eb.N_CONV1 == 37 and eb.N_DW == 11 and eb.n_gemm(576) == 256 + 3 + 1 + 6 and eb.n_gemm(1152, 2) == 256 + 5 + 2 + 6
    assert eb.n_plan(1152, [0, 0, 1, 0]) == 1152 + 5 + 1 + 6 and eb.n_plan(64, [4, 0, 0, 0]) == 64 + 1 + 1 + 6
    assert eb.n_s3(1152) == 434 and (eb.TC_LN_NM, eb.TC_LN_NV) == (1 + 4 + 1, 2 + 4 + 1 + 1) and eb.TC_ATT == (2, 2, 2, 8, 8)
    assert eb.N_SIN == 2 * eb.N_SIN_MEASURED and eb.C314 != 3.14 and abs(eb.C314 - 3.14) < 3.14 * eb.U and abs(eb.C005 - 0.005) < 0.005 * eb.U


# ------------------------------------------------------------------------------------------------ 4. rejections
def test_entry_rejects_bad_arguments_without_touching_the_gpu():
    """Every call below must return ST_EINVAL; none is a valid call, and a call that got as far as a launch returns a HIP error code on a machine
    without a GPU, never ST_EINVAL.  The addresses are never dereferenced on the host."""
    from stitch_amd._lib import lib
    base = 0x7f0000000000
    A, B_, Cc, D, E_ = (base + (i << 30) for i in range(5))

    def rejected(fn, good, **bad):
        names = list(good)
        for k, v in bad.items():
            for val in (v if isinstance(v, list) else [v]):
                args = [val if n == k else good[n] for n in names]
                assert fn(*args) == EINVAL, (fn.__name__, k, val)

    # ---- csrc/nn.hip
    good = dict(x=A, out=B_, B=2, H=5, W=7, C=8, k=3, s=2, p=1, stream=None)
    rejected(lib.st_maxpool_nhwc, good, x=None, out=None, B=0, H=0, W=0, C=0, k=0, s=0, p=[-1, 2])
    rejected(lib.st_maxpool_nhwc, dict(good, k=2, p=0), H=1, W=1, p=2)                                  # H + 2 p < k; 2 p > k
    rejected(lib.st_maxpool_nhwc, dict(good, k=5, p=2), H=0, W=0)
    assert lib.st_maxpool_nhwc(A, B_, 1, 1, 7, 8, 4, 1, 1, None) == EINVAL                           # 1 + 2 < 4
    good = dict(x=A, w=B_, bias=Cc, out=D, B=2, H=3, W=3, C=8, stream=None)
    rejected(lib.st_dwconv3x3_residual, good, x=None, w=None, bias=None, out=None, B=[0, -1], H=[0, -1], W=[0, -1], C=[0, -4, 6])
    good = dict(out=A, ld=64, rows=10, dim=64, coords=B_, ldc=2, Wg=0, ws=0, period=0, cscale=1.0, coff=0.0, accumulate=0, stream=None)
    rejected(lib.st_sine_pe, good, out=None, ld=[63, 0, -64], rows=[0, -1], dim=[0, 6, -4], ldc=[1, 0, -2], ws=-1, period=-1, accumulate=-1)
    rejected(lib.st_sine_pe, dict(good, coords=None, Wg=5), Wg=[0, -5], ld=60)
    good = dict(src=A, lds=8, dst=B_, ldd=8, rows=4, cols=8, stream=None)
    rejected(lib.st_copy2d, good, src=None, dst=None, lds=[7, 0, -8], ldd=[7, 0], rows=[0, -1], cols=[0, -1])
    good = dict(src=A, dst=B_, B=1, C=3, H=4, W=4, ldo=4, mul=1.0, div=127.5, sub=1.0, stream=None)
    rejected(lib.st_prep_image, good, src=None, dst=None, B=[0, -1], C=[0, -1], H=[0, -1], W=[0, -1], ldo=[2, 0])
    # ---- csrc/composition.hip
    good = dict(x=A, ldx=8, out=B_, ldo=8, B=1, H=5, W=5, C=8, oh=7, ow=7, stream=None)
    rejected(lib.st_resize_nearest_rows, good, x=None, out=None, ldx=[4, 10, 0], ldo=[4, 10, 0], B=0, H=0, W=0, C=[0, 6, -4], oh=[0, -1], ow=[0, -1])
    good = dict(a=A, lda=8, b=B_, ldb=8, out=Cc, ldo=8, rows=5, C=8, stream=None)
    rejected(lib.st_sub_rows, good, a=None, b=None, out=None, lda=[4, 10], ldb=[4, 10], ldo=[4, 10], rows=[0, -1], C=[0, 6])
    ptrs = dict(warp1=A, warp2=A + 4096, mask1=B_, mask2=B_ + 4096, net_out=Cc, ld_net=4, lm1=D, lm2=D + 4096, stitched=E_, B=1, H=4, W=4, stream=None)
    rejected(lib.st_compose_blend, ptrs, warp1=None, warp2=None, mask1=None, mask2=None, net_out=None, lm1=None, lm2=None, stitched=None,
             ld_net=[0, -4], B=0, H=0, W=[0, -1])
    rejected(lib.st_compose_normalize, dict(x=A, out=B_, n=16, stream=None), x=None, out=None, n=[0, -1])
    # ---- PatchEmbed
    good = dict(maps=A, w=B_, bias=Cc, out=D, M=2, H=12, W=20, Ho=8, Wo=12, stream=None)
    rejected(lib.st_patch_conv1, good, maps=None, w=None, bias=None, out=None, M=[0, -1], H=0, W=0, Ho=[0, -1], Wo=[0, -1])
    good = dict(maps=A, w0=B_, b0=Cc, w2=D, b2=D + 4096, s2=E_, M=3, H=64, W=64, stream=None)
    rejected(lib.st_patch_conv12, good, maps=[None, A + 4, A + 8], w0=None, b0=None, w2=[None, D + 4], b2=None, s2=None, M=[0, -1], H=[32, 60, 0], W=[32, 128])
    good = dict(maps=A, w0=B_, b0=Cc, w2=D, b2=D + 4096, planes=E_, pstride=5 * 256 * 32, M=3, H=64, W=64, stream=None)
    rejected(lib.st_patch_conv12_planes, good, maps=[None, A + 4], w0=None, b0=None, w2=[None, D + 4], b2=None, planes=[None, E_ + 2, E_ + 8],
             pstride=[3 * 256 * 32 - 8, 3 * 256 * 32 + 4, 0], M=[0, -1], H=32, W=32)
    w11 = (C.c_void_p * 11)(*[Cc + 4096 * i for i in range(11)])
    hole = (C.c_void_p * 11)(*[Cc + 4096 * i if i != 6 else None for i in range(11)])
    good = dict(maps=A, weights=w11, ld_f0=128, pe_bias=B_, s1=D, s2=D + (1 << 20), s3=D + (2 << 20), s4=D + (3 << 20), tokens=E_, M=2, H=12, W=20,
                ws=None, ws_floats=0, stream=None)
    rejected(lib.st_patch_embed, good, maps=None, weights=[None, hole], ld_f0=[63, 0], pe_bias=None, s1=None, s2=None, s3=None, s4=None, tokens=None,
             M=[0, -1], H=[0, -8], W=[0, -8])
    rejected(lib.st_patch_embed, dict(good, H=64, W=64, s1=None), maps=A + 4)          # no scratch and a map pointer the fused launch cannot take
    good = dict(maps=A, weights=w11, ld_f0=128, pe_bias=B_, planes=D, pstride=5 * 256 * 32, c4=D + (1 << 24), c4_pstride=64 * 1152, s3=D + (2 << 24),
                s4=D + (3 << 24), tokens=E_, M=3, H=64, W=64, tail=None, tail_bytes=0, ws=None, ws_floats=0, stream=None)
    rejected(lib.st_patch_embed_split3, good, maps=[None, A + 4], weights=[None, hole], ld_f0=63, pe_bias=None, planes=[None, D + 8], c4=None, s3=None,
             s4=None, tokens=None, M=[0, -1], H=[60, 32], W=[60, 32], pstride=[3 * 256 * 32 - 8, 3 * 256 * 32 + 4])
    # ---- the token chain
    w16 = (C.c_void_p * 16)(*[Cc + 4096 * i for i in range(16)])
    hole = (C.c_void_p * 16)(*[Cc + 4096 * i if i != 9 else None for i in range(16)])
    good = dict(corr=A, ld=148, coords=B_, kv=D, weights=w16, rows=17, ntok=5, stream=None)
    rejected(lib.st_decoder_token_chain, good, corr=None, ld=[147, 144, 150, 0, -148], coords=None, kv=None, weights=[None, hole], rows=[0, -1], ntok=[0, 9, -1])
