"""PatchEmbed (both conv1 kernels, the fused c0 + c2 kernel in its fp32 and plane forms, st_patch_embed / st_patch_embed_split3), the decoder
token chain and the small NHWC kernels over the shapes, paths and edges at which they can go wrong: every tolerance is ratio <= 1 against the
first-order bound of tests/_embed_bounds.py (counts documented there, shown sound and sharp by tests/test_embed_bounds_cpu.py), everything else
is bit equality -- with an analytic value, with the unfused launches, with a permuted or repeated run, or with a float32 torch restatement.
Every output sits in a buffer with sentinel rows / columns that must be untouched afterwards.  The largest ratio of every case is recorded
through tests/_measure.py."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import _embed_bounds as eb  # noqa: E402
from _measure import check  # noqa: E402

NAN = float("nan")
SENT = -777.25


@pytest.fixture(scope="module")
def ops():
    import stitch_amd
    assert torch.cuda.is_available()
    return stitch_amd.ops


def dev(t):
    return t.cuda().contiguous()


def dev_off(t, off):
    """t on the GPU, contiguous, its first element `off` floats behind a 256-byte boundary"""
    buf = torch.empty(t.numel() + off, device="cuda")
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v


def bar(name, out, ref, E):
    return check(f"embed_{name}_err_over_E", eb.ratio(out.cpu(), ref, E), 1.0, inclusive=True, note="|out - fp64| <= E elementwise (tests/_embed_bounds.py)")


def framed(rows, cols, extra_rows=3, extra_cols=0, fill=NAN):
    """-> (buffer [rows + extra_rows, cols + extra_cols] of `fill`, its [rows, cols] corner view)"""
    wide = torch.full((rows + extra_rows, cols + extra_cols), fill, device="cuda")
    return wide, wide[:rows, :cols]


def frame_untouched(wide, rows, cols, fill=NAN):
    rest = torch.cat([wide[rows:].reshape(-1), wide[:rows, cols:].reshape(-1)])
    return bool(torch.isnan(rest).all()) if fill != fill else bool((rest == fill).all())


# ------------------------------------------------------------------------------------------------ n_sin
def test_n_sin_measurement_stands(ops):
    """sinf / cosf of the device library against the fp64 function of the same fp32 argument, over every argument the cases of this file form
    (the sine_pe kernel writes them unchanged): the figure of _embed_bounds.N_SIN_MEASURED, whose double is the allowance"""
    xy = [eb.sine_xy(m, eb.SINE_ROWS[m], 70) for m in eb.SINE_MODES]
    xy += [eb.tc_inputs(k, r, n, 50 + r)["coords"] for r, n in eb.TC_CASES for k in ("random", "grid", "frac", "far")]
    xy = torch.cat(xy)
    out = torch.empty(len(xy), 192, device="cuda")
    ops.sine_pe(out, 192, coords=dev(xy))
    a = eb.sine_args32(xy, 192).double()
    ref = torch.cat([torch.sin(a[:, 0]), torch.cos(a[:, 0]), torch.sin(a[:, 1]), torch.cos(a[:, 1])], -1)
    err = (out.cpu().double() - ref).abs() / eb.U
    print(f"n_sin: max |sinf - sin| = {err.max().item():.4f} u over {ref.numel()} values, max |a| = {a.abs().max().item():.1f}")
    check("embed_n_sin_measured_u", err.max().item(), eb.N_SIN, inclusive=True, note="allowance = 2 x the documented measurement")


# ------------------------------------------------------------------------------------------------ conv1
@pytest.mark.parametrize("case", eb.CONV1_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv1_matrix(ops, case):
    M, H, W, Ho, Wo, off = case
    maps, w, b = eb.conv1_inputs(M, H, W, 10 + H)
    wd, bd = dev(w), dev(b)
    wide, out = framed(M * Ho * Wo, 16)
    ops.patch_conv1(dev_off(maps.reshape(M, -1), off), wd, bd, out, M, H, W, Ho, Wo)
    ref, E = eb.conv1_bound(maps, w, b, Ho, Wo)
    bar("conv1_" + "x".join(map(str, case)), out, ref, E)
    assert frame_untouched(wide, M * Ho * Wo, 16)
    imp, pos = eb.impulse_maps(H, W)
    n = len(pos)
    wide, out = framed(n * Ho * Wo, 16)
    ops.patch_conv1(dev_off(imp.reshape(n, -1), off), wd, bd, out, n, H, W, Ho, Wo)
    got = out.cpu().reshape(n, Ho, Wo, 16)
    for i, p in enumerate(pos):
        assert torch.equal(got[i], eb.conv1_impulse_expected(p, w, b, Ho, Wo)), (case, p)
    assert frame_untouched(wide, n * Ho * Wo, 16)


# ------------------------------------------------------------------------------------------------ fused c0 + c2
def conv12_dev(wt):
    return dev(wt["c0"].reshape(16, 36).t()), dev(wt["b0"]), dev(eb.pack_conv_w(wt["c2"])), dev(wt["b2"])


@pytest.mark.parametrize("kind,M", [("dense", 1), ("dense", 2), ("dense", 3), ("dense", 257), ("frame", 2), ("seam", 3), ("b0_neg", 1), ("ones", 3)])
def test_conv12_fused_equals_unfused_and_fp64(ops, kind, M):
    maps, wt = eb.conv12_inputs(kind, M, 20 + M)
    w0, b0, w2, b2 = conv12_dev(wt)
    md = dev(maps.reshape(M, 4096))
    s1 = torch.empty(M * 1024, 16, device="cuda")
    ops.patch_conv1(md, w0, b0, s1, M, 64, 64, 32, 32)
    two = torch.empty(M * 256, 32, device="cuda")
    kw = dict(geom=(M, 32, 16, 6, 3, 2, 1, 2, 1), bias=b2, act="relu", split_k=1)
    ops.conv_gemm(s1.view(-1, 32), w2, two, **kw)
    plan = ops.gemm_last_plan()
    assert plan[2] == 1 and plan[0] not in (0, 1), plan                            # unsplit, a folding kernel: the fused kernel's arithmetic
    wide, one = framed(M * 256, 32)
    ops.patch_conv12(md, w0, b0, w2, b2, one, M)
    assert torch.equal(one, two), (kind, M, (one - two).abs().max().item())
    assert frame_untouched(wide, M * 256, 32)
    ref, E = eb.conv12_bound(maps, wt, eb.n_plan(576, plan))
    bar(f"conv12_{kind}_M{M}", one, ref, E)
    if kind == "b0_neg":
        assert torch.equal(one.cpu(), wt["b2"].clamp_min(0).expand(M * 256, 32))
    if kind == "ones":                                                             # every map gives the same, map-independent, result
        assert torch.equal(one[:256], one[256:512]) and torch.equal(one[:256], one[512:])


@pytest.mark.parametrize("M", [3, 1])
def test_conv12_planes_are_the_split_of_the_fp32_result(ops, M):
    maps, wt = eb.conv12_inputs("dense", M, 40 + M)
    w0, b0, w2, b2 = conv12_dev(wt)
    md = dev(maps.reshape(M, 4096))
    one = torch.empty(M * 256, 32, device="cuda")
    ops.patch_conv12(md, w0, b0, w2, b2, one, M)
    pl = ops.Planes(5 * 256, 32, torch.device("cuda"))
    pl.t.fill_(SENT)
    sent = pl.t[0, 0, 0, 0].item()
    ops.patch_conv12_planes(md, w0, b0, w2, b2, pl, M)
    want = ops.split3_pack(one)
    assert want.t.shape == (3, 1, M * 256, 32)
    for p, name in enumerate(("hi", "mid", "lo")):
        assert torch.equal(pl.t[p, 0, :M * 256], want.t[p, 0]), name
        assert bool((pl.t[p, 0, M * 256:] == sent).all()), name                    # rows >= M * 256 of every plane untouched
    hi, mid, lo = eb.split3_parts(one.cpu())
    assert torch.equal(want.t[0, 0].cpu(), hi) and torch.equal(want.t[1, 0].cpu(), mid) and torch.equal(want.t[2, 0].cpu(), lo)


# ------------------------------------------------------------------------------------------------ st_patch_embed / st_patch_embed_split3
def embed_dev(wt):
    return [dev(wt["c0"].reshape(16, 36).t()), dev(wt["b0"]), dev(eb.pack_conv_w(wt["c2"])), dev(wt["b2"]), dev(eb.pack_conv_w(wt["c4"])), dev(wt["b4"]),
            dev(wt["f0"]), dev(wt["f2"]), dev(wt["fb2"]), dev(wt["lw"]), dev(wt["lb"])]


class Embed:
    """one PatchEmbed problem on the GPU with its scratch and the plans of the fp32 GEMMs its routes run"""

    def __init__(self, ops, M, H, W, seed, off=0, dense=False):
        self.ops, self.M, self.H, self.W = ops, M, H, W
        self.maps, self.wt = torch.randn(M, H, W, generator=eb.gen(seed)) * 3, eb.embed_weights(seed + 1, dense=dense)
        Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
        self.g = (Hp // 2, Wp // 2, Hp // 4, Wp // 4, Hp // 8, Wp // 8)
        self.P = self.g[4] * self.g[5]
        self.tab = eb.embed_table(self.P, seed + 2)
        self.md, self.w11, self.tabd = dev_off(self.maps.reshape(M, -1), off), embed_dev(self.wt), dev(self.tab)
        H1, W1, H2, W2, _, _ = self.g
        e = lambda *s: torch.empty(*s, device="cuda")                               # noqa: E731
        self.s1, self.s2, self.s3, self.s4 = e(M * H1 * W1, 16), e(M * H2 * W2, 32), e(M * self.P, 64), e(M * self.P, 128)

    def plans(self, fused):
        ops, M, (H1, W1, H2, W2, H3, W3), w = self.ops, self.M, self.g, self.w11
        p = {}
        if not fused:
            p["c2"] = ops.gemm_plan(self.s1.view(-1, 32), w[2], self.s2, geom=(M, H1, W1 // 2, 6, 3, 2, 1, 2, 1, H2, W2), bias=w[3], act="relu")
        p["c4"] = ops.gemm_plan(self.s2, w[4], self.s3, geom=(M, H2, W2, 6, 6, 2, 2, 2, 2, H3, W3), bias=w[5])
        p["f0"] = ops.gemm_plan(self.s3, w[6][:, :64], self.s4, aux0=self.tabd, row_mod=self.P, act="relu")
        p["f2"] = ops.gemm_plan(self.s4, w[7], self.s4, bias=w[8])
        return p

    def run(self, s1):
        wide, tok = framed(self.M * self.P, 128)
        self.ops.patch_embed(self.md, self.w11, 128, self.tabd, s1, self.s2, self.s3, self.s4, tok, self.M, self.H, self.W)
        assert frame_untouched(wide, self.M * self.P, 128)
        return tok

    def bound(self, route, fused):
        return eb.embed_bound(self.maps, self.wt, self.tab, route, self.plans(fused))


@pytest.mark.parametrize("dense", [False, True])
def test_patch_embed_fused_route(ops, dense):
    e = Embed(ops, 3, 64, 64, 60, dense=dense)
    tok = e.run(None)
    ref, E = e.bound("fp32", True)
    bar("embed_64x64_fused" + ("_dense" if dense else ""), tok, ref, E)
    assert torch.equal(e.run(e.s1), tok)                                            # scratch given or not: the same launches, the same bits


def test_patch_embed_misaligned_maps_fall_back(ops):
    """cost maps one float off 16 bytes: the fused launch cannot take them, the raw entry says so when it has no scratch, the wrapper retries with
    scratch, and the unfused route (the scalar conv1 kernel) computes the same operator"""
    import ctypes as C
    from stitch_amd._lib import lib
    e = Embed(ops, 3, 64, 64, 61, off=1)
    arr = (C.c_void_p * 11)(*[w.data_ptr() for w in e.w11])
    wide, tok = framed(3 * 64, 128)
    rc = lib.st_patch_embed(e.md.data_ptr(), arr, 128, e.tabd.data_ptr(), None, e.s2.data_ptr(), e.s3.data_ptr(), e.s4.data_ptr(), tok.data_ptr(), 3, 64, 64,
                            None, 0, None)
    assert rc == 1001 and frame_untouched(wide, 0, 0)                               # rejected before any launch: nothing written
    tok = e.run(None)
    ref, E = e.bound("fp32", False)
    bar("embed_64x64_misaligned", tok, ref, E)


@pytest.mark.parametrize("shape", [s for s in eb.EMBED_SHAPES if s[1:] != (64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_patch_embed_unfused_shapes(ops, shape):
    M, H, W = shape
    e = Embed(ops, M, H, W, 62 + H)
    tok = e.run(e.s1)
    ref, E = e.bound("fp32", False)
    bar(f"embed_{H}x{W}", tok, ref, E)


@pytest.mark.parametrize("tail", [True, False])
def test_patch_embed_split3_route(ops, tail):
    e = Embed(ops, 3, 64, 64, 70)
    tok32 = e.run(None)
    ref, E32 = e.bound("fp32", True)
    pl = ops.Planes(5 * 256, 32, torch.device("cuda"))
    pl.t.fill_(SENT)
    sent = pl.t[0, 0, 0, 0].item()
    c4p = ops.split3_pack(e.w11[4])
    image = ops.pe_tail_split3_pack(e.w11[6], e.w11[7]) if tail else None
    wide, tok = framed(3 * 64, 128)
    ops.patch_embed_split3(e.md, e.w11, 128, e.tabd, pl, c4p, e.s3, None if tail else e.s4, tok, 3, 64, 64, tail_image=image)
    assert frame_untouched(wide, 3 * 64, 128) and bool((pl.t[:, :, 768:] == sent).all())
    route = "split3_tail" if tail else "split3"
    ref3, E3 = e.bound(route, True)
    bar("embed_64x64_for_" + route, tok32, ref, E32)
    bar(f"embed_{route}", tok, ref3, E3)
    bar(f"embed_{route}_vs_fp32_route", tok, tok32.cpu().double(), E32 + E3)


# ------------------------------------------------------------------------------------------------ the token chain
def seeded_tc_weights(sd):
    p = "flow_backbone.memory_decoder."
    c = p + "decoder_layer.cross_attend."
    names = [p + "flow_token_encoder.0.weight", p + "flow_token_encoder.0.bias", p + "flow_token_encoder.2.weight", p + "flow_token_encoder.2.bias",
             c + "norm1.weight", c + "norm1.bias", c + "q.weight", c + "q.bias", c + "proj.weight", c + "proj.bias", c + "norm2.weight", c + "norm2.bias",
             c + "ffn.0.weight", c + "ffn.0.bias", c + "ffn.3.weight", c + "ffn.3.bias"]
    w = {k: sd[n].detach().float().reshape(64, -1) if n.endswith("weight") and sd[n].dim() > 1 else sd[n].detach().float() for k, n in zip(eb.TC_NAMES, names)}
    w["w0"] = torch.cat([w["w0"], torch.zeros(64, 3)], 1)                          # 81 -> 84 zero-padded columns
    return w


def run_tc(ops, d, rows, ntok, ld):
    """-> cost_global [rows, 64] (on the GPU) after checking that nothing but columns 84..147 of the first `rows` rows changed"""
    wide = torch.full((rows + 3, ld), SENT, device="cuda")
    wide[:rows, :84] = dev(d["x"])
    before = wide.clone()
    ops.decoder_token_chain(wide[:rows], dev(d["coords"]), dev(d["kv"]), [dev(d["w"][n]) for n in eb.TC_NAMES], rows, ntok)
    assert torch.equal(wide[:rows, :84], before[:rows, :84]) and torch.equal(wide[:rows, 148:], before[:rows, 148:]) and torch.equal(wide[rows:], before[rows:])
    return wide[:rows, 84:148]


@pytest.mark.parametrize("case", list(enumerate(eb.TC_CASES)), ids=lambda c: f"{c[1][0]}x{c[1][1]}")
def test_token_chain_matrix(ops, seeded_sd, case):
    i, (rows, ntok) = case
    for j, kind in enumerate(eb.TC_KINDS + ("seeded",)):
        d = eb.tc_inputs("random" if kind == "seeded" else kind, rows, ntok, 50 + rows, w=seeded_tc_weights(seeded_sd) if kind == "seeded" else None)
        out = run_tc(ops, d, rows, ntok, eb.TC_LD[(i + j) % 3])
        ref, E = eb.tc_bound(d["x"], d["coords"], d["kv"], ntok, d["w"])
        bar(f"tc_{rows}x{ntok}_{kind}", out, ref, E)


@pytest.mark.parametrize("case", list(enumerate(eb.TC_CASES)), ids=lambda c: f"{c[1][0]}x{c[1][1]}")
def test_token_chain_properties(ops, case):
    i, (rows, ntok) = case
    ld = eb.TC_LD[i % 3]
    d = eb.tc_inputs("random", rows, ntok, 50 + rows)
    out = run_tc(ops, d, rows, ntok, ld)
    assert torch.equal(run_tc(ops, d, rows, ntok, ld), out)                        # a second call repeats the bits
    perm = torch.randperm(rows, generator=eb.gen(rows))
    kv = d["kv"].reshape(rows, ntok, 128)
    dp = dict(d, x=d["x"][perm], coords=d["coords"][perm], kv=kv[perm].reshape(-1, 128))
    assert torch.equal(run_tc(ops, dp, rows, ntok, ld), out[perm.cuda()])          # a row's result does not depend on its place in the tile
    if ntok == 1:                                                                  # one token: its weight is exp(0) / 1, whatever k is
        k2 = d["kv"].clone()
        k2[:, :64] = torch.randn(rows, 64, generator=eb.gen(7)) * 50
        assert torch.equal(run_tc(ops, dict(d, kv=k2), rows, ntok, ld), out)


# ------------------------------------------------------------------------------------------------ the small kernels
@pytest.mark.parametrize("ksp", eb.MAXPOOL_KSP)
def test_maxpool_matrix(ops, ksp):
    k, s, p = ksp
    for H, W in eb.MAXPOOL_HW + (((1, 1),) if p else ()):
        for Cc in eb.MAXPOOL_C:
            x = -torch.rand(2, Cc, H, W, generator=eb.gen(H + Cc)) - 0.5            # all negative: a pad read as 0 wins the maximum
            ref = F.max_pool2d(x, k, s, p)
            Ho, Wo = ref.shape[2:]
            wide, out = framed(2 * Ho * Wo, Cc)
            ops.maxpool(dev(x.permute(0, 2, 3, 1).reshape(-1, Cc)), out, 2, H, W, Cc, k, s, p)
            assert torch.equal(out.cpu().reshape(2, Ho, Wo, Cc).permute(0, 3, 1, 2), ref), (ksp, H, W, Cc)
            assert frame_untouched(wide, 2 * Ho * Wo, Cc)


@pytest.mark.parametrize("shape", eb.DWCONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dwconv3x3_residual_matrix(ops, shape):
    B, H, W, Cc = shape
    x, w, b = torch.randn(B, H, W, Cc, generator=eb.gen(60)), torch.randn(9, Cc, generator=eb.gen(61)), torch.randn(Cc, generator=eb.gen(62))
    wide, out = framed(B * H * W, Cc)
    ops.dwconv3x3_residual(dev(x.reshape(-1, Cc)), dev(w), dev(b), out, B, H, W, Cc)
    ref, E = eb.dwconv_bound(x, w, b)
    bar("dwconv_" + "x".join(map(str, shape)), out.reshape(B, H, W, Cc), ref, E)
    assert frame_untouched(wide, B * H * W, Cc)


@pytest.mark.parametrize("mode", list(eb.SINE_MODES))
def test_sine_pe_matrix(ops, mode):
    worst = 0.0
    for dim in eb.SINE_DIMS:
        for rows in (eb.SINE_ROWS[mode], 1):
            xy = eb.sine_xy(mode, rows, 70)
            pe, Epe = eb.sine_pe_bound(xy, dim)
            kw = dict(eb.SINE_MODES[mode], **({"coords": dev(xy)} if mode == "coords" else {}))
            for acc in (0, 1, max(dim // 2, 2)):
                prev = torch.randn(rows, dim, generator=eb.gen(dim + acc))
                wide, out = framed(rows, dim, extra_cols=6, fill=SENT)
                out.copy_(prev)
                ops.sine_pe(out, dim, accumulate=acc, **kw)
                added = torch.arange(dim) >= (0 if acc == 1 else acc if acc > 1 else dim)
                ref = torch.where(added, prev.double() + pe, pe)
                E = torch.where(added, Epe + eb.U * ref.abs(), Epe)
                worst = max(worst, eb.ratio(out.cpu(), ref, E))
                assert frame_untouched(wide, rows, dim, SENT), (mode, dim, rows, acc)
    check(f"embed_sine_pe_{mode}_err_over_E", worst, 1.0, inclusive=True)


def test_copy2d_and_prep_image(ops):
    for rows, cols in ((37, 19), (37, 1), (1, 19), (300, 7)):
        src_w = torch.randn(rows, cols + 5, generator=eb.gen(rows + cols)).cuda()
        dst_w = torch.full((rows, cols + 9), SENT, device="cuda")
        for a, b in ((0, 0), (3, 2), (5, 9), (0, 9)):
            dst_w.fill_(SENT)
            ops.copy2d(src_w[:, a:a + cols], dst_w[:, b:b + cols])
            want = torch.full_like(dst_w, SENT)
            want[:, b:b + cols] = src_w[:, a:a + cols]
            assert torch.equal(dst_w, want), (rows, cols, a, b)
    x = (torch.rand(2, 3, 5, 7, generator=eb.gen(90)) * 255).round()
    x.view(-1)[:6] = torch.tensor([0.0, 255.0, 127.5, 0.3, 254.7, 1.0])
    for mul, div, sub in eb.PREP_SCALINGS:
        for ldo in (3, 4, 8):
            wide, out = framed(2 * 35, ldo)
            ops.prep_image(dev(x), out, ldo, mul, div, sub)
            assert torch.equal(out.cpu(), eb.prep32(x, ldo, mul, div, sub)), (mul, div, sub, ldo)
            assert bool((out[:, 3:] == 0).all()) and frame_untouched(wide, 2 * 35, ldo)


@pytest.mark.parametrize("case", eb.RESIZE_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}to{c[1][0]}x{c[1][1]}")
def test_resize_nearest_rows_matrix(ops, case):
    (H, W), (oh, ow) = case
    for Cc in (4, 8):
        x = torch.randn(2, Cc, H, W, generator=eb.gen(H + oh))
        xw = torch.full((2 * H * W, Cc + 4), SENT, device="cuda")
        xw[:, :Cc] = dev(x.permute(0, 2, 3, 1).reshape(-1, Cc))
        wide, out = framed(2 * oh * ow, Cc, extra_cols=4)
        ops.resize_nearest_rows(xw[:, :Cc], out, 2, H, W, Cc, oh, ow)
        assert torch.equal(out.cpu().reshape(2, oh, ow, Cc).permute(0, 3, 1, 2), F.interpolate(x, size=(oh, ow), mode="nearest")), (case, Cc)
        assert frame_untouched(wide, 2 * oh * ow, Cc)


def test_sub_rows_blend_and_normalize(ops):
    a, b = torch.randn(41, 12, generator=eb.gen(91)).cuda(), torch.randn(41, 16, generator=eb.gen(92)).cuda()
    wide, out = framed(41, 8, extra_cols=4)
    ops.sub_rows(a[:, 4:12], b[:, :8], out)
    assert torch.equal(out, a[:, 4:12] - b[:, :8]) and frame_untouched(wide, 41, 8)
    for H, W in eb.BLEND_HW:
        g = eb.gen(H)
        w1, w2 = (torch.rand(2, 3, H, W, generator=g) * 2 - 1 for _ in range(2))
        m1, m2 = torch.rand(2, 3, H, W, generator=g), torch.rand(2, 3, H, W, generator=g)           # soft masks
        net = torch.rand(2 * H * W, 4, generator=g)
        l1, l2, st = (torch.empty(2, 3, H, W, device="cuda") for _ in range(3))
        ops.compose_blend(dev(w1), dev(w2), dev(m1), dev(m2), dev(net)[:, 1:2], l1, l2, st)
        want = eb.blend32(w1, w2, m1, m2, net[:, 1].reshape(2, 1, H, W))
        assert torch.equal(l1.cpu(), want[0]) and torch.equal(l2.cpu(), want[1]) and torch.equal(st.cpu(), want[2]), (H, W)
    x = eb.normalize_inputs(93)
    wide, out = framed(1, x.numel(), extra_rows=1)
    ops.compose_normalize(dev(x), out.view(x.shape))
    assert torch.equal(out.cpu().view(x.shape), eb.normalize32(x)) and frame_untouched(wide, 1, x.numel())
    assert out.min().item() == -1.0 and out.max().item() == 1.0
