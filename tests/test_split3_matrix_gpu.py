"""The split3 GEMM (csrc/gemm_split3.h through conv_gemm_split3_launch) over its tile configurations, K-ring residues, ragged edges, geometry,
batching, split-K, the persistent walk, epilogue modes, the second A source and the automatic plan: every case against the fp64 product.

Two bars per case:

(a) elementwise: |C - ref| <= tau(K, split) * S per element, S = |x| (*) |w| evaluated in fp64.  tau follows from how the kernel
    accumulates, with u = 2^-24 (the fp32 unit roundoff):
      - x = hi + mid + lo exactly; the three dropped products mid.lo, lo.mid, lo.lo are <= 2 u |x||w| together;
      - per 16 k, six v_mfma_f32_32x32x16_bf16 add exact bf16 products into the fp32 accumulator, one rounding each (<= u |acc|);
        the accumulator is folded into a running total every 256 k (KBLK = 8 K steps), so |acc| <= S of its block and the MFMA roundings
        of all blocks together are <= 6 * min(K, 256) / 16 * u * S;
      - one rounding per fold (ceil(K / 256)), one per split-K slice in the reduction (split), the final acc + tot, the two consumer groups'
        sum (KPAR), the epilogue's fma: together <= (ceil(K / 256) + split + 3) u S.
    tau = u * (6 * min(K, 256) / 16 + ceil(K / 256) + split + 6): fixed, not fitted.  A race, a dropped or duplicated K step, a wrong tap or
    a wrong swizzle moves an element by a whole 16-k slice of products, i.e. about 16 / K of S -- orders of magnitude above tau.
(b) the contraction is no less accurate than the fp32-MFMA kernel on the same inputs: rms error against fp64 <= 1.25x that kernel's, max
    <= 1.5x + 1e-7 (the bars of test_split3_gpu.py::test_split3_conv_vs_fp32_kernel_and_fp64).

Outputs are written into a column slice of a wider NaN-filled buffer: every element outside the [M, N] view must still be NaN afterwards."""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _measure import check  # noqa: E402

U = 2.0 ** -24
STAGES = {31: 3, 32: 4, 33: 4, 34: 3, 35: 3, 36: 4, 37: 3, 38: 4, 39: 4}
NS = [40, 72, 126, 136]                     # ragged against 32-, 64- and 128-wide tiles


@pytest.fixture(scope="module")
def ops():
    import stitch_amd
    assert torch.cuda.is_available()
    return stitch_amd.ops


@pytest.fixture(scope="module")
def ws(ops):
    return ops.new_workspace(torch.device("cuda"))


def tau(K, split=1):
    return U * (6 * min(K, 256) / 16 + math.ceil(K / 256) + split + 6)


def rnd(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def nan_wide(rows, N, off=1, pad=3):
    """[rows, N] view at column `off` of a NaN-filled [rows, N + off + pad] buffer"""
    wide = torch.full((rows, N + off + pad), float("nan"), device="cuda")
    return wide, wide[:, off:off + N]


def untouched(wide, off, N):
    outside = torch.cat([wide[:, :off].flatten(), wide[:, off + N:].flatten()])
    return bool(torch.isnan(outside).all())


def conv64(x, w, B, H, W, Cin, kh, kw, sh, sw, ph, pw, dil, Ho, Wo):
    """channels-last conv in fp64: x [B*H*W, Cin], w [N, kh*kw*Cin] (tap-major) -> [B*Ho*Wo, N]; zero padding ph / pw on the top / left
    and as much as the output size needs on the bottom / right (the kernels read every tap outside the image as zero)"""
    N = w.shape[0]
    X = x.double().view(B, H, W, Cin).permute(0, 3, 1, 2)
    Wt = w.double().view(N, kh, kw, Cin).permute(0, 3, 1, 2)
    need_h, need_w = (Ho - 1) * sh + dil[0] * (kh - 1) + 1, (Wo - 1) * sw + dil[1] * (kw - 1) + 1
    X = F.pad(X, (pw, max(0, need_w - W - pw), ph, max(0, need_h - H - ph)))
    r = F.conv2d(X, Wt, stride=(sh, sw), dilation=dil)[:, :, :Ho, :Wo]
    return r.permute(0, 2, 3, 1).reshape(-1, N)


def bars(name, C, ref, S, t, fp32=None):
    """bar (a) against tau * S; bar (b) against the fp32 kernel's output `fp32` on the same inputs (when given)"""
    err = (C.double() - ref).abs()
    lim = t * S
    ratio = torch.where(lim > 0, err / lim.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf"))).max().item()
    check(f"s3m_{name}_err_over_tau", ratio, 1.0, inclusive=True, note="|C - ref| <= tau(K) |x|(*)|w| elementwise")
    if fp32 is not None:
        scale = ref.pow(2).mean().sqrt().item()
        es, ee = err.pow(2).mean().sqrt().item() / scale, (fp32.double() - ref).pow(2).mean().sqrt().item() / scale
        check(f"s3m_{name}_rms_vs_fp64", es, 1.25 * ee, note="1.25x the fp32 kernel's rms error")
        check(f"s3m_{name}_max_vs_fp64", err.max().item() / scale, 1.5 * (fp32.double() - ref).abs().max().item() / scale + 1e-7,
              note="1.5x the fp32 kernel's max error + 1e-7")


def conv_case(ops, name, *, tile, B=1, H=1, W=1, Cin=32, N=64, kh=1, kw=1, sh=1, sw=1, ph=None, pw=None, dil=(1, 1), out_hw=None, plain=False,
              split=1, ws=None, seed=0):
    """One conv (or plain product, `plain`: M = W rows) through split3 with an explicit tile into a NaN-framed column slice; bars (a), (b),
    the untouched frame and the plan the launcher reports."""
    ph = (dil[0] * (kh - 1)) // 2 if ph is None else ph
    pw = (dil[1] * (kw - 1)) // 2 if pw is None else pw
    K = kh * kw * Cin
    x, w = rnd((B * H * W, Cin), seed), rnd((N, K), seed + 1, K ** -0.5)
    if plain:
        geom, Ho, Wo = None, 1, W
        assert B == 1 and H == 1 and kh == kw == 1
    else:
        Ho = (H + 2 * ph - dil[0] * (kh - 1) - 1) // sh + 1
        Wo = (W + 2 * pw - dil[1] * (kw - 1) - 1) // sw + 1
        geom = (B, H, W, kh, kw, sh, sw, ph, pw)
        if out_hw is not None:
            Ho, Wo = out_hw
            geom = geom + (Ho, Wo)
    M = B * Ho * Wo
    wide, out = nan_wide(M, N)
    kw_ = dict(geom=geom, dil=dil)
    xp, wp = ops.split3_pack(x), ops.split3_pack(w)
    with (ops.workspace_scope(ws) if ws is not None else contextlib.nullcontext()):
        ops.conv_gemm(xp, wp, out, tile=tile, split_k=split, **kw_)
        plan = ops.gemm_last_plan()
        assert ops.gemm_plan(xp, wp, out, tile=tile, split_k=split, **kw_) == plan, (name, plan)      # the plan-only entry answers what the launch did
    oe = torch.empty(M, N, device="cuda")
    ops.conv_gemm(x, w, oe, **kw_)
    torch.cuda.synchronize()
    assert plan[:2] == [8, tile] and plan[2] == split, (name, plan)
    ref = conv64(x, w, B, H, W, Cin, kh, kw, sh, sw, ph, pw, dil, Ho, Wo)
    S = conv64(x.abs(), w.abs(), B, H, W, Cin, kh, kw, sh, sw, ph, pw, dil, Ho, Wo)
    bars(name, out, ref, S, tau(K, plan[2]), oe)
    assert untouched(wide, 1, N), f"{name}: a write outside the [M, N] view"


# (ntiles, shape): K / 32 = ntiles hits every residue of a 3- and a 4-deep ring, one whole 256-k block (8), a fold with a single step behind
# it (9, 17, 33) and two whole blocks (16).  M = 874 (two 19 x 23 maps) or 1001 rows: ragged against 32, 64 and 128.
NTILE_SHAPES = [
    (1, dict(B=2, H=19, W=23, Cin=32)),                        # 1x1
    (2, dict(W=1001, Cin=64, plain=True)),
    (3, dict(B=2, H=19, W=23, Cin=32, kh=3)),                  # 3x1
    (4, dict(B=2, H=19, W=23, Cin=128)),
    (5, dict(B=2, H=19, W=23, Cin=32, kw=5)),                  # 1x5
    (7, dict(B=2, H=19, W=23, Cin=32, kh=7)),                  # 7x1
    (8, dict(W=1001, Cin=256, plain=True)),
    (9, dict(B=2, H=19, W=23, Cin=96, kh=3)),                  # 3x1
    (16, dict(B=2, H=19, W=23, Cin=512)),
    (17, dict(W=1001, Cin=544, plain=True)),
    (33, dict(B=2, H=19, W=23, Cin=96, kw=11)),                # 1x11
]


@pytest.mark.parametrize("tile", [31, 32, 33, 34, 35, 36, 37, 38, 39])
def test_every_tile_at_every_ring_residue(ops, tile):
    """Every cfg, explicit tile, at K-step counts {1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33}; both M and N ragged; C a column slice with ldc > N."""
    seen = set()
    for i, (nt, shp) in enumerate(NTILE_SHAPES):
        K = shp.get("kh", 1) * shp.get("kw", 1) * shp["Cin"]
        assert K == 32 * nt
        seen.add(nt % STAGES[tile])
        conv_case(ops, f"t{tile}_nt{nt}", tile=tile, N=NS[(i + tile) % 4], seed=100 * tile + i, **shp)
    assert seen == set(range(STAGES[tile]))


@pytest.mark.parametrize("tile", [34, 36, 37])
def test_geometry(ops, tile):
    """stride 2, dilation, asymmetric 1 x k / k x 1 taps, explicit output size (bottom / right rows and columns read from zero padding)
    on a 3-stage, a 4-stage and the persistent kernel."""
    s = 10 * tile
    conv_case(ops, f"t{tile}_s2_3x3", tile=tile, B=2, H=19, W=23, Cin=32, N=72, kh=3, kw=3, sh=2, sw=2, seed=s)
    conv_case(ops, f"t{tile}_dil23_3x3", tile=tile, B=1, H=21, W=25, Cin=64, N=40, kh=3, kw=3, dil=(2, 3), seed=s + 2)
    conv_case(ops, f"t{tile}_1x7", tile=tile, B=2, H=17, W=29, Cin=64, N=136, kh=1, kw=7, seed=s + 4)
    conv_case(ops, f"t{tile}_5x1_s21", tile=tile, B=1, H=31, W=15, Cin=96, N=126, kh=5, kw=1, sh=2, sw=1, seed=s + 6)
    # PatchEmbed's form Conv2d(32, 64, 6, 2, 2) with one more output row / column than the input gives (asymmetric zero padding)
    conv_case(ops, f"t{tile}_6x6_s2_geom11", tile=tile, B=3, H=19, W=21, Cin=32, N=64, kh=6, kw=6, sh=2, sw=2, ph=2, pw=2, out_hw=(10, 11),
              seed=s + 8)


@pytest.mark.parametrize("tile", [31, 32, 33, 34, 35, 36])
def test_split_k_slices(ops, ws, tile):
    """Split-K with uneven slices, one of them at ntiles % STAGES == 1: 34 steps at split 4 = 9, 9, 9, 7 (9 % 4 == 1, 7 % 3 == 1);
    17 steps at split 2 = 9, 8; an explicit workspace."""
    conv_case(ops, f"t{tile}_split4_34steps", tile=tile, B=2, H=19, W=23, Cin=64, N=72, kw=17, split=4, ws=ws, seed=20 * tile)
    conv_case(ops, f"t{tile}_split2_17steps", tile=tile, W=1001, Cin=544, N=126, plain=True, split=2, ws=ws, seed=20 * tile + 2)


@pytest.mark.parametrize("tile", [31, 32, 33, 34, 35, 36, 37])
def test_batched(ops, tile):
    """batch = 3 products A_b . W_b^T (the aggregate's form) with ragged M and N, planes stacked along the rows (bsa = M * 32, bsw = N * 32)
    and C a column slice of a NaN-framed buffer (bsc = M * ldc)."""
    Bb, M, N, K = 3, 437, 72, 288
    a, w = rnd((Bb * M, K), 30 + tile), rnd((Bb * N, K), 40 + tile, K ** -0.5)
    wide, out = nan_wide(Bb * M, N)
    ldc = wide.stride(0)
    ops.conv_gemm(ops.split3_pack(a), ops.split3_pack(w), out[:M], M=M, N=N, batch=Bb, bsa=M * 32, bsw=N * 32, bsc=M * ldc, tile=tile)
    plan = ops.gemm_last_plan()
    oe = torch.empty(Bb * M, N, device="cuda")
    ops.conv_gemm(a, w, oe[:M], M=M, N=N, batch=Bb, bsa=M * K, bsw=N * K, bsc=M * N)
    torch.cuda.synchronize()
    assert plan[:3] == [8, tile, 1], plan
    a3, w3 = a.double().view(Bb, M, K), w.double().view(Bb, N, K)
    ref, S = (a3 @ w3.transpose(1, 2)).reshape(-1, N), (a3.abs() @ w3.abs().transpose(1, 2)).reshape(-1, N)
    bars(f"t{tile}_batch3", out, ref, S, tau(K), oe)
    assert untouched(wide, 1, N)


def test_kpar_tiles_reject_batch_and_split(ops, ws):
    """tile_cfg 38 / 39 run neither batches nor split-K (conv_gemm_split3_launch)."""
    M, N, K = 256, 64, 256
    ap, wp = ops.split3_pack(rnd((2 * M, K), 50)), ops.split3_pack(rnd((2 * N, K), 51))
    out = torch.empty(2 * M, N, device="cuda")
    for tile in (38, 39):
        with pytest.raises(ops.StitchErrorBase):
            ops.conv_gemm(ap, wp, out[:M], M=M, N=N, batch=2, bsa=M * 32, bsw=N * 32, bsc=M * N, tile=tile)
        with pytest.raises(ops.StitchErrorBase), ops.workspace_scope(ws):
            ops.conv_gemm(ap, wp, out[:M], M=M, N=N, tile=tile, split_k=2)


def test_persistent_walk(ops):
    """tile_cfg 37: nkt in {1, 2, 3, 8, 9} with 1 323 tiles on 512 workgroup slots (walks of 2 or 3 tiles); batch 3 (G = 512 / 3 = 170 slots for
    320 tiles per batch); the transposed second store (st_corr_volume_split3) at M = N = 1000 (M % 64 != 0)."""
    M, N = 4000, 1300
    for nkt in (1, 2, 3, 8, 9):
        conv_case(ops, f"t37_walk_nkt{nkt}", tile=37, W=M, N=N, Cin=32 * nkt, plain=True, seed=60 + nkt)
    Bb, M, N, K = 3, 2000, 600, 96
    a, w = rnd((Bb * M, K), 70), rnd((Bb * N, K), 71, K ** -0.5)
    wide, out = nan_wide(Bb * M, N)
    ldc = wide.stride(0)
    ops.conv_gemm(ops.split3_pack(a), ops.split3_pack(w), out[:M], M=M, N=N, batch=Bb, bsa=M * 32, bsw=N * 32, bsc=M * ldc, tile=37)
    plan = ops.gemm_last_plan()
    oe = torch.empty(Bb * M, N, device="cuda")
    ops.conv_gemm(a, w, oe[:M], M=M, N=N, batch=Bb, bsa=M * K, bsw=N * K, bsc=M * N)
    torch.cuda.synchronize()
    assert plan == [8, 37, 1, 1], plan
    a3, w3 = a.double().view(Bb, M, K), w.double().view(Bb, N, K)
    bars("t37_walk_batch3", out, (a3 @ w3.transpose(1, 2)).reshape(-1, N), (a3.abs() @ w3.abs().transpose(1, 2)).reshape(-1, N), tau(K), oe)
    assert untouched(wide, 1, N)
    # c_t
    B, Nn, Cc = 2, 1000, 96
    f1, f2 = rnd((B, Nn, Cc), 72), rnd((B, Nn, Cc), 73)
    v12, v21 = torch.empty(B, Nn, Nn, device="cuda"), torch.empty(B, Nn, Nn, device="cuda")
    e12, e21 = torch.empty(B, Nn, Nn, device="cuda"), torch.empty(B, Nn, Nn, device="cuda")
    ops.corr_volume_split3(ops.split3_pack(f1.view(B * Nn, Cc)), ops.split3_pack(f2.view(B * Nn, Cc)), v12, v21, B, Nn, Cc)
    plan = ops.gemm_last_plan()
    ops.corr_volume_both(f1, f2, e12, e21)
    torch.cuda.synchronize()
    assert plan == [8, 37, 1, 1], plan
    assert torch.equal(v21, v12.transpose(1, 2).contiguous())
    ref, S = f1.double() @ f2.double().transpose(1, 2), f1.double().abs() @ f2.double().abs().transpose(1, 2)
    bars("t37_corr_ct", v12.reshape(-1, Nn), ref.reshape(-1, Nn), S.reshape(-1, Nn), tau(Cc), e12.reshape(-1, Nn))


@pytest.mark.parametrize("tile", [32, 36, 37, 38, 39])
def test_gru_epilogue_and_planes(ops, tile):
    """The GRU epilogue (act tanh, (1 - z) h + z tanh(acc + bias)) with planes emission on each kernel family: the four-consumer body with its
    epilogue after the loop (32) and ahead of it (36: one sub-tile per wave), the persistent walk (37), the two-group bodies (38; 39 with its
    epilogue ahead).  C against the epilogue in fp64 at the fp32 epilogue tests' 2e-5 (tests/test_ops_gpu.py); the planes equal
    st_split3_pack(C) bit for bit and leave the neighbouring chunks alone."""
    B, H, W, Cin, N = 2, 16, 16, 64, 96                       # M = 512 (whole 32-row tiles, as planes need); K = 576 (18 steps)
    M, K = B * H * W, 9 * Cin
    s = 80 + tile
    x, w, bias = rnd((M, Cin), s), rnd((N, K), s + 1, K ** -0.5), rnd((N,), s + 2)
    z = torch.rand(M, N, generator=torch.Generator().manual_seed(s + 3)).cuda()
    h = rnd((M, N), s + 4)
    geom = (B, H, W, 3, 3, 1, 1, 1, 1)
    wide, out = nan_wide(M, N)
    pl = ops.Planes(M, 160, "cuda")
    pl.t.zero_()
    ops.conv_gemm(ops.split3_pack(x), ops.split3_pack(w), out, geom=geom, bias=bias, act="tanh", epi="gru", aux1=z, aux2=h,
                  out_planes=pl.cols(32, 128), tile=tile, split_k=1)
    plan = ops.gemm_last_plan()
    torch.cuda.synchronize()
    assert plan[:3] == [8, tile, 1], plan
    acc = conv64(x, w, B, H, W, Cin, 3, 3, 1, 1, 1, 1, (1, 1), H, W) + bias.double()
    want = (1 - z.double()) * h.double() + z.double() * torch.tanh(acc)
    check(f"s3m_t{tile}_gru_epilogue_max_abs", (out.double() - want).abs().max().item(), 2e-5, note="the fp32 epilogue tests' tolerance")
    assert untouched(wide, 1, N)
    assert torch.equal(pl.t[:, 1:4], ops.split3_pack(out.contiguous()).t)
    assert bool((pl.t[:, 0] == 0).all()) and bool((pl.t[:, 4] == 0).all())


@pytest.mark.parametrize("tile", [32, 34, 39])
def test_second_source(ops, tile):
    """a2: input channels below a2_channels come from a second activation (the q conv's [r*h | x]); 1x5 taps, 10 K steps."""
    B, H, W, Cin, N, a2c = 2, 19, 23, 64, 72, 32
    K = 5 * Cin
    x, x2, w = rnd((B * H * W, Cin), 90 + tile), rnd((B * H * W, Cin), 91 + tile), rnd((N, K), 92 + tile, K ** -0.5)
    xe = torch.cat([x2[:, :a2c], x[:, a2c:]], 1).contiguous()
    geom = (B, H, W, 1, 5, 1, 1, 0, 2)
    M = B * H * W
    wide, out = nan_wide(M, N)
    ops.conv_gemm(ops.split3_pack(x), ops.split3_pack(w), out, geom=geom, a2=ops.split3_pack(x2), a2_channels=a2c, tile=tile, split_k=1)
    plan = ops.gemm_last_plan()
    oe = torch.empty(M, N, device="cuda")
    ops.conv_gemm(xe, w, oe, geom=geom)
    torch.cuda.synchronize()
    assert plan[:3] == [8, tile, 1], plan
    ref = conv64(xe, w, B, H, W, Cin, 1, 5, 1, 1, 0, 2, (1, 1), H, W)
    S = conv64(xe.abs(), w.abs(), B, H, W, Cin, 1, 5, 1, 1, 0, 2, (1, 1), H, W)
    bars(f"t{tile}_a2", out, ref, S, tau(K), oe)
    assert untouched(wide, 1, N)


def test_automatic_plan_is_pinned(ops, ws):
    """tile = 0: the launcher's choice (conv_gemm_split3_launch) as st_gemm_last_plan reports it, each run checked against bar (a)."""
    def auto(name, want, seed, tile=0, **shp):
        K = shp.get("kh", 1) * shp.get("kw", 1) * shp["Cin"]
        B, H, W = shp.get("B", 1), shp.get("H", 1), shp["W"]
        kh, kw = shp.get("kh", 1), shp.get("kw", 1)
        x, w = rnd((B * H * W, shp["Cin"]), seed), rnd((shp["N"], K), seed + 1, K ** -0.5)
        geom = None if shp.get("plain") else (B, H, W, kh, kw, 1, 1, kh // 2, kw // 2)
        out = torch.empty(B * H * W, shp["N"], device="cuda")
        with ops.workspace_scope(ws):
            ops.conv_gemm(ops.split3_pack(x), ops.split3_pack(w), out, geom=geom, tile=tile, split_k=0)
        plan = ops.gemm_last_plan()
        torch.cuda.synchronize()
        assert plan == want, (name, plan, want)
        ref = conv64(x, w, B, H, W, shp["Cin"], kh, kw, 1, 1, kh // 2, kw // 2, (1, 1), H, W)
        S = conv64(x.abs(), w.abs(), B, H, W, shp["Cin"], kh, kw, 1, 1, kh // 2, kw // 2, (1, 1), H, W)
        bars(name, out, ref, S, tau(K, plan[2]))

    auto("auto_persist_many_short_tiles", [8, 37, 1, 1], 120, W=4096, Cin=64, N=2048, plain=True)           # 64 x 32 = 2 048 64x64 tiles, K = 64
    auto("auto_128x64_fills_the_cus", [8, 32, 1, 0], 122, W=8192, Cin=256, N=256, plain=True)              # 64 x 4 = 256 128x64 tiles
    auto("auto_64x64_below_256_tiles", [8, 34, 1, 0], 124, W=4096, Cin=256, N=256, plain=True)             # 32 x 4 = 128 128x64 tiles
    auto("auto_kpar_1x11_33steps", [8, 39, 1, 0], 126, B=2, H=64, W=64, Cin=96, N=128, kw=11)              # one 64x64 tile per CU, K = 1 056
    auto("auto_kpar_3x3_k1152", [8, 39, 1, 0], 128, B=2, H=64, W=64, Cin=128, N=128, kh=3, kw=3)
    auto("auto_below_kpar_k992", [8, 34, 1, 0], 130, B=2, H=64, W=64, Cin=32, N=128, kw=31)                # K = 992 < 1 024: no second group
    auto("auto_split2_tile34", [8, 34, 2, 0], 132, tile=34, B=2, H=64, W=64, Cin=96, N=128, kw=11)         # tile 34 given, split_k = 0


KPAR_SHAPES = [(1, dict(Cin=32)), (5, dict(Cin=32, kw=5)), (9, dict(Cin=96, kh=3)), (33, dict(Cin=96, kw=11))]


@pytest.mark.parametrize("tile", [38, 39])
def test_kpar_reduction_is_stable(ops, tile):
    """Regression guard for the two-consumer-group reduction (KPAR = 2): group 1's partial accumulators cross LDS over the start of stage 0,
    which holds the last K step's fragments when ntiles % 4 == 1 -- they were once written before every wave had read those fragments.
    At ntiles in {1, 5, 9, 33} on the M = 8 192, N = 128 shape (one tile per CU for 39), 20 launches each must be bitwise identical to the
    first (no atomics, no split-K: the kernels are deterministic) and within bar (a).  Passing cannot prove that the race is absent (it
    needs a wave to run ahead at the wrong moment); the barrier that closes it is justified by reading the code."""
    B, H, W, N = 2, 64, 64, 128
    for nt, shp in KPAR_SHAPES:
        kh, kw, Cin = shp.get("kh", 1), shp.get("kw", 1), shp["Cin"]
        K = kh * kw * Cin
        assert K == 32 * nt
        x, w = rnd((B * H * W, Cin), 110 + nt), rnd((N, K), 111 + nt, K ** -0.5)
        xp, wp = ops.split3_pack(x), ops.split3_pack(w)
        geom = (B, H, W, kh, kw, 1, 1, kh // 2, kw // 2)
        outs = [torch.empty(B * H * W, N, device="cuda") for _ in range(20)]
        for o in outs:
            ops.conv_gemm(xp, wp, o, geom=geom, tile=tile, split_k=1)
        torch.cuda.synchronize()
        assert ops.gemm_last_plan()[:3] == [8, tile, 1]
        ndiff = sum(not torch.equal(o, outs[0]) for o in outs[1:])
        assert ndiff == 0, f"tile {tile}, {nt} K steps: {ndiff} of 19 repeats differ from the first launch"
        ref = conv64(x, w, B, H, W, Cin, kh, kw, 1, 1, kh // 2, kw // 2, (1, 1), H, W)
        S = conv64(x.abs(), w.abs(), B, H, W, Cin, kh, kw, 1, 1, kh // 2, kw // 2, (1, 1), H, W)
        bars(f"t{tile}_kpar_repeat_nt{nt}", outs[0], ref, S, tau(K))
