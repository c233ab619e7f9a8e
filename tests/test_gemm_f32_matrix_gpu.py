"""The fp32-MFMA implicit-GEMM family (csrc/gemm.hip through conv_gemm_launch / st_conv_gemm_pair / st_corr_volume_both) over its tiles, K-ring
residues, K-block folds, ragged edges, geometry, split-K slices (empty ones included), batches, the persistent walk, epilogue forms, the
second A source, the pair kernel, the small kernels and the automatic plan: every case against the fp64 product.

Two bars per case, both fixed from the code and not from a run:

(a) elementwise against fp64: |C - ref| <= tau(K, split) * S per element, S = |x| (*) |w| evaluated in fp64, u = 2^-24 and

        tau(K, split) = u * (min(K, 256) + ceil(K / 256) + split + 6)

    v_mfma_f32_32x32x2_f32 is an fp32 fma chain: one rounding per k inside a block of at most 256 k (KBLK = 8 K steps: every kernel of the
    family folds its accumulator into a running total there and restarts from zero), one rounding per fold, one per split-K slice in the
    reducer, and 6 for acc + tot, alpha, bias and the epilogue's own operations.  First-order worst case.  A plain fp32 chain on the CPU that
    rounds twice per k (product, then add) with the same fold and slice structure stays below 0.09 of it; the kernels measure at most 0.13
    (one K step, where tau is smallest), and a scratch build that drops the MFMAs of one K step of conv_gemm_dma_body measured 8.5e4 at
    K = 96 and 3.3e3 at K = 1056.  The kernels that never fold (skinny_gemm_kernel and the two narrow-conv kernels: each lane runs one fmaf chain
    over its share of K and a wave reduction adds the 64 partial sums) get the same tau with min(K, 256) -> K: tau(K, 1, folds=False).
(b) bit identity inside the family: every tile pairs k the same way, folds at the same K steps and ends with the same epilogue, so the
    result of any tile equals the register-staged 64x64 kernel's (tile=3) on the same inputs with the same split_k, bit for bit.  Where
    tile 3 cannot run the case (second A source, transposed copy) the comparison is with the formulation it can run (the concatenated
    buffer; out12.transpose).  A tile-3 case has nothing to be compared with (it is the yardstick) and carries bar (a) alone, as do the
    skinny and narrow kernels: they sum k in another order (per-lane strided chains + a wave reduction) and make no such claim.

Cases with an activation or a gate in the epilogue: bar (a) and (b) are applied to a run of the same contraction with epi="store",
act="none"; the epilogue run is compared with the epilogue evaluated in fp64 on the fp64 contraction at the 2e-5 of tests/test_ops_gpu.py
(as test_split3_matrix_gpu.py::test_gru_epilogue_and_planes does) and must equal tile 3's epilogue run bit for bit.

Every output is a column slice (first column 1, ldc > N) of a NaN-filled buffer whose other elements must still be NaN afterwards, and every
case asserts the plan st_gemm_last_plan reports: [family, tile, split, walk]; family 3 = LDS-DMA, 2 = register-staged, 4 = row-streaming,
0 = skinny, 1 = narrow."""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _measure import check  # noqa: E402
from test_split3_matrix_gpu import NS, NTILE_SHAPES, conv64, nan_wide, rnd, untouched  # noqa: E402

U = 2.0 ** -24
NAN = float("nan")
REG_TILES, DMA_TILES = [1, 2, 3, 4], [12, 13, 14, 15]
ACT64 = dict(none=lambda v: v, relu=torch.relu, gelu=F.gelu, tanh=torch.tanh, sigmoid=torch.sigmoid, lrelu=lambda v: F.leaky_relu(v, 0.01))


@pytest.fixture(scope="module")
def ops():
    import stitch_amd
    assert torch.cuda.is_available()
    return stitch_amd.ops


@pytest.fixture(scope="module")
def ws(ops):
    return ops.new_workspace(torch.device("cuda"))


def tau(K, split=1, folds=True):
    return U * ((min(K, 256) if folds else K) + math.ceil(K / 256) + split + 6)


def fam(tile):
    """register-staged tiles 1..4 -> family 2, LDS-DMA tiles 12..15 -> family 3"""
    return 3 if tile > 10 else 2


def bar_a(name, C, ref, S, t):
    err = (C.double() - ref).abs()
    lim = t * S
    ratio = torch.where(lim > 0, err / lim.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf"))).max().item()
    if math.isnan(ratio):
        ratio = float("inf")                                    # an element the kernel never wrote
    return check(f"f32m_{name}_err_over_tau", ratio, 1.0, inclusive=True, note="|C - ref| <= tau(K, split) |x|(*)|w| elementwise, fp64 reference")


class Problem:
    """One contraction (a conv, or a plain product of W rows with `plain`): inputs on the GPU, its fp64 result `ref` and S = |x| (*) |w|."""

    def __init__(self, *, B=1, H=1, W=1, Cin=32, N=64, kh=1, kw=1, sh=1, sw=1, ph=None, pw=None, dil=(1, 1), out_hw=None, plain=False, seed=0):
        ph = (dil[0] * (kh - 1)) // 2 if ph is None else ph
        pw = (dil[1] * (kw - 1)) // 2 if pw is None else pw
        self.K, self.N = kh * kw * Cin, N
        self.x, self.w = rnd((B * H * W, Cin), seed), rnd((N, self.K), seed + 1, self.K ** -0.5)
        if plain:
            assert B == 1 and H == 1 and kh == kw == 1
            geom, Ho, Wo = None, 1, W
        else:
            Ho = (H + 2 * ph - dil[0] * (kh - 1) - 1) // sh + 1
            Wo = (W + 2 * pw - dil[1] * (kw - 1) - 1) // sw + 1
            geom = (B, H, W, kh, kw, sh, sw, ph, pw)
            if out_hw is not None:
                Ho, Wo = out_hw
                geom = geom + (Ho, Wo)
        self.M, self.kw = B * Ho * Wo, dict(geom=geom, dil=dil)
        self.g = (B, H, W, Cin, kh, kw, sh, sw, ph, pw, dil, Ho, Wo)
        self.ref, self.S = self.fp64(self.x), self.fp64(self.x.abs(), self.w.abs())

    def fp64(self, x, w=None):
        return conv64(x, self.w if w is None else w, *self.g)

    def run(self, ops, tile, split=1, ws=None, x=None, zr=False, **epi):
        """one launch into a fresh NaN-framed column slice (and a second one for out2 with `zr`); the workspace is NaN-filled first, so a slab
        that a K slice did not write shows in the result.  -> (wide, out, plan, wide2, out2)"""
        wide, out = nan_wide(self.M, self.N // 2 if zr else self.N)
        wide2, out2 = nan_wide(self.M, self.N // 2) if zr else (None, None)
        kw = dict(self.kw, tile=tile, split_k=split, **epi)
        if zr:
            kw["out2"] = out2
        x = self.x if x is None else x
        if ws is not None:
            ws.fill_(NAN)
        with (ops.workspace_scope(ws) if ws is not None else contextlib.nullcontext()):
            ops.conv_gemm(x, self.w, out, **kw)
            plan = ops.gemm_last_plan()
            assert ops.gemm_plan(x, self.w, out, **kw) == plan, (kw, plan)        # the plan-only entry answers what the launch did
        return wide, out, plan, wide2, out2


def contraction(ops, name, p, tile, split=1, ws=None, want=None, twice=False, ref_tile=3):
    """The raw contraction of problem `p` on `tile`: plan, bar (a), the NaN frame, bar (b) against `ref_tile` (None: no comparison),
    and with `twice` a second launch into a fresh buffer that must be bit-equal (deterministic reducer)."""
    wide, out, plan, _, _ = p.run(ops, tile, split, ws)
    torch.cuda.synchronize()
    want = [fam(tile), tile, split, 0] if want is None else want
    assert plan == want, (name, plan, want)
    ratio = bar_a(name, out, p.ref, p.S, tau(p.K, split))
    assert untouched(wide, 1, p.N), f"{name}: a write outside the [M, N] view"
    if twice:
        _, again, _, _, _ = p.run(ops, tile, split, ws)
        assert torch.equal(out, again), f"{name}: two launches differ"
    if ref_tile is not None and tile != ref_tile:
        _, out3, plan3, _, _ = p.run(ops, ref_tile, split, ws)
        assert plan3[:3] == [fam(ref_tile), ref_tile, split], (name, plan3)
        assert torch.equal(out, out3), f"{name}: not bit-identical to tile {ref_tile} ({(out != out3).sum().item()} elements differ)"
    return ratio


def conv_case(ops, name, *, tile, split=1, ws=None, want=None, twice=False, **shape):
    return contraction(ops, name, Problem(**shape), tile, split, ws, want, twice)


def epilogue(ops, name, p, tile, form, seed, *, want=None, split=1, ws=None, ref_tile=3):
    """The contraction of `p` with the epilogue `form` = dict(bias, alpha, aux0 = "id" | ("div", d) | ("mod", m), act, epi): the plan, the
    result against the epilogue in fp64 on the fp64 contraction at 2e-5, the NaN frame(s), bit identity with `ref_tile`'s run."""
    M, N = p.M, p.N
    act, epi, alpha = form.get("act", "none"), form.get("epi", "store"), form.get("alpha", 1.0)
    kw = dict(act=act, epi=epi, alpha=alpha)
    v = p.ref * alpha
    if form.get("bias"):
        kw["bias"] = rnd((N,), seed)
        v = v + kw["bias"].double()
    a0, rows = form.get("aux0"), torch.arange(M, device="cuda")
    if a0 == "id":
        kw["aux0"] = rnd((M, N), seed + 1)
        v = v + kw["aux0"].double()
    elif a0 is not None and a0[0] == "div":
        kw.update(aux0=rnd(((M + a0[1] - 1) // a0[1], N), seed + 1), row_div=a0[1])
        v = v + kw["aux0"].double()[rows // a0[1]]
    elif a0 is not None:
        kw.update(aux0=rnd((a0[1], N), seed + 1), row_mod=a0[1])
        v = v + kw["aux0"].double()[rows % a0[1]]
    v = ACT64[act](v)
    zr = epi == "zr"
    if epi != "store":
        h = rnd((M, N // 2 if zr else N), seed + 2)
        kw["aux1"] = torch.rand(M, N, generator=torch.Generator().manual_seed(seed + 3)).cuda() if epi == "gru" else h
    if epi == "add":
        v = v + h.double()
    elif epi == "mul":
        v = v * h.double()
    elif epi == "axpy":
        kw["scale_ptr"] = torch.tensor([0.37]).cuda()
        v = h.double() + kw["scale_ptr"].double() * v
    elif epi == "gru":
        kw["aux2"] = h
        v = (1 - kw["aux1"].double()) * h.double() + kw["aux1"].double() * v
    wide, out, plan, wide2, out2 = p.run(ops, tile, split, ws, zr=zr, **kw)
    torch.cuda.synchronize()
    want = [fam(tile), tile, split, 0] if want is None else want
    assert plan == want, (name, plan, want)
    note = "the fp32 epilogue tests' tolerance (tests/test_ops_gpu.py)"
    if zr:
        half = N // 2
        check(f"f32m_{name}_epi_max_abs", (out.double() - v[:, :half]).abs().max().item(), 2e-5, note=note)
        check(f"f32m_{name}_epi_rh_max_abs", (out2.double() - v[:, half:] * h.double()).abs().max().item(), 2e-5, note=note)
        assert untouched(wide, 1, half) and untouched(wide2, 1, half), f"{name}: a write outside the [M, N / 2] views"
    else:
        check(f"f32m_{name}_epi_max_abs", (out.double() - v).abs().max().item(), 2e-5, note=note)
        assert untouched(wide, 1, N), f"{name}: a write outside the [M, N] view"
    if ref_tile is not None and tile != ref_tile:
        _, o3, plan3, _, o32 = p.run(ops, ref_tile, split, ws, zr=zr, **kw)
        assert plan3[:3] == [fam(ref_tile), ref_tile, split], (name, plan3)
        assert torch.equal(out, o3) and (not zr or torch.equal(out2, o32)), f"{name}: not bit-identical to tile {ref_tile}"


# ------------------------------------------------------------------------------------------------ 1. every tile at every ring residue
@pytest.mark.parametrize("tile", REG_TILES + DMA_TILES)
def test_every_tile_at_every_ring_residue(ops, tile):
    """Explicit tile, split_k = 1, K / 32 in {1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33}: the short-ring start-up (fewer tiles than the ring is deep),
    every residue of the 4-deep ring's tail, one whole 256-k block (8: no fold), a fold with a single step behind it (9, 17, 33) and two whole
    blocks (16); M = 874 or 1001 and N in {40, 72, 126, 136}, ragged against 32, 64 and 128.  The register-staged tiles also take K that are
    not whole 32-steps, on the vector path (Cin = 36: K = 36 and 108) and on the scalar-gather path (Cin = 3, 7x7 stride 2: K = 147; Cin = 1,
    6x6 stride 2: K = 36 -- neither padded to 4 channels); an LDS-DMA tile refuses them."""
    seen = set()
    f = "dma" if tile > 10 else "reg"
    for i, (nt, shp) in enumerate(NTILE_SHAPES):
        assert shp.get("kh", 1) * shp.get("kw", 1) * shp["Cin"] == 32 * nt
        seen.add(nt % 4)
        conv_case(ops, f"{f}_t{tile}_nt{nt}", tile=tile, N=NS[(i + tile) % 4], seed=100 * tile + i, **shp)
    assert seen == {0, 1, 2, 3}
    odd = [("k36_1x1", dict(B=2, H=19, W=23, Cin=36, N=72)),
           ("k108_3x1", dict(B=2, H=19, W=23, Cin=36, N=126, kh=3)),
           ("k147_7x7_s2_cin3", dict(B=1, H=37, W=45, Cin=3, N=40, kh=7, kw=7, sh=2, sw=2)),
           ("k36_6x6_s2_cin1", dict(B=3, H=30, W=26, Cin=1, N=72, kh=6, kw=6, sh=2, sw=2, ph=2, pw=2))]
    for i, (nm, shp) in enumerate(odd):
        if tile > 10:
            p = Problem(seed=100 * tile + 50 + i, **shp)
            with pytest.raises(ops.StitchErrorBase):
                p.run(ops, tile)
        else:
            conv_case(ops, f"reg_t{tile}_{nm}", tile=tile, seed=100 * tile + 50 + i, **shp)


# ------------------------------------------------------------------------------------------------ 2. geometry
@pytest.mark.parametrize("tile", [3] + DMA_TILES)
def test_geometry(ops, tile):
    """stride 2, dilation (2, 3), asymmetric 1 x k / k x 1 taps, and an explicit output size one row and one column larger than the input gives
    (geom of length 11: the bottom / right taps read zero padding) -- the shapes of test_split3_matrix_gpu.py::test_geometry."""
    s, f = 2000 + 10 * tile, ("dma" if tile > 10 else "reg")
    conv_case(ops, f"{f}_t{tile}_s2_3x3", tile=tile, B=2, H=19, W=23, Cin=32, N=72, kh=3, kw=3, sh=2, sw=2, seed=s)
    conv_case(ops, f"{f}_t{tile}_dil23_3x3", tile=tile, B=1, H=21, W=25, Cin=64, N=40, kh=3, kw=3, dil=(2, 3), seed=s + 2)
    conv_case(ops, f"{f}_t{tile}_1x7", tile=tile, B=2, H=17, W=29, Cin=64, N=136, kh=1, kw=7, seed=s + 4)
    conv_case(ops, f"{f}_t{tile}_5x1_s21", tile=tile, B=1, H=31, W=15, Cin=96, N=126, kh=5, kw=1, sh=2, sw=1, seed=s + 6)
    conv_case(ops, f"{f}_t{tile}_6x6_s2_geom11", tile=tile, B=3, H=19, W=21, Cin=32, N=64, kh=6, kw=6, sh=2, sw=2, ph=2, pw=2, out_hw=(10, 11),
              seed=s + 8)


# ------------------------------------------------------------------------------------------------ 3. split-K slices
@pytest.mark.parametrize("tile", REG_TILES + DMA_TILES)
def test_split_k_slices(ops, ws, tile):
    """per = ceil(steps / split): 9 steps at split 4 = 3, 3, 3, 0 and at split 8 = 2, 2, 2, 2, 1, 0, 0, 0 -- the empty slices (a workgroup with
    no K step must still write a zero slab for the reducer); on tiles 3 and 12..15 also 34 steps at split 4 = 9, 9, 9, 7 and 17 steps at
    split 2 = 9, 8, and the reducer's own epilogue in GRU and z|r form.  The workspace is NaN before every launch and two launches into fresh
    buffers must agree bit for bit."""
    s, f = 3000 + 20 * tile, ("dma" if tile > 10 else "reg")
    nine = dict(B=2, H=19, W=23, Cin=96, N=72, kh=3)
    conv_case(ops, f"{f}_t{tile}_split4_9steps_empty", tile=tile, split=4, ws=ws, twice=True, seed=s, **nine)
    conv_case(ops, f"{f}_t{tile}_split8_9steps_empty", tile=tile, split=8, ws=ws, twice=True, seed=s + 2, **nine)
    if tile in (1, 2, 4):
        return
    conv_case(ops, f"{f}_t{tile}_split4_34steps", tile=tile, split=4, ws=ws, twice=True, B=2, H=19, W=23, Cin=64, N=72, kw=17, seed=s + 4)
    conv_case(ops, f"{f}_t{tile}_split2_17steps", tile=tile, split=2, ws=ws, twice=True, W=1001, Cin=544, N=126, plain=True, seed=s + 6)
    p = Problem(seed=s + 8, **nine)
    epilogue(ops, f"{f}_t{tile}_split4_gru", p, tile, dict(bias=True, act="tanh", epi="gru"), s + 10, split=4, ws=ws)
    epilogue(ops, f"{f}_t{tile}_split8_zr", p, tile, dict(aux0="id", act="sigmoid", epi="zr"), s + 14, split=8, ws=ws)


# ------------------------------------------------------------------------------------------------ 4. batches
@pytest.mark.parametrize("tile", [3] + DMA_TILES)
def test_batched(ops, tile):
    """batch = 3 products A_b . W_b^T through ops.conv_gemm(batch=, bsa=, bsw=, bsc=, M=, N=) (the form flowformer.py uses): ragged M and N,
    C a column slice of a NaN-framed buffer (bsc = M * ldc); reference per batch in fp64."""
    Bb, M, N, K = 3, 437, 72, 288

    def run(t):
        wide, out = nan_wide(Bb * M, N)
        ops.conv_gemm(a, w, out[:M], M=M, N=N, batch=Bb, bsa=M * K, bsw=N * K, bsc=M * wide.stride(0), tile=t)
        return wide, out, ops.gemm_last_plan()

    a, w = rnd((Bb * M, K), 4000 + tile), rnd((Bb * N, K), 4100 + tile, K ** -0.5)
    wide, out, plan = run(tile)
    torch.cuda.synchronize()
    assert plan == [fam(tile), tile, 1, 0], plan
    a3, w3 = a.double().view(Bb, M, K), w.double().view(Bb, N, K)
    ref, S = (a3 @ w3.transpose(1, 2)).reshape(-1, N), (a3.abs() @ w3.abs().transpose(1, 2)).reshape(-1, N)
    bar_a(f"{'dma' if tile > 10 else 'reg'}_t{tile}_batch3", out, ref, S, tau(K))
    assert untouched(wide, 1, N)
    if tile != 3:
        _, out3, plan3 = run(3)
        assert plan3 == [2, 3, 1, 0] and torch.equal(out, out3)


# ------------------------------------------------------------------------------------------------ 5. the persistent walk
@pytest.mark.parametrize("tile", DMA_TILES)
def test_persistent_walk(ops, ws, tile):
    """M = 4000, N = 1300 is more than 512 workgroups on every LDS-DMA tile (1 323 / 672 / 1 312 / 693 for 13 / 12 / 14 / 15), so with
    K / 32 in {4, 8, 12, 16} a workgroup walks several M tiles (the last one ragged) on one continuous ring; 12 and 16 steps put a fold
    inside a walked tile.  The same shape at 5 steps (not a whole number of ring turns) and with split_k = 2 must not walk and must still
    be right."""
    for nkt in (4, 8, 12, 16):
        conv_case(ops, f"walk_t{tile}_nkt{nkt}", tile=tile, want=[3, tile, 1, 1], W=4000, N=1300, Cin=32 * nkt, plain=True, seed=5000 + 20 * tile + nkt)
    conv_case(ops, f"dma_t{tile}_nowalk_nkt5", tile=tile, want=[3, tile, 1, 0], W=4000, N=1300, Cin=160, plain=True, seed=5400 + tile)
    conv_case(ops, f"dma_t{tile}_nowalk_split2", tile=tile, split=2, ws=ws, want=[3, tile, 2, 0], W=4000, N=1300, Cin=256, plain=True,
              seed=5500 + tile)


def test_persistent_walk_batched(ops):
    """batch 3 on tile 13: 512 / 3 = 170 workgroup slots for the 320 tiles of a batch."""
    Bb, M, N, K = 3, 2000, 600, 128

    def run(t):
        wide, out = nan_wide(Bb * M, N)
        ops.conv_gemm(a, w, out[:M], M=M, N=N, batch=Bb, bsa=M * K, bsw=N * K, bsc=M * wide.stride(0), tile=t)
        return wide, out, ops.gemm_last_plan()

    a, w = rnd((Bb * M, K), 5600), rnd((Bb * N, K), 5601, K ** -0.5)
    wide, out, plan = run(13)
    torch.cuda.synchronize()
    assert plan == [3, 13, 1, 1], plan
    a3, w3 = a.double().view(Bb, M, K), w.double().view(Bb, N, K)
    bar_a("walk_t13_batch3", out, (a3 @ w3.transpose(1, 2)).reshape(-1, N), (a3.abs() @ w3.abs().transpose(1, 2)).reshape(-1, N), tau(K))
    assert untouched(wide, 1, N)
    _, out3, plan3 = run(3)
    assert plan3 == [2, 3, 1, 0] and torch.equal(out, out3)


@pytest.mark.parametrize("B,Nn,Cc,walk", [(2, 2000, 128, 1), (2, 1000, 160, 0)])
def test_transposed_copy(ops, B, Nn, Cc, walk):
    """st_corr_volume_both: f1 . f2^T with the transposed second store.  (2, 2000, 128): 1 024 tiles on 512 / 2 slots, walking, M % 64 != 0;
    (2, 1000, 160): five K steps, not walking.  out12 under bar (a) (alpha = 1) and equal to the register-staged kernel's batched product,
    which cannot write the copy itself; out21 equal to out12 transposed, bit for bit."""
    f1, f2 = rnd((B, Nn, Cc), 5700 + Cc), rnd((B, Nn, Cc), 5701 + Cc)
    both = torch.full((2 * B, Nn, Nn), NAN, device="cuda")
    ops.corr_volume_both(f1, f2, both[:B], both[B:])
    plan = ops.gemm_last_plan()
    torch.cuda.synchronize()
    assert plan == [3, 13, 1, walk], plan
    assert torch.equal(both[B:], both[:B].transpose(1, 2))
    ref, S = f1.double() @ f2.double().transpose(1, 2), f1.double().abs() @ f2.double().abs().transpose(1, 2)
    bar_a(f"{'walk' if walk else 'dma'}_t13_ct_c{Cc}", both[:B].reshape(-1, Nn), ref.reshape(-1, Nn), S.reshape(-1, Nn), tau(Cc))
    out3 = torch.empty(B * Nn, Nn, device="cuda")
    ops.conv_gemm(f1.view(B * Nn, Cc), f2.view(B * Nn, Cc), out3[:Nn], M=Nn, N=Nn, batch=B, bsa=Nn * Cc, bsw=Nn * Cc, bsc=Nn * Nn, tile=3)
    assert ops.gemm_last_plan() == [2, 3, 1, 0]
    assert torch.equal(both[:B].reshape(-1, Nn), out3)


# ------------------------------------------------------------------------------------------------ 6. epilogue forms x kernel families
BASE_FORMS = [
    ("bias_alpha", dict(bias=True, alpha=0.5)),
    ("div7_relu_add", dict(bias=True, aux0=("div", 7), act="relu", epi="add")),
    ("mod5_gelu_axpy", dict(aux0=("mod", 5), act="gelu", epi="axpy", alpha=0.5)),
    ("tanh_gru", dict(bias=True, act="tanh", epi="gru")),
    ("sigmoid_zr", dict(aux0="id", act="sigmoid", epi="zr")),
    ("lrelu_mul", dict(bias=True, act="lrelu", epi="mul")),
]
# one more form per family, a different one each, so that no two families run the same set
EXTRA_FORM = {
    3: ("relu_mul_mod64", dict(aux0=("mod", 64), act="relu", epi="mul")),
    13: ("gelu_add_div8", dict(bias=True, aux0=("div", 8), act="gelu", epi="add")),
    12: ("tanh_axpy", dict(bias=True, act="tanh", epi="axpy")),
    14: ("sigmoid_add_id", dict(aux0="id", act="sigmoid", epi="add")),
    15: ("lrelu_gru", dict(act="lrelu", epi="gru", alpha=0.5)),
    "walk": ("gelu_mul_mod64", dict(bias=True, aux0=("mod", 64), act="gelu", epi="mul")),
}


@pytest.mark.parametrize("tile", [3, 13, 12, 14, 15])
def test_epilogue_forms_tiled(ops, tile):
    """3x3 conv, K = 576 (18 steps), M = 874, N = 126 on the register-staged kernel, the 64x64 LDS-DMA kernel, TM = 2 (12), 128x32 (14) and TN = 2
    (15): bias + alpha, aux0 through row_div and row_mod, every activation and every epi."""
    p = Problem(B=2, H=19, W=23, Cin=64, N=126, kh=3, kw=3, seed=6000 + tile)
    f = "dma" if tile > 10 else "reg"
    contraction(ops, f"{f}_t{tile}_epi_raw", p, tile)
    for i, (nm, form) in enumerate(BASE_FORMS + [EXTRA_FORM[tile]]):
        epilogue(ops, f"{f}_t{tile}_{nm}", p, tile, form, 6100 + 100 * tile + 10 * i)


def test_epilogue_forms_walk(ops):
    """the same forms in the persistent walk (epilogue operands of the next M tile are fetched under the MFMAs of the current one): a plain
    20 000 x 126 product, K = 256, 626 tiles on 512 slots."""
    p = Problem(W=20000, Cin=256, N=126, plain=True, seed=6900)
    contraction(ops, "walk_t13_epi_raw", p, 13, want=[3, 13, 1, 1])
    for i, (nm, form) in enumerate(BASE_FORMS + [EXTRA_FORM["walk"]]):
        epilogue(ops, f"walk_t13_{nm}", p, 13, form, 6910 + 10 * i, want=[3, 13, 1, 1])


ROWS_FORMS = [
    ("bias_alpha", dict(bias=True, alpha=0.5)),
    ("div8_relu_add", dict(bias=True, aux0=("div", 8), act="relu", epi="add")),
    ("mod64_gelu_axpy", dict(aux0=("mod", 64), act="gelu", epi="axpy", alpha=0.5)),
    ("id_tanh_mul", dict(aux0="id", act="tanh", epi="mul")),
    ("sigmoid_add", dict(bias=True, act="sigmoid", epi="add")),
    ("lrelu_mul", dict(bias=True, act="lrelu", epi="mul")),
]


@pytest.mark.parametrize("K", [64, 128])
def test_epilogue_forms_rowstream(ops, K):
    """rowstream_gemm_kernel (tile=20; plain matrices, K = 64 / 128): the forms it takes -- aux0 with row_div <= 1 or 8 and row_mod a multiple
    of 32, no gru, no zr.  With tile=20 the forms it does not take are refused; with tile=0 at a shape the dispatcher would give it
    (M >= 16 384, K = 64) a gru epilogue falls to the register-staged 64x64 kernel (K < 128: no DMA ring) and is still right."""
    p = Problem(W=4100, Cin=K, N=126, plain=True, seed=7000 + K)
    contraction(ops, f"rows_k{K}_epi_raw", p, 20, want=[4, 20, 1, 1])
    for i, (nm, form) in enumerate(ROWS_FORMS):
        epilogue(ops, f"rows_k{K}_{nm}", p, 20, form, 7100 + K + 10 * i, want=[4, 20, 1, 1])
    for form in (dict(act="tanh", epi="gru"), dict(act="sigmoid", epi="zr"), dict(aux0=("div", 7)), dict(aux0=("mod", 5))):
        with pytest.raises(ops.StitchErrorBase):
            epilogue(ops, f"rows_k{K}_refused", p, 20, form, 7200)
    if K == 64:
        big = Problem(W=40000, Cin=64, N=126, plain=True, seed=7300)
        contraction(ops, "rows_k64_auto_raw", big, 0, want=[4, 20, 1, 1])
        epilogue(ops, "reg_t3_rows_shape_gru", big, 0, dict(bias=True, act="tanh", epi="gru"), 7310, want=[2, 3, 1, 0], ref_tile=None)


# ------------------------------------------------------------------------------------------------ 7. second A source, pair kernel
@pytest.mark.parametrize("tile", DMA_TILES)
@pytest.mark.parametrize("kh,kw", [(1, 5), (3, 3)])
def test_second_a_source(ops, tile, kh, kw):
    """a2: input channels below a2_channels come from a second buffer of the same geometry, whose other channels are NaN here (never read).
    Against fp64 on the concatenated buffer, and bit-equal to tile 3 on that buffer (tile 3 takes no second source).  15 and 27 K steps."""
    B, H, W, Cin, N, a2c = 2, 19, 23, 96, NS[(tile + kh) % 4], 32
    p = Problem(B=B, H=H, W=W, Cin=Cin, N=N, kh=kh, kw=kw, seed=8000 + 10 * tile + kh)
    x2 = rnd((B * H * W, Cin), 8001 + 10 * tile + kh)
    xe = torch.cat([x2[:, :a2c], p.x[:, a2c:]], 1).contiguous()
    x2[:, a2c:] = NAN
    wide, out, plan, _, _ = p.run(ops, tile, a2=x2, a2_channels=a2c)
    torch.cuda.synchronize()
    assert plan == [3, tile, 1, 0], plan
    bar_a(f"dma_t{tile}_a2_{kh}x{kw}", out, p.fp64(xe), p.fp64(xe.abs(), p.w.abs()), tau(p.K))
    assert untouched(wide, 1, N)
    _, out3, plan3, _, _ = p.run(ops, 3, x=xe)
    assert plan3 == [2, 3, 1, 0] and torch.equal(out, out3)


def test_pair_kernel(ops):
    """st_conv_gemm_pair: two convs of different K-step residues (9 and 18 steps) and widths in one launch, each member under bar (a) and
    bit-equal to its own tile-3 launch; then the pair with epilogues (bias + relu; bias + relu + residual add) against fp64 at 2e-5."""
    p0 = Problem(B=2, H=19, W=23, Cin=32, N=72, kh=3, kw=3, seed=8500)
    p1 = Problem(B=2, H=19, W=23, Cin=64, N=40, kh=3, kw=3, seed=8502)
    (w0, o0), (w1, o1) = nan_wide(p0.M, p0.N), nan_wide(p1.M, p1.N)
    ops.conv_gemm_pair((p0.x, p0.w, o0, dict(p0.kw)), (p1.x, p1.w, o1, dict(p1.kw)))
    plan = ops.gemm_last_plan()
    torch.cuda.synchronize()
    assert plan == [3, 13, 1, 3], plan
    for i, (p, wide, o) in enumerate([(p0, w0, o0), (p1, w1, o1)]):
        bar_a(f"pair_member{i}", o, p.ref, p.S, tau(p.K))
        assert untouched(wide, 1, p.N)
        _, o3, plan3, _, _ = p.run(ops, 3)
        assert plan3 == [2, 3, 1, 0] and torch.equal(o, o3)
    b0, b1, res = rnd((p0.N,), 8510), rnd((p1.N,), 8511), rnd((p1.M, p1.N), 8512)
    (w0, o0), (w1, o1) = nan_wide(p0.M, p0.N), nan_wide(p1.M, p1.N)
    ops.conv_gemm_pair((p0.x, p0.w, o0, dict(p0.kw, bias=b0, act="relu")), (p1.x, p1.w, o1, dict(p1.kw, bias=b1, act="relu", epi="add", aux1=res)))
    torch.cuda.synchronize()
    note = "the fp32 epilogue tests' tolerance (tests/test_ops_gpu.py)"
    check("f32m_pair_member0_relu_epi_max_abs", (o0.double() - torch.relu(p0.ref + b0.double())).abs().max().item(), 2e-5, note=note)
    check("f32m_pair_member1_relu_add_epi_max_abs", (o1.double() - (torch.relu(p1.ref + b1.double()) + res.double())).abs().max().item(), 2e-5, note=note)
    assert untouched(w0, 1, p0.N) and untouched(w1, 1, p1.N)
    _, r0, _, _, _ = p0.run(ops, 3, bias=b0, act="relu")
    _, r1, _, _, _ = p1.run(ops, 3, bias=b1, act="relu", epi="add", aux1=res)
    assert torch.equal(o0, r0) and torch.equal(o1, r1)


# ------------------------------------------------------------------------------------------------ 8. the small kernels
def test_skinny_kernel(ops):
    """skinny_gemm_kernel: M in {1, 5, 8} x N in {3, 257, 4096} x K in {32, 100, 4096} with bias, alpha and an activation; a lane runs one
    fmaf chain over k = 4 lane + 256 i and a wave reduction adds the 64 chains: no fold, tau with K in place of min(K, 256), no bar (b).
    M = 9 falls through to the MFMA kernels."""
    wfull = rnd((4096, 4096), 9000)
    for K in (32, 100, 4096):
        for N in (3, 257, 4096):
            w = (wfull[:N, :K] * K ** -0.5).contiguous()
            for M in (1, 5, 8, 9):
                a, bias = rnd((M, K), 9001 + M + K), rnd((N,), 9002 + N)
                wide, out = nan_wide(M, N)
                ops.conv_gemm(a, w, out, bias=bias, alpha=0.5, split_k=1)
                plan = ops.gemm_last_plan()
                torch.cuda.synchronize()
                # M = 9: the 64x64 tile, or 128x32 for N <= 32; the LDS-DMA ring from K = 128 up when K is whole 32-steps
                mfma = [3, 14 if N <= 32 else 13, 1, 0] if K == 4096 else [2, 4 if N <= 32 else 3, 1, 0]
                assert plan == ([0, 0, 1, 0] if M <= 8 else mfma), (M, N, K, plan)
                acc, S = a.double() @ w.double().T, a.double().abs() @ w.double().abs().T
                name = f"{'skinny' if M <= 8 else 'dma' if K == 4096 else 'reg'}_m{M}_n{N}_k{K}"
                # |alpha acc + bias - ref| <= tau (alpha S + |bias|): the bound goes through the affine epilogue as it is
                bar_a(name, out, 0.5 * acc + bias.double(), 0.5 * S + bias.double().abs(), tau(K, 1, folds=M > 8))
                assert untouched(wide, 1, N), name
                if M == 5:
                    wide, out = nan_wide(M, N)
                    ops.conv_gemm(a, w, out, bias=bias, alpha=0.5, act="tanh", split_k=1)
                    assert ops.gemm_last_plan() == [0, 0, 1, 0]
                    check(f"f32m_{name}_tanh_epi_max_abs", (out.double() - torch.tanh(0.5 * acc + bias.double())).abs().max().item(), 2e-5,
                          note="the fp32 epilogue tests' tolerance (tests/test_ops_gpu.py)")
                    assert untouched(wide, 1, N), name


@pytest.mark.parametrize("B,H,W", [(2, 40, 13), (2, 24, 22)])
@pytest.mark.parametrize("N", [1, 2])
def test_narrow_conv3x3_kernel(ops, B, H, W, N):
    """narrow_conv3x3_kernel<2> (3x3, stride 1, pad 1, Cin = 256, N <= 2; 8 output pixels of a row per wave) at W not a multiple of 8 and
    B H W >= 1 024: a lane runs one chain over 9 taps x its 4 channels, a butterfly adds the 64 lanes: no fold, tau with K, no bar (b)."""
    p = Problem(B=B, H=H, W=W, Cin=256, N=N, kh=3, kw=3, seed=9100 + W + N)
    assert p.M >= 1024 and W % 8
    wide, out, plan, _, _ = p.run(ops, 0)
    torch.cuda.synchronize()
    assert plan == [1, 0, 1, 0], plan
    bar_a(f"narrow3x3_w{W}_n{N}", out, p.ref, p.S, tau(p.K, 1, folds=False))
    assert untouched(wide, 1, N)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("Cin", [128, 100])
@pytest.mark.parametrize("N", [1, 3, 4])
def test_narrow_conv_kernel(ops, k, Cin, N):
    """narrow_conv_kernel<4> (N <= 4, one wave per output pixel) at M = 1 024, the threshold; M = 1 023 must take the MFMA path instead:
    N <= 32 gives the 128x32 tile, on the LDS-DMA ring when Cin % 32 == 0 and K >= 128, register-staged otherwise."""
    p = Problem(B=1, H=32, W=32, Cin=Cin, N=N, kh=k, kw=k, seed=9200 + 10 * Cin + N + k)
    wide, out, plan, _, _ = p.run(ops, 0)
    torch.cuda.synchronize()
    assert p.M == 1024 and plan == [1, 0, 1, 0], plan
    bar_a(f"narrow_{k}x{k}_c{Cin}_n{N}", out, p.ref, p.S, tau(p.K, 1, folds=False))
    assert untouched(wide, 1, N)
    q = Problem(B=1, H=31, W=33, Cin=Cin, N=N, kh=k, kw=k, seed=9300 + 10 * Cin + N + k)
    assert q.M == 1023
    mfma = [3, 14, 1, 0] if Cin % 32 == 0 and q.K >= 128 else [2, 4, 1, 0]
    contraction(ops, f"{'dma_t14' if mfma[0] == 3 else 'reg_t4'}_m1023_{k}x{k}_c{Cin}_n{N}", q, 0, want=mfma)


# ------------------------------------------------------------------------------------------------ 9. the automatic plan
AUTO = [
    # name, expected plan, shape -- each derived by hand from the text of conv_gemm_launch (64x64 tiles unless N <= 32; DMA when Cin % 32 == 0, K >= 128)
    ("plain_4096x128x2560", [3, 13, 2, 0], dict(W=4096, Cin=2560, N=128, plain=True)),          # 64 x 2 = 128 tiles < 256: split ceil(256 / 128) = 2
    ("conv3x3_874x72_c64", [3, 13, 2, 0], dict(B=2, H=19, W=23, Cin=64, N=72, kh=3, kw=3)),      # 28 tiles: split 10, capped by K / 256 = 2
    ("plain_8192x24x256", [3, 14, 1, 0], dict(W=8192, Cin=256, N=24, plain=True)),              # N <= 32: 128x32; K < 512: no split; 64 tiles: no walk
    ("plain_300x70x36", [2, 3, 1, 0], dict(W=300, Cin=36, N=70, plain=True)),                   # Cin % 32 != 0
    ("plain_4096x128x96", [2, 3, 1, 0], dict(W=4096, Cin=96, N=128, plain=True)),               # K < 128
    ("plain_5x4096x4096", [0, 0, 1, 0], dict(W=5, Cin=4096, N=4096, plain=True)),               # M <= 8: skinny
    ("conv3x3_2048x2_c256", [1, 0, 1, 0], dict(B=2, H=32, W=32, Cin=256, N=2, kh=3, kw=3)),      # N <= 4, M >= 1 024: narrow
    ("plain_65536x128x128", [3, 13, 1, 1], dict(W=65536, Cin=128, N=128, plain=True)),          # 2 048 tiles > 512, 4 steps: walk (not row-streamed: M < 262 144, N < 384)
    ("plain_40000x128x64", [4, 20, 1, 1], dict(W=40000, Cin=64, N=128, plain=True)),            # K = 64, M >= 16 384: row-streaming
    ("plain_19200x64x1024", [3, 13, 2, 0], dict(W=19200, Cin=1024, N=64, plain=True)),          # 300 tiles: the 257..511 rule, K >= 1 024
    ("conv3x3_874x24_c64", [3, 14, 2, 0], dict(B=2, H=19, W=23, Cin=64, N=24, kh=3, kw=3)),      # 128x32: 7 tiles, split 37 capped by K / 256 = 2
    ("plain_1000x24x100", [2, 4, 1, 0], dict(W=1000, Cin=100, N=24, plain=True)),               # N <= 32 without the ring: register-staged 128x32
    ("plain_300x70x1028", [2, 3, 4, 0], dict(W=300, Cin=1028, N=70, plain=True)),               # register-staged: 10 tiles, ceil(512 / 10) = 52 capped by K / 256 = 4
    ("plain_64x64x8192", [3, 13, 16, 0], dict(W=64, Cin=8192, N=64, plain=True)),               # one tile: split 256, K / 256 = 32, capped at 16
    ("plain_512x256x4096", [3, 13, 8, 0], dict(W=512, Cin=4096, N=256, plain=True)),            # 32 tiles: split 8
    ("plain_8192x128x512", [3, 13, 1, 0], dict(W=8192, Cin=512, N=128, plain=True)),            # exactly 256 tiles: neither rule applies
    ("plain_16384x128x128", [3, 13, 1, 0], dict(W=16384, Cin=128, N=128, plain=True)),          # exactly 512 tiles: not more than the slots, no walk
    ("plain_16448x128x128", [3, 13, 1, 1], dict(W=16448, Cin=128, N=128, plain=True)),          # 514 tiles: walk
    ("plain_32768x384x128", [4, 20, 1, 1], dict(W=32768, Cin=128, N=384, plain=True)),          # N >= 384 and M >= 32 768: row-streaming
]


@pytest.mark.parametrize("name,want,shape", AUTO, ids=[a[0] for a in AUTO])
def test_automatic_plan_is_pinned(ops, ws, name, want, shape):
    """tile = 0, split_k = 0 and a workspace: conv_gemm_launch's own choice of family, tile, split and walk as st_gemm_last_plan reports it,
    each run under bar (a) with the split it chose (the kernels that never fold with K in tau) and, for the MFMA kernels, bar (b)."""
    p = Problem(seed=9500 + AUTO.index((name, want, shape)), **shape)
    wide, out, plan, _, _ = p.run(ops, 0, 0, ws)
    torch.cuda.synchronize()
    assert plan == want, (name, plan, want)
    bar_a(f"auto_{name}", out, p.ref, p.S, tau(p.K, plan[2], folds=plan[0] >= 2))
    assert untouched(wide, 1, p.N)
    if plan[0] >= 2:
        _, out3, plan3, _, _ = p.run(ops, 3, plan[2], ws)
        assert plan3[:3] == [2, 3, plan[2]] and torch.equal(out, out3), name
