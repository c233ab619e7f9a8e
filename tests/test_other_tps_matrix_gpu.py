"""tps_other_maps_kernel (csrc/tps_other.hip) past its own branch points: the float32 sum for w_0 above its 128-element block (numpy's
halving recursion on an explicit stack in LDS) and the staging loop past one chunk of 256 centres, through the C-ABI with teacher-forced
weights (no n^3 solve), over _other_tps_ref.N_TABLE = 1 .. 4096 control points; the same entry at the linspace edges (H or W of 1, 63 / 64
/ 65 columns, 3 / 4 / 5 rows); the wrapper behind a real fit at n = 150 and 300, de-duplication past the block included; and the remap at
1, 7 and 64 planes, a 1 x 1 source and a source that drives the sum past both ends of 0..255.

Reference: tests/_other_tps_ref.py (fp64, index order, w_0 as numpy's float32 np.sum).  tests/test_other_tps_cpu.py shows on the CPU what
this file relies on: the restated sum is numpy's on every case used here, each of three wrong sums gives another w_0 (and another probe
value) at every n >= 130 where it is a different sequence of additions, a dropped partial chunk moves most pixels by more than 4 ulps, and
no probe value sits within 2 fp64 ulps of a float32 rounding boundary.

Bars.  Maps: every value within 1 float32 ulp of the restatement (the GPU's fp64 log may differ from the host's in the last place) and the
share of values that differ at all at most 1e-4 -- pooled over the whole table for the teacher-forced matrix (23 x 4810 x 2 values), over
both maps of a case elsewhere.  The w_0 probe and the remap: bit for bit.  Every operand sits inside a NaN frame; both map frames must be
untouched outside their views."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _other_tps_ref as R  # noqa: E402
from _measure import check  # noqa: E402
from test_geom_matrix_gpu import _release_frames, frame, frame_intact, ops, put, st  # noqa: E402,F401
from test_other_tps_gpu import _adversarial_maps, _planes, _remap_both, table, ulps  # noqa: E402,F401

CANVAS = (37, 130)                  # 3 block columns of 64 (the last with 2 live lanes), 10 block rows of 4 (the last with 1 live row)
DIFFERS_CAP = 1e-4                  # the bar of test_other_tps_gpu.test_maps_match_the_restatement


def launch_maps(st, kw, aw, centres, H, W):
    """st_tps_other_maps on framed operands -> (mapx, mapy) numpy; asserts both output frames intact"""
    n = centres.shape[0]
    fx, fy = frame((H, W)), frame((H, W))
    ins = [put(torch.from_numpy(np.ascontiguousarray(a))) for a in (centres, kw, aw)]
    st.check(st.lib.st_tps_other_maps(st.p(ins[0]), st.p(ins[1]), st.p(ins[2]), n, H, W, st.p(fx[1]), st.p(fy[1]), st.stream()),
             "st_tps_other_maps")
    torch.cuda.synchronize()
    assert frame_intact(*fx) and frame_intact(*fy), f"n = {n}, {H} x {W}: a write outside the map"
    return fx[1].cpu().numpy(), fy[1].cpu().numpy()


def map_ulps(got, ref):
    """[2, H, W] distances in float32 ulps; a NaN or an unwritten value counts as far off"""
    g, r = np.stack(got), np.stack(ref)
    assert np.isfinite(r).all()
    return np.where(np.isfinite(g), ulps(np.where(np.isfinite(g), g, 0).astype(np.float32), r), 1 << 40)


# ================================================================================================ B. the C entry, teacher-forced
@pytest.fixture(scope="module")
def matrix(st):
    """every n of the table once: the 37 x 130 maps and the 1 x 1 probe, GPU and restatement -> {n: (ulps [2,37,130], probe got, want)}"""
    out = {}
    for n in R.N_TABLE:
        kw, aw, centres = R.case(n)
        u = map_ulps(launch_maps(st, kw, aw, centres, *CANVAS), R.maps(kw, aw, centres, *CANVAS))
        pk, pa, pc = R.probe_case(n)
        got = np.stack(launch_maps(st, pk, pa, pc, 1, 1)).reshape(2)
        want = np.stack(R.maps(pk, pa, pc, 1, 1)).reshape(2)
        out[n] = (u, got, want)
    return out


@pytest.mark.parametrize("n", R.N_TABLE)
def test_maps_matrix_within_one_ulp(matrix, n):
    u = matrix[n][0]
    print(f"[n = {n}] 37 x 130 maps: ulps max {u.max()}, differ at {int((u != 0).sum())} of {u.size}")
    check(f"other_maps_matrix_n{n}_max_ulps", u.max(), 1, inclusive=True)


def test_maps_matrix_differs_frac(matrix):
    """pooled over the table: 23 x 4810 x 2 = 221260 values, of which the cap lets 22 differ"""
    assert sorted(matrix) == sorted(R.N_TABLE)
    differs = sum(int((matrix[n][0] != 0).sum()) for n in R.N_TABLE)
    total = sum(matrix[n][0].size for n in R.N_TABLE)
    print(f"[table] {differs} of {total} map values differ from the restatement")
    check("other_maps_matrix_differs_frac", differs / total, DIFFERS_CAP, inclusive=True)


@pytest.mark.parametrize("n", R.N_TABLE)
def test_w0_probe_bit_equal(matrix, n):
    """float32(U(3) * w_0[axis]) and nothing else: w_0 itself, to the bit (n = 1: the empty sum, w_0 = -0.0, maps +0.0)"""
    _, got, want = matrix[n]
    assert got.tobytes() == want.tobytes(), (n, got, want)


@pytest.mark.parametrize("hw", [(1, 1), (1, 65), (5, 1), (3, 63), (4, 64), (5, 65)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_maps_shape_edges(st, hw):
    """n = 300 (two chunks, three levels of the sum) at the linspace special cases: W == 1, H == 1, the last sample exactly 1"""
    H, W = hw
    kw, aw, centres = R.case(300)
    u = map_ulps(launch_maps(st, kw, aw, centres, H, W), R.maps(kw, aw, centres, H, W))
    print(f"[{H} x {W}] ulps max {u.max()}, differ at {int((u != 0).sum())} of {u.size}")
    assert u.max() <= 1
    assert np.mean(u != 0) <= DIFFERS_CAP              # fewer than 10^4 values: none may differ


# ================================================================================================ C. the wrapper behind a real fit
FIT_HW = (200, 260)


def fit_points(n, dup=0):
    """n pixel points on a 200 x 260 canvas: a jittered grid (cells of at least 13 px, jitter within the middle half of a cell, so any two
    points are at least half a cell apart), sources 1.5 px of noise away; dup: that many points take the destination of another"""
    H, W = FIT_HW
    rows, cols = {150: (10, 15), 300: (15, 20)}[n]
    rng = np.random.default_rng(9000 + n + dup)
    ch, cw = H / rows, W / cols
    gy, gx = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    dst = np.stack([(gx.ravel() + 0.5 + rng.uniform(-0.25, 0.25, n)) * cw, (gy.ravel() + 0.5 + rng.uniform(-0.25, 0.25, n)) * ch], 1)
    dst = dst[rng.permutation(n)].astype(np.float32)
    src = (dst + rng.normal(0, 1.5, dst.shape)).astype(np.float32)
    if dup:
        pick = rng.choice(n, 2 * dup, replace=False)
        dst[pick[:dup]] = dst[pick[dup:]]              # `dup` sites now occur twice, with different sources
    return R.normalise(src, H, W), R.normalise(dst, H, W)


@pytest.mark.parametrize("n,dup", [(150, 0), (300, 0), (150, 6)], ids=["n150", "n300", "n150_dup6"])
def test_wrapper_fit_and_maps_past_the_block(ops, n, dup):
    """ops.tps_other_maps without weights: the fit, then the maps on the large-n branches; against the restatement teacher-forced on
    the GPU's own theta.  The gap of theta to numpy's fp64 solve is printed, not bounded (the solve has its own bar in
    tests/test_post_matrix_gpu.py).  With 6 coincident sites the wrapper must fit the 144 first occurrences."""
    H, W = FIT_HW
    c_src, c_dst = fit_points(n, dup)
    assert len(c_dst) == n
    mx, my = ops.tps_other_maps(torch.from_numpy(c_src).cuda(), torch.from_numpy(c_dst).cuda(), H, W)
    k_src, k_dst = R.dedup_first(c_src, c_dst)
    assert len(k_dst) == n - dup and len(np.unique(k_dst, axis=0)) == n - dup
    kw, aw = (t.cpu().numpy() for t in ops.tps_other_solve(torch.from_numpy(k_src).cuda(), torch.from_numpy(k_dst).cuda()))
    assert kw.shape == (n - dup, 2)
    rk, ra = R.fit(k_src, k_dst)
    gap = max(np.abs(rk[1:] - kw[1:]).max(), np.abs(ra - aw).max()) / np.abs(rk).max()
    u = map_ulps((mx.cpu().numpy(), my.cpu().numpy()), R.maps(kw, aw, k_dst, H, W))
    tag = f"n{n}" + (f"_dup{dup}" if dup else "")
    print(f"[{tag} {H}x{W}] ulps max {u.max()}, differ at {int((u != 0).sum())} of {u.size}; theta vs numpy fp64 solve {gap:.2e} of max |kw|")
    assert u.max() <= 1
    check(f"other_maps_matrix_fit_{tag}_differs_frac", np.mean(u != 0), DIFFERS_CAP, inclusive=True)


# ================================================================================================ D. remap corners
@pytest.mark.parametrize("P", [1, 7, 64])
def test_remap_bit_exact_plane_counts(ops, table, P):
    """one plane, an odd count and the accepted maximum: source 9 x 11, output 6 x 70 (two block columns, two block rows)"""
    rng = np.random.default_rng(300 + P)
    planes = _planes(P, 9, 11, rng)
    mx, my = _adversarial_maps(6, 70, rng, 9, 11)
    got, ref = _remap_both(ops, planes, mx, my, table)
    assert got.shape == (P, 6, 70) and np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    assert (got > 0).any() and (got == 0).any()


def test_remap_bit_exact_one_pixel_source(ops, table):
    rng = np.random.default_rng(311)
    planes = _planes(6, 1, 1, rng)
    planes[0] = 255.0
    mx, my = _adversarial_maps(5, 65, rng, 1, 1)
    mx[2, :8] = np.float32([0, -0.5, 0.5, 1, -1, 2, -2, 0.25])            # every tap column that can hold the one pixel, and none
    my[2, :8] = np.float32([0, 0.5, -0.5, 0, 1, 0, 0, 2])
    got, ref = _remap_both(ops, planes, mx, my, table)
    assert got.shape == (6, 5, 65) and np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    assert got[0, 2, 0] == 255 and (got[0] > 0).sum() >= 6


def test_remap_saturates_on_a_checkerboard(ops, table):
    """0 / 255 squares of 2 x 2 pixels sampled at half-pixel positions: the taps (-3, 19, 19, -3) / 32 over (0, 255, 255, 0) give
    1.1875 x 255, over (255, 0, 0, 255) give -0.1875 x 255, so the sum leaves 0..255 on both sides and the clamp decides the byte.
    (Squares of one pixel cannot show it: there the half-pixel taps over alternating values sum to exactly 127.5.)"""
    Hs, Ws = 12, 14
    yy, xx = np.meshgrid(np.arange(Hs), np.arange(Ws), indexing="ij")
    board = (255.0 * (((yy // 2) + (xx // 2)) % 2)).astype(np.float32)
    planes = np.stack([board, 255.0 - board])
    H, W = Hs + 2, 70
    my, mx = np.meshgrid(np.arange(H, dtype=np.float32) - 0.5, (np.arange(W, dtype=np.float32) % (Ws + 2)) - 0.5, indexing="ij")
    mx, my = np.ascontiguousarray(mx), np.ascontiguousarray(my)
    raw = R.remap_cubic(R.quantise(planes), mx, my, table, saturate=False)
    assert (raw < 0).sum() >= 50 and (raw > 255).sum() >= 50, (raw.min(), raw.max())
    got, ref = _remap_both(ops, planes, mx, my, table)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    assert np.array_equal(got, np.clip(raw, 0, 255).astype(np.float32)) and got.min() == 0 and got.max() == 255
