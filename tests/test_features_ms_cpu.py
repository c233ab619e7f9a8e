"""The CPU restatement of csrc/features_ms.hip (tests/_features_ms_ref.py) against plain scalar Python loops, its accuracy on procedural scenes
rotated and zoomed beyond what feature_align finds, the degenerate inputs, planted defects that must each fail one of those assertions, the C
entries' rejections and the compiler's resource report of csrc/features_ms.hip."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import _features_ms_ref as ms
import _features_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "seamless-through-breaking-rethinking-image-stitching-for-optimal-alignment_amd")
NONE = frozenset()
SIZES = ((64, 64), (80, 80), (100, 125))


def _img(h, w, seed=1):
    return ref.small_pair(h, w, seed)[0][0]


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------------
def test_level_sizes_and_slots_of_the_contract():
    assert ms.level_sizes(64, 64, 6) == [(64, 64)] and ms.level_sizes(79, 64, 6) == [(79, 64)] and ms.level_sizes(64, 80, 6) == [(64, 80)]
    assert ms.level_sizes(80, 80, 6) == [(80, 80), (64, 64)] and ms.level_sizes(80, 80, 1) == [(80, 80)]
    assert len(ms.level_sizes(100, 125, 6)) == 3
    assert len(ms.level_sizes(512, 512, 8)) == 8 and ms.level_sizes(512, 512, 8)[-1] == (105, 105) and len(ms.level_sizes(512, 512, 6)) == 6
    assert len(ms.level_sizes(1024, 1024, 8)) == 8 and ms.level_sizes(1024, 1024, 8)[-1] == (214, 214)
    want = {(64, 64, 6): 16, (80, 80, 6): 52, (100, 125, 6): 136, (192, 256, 6): 556, (512, 512, 6): 2848, (1024, 1024, 8): 11508, (640, 640, 6): 4304, (640, 640, 8): 4548}
    for (h, w, lv), n in want.items():
        assert ms.slots(h, w, lv) == n == sum(4 * -(-a // 32) * -(-b // 32) for a, b in ms.level_sizes(h, w, lv)), (h, w, lv)
    assert max(ms.slots(1024, 1024, lv) for lv in range(1, 9)) == 11508 < 32768          # the 16-bit slot field of the match


# ---- the stages against loops ------------------------------------------------------------------------------------------------------------------
def check_pyramid(defects=NONE):
    """every pixel of every level, the last row and column among them; the slot -> level map"""
    fxs = set()
    for h, w in SIZES:
        pyr = ms.pyramid(_img(h, w), 6, defects)
        assert [p.shape for p in pyr] == ms.level_sizes(h, w, 6) and np.array_equal(pyr[0], ref.luma(_img(h, w)))
        for src, dst in zip(pyr, pyr[1:]):
            Hs, Ws = src.shape
            assert dst.shape == (4 * Hs // 5, 4 * Ws // 5)
            for i in range(dst.shape[0]):
                for j in range(dst.shape[1]):
                    sx, sy = 160 * (2 * j + 1) - 128, 160 * (2 * i + 1) - 128
                    x0, fx, y0, fy = sx >> 8, sx & 255, sy >> 8, sy & 255
                    x1, y1 = min(x0 + 1, Ws - 1), min(y0 + 1, Hs - 1)
                    a, b, c, d = int(src[y0, x0]), int(src[y0, x1]), int(src[y1, x0]), int(src[y1, x1])
                    assert dst[i, j] == ((256 - fx) * (256 - fy) * a + fx * (256 - fy) * b + (256 - fx) * fy * c + fx * fy * d + (1 << 15)) >> 16, (i, j)
                    fxs.add(fx)
            assert 0 <= dst.min() and dst.max() <= 255
        levels = ms.slot_levels(h, w, 6)
        at = 0
        for l, (a, b) in enumerate(ms.level_sizes(h, w, 6)):
            for _ in range(ref.slots(a, b)):
                assert levels[at] == l
                at += 1
        assert at == len(levels) == ms.slots(h, w, 6)
    assert fxs == {32, 96, 160, 224}                           # 320 j + 32 mod 256: a centre-aligned x 5/4 sample never falls on a pixel (fx = 0)
    flat = np.full((70, 90), 131, np.int64)
    assert (ms.downsample(flat) == 131).all()                   # the weights sum to 2^16
    ramp = np.tile(np.arange(90, dtype=np.int64) * 2, (70, 1))
    assert ms.downsample(ramp)[0, 0] == 0 and ms.downsample(ramp)[0, -1] == (2 * (320 * 71 + 32) + 128) >> 8      # position j 5/4 + 1/8 of a ramp


def _candidates_loop(R, border):
    H, W = R.shape
    out = np.zeros((H, W), bool)
    for y in range(border, H - border):
        for x in range(border, W - border):
            r = R[y, x]
            ok = r > 0
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dy or dx:
                        q = R[y + dy, x + dx]
                        ok = ok and (r > q if (dy < 0 or (dy == 0 and dx < 0)) else r >= q)
            out[y, x] = ok
    return out


def _select_loop(R, cand):
    H, W = R.shape
    CW = -(-W // 32)
    kp = np.full((4 * -(-H // 32) * CW, 2), -1, np.int32)
    for cy in range(-(-H // 32)):
        for cx in range(CW):
            found = [(-int(R[y, x]), y * W + x) for y in range(32 * cy, min(32 * cy + 32, H)) for x in range(32 * cx, min(32 * cx + 32, W)) if cand[y, x]]
            for rank, (_, idx) in enumerate(sorted(found)[:4]):
                kp[4 * (cy * CW + cx) + rank] = idx % W, idx // W
    return kp


def check_corners_and_border(defects=NONE):
    """the corners of every level against loops with the border at 20: x = 19 and x = W - 20 are out, x = 20 and x = W - 21 are in"""
    band = False
    for h, w in SIZES:
        for Y in ms.pyramid(_img(h, w), 6):
            R = ref.harris(Y)
            kp, _, box = ms.detect_level(Y, True, defects)
            assert np.array_equal(kp, _select_loop(R, _candidates_loop(R, 20)))
            v = kp[kp[:, 0] >= 0]
            assert (v[:, 0] >= 20).all() and (v[:, 0] <= Y.shape[1] - 21).all() and (v[:, 1] >= 20).all() and (v[:, 1] <= Y.shape[0] - 21).all()
            assert np.array_equal(box, ref.window_sum(Y, 2))
            band = band or bool((ms.candidates(R, 16) & ~ms.candidates(R, 20)).any())
    assert band                                                 # (the scenes do have corners between 16 and 19 px from an edge)
    R = np.full((64, 90), -5, np.int64)
    for y, x in ((19, 40), (20, 44), (43, 48), (44, 52), (30, 19), (32, 20), (34, 69), (36, 70)):
        R[y, x] = 900 + x
    got = np.argwhere(ms.candidates(R, 16 if "border_16" in defects else ms.BORDER))
    assert got.tolist() == [[20, 44], [32, 20], [34, 69], [43, 48]]


def _bin_scalar(m10, m01):
    t = ms.cs_table()
    best, at = None, 0
    for b in range(32):
        v = int(m10) * int(t[b, 0]) + int(m01) * int(t[b, 1])
        if best is None or v > best:
            best, at = v, b
    return at


def check_moments_and_bins(defects=NONE):
    t = ms.cs_table()
    assert [int(v) for v in t[:9, 0]] == list(ms.QUARTER) and [int(v) for v in t[:9, 1]] == list(ms.QUARTER[::-1])
    for b in range(32):                                         # a quarter turn further: (c, s) -> (-s, c); the angle grows counter-clockwise in (x, y)
        assert tuple(t[(b + 8) % 32]) == (-t[b, 1], t[b, 0]) and abs(np.degrees(np.arctan2(t[b, 1], t[b, 0])) % 360 - 11.25 * b) < 0.06
    d = ms.disc()
    assert len(d) == 709 and (d ** 2).sum(1).max() == 225 and len({tuple(r) for r in d.tolist()}) == 709
    for h, w in SIZES:
        for Y in ms.pyramid(_img(h, w), 6):
            kp, bins, _ = ms.detect_level(Y, True, defects)
            m10, m01 = ms.moments(Y, kp)
            assert (kp[:, 0] >= 0).sum() >= 4
            for i, (x, y) in enumerate(kp.tolist()):
                a = b = 0
                if x >= 0:
                    for dy in range(-15, 16):
                        for dx in range(-15, 16):
                            if dx * dx + dy * dy <= 225:
                                a += dx * int(Y[y + dy, x + dx])
                                b += dy * int(Y[y + dy, x + dx])
                assert (m10[i], m01[i]) == (a, b)
                assert bins[i] == (_bin_scalar(a, b) if x >= 0 else 0), (i, a, b)
            assert not ms.detect_level(Y, False, defects)[1].any()
    # planted: the flat patch, vectors exactly between two bins (equal products: the lower bin), the bins themselves, random ones
    rng = np.random.default_rng(5)
    vec, ties = [(0, 0)], 0
    for b in range(32):
        n = (b + 1) % 32
        dx, dy = int(t[n, 0] - t[b, 0]), int(t[n, 1] - t[b, 1])
        mid = (-dy * 7, dx * 7) if -dy * int(t[b, 0]) + dx * int(t[b, 1]) > 0 else (dy * 7, -dx * 7)
        vec += [mid, (int(t[b, 0]) * 3, int(t[b, 1]) * 3)]
        prod = [mid[0] * int(c) + mid[1] * int(s) for c, s in t]
        ties += prod[b] == prod[n] == max(prod)
    assert ties == 32
    vec += [tuple(v) for v in rng.integers(-2700000, 2700000, (200, 2)).tolist()]
    got = ms.bins_of(np.array([v[0] for v in vec]), np.array([v[1] for v in vec]), defects)
    assert got.dtype == np.uint8 and got.tolist() == [_bin_scalar(*v) for v in vec]
    assert got[0] == 0 and got[1:65:2].tolist() == [min(b, (b + 1) % 32) for b in range(32)] and got[2:66:2].tolist() == list(range(32))


def check_steering_and_descriptor(defects=NONE):
    """the steered offsets of all 32 bins against Python integers, none beyond 17; the bits of every slot from the box sums of its own level"""
    pat = ref.brief_pattern().astype(np.int64)
    t = ms.cs_table()
    o = ms.steered(np.arange(32), defects)
    for b in range(32):
        c, s = int(t[b, 0]), int(t[b, 1])
        for k in range(256):
            for e in (0, 2):
                px, py = int(pat[k, e]), int(pat[k, e + 1])
                assert (o[b, k, e], o[b, k, e + 1]) == ((px * c - py * s + 512) >> 10, (px * s + py * c + 512) >> 10), (b, k)
    assert np.abs(o).max() <= 17 and np.array_equal(o[0], pat)                   # bin 0 is the identity
    assert np.array_equal(o[16], -pat) and np.array_equal(o[8][:, 0], -pat[:, 1]) and np.array_equal(o[8][:, 1], pat[:, 0])
    h, w = 100, 125
    f = ms.features(_img(h, w), 6, True, defects)
    levels, start = ms.slot_levels(h, w, 6), ms.slot_starts(h, w, 6)
    assert len(f["box"]) == 3 and levels.max() == 2
    for slot, (x, y) in enumerate(f["kp"].tolist()):
        box, words = f["box"][levels[slot]], [0] * 8
        if x >= 0:
            off = ms.steered(f["bins"][slot:slot + 1])[0]
            for k in range(256):
                if box[y + off[k, 1], x + off[k, 0]] < box[y + off[k, 3], x + off[k, 2]]:
                    words[k >> 5] |= 1 << (k & 31)
        assert f["desc"][slot].tolist() == words, slot
    assert all((f["kp"][start[l]:start[l + 1], 0] >= 0).sum() >= 4 for l in range(3))


def check_level0_coordinates(defects=NONE):
    for h, w in SIZES:
        kp = ms.features(_img(h, w), 6)["kp"]
        xy, levels = ms.level0(kp, h, w, 6, defects), ms.slot_levels(h, w, 6)
        for slot, (x, y) in enumerate(kp.tolist()):
            l = int(levels[slot])
            for got, v in ((xy[slot, 0], x), (xy[slot, 1], y)):
                want = Fraction((2 * v + 1) * 5 ** l, 2 * 4 ** l) - Fraction(1, 2) if x >= 0 else Fraction(-1)
                assert Fraction(float(got)) == want, (slot, l, v)
    far = ms.level0(np.array([[1023, 1023]] * 11508, np.int32), 1024, 1024, 8)[-1]
    assert Fraction(float(far[0])) == Fraction(2047 * 5 ** 7, 2 * 4 ** 7) - Fraction(1, 2)          # exact at the largest level and coordinate too


CHECKS = (check_pyramid, check_corners_and_border, check_moments_and_bins, check_steering_and_descriptor, check_level0_coordinates)


@pytest.mark.parametrize("check", CHECKS, ids=lambda c: c.__name__)
def test_restatement_against_loops(check):
    check(NONE)


@pytest.mark.parametrize("defect", ms.DEFECTS)
def test_planted_defects_are_noticed(defect):
    failed = None
    for check in CHECKS[::-1]:                                  # (the quick checks first)
        try:
            check(frozenset({defect}))
        except AssertionError:
            failed = check.__name__
            break
    assert failed, f"no assertion notices {defect}"
    print(f"{defect}: noticed by {failed}")


def test_one_upright_level_is_feature_align_with_border_20(monkeypatch):
    a, b = ref.small_pair(96, 130)
    got = ms.homography(a, b, levels=1, oriented=False)
    assert not np.array_equal(got["kp1"], ref.homography(a, b)["kp1"])                   # (the border does matter on this pair)
    monkeypatch.setattr(ref, "BORDER", 20)
    want = ref.homography(a, b)
    for k in ("kp1", "kp2", "desc1", "desc2", "nn", "matches", "count", "mask", "info", "H", "motion"):
        assert np.array_equal(got[k], want[k]), k
    assert want["info"][0, 0] == 1 and not got["bins1"].any() and np.array_equal(got["xy"][0], np.where(got["kp1"] >= 0, got["kp1"], -1).astype(np.float64))


# ---- accuracy ----------------------------------------------------------------------------------------------------------------------------------
# (h, w, motion = (tx, ty, rotation, px, py[, scale]), inliers and corner error measured with this restatement on scene seed 3: README.md,
# feature_align_ms, accuracy table).  The margins are those of test_features_cpu.py: 3 x the measured error covers the spread over scene
# seeds (0.33 .. 0.99 px at one motion), half the measured inliers likewise.
MEASURED = [(512, 512, (80, 10, 0, 0, 0), 1081, 0.242), (512, 512, (100, 20, 15, 0, 0), 830, 0.205), (512, 512, (40, 10, 30, 0, 0), 697, 0.458),
            (512, 512, (20, 10, 45, 1e-4, 0), 572, 0.754), (512, 512, (30, -20, 90, 0, 0), 1082, 0.157), (512, 512, (40, 20, 180, 1e-4, -5e-5), 981, 0.191),
            (512, 512, (40, 0, 0, 0, 0, 1.25), 678, 0.104), (512, 512, (30, 10, 10, 0, 0, 1.5), 314, 0.535), (512, 512, (30, 10, -20, 0, 0, 0.667), 288, 1.142),
            (512, 512, (10, 10, 0, 0, 0, 2.0), 175, 0.626),
            (192, 256, (10, 5, 90, 0, 0), 124, 0.486), (192, 256, (10, 5, 40, 0, 0), 101, 1.540), (192, 256, (10, 5, 180, 0, 0), 195, 0.312),
            (192, 256, (10, 5, 10, 0, 0, 1.5), 42, 0.742), (192, 256, (10, 5, -25, 0, 0, 1.3), 70, 1.413)]
NEEDS_THE_FEATURE = ((30, -20, 90, 0, 0), (30, 10, 10, 0, 0, 1.5))


@pytest.mark.parametrize("row", MEASURED, ids=lambda r: f"{r[0]}x{r[1]}_rot{r[2][2]}_x{r[2][5] if len(r[2]) > 5 else 1}")
def test_accuracy_and_direction_on_rotated_and_zoomed_pairs(row):
    h, w, motion, inliers, error = row
    a, b, Hgt = ref.pair(h, w, motion, 3)
    res = ms.homography(a, b)
    info, Hf = res["info"][0], res["H"][0].astype(np.float64)
    err = ref.corner_error(Hf, Hgt, h, w)
    print(f"{h}x{w} {motion}: keypoints {info[1]} / {info[2]}, matches {info[3]}, inliers {info[5]}, corner error {err:.3f} px")
    assert info[0] == 1
    assert err < 3 * error and info[5] >= inliers / 2
    if motion in NEEDS_THE_FEATURE:                             # feature_align's own contract finds no model here
        old = ref.homography(a, b)["info"][0]
        print(f"    feature_align: matches {old[3]}, inliers {old[5]}, valid {old[0]}")
        assert old[0] == 0
    # the direction: image 2 resampled through H lands on image 1
    g1, g2 = a[0, 0].astype(np.float64), b[0, 0].astype(np.float64)
    warped = ref.resample(g2, Hf, h, w)
    inside = ref.resample(np.ones_like(g2), Hf, h, w) > 0.999
    adj = lambda g: (g - 10.0) / 0.85                                                     # noqa: E731  (the known gain and bias of image 2)
    print(f"    overlap {inside.mean():.2f}, mean |difference| warped {np.abs(adj(warped) - g1)[inside].mean():.2f}, unwarped {np.abs(adj(g2) - g1)[inside].mean():.2f}")
    assert inside.mean() > 0.3
    assert np.abs(adj(warped) - g1)[inside].mean() < np.abs(adj(g2) - g1)[inside].mean() / 3


# ---- degenerate images ---------------------------------------------------------------------------------------------------------------------------
def test_degenerate_images_and_their_info():
    res = {n: ms.homography(*ref.degenerate(n)) for n in ref.DEGENERATE}
    info = {n: r["info"][0].tolist() for n, r in res.items()}
    print(info)
    c = res["constant"]
    assert info["constant"] == [0, 0, 0, 0, -1, 0, 0, 0] and (c["kp1"] == -1).all() and not c["desc1"].any() and not c["bins1"].any() and (c["xy"] == -1).all()
    assert len(c["pyr1"]) == 2 and all((p == c["pyr1"][0][0, 0, 0]).all() for p in c["pyr1"])
    i = info["identical"]
    assert i[0] == 1 and i[1] == i[2] == i[3] == i[5] > 12 and np.abs(res["identical"]["H"][0].astype(np.float64) - np.eye(3)).max() < 1e-9
    assert np.abs(res["identical"]["motion"]).max() < 1e-9 and np.array_equal(res["identical"]["bins1"], res["identical"]["bins2"])
    assert info["unrelated"][0] == 0 and info["unrelated"][3] < 8 and info["unrelated"][4] == -1 and info["unrelated"][1] > 20
    assert np.array_equal(res["unrelated"]["H"][0], np.eye(3, dtype=np.float32)) and not res["unrelated"]["motion"].any()
    assert info["checker"][0] == 0 and info["checker"][3] < 8 and info["checker"][1] == info["checker"][2] > 20
    assert info["nonfinite"][1] > 20 and info["nonfinite"][3] >= 8


# ---- entries and binary ------------------------------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_touching_the_gpu():
    from stitch_amd._lib import lib
    base = 0x7f0000000000                                                   # never dereferenced on the host
    P = [base + (i << 32) for i in range(12)]
    B, H, W, lv, hyp = 2, 81, 100, 6, 100
    N = lib.st_feature_ms_slots(H, W, lv)
    sizes = (C.c_int32 * 16)()
    assert lib.st_feature_ms_level_sizes(H, W, lv, C.cast(sizes, C.c_void_p)) == 2 and list(sizes) == [81, 100, 64, 80] + [0] * 12
    assert lib.st_feature_ms_level_sizes(H, W, lv, None) == 2 and lib.st_feature_ms_level_sizes(H, W, 1, None) == 1
    for h, w, l in ((64, 64, 6), (79, 64, 6), (80, 80, 6), (100, 125, 6), (192, 256, 6), (512, 512, 6), (512, 512, 8), (640, 640, 8), (1024, 1024, 8), (1024, 64, 3)):
        assert lib.st_feature_ms_slots(h, w, l) == ms.slots(h, w, l) and lib.st_feature_ms_level_sizes(h, w, l, None) == len(ms.level_sizes(h, w, l)), (h, w, l)
    assert N == ms.slots(H, W, lv) == 72
    for bad in ((63, 64, 6), (64, 1025, 6), (64, 64, 0), (64, 64, 9)):
        assert lib.st_feature_ms_slots(*bad) == 0 and lib.st_feature_ms_level_sizes(*bad, None) == 0, bad
    wsb = lib.st_feature_ms_workspace_bytes
    need = wsb(B, H, W, lv, hyp)
    assert need > 0 and need % 16 == 0 and wsb(B, H, W, lv, hyp + 8) > need > wsb(B, H, W, 1, hyp) and 0 < wsb(64, 1024, 1024, 8, 65536) < 2 ** 31
    for bad in ((0, H, W, lv, hyp), (65, H, W, lv, hyp), (B, 63, W, lv, hyp), (B, H, 63, lv, hyp), (B, 1025, W, lv, hyp), (B, H, 1025, lv, hyp), (B, H, W, lv, 0),
                (B, H, W, lv, 65537), (-1, H, W, lv, hyp), (B, H, W, 0, hyp), (B, H, W, 9, hyp)):
        assert wsb(*bad) == 0, bad
    off = (C.c_int64 * 13)()
    assert lib.st_feature_ms_workspace_layout(B, H, W, lv, hyp, C.cast(off, C.c_void_p)) == 0 and off[12] == need and list(off) == sorted(off) and off[0] == 0
    assert all(o % 16 == 0 for o in off)
    assert lib.st_feature_ms_workspace_layout(B, H, W, lv, hyp, None) == 1001 and lib.st_feature_ms_workspace_layout(B, 63, W, lv, hyp, C.cast(off, C.c_void_p)) == 1001
    px, pl, bn, big = B * H * W, B * (81 * 100 + 64 * 80), B * N, 1 << 40
    nan, inf = float("nan"), float("inf")

    def sweep(call, regions, outputs, shape_args):
        """nulls, shapes, and every output against every other operand: overlapping at its first and last byte"""
        for name in regions:
            assert call(**{name: None}) == 1001, name
        for kw in shape_args:
            assert call(**kw) == 1001, kw
        for a in outputs:
            for b in regions:
                if a != b:
                    pa, pb = regions[a], regions[b]
                    assert call(**{a: pb[0]}) == 1001 and call(**{a: pb[0] + pb[1] - 1}) == 1001 and call(**{a: pb[0] - pa[1] + 1}) == 1001, (a, b)

    shapes = [dict(B=0), dict(B=65), dict(H=63), dict(W=63), dict(H=1025), dict(W=1025), dict(B=-1), dict(levels=0), dict(levels=9), dict(levels=-1)]
    params = [dict(max_hyp=0), dict(max_hyp=65537), dict(thr=0.0), dict(thr=-1.0), dict(thr=nan), dict(thr=inf), dict(thr=-inf), dict(min_inliers=-1)]
    clean_shape = (2, 81, 100, 6)

    # (a call that passes every check would launch: each sweep therefore keeps one argument bad -- a stream is never needed)
    def pyramid(img=P[0], pyr=P[1], B=B, H=H, W=W, levels=lv):
        return lib.st_feature_ms_pyramid(img, 0 if (img, pyr, B, H, W, levels) == (P[0], P[1], *clean_shape) else B, H, W, levels, pyr, None)
    sweep(pyramid, dict(img=(P[0], 12 * px), pyr=(P[1], pl)), ("pyr",), shapes)

    def detect(pyr=P[0], kp=P[1], bins=P[2], box=P[3], B=B, H=H, W=W, levels=lv, oriented=1):
        clean = (pyr, kp, bins, box, B, H, W, levels, oriented) == (*P[:4], *clean_shape, 1)
        return lib.st_feature_ms_detect(pyr, 0 if clean else B, H, W, levels, oriented, kp, bins, box, None)
    sweep(detect, dict(pyr=(P[0], pl), kp=(P[1], 8 * bn), bins=(P[2], bn), box=(P[3], 2 * pl)), ("kp", "bins", "box"), shapes + [dict(oriented=2), dict(oriented=-1)])

    def describe(box=P[0], kp=P[1], bins=P[2], desc=P[3], B=B, H=H, W=W, levels=lv):
        clean = (box, kp, bins, desc, B, H, W, levels) == (*P[:4], *clean_shape)
        return lib.st_feature_ms_describe(box, kp, bins, 0 if clean else B, H, W, levels, desc, None)
    sweep(describe, dict(box=(P[0], 2 * pl), kp=(P[1], 8 * bn), bins=(P[2], bn), desc=(P[3], 32 * bn)), ("desc",), shapes)

    def match(kp1=P[0], desc1=P[1], kp2=P[2], desc2=P[3], nn=P[4], matches=P[5], count=P[6], B=B, H=H, W=W, levels=lv):
        clean = (kp1, desc1, kp2, desc2, nn, matches, count, B, H, W, levels) == (*P[:7], *clean_shape)
        return lib.st_feature_ms_match(kp1, desc1, kp2, desc2, 0 if clean else B, H, W, levels, nn, matches, count, None)
    sweep(match, dict(kp1=(P[0], 8 * bn), desc1=(P[1], 32 * bn), kp2=(P[2], 8 * bn), desc2=(P[3], 32 * bn), nn=(P[4], 24 * bn), matches=(P[5], 8 * bn),
                      count=(P[6], 4 * B)), ("nn", "matches", "count"), shapes)

    rneed = 32 * bn + 4 * B * hyp

    def ransac(kp1=P[0], kp2=P[1], matches=P[2], count=P[3], motion=P[4], Hm=P[5], info=P[6], mask=P[7], xy=P[8], ws=P[9], B=B, H=H, W=W, levels=lv, max_hyp=hyp, thr=3.0,
               min_inliers=12, nbytes=rneed):
        clean = (kp1, kp2, matches, count, motion, Hm, info, mask, xy, ws, B, H, W, levels, max_hyp, thr, min_inliers, nbytes) == (*P[:10], *clean_shape, hyp, 3.0, 12, rneed)
        return lib.st_feature_ms_ransac(kp1, kp2, matches, count, 0 if clean else B, H, W, levels, max_hyp, thr, min_inliers, 1, motion, Hm, info, mask, xy, ws, nbytes, None)
    sweep(ransac, dict(kp1=(P[0], 8 * bn), kp2=(P[1], 8 * bn), matches=(P[2], 8 * bn), count=(P[3], 4 * B), motion=(P[4], 32 * B), Hm=(P[5], 36 * B), info=(P[6], 32 * B),
                       mask=(P[7], bn), xy=(P[8], 32 * bn), ws=(P[9], rneed)), ("motion", "Hm", "info", "mask", "xy", "ws"),
          shapes[:7] + [dict(levels=0), dict(levels=9)] + params + [dict(nbytes=rneed - 1), dict(nbytes=0), dict(ws=P[9] + 8), dict(max_hyp=hyp + 1),
                                                                      dict(H=H + 32, nbytes=rneed)])

    def homography(img1=P[0], img2=P[1], motion=P[2], Hm=P[3], info=P[4], ws=P[5], B=B, H=H, W=W, levels=lv, oriented=1, max_hyp=hyp, thr=3.0, min_inliers=12,
                   nbytes=need):
        clean = (img1, img2, motion, Hm, info, ws, B, H, W, levels, oriented, max_hyp, thr, min_inliers, nbytes) == (*P[:6], *clean_shape, 1, hyp, 3.0, 12, need)
        return lib.st_feature_ms_homography(img1, img2, 0 if clean else B, H, W, levels, oriented, max_hyp, thr, min_inliers, 1, motion, Hm, info, ws, nbytes, None)
    sweep(homography, dict(img1=(P[0], 12 * px), img2=(P[1], 12 * px), motion=(P[2], 32 * B), Hm=(P[3], 36 * B), info=(P[4], 32 * B), ws=(P[5], need)),
          ("motion", "Hm", "info", "ws"),
          shapes + params + [dict(oriented=2), dict(oriented=-1), dict(nbytes=need - 1), dict(nbytes=0), dict(ws=P[5] + 8), dict(max_hyp=hyp + 8), dict(H=H + 32),
                             dict(B=B + 1), dict(H=1025, nbytes=big)])


LDS = {"ftms_luma_kernel": 0, "ftms_down_kernel": 0, "ftms_detect_kernel": 19680, "ftms_describe_kernel": 0, "ftms_norm_kernel": 0, "ftms_refit_kernel": 46360}


def test_kernels_use_no_scratch_and_the_lds_of_the_readme():
    """from the compiler's metadata of csrc/features_ms.hip, built with the library's own flags (README.md, feature_align_ms, kernel table)"""
    spec = importlib.util.spec_from_file_location("_stitch_build", os.path.join(PKG, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert build.SOURCES["features_ms.hip"] == ["-ffp-contract=off"]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "features_ms.s")
        subprocess.check_call(build.compile_cmd("features_ms.hip", out, ["-S", "--cuda-device-only"]), stderr=subprocess.DEVNULL)
        text = open(out).read()
    rep = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+)\n.*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)",
                         text, re.S):
        rep[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    assert len(rep) == len(LDS), sorted(rep)
    readme = open(os.path.join(ROOT, "README.md")).read()
    table = readme[readme.index("## feature_align_ms"):]
    for key, want in LDS.items():
        (name, r), = [(n, r) for n, r in rep.items() if key in n]
        print(key, r)
        assert r["lds"] == want < 65536, (name, r)
        assert r["scratch"] == 0 and r["spill"] == 0 and r["vgpr"] <= 256, (name, r)
        row, = [ln for ln in table.splitlines() if ln.startswith(f"| `{key}`")]
        assert f"| {want} |" in row and f"| {r['vgpr']} |" in row, row
