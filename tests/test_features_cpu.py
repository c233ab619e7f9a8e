"""The CPU restatement of csrc/features.hip (tests/_features_ref.py) against plain per-pixel / per-pair / scalar Python loops, its accuracy on
procedural scenes with known homographies, the degenerate inputs, planted defects that must each fail one of those assertions, the C
entries' rejections and the compiler's resource report of csrc/features.hip."""
import importlib.util
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _features_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = frozenset()
SIZES = ((64, 64), (65, 97), (96, 130))


def _img(h, w, seed=1):
    return ref.small_pair(h, w, seed)[0][0]


# ---- the stages against loops ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_luma_harris_and_box_sum_per_pixel(size):
    h, w = size
    img = _img(h, w).copy()
    img[0, 3, 5], img[1, 7, 9], img[2, 2, 2], img[0, 9, 1], img[1, 0, 0] = np.nan, np.inf, -np.inf, 300.7, -4.0
    Y = ref.luma(img)
    R, S = ref.harris(Y), ref.window_sum(Y, 2)
    pix = lambda v: 0 if math.isnan(v) else int(min(max(v, 0.0), 255.0))                  # noqa: E731
    for y in range(h):
        for x in range(w):
            r, g, b = (pix(float(img[c, y, x])) for c in range(3))
            assert Y[y, x] == (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16
    assert Y[3, 5] == ref.luma(np.where(np.isnan(img), 0, img))[3, 5] and 0 <= Y.min() and Y.max() <= 255
    yc = lambda y, x: int(Y[min(max(y, 0), h - 1), min(max(x, 0), w - 1)])               # noqa: E731
    gx = np.zeros((h, w), np.int64)
    gy = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            gx[y, x] = (yc(y - 1, x + 1) + 2 * yc(y, x + 1) + yc(y + 1, x + 1)) - (yc(y - 1, x - 1) + 2 * yc(y, x - 1) + yc(y + 1, x - 1))
            gy[y, x] = (yc(y + 1, x - 1) + 2 * yc(y + 1, x) + yc(y + 1, x + 1)) - (yc(y - 1, x - 1) + 2 * yc(y - 1, x) + yc(y - 1, x + 1))
    for y in range(h):
        for x in range(w):
            sl = np.s_[max(y - 3, 0):y + 4, max(x - 3, 0):x + 4]
            A, B, Cc = int((gx[sl] ** 2).sum()), int((gy[sl] ** 2).sum()), int((gx[sl] * gy[sl]).sum())
            assert R[y, x] == 16 * (A * B - Cc * Cc) - (A + B) ** 2
            assert S[y, x] == int(Y[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3].sum())


def _planted_response(h, w):
    """equal responses side by side, diagonally, across a cell edge, and a plateau"""
    R = np.full((h, w), -5, np.int64)
    rng = np.random.default_rng(3)
    R[16:h - 16, 16:w - 16] = rng.integers(-50, 60, (h - 32, w - 32))
    R[24, 20] = R[24, 21] = 900
    R[25, 30] = R[26, 31] = 800
    R[28, 31] = R[28, 32] = R[29, 32] = 700
    R[40:43, 40:43] = 600
    R[18, 18] = R[18, 20] = R[20, 18] = R[20, 20] = 950                                   # five equal maxima in one cell: index order
    R[22, 24] = 950
    R[16, 16] = R[h - 17, w - 17] = 10 ** 15
    R[15, 30] = R[30, 15] = 10 ** 16                                                      # inside the border: never a candidate, but a neighbour
    return R


def _candidates_loop(R):
    h, w = R.shape
    ok = np.zeros((h, w), bool)
    for y in range(16, h - 16):
        for x in range(16, w - 16):
            good = R[y, x] > 0
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if (dy, dx) != (0, 0):
                        lower = (y + dy) * w + x + dx < y * w + x
                        good = good and (R[y, x] > R[y + dy, x + dx] if lower else R[y, x] >= R[y + dy, x + dx])
            ok[y, x] = good
    return ok


def _select_loop(R, cand):
    h, w = R.shape
    ch, cw = -(-h // 32), -(-w // 32)
    kp = np.full((4 * ch * cw, 2), -1, np.int32)
    for cy in range(ch):
        for cx in range(cw):
            c = [(-int(R[y, x]), y * w + x) for y in range(32 * cy, min(32 * cy + 32, h)) for x in range(32 * cx, min(32 * cx + 32, w)) if cand[y, x]]
            for rank, (_, idx) in enumerate(sorted(c)[:4]):
                kp[4 * (cy * cw + cx) + rank] = (idx % w, idx // w)
    return kp


def check_nms_and_cells(defects=NONE):
    for h, w in SIZES:
        R = _planted_response(h, w)
        cand = ref.candidates(R, defects)
        assert np.array_equal(cand, _candidates_loop(R)), (h, w)
        assert cand[24, 20] and not cand[24, 21] and cand[22, 24] and cand[25, 30] and not cand[26, 31] and cand[40, 40] and cand[40:43, 40:43].sum() == 1
        assert cand[16, 16] and cand[h - 17, w - 17] and not cand[15, 30] and not cand[16, 30]
        kp = ref.select(R, cand)
        assert np.array_equal(kp, _select_loop(R, cand)) and len(kp) == ref.slots(h, w)
        assert kp[:4].tolist() == [[16, 16], [18, 18], [20, 18], [18, 20]]               # R descending, then row-major index ascending
        R2 = ref.harris(ref.luma(_img(h, w)))
        c2 = ref.candidates(R2, defects)
        assert np.array_equal(c2, _candidates_loop(R2)) and np.array_equal(ref.select(R2, c2), _select_loop(R2, c2))


def _kp_and_box(h, w):
    kp, box = ref.detect(_img(h, w))
    return kp, box


def check_descriptor_bits_and_packing(defects=NONE):
    pat = ref.brief_pattern()
    assert pat.shape == (256, 4) and pat.dtype == np.int8 and pat.min() == -12 and pat.max() == 12
    for i in (0, 1, 517, 1023):                                                           # the table against scalar integer arithmetic
        x = ref.PATTERN_KEY ^ i
        x ^= x >> 16
        x = x * 0x85EBCA6B & 0xFFFFFFFF
        x ^= x >> 13
        x = x * 0xC2B2AE35 & 0xFFFFFFFF
        x ^= x >> 16
        assert pat.reshape(-1)[i] == x % 25 - 12
    for h, w in SIZES:
        kp, box = _kp_and_box(h, w)
        desc = ref.describe(box, kp, defects)
        assert desc.dtype == np.uint32 and desc.shape == (len(kp), 8)
        for s, (x, y) in enumerate(kp):
            words = [0] * 8
            if x >= 0:
                for k in range(256):
                    ax, ay, bx, by = (int(v) for v in pat[k])
                    if box[y + ay, x + ax] < box[y + by, x + bx]:
                        words[k >> 5] |= 1 << (k & 31)
            assert desc[s].tolist() == words, (h, w, s)
        assert (desc[kp[:, 0] < 0] == 0).all() and (kp[:, 0] >= 0).any()


def _planted_descriptors(N=48, seed=9):
    """random descriptors with unused slots, exact duplicates (distance 0 twice) and equal distances to two candidates"""
    rng = np.random.default_rng(seed)
    d1 = rng.integers(0, 2 ** 32, (N, 8), dtype=np.uint64).astype(np.uint32)
    d2 = d1[rng.permutation(N)].copy()
    d2 ^= (rng.random((N, 8)) < 0.3).astype(np.uint32) << rng.integers(0, 32, (N, 8)).astype(np.uint32)
    kp1 = np.stack([np.arange(N) + 16, np.arange(N) + 16], 1).astype(np.int32)
    kp2 = kp1.copy()
    kp1[[3, 17]] = -1
    kp2[[5, 6, 40]] = -1
    d1[[3, 17]] = 0
    d2[[5, 6, 40]] = 0
    d2[11] = d2[10]                                                                        # two equal candidates: the lowest slot, d2 = d1
    d2[30] = d2[31] = d1[8] ^ np.array([1, 0, 0, 0, 0, 0, 0, 0], np.uint32)
    d1[20] = d1[21]                                                                        # two equal queries: the reverse direction's tie
    return kp1, d1, kp2, d2


def _nearest_loop(kq, dq, kc, dc):
    out = []
    for i in range(len(kq)):
        best, d1, d2 = -1, 257, 257
        if kq[i, 0] >= 0:
            for j in range(len(kc)):
                if kc[j, 0] < 0:
                    continue
                d = sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(dq[i], dc[j]))
                if d < d1:
                    best, d1, d2 = j, d, d1
                elif d < d2:
                    d2 = d
        out.append((best, d1, d2))
    return np.array(out, np.int32)


def check_match_both_directions_and_compaction(defects=NONE):
    kp1, d1, kp2, d2 = _planted_descriptors()
    nn, matches, m = ref.match(kp1, d1, kp2, d2, defects)
    f, r = _nearest_loop(kp1, d1, kp2, d2), _nearest_loop(kp2, d2, kp1, d1)
    assert np.array_equal(nn[0], f) and np.array_equal(nn[1], r)
    assert f[3].tolist() == [-1, 257, 257] and f[8, 0] == 30 and f[8, 1] == f[8, 2] == 1
    want = [(i, int(f[i, 0])) for i in range(len(kp1)) if f[i, 0] >= 0 and f[i, 1] < 80 and 10 * f[i, 1] < 8 * f[i, 2] and r[f[i, 0], 0] == i]
    assert m == len(want) > 8 and matches[:m].tolist() == [list(p) for p in want] and (matches[m:] == -1).all()
    one = np.full_like(kp2, -1)                                                            # one candidate: d2 = 257; none: no best
    one[7] = kp2[7]
    assert (ref.nearest(kp1, d1, one, d2, defects)[kp1[:, 0] >= 0, 2] == 257).all()
    assert (ref.nearest(kp1, d1, np.full_like(kp2, -1), d2, defects)[:, 0] == -1).all()


def _fmix(x):
    x ^= x >> 16
    x = x * 0x85EBCA6B & 0xFFFFFFFF
    x ^= x >> 13
    x = x * 0xC2B2AE35 & 0xFFFFFFFF
    return x ^ x >> 16


def _rows_scalar(x, y, u, v):
    return [[x, y, 1.0, 0.0, 0.0, 0.0, -u * x, -u * y, u], [0.0, 0.0, 0.0, x, y, 1.0, -v * x, -v * y, v]]


def _solve_scalar(A):
    A = [[float(v) for v in row] for row in A]
    for c in range(8):
        piv = max(range(c, 8), key=lambda r: (abs(A[r][c]), -r))
        if not abs(A[piv][c]) >= 1e-10:
            return None
        A[c], A[piv] = A[piv], A[c]
        for r in range(c + 1, 8):
            f = A[r][c] / A[c][c]
            for k in range(c + 1, 9):
                A[r][k] = A[r][k] - f * A[c][k]
    x = [0.0] * 8
    for r in range(7, -1, -1):
        s = A[r][8]
        for k in range(r + 1, 8):
            s = s - A[r][k] * x[k]
        x[r] = s / A[r][r]
    return x


def _inlier_scalar(h, p, sx, sy, thr2):
    x, y, u, v = (float(t) for t in p)
    den = (h[6] * x + h[7] * y) + 1.0
    if not den > 0.0:
        return False
    px, py = ((h[0] * x + h[1] * y) + h[2]) / den, ((h[3] * x + h[4] * y) + h[5]) / den
    ex, ey = (px - u) * sx, (py - v) * sy
    return ex * ex + ey * ey < thr2


def _ransac_scalar(kp1, kp2, matches, m, H, W, max_hyp, thr, min_inliers, seed):
    """the whole of contract section 5 and 6 in Python floats (IEEE double, one rounding per operation)"""
    sx, sy, thr2 = 0.5 * W, 0.5 * H, thr * thr
    mc = [((kp1[i][0] - sx) / sx, (kp1[i][1] - sy) / sy, (kp2[j][0] - sx) / sx, (kp2[j][1] - sy) / sy) for i, j in matches[:m].tolist()]
    best, winner, h = -1, -1, None
    if m >= 8:
        for k in range(max_hyp):
            key = _fmix((seed & 0xFFFFFFFF) ^ _fmix(k))
            idx = [_fmix(key ^ (t + 1)) % m for t in range(4)]
            if len(set(idx)) < 4:
                continue
            x = _solve_scalar([row for i in idx for row in _rows_scalar(*mc[i])])
            if x is None:
                continue
            score = sum(_inlier_scalar(x, p, sx, sy, thr2) for p in mc)
            if score > best:
                best, winner, h = score, k, x
    mask = [False] * m
    if h is not None:
        mask = [_inlier_scalar(h, p, sx, sy, thr2) for p in mc]
        for _ in range(2):
            S = [[[0.0] * 9 for _ in range(8)] for _ in range(4)]                       # four interleaved partial sums per entry
            for i, (p, on) in enumerate(zip(mc, mask)):
                if on:
                    for row in _rows_scalar(*p):
                        for r in range(8):
                            for c in range(9):
                                S[i % 4][r][c] = S[i % 4][r][c] + row[r] * row[c]
            A = [[(S[0][r][c] + S[1][r][c]) + (S[2][r][c] + S[3][r][c]) for c in range(9)] for r in range(8)]
            x = _solve_scalar(A)
            if x is not None:
                h = x
            mask = [_inlier_scalar(h, p, sx, sy, thr2) for p in mc]
    count = sum(mask)
    valid = h is not None and count >= min_inliers
    Hp, motion = np.eye(3), np.zeros((4, 2))
    if valid:
        g = h + [1.0]
        M = [[g[3 * r] / sx, g[3 * r + 1] / sy, (g[3 * r + 2] - g[3 * r]) - g[3 * r + 1]] for r in range(3)]
        P = [[sx * M[0][c] + sx * M[2][c] for c in range(3)], [sy * M[1][c] + sy * M[2][c] for c in range(3)], M[2]]
        Hp = np.array([[P[r][c] / P[2][2] for c in range(3)] for r in range(3)])
        for q, (xn, yn, cx, cy) in enumerate(((-1.0, -1.0, 0.0, 0.0), (1.0, -1.0, float(W), 0.0), (-1.0, 1.0, 0.0, float(H)), (1.0, 1.0, float(W), float(H)))):
            den = (g[6] * xn + g[7] * yn) + 1.0
            motion[q] = (((g[0] * xn + g[1] * yn) + g[2]) / den * sx + sx) - cx, (((g[3] * xn + g[4] * yn) + g[5]) / den * sy + sy) - cy
    info = [int(valid), int((kp1[:, 0] >= 0).sum()), int((kp2[:, 0] >= 0).sum()), m, winner, count, 0, 0]
    return motion.astype(np.float32), Hp.astype(np.float32), info, mask


def check_draws(defects=NONE):
    for seed, m in ((1, 8), (0x9E3779B9, 523), (7, 4096)):
        got = ref.draws(seed, np.arange(300), m, defects)
        for k in (0, 1, 63, 64, 299):
            key = _fmix(seed ^ _fmix(k))
            assert got[k].tolist() == [_fmix(key ^ (t + 1)) % m for t in range(4)], (seed, m, k)


def check_four_point_solve(defects=NONE):
    rng = np.random.default_rng(2)
    Hm = ref.homography_matrix(2, 2, 0.1, -0.05, 4.0, 0.02, -0.01)
    p = rng.uniform(-1, 1, (5, 4, 2))
    q = np.concatenate([p, np.ones((5, 4, 1))], 2) @ Hm.T
    mc = np.concatenate([p, q[..., :2] / q[..., 2:]], 2)
    A = ref.rows(mc).reshape(5, 8, 9)
    ok, x = ref.solve8(A)
    assert ok.all()
    for k in range(5):
        assert np.abs(x[k] - np.linalg.solve(A[k, :, :8], A[k, :, 8])).max() < 1e-10
        assert x[k].tolist() == _solve_scalar(A[k].tolist())
        assert np.abs(np.append(x[k], 1).reshape(3, 3) - Hm / Hm[2, 2]).max() < 1e-10
    A[1, 3] = A[1, 2]                                                                      # a repeated row: singular, void
    A[2, :, 0] = 0.0
    ok, _ = ref.solve8(A)
    assert ok.tolist() == [True, False, False, True, True]
    T = np.zeros((1, 8, 9))                                                                # equal pivot candidates: the lowest row
    T[0, :, :8] = np.eye(8)[::-1]
    T[0, :, 0] = 1.0
    T[0, :, 8] = np.arange(8)
    ok, x = ref.solve8(T)
    assert ok[0] and x[0].tolist() == _solve_scalar(T[0].tolist())


def check_scoring_and_refit(defects=NONE):
    """the planted match lists: scores, winner, inlier mask, refit, H, motion and info against the scalar loops, bit for bit"""
    H, W = 96, 128
    for name in ref.PLANTED:
        kp1, kp2, matches, m = ref.planted_matches(name, H, W)
        for seed, max_hyp in ((7, 96), (1, 33)):
            got = ref.ransac(kp1, kp2, matches, m, H, W, max_hyp, 3.0, 6, seed, defects)
            want = _ransac_scalar(kp1, kp2, matches, m, H, W, max_hyp, 3.0, 6, seed)
            assert got[2].tolist() == want[2], (name, got[2].tolist(), want[2])
            assert got[3][:m].astype(bool).tolist() == want[3] and not got[3][m:].any(), name
            assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (name, got[1], want[1])
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (name, got[0], want[0])
    kp1, kp2, matches, m = ref.planted_matches("outliers", H, W)
    motion, Hf, info, mask = ref.ransac(kp1, kp2, matches, m, H, W, 96, 3.0, 6, 7, defects)
    assert info[0] == 1 and info[5] == 26 and mask[:m].sum() == 26 and not mask[:40:3].any()
    c = np.array([[0, 0, 1], [W, 0, 1], [0, H, 1], [W, H, 1]], np.float64)                # motion = H(corner) - corner: what dlt4 inverts
    pc = c @ Hf.astype(np.float64).T
    assert np.abs(pc[:, :2] / pc[:, 2:] - c[:, :2] - motion).max() < 1e-4
    for name, valid in (("m8", 1), ("line", 0), ("few", 0)):
        k1, k2, mt, mm = ref.planted_matches(name, H, W)
        _, Hq, inf, _, scores = ref.ransac(k1, k2, mt, mm, H, W, 96, 3.0, 6, 7, defects, return_scores=True)
        assert inf[0] == valid and inf[3] == mm
        if name == "m8":
            assert 0.4 < (scores < 0).mean() < 0.8 and inf[5] == 8                         # most hypotheses repeat an index
        else:
            assert (scores < 0).all() and inf[4] == -1 and np.array_equal(Hq, np.eye(3, dtype=np.float32))


CHECKS = (check_nms_and_cells, check_descriptor_bits_and_packing, check_match_both_directions_and_compaction, check_draws, check_four_point_solve,
          check_scoring_and_refit)


@pytest.mark.parametrize("check", CHECKS, ids=lambda c: c.__name__)
def test_restatement_against_loops(check):
    check(NONE)


@pytest.mark.parametrize("defect", ref.DEFECTS)
def test_planted_defects_are_noticed(defect):
    failed = None
    for check in CHECKS:
        try:
            check(frozenset({defect}))
        except AssertionError:
            failed = check.__name__
            break
    assert failed, f"no assertion notices {defect}"
    print(f"{defect}: noticed by {failed}")


# ---- accuracy ----------------------------------------------------------------------------------------------------------------------------------
# measured with this restatement (README.md, feature_align, accuracy table): corner error 0.08 .. 0.44 px over the five 512x512 scenes and 0.44 px
# on the 192x256 one; the bound is 3 x the worst, which lies between the 0.5 px floor and thr = 3 px
ACCURACY_BOUND = 3 * 0.45
SCENES = [(512, 512, mo, 3 + i) for i, mo in enumerate(ref.MOTIONS)] + [(192, 256, (32, 4, 0, 0, 0), 3)]


@pytest.mark.parametrize("scene", SCENES, ids=lambda s: f"{s[0]}x{s[1]}_seed{s[3]}")
def test_accuracy_and_direction_on_known_homographies(scene):
    h, w, motion, seed = scene
    a, b, Hgt = ref.pair(h, w, motion, seed)
    res = ref.homography(a, b)
    info, Hf = res["info"][0], res["H"][0].astype(np.float64)
    err = ref.corner_error(Hf, Hgt, h, w)
    print(f"{h}x{w} {motion}: keypoints {info[1]} / {info[2]}, matches {info[3]}, inliers {info[5]}, corner error {err:.3f} px")
    assert 0.5 <= ACCURACY_BOUND <= 3.0
    assert info[0] == 1 and info[5] >= 100 and err < ACCURACY_BOUND < 1.5
    # the direction: image 2 resampled through H lands on image 1
    g1, g2 = a[0, 0].astype(np.float64), b[0, 0].astype(np.float64)
    warped = ref.resample(g2, Hf, h, w)
    inside = ref.resample(np.ones_like(g2), Hf, h, w) > 0.999
    adj = lambda g: (g - 10.0) / 0.85                                                     # noqa: E731  (the known gain and bias of image 2)
    assert inside.mean() > 0.3
    assert np.abs(adj(warped) - g1)[inside].mean() < np.abs(adj(g2) - g1)[inside].mean() / 3


# ---- degenerate images ---------------------------------------------------------------------------------------------------------------------------
def test_degenerate_images_and_their_info():
    res = {n: ref.homography(*ref.degenerate(n)) for n in ref.DEGENERATE}
    info = {n: r["info"][0].tolist() for n, r in res.items()}
    print(info)
    assert info["constant"] == [0, 0, 0, 0, -1, 0, 0, 0] and (res["constant"]["kp1"] == -1).all() and not res["constant"]["desc1"].any()
    i = info["identical"]
    assert i[0] == 1 and i[1] == i[2] == i[3] == i[5] > 12 and np.abs(res["identical"]["H"][0].astype(np.float64) - np.eye(3)).max() < 1e-9
    assert np.abs(res["identical"]["motion"]).max() < 1e-9
    assert info["unrelated"][0] == 0 and info["unrelated"][3] < 8 and info["unrelated"][4] == -1 and info["unrelated"][1] > 20
    assert np.array_equal(res["unrelated"]["H"][0], np.eye(3, dtype=np.float32)) and not res["unrelated"]["motion"].any()
    c = res["checker"]
    assert info["checker"][1] == info["checker"][2] == 48 and info["checker"][0] == 0                         # every cell full: ties fall to the lowest index
    assert (c["nn"][0, 0, :, 1] == c["nn"][0, 0, :, 2]).all() and info["checker"][3] == 0                     # every best has an equal: the ratio test rejects all
    assert info["nonfinite"][1] > 20 and info["nonfinite"][3] >= 8


# ---- entries and binary ------------------------------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_touching_the_gpu():
    import ctypes as C
    from stitch_amd._lib import lib
    base = 0x7f0000000000                                                   # never dereferenced on the host
    P = [base + (i << 32) for i in range(12)]
    B, H, W, hyp = 2, 65, 97, 100
    N = lib.st_feature_slots(H, W)
    assert N == ref.slots(H, W) == 48 and lib.st_feature_slots(512, 512) == 1024 and lib.st_feature_slots(63, 64) == 0 and lib.st_feature_slots(64, 1025) == 0
    wsb = lib.st_feature_workspace_bytes
    need = wsb(B, H, W, hyp)
    assert need > 0 and need % 16 == 0 and wsb(B, H, W, hyp + 8) > need and 0 < wsb(64, 1024, 1024, 65536) < 2 ** 31
    for bad in ((0, H, W, hyp), (65, H, W, hyp), (B, 63, W, hyp), (B, H, 63, hyp), (B, 1025, W, hyp), (B, H, 1025, hyp), (B, H, W, 0), (B, H, W, 65537), (-1, H, W, hyp)):
        assert wsb(*bad) == 0, bad
    off = (C.c_int64 * 10)()
    assert lib.st_feature_workspace_layout(B, H, W, hyp, C.cast(off, C.c_void_p)) == 0 and off[9] == need and list(off) == sorted(off) and off[0] == 0
    assert lib.st_feature_workspace_layout(B, H, W, hyp, None) == 1001 and lib.st_feature_workspace_layout(B, 63, W, hyp, C.cast(off, C.c_void_p)) == 1001
    assert lib.st_feature_brief_pattern(None) == 1001
    px, bn, big = B * H * W, B * N, 1 << 40
    nan, inf = float("nan"), float("inf")

    def sweep(call, regions, outputs, shape_args):
        """nulls, shapes, and every output against every other operand: overlapping at its first and last byte"""
        for name in regions:
            assert call(**{name: None}) == 1001, name
        for kw in shape_args:
            assert call(**kw) == 1001, kw
        assert call() is not None
        for a in outputs:
            for b in regions:
                if a != b:
                    pa, pb = regions[a], regions[b]
                    assert call(**{a: pb[0]}) == 1001 and call(**{a: pb[0] + pb[1] - 1}) == 1001 and call(**{a: pb[0] - pa[1] + 1}) == 1001, (a, b)

    shapes = [dict(B=0), dict(B=65), dict(H=63), dict(W=63), dict(H=1025), dict(W=1025), dict(B=-1)]
    params = [dict(max_hyp=0), dict(max_hyp=65537), dict(thr=0.0), dict(thr=-1.0), dict(thr=nan), dict(thr=inf), dict(thr=-inf), dict(min_inliers=-1)]

    # (a call that passes every check would launch: each sweep therefore keeps one argument bad -- a stream is never needed)
    def detect(img=P[0], kp=P[1], box=P[2], B=B, H=H, W=W, bad=True):
        return lib.st_feature_detect(img, 0 if bad and (img, kp, box, B, H, W) == (P[0], P[1], P[2], 2, 65, 97) else B, H, W, kp, box, None)
    sweep(detect, dict(img=(P[0], 12 * px), kp=(P[1], 8 * bn), box=(P[2], 2 * px)), ("kp", "box"), shapes)

    def describe(box=P[0], kp=P[1], desc=P[2], B=B, H=H, W=W):
        return lib.st_feature_describe(box, kp, 0 if (box, kp, desc, B, H, W) == (P[0], P[1], P[2], 2, 65, 97) else B, H, W, desc, None)
    sweep(describe, dict(box=(P[0], 2 * px), kp=(P[1], 8 * bn), desc=(P[2], 32 * bn)), ("desc",), shapes)

    def match(kp1=P[0], desc1=P[1], kp2=P[2], desc2=P[3], nn=P[4], matches=P[5], count=P[6], B=B, H=H, W=W):
        clean = (kp1, desc1, kp2, desc2, nn, matches, count, B, H, W) == (*P[:7], 2, 65, 97)
        return lib.st_feature_match(kp1, desc1, kp2, desc2, 0 if clean else B, H, W, nn, matches, count, None)
    sweep(match, dict(kp1=(P[0], 8 * bn), desc1=(P[1], 32 * bn), kp2=(P[2], 8 * bn), desc2=(P[3], 32 * bn), nn=(P[4], 24 * bn), matches=(P[5], 8 * bn),
                      count=(P[6], 4 * B)), ("nn", "matches", "count"), shapes)
    assert lib.st_feature_match(P[0], P[1], P[0], P[1], 0, H, W, P[4], P[5], P[6], None) == 1001

    rneed = 32 * bn + 4 * B * hyp

    def ransac(kp1=P[0], kp2=P[1], matches=P[2], count=P[3], motion=P[4], Hm=P[5], info=P[6], mask=P[7], ws=P[8], B=B, H=H, W=W, max_hyp=hyp, thr=3.0, min_inliers=12,
               nbytes=rneed):
        clean = (kp1, kp2, matches, count, motion, Hm, info, mask, ws, B, H, W, max_hyp, thr, min_inliers, nbytes) == (*P[:9], 2, 65, 97, hyp, 3.0, 12, rneed)
        return lib.st_feature_ransac(kp1, kp2, matches, count, 0 if clean else B, H, W, max_hyp, thr, min_inliers, 1, motion, Hm, info, mask, ws, nbytes, None)
    sweep(ransac, dict(kp1=(P[0], 8 * bn), kp2=(P[1], 8 * bn), matches=(P[2], 8 * bn), count=(P[3], 4 * B), motion=(P[4], 32 * B), Hm=(P[5], 36 * B), info=(P[6], 32 * B),
                       mask=(P[7], bn), ws=(P[8], rneed)), ("motion", "Hm", "info", "mask", "ws"),
          shapes + params + [dict(nbytes=rneed - 1), dict(nbytes=0), dict(ws=P[8] + 8), dict(max_hyp=hyp + 1), dict(H=H + 32, nbytes=rneed)])

    def homography(img1=P[0], img2=P[1], motion=P[2], Hm=P[3], info=P[4], ws=P[5], B=B, H=H, W=W, max_hyp=hyp, thr=3.0, min_inliers=12, nbytes=need):
        clean = (img1, img2, motion, Hm, info, ws, B, H, W, max_hyp, thr, min_inliers, nbytes) == (*P[:6], 2, 65, 97, hyp, 3.0, 12, need)
        return lib.st_feature_homography(img1, img2, 0 if clean else B, H, W, max_hyp, thr, min_inliers, 1, motion, Hm, info, ws, nbytes, None)
    sweep(homography, dict(img1=(P[0], 12 * px), img2=(P[1], 12 * px), motion=(P[2], 32 * B), Hm=(P[3], 36 * B), info=(P[4], 32 * B), ws=(P[5], need)),
          ("motion", "Hm", "info", "ws"),
          shapes + params + [dict(nbytes=need - 1), dict(nbytes=0), dict(ws=P[5] + 8), dict(max_hyp=hyp + 8), dict(H=H + 32), dict(B=B + 1), dict(H=1025, nbytes=big)])
    assert lib.st_feature_homography(P[0], P[0], 0, H, W, hyp, 3.0, 12, 1, P[2], P[3], P[4], P[5], need, None) == 1001


LDS = {"ft_detect_kernel": 17552, "ft_describe_kernel": 0, "ft_match_kernel": 33792, "ft_compact_kernel": 64, "ft_norm_kernel": 0, "ft_hyp_kernel": 36864,
       "ft_refit_kernel": 38936}


def test_kernels_use_no_scratch_and_the_lds_of_the_readme():
    """from the compiler's metadata of csrc/features.hip, built with the library's own flags (README.md, feature_align, kernel table)"""
    spec = importlib.util.spec_from_file_location("_stitch_build", os.path.join(ROOT, "seamless-through-breaking-rethinking-image-stitching-for-optimal-alignment_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert build.SOURCES["features.hip"] == ["-ffp-contract=off"]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "features.s")
        subprocess.check_call(build.compile_cmd("features.hip", out, ["-S", "--cuda-device-only"]), stderr=subprocess.DEVNULL)
        text = open(out).read()
    rep = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+)\n.*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)",
                         text, re.S):
        rep[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    assert len(rep) == len(LDS), sorted(rep)
    readme = open(os.path.join(ROOT, "README.md")).read()
    table = readme[readme.index("## feature_align"):]
    for key, want in LDS.items():
        (name, r), = [(n, r) for n, r in rep.items() if key in n]
        print(key, r)
        assert r["lds"] == want <= 65536, (name, r)
        assert r["scratch"] == 0 and r["spill"] == 0 and r["vgpr"] <= 256, (name, r)
        row, = [ln for ln in table.splitlines() if ln.startswith(f"| `{key}`")]
        assert f"| {want} |" in row and f"| {r['vgpr']} |" in row, row
