"""dense_flow without a GPU (README.md, "dense_flow"): every vectorised stage of tests/_dense_flow_ref.py against plain scalar loops, the accuracy of
the contract on procedural scenes with a known flow, degenerate inputs, planted defects, the C entries' rejections and the compiler's resource report."""
import importlib.util
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _dense_flow_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = frozenset()
SIZES = ((16, 16), (33, 65), (48, 40))
G = (1, 4, 6, 4, 1)


def _clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def _img(h, w, seed=1):
    """a textured fp32 [3,h,w] image"""
    g = ref.scene(max(h, 64), max(w, 64), seed)[:h, :w]
    return ref.rgb(g)


def _levels(h, w, seed=1, shift=1.3):
    """(V1, V2, m1, m2, U) int64 at one level: two shifted cuts of one scene, masks with holes, a small non-zero flow with fractions and outliers"""
    rng = np.random.default_rng(seed)
    from scipy import ndimage as ndi
    big = ref.scene(max(h, 64) + 8, max(w, 64) + 8, seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    a = ndi.map_coordinates(big, [ys + 4, xs + 4], order=1)
    b = ndi.map_coordinates(big, [ys + 4 - 0.6 * shift, xs + 4 - shift], order=1) * 0.85 + 10
    V1, m1 = ref.level0(ref.rgb(a), None)
    V2, m2 = ref.level0(ref.rgb(b), None)
    m1[h // 2:h // 2 + 3, 2:6] = 0
    m2[3:8, w - 7:w - 2] = 0
    m2[h - 2, 1] = 0
    U = rng.integers(-200, 200, (2, h, w)).astype(np.int64)
    U[:, 0, 0] = (-300, -257)                     # negative coordinates: the shift is arithmetic
    U[:, 5, w - 2] = (0, 17)                      # x0 = W - 2: the last sample with four taps
    U[:, 6, w - 2] = (256, 0)                     # x0 = W - 1: outside
    U[:, h - 2, 3] = (5, 255)                     # y0 = H - 2
    U[:, h - 2, 4] = (5, 256)                     # y0 = H - 1
    return V1, V2, m1, m2, U


# ---- the stages in loops -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_luma_and_mask_rules_per_pixel(size):
    h, w = size
    img = _img(h, w) + np.float32(0.75)
    nxt = np.nextafter(np.float32(0.5), np.float32(1))
    img[0, 1, 1], img[1, 1, 2], img[2, 2, 2], img[0, 3, 3], img[1, 4, 4], img[2, 5, 5] = np.nan, -np.inf, np.inf, -3.0, 255.9, 300.0
    mask = np.ones((3, h, w), np.float32)
    mask[0, 0, :6] = (0.5, nxt, np.nan, np.inf, -np.inf, 0.0)
    mask[1:, 2, :] = 0                              # only channel 0 is read
    V, m = ref.level0(img, mask)
    for y in range(h):
        for x in range(w):
            p = []
            for c in range(3):
                v = float(img[c, y, x])
                p.append(0 if v != v else int(min(max(v, 0.0), 255.0)))
            assert V[y, x] == 16 * ((19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 0x8000) >> 16), (y, x)
            assert m[y, x] == (1 if float(mask[0, y, x]) > 0.5 else 0), (y, x)
    assert m[0, :6].tolist() == [0, 1, 0, 1, 0, 0] and m[2].all() and 0 <= V.min() and V.max() <= 4080
    assert np.array_equal(ref.level0(img, mask[:1])[1], m) and ref.level0(img, None)[1].all()


def _down_loop(V, m):
    H, W = V.shape
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    Vc, mc, dn = np.zeros((Hc, Wc), np.int64), np.zeros((Hc, Wc), np.int64), np.zeros((Hc, Wc), np.int64)
    for i in range(Hc):
        for j in range(Wc):
            num = den = 0
            for a in range(5):
                for b in range(5):
                    yy, xx = _clamp(2 * i + a - 2, 0, H - 1), _clamp(2 * j + b - 2, 0, W - 1)
                    num += G[a] * G[b] * int(m[yy, xx]) * int(V[yy, xx])
                    den += G[a] * G[b] * int(m[yy, xx])
            Vc[i, j], mc[i, j], dn[i, j] = ((2 * num + den) // (2 * den) if den > 0 else 0), int(den >= 128), den
    return Vc, mc, dn


def check_pyramid(defects=NONE):
    for h, w in SIZES:
        V, m = ref.level0(_img(h, w), None)
        m[:] = 1
        m[0:7, 0:7] = 0                                                           # den = 0 round coarse (1, 1) .. (2, 2)
        # round coarse (5, 5) = fine (10, 10): columns 8 and 9 whole and two taps of column 10 -> den = 16 + 64 + 48 = 128
        m[8:13, 8:13] = 0
        m[8:13, 8:10] = 1
        m[[9, 11], 10] = 1
        # round coarse (5, 8) = fine (10, 16): the same less the corner tap -> den = 127
        if w >= 33:
            m[8:13, 14:19] = 0
            m[8:13, 14:16] = 1
            m[[9, 11], 16] = 1
            m[8, 14] = 0
        Vc, mc = ref.down(V, m, defects)
        Vl, ml, dn = _down_loop(V, m)
        assert Vc.shape == ((h + 1) // 2, (w + 1) // 2)
        assert dn[1, 1] == 0 and Vl[1, 1] == 0 and ml[1, 1] == 0 and dn[5, 5] == 128 and ml[5, 5] == 1
        if w >= 33:
            assert dn[5, 8] == 127 and ml[5, 8] == 0
        assert np.array_equal(Vc, Vl) and np.array_equal(mc, ml), (h, w)
    # levels: halved while the smaller side is at least 32 and the count allows
    assert ref.level_sizes(16, 16, 5) == [(16, 16)] and ref.level_sizes(31, 33, 5) == [(31, 33)] and ref.level_sizes(32, 32, 5) == [(32, 32), (16, 16)]
    assert ref.level_sizes(33, 65, 8) == [(33, 65), (17, 33)] and ref.level_sizes(512, 512, 8) == [(512, 512), (256, 256), (128, 128), (64, 64), (32, 32), (16, 16)]
    assert ref.level_sizes(512, 512, 3) == [(512, 512), (256, 256), (128, 128)] and ref.level_sizes(1024, 32, 5) == [(1024, 32), (512, 16)]


def _sample_loop(V2, m2, U):
    H, W = V2.shape
    J, w2 = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            sx, sy = 256 * x + int(U[0, y, x]), 256 * y + int(U[1, y, x])
            x0, fx, y0, fy = sx >> 8, sx & 255, sy >> 8, sy & 255                 # Python's >> is arithmetic, & of a negative two's complement
            if not (0 <= x0 <= W - 2 and 0 <= y0 <= H - 2):
                continue
            if not (m2[y0, x0] and m2[y0, x0 + 1] and m2[y0 + 1, x0] and m2[y0 + 1, x0 + 1]):
                continue
            w2[y, x] = 1
            J[y, x] = ((256 - fx) * (256 - fy) * int(V2[y0, x0]) + fx * (256 - fy) * int(V2[y0, x0 + 1]) + (256 - fx) * fy * int(V2[y0 + 1, x0])
                       + fx * fy * int(V2[y0 + 1, x0 + 1]) + (1 << 15)) >> 16
    return J, w2


def check_bilinear_sample(defects=NONE):
    for h, w in SIZES:
        V1, V2, m1, m2, U = _levels(h, w)
        J, w2 = ref.sample(V2, m2, U[0], U[1], defects)
        Jl, wl = _sample_loop(V2, m2, U)
        assert wl[0, 0] == 0 and wl[5, w - 2] == 1 and wl[6, w - 2] == 0 and wl[h - 2, 3] == 1 and wl[h - 2, 4] == 0 and 0 < wl.mean() < 1
        assert (-300 >> 8, -300 & 255) == (-2, 212)
        assert np.array_equal(w2, wl) and np.array_equal(J, Jl), (h, w)


def check_gradients_and_window_sums(defects=NONE):
    for (h, w), r in zip(SIZES, (1, 4, 7)):
        V1, V2, m1, m2, U = _levels(h, w)
        gx, gy, w1 = ref.gradients(V1, m1)
        for y in range(h):
            for x in range(w):
                xl, xr, yu, yd = max(x - 1, 0), min(x + 1, w - 1), max(y - 1, 0), min(y + 1, h - 1)
                assert gx[y, x] == V1[y, xr] - V1[y, xl] and gy[y, x] == V1[yd, x] - V1[yu, x]
                assert w1[y, x] == (m1[y, x] & m1[y, xl] & m1[y, xr] & m1[yu, x] & m1[yd, x])
        f = gx * gy + 1                                                           # non-zero at the border
        S = ref.window_sum(f, r, defects)
        for y in range(h):
            for x in range(w):
                s = 0
                for dy in range(-r, r + 1):
                    for dx in range(-r, r + 1):
                        if 0 <= y + dy < h and 0 <= x + dx < w:
                            s += int(f[y + dy, x + dx])
                assert S[y, x] == s, (h, w, r, y, x)


def _solve_scalar(n, Sx, Sy, St, Sxx, Sxy, Syy, Sxt, Syt, r, damping):
    """Python ints are exact, Python floats are IEEE doubles with one rounding per operation, round() rounds half to even"""
    A, Cq, Bm = n * Sxx - Sx * Sx + damping * n * n, n * Syy - Sy * Sy + damping * n * n, n * Sxy - Sx * Sy
    bx, by = n * Sxt - Sx * St, n * Syt - Sy * St
    assert max(abs(v) for v in (A, Cq, Bm, bx, by)) < 2 ** 53
    A, Cq, Bm, bx, by = float(A), float(Cq), float(Bm), float(bx), float(by)
    det = A * Cq - Bm * Bm
    if n < (2 * r + 1) ** 2 // 4 or not det > 0.0:
        return 0, 0, 0
    dx, dy = -512.0 * ((Cq * bx - Bm * by) / det), -512.0 * ((A * by - Bm * bx) / det)
    return round(min(max(dx, -256.0), 256.0)), round(min(max(dy, -256.0), 256.0)), 1


# planted sums (n, Sx, Sy, St, Sxx, Sxy, Syy, Sxt, Syt) at r = 4, damping 0: A = C = 65536, so dU = -Sxt / 2: ties, the clamp, det <= 0, n at the threshold
PLANTED = [((64, 0, 0, 0, 1024, 0, 1024, 1, 3), (0, -2, 1)), ((64, 0, 0, 0, 1024, 0, 1024, -5, -7), (2, 4, 1)), ((64, 0, 0, 0, 1024, 0, 1024, 1000, -1000), (-256, 256, 1)),
           ((64, 0, 0, 0, 1024, 0, 1024, 511, -513), (-256, 256, 1)), ((64, 0, 0, 0, 1024, 0, 1024, 9, -11), (-4, 6, 1)),
           ((64, 0, 0, 0, 0, 0, 0, 5, 5), (0, 0, 0)), ((64, 0, 0, 0, 1024, 1024, 1024, 5, 5), (0, 0, 0)), ((64, 0, 0, 0, 1024, 2048, 1024, 5, 5), (0, 0, 0)),
           ((20, 0, 0, 0, 1024, 0, 1024, 64, 0), (-32, 0, 1)), ((19, 0, 0, 0, 1024, 0, 1024, 64, 0), (0, 0, 0)), ((0, 0, 0, 0, 0, 0, 0, 0, 0), (0, 0, 0)),
           ((64, 640, 0, 64, 7424, 0, 1024, 643, 0), (-2, 0, 1))]                  # zero-mean: A = 64 * 7424 - 640^2 = 65536, bx = 64 * 643 - 640 * 64 = 192


def check_solve(defects=NONE):
    for sums, want in PLANTED:
        got = ref.solve(*(np.array([[v]], np.int64) for v in sums), 4, 0, defects)
        assert _solve_scalar(*sums, 4, 0) == want, (sums, want)
        assert tuple(int(g[0, 0]) for g in got) == want, (sums, want, got)
    for (h, w), r, damping in zip(SIZES, (1, 4, 7), (0, 65536, 1 << 24)):
        V1, V2, m1, m2, U = _levels(h, w)
        gx, gy, w1 = ref.gradients(V1, m1)
        J, w2 = ref.sample(V2, m2, U[0], U[1])
        wt = w1 & w2
        gx, gy, It = wt * gx, wt * gy, wt * (J - V1)
        S = [ref.window_sum(f, r) for f in (wt, gx, gy, It, gx * gx, gx * gy, gy * gy, gx * It, gy * It)]
        dx, dy, ok = ref.solve(*S, r, damping, defects)
        for y in range(h):
            for x in range(w):
                assert (int(dx[y, x]), int(dy[y, x]), int(ok[y, x])) == _solve_scalar(*(int(s[y, x]) for s in S), r, damping), (h, w, y, x)
    # the bound on the radius: |gx|, |gy|, |It| <= 8160, so every entry is below n^2 (2 * 8160^2 + 2^24) with n = (2r + 1)^2: below 2^53 up to r = 43
    bound = lambda r: (2 * r + 1) ** 4 * (2 * 8160 ** 2 + (1 << 24))              # noqa: E731
    assert bound(43) < 2 ** 53 <= bound(44) and ref.MAX_RADIUS <= 43


def check_median_and_upscale(defects=NONE):
    for h, w in SIZES:
        U = _levels(h, w)[4]
        M = ref.median3(U[0])
        for y in range(h):
            for x in range(w):
                nb = sorted(int(U[0, _clamp(y + a, 0, h - 1), _clamp(x + b, 0, w - 1)]) for a in (-1, 0, 1) for b in (-1, 0, 1))
                assert M[y, x] == nb[4], (h, w, y, x)
        H2, W2 = 2 * h - 1, 2 * w - 1                                             # odd: the last row and column have no partner
        up = ref.upscale(U, H2, W2, defects)
        for y in (0, 1, 2, H2 - 2, H2 - 1):
            for x in range(W2):
                assert up[0, y, x] == 2 * U[0, y >> 1, x >> 1] and up[1, y, x] == 2 * U[1, y >> 1, x >> 1]
        assert np.array_equal(ref.upscale(U, 2 * h, 2 * w, defects)[:, 1::2, 1::2], 2 * U)


def _update_loop(V1, V2, m1, m2, U, r, damping):
    H, W = V1.shape
    J, w2 = _sample_loop(V2, m2, U)
    T = np.zeros((9, H, W), dtype=object)
    for y in range(H):
        for x in range(W):
            xl, xr, yu, yd = max(x - 1, 0), min(x + 1, W - 1), max(y - 1, 0), min(y + 1, H - 1)
            if m1[y, x] & m1[y, xl] & m1[y, xr] & m1[yu, x] & m1[yd, x] & w2[y, x]:
                gx, gy, it = int(V1[y, xr] - V1[y, xl]), int(V1[yd, x] - V1[yu, x]), int(J[y, x] - V1[y, x])
                T[:, y, x] = (1, gx, gy, it, gx * gx, gx * gy, gy * gy, gx * it, gy * it)
    out, ok = np.zeros((2, H, W), np.int64), np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            s = [0] * 9
            for yy in range(max(y - r, 0), min(y + r, H - 1) + 1):
                for xx in range(max(x - r, 0), min(x + r, W - 1) + 1):
                    for k in range(9):
                        s[k] += T[k, yy, xx]
            dx, dy, o = _solve_scalar(*s, r, damping)
            out[:, y, x], ok[y, x] = (int(U[0, y, x]) + dx, int(U[1, y, x]) + dy), o
    return out, ok


def check_one_iteration(defects=NONE):
    for (h, w), r in zip(SIZES, (4, 2, 3)):
        V1, V2, m1, m2, U = _levels(h, w)
        U = U // 4
        want, ok = _update_loop(V1, V2, m1, m2, U, r, 65536)
        got, gok = ref.update(V1, V2, m1, m2, U, r, 65536, defects)
        assert np.array_equal(got, want) and np.array_equal(gok, ok) and 0 < ok.mean() and np.abs(want - U).max() > 8, (h, w)
        full, fok = ref.iterate(V1, V2, m1, m2, U, r, 65536, defects)
        assert np.array_equal(full, np.stack([ref.median3(want[0]), ref.median3(want[1])])) and np.array_equal(fok, ok)
        assert not np.array_equal(full, want)                                     # the median does something here


def check_schedule(defects=NONE):
    """the whole call against the stages applied by hand, and a shift that only the coarse levels can find"""
    a, b, m2, f = ref.flow_pair(64, 96, 6, seed=5)
    flow, sup, F = ref.dense_flow(a, b, None, m2, levels=3, iters=2, radius=3, damping=4096, defects=defects)
    V1, m1 = ref.level0(a, None)
    V2, mm2 = ref.level0(b, m2)
    V1s, m1s, V2s, m2s = *ref.pyramid(V1, m1, 3), *ref.pyramid(V2, mm2, 3)
    assert [v.shape for v in V1s] == [(64, 96), (32, 48), (16, 24)]
    U = np.zeros((2, 16, 24), np.int64)
    for l in (2, 1, 0):
        if l < 2:
            U = 2 * U[:, np.arange(V1s[l].shape[0])[:, None] >> 1, np.arange(V1s[l].shape[1])[None, :] >> 1]
        for _ in range(2):
            Un, ok = ref.update(V1s[l], V2s[l], m1s[l], m2s[l], U, 3, 4096)
            U = np.stack([ref.median3(Un[0]), ref.median3(Un[1])])
        assert np.array_equal(F["u"][l], U), l
    assert np.array_equal(flow, (U / 256).astype(np.float32)) and flow.dtype == np.float32 and np.array_equal(sup, ok)
    assert np.array_equal(flow.astype(np.float64) * 256, U)                        # exact in fp32
    e = ref.endpoint_error(flow, sup, f, m2[None], 6, margin=8)
    assert e[0] < e[2] / 3, e


CHECKS = (check_pyramid, check_bilinear_sample, check_gradients_and_window_sums, check_solve, check_median_and_upscale, check_one_iteration, check_schedule)


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
# (h, w, amplitude) -> the mean endpoint error measured with this restatement at the defaults (README.md, dense_flow, accuracy table)
MEASURED = {(192, 256, 3): 0.186, (192, 256, 8): 0.223, (512, 512, 3): 0.159, (512, 512, 8): 0.170}


@pytest.mark.parametrize("case", sorted(MEASURED), ids=lambda c: f"{c[0]}x{c[1]}_amp{c[2]}")
def test_accuracy_on_known_flows(case):
    h, w, amp = case
    a, b, m2, f = ref.flow_pair(h, w, amp, seed=3)
    assert not b[:, :, w - w // 5:].any() and not m2[:, :, w - w // 5:].any() and m2[:, :, :w - w // 5].all()
    flow, sup, _ = ref.dense_flow(a, b, None, m2, **ref.DEFAULTS)
    mean, p99, zero, n = ref.endpoint_error(flow, sup, f, m2[None], amp)
    print(f"{h}x{w} amplitude {amp}: mean {mean:.4f} px, 99th percentile {p99:.4f} px, zero flow {zero:.4f} px over {n} pixels")
    assert n > 0.4 * h * w and abs(np.abs(f).max() - amp) < 0.05 * amp
    assert mean < zero / 3
    assert mean < 3 * MEASURED[case] and p99 < 3.0
    assert not sup[:, w - w // 5 + 8:].any()                                       # nothing is supported inside image 2's hole


# ---- degenerate inputs ---------------------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs_and_their_support():
    h, w = 48, 64
    const = np.full((3, h, w), 90.0, np.float32)
    # constant images: no gradient, so A = C = damping n^2 and b = 0.  With damping > 0 the determinant is positive, so a pixel is supported iff n passes: with a
    # zero flow the last row and column have no four taps (x0 = W - 1), which leaves the bottom-right corner alone with n = 16 < 81 div 4 and every other pixel
    # supported with a zero step; with damping 0 the determinant is 0: unsupported everywhere.  The flow is 0 either way.
    corner = np.ones((h, w), np.uint8)
    corner[-1, -1] = 0
    flow, sup, _ = ref.dense_flow(const, const * 0.5)
    assert not flow.any() and np.array_equal(sup, corner)
    flow, sup, _ = ref.dense_flow(const, const * 0.5, damping=0)
    assert not flow.any() and not sup.any()
    a = _img(h, w, 4)
    flow, sup, F = ref.dense_flow(a, a)
    assert not flow.any() and np.array_equal(sup, corner) and all(not u.any() for u in F["u"])       # identical images: exactly 0 at every level
    flow, sup, F = ref.dense_flow(a, _img(h, w, 5), None, np.zeros((1, h, w), np.float32))
    assert not flow.any() and not sup.any() and not any(m.any() for m in F["m2"])  # image 2 fully masked: n = 0 everywhere
    b = _img(h, w, 4) * 0.85 + 10
    bad, fixed = a.copy(), a.copy()
    bad[:, 10:14, 10:14], fixed[:, 10:14, 10:14] = np.nan, 0
    bad[:, 20:22, 30:33], fixed[:, 20:22, 30:33] = np.inf, 255
    bad[:, 30, 5], fixed[:, 30, 5] = -np.inf, 0
    r1, r2 = ref.dense_flow(bad, b), ref.dense_flow(fixed, b)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1]) and np.isfinite(r1[0]).all()


# ---- entries and binary ------------------------------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_touching_the_gpu():
    import ctypes as C
    from stitch_amd._lib import lib
    base = 0x7f0000000000                                                   # never dereferenced on the host
    P = [base + (i << 36) for i in range(12)]
    B, H, W, L = 2, 33, 65, 3
    px = B * H * W
    n = C.c_int64(0)
    nref = C.cast(C.byref(n), C.c_void_p)
    wsb = lib.st_dense_flow_workspace_bytes
    assert wsb(B, H, W, L, nref) == 0
    need = n.value
    lpx = B * (33 * 65 + 17 * 33)
    assert need % 16 == 0 and 14 * lpx + 9 * px <= need <= 14 * lpx + 9 * px + 16 * 8
    assert wsb(B, H, W, 1, nref) == 0 and n.value < need and wsb(64, 1024, 1024, 8, nref) == 0 and 2 ** 30 < n.value < 2 ** 31
    for bad in ((0, H, W, L), (65, H, W, L), (B, 15, W, L), (B, H, 15, L), (B, 1025, W, L), (B, H, 1025, L), (B, H, W, 0), (B, H, W, 9), (-1, H, W, L)):
        assert wsb(*bad, nref) == 1001, bad
    assert wsb(B, H, W, L, None) == 1001
    off = (C.c_int64 * 28)()
    assert lib.st_dense_flow_workspace_layout(B, H, W, L, C.cast(off, C.c_void_p)) == 0 and off[0] == 2 and off[27] == need and off[1] == 0
    used = [off[1], off[9], off[17], off[2], off[10], off[18], off[25], off[26], off[27]]
    assert used == sorted(used) and all(v % 16 == 0 for v in used) and all(off[k + l] == -1 for k in (1, 9, 17) for l in range(2, 8))
    assert lib.st_dense_flow_workspace_layout(B, H, W, L, None) == 1001 and lib.st_dense_flow_workspace_layout(B, 15, W, L, C.cast(off, C.c_void_p)) == 1001

    def sweep(call, regions, outputs, bad_args):
        """nulls, shapes and parameters, and every output against every other operand: overlapping at its first and last byte"""
        for name in regions:
            if not name.startswith("mask"):
                assert call(**{name: None}) == 1001, name
        for kw in bad_args:
            assert call(**kw) == 1001, kw
        for a in outputs:
            for b in regions:
                if a != b:
                    pa, pb = regions[a], regions[b]
                    assert call(**{a: pb[0]}) == 1001 and call(**{a: pb[0] + pb[1] - 16}) == 1001 and call(**{a: pb[0] - pa[1] + 16}) == 1001, (a, b)

    shapes = [dict(B=0), dict(B=65), dict(H=15), dict(W=15), dict(H=1025), dict(W=1025), dict(B=-1)]
    masks = [dict(c1=0), dict(c1=2), dict(c2=4), dict(c2=-1)]
    params = [dict(levels=0), dict(levels=9), dict(iters=0), dict(iters=17), dict(radius=0), dict(radius=8), dict(damping=-1), dict(damping=(1 << 24) + 1)]

    # (a call that passes every check would launch: each sweep therefore keeps one argument bad -- a stream is never needed)
    def flow(img1=P[0], img2=P[1], mask1=P[2], mask2=P[3], flow=P[4], sup=P[5], ws=P[6], c1=1, c2=3, B=B, H=H, W=W, levels=L, iters=4, radius=4, damping=65536, nbytes=need):
        clean = (img1, img2, mask1, mask2, flow, sup, ws, c1, c2, B, H, W, levels, iters, radius, damping, nbytes) == (*P[:7], 1, 3, 2, 33, 65, 3, 4, 4, 65536, need)
        return lib.st_dense_flow(img1, img2, mask1, c1, mask2, c2, 0 if clean else B, H, W, levels, iters, radius, damping, flow, sup, ws, nbytes, None)
    assert flow() == 1001
    sweep(flow, dict(img1=(P[0], 12 * px), img2=(P[1], 12 * px), mask1=(P[2], 4 * px), mask2=(P[3], 12 * px), flow=(P[4], 8 * px), sup=(P[5], px), ws=(P[6], need)),
          ("flow", "sup", "ws"), shapes + masks + params + [dict(nbytes=need - 1), dict(nbytes=0), dict(ws=P[6] + 8), dict(H=H + 32), dict(B=B + 1), dict(levels=1, H=64)])
    # absent masks are accepted: the only bad argument left is the one under test
    assert flow(mask1=None, mask2=None, radius=8) == 1001 and flow(mask1=None, c1=7, iters=0) == 1001 and flow(mask1=None, mask2=None, flow=P[0]) == 1001

    def pyramid(img1=P[0], img2=P[1], mask1=P[2], mask2=P[3], ws=P[6], c1=1, c2=3, B=B, H=H, W=W, levels=L, nbytes=need):
        clean = (img1, img2, mask1, mask2, ws, c1, c2, B, H, W, levels, nbytes) == (P[0], P[1], P[2], P[3], P[6], 1, 3, 2, 33, 65, 3, need)
        return lib.st_dense_flow_pyramid(img1, img2, mask1, c1, mask2, c2, 0 if clean else B, H, W, levels, ws, nbytes, None)
    sweep(pyramid, dict(img1=(P[0], 12 * px), img2=(P[1], 12 * px), mask1=(P[2], 4 * px), mask2=(P[3], 12 * px), ws=(P[6], need)), ("ws",),
          shapes + masks + params[:2] + [dict(nbytes=need - 1), dict(ws=P[6] + 4), dict(H=H + 32)])

    def iterate(v1=P[0], v2=P[1], m1=P[2], m2=P[3], u=P[4], u_out=P[5], sup=P[6], ws=P[7], B=B, H=H, W=W, radius=4, damping=65536, nbytes=8 * px):
        clean = (v1, v2, m1, m2, u, u_out, sup, ws, B, H, W, radius, damping, nbytes) == (*P[:8], 2, 33, 65, 4, 65536, 8 * px)
        return lib.st_dense_flow_iterate(v1, v2, m1, m2, u, 0 if clean else B, H, W, radius, damping, u_out, sup, ws, nbytes, None)
    sweep(iterate, dict(v1=(P[0], 2 * px), v2=(P[1], 2 * px), m1=(P[2], px), m2=(P[3], px), u=(P[4], 8 * px), u_out=(P[5], 8 * px), sup=(P[6], px), ws=(P[7], 8 * px)),
          ("u_out", "sup", "ws"), shapes + params[4:] + [dict(nbytes=8 * px - 1), dict(ws=P[7] + 8), dict(H=H + 1)])


# kernel -> (LDS bytes, VGPRs) of the compiler's resource report (README.md, dense_flow, kernel table)
RESOURCES = {"df_luma_kernel": (0, 11), "df_down_kernel": (0, 20), "df_init_kernel": (0, 6), "df_iterate_kernel": (44244, 64), "df_median_kernel": (0, 27)}


def test_kernels_use_no_scratch_and_the_resources_of_the_readme():
    """from the compiler's metadata of csrc/dense_flow.hip, built with the library's own flags"""
    spec = importlib.util.spec_from_file_location("_stitch_build", os.path.join(ROOT, "seamless-through-breaking-rethinking-image-stitching-for-optimal-alignment_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert build.SOURCES["dense_flow.hip"] == ["-ffp-contract=off"]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "dense_flow.s")
        subprocess.check_call(build.compile_cmd("dense_flow.hip", out, ["-S", "--cuda-device-only"]), stderr=subprocess.DEVNULL)
        text = open(out).read()
    rep = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+)\n.*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)",
                         text, re.S):
        rep[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    assert len(rep) == len(RESOURCES), sorted(rep)
    assert "atomic" not in text.split(".amdgpu_metadata")[0]
    readme = open(os.path.join(ROOT, "README.md")).read()
    table = readme[readme.index("## dense_flow"):]
    table = table[:table.index("\nMeasurements (")]                               # (the measurements have a table of kernel rows of their own)
    for key, (lds, vgpr) in RESOURCES.items():
        (name, r), = [(n, r) for n, r in rep.items() if key in n]
        print(key, r)
        assert r["lds"] == lds <= 65536 and r["vgpr"] == vgpr <= 256, (name, r)
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
        row, = [ln for ln in table.splitlines() if ln.startswith(f"| `{key}`")]
        assert f"| {lds} |" in row and f"| {vgpr} |" in row, row
