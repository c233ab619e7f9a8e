"""Exposure compensation without a GPU: the CPU restatement of the contract (tests/_exposure_ref.py) against a brute-force loop,
numpy.linalg.solve, the closed form of the minimiser and a sample-by-sample scalar form; the property the feature is wanted for on the
smooth scene of tests/test_multiband_cpu.py; nine planted defects, each of which must fail one of those assertions; the C entries'
argument checks and the kernels' register / LDS / scratch metadata."""
import importlib.util
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _exposure_ref as ref
import _multiband_ref as mb
from _multiband_cases import mask_cases, noise_pair, quads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = frozenset()
f32 = np.float32


# ---- statistics ---------------------------------------------------------------------------------------------------------------------------
def brute_stats(img1, img2, k1, k2, block):
    """pixel by pixel in Python integers"""
    _, H, W = img1.shape
    Th, Tw = -(-H // block), -(-W // block)
    rec = np.zeros((Th, Tw, 9), np.int64)
    for y in range(H):
        for x in range(W):
            if not (k1[0, y, x] > 0.5 and k2[0, y, x] > 0.5):
                continue
            r = rec[y // block, x // block]
            r[0] += 1
            for base, img in ((1, img1), (5, img2)):
                p = [int(min(max(float(img[c, y, x]), 0.0), 255.0)) for c in range(3)]          # int(): toward zero
                for c in range(3):
                    r[base + c] += p[c]
                r[base + 3] += (19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 0x8000) >> 16
    return rec


def check_stats(defects=NONE):
    for H, W in ((1, 1), (1, 9), (9, 1), (7, 7), (16, 16), (17, 33), (33, 70)):
        img1, img2 = noise_pair(H, W, 100 + H)
        if H * W >= 500:
            assert img1.min() < 0 and img1.max() > 255 and (img1 != np.trunc(img1)).any()
        for name, (k1, k2) in mask_cases(H, W).items():
            for block in (8, 32):
                got = ref.stats(img1, img2, k1, k2, block, defects)
                assert got.shape == (-(-H // block), -(-W // block), 9)
                assert np.array_equal(got, brute_stats(img1, img2, k1, k2, block)), (H, W, name, block)
    # the luma rounds: a grey pixel keeps its value (19595 + 38470 + 7471 = 65536), which the sum without the 0x8000 term loses
    grey = np.full((3, 4, 4), 200.0, f32)
    one = np.ones((1, 4, 4), f32)
    assert ref.stats(grey, grey, one, one, 8, defects)[0, 0].tolist() == [16] + [3200] * 8


# ---- the solve ----------------------------------------------------------------------------------------------------------------------------
def check_solve(defects=NONE):
    rng = np.random.default_rng(20260102)
    for k in range(200):
        N = int(rng.integers(1, 4097))
        S1, S2 = int(N * rng.uniform(1, 255)), int(N * rng.uniform(1, 255))
        G1, G2 = (1.0, 1.0) if k % 2 else (float(f32(rng.uniform(0.5, 2))), float(f32(rng.uniform(0.5, 2))))
        # the system's condition number is 1 + (alpha / beta) (a^2 + b^2) <= 1 + (0.3 / 5)^2 * 2 * 255^2 = 469 here (164 at the defaults), so
        # either solver is within a few 469 * 2^-53 = 5e-14 of the solution: 1e-12 separates a wrong formula from rounding
        sn, sg = (10.0, 0.1) if k % 4 < 2 else (float(rng.uniform(5, 30)), float(rng.uniform(0.05, 0.3)))
        alpha, beta = ref.weights(sn, sg)
        g = np.array(ref.solve64(N, S1, S2, G1, G2, alpha, beta))
        n2 = float(N) ** 2
        A = np.array([[alpha * S1 * S1 + beta * n2, -alpha * S1 * S2], [-alpha * S1 * S2, alpha * S2 * S2 + beta * n2]])
        want = np.linalg.solve(A, np.array([beta * n2 * G1, beta * n2 * G2]))
        assert np.abs(g - want).max() <= 1e-12 * np.abs(want).max(), (k, g, want)
        # the minimiser of alpha (g1 a - g2 b)^2 + beta ((G1 - g1)^2 + (G2 - g2)^2) over the overlap means a, b leaves the residual
        # g1 a - g2 b = (G1 a - G2 b) / (1 + (alpha / beta) (a^2 + b^2))
        a, b = S1 / N, S2 / N
        if abs(G1 * a - G2 * b) > 1e-3:
            shrink = (g[0] * a - g[1] * b) / (G1 * a - G2 * b)
            assert abs(shrink - 1 / (1 + alpha / beta * (a * a + b * b))) <= 1e-9, k
    alpha, beta = ref.weights()
    # equal sums: the float64 value is 1 - 2^-52, the fp32 gain exactly 1
    g1, g2 = ref.solve64(3000, 3000 * 131, 3000 * 131, 1.0, 1.0, alpha, beta)
    assert abs(g1 - 1) <= 2.0 ** -51 and abs(g2 - 1) <= 2.0 ** -51
    assert ref.solve(3000, 3000 * 131, 3000 * 131, 1.0, 1.0, alpha, beta) == (f32(1), f32(1))
    assert ref.solve(0, 0, 0, 1.25, 0.75, alpha, beta) == (f32(1.25), f32(0.75))                # N = 0: the prior
    assert ref.solve(100, 0, 0, 1.25, 0.75, alpha, beta) == (f32(1.25), f32(0.75))              # black overlap (S = 0): the prior, det = (beta n2)^2
    # a weak prior lets image 1's gain fall below 0.25 (g1 -> 1 - a (a - b) / (a^2 + b^2)): clamped; above 4 only a prior above 4 leads
    a, b = ref.weights(10.0, 1000.0)
    raw = ref.solve64(1000, 1000 * 250, 1000 * 2, 1.0, 1.0, a, b)
    assert 0 < raw[0] < 0.25 and ref.solve(1000, 1000 * 250, 1000 * 2, 1.0, 1.0, a, b) == (f32(0.25), f32(raw[1]))
    raw = ref.solve64(1000, 1000 * 90, 1000 * 90, 6.0, 5.0, alpha, beta)
    assert raw[0] > 4 and raw[1] > 4 and ref.solve(1000, 1000 * 90, 1000 * 90, 6.0, 5.0, alpha, beta) == (f32(4), f32(4))


def check_identity(defects=NONE):
    H, W = 40, 70
    img, other = noise_pair(H, W, 5)
    k1, k2 = quads(H, W)
    p = ref.to_u8(img).astype(f32)
    for mode in ("gain", "blocks"):
        for channels in (False, True):
            o1, o2, t = ref.compensate(img, img, k1, k2, mode, 8, channels, defects=defects)        # equal images: gains exactly 1, pixels back
            assert (t == 1).all() and np.array_equal(o1, p) and np.array_equal(o2, p), (mode, channels)
            for name in ("disjoint", "both_empty", "m2_empty"):                                      # empty overlap: the truncated inputs
                e1, e2 = mask_cases(H, W)[name]
                o1, o2, t = ref.compensate(img, other, e1, e2, mode, 8, channels, defects=defects)
                assert (t == 1).all() and np.array_equal(o1, p) and np.array_equal(o2, ref.to_u8(other).astype(f32)), (mode, channels, name)


# ---- blocks mode --------------------------------------------------------------------------------------------------------------------------
def gain_scene(H=70, W=100, seed=6, gain2=0.7):
    """noise under two quadrilaterals, image 2 darker and with a gradient: the tile gains differ and the global gains are not 1"""
    rng = np.random.default_rng(seed)
    base = rng.random((3, H, W)) * 200 + 30
    ramp = 1 + 0.3 * np.linspace(-1, 1, W)[None, None, :]
    k1, k2 = quads(H, W)
    return base.astype(f32), (base * gain2 * ramp + rng.random((3, H, W)) * 4).astype(f32), k1, k2


def scalar_smooth(t, times):
    """(0.25, 0.5, 0.25) sample by sample in np.float32 scalars: along W, rounded, then along H; indices clamped"""
    q, h = f32(0.25), f32(0.5)

    def one(v):
        n = len(v)
        return [(q * v[max(i - 1, 0)] + h * v[i]) + q * v[min(i + 1, n - 1)] for i in range(n)]
    t = np.asarray(t, f32)
    for _ in range(times):
        rows = np.array([one(list(r)) for r in t], dtype=f32)
        t = np.array([one(list(c)) for c in rows.T], dtype=f32).T
    return t


def scalar_gain(table, y, x, block):
    Th, Tw = table.shape
    one = f32(1)

    def coord(v, n):
        u = (f32(v) + f32(0.5)) / f32(block) - f32(0.5)
        i0 = int(np.floor(u))
        return min(max(i0, 0), n - 1), min(max(i0 + 1, 0), n - 1), f32(u - f32(i0))
    y0, y1, fy = coord(y, Th)
    x0, x1, fx = coord(x, Tw)
    return (table[y0, x0] * (one - fx) + table[y0, x1] * fx) * (one - fy) + (table[y1, x0] * (one - fx) + table[y1, x1] * fx) * fy


def scalar_finish(p, g):
    return min(f32(np.floor(f32(f32(p) * f32(g)) + f32(0.5))), f32(255))


def rounding_pairs():
    """(p, g) where p g + 0.5 lies within half an fp32 step below 1: only the product rounded on its own reaches 1.  (With g >= 0.25, as the
    gain clamp leaves it, p g + 0.5 changes binade only at p = 1, where the product is exact.)"""
    ps, gs = [], []
    for p in range(2, 256):
        g = f32(0.5) / f32(p)
        for _ in range(8):
            g = np.nextafter(g, f32(0))
            ps.append(p), gs.append(g)
    return np.array(ps, f32), np.array(gs, f32)


def check_blocks(defects=NONE):
    img1, img2, k1, k2 = gain_scene()
    alpha, beta = ref.weights()
    for block, channels in ((8, False), (8, True), (16, False), (32, False)):
        rec = ref.stats(img1, img2, k1, k2, block, defects)
        G = ref.global_gains(rec, alpha, beta)
        assert (np.abs(G - 1) > 0.02).all()
        ids = (0, 1, 2) if channels else (3,)
        mc = block * block // 8
        raw = ref.tile_gains(rec, G, ids, mc, alpha, beta, defects)
        few = rec[..., 0] < mc
        assert few.any() and (~few).any() and ((rec[..., 0] > 0) & few).any()                       # empty tiles, sparse tiles, solved tiles
        for s, p in enumerate(ids):
            for im in range(2):
                assert (raw[s, im][few] == G[p, im]).all(), (block, channels)                         # below min_count: the global gain
                assert (raw[s, im][~few] != G[p, im]).any()
        assert np.array_equal(ref.tile_gains(rec, G, ids, 0, alpha, beta, defects)[..., rec[..., 0] == 0],
                              raw[..., rec[..., 0] == 0])                                             # min_count 0: only the empty tiles keep it
        for times in (0, 1, 2, 3):
            sm = ref.smooth(raw, times, defects)
            assert sm.dtype == f32
            for s in range(len(ids)):
                for im in range(2):
                    assert np.array_equal(sm[s, im], scalar_smooth(raw[s, im], times)), (block, times)
        tables = ref.gain_tables(img1, img2, k1, k2, "blocks", block, channels, defects=defects)
        assert np.array_equal(tables, ref.smooth(raw, 2, defects))
    # interpolation and the apply step, sample by sample: a 3 x 4 table of block 8 over a 21 x 30 canvas (ragged), a 1 x 1 table, a table
    # smaller and one larger than the canvas' grid
    rng = np.random.default_rng(8)
    H, W = 21, 30
    a, b = noise_pair(H, W, 9)
    for th, tw, block in ((3, 4, 8), (1, 1, 8), (2, 2, 8), (5, 6, 8), (1, 2, 32), (2, 1, 16)):
        t = (rng.random((1, 2, th, tw)) * 2.5 + 0.3).astype(f32)
        g = [ref.interpolate(t[0, im], H, W, block, defects) for im in range(2)]
        o1, o2 = ref.apply(a, b, t, block, defects)
        assert o1.dtype == f32 and o1.shape == (3, H, W)
        for im, (img, o) in enumerate(((a, o1), (b, o2))):
            p = ref.to_u8(img)
            for y in range(H):
                for x in range(W):
                    sg = scalar_gain(t[0, im], y, x, block)
                    assert g[im][y, x] == sg, (th, tw, block, y, x)
                    for c in range(3):
                        assert o[c, y, x] == scalar_finish(p[c, y, x], sg), (th, tw, block, c, y, x)
    # the clamp at 255 and the two roundings of p g + 0.5
    white = np.full((3, 4, 4), 255.0, f32)
    o1, _ = ref.apply(white, white, np.full((1, 2, 1, 1), 1.5, f32), 8, defects)
    assert (o1 == 255).all()
    ps, gs = rounding_pairs()
    want = np.array([scalar_finish(p, g) for p, g in zip(ps, gs)], f32)
    assert (want == 1).any() and (want == 0).any()
    assert np.array_equal(ref.finish(ps, gs, defects), want)
    # per-channel tables reach their own channel
    t3 = (rng.random((3, 2, 3, 4)) + 0.5).astype(f32)
    o1, o2 = ref.apply(a, b, t3, 8, defects)
    for c in range(3):
        c1, c2 = ref.apply(a, b, t3[c:c + 1], 8, defects)
        assert np.array_equal(o1[c], c1[c]) and np.array_equal(o2[c], c2[c])


CHECKS = (check_stats, check_solve, check_identity, check_blocks)


def test_statistics_equal_a_brute_force_loop():
    check_stats()


def test_solve_equals_the_normal_equations_and_the_closed_form():
    check_solve()


def test_equal_images_and_an_empty_overlap_come_back_truncated():
    check_identity()


def test_blocks_mode_smoothing_interpolation_and_apply_equal_the_scalar_form():
    check_blocks()


@pytest.mark.parametrize("defect", ref.DEFECTS)
def test_a_planted_defect_fails_an_assertion(defect):
    failed = []
    for check in CHECKS:
        try:
            check(frozenset({defect}))
        except AssertionError:
            failed.append(check.__name__)
    assert failed, f"no assertion notices {defect}"


# ---- the scene of tests/test_multiband_cpu.py ----------------------------------------------------------------------------------------------
def test_compensation_narrows_the_gain_difference_on_the_smooth_scene():
    """120 x 220, image 2 at 0.8 x the gain of image 1.  The ratio of the overlap means moves toward 1 with the default prior (sigma_g = 0.1)
    and further with a weak one (sigma_g = 1); the far-field difference -- the multiband output's mean 64 px left of the seam minus its mean
    64 px right of it, less the same difference of the scene -- is smaller with compensation in front of the blend than without."""
    H, W = 120, 220
    y, x = np.mgrid[:H, :W].astype(np.float64)
    scene = np.stack([128 + 80 * np.sin(x / 37 + y / 53), 128 + 60 * np.cos(x / 29), 100 + 0.3 * x])
    m1 = (x < 130) & (y > 10) & (y < 110)
    m2 = (x > 70 + 0.2 * y) & (y > 20) & (y < 118) & (x < 215)
    img1, img2 = scene.astype(f32), (0.8 * scene).astype(f32)
    k1, k2 = m1[None].astype(f32), m2[None].astype(f32)
    O = m1 & m2

    def ratio(a, b):
        return a[:, O].mean() / b[:, O].mean()

    _, _, Wf, U = mb.fields(img1, img2, k1, k2)
    rows = [r for r in range(30, 100)]
    seam = {r: int(np.nonzero((Wf[r] < 0.5) & U[r])[0].min()) for r in rows}
    assert all(seam[r] - 68 >= 0 and m1[r, seam[r] - 68] and m2[r, seam[r] + 67] for r in rows)

    def far_field(img):
        left = np.mean([img[:, r, seam[r] - 68:seam[r] - 60].mean() for r in rows])
        right = np.mean([img[:, r, seam[r] + 60:seam[r] + 68].mean() for r in rows])
        return left - right

    own = far_field(scene)
    r0 = ratio(ref.to_u8(img1).astype(f32), ref.to_u8(img2).astype(f32))
    plain = far_field(mb.blend(img1, img2, k1, k2, 5)) - own
    print(f"exposure scene: uncompensated overlap-mean ratio {r0:.4f}, far-field difference {plain:.2f} grey levels")
    for mode in ("gain", "blocks"):
        res = {}
        for sg in (0.1, 1.0):
            o1, o2, t = ref.compensate(img1, img2, k1, k2, mode, sigma_g=sg)
            res[sg] = (ratio(o1, o2), far_field(mb.blend(o1, o2, k1, k2, 5)) - own)
            print(f"exposure scene: {mode}, sigma_g {sg}: gains {t[0, 0].mean():.4f} / {t[0, 1].mean():.4f}, overlap-mean ratio {res[sg][0]:.4f}, "
                  f"far-field difference {res[sg][1]:.2f} grey levels")
        assert abs(res[1.0][0] - 1) < abs(res[0.1][0] - 1) < abs(r0 - 1), mode
        assert abs(res[0.1][1]) < abs(plain) and abs(res[1.0][1]) < abs(plain), mode


# ---- entries and binary --------------------------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_touching_the_gpu():
    from stitch_amd._lib import lib
    base = 0x7f0000000000                                                   # never dereferenced on the host
    img1, img2, k1, k2, out1, out2, ws, gains = (base + (i << 32) for i in range(8))
    H, W = 37, 53
    wsb = lib.st_exposure_workspace_bytes
    need = wsb(H, W, 8)
    assert need >= 4 * 9 * 5 * 7 + 32 + 2 * 4 * 6 * 5 * 7 and need % 16 == 0
    assert wsb(0, 5, 32) == 0 and wsb(5, 0, 32) == 0 and wsb(4097, 5, 32) == 0 and wsb(5, 4097, 32) == 0
    assert all(wsb(5, 5, b) == 0 for b in (-8, 0, 1, 4, 12, 24, 33, 128)) and all(wsb(4096, 4096, b) > 0 for b in (8, 16, 32, 64))
    nimg, nmask = 12 * H * W, 4 * H * W

    def comp(img1=img1, img2=img2, k1=k1, k2=k2, H=H, W=W, mode=1, block=8, channels=0, min_count=8, smooth=2, sn=10.0, sg=0.1, out1=out1, out2=out2,
             gains=gains, ws=ws, nbytes=need):
        return lib.st_exposure_compensate(img1, img2, k1, k2, H, W, mode, block, channels, min_count, smooth, sn, sg, out1, out2, gains, ws, nbytes, None)
    for name in ("img1", "img2", "k1", "k2", "out1", "out2", "ws"):
        assert comp(**{name: None}) == 1001, name
    big = 1 << 40
    assert comp(H=0) == 1001 and comp(W=0) == 1001 and comp(H=4097, nbytes=big) == 1001 and comp(W=4097, nbytes=big) == 1001
    assert all(comp(block=b, nbytes=big) == 1001 for b in (0, 4, 12, 128, -8))
    assert comp(mode=-1) == 1001 and comp(mode=2) == 1001
    assert comp(smooth=-1) == 1001 and comp(smooth=9) == 1001 and comp(min_count=-1) == 1001
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-200, 1e200):     # (the last two: 1 / sigma^2 leaves fp64)
        assert comp(sn=bad) == 1001 and comp(sg=bad) == 1001, bad
    assert comp(nbytes=need - 1) == 1001 and comp(ws=ws + 8) == 1001
    # an output may be its own input and nothing else
    assert comp(out1=img1 + 4) == 1001 and comp(out1=img1 - 4) == 1001 and comp(out2=img2 + nimg - 4) == 1001
    assert comp(out1=img2) == 1001 and comp(out2=img1) == 1001 and comp(out1=out2) == 1001 and comp(out1=out2 + nimg - 4) == 1001
    assert comp(out1=k1) == 1001 and comp(out2=k2 + nmask - 4) == 1001 and comp(out2=k1 - nimg + 4) == 1001

    def stats(img1=img1, img2=img2, k1=k1, k2=k2, H=H, W=W, block=8, rec=ws):
        return lib.st_exposure_stats(img1, img2, k1, k2, H, W, block, rec, None)
    for name in ("img1", "img2", "k1", "k2", "rec"):
        assert stats(**{name: None}) == 1001, name
    assert stats(H=0) == 1001 and stats(W=4097) == 1001 and stats(block=9) == 1001

    def apply(img1=img1, img2=img2, t=gains, th=5, tw=7, H=H, W=W, block=8, out1=out1, out2=out2):
        return lib.st_exposure_apply(img1, img2, t, th, tw, H, W, block, 0, out1, out2, None)
    for name in ("img1", "img2", "t", "out1", "out2"):
        assert apply(**{name: None}) == 1001, name
    assert apply(H=0) == 1001 and apply(W=4097) == 1001 and apply(block=9) == 1001 and apply(th=0) == 1001 and apply(tw=4097) == 1001
    assert apply(out1=img1 + 4) == 1001 and apply(out2=img1) == 1001 and apply(out1=out2) == 1001


def test_kernels_use_no_scratch_and_the_stated_lds():
    """from the compiler's metadata of csrc/exposure.hip, built with the library's own flags (README.md, exposure compensation, kernel table)"""
    spec = importlib.util.spec_from_file_location("_stitch_build", os.path.join(ROOT, "seamless-through-breaking-rethinking-image-stitching-for-optimal-alignment_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert build.SOURCES["exposure.hip"] == ["-ffp-contract=off"]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "exposure.s")
        subprocess.check_call(build.compile_cmd("exposure.hip", out, ["-S", "--cuda-device-only"]), stderr=subprocess.DEVNULL)
        text = open(out).read()
    rep = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+)\n.*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)",
                         text, re.S):
        rep[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    lds = {"ec_stats_kernel": [144], "ec_global_kernel": [1224], "ec_tile_gain_kernel": [0], "ec_smooth_kernel": [0], "ec_apply_kernel": [0, 0]}
    assert len(rep) == sum(len(v) for v in lds.values()), sorted(rep)
    for key, want in lds.items():
        found = [(n, r) for n, r in rep.items() if key in n]
        assert [r["lds"] for _, r in found] == want, found
        for name, r in found:
            assert r["scratch"] == 0 and r["spill"] == 0 and r["vgpr"] <= 64, (name, r)
