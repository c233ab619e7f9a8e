"""multiband_fusion without a GPU: the CPU restatement of the contract (tests/_multiband_ref.py) against brute force, scipy and a float64
pyramid built from scipy's correlate1d; the properties the blend is wanted for; nine planted defects, each of which must fail one of
those assertions; the C entries' argument checks and the kernels' register / scratch metadata."""
import importlib.util
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
from scipy import ndimage

import _multiband_bounds as bounds
import _multiband_ref as ref
from _multiband_cases import edt_cases, mask_cases, noise_pair, quads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = frozenset()


def brute_edt(m, border):
    """D and, per pixel, the lowest row-major index among the canvas sites at distance D (-1: none / only the ring)"""
    H, W = m.shape
    mp = np.pad(m, 1, constant_values=True)
    if border:
        mp[0, :] = mp[-1, :] = mp[:, 0] = mp[:, -1] = False
    ys, xs = np.nonzero(~mp)
    ys, xs = ys - 1, xs - 1
    inside = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
    flat = np.where(inside, ys * W + xs, np.iinfo(np.int64).max)
    D = np.full((H, W), ref.INT32_MAX, np.int64)
    I = np.full((H, W), -1, np.int64)
    if len(ys) == 0:
        return D, I
    for y in range(H):
        for x in range(W):
            d = (ys - y) ** 2 + (xs - x) ** 2
            D[y, x] = d.min()
            eq = flat[d == d.min()].min()
            I[y, x] = -1 if eq == np.iinfo(np.int64).max else eq
    return D, I


def check_edt(defects=NONE):
    for name, m in edt_cases():
        for border in (True, False):
            D, I = ref.edt_sq(m, border, True, defects=defects)
            bD, bI = brute_edt(m, border)
            assert D.dtype == np.int32 and I.dtype == np.int32
            assert np.array_equal(D, bD), (name, border)
            assert np.array_equal(I, bI), (name, border)                   # a site at distance D, the lowest index among the equals
            assert np.array_equal(ref.edt_sq(m, border, defects=defects), D)
            if border or not m.all():                                      # scipy needs a site; the ring is modelled by padding
                mp = np.pad(m, 1, constant_values=not border)
                if border:
                    mp[0, :] = mp[-1, :] = mp[:, 0] = mp[:, -1] = False
                s = ndimage.distance_transform_edt(mp)[1:-1, 1:-1]
                assert np.array_equal(np.rint(s * s).astype(np.int64), D), (name, border)


def check_fields(defects=NONE):
    """ownership and extension against brute force: integers only"""
    H, W = 13, 17
    img1, img2 = noise_pair(H, W, 1)
    a, b = ref.to_u8(img1), ref.to_u8(img2)
    assert a.min() == 0 and a.max() == 255 and np.array_equal(a, np.trunc(a))
    for name, (k1, k2) in mask_cases(H, W).items():
        I1f, I2f, Wf, U = ref.fields(img1, img2, k1, k2, defects=defects)
        m1, m2 = k1[0] > 0.5, k2[0] > 0.5
        D1, D2 = brute_edt(m1, True)[0], brute_edt(m2, True)[0]
        W1 = m1 & (~m2 | (D1 >= D2))                                        # ties go to image 1
        assert np.array_equal(U, m1 | m2)
        if not U.any():
            assert not I1f.any() and not I2f.any() and not Wf.any()
            continue
        _, near = brute_edt(~U, False)                                      # the canvas ring is not a site here
        q = np.where(U, np.arange(H * W).reshape(H, W), near)
        C = np.where(W1[None], a, b).reshape(3, -1)[:, q]
        assert np.array_equal(Wf, W1.reshape(-1)[q].astype(np.float32)), name
        assert np.array_equal(I1f, np.where(m1[None], a, C)), name
        assert np.array_equal(I2f, np.where(m2[None], b, C)), name
        hard = ref.blend(img1, img2, k1, k2, 0, defects=defects)            # levels = 0: the hard-seam composite, exact
        assert np.array_equal(hard, np.where(U[None], np.where(W1[None], a, b), 0)), name


def scalar_reduce2(a):
    """REDUCE written out sample by sample in np.float32 scalars: along W, rounded, then along H"""
    f = np.float32
    g = [f(v) for v in ref.G5]

    def one(v):
        n = len(v)
        out = []
        for i in range((n + 1) // 2):
            t = [v[min(max(2 * i + k - 2, 0), n - 1)] for k in range(5)]
            out.append((((g[0] * t[0] + g[1] * t[1]) + g[2] * t[2]) + g[3] * t[3]) + g[4] * t[4])
        return out
    rows = np.array([one(list(r)) for r in a], dtype=f)
    return np.array([one(list(c)) for c in rows.T], dtype=f).T


def scalar_expand2(a, h, w):
    f = np.float32

    def one(v, n):
        m = len(v)
        out = []
        for j in range(n):
            c = j >> 1
            lo, hi = v[max(c - 1, 0)], v[min(c + 1, m - 1)]
            out.append(v[c] * f(0.5) + hi * f(0.5) if j & 1 else (lo * f(0.125) + v[c] * f(0.75)) + hi * f(0.125))
        return out
    rows = np.array([one(list(r), w) for r in a], dtype=f)
    return np.array([one(list(c), h) for c in rows.T], dtype=f).T


def check_filters(defects=NONE):
    """REDUCE and EXPAND bit for bit against the sample-by-sample scalar form (taps, clamped border, order of the sums, W before H)"""
    rng = np.random.default_rng(2)
    for H, W in ((1, 1), (1, 6), (5, 1), (7, 9), (6, 8)):
        a = (rng.random((H, W)) * 255).astype(np.float32)
        r = ref.reduce2(a, defects)
        assert r.dtype == np.float32 and r.shape == ((H + 1) // 2, (W + 1) // 2)
        assert np.array_equal(r, scalar_reduce2(a)), (H, W)
        assert np.array_equal(ref.expand2(r, H, W, defects), scalar_expand2(r, H, W)), (H, W)


def scipy_blend64(img1, img2, k1, k2, levels, truncate=True):
    """the pyramid in float64 from scipy.ndimage.correlate1d(mode='nearest'): REDUCE = correlate with g, every second sample; EXPAND = each
    coarse sample twice, correlate with (0, 0.125, 0.375, 0.375, 0.125) -- the same taps and the same clamped border, written differently"""
    I1f, I2f, Wf, U = ref.fields(img1, img2, k1, k2, np.float64, truncate=truncate)

    def red(a):
        for ax in (-1, -2):
            a = np.take(ndimage.correlate1d(a, ref.G5, axis=ax, mode="nearest"), np.arange(0, a.shape[ax], 2), axis=ax)
        return a

    def exp(a, h, w):
        for ax, n in ((-1, w), (-2, h)):
            a = np.take(ndimage.correlate1d(np.repeat(a, 2, axis=ax), [0, 0.125, 0.375, 0.375, 0.125], axis=ax, mode="nearest"), np.arange(n), axis=ax)
        return a
    Ga, Gb, Gw = [I1f], [I2f], [Wf]
    for _ in range(ref.effective_levels(*Wf.shape, levels)):
        Ga.append(red(Ga[-1])), Gb.append(red(Gb[-1])), Gw.append(red(Gw[-1]))
    R = Gb[-1] + Gw[-1] * (Ga[-1] - Gb[-1])
    for l in range(len(Ga) - 2, -1, -1):
        h, w = Gw[l].shape
        La, Lb = Ga[l] - exp(Ga[l + 1], h, w), Gb[l] - exp(Gb[l + 1], h, w)
        R = exp(R, h, w) + (Lb + Gw[l] * (La - Lb))
    return np.where(U[None], np.clip(R, 0, 255), 0)


def check_pyramid(defects=NONE, sizes=((96, 200),), report=None):
    """float32 restatement within the a priori bound of the float64 evaluation (uniform noise)"""
    for H, W in sizes:
        img1, img2 = noise_pair(H, W, 3, 0.0, 256.0)
        k1, k2 = quads(H, W)
        for L in (1, 2, 3, 5):
            want = scipy_blend64(img1, img2, k1, k2, L)
            got = ref.blend(img1, img2, k1, k2, L, defects=defects)
            assert got.dtype == np.float32
            err = np.abs(got.astype(np.float64) - want).max()
            bound = bounds.pyramid_bound(ref.effective_levels(H, W, L))
            if report is not None:
                report.append((H, W, L, err, bound))
            assert err <= bound, (H, W, L, err, bound)
            assert np.abs(ref.blend(img1, img2, k1, k2, L, np.float64, defects=defects) - want).max() <= 1e-9, (H, W, L)


def check_properties(defects=NONE):
    H, W = 48, 64
    img, other = noise_pair(H, W, 4)
    k1, k2 = quads(H, W)
    U = (k1[0] > 0.5) | (k2[0] > 0.5)
    for L in (1, 3, 5):
        bound = bounds.pyramid_bound(ref.effective_levels(H, W, L))
        # identical images come back inside U (the Laplacian pyramid reconstructs exactly; what is left is fp32 rounding) ...
        out = ref.blend(img, img, k1, k2, L, defects=defects)
        assert np.abs(out - ref.to_u8(img))[:, U].max() <= bound, L
        assert not out[:, ~U].any()
        # ... and La - Lb cancels exactly, so the weights do not touch a single bit: the same output as with both masks = U
        u = U[None].astype(np.float32)
        assert np.array_equal(out, ref.blend(img, img, u, u, L, defects=defects)), L
        # the output never leaves 0..255, whatever the Laplacians overshoot to
        rng = np.random.default_rng(5)
        hard1, hard2 = (rng.random((3, H, W)) < 0.5) * 255.0, (rng.random((3, H, W)) < 0.5) * 255.0
        out = ref.blend(hard1, hard2, k1, k2, L, defects=defects)
        assert out.min() >= 0 and out.max() <= 255, L
        unclamped = ref.blend(hard1, hard2, k1, k2, L, defects=frozenset(defects) | {"no_final_clamp"})
        assert unclamped.min() < 0 or unclamped.max() > 255                 # (the case does exercise the clamp)
    # two constant images across a straight seam: every row monotone, and beyond 2^(L+2) px from the seam the pixel's own image
    H, W, seam = 6, 300, 150
    a, b = np.full((3, H, W), 200.0), np.full((3, H, W), 40.0)
    for L in (1, 3, 5):
        wf = np.broadcast_to(np.arange(W) < seam, (H, W))
        r64 = ref.pyramid_blend(a, b, wf.astype(np.float64), L, defects)
        assert (np.diff(r64, axis=-1) <= 1e-9).all(), L
        r32 = ref.pyramid_blend(a.astype(np.float32), b.astype(np.float32), wf.astype(np.float32), L, defects)
        far, bound = 2 ** (L + 2), bounds.pyramid_bound(L)
        assert np.abs(r32[..., :seam - far] - 200).max() <= bound and np.abs(r32[..., seam + far:] - 40).max() <= bound, L


CHECKS = (check_edt, check_fields, check_filters, check_pyramid, check_properties)


def test_edt_restatement_equals_brute_force_and_scipy():
    check_edt()


def test_ownership_and_extension_equal_brute_force():
    check_fields()


def test_reduce_and_expand_equal_the_scalar_form():
    check_filters()


def test_float32_pyramid_is_within_the_derived_bound_of_float64():
    report = []
    check_pyramid(report=report)
    for H, W, L, err, bound in report:
        print(f"multiband pyramid {H}x{W} L={L}: |f32 - f64| = {err:.3e} grey levels, bound {bound:.3e}")
    assert all(b < 0.05 for *_, b in report)                               # the bound itself stays far below one grey level


def test_properties():
    check_properties()


def _largest_step(img, keep):
    """largest |difference| between 4-neighbours that both lie in `keep`"""
    dx = np.abs(np.diff(img, axis=-1))[:, keep[:, 1:] & keep[:, :-1]]
    dy = np.abs(np.diff(img, axis=-2))[:, keep[1:, :] & keep[:-1, :]]
    return max(dx.max(), dy.max())


def test_seam_step_on_a_smooth_scene_with_a_gain_difference():
    """120 x 220, image 2 at 0.8 x the gain of image 1, float64, pixels not truncated: at L = 5 the largest neighbour step more than 8 px
    inside the union is at most 1.25 x the scene's own, where ave_fusion's is at least 5 x."""
    H, W = 120, 220
    y, x = np.mgrid[:H, :W].astype(np.float64)
    scene = np.stack([128 + 80 * np.sin(x / 37 + y / 53), 128 + 60 * np.cos(x / 29), 100 + 0.3 * x])
    m1 = (x < 130) & (y > 10) & (y < 110)
    m2 = (x > 70 + 0.2 * y) & (y > 20) & (y < 118) & (x < 215)
    img1, img2 = scene, 0.8 * scene
    k1, k2 = m1[None].astype(np.float32), m2[None].astype(np.float32)
    keep = ref.edt_sq(m1 | m2, True) > 64
    own = _largest_step(scene, keep)
    multi = _largest_step(ref.blend(img1, img2, k1, k2, 5, np.float64, truncate=False), keep)
    hard = _largest_step(ref.blend(img1, img2, k1, k2, 0, np.float64, truncate=False), keep)
    with np.errstate(invalid="ignore", divide="ignore"):
        ave = np.nan_to_num((img1 * m1 + img2 * m2) / (m1.astype(np.float64) + m2))
    ave = _largest_step(ave, keep)
    print(f"largest neighbour step: scene {own:.2f}, multi-band L=5 {multi:.2f} ({multi / own:.2f} x), ave_fusion {ave:.2f} ({ave / own:.2f} x), hard seam {hard:.2f}")
    assert multi <= 1.25 * own
    assert ave >= 5 * own


@pytest.mark.parametrize("defect", ref.DEFECTS)
def test_a_planted_defect_fails_an_assertion(defect):
    failed = []
    for check in CHECKS:
        try:
            check(frozenset({defect}))
        except AssertionError:
            failed.append(check.__name__)
    assert failed, f"no assertion notices {defect}"


# ---- entries and binary --------------------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_touching_the_gpu():
    from stitch_amd._lib import lib
    base = 0x7f0000000000                                                   # never dereferenced on the host
    img1, img2, k1, k2, out, ws = (base + (i << 32) for i in range(6))
    H, W, L = 37, 53, 5
    need = lib.st_multiband_workspace_bytes(H, W, L)
    assert need > 7 * 4 * H * W and need % 16 == 0

    def blend(img1=img1, img2=img2, k1=k1, k2=k2, H=H, W=W, L=L, out=out, ws=ws, nbytes=need):
        return lib.st_multiband_blend(img1, img2, k1, k2, H, W, L, out, ws, nbytes, None)
    for name in ("img1", "img2", "k1", "k2", "out", "ws"):
        assert blend(**{name: None}) == 1001, name
    big = 1 << 40
    assert blend(H=0) == 1001 and blend(W=0) == 1001 and blend(H=4097, nbytes=big) == 1001 and blend(W=4097, nbytes=big) == 1001
    assert blend(L=-1) == 1001 and blend(L=17, nbytes=big) == 1001
    assert blend(nbytes=need - 1) == 1001 and blend(ws=ws + 8) == 1001
    wsb = lib.st_multiband_workspace_bytes
    assert wsb(0, 5, 5) == 0 and wsb(5, 0, 5) == 0 and wsb(4097, 5, 5) == 0 and wsb(5, 4097, 5) == 0 and wsb(5, 5, -1) == 0 and wsb(5, 5, 17) == 0
    assert 0 < wsb(1, 1, 0) <= wsb(1, 1, 16) and wsb(4096, 4096, 16) > 0
    assert wsb(64, 64, 16) == wsb(64, 64, 6) > wsb(64, 64, 5)              # capped where both sides reach 1
    edt = lib.st_edt_sq_u8
    assert edt(None, 4, 4, 1, out, None, None) == 1001 and edt(k1, 4, 4, 1, None, None, None) == 1001
    assert edt(k1, 0, 4, 1, out, None, None) == 1001 and edt(k1, 4, 0, 1, out, None, None) == 1001
    assert edt(k1, 4097, 4, 1, out, None, None) == 1001 and edt(k1, 4, 4097, 0, out, ws, None) == 1001


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_kernels_use_no_scratch_and_do_not_spill():
    """from the compiler's metadata of csrc/multiband.hip, built with the library's own flags"""
    spec = importlib.util.spec_from_file_location("_stitch_build", os.path.join(ROOT, "seamless-through-breaking-rethinking-image-stitching-for-optimal-alignment_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert build.SOURCES["multiband.hip"] == ["-ffp-contract=off"]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "multiband.s")
        subprocess.check_call(build.compile_cmd("multiband.hip", out, ["-S", "--cuda-device-only"]), stderr=subprocess.DEVNULL)
        text = open(out).read()
    rep = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+)\n.*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)",
                         text, re.S):
        rep[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    lds = {"edt_cols_kernel": 8192, "edt_rows_d_kernel": 16384, "edt_rows_idx_kernel": 16384, "mb_masks_kernel": 0, "mb_fields_kernel": 0, "mb_reduce_kernel": 0, "mb_top_kernel": 0,
           "mb_down_kernel": 0}
    assert len(rep) == len(lds), sorted(rep)
    for key, want in lds.items():
        (name, r), = [(n, r) for n, r in rep.items() if key in n]
        assert r["scratch"] == 0 and r["spill"] == 0 and r["lds"] == want and r["vgpr"] <= 64, (name, r)
