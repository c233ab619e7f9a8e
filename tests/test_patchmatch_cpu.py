"""patchmatch_inpainter without a GPU: the vectorised restatement tests/_patchmatch_ref.py against pixel-by-pixel Python loops (pyramid, source
and target planes, SAD, vote, hash, one search sweep), its properties and degenerate cases, the fill against Telea on two periodic scenes, nine
planted defects that must each fail one of those assertions, the C entries' rejections and the compiler's resource report of
csrc/patchmatch.hip."""
import importlib.util
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _patchmatch_ref as ref
import _telea_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = frozenset()
SIZES = ((63, 65), (33, 47), (15, 15), (16, 130))
SMALL = ((33, 47), (15, 15))                              # where the 49-term loops run


def cases(sizes, scene="ramp"):
    for H, W in sizes:
        for name, hole in ref.masks(H, W).items():
            img = ref.scene(scene, H, W).copy()
            img[hole] = 0
            yield f"{H}x{W} {name}", img, hole


# ---- the scalar statements -------------------------------------------------------------------------------------------------------------------
def fmix_scalar(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = x * 0x85EBCA6B & 0xFFFFFFFF
    x ^= x >> 13
    x = x * 0xC2B2AE35 & 0xFFFFFFFF
    return x ^ x >> 16


def hash_scalar(seed, level, it, k, idx):
    return fmix_scalar(fmix_scalar((seed & 0xFFFFFFFF) ^ fmix_scalar(level * 65536 + it * 256 + k)) ^ idx)


def half_up(S, n):
    return (2 * S + n) // (2 * n)


def down_scalar(img, hole):
    H, W = hole.shape
    h2, w2 = -(-H // 2), -(-W // 2)
    out, oh = np.zeros((h2, w2, 3), np.uint8), np.zeros((h2, w2), bool)
    for i in range(h2):
        for j in range(w2):
            kids = [(min(2 * i + a, H - 1), min(2 * j + b, W - 1)) for a in (0, 1) for b in (0, 1)]
            known = [k for k in kids if not hole[k]]
            oh[i, j] = len(known) < 4
            for c in range(3):
                out[i, j, c] = half_up(sum(int(img[k][c]) for k in known), len(known)) if known else 0
    return out, oh


def classify_scalar(hole):
    H, W = hole.shape
    src, tgt = np.zeros((H, W), bool), np.zeros((H, W), bool)
    for y in range(3, H - 3):
        for x in range(3, W - 3):
            any_hole = bool(hole[y - 3:y + 4, x - 3:x + 4].any())
            src[y, x], tgt[y, x] = not any_hole, any_hole
    return src, tgt


def sad_scalar(img, p, q):
    a = img[p[0] - 3:p[0] + 4, p[1] - 3:p[1] + 4].astype(np.int64)
    b = img[q[0] - 3:q[0] + 4, q[1] - 3:q[1] + 4].astype(np.int64)
    assert a.shape == b.shape == (7, 7, 3)
    return int(np.abs(a - b).sum())


def vote_scalar(img, hole, tgt, nnf):
    H, W = hole.shape
    out = img.copy()
    for y, x in np.argwhere(hole):
        S, n = [0, 0, 0], 0
        for py in range(max(y - 3, 3), min(y + 3, H - 4) + 1):
            for px in range(max(x - 3, 3), min(x + 3, W - 4) + 1):
                assert tgt[py, px]
                qy, qx = nnf[py, px, 0] + y - py, nnf[py, px, 1] + x - px
                for c in range(3):
                    S[c] += int(img[qy, qx, c])
                n += 1
        out[y, x] = [half_up(s, n) for s in S]
    return out


def sweep_scalar(img, src, tgt, nnf, seed, level, it):
    H, W = tgt.shape
    new, cost = nnf.copy(), np.full((H, W), -1, np.int64)
    for py, px in np.argwhere(tgt):
        p = (int(py), int(px))
        best = (int(nnf[py, px, 0]), int(nnf[py, px, 1]))
        bc = sad_scalar(img, p, best)

        def trial(c):
            nonlocal best, bc
            if 0 <= c[0] < H and 0 <= c[1] < W and src[c]:
                d = sad_scalar(img, p, c)
                if d < bc:
                    best, bc = c, d
        for s in (1, 2 ** (1 + it % 3)):
            for dy, dx in ((0, -s), (0, s), (-s, 0), (s, 0)):
                ny, nx = p[0] + dy, p[1] + dx
                if 0 <= ny < H and 0 <= nx < W and tgt[ny, nx]:
                    trial((int(nnf[ny, nx, 0]) - dy, int(nnf[ny, nx, 1]) - dx))
        R, k = max(H, W), 0
        while R >= 1:
            r = hash_scalar(seed, level, it, k, p[0] * W + p[1])
            trial((best[0] + (r & 0xFFFF) % (2 * R + 1) - R, best[1] + (r >> 16) % (2 * R + 1) - R))
            R, k = R // 2, k + 1
        new[py, px], cost[py, px] = best, bc
    return new, cost


# ---- the checks: each takes the planted defects of the restatement ------------------------------------------------------------------------------
def check_hash(d=NONE):
    idx = np.array([0, 1, 2, 77, 4095, 65535, 65536, 4096 * 4096 - 1])
    for seed, level, it, k in ((1, 0, 0, 0), (1, 0, 1, 0), (1, 3, 2, 5), (0xDEADBEEF, 7, 63, 12), (2, 1, ref.INIT_IT, 0), (-5, 2, 7, 1)):
        got = ref.pm_hash(seed, level, it, k, idx, d)
        assert got.tolist() == [hash_scalar(seed, level, it, k, int(i)) for i in idx], (seed, level, it, k)
    assert fmix_scalar(1) == 0x514E28B7 and int(ref.fmix32(1)) == 0x514E28B7            # murmur3's finaliser of 1


def check_levels(d=NONE):
    lc = ref.level_count
    assert [lc(64, 80), lc(63, 65), lc(64, 64), lc(127, 127), lc(128, 4096), lc(4096, 4096), lc(15, 4096)] == [2, 2, 2, 3, 3, 8, 1]
    assert [lc(64, 80, 4), lc(64, 80, 1), lc(30, 30, 8), lc(28, 60, 8), lc(4096, 4096, 8), lc(4096, 4096, 3), lc(59, 59, 8)] == [3, 1, 2, 1, 8, 3, 3]


def check_pyramid(d=NONE):
    for tag, img, hole in cases(SIZES):
        got, want = ref.down(img, hole, d), down_scalar(img, hole)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), tag
        if min(got[1].shape) >= 8:                                   # and once more, on a level that has partly known pixels
            got2, want2 = ref.down(*got, d), down_scalar(*want)
            assert np.array_equal(got2[1], want2[1]) and np.array_equal(got2[0], want2[0]), tag


def check_classify(d=NONE):
    for tag, _, hole in cases(SIZES):
        got, want = ref.classify(hole, d), classify_scalar(hole)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), tag
        assert list(map(tuple, np.argwhere(got[0]))) == [(y, x) for y in range(hole.shape[0]) for x in range(hole.shape[1]) if want[0][y, x]]     # row-major


def check_sad(d=NONE):
    rng = np.random.default_rng(5)
    for H, W in SIZES:
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        img[..., 2] = np.where(rng.random((H, W)) < 0.5, 255, 0)     # (a channel left out shows at once)
        p = np.stack([rng.integers(3, H - 3, 40), rng.integers(3, W - 3, 40)], 1)
        q = np.stack([rng.integers(3, H - 3, 40), rng.integers(3, W - 3, 40)], 1)
        assert ref.sad(img, p, q, d).tolist() == [sad_scalar(img, tuple(a), tuple(b)) for a, b in zip(p, q)]
    flat0, flat1 = np.zeros((15, 15, 3), np.uint8), np.full((15, 15, 3), 255, np.uint8)
    both = np.concatenate([flat0, flat1], 1)
    assert ref.sad(both, np.array([[7, 7]]), np.array([[7, 22]]), d).tolist() == [49 * 3 * 255]


def _level_state(img, hole, seed, d):
    src, tgt = ref.classify(hole, d)
    if not src.any() or not tgt.any():
        return None
    nnf = ref.init_nnf(src, tgt, seed, 0, None, d)
    return src, tgt, nnf


def check_vote(d=NONE):
    ran = 0
    for tag, img, hole in cases(SMALL):
        st = _level_state(img, hole, 1, d)
        if st is None:
            continue
        src, tgt, nnf = st
        assert np.array_equal(ref.vote(img, hole, tgt, nnf, d), vote_scalar(img, hole, tgt, nnf)), tag
        ran += 1
    assert ran >= 6


def check_sweep(d=NONE):
    """two sweeps from the initialisation, on the ramp and on the checkerboard (equal costs everywhere: the tie rule decides)"""
    ran = 0
    for scene in ("ramp", "checker"):
        for tag, img, hole in cases(((20, 26), (15, 15)), scene):
            st = _level_state(img, hole, 1, d)
            if st is None:
                continue
            src, tgt, nnf = st
            cur = ref.vote(img, hole, tgt, nnf, d)
            for it in (0, 1):
                got = ref.search(cur, src, tgt, nnf, 1, 0, it, d)
                want = sweep_scalar(cur, src, tgt, nnf, 1, 0, it)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (scene, tag, it)
                before = ref.sad(cur, np.argwhere(tgt), nnf[tgt], d)
                assert (got[1][tgt] <= before).all(), tag                          # a sweep never raises a target's recomputed cost
                assert src[got[0][tgt][:, 0], got[0][tgt][:, 1]].all(), tag
                nnf = got[0]
                cur = ref.vote(cur, hole, tgt, nnf, d)
            ran += 1
    assert ran >= 6


def check_init_from_the_coarse_level(d=NONE):
    """every finer target whose coarse centre is a target and whose doubled match is a source takes it; the others the hash draw"""
    H, W = 33, 47
    hole = ref.masks(H, W)["corner"]
    img = ref.scene("ramp", H, W).copy()
    img[hole] = 0
    (_, h0), (i1, h1) = ref.pyramid(img, hole, 2, d)
    s0, t0 = ref.classify(h0, d)
    s1, t1 = ref.classify(h1, d)
    n1 = ref.init_nnf(s1, t1, 3, 1, None, d)
    n0 = ref.init_nnf(s0, t0, 3, 0, (n1, t1), d)
    srclist = [tuple(p) for p in np.argwhere(s0)]
    took = 0
    for y, x in np.argwhere(t0):
        cy, cx = min(max(y >> 1, 3), h1.shape[0] - 4), min(max(x >> 1, 3), h1.shape[1] - 4)
        want = srclist[hash_scalar(3, 0, ref.INIT_IT, 0, int(y * W + x)) % len(srclist)]
        if t1[cy, cx]:
            q = (min(max(2 * n1[cy, cx, 0] + (y & 1), 3), H - 4), min(max(2 * n1[cy, cx, 1] + (x & 1), 3), W - 4))
            if s0[q]:
                want, took = q, took + 1
        assert tuple(n0[y, x]) == want
    assert 0 < took and (n0[~t0] == -1).all()


def check_properties(d=NONE):
    for tag, img, hole in cases(SIZES):
        a = ref.patchmatch(img, hole, 4, 2, 1, d)
        assert np.array_equal(a[0][~hole], img[~hole]), tag                         # known pixels byte for byte
        assert a[1][0] == int(ref.classify(hole)[0].any() and hole.any()), tag
        if not a[1][0]:
            assert np.array_equal(a[0], img) and (a[2] == -1).all() and (a[3] == -1).all(), tag
    for H, W in SMALL:
        for name, hole in ref.masks(H, W).items():
            img = np.full((H, W, 3), (9, 200, 77), np.uint8)
            dirty = img.copy()
            dirty[hole] = 0
            out, info, _, sad = ref.patchmatch(dirty, hole, None, 2, 1, d)
            if info[0]:
                assert np.array_equal(out, img) and sad.max() == 0, name            # a constant image gives the constant exactly
    img, hole = next((i, h) for t, i, h in cases(((33, 47),)) if t.endswith("noise"))
    a, b, c = (ref.patchmatch(img, hole, 2, 2, s, d) for s in (1, 1, 2))
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not np.array_equal(a[2], c[2])     # the same seed, the same bytes


def check_degenerate(d=NONE):
    H, W = 40, 50
    img = ref.scene("ramp", H, W)
    pm = lambda m, **kw: ref.patchmatch(img, m, defects=d, **kw)                    # noqa: E731
    none, all_ = np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8)
    out, info, nnf, sad = pm(none)
    assert np.array_equal(out, img) and info == [0, 0, 34 * 44, 0] and (nnf == -1).all() and (sad == -1).all()
    out, info, nnf, sad = pm(all_)
    assert np.array_equal(out, img) and info == [0, 0, 0, 34 * 44]
    strip6 = all_.copy()
    strip6[:, 20:26] = 0                                             # no source at level 0: six known columns hold no 7x7 box
    out, info, _, _ = pm(strip6)
    assert np.array_equal(out, img) and info == [0, 0, 0, 34 * 44]
    strip8 = np.ones((64, 64), np.uint8)
    strip8[:, 4:12] = 0                                              # a coarse level without sources: the strip is 4 wide there
    img8 = ref.scene("ramp", 64, 64)
    out, info, nnf, sad = ref.patchmatch(img8, strip8, 3, 2, 1, d)
    assert info == [1, 0, 2 * 58, 58 * 58 - 2 * 58] and np.array_equal(out[:, 4:12], img8[:, 4:12]) and (sad[ref.classify(strip8 != 0)[1]] >= 0).all()
    assert set(nnf[..., 1][nnf[..., 1] >= 0].tolist()) == {7, 8}
    out0 = ref.patchmatch(img8, strip8, 3, 0, 1, d)
    assert out0[1] == info and (out0[3] == -1).all() and (out0[2][..., 0] >= 0).sum() == info[3]      # no sweep: the initialisation, no cost


CHECKS = [check_hash, check_levels, check_pyramid, check_classify, check_sad, check_vote, check_sweep, check_init_from_the_coarse_level, check_properties,
          check_degenerate]


@pytest.mark.parametrize("check", CHECKS, ids=lambda c: c.__name__)
def test_restatement(check):
    check()


@pytest.mark.parametrize("defect", ref.DEFECTS)
def test_a_planted_defect_fails_an_assertion(defect):
    failed = None
    for check in CHECKS:
        try:
            check(frozenset({defect}))
        except AssertionError:
            failed = check.__name__
            break
    assert failed, f"no assertion notices {defect}"
    print(f"{defect}: noticed by {failed}")


def test_periodic_scenes_fill_ten_times_closer_than_telea():
    """64x80, a 24x24 hole, 4 levels, 4 sweeps, seed 1: the exemplar fill reproduces a periodic texture, the Telea fill smears the border inwards"""
    H, W = 64, 80
    hole = np.zeros((H, W), bool)
    hole[20:44, 28:52] = True
    for name in ("stripes", "checker", "constant"):
        gt = ref.scene(name, H, W)
        img = gt.copy()
        img[hole] = 0
        mae = lambda a: float(np.abs(a.astype(np.int64) - gt.astype(np.int64))[hole].mean())      # noqa: E731
        pm = mae(ref.patchmatch(img, hole, 4, 4, 1)[0])
        telea = mae(_telea_ref.telea(img, hole, 64)[0])
        print(f"{name}: patchmatch MAE {pm:.4f}, Telea MAE {telea:.2f} grey levels in the hole")
        if name == "constant":
            assert pm == 0.0
        else:
            assert telea > 20 and pm < telea / 10, (name, pm, telea)


# ---- entries and binary --------------------------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_touching_the_gpu():
    from stitch_amd._lib import lib
    base = 0x7f0000000000                                                   # never dereferenced on the host
    img, mask, out, info, nnf, sad, ws = (base + (i << 32) for i in range(7))
    H, W = 37, 53
    n = H * W
    wsb, nlev = lib.st_patchmatch_workspace_bytes, lib.st_patchmatch_levels
    need = wsb(H, W, 0)
    assert need >= 26 * n - 8 * (6 * H + 6 * W) and need % 16 == 0 and wsb(H, W, 1) == need < wsb(H, W, 2) == wsb(H, W, 8)
    for bad in ((14, 53, 0), (37, 14, 0), (4097, 53, 0), (37, 4097, 0), (-1, 53, 0), (37, 53, -1), (37, 53, 9)):
        assert wsb(*bad) == 0 and nlev(*bad) == 0, bad
    assert 0 < wsb(4096, 4096, 0) < 2 ** 31 and wsb(4096, 4096, 8) == wsb(4096, 4096, 0) and wsb(15, 15, 0) > 0
    for (h, w), lv in (((64, 80), None), ((63, 65), 4), ((4096, 4096), None), ((15, 4096), 8), ((59, 59), 8), ((128, 4096), None)):
        assert nlev(h, w, lv or 0) == ref.level_count(h, w, lv), (h, w, lv)
    big = 1 << 40

    def call(img=img, mask=mask, H=H, W=W, levels=0, iters=4, seed=1, out=out, info=info, nnf=nnf, sad=sad, ws=ws, nbytes=need):
        return lib.st_patchmatch_fill(img, mask, H, W, levels, iters, seed, out, info, nnf, sad, ws, nbytes, None)
    for name in ("img", "mask", "out", "info", "ws"):
        assert call(**{name: None}) == 1001, name
    assert call(H=14) == 1001 and call(W=14) == 1001 and call(H=4097, nbytes=big) == 1001 and call(W=4097, nbytes=big) == 1001 and call(H=-3) == 1001
    assert call(levels=-1) == 1001 and call(levels=9, nbytes=big) == 1001 and call(iters=-1) == 1001 and call(iters=65) == 1001
    assert call(nbytes=need - 1) == 1001 and call(nbytes=0) == 1001 and call(ws=ws + 8) == 1001 and call(H=H + 1) == 1001 and call(levels=2) == 1001
    sizes = dict(out=3 * n, info=16, nnf=8 * n, sad=4 * n)
    args = dict(out=out, info=info, nnf=nnf, sad=sad)
    for a, abytes in sizes.items():                                         # the overlaps, with and without the optional planes
        for src, sbytes in ((img, 3 * n), (mask, n), (ws, need)):
            assert call(**{a: src}) == 1001 and call(**{a: src + sbytes - 1}) == 1001 and call(**{a: src - abytes + 1}) == 1001, a
        for b, bbytes in sizes.items():
            if a != b:
                assert call(**{a: args[b] + bbytes - 1}) == 1001 and call(**{a: args[b] - abytes + 1}) == 1001, (a, b)
    assert call(img=ws + 16) == 1001 and call(mask=ws + need - 1) == 1001 and call(img=ws - 3 * n + 1) == 1001
    assert call(nnf=None, sad=None, out=img + 3 * n - 1) == 1001 and call(nnf=None, sad=None, info=ws) == 1001


def test_kernels_use_no_scratch_and_the_search_is_byte_sads():
    """from the compiler's metadata of csrc/patchmatch.hip, built with the library's own flags (README.md, patchmatch_inpainter, kernel table)"""
    spec = importlib.util.spec_from_file_location("_stitch_build", os.path.join(ROOT, "seamless-through-breaking-rethinking-image-stitching-for-optimal-alignment_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert build.SOURCES["patchmatch.hip"] == []
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "patchmatch.s")
        subprocess.check_call(build.compile_cmd("patchmatch.hip", out, ["-S", "--cuda-device-only"]), stderr=subprocess.DEVNULL)
        text = open(out).read()
    rep = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+)\n.*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)",
                         text, re.S):
        rep[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    lds = {"pm_pack_kernel": 0, "pm_down_kernel": 0, "pm_classify_kernel": 16, "pm_scan_kernel": 128, "pm_compact_kernel": 16, "pm_decide_kernel": 0,
           "pm_init_kernel": 0, "pm_vote_kernel": 0, "pm_sweep_kernel": 0, "pm_output_kernel": 0}
    assert len(rep) == len(lds), sorted(rep)
    for key, want in lds.items():
        (name, r), = [(n, r) for n, r in rep.items() if key in n]
        print(key, r)
        assert r["lds"] == want, (name, r)
        assert r["scratch"] == 0 and r["spill"] == 0 and r["vgpr"] <= 128, (name, r)      # (128: four waves per SIMD; the scan's 1024-thread workgroup needs it)
    body = text[text.index("pm_sweep_kernel"):]
    body = body[:body.index("s_endpgm")]
    assert body.count("v_sad_u8") >= 49                                                   # the target patch in registers, one byte-SAD per pixel pair
