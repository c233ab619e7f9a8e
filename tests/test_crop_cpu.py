"""inner_crop without a GPU: the candidate rule of tests/_crop_ref.py against brute force over all rectangles, the runs against a scalar loop,
the planted ties, the two-level row search against the plain outward scan and its read bound, nine planted defects that must each fail one
of those assertions, the C entries' rejections and the compiler's resource report of csrc/crop.hip."""
import functools
import importlib.util
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _crop_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = frozenset()


@functools.lru_cache(maxsize=None)
def small_masks():
    """every size 1x1 .. 6x7 at densities 0.5 / 0.8 / 0.95 / 1.0, twelve seeded masks each (2016), plus all ones, all zeros and a single zero,
    each with its brute-force rectangle"""
    rng = np.random.default_rng(20261020)
    out = []
    for H in range(1, 7):
        for W in range(1, 8):
            ms = [rng.random((H, W)) < d for d in (0.5, 0.8, 0.95, 1.0) for _ in range(12)]
            ms += [np.ones((H, W), bool), np.zeros((H, W), bool)]
            single = np.ones((H, W), bool)
            single[rng.integers(H), rng.integers(W)] = False
            ms.append(single)
            out += [(m, ref.rect_brute(m)) for m in ms]
    return out


def scalar_runs(u):
    H, W = u.shape
    r = np.zeros((H, W), np.int16)
    for x in range(W):
        n = 0
        for y in range(H):
            n = n + 1 if u[y, x] else 0
            r[y, x] = n
    return r


def plain_scan(row):
    """L and R by the definition: the nearest position on each side with a strictly smaller run"""
    row = np.asarray(row, np.int64)
    W = len(row)
    L, R = [-1] * W, [W] * W
    for x in range(W):
        lo = np.nonzero(row[:x] < row[x])[0]
        hi = np.nonzero(row[x + 1:] < row[x])[0]
        L[x] = int(lo[-1]) if len(lo) else -1
        R[x] = int(hi[0]) + x + 1 if len(hi) else W
    return L, R


def check_rule(defects=NONE):
    seen = 0
    for m, want in small_masks():
        assert ref.rect(m, defects) == want, (m.astype(int).tolist(), want)
        seen += 1
    assert seen == 42 * 51


def check_runs(defects=NONE):
    rng = np.random.default_rng(7)
    for H, W in ((1, 1), (1, 5), (5, 1), (15, 3), (16, 3), (17, 3), (31, 4), (32, 4), (33, 4), (40, 7), (100, 3)):
        for d in (0.5, 0.9, 1.0):
            u = rng.random((H, W)) < d
            got = ref.runs(u, defects)
            assert got.dtype == np.int16 and np.array_equal(got, scalar_runs(u)), (H, W, d)
    for H in (32, 33, 48):                                           # an unset pixel on the last row of a segment, and on the first of the next
        S = -(-H // 16)
        for y in (S - 1, S, 5 * S - 1, 5 * S):
            u = np.ones((H, 2), bool)
            u[y, 0] = False
            assert np.array_equal(ref.runs(u, defects), scalar_runs(u)), (H, y)


def check_ties(defects=NONE):
    def mask(H, W, rects):
        u = np.zeros((H, W), bool)
        for t, l, h, w in rects:
            u[t:t + h, l:l + w] = True
        return u
    cases = [(mask(5, 9, [(1, 1, 3, 3), (1, 5, 3, 3)]), [1, 1, 1, 3, 3, 9]),              # equal squares side by side: the lowest left
             (mask(9, 5, [(1, 1, 3, 3), (5, 1, 3, 3)]), [1, 1, 1, 3, 3, 9]),              # one above the other: the lowest top
             (mask(4, 7, [(0, 0, 2, 6), (0, 0, 3, 4)]), [1, 0, 0, 2, 6, 12]),             # 2 x 6 against 3 x 4 at the same corner: the smallest h
             (mask(8, 8, [(4, 0, 2, 6), (0, 2, 3, 4)]), [1, 0, 2, 3, 4, 12]),             # equal areas at different tops: the lowest top, though it lies further right
             (mask(6, 9, [(3, 0, 3, 4), (1, 5, 2, 4)]), [1, 3, 0, 3, 4, 12])]         # (area first: 12 against 8)
    for u, want in cases:
        assert ref.rect_brute(u) == want, want
        assert ref.rect(u, defects) == want, want


def search_rows():
    rows = []
    for W in (1, 63, 64, 65, 130, 4095, 4096):
        x = np.arange(W)
        rows.append((f"equal {W}", np.full(W, 7)))
        rows.append((f"ascending {W}", x + 1))
        rows.append((f"descending {W}", W - x))
        for at in (0, 63, 64, W - 1):
            if at < W:
                r = np.full(W, 9)
                r[at] = 2
                rows.append((f"low at {at} of {W}", r))
    for W in (130, 300):
        r = np.full(W, 3)
        r[60:68] = 8                                                 # a plateau across 63 | 64
        r[120:136] = 5                                               # and one across 127 | 128
        rows.append((f"plateaus {W}", r))
        r2 = np.full(W, 8)
        r2[62:66] = 3
        r2[127:129] = 0
        rows.append((f"dips {W}", r2))
    rng = np.random.default_rng(11)
    for W in (64, 200, 257):
        rows.append((f"noise {W}", rng.integers(0, 6, W)))
    return rows


def check_search(defects=NONE):
    for name, row in search_rows():
        if defects and len(row) > 300:                               # (a defect shows at the small widths; the long rows are for the shipped form)
            continue
        L, R, _ = ref.search_reads(row, defects)
        wl, wr = plain_scan(row)
        live = [x for x in range(len(row)) if row[x] > 0]
        assert [L[x] for x in live] == [wl[x] for x in live], name
        assert [R[x] for x in live] == [wr[x] for x in live], name
        L2, R2 = ref.lr(row, defects)
        assert [L2[x] for x in live] == [wl[x] for x in live] and [R2[x] for x in live] == [wr[x] for x in live], name


def check_bound(defects=NONE):
    assert ref.SEARCH_BOUND == 190
    x = np.arange(4096)
    worst = np.full(4096, 9)
    worst[0] = worst[4095] = 1                                       # every position walks all the block minima on both sides
    worst[64 * 30 + 5] = 8                                           # and block 30 scans itself first, in vain on both sides
    for name, row in (("equal", np.full(4096, 4096)), ("ascending", x + 1), ("descending", 4096 - x), ("worst", worst)):
        _, _, reads = ref.search_reads(row, defects)
        top = max(max(p) for p in reads)
        assert top <= ref.SEARCH_BOUND, (name, top)
    assert max(max(p) for p in ref.search_reads(np.full(4096, 4096))[2]) == 1 + 63            # the commonest row: the minima alone


def check_masks(defects=NONE):
    half = np.float32(0.5)
    vals = np.array([[0.0, half, np.nextafter(half, np.float32(1)), 1.0, np.nan, np.inf, -np.inf, -1.0]], np.float32)[None]
    want = [False, False, True, True, False, True, False, False]
    assert ref.union(vals, None, defects)[0].tolist() == want
    assert ref.union(np.zeros_like(vals), vals, defects)[0].tolist() == want
    assert ref.union(vals, np.ones_like(vals), defects).all()


def check_key(defects=NONE):
    full = ref.key(0, 0, 4096, 4096, defects)
    assert full < 1 << 64 and ref.decode(full, defects) == [1, 0, 0, 4096, 4096, 1 << 24]
    assert full > ref.key(0, 0, 4095, 4096, defects) > ref.key(1, 0, 4095, 4096, defects) > 0
    for t, l, h, w in ((4095, 4095, 1, 1), (0, 4095, 4096, 1), (4095, 0, 1, 4096), (17, 5, 300, 7)):
        assert ref.decode(ref.key(t, l, h, w, defects), defects) == [1, t, l, h, w, h * w]
    assert ref.decode(0, defects) == [0] * 6


CHECKS = (check_masks, check_key, check_ties, check_runs, check_search, check_rule, check_bound)


def test_candidate_rule_equals_brute_force_over_all_rectangles():
    check_rule()


def test_runs_equal_the_scalar_loop():
    check_runs()


def test_planted_ties_take_the_documented_branch():
    check_ties()


def test_two_level_search_finds_what_the_plain_scan_finds():
    check_search()


def test_search_reads_stay_within_the_bound():
    check_bound()


def test_mask_rule_and_key_range():
    check_masks()
    check_key()


@pytest.mark.parametrize("defect", ref.DEFECTS)
def test_a_planted_defect_fails_an_assertion(defect):
    failed = None
    for check in CHECKS:
        if check is check_bound:                                     # (a condition on the shipped search's cost, not on its result)
            continue
        try:
            check(frozenset({defect}))
        except AssertionError:
            failed = check.__name__
            break
    assert failed, f"no assertion notices {defect}"


# ---- entries and binary --------------------------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_touching_the_gpu():
    from stitch_amd._lib import lib
    base = 0x7f0000000000                                                   # never dereferenced on the host
    k1, k2, info, runs, ws = (base + (i << 32) for i in range(5))
    H, W = 37, 53
    wsb = lib.st_inner_rect_workspace_bytes
    need = wsb(H, W)
    assert need >= 2 * H * W + 8 * H and need % 16 == 0
    assert wsb(0, 5) == 0 and wsb(5, 0) == 0 and wsb(4097, 5) == 0 and wsb(5, 4097) == 0 and wsb(-1, 5) == 0
    assert 0 < wsb(4096, 4096) < 2 ** 31 and wsb(1, 1) > 0
    big = 1 << 40

    def call(k1=k1, k2=k2, H=H, W=W, info=info, runs=runs, ws=ws, nbytes=need):
        return lib.st_inner_rect(k1, k2, H, W, info, runs, ws, nbytes, None)
    for name in ("k1", "info", "ws"):
        assert call(**{name: None}) == 1001, name
    assert call(H=0) == 1001 and call(W=0) == 1001 and call(H=4097, nbytes=big) == 1001 and call(W=4097, nbytes=big) == 1001 and call(H=-3) == 1001
    assert call(nbytes=need - 1) == 1001 and call(nbytes=0) == 1001 and call(ws=ws + 8) == 1001 and call(H=H + 1) == 1001
    n = H * W
    for k2_ in (k2, None):                                                  # the overlaps, with and without the second mask
        assert call(k2=k2_, info=k1) == 1001 and call(k2=k2_, info=k1 + 4 * n - 4) == 1001
        assert call(k2=k2_, runs=k1 + 4 * n - 2) == 1001 and call(k2=k2_, runs=k1 - 2 * n + 2) == 1001
        assert call(k2=k2_, info=runs) == 1001 and call(k2=k2_, info=runs + 2 * n - 4) == 1001 and call(k2=k2_, runs=info - 2 * n + 2) == 1001
        assert call(k2=k2_, info=ws) == 1001 and call(k2=k2_, info=ws + need - 4) == 1001 and call(k2=k2_, info=ws - 20) == 1001
        assert call(k2=k2_, runs=ws + need - 2) == 1001 and call(k2=k2_, runs=ws - 2 * n + 2) == 1001
        assert call(k2=k2_, k1=ws + 16) == 1001 and call(k2=k2_, k1=ws - 4 * n + 4) == 1001
    assert call(info=k2) == 1001 and call(info=k2 + 4 * n - 4) == 1001 and call(runs=k2 + 4 * n - 2) == 1001 and call(k2=ws + need - 4) == 1001


def test_kernels_use_no_scratch_and_the_stated_lds():
    """from the compiler's metadata of csrc/crop.hip, built with the library's own flags (README.md, inner_crop, kernel table)"""
    spec = importlib.util.spec_from_file_location("_stitch_build", os.path.join(ROOT, "seamless-through-breaking-rethinking-image-stitching-for-optimal-alignment_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert build.SOURCES["crop.hip"] == []
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "crop.s")
        subprocess.check_call(build.compile_cmd("crop.hip", out, ["-S", "--cuda-device-only"]), stderr=subprocess.DEVNULL)
        text = open(out).read()
    rep = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+)\n.*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)",
                         text, re.S):
        rep[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    lds = {"crop_runs_kernel": 4096, "crop_rows_kernel": 8352, "crop_pick_kernel": 128}
    assert len(rep) == len(lds), sorted(rep)
    for key, want in lds.items():
        (name, r), = [(n, r) for n, r in rep.items() if key in n]
        assert r["lds"] == want, (name, r)
        assert r["scratch"] == 0 and r["spill"] == 0 and r["vgpr"] <= 128, (name, r)      # (1024-thread workgroups: at most 128 VGPRs)
