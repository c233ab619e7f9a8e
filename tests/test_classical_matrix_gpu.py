"""The classical-path C entries (csrc/features.hip, features_ms.hip, dense_flow.hip, patchmatch.hip, seam_gc.hip, crop.hip) outside and at the
edge of their contract, on the GPU.  Every comparison is bit equality with the CPU restatements.

A. `test_refusals_on_live_buffers`: the refusal table of tests/_classical_cases.py (null cases left out) on live buffers.  All operands of
   an entry lie in one arena, each with room for the base and for the lied-about shape and a slot of padding on either side, so a call
   that a missing check lets through stays inside the arena.  Every refused call returns 1001 and leaves every byte of the arena as it was.
   Then the base record returns 0 and equals the restatement, and the accepted rows (an optional pointer null, an input starting where
   another input starts) return 0 with the bits of the equal call the table names.

B. The stage entries on device data that no pipeline produces.  Every index or count that a stage kernel loads from device memory and then
   uses in an address, and the line that bounds it (also DESIGN.md, "Device-loaded indices of the classical path"):

     ft_describe_kernel     kp (x, y) -> box[(y + dy) W + x + dx]       `if (x >= FT_BORDER && x < W - FT_BORDER && y >= ... )`: else nothing is read
     ftms_describe_kernel   kp (x, y) -> box of the slot's level         the same test against the slot's own H_l, W_l and FTMS_BORDER
                            bins[slot] -> ftms_cs.v[2 bin]                `& (FTMS_BINS - 1)`
     ft_match_kernel        kp x only as a flag (`>= 0`); candidate indices are loop counters
     ft_compact_kernel      nn[.,0] = j -> r[3 j]                         `j >= 0 && j < N` first in the same condition
     ft_count               count[b] -> loop bounds, sm[p], mb[4 p]       `min(max(count[b], 0), N)`
     ft_norm_kernel         matches (i, j) -> kp1[i], kp2[j]              `min(max(., 0), N - 1)`
     ftms_norm_kernel       the same, and the slot (not the value) picks the level
     ft_hyp_kernel          draws `% m` with m from ft_count (>= 8 where used)
     ft_refit_kernel        scores only compared; winner = 65535 - (best & 65535) feeds the hash alone; sm[p], p < m <= N <= 4096
     ftms_refit_kernel      m = ft_count(count, b, min(N, FTMS_MAX_SLOTS)): sm[FTMS_MAX_SLOTS]
     df_iterate_kernel      U -> sx = 256 x + ux, xs = sx >> 8 -> v2[ys W + xs]  `xs >= 0 && xs <= W - 2 && ys >= 0 && ys <= H - 2`; the sum is
                            defined while it stays inside int32: |u| <= 2^31 - 1 - 256 * 1023 - 256 (header)
     df_median_kernel       values only
     seam_gc                gc_push_kernel / gc_gather_kernel follow a positive residual to h[p + step] with no test of their own: the setup
                            leaves none across the canvas edge.  This is a documented precondition of st_seam_gc_round (header); a workspace
                            that st_seam_gc_begin never initialised is not run here.  gc_bfs_kernel, gc_side_kernel, gc_info_kernel and the
                            record sums index by thread and tile alone.
     patchmatch             boff, lv, tgt, src, nnf are written by the kernels of the same st_patchmatch_fill call (pm_scan_kernel from
                            block counts of at most 1024 each, lists sized (h - 6)(w - 6)); no entry takes them from the caller, so
                            there is no stage data to feed.

   The restatements apply the same rules through `describe_guarded`, `ms_describe_guarded`, `ransac_guarded`, `ms_ransac_guarded` of
   tests/_classical_cases.py; for the flow `_dense_flow_ref.update` reads a mask byte as set iff nonzero, as the kernel does.

C. Corners of the accepted range: the longest strips, the largest batch, thin seam canvases, saturated pixels.  The restatements form their
   sums in int64 (numpy) and Python ints throughout (asserted in tests/test_classical_reject_cpu.py), so equality here checks the kernels'
   int, int16 and uint16 arithmetic at its extremes: max |gx| = max |It| = 4080, Sobel +-1020, a 15 x 15 window sum past 2^31."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _classical_cases as cc
import _dense_flow_ref as dfref
import _features_ms_ref as msref
import _features_ref as ftref
import _seam_gc_ref as gcref
from _blend_cases import frame_at, intact, workspace_frame

pytestmark = pytest.mark.gpu
FILL = 0xA5


# ---- A: the arena ------------------------------------------------------------------------------------------------------------------------------
def _clamped(entry, rec):
    lim, out = cc.LIMITS[cc.family(entry)], {}
    for k, v in rec.items():
        if k in lim and isinstance(v, int):
            lo, hi = lim[k]
            v = max(v, lo) if hi is None else min(max(v, lo), hi)
        if k.endswith("_channels") and v not in (1, 3):
            v = 3
        out[k] = v
    return out


class Arena:
    """all device operands of an entry in one allocation: operand i at (3 i + 1) slots, a slot at least the largest operand any case of the
    table names (the workspace of a lied-about shape: that of the nearest accepted shape, plus 5 % and a page)"""

    def __init__(self, entry):
        self.entry = entry
        self.ops = [a.name for a in cc.entries()[entry] if a.role in ("in", "out", "ws")]
        self.role = {a.name: a.role for a in cc.entries()[entry]}
        big = 0
        for case in [None] + [c for c in cc.table() if c.entry == entry]:
            rec = cc.base(entry) if case is None else cc.record(case)
            sz = dict(cc.sizes(entry, rec))
            if "workspace" in self.ops:
                sz["workspace"] = int(1.05 * cc._need(entry, _clamped(entry, rec))) + 4096
            big = max(big, max(sz.values()))
        self.slot = (big + 255) // 256 * 256
        self.size = dict(cc.sizes(entry, cc.base(entry)))
        if "workspace" in self.ops:
            self.size["workspace"] = cc.base(entry)["workspace_bytes"]
        total = (3 * len(self.ops) + 1) * self.slot
        self.raw = torch.full((total + 256,), FILL, dtype=torch.uint8, device="cuda")
        self.pad = -self.raw.data_ptr() % 256
        self.buf = self.raw[self.pad:self.pad + total]

    def offset(self, op):
        return (3 * self.ops.index(op) + 1) * self.slot

    def address(self, op):
        return self.buf.data_ptr() + self.offset(op)

    def put(self, op, array):
        flat = torch.from_numpy(np.ascontiguousarray(array).reshape(-1).view(np.uint8).copy())
        self.buf[self.offset(op):self.offset(op) + flat.numel()] = flat.cuda()

    def get(self, op, dtype, shape=None):
        n = self.size[op]
        a = self.buf[self.offset(op):self.offset(op) + n].cpu().numpy().view(dtype)
        return a if shape is None else a.reshape(shape)

    def call(self, rec):
        rc = cc.call(self.entry, rec, self.address)                         # (stream = NULL: the tests run on the default stream)
        torch.cuda.synchronize()
        return rc


def _outs_equal(arena, expected, tag):
    for op, want in expected.items():
        got = arena.get(op, want.dtype, want.shape)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (tag, op, int((got != want).sum()))


def _gc_finish_equals_restatement(arena, ins, from_state):
    """drive the workspace of the arena to the end with the library's own loop, then st_seam_gc_finish into fresh buffers"""
    from stitch_amd._lib import lib
    s = cc._SCALARS["gc"]
    H, W, ws, nbytes = s["H"], s["W"], arena.address("workspace"), arena.size["workspace"]
    status = lambda: arena.get("workspace", np.int32)[:8].tolist()                           # noqa: E731
    st, guard = status(), 0
    while not st[3] and guard < 4096:
        fn = lib.st_seam_gc_relabel if st[1] else lib.st_seam_gc_round
        assert fn(H, W, C.c_void_p(ws), nbytes, None) == 0
        torch.cuda.synchronize()
        st, guard = status(), guard + 1
    assert st[3], (from_state, st)
    sb, side = frame_at((H, W), torch.uint8)
    ib, info = frame_at((4,), torch.int32)
    assert lib.st_seam_gc_finish(H, W, C.c_void_p(side.data_ptr()), C.c_void_p(info.data_ptr()), C.c_void_p(ws), nbytes, None) == 0
    torch.cuda.synchronize()
    wside, winfo = gcref.seam(ins["img1"], ins["img2"], ins["mask1"], ins["mask2"])
    assert winfo[0] == 1 and np.array_equal(side.cpu().numpy(), wside) and np.array_equal(info.cpu().numpy(), winfo), from_state
    assert intact(sb, side) and intact(ib, info)


def _gc_state(stage):
    """the bytes of a workspace after st_seam_gc_begin ("begun") or after the last round ("done"), and the inputs that led there"""
    from stitch_amd._lib import lib
    ins, _ = cc.fixture("st_seam_gc_begin")
    a = Arena("st_seam_gc_begin")
    for op, v in ins.items():
        a.put(op, v)
    assert a.call(cc.base("st_seam_gc_begin")) == 0
    if stage == "done":
        s = cc._SCALARS["gc"]
        for _ in range(4096):
            st = a.get("workspace", np.int32)[:8].tolist()
            if st[3]:
                break
            fn = lib.st_seam_gc_relabel if st[1] else lib.st_seam_gc_round
            assert fn(s["H"], s["W"], C.c_void_p(a.address("workspace")), a.size["workspace"], None) == 0
            torch.cuda.synchronize()
    return a.get("workspace", np.uint8).copy(), ins


@pytest.mark.parametrize("entry", cc.launching(), ids=lambda e: e[3:])
def test_refusals_on_live_buffers(entry):
    arena = Arena(entry)
    ins, expected = cc.fixture(entry)
    gc_ins = None
    if entry in ("st_seam_gc_round", "st_seam_gc_relabel", "st_seam_gc_finish"):
        state, gc_ins = _gc_state("done" if entry == "st_seam_gc_finish" else "begun")
        ins = dict(ins, workspace=state)
    for op, v in ins.items():
        arena.put(op, v)
    before = arena.raw.clone()
    base = cc.base(entry)
    # refused: 1001, and not a byte of the arena moved
    rows = [c for c in cc.refusals(entry) if c.kind != "null"]
    assert len(rows) >= 3
    for case in rows:
        assert arena.call(cc.record(case)) == cc.EINVAL, cc.case_id(case)
        assert torch.equal(arena.raw, before), cc.case_id(case)
    # the base record is accepted and equals the restatement
    assert arena.call(base) == 0
    allowed = torch.zeros_like(arena.raw, dtype=torch.bool)
    for op in arena.ops:
        if arena.role[op] != "in":
            allowed[arena.pad + arena.offset(op):arena.pad + arena.offset(op) + arena.size[op]] = True
    assert not ((arena.raw != before) & ~allowed).any(), "the base call wrote outside its outputs and workspace"
    for op in ins:
        if arena.role[op] == "in":
            assert np.array_equal(arena.get(op, np.uint8), np.ascontiguousarray(ins[op]).reshape(-1).view(np.uint8)), ("input changed", op)
    if expected is not None:
        _outs_equal(arena, expected, "base")
    elif entry == "st_dense_flow_pyramid":
        from stitch_amd import ops
        s, res = cc._SCALARS["df"], cc._df_want()[4]
        L = ops.dense_flow_workspace_layout(s["B"], s["H"], s["W"], s["levels"])
        raw = arena.get("workspace", np.uint8)
        assert L["levels"] == len(res[0][2]["v1"]) == 2
        for l in range(L["levels"]):
            h, w = res[0][2]["v1"][l].shape
            v = raw[L["v"][l]:L["v"][l] + 4 * s["B"] * h * w].view(np.int16).reshape(2, s["B"], h, w)
            m = raw[L["m"][l]:L["m"][l] + 2 * s["B"] * h * w].reshape(2, s["B"], h, w)
            for k in range(s["B"]):
                f = res[k][2]
                assert np.array_equal(v[0, k], f["v1"][l]) and np.array_equal(v[1, k], f["v2"][l]) and np.array_equal(m[0, k], f["m1"][l]) and np.array_equal(m[1, k], f["m2"][l])
    elif entry == "st_seam_gc_finish":
        wside, winfo = gcref.seam(gc_ins["img1"], gc_ins["img2"], gc_ins["mask1"], gc_ins["mask2"])
        assert np.array_equal(arena.get("side_out", np.uint8, wside.shape), wside) and np.array_equal(arena.get("info_out", np.int32), winfo)
    else:                                                                                     # begin, round, relabel: the cut they lead to
        _gc_finish_equals_restatement(arena, gc_ins if gc_ins is not None else ins, entry)
    outs = [op for op in arena.ops if arena.role[op] == "out"] or ["workspace"]
    base_bits = {op: arena.get(op, np.uint8).copy() for op in outs}
    # accepted rows: the same bits as the equal call
    for case in cc.accepted(entry):
        arena.raw.copy_(before)
        if case.equal is not None:
            kind, op = case.equal[0], case.equal[1]
            n = arena.size[op]
            if kind == "copy":
                arena.buf[arena.offset(op):arena.offset(op) + n] = arena.buf[arena.offset(case.equal[2]):arena.offset(case.equal[2]) + n].clone()
            else:
                arena.put(op, np.full(n // 4, 1.0 if kind == "ones" else 0.0, np.float32))
            assert arena.call(base) == 0, cc.case_id(case)
            want_bits = {op: arena.get(op, np.uint8).copy() for op in outs}
            arena.raw.copy_(before)
        else:
            want_bits = base_bits
        assert arena.call(cc.record(case)) == 0, cc.case_id(case)
        for op, want in want_bits.items():
            if cc.record(case)[op] is not None:
                assert np.array_equal(arena.get(op, np.uint8), want), (cc.case_id(case), op)


# ---- B and C: one call inside frames ---------------------------------------------------------------------------------------------------------
def run(entry, scalars, ins, outs, ws=None):
    """the entry on framed operands: every input (an array, or None for a null pointer) and output (bytes) in a sentinel frame of its own,
    the workspace exactly `ws` bytes -> {output: uint8 array}; returns 0, leaves every frame intact and every input as it was"""
    frames, rec = {}, {}
    for a in cc.entries()[entry]:
        if a.role == "scalar":
            rec[a.name] = ws if a.name == "workspace_bytes" else scalars[a.name]
            continue
        rec[a.name] = None
        if a.role == "in" and ins.get(a.name) is not None:
            v = np.ascontiguousarray(ins[a.name])
            frames[a.name] = frame_at((v.nbytes,), torch.uint8, v.reshape(-1).view(np.uint8).copy())
        elif a.role == "out":
            frames[a.name] = frame_at((outs[a.name],), torch.uint8)
        elif a.role == "ws":
            frames[a.name] = workspace_frame(ws)
        if a.name in frames:
            rec[a.name] = cc.Ptr(a.name, 0)
    assert cc.call(entry, rec, lambda op: frames[op][1].data_ptr()) == 0, (entry, scalars)
    torch.cuda.synchronize()
    for name, (buf, view) in frames.items():
        assert intact(buf, view), (entry, name)
        if name in ins:
            assert np.array_equal(view.cpu().numpy(), np.ascontiguousarray(ins[name]).reshape(-1).view(np.uint8)), (entry, name, "input changed")
    return {name: frames[name][1].cpu().numpy() for name in outs}


def _eq(got, want, tag):
    want = np.ascontiguousarray(want)
    g = got.view(want.dtype).reshape(want.shape)
    assert np.array_equal(g.view(np.uint8), want.view(np.uint8)), (tag, int((g != want).sum()))


FT_SIZES = ((65, 97), (96, 128))


@functools.lru_cache(maxsize=None)
def _clean(H, W):
    a = ftref.small_pair(H, W)
    (kp1, box1), (kp2, box2) = ftref.detect(a[0][0]), ftref.detect(a[1][0])
    return dict(kp1=kp1, box1=box1, kp2=kp2, box2=box2, desc1=ftref.describe(box1, kp1), desc2=ftref.describe(box2, kp2))


@pytest.mark.parametrize("size", FT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_describe_on_hostile_keypoints(size):
    H, W = size
    c, N = _clean(H, W), ftref.slots(H, W)
    hostile = cc.hostile_keypoints(H, W, ftref.BORDER, N)
    sc = dict(B=2, H=H, W=W)
    got = run("st_feature_describe", sc, dict(box=np.stack([c["box1"], c["box1"]]).astype(np.uint16), kp=np.stack([c["kp1"], hostile])), dict(desc_out=64 * N))
    want = np.stack([c["desc1"], cc.describe_guarded(c["box1"], hostile)])
    _eq(got["desc_out"], want, "describe")
    assert (want[1] != 0).any() and (want[1][:6] == 0).all()
    solo = run("st_feature_describe", dict(sc, B=1), dict(box=c["box1"][None].astype(np.uint16), kp=c["kp1"][None]), dict(desc_out=32 * N))
    _eq(solo["desc_out"], want[:1], "solo")


@pytest.mark.parametrize("size", FT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ms_describe_on_hostile_keypoints_and_bins(size):
    H, W = size
    levels = 2
    f = msref.features(ftref.small_pair(H, W)[0][0], levels=levels)
    sizes, starts, N = msref.level_sizes(H, W, levels), msref.slot_starts(H, W, levels), msref.slots(H, W, levels)
    assert len(sizes) == (2 if H == 96 else 1)
    kp = np.concatenate([cc.hostile_keypoints(h, w, msref.BORDER, int(starts[l + 1] - starts[l])) for l, (h, w) in enumerate(sizes)])
    if len(sizes) == 2:
        kp[starts[1] + 20] = (W - msref.BORDER - 1, H - msref.BORDER - 1)                   # inside level 0, outside level 1's smaller plane
        kp[starts[1] + 21] = (sizes[1][1] - msref.BORDER - 1, sizes[1][0] - msref.BORDER - 1)
    bins = np.resize(np.array([32, 255, 31, 0, 33, 128, 7, 64], np.uint8), N)
    sc = dict(B=2, H=H, W=W, levels=levels)
    box = msref.pack_levels([np.stack([b, b]) for b in f["box"]]).astype(np.uint16)
    got = run("st_feature_ms_describe", sc, dict(box=box, kp=np.stack([f["kp"], kp]), bins=np.stack([f["bins"], bins])), dict(desc_out=64 * N))
    want = np.stack([f["desc"], cc.ms_describe_guarded(f["box"], kp, bins, H, W, levels)])
    _eq(got["desc_out"], want, "ms describe")
    assert (want[1] != 0).any(1).sum() >= 4 * len(sizes)
    if len(sizes) == 2:
        assert (want[1][starts[1] + 20] == 0).all() and (want[1][starts[1] + 21] != 0).any()
    solo = run("st_feature_ms_describe", dict(sc, B=1), dict(box=msref.pack_levels([b[None] for b in f["box"]]).astype(np.uint16), kp=f["kp"][None], bins=f["bins"][None]),
               dict(desc_out=32 * N))
    _eq(solo["desc_out"], want[:1], "solo")


MATCH_CASES = ("both_unused", "first_unused", "second_unused", "all_equal")


def _match_case(name, c, N):
    kp1, kp2, d1, d2 = c["kp1"].copy(), c["kp2"].copy(), c["desc1"].copy(), c["desc2"].copy()
    if name in ("both_unused", "first_unused"):
        kp1[:] = -1
    if name in ("both_unused", "second_unused"):
        kp2[:] = -1
    if name == "all_equal":
        kp1[:], kp2[:] = (20, 20), (21, 21)
        d1[:], d2[:] = 0x9E3779B9, 0x9E3779B9
    return kp1, d1, kp2, d2


@pytest.mark.parametrize("entry,size", [("st_feature_match", (65, 97)), ("st_feature_match", (96, 128)), ("st_feature_match", (128, 128)), ("st_feature_ms_match", (96, 128))],
                         ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_match_on_unused_and_tied_slots(entry, size):
    """N = 48, N = 64 (128 x 128: exactly one wave of candidates) and, over two levels, N = 96"""
    H, W = size
    ms = entry == "st_feature_ms_match"
    if ms:
        f1, f2 = (msref.features(t[0], levels=2) for t in ftref.small_pair(H, W))
        c, N = dict(kp1=f1["kp"], kp2=f2["kp"], desc1=f1["desc"], desc2=f2["desc"]), msref.slots(H, W, 2)
    else:
        c, N = _clean(H, W), ftref.slots(H, W)
    assert N == {(65, 97): 48, (96, 128): 96 if ms else 48, (128, 128): 64}[size]
    sc = dict(B=2, H=H, W=W, levels=2)
    outs = dict(nn_out=48 * N, matches_out=16 * N, count_out=8)
    clean = ftref.match(c["kp1"], c["desc1"], c["kp2"], c["desc2"])
    assert clean[2] >= 8
    for name in MATCH_CASES:
        kp1, d1, kp2, d2 = _match_case(name, c, N)
        want = ftref.match(kp1, d1, kp2, d2)
        assert want[2] == 0, name
        got = run(entry, sc, dict(kp1=np.stack([c["kp1"], kp1]), desc1=np.stack([c["desc1"], d1]), kp2=np.stack([c["kp2"], kp2]), desc2=np.stack([c["desc2"], d2])), outs)
        _eq(got["nn_out"], np.stack([clean[0], want[0]]).transpose(1, 0, 2, 3), name)
        _eq(got["matches_out"], np.stack([clean[1], want[1]]), name)
        _eq(got["count_out"], np.array([clean[2], 0], np.int32), name)
    solo = run(entry, dict(sc, B=1), dict(kp1=c["kp1"][None], desc1=c["desc1"][None], kp2=c["kp2"][None], desc2=c["desc2"][None]),
               dict(nn_out=24 * N, matches_out=8 * N, count_out=4))
    _eq(solo["matches_out"], clean[1][None], "solo")
    _eq(solo["nn_out"], clean[0][:, None], "solo")


def _ransac_cases(H, W):
    """{name: (kp1, kp2, matches, count)} of the hostile item"""
    kp1, kp2, matches, m = cc.planted_list(H, W)
    N, out = len(kp1), {}
    for name in cc.HOSTILE_COUNTS:
        out["count " + name] = (kp1, kp2, matches, cc.hostile_count(name, N))
    for bad in cc.HOSTILE_INDICES:
        out[f"index {bad}"] = cc.hostile_matches(H, W, bad)
    k1, k2 = kp1.copy(), kp2.copy()
    k1[matches[2, 0]], k2[matches[7, 1]] = -1, -1
    out["unused keypoints in the list"] = (k1, k2, matches, m)
    same = matches.copy()
    same[:m] = matches[4]
    out["all matches identical"] = (kp1, kp2, same, m)
    return out


@pytest.mark.parametrize("entry", ("st_feature_ransac", "st_feature_ms_ransac"), ids=lambda e: e[3:])
@pytest.mark.parametrize("size", FT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ransac_on_hostile_counts_and_indices(entry, size):
    H, W = size
    ms = entry == "st_feature_ms_ransac"
    kw = dict(max_hyp=256, thr=3.0, min_inliers=6, seed=7)
    guarded = (lambda *a: cc.ms_ransac_guarded(*a, 1, **kw)) if ms else (lambda *a: cc.ransac_guarded(*a, **kw))
    ck1, ck2, cm, cn = cc.planted_list(H, W)
    N = len(ck1)
    clean = guarded(ck1, ck2, cm, cn, H, W)
    assert clean[2][0] == 1
    sc = dict(B=2, H=H, W=W, levels=1, **kw)
    need = 32 * 2 * N + 4 * 2 * 256
    outs = dict(motion_out=64, H_out=72, info_out=64, mask_out=2 * N, **(dict(xy_out=64 * N) if ms else {}))
    for name, (kp1, kp2, matches, count) in _ransac_cases(H, W).items():
        want = guarded(kp1, kp2, matches, count, H, W)
        got = run(entry, sc, dict(kp1=np.stack([ck1, kp1]), kp2=np.stack([ck2, kp2]), matches=np.stack([cm, matches]).astype(np.int32), count=np.array([cn, count], np.int32)),
                  outs, ws=need)
        for op, k in (("motion_out", 0), ("H_out", 1), ("info_out", 2), ("mask_out", 3)):
            _eq(got[op], np.stack([clean[k], want[k]]), (name, op))
        if ms:
            _eq(got["xy_out"], np.stack([clean[4], want[4]]).transpose(1, 0, 2, 3), (name, "xy"))
        if name == "all matches identical":
            assert want[2][0] == 0 and want[2][4] == -1 and np.array_equal(want[1], np.eye(3, dtype=np.float32)) and not want[0].any()
        if name in ("count -5", "count 0", "count 7"):
            assert want[2][0] == 0 and want[2][3] == max(cc.hostile_count(name[6:], N), 0)
        if name in ("count N+1", "count i32max"):
            assert want[2][3] == N
    solo = run(entry, dict(sc, B=1), dict(kp1=ck1[None], kp2=ck2[None], matches=cm[None], count=np.array([cn], np.int32)),
               dict(motion_out=32, H_out=36, info_out=32, mask_out=N, **(dict(xy_out=32 * N) if ms else {})), ws=32 * N + 4 * 256)
    _eq(solo["H_out"], clean[1][None], "solo")
    _eq(solo["info_out"], clean[2][None], "solo")


@pytest.mark.parametrize("radius", (4, 7))
def test_flow_iterate_on_hostile_flow_and_mask_bytes(radius):
    """33 x 65: U of +-2^20, +-(2^31 - 1) / 2 and the bound the header states, sample positions exactly at -1, 0, W - 2, W - 1 (and H), mask
    bytes 2 and 255 beside 0 and 1 (set iff nonzero)"""
    H, W = 33, 65
    a, b, m2f, _ = dfref.flow_pair(H, W, 1.5, 3)
    _, _, fields = dfref.dense_flow(a, b, None, m2f, levels=1, iters=2, radius=radius)
    v1, v2, m1, m2, U = fields["v1"][0], fields["v2"][0], fields["m1"][0], fields["m2"][0], fields["u"][0]
    rng = np.random.default_rng(9)
    hm1, hm2 = (rng.choice(np.array([0, 1, 2, 255]), (H, W), p=[0.1, 0.3, 0.3, 0.3]) for _ in range(2))
    hU = cc.hostile_flow(H, W)
    assert np.abs(hU).max() == cc.FLOW_U_BOUND and (256 * (W - 1) + hU[0]).max() < 2 ** 31
    clean, want = dfref.iterate(v1, v2, m1, m2, U, radius, 65536), dfref.iterate(v1, v2, hm1, hm2, hU, radius, 65536)
    assert want[1].any() and not want[1].all()
    px = H * W
    sc = dict(B=2, H=H, W=W, radius=radius, damping=65536)
    ins = dict(v1=np.stack([v1, v1]).astype(np.int16), v2=np.stack([v2, v2]).astype(np.int16), m1=np.stack([m1, hm1]).astype(np.uint8), m2=np.stack([m2, hm2]).astype(np.uint8),
               u=np.stack([U, hU]).astype(np.int32))
    got = run("st_dense_flow_iterate", sc, ins, dict(u_out=16 * px, support_out=2 * px), ws=16 * px)
    _eq(got["u_out"], np.stack([clean[0], want[0]]).astype(np.int32), "u")
    _eq(got["support_out"], np.stack([clean[1], want[1]]).astype(np.uint8), "support")
    solo = run("st_dense_flow_iterate", dict(sc, B=1), {k: v[:1] for k, v in ins.items()}, dict(u_out=8 * px, support_out=px), ws=8 * px)
    _eq(solo["u_out"], clean[0][None].astype(np.int32), "solo")


# ---- C: corners of the accepted range ----------------------------------------------------------------------------------------------------------
def _ft_run(a, b, ms=False, levels=2, max_hyp=256, want=None):
    """the whole front end on framed operands against the restatement (`want`: its result, when the caller has it)"""
    from stitch_amd import ops
    B, _, H, W = a.shape
    sc = dict(B=B, H=H, W=W, levels=levels, oriented=1, max_hyp=max_hyp, thr=3.0, min_inliers=6, seed=1)
    ws = ops.feature_ms_workspace_bytes(B, H, W, levels, max_hyp) if ms else ops.feature_workspace_bytes(B, H, W, max_hyp)
    got = run("st_feature_ms_homography" if ms else "st_feature_homography", sc, dict(img1=a, img2=b), dict(motion_out=32 * B, H_out=36 * B, info_out=32 * B), ws=ws)
    if want is None:
        want = msref.homography(a, b, levels=levels, max_hyp=max_hyp, min_inliers=6) if ms else ftref.homography(a, b, max_hyp=max_hyp, min_inliers=6)
    for op, k in (("motion_out", "motion"), ("H_out", "H"), ("info_out", "info")):
        _eq(got[op], want[k], (op, H, W))
    return want


@pytest.mark.parametrize("ms", (False, True), ids=("features", "features_ms"))
@pytest.mark.parametrize("size", ((64, 1024), (1024, 64)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_features_on_the_longest_strips(size, ms):
    a, b = cc.strip_pair(*size)
    want = _ft_run(a, b, ms)
    assert want["info"][0, 0] == 1 and want["kp1"].shape[1] == 256
    if ms:
        assert len(want["pyr1"]) == 1                                                       # 4 * 64 / 5 < 64: one level


@pytest.mark.parametrize("ms", (False, True), ids=("features", "features_ms"))
def test_features_on_the_largest_batch(ms):
    items = cc.batch_items(64, 64)
    a, b = cc.cycled([i[0] for i in items], 16), cc.cycled([i[1] for i in items], 16)
    assert a.shape == (64, 3, 64, 64)
    four = (msref.homography if ms else ftref.homography)(a[:4], b[:4], max_hyp=256, min_inliers=6, **(dict(levels=2) if ms else {}))
    want = {k: np.concatenate([four[k]] * 16) for k in ("motion", "H", "info")}
    _ft_run(a, b, ms, want=want)
    assert np.array_equal(want["info"][:4], want["info"][60:])


@pytest.mark.parametrize("name", cc.SATURATED)
@pytest.mark.parametrize("ms", (False, True), ids=("features", "features_ms"))
def test_features_on_saturated_pixels(name, ms):
    a, b = cc.saturated_pair(name)
    want = _ft_run(a, b, ms)
    H, W = a.shape[2:]
    if ms:
        pyr = run("st_feature_ms_pyramid", dict(B=1, H=H, W=W, levels=2), dict(img=a), dict(pyr_out=msref.pack_levels(want["pyr1"]).size))
        _eq(pyr["pyr_out"], msref.pack_levels(want["pyr1"]).astype(np.uint8), "pyr")
        N = want["kp1"].shape[1]
        got = run("st_feature_ms_detect", dict(B=1, H=H, W=W, levels=2, oriented=1), dict(pyr=msref.pack_levels(want["pyr1"]).astype(np.uint8)),
                  dict(kp_out=8 * N, bins_out=N, box_out=2 * msref.pack_levels(want["box1"]).size))
        _eq(got["kp_out"], want["kp1"], "kp"), _eq(got["bins_out"], want["bins1"], "bins"), _eq(got["box_out"], msref.pack_levels(want["box1"]).astype(np.uint16), "box")
    else:
        for img, kp, box in ((a, want["kp1"], want["box1"]), (b, want["kp2"], want["box2"])):
            got = run("st_feature_detect", dict(B=1, H=H, W=W), dict(img=img), dict(kp_out=8 * kp.shape[1], box_out=2 * H * W))
            _eq(got["kp_out"], kp, "kp"), _eq(got["box_out"], box.astype(np.uint16), "box")


def _flow_run(a, b, **kw):
    from stitch_amd import ops
    B, _, H, W = a.shape
    sc = dict(B=B, H=H, W=W, levels=8, iters=16, radius=7, damping=65536, mask1_channels=1, mask2_channels=1)
    sc.update(kw)
    got = run("st_dense_flow", sc, dict(img1=a, img2=b, mask1=None, mask2=None), dict(flow_out=8 * B * H * W, support_out=B * H * W),
              ws=ops.dense_flow_workspace_bytes(B, H, W, sc["levels"]))
    return got, sc


@functools.lru_cache(maxsize=None)
def _flow_want(key, levels, iters):
    a, b = cc.flow_items(key)
    return [dfref.dense_flow(a[k], b[k], None, None, levels=levels, iters=iters, radius=7, damping=65536) for k in range(len(a))]


@pytest.mark.parametrize("size", ((16, 1024), (1024, 16), (32, 1024)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_flow_on_the_longest_strips(size):
    """one level at 16 rows, two at 32 (the coarse one 16 x 512); radius 7, iters 16, levels 8"""
    a, b = cc.flow_items(size)
    want = _flow_want(size, 8, 16)
    assert len(want[0][2]["u"]) == (2 if size == (32, 1024) else 1)
    got, _ = _flow_run(a, b)
    _eq(got["flow_out"], np.stack([w[0] for w in want]), "flow")
    _eq(got["support_out"], np.stack([w[1] for w in want]).astype(np.uint8), "support")
    assert want[0][1].any()


def test_flow_on_the_largest_batch():
    a4, b4 = cc.flow_items("batch")
    want = _flow_want("batch", 8, 4)
    a, b = cc.cycled([a4], 16), cc.cycled([b4], 16)
    assert a.shape == (64, 3, 16, 16)
    got, _ = _flow_run(a, b, iters=4)
    flow = np.concatenate([np.stack([w[0] for w in want])] * 16)
    _eq(got["flow_out"], flow, "flow")
    _eq(got["support_out"], np.concatenate([np.stack([w[1] for w in want]).astype(np.uint8)] * 16), "support")
    assert np.array_equal(flow[:4], flow[60:]) and not np.array_equal(flow[0], flow[1])


@pytest.mark.parametrize("name", cc.SATURATED)
def test_flow_on_saturated_pixels(name):
    a, b = cc.saturated_pair(name)
    want = dfref.dense_flow(a[0], b[0], None, None, levels=5, iters=4, radius=7, damping=65536)
    got, _ = _flow_run(a, b, levels=5, iters=4)
    _eq(got["flow_out"], want[0][None], "flow")
    _eq(got["support_out"], want[1][None].astype(np.uint8), "support")


@pytest.mark.parametrize("size", ((1, 4096), (4096, 1), (2, 4096)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_seam_gc_on_the_thinnest_canvases(size):
    """the overlap band crosses five 32-wide tiles; begin, the rounds the status record asks for, finish -- all on framed operands"""
    from stitch_amd import ops
    from stitch_amd._lib import lib
    H, W = size
    i1, i2, k1, k2 = cc.thin_seam_scene(H, W)
    wside, winfo = gcref.seam(i1, i2, k1, k2)
    assert winfo[0] == 1 and 0 < (wside == 0).sum() < 160
    need = ops.seam_gc_workspace_bytes(H, W)
    fr = {n: frame_at((v.nbytes,), torch.uint8, np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy()) for n, v in dict(img1=i1, img2=i2, mask1=k1, mask2=k2).items()}
    fr.update(workspace=workspace_frame(need), side=frame_at((H * W,), torch.uint8), info=frame_at((4,), torch.int32))
    p = lambda n: C.c_void_p(fr[n][1].data_ptr())                                           # noqa: E731
    assert lib.st_seam_gc_begin(p("img1"), p("img2"), p("mask1"), p("mask2"), H, W, p("workspace"), need, None) == 0
    record = fr["workspace"][1][:32].view(torch.int32)
    st, calls = record.tolist(), 0
    while not st[3] and calls < ops.SEAM_GC_MAX_ROUNDS:
        assert (lib.st_seam_gc_relabel if st[1] else lib.st_seam_gc_round)(H, W, p("workspace"), need, None) == 0
        st, calls = record.tolist(), calls + 1
    assert st[3], ("not converged", st)                                                     # converged
    assert lib.st_seam_gc_finish(H, W, p("side"), p("info"), p("workspace"), need, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(fr["side"][1].cpu().numpy().reshape(H, W), wside) and np.array_equal(fr["info"][1].cpu().numpy(), winfo)
    assert all(intact(buf, view) for buf, view in fr.values())
