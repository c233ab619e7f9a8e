"""The geometric solvers of csrc/geom.hip -- st_tps_solve_grid (tps_solve_kernel, tps_warp_kernel), st_dlt4, st_mat3_sandwich -- over the
sizes at which a 256-thread stride, a 4 x 64 pixel block, a 64-thread block or a batch stride can go wrong, which the single-shape tests of
test_ops_gpu.py (N = 169, B = 2, C = 3) never reach.  The generators, references, bars and case tables are those of
tests/_solve_bounds.py; tests/test_solve_bounds_cpu.py shows on the CPU that restatements of the kernels meet the bars, that planted
defects do not, and that the tables cover their axes.

Every operand -- the control points, the image, T, the fp64 work area, out and idx (an integer sentinel) -- sits at an offset inside a
NaN-filled buffer (frame / frame_intact of tests/test_geom_matrix_gpu.py, the nan_wide / untouched idea of test_split3_matrix_gpu.py):
every frame must be intact afterwards, a buffer that a form of the call leaves out must be untouched altogether, and a read outside an
input view would put a NaN into a result.  The entries are called through lib.st_* directly.

1. TPS solve, per (kind, N, B):  e_max(T) <= 4 max(e_max(control), 2^-24 max|T_ref|), both against the refined reference, the ratio recorded
   for every case; T equals the numpy restatement of the kernel bit for bit (every step of the elimination is one IEEE fp64 operation on
   one row, so nothing but the pivot order and the operation order decides the bits: this is the bar that sees a narrowed pivot search);
   item b of a B = 3 call equals the same item solved alone, bit for bit.
2. TPS warp, per (N, in_hw, out_hw, C): positions and taps from the kernel's returned T.  idx equals oracle.geom.tps_indices and the
   fp64 floor except where the fp64 position lies within E of a deciding integer (at most 1 % of a case, else the test fails); out is
   within the pixel bound of the fp64 `_interpolate` on the remaining samples; max err / E recorded.
3. The optional forms (out = NULL, idx = NULL, both) give the same T, idx and out bit for bit; the ST_EINVAL guards return 1001 and
   launch nothing.
4. A singular item (two coincident points; all points on one line; fewer than three points) does not poison its neighbours.
5. dlt4 and 6. mat3_sandwich equal the project's bit-exact restatements at every B around the 64-thread block."""
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _solve_bounds as sb  # noqa: E402
from _measure import check  # noqa: E402
from test_geom_matrix_gpu import _KEEP, SENTINEL, cid, frame, frame_intact, put  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ST_EINVAL = 1001
LARGE_SECONDS = 5.0                                              # "a few seconds": the budget of one case of this suite


@pytest.fixture(scope="module")
def st():
    """the C entry points, the error check and the two helpers of ops.py that turn a tensor into a pointer and name the stream"""
    import stitch_amd
    from stitch_amd._lib import check as rc_check
    from stitch_amd._lib import lib
    assert torch.cuda.is_available()

    class St:
        pass
    s = St()
    s.lib, s.check, s.p, s.stream = lib, rc_check, stitch_amd.ops._p, stitch_amd.ops._stream
    return s


@pytest.fixture(autouse=True)
def _release_frames():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def all_fill(buf):
    """a buffer that the call must not have touched at all, view included"""
    return bool(torch.isnan(buf).all()) if buf.dtype.is_floating_point else bool((buf == SENTINEL[buf.dtype]).all())


def run_tps(st, src, tgt, img=None, out_hw=(0, 0), want_out=False, want_idx=False, in_hw=None):
    """one call of st_tps_solve_grid with every operand framed.  src, tgt [B, N, 2] numpy; img [B, C, H, W] numpy or None.  The frames of
    out and idx exist in every form; a form that leaves one out hands NULL and the whole buffer must keep its fill.
    -> dict(T [B, 2, n3], out [B, C, oh, ow] or None, idx [B, oh, ow, 4] or None, seconds)"""
    B, N, _ = src.shape
    n3 = N + 3
    oh, ow = out_hw
    Cc, H, W = (img.shape[1:] if img is not None else (0,) + tuple(in_hw or (0, 0)))
    s, t = put(torch.from_numpy(np.array(src))), put(torch.from_numpy(np.array(tgt)))             # copies: the cached cases are read-only
    Ud = put(torch.from_numpy(np.ascontiguousarray(img))) if img is not None else None
    bw, work = frame((B * n3 * (N + 5),), torch.float64)
    bT, T = frame((B, 2, n3))
    bo, out = frame((B, max(Cc, 1), max(oh, 1), max(ow, 1)))
    bi, idx = frame((B, max(oh, 1), max(ow, 1), 4), torch.int32)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st.check(st.lib.st_tps_solve_grid(st.p(Ud), st.p(s), st.p(t), st.p(work), st.p(T), st.p(out) if want_out else None,
                                      st.p(idx) if want_idx else None, B, Cc, H, W, N, oh, ow, st.stream()), "st_tps_solve_grid")
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    assert frame_intact(bw, work) and frame_intact(bT, T), "a write outside the work area or outside T"
    assert frame_intact(bo, out) if want_out else all_fill(bo), "out: a write outside the view, or into a buffer the call was not given"
    assert frame_intact(bi, idx) if want_idx else all_fill(bi), "idx: a write outside the view, or into a buffer the call was not given"
    return dict(T=T.cpu().numpy(), out=out.cpu().numpy() if want_out else None, idx=idx.cpu().numpy() if want_idx else None, seconds=seconds)


_RESTATED = {}


def restated(kind, N, b):
    if (kind, N, b) not in _RESTATED:
        src, tgt, _, _ = sb.solve_case(kind, N)
        _RESTATED[kind, N, b] = sb.solve_kernel(src[b], tgt[b])[0]
    return _RESTATED[kind, N, b]


# ================================================================================================ 1. the solve
def solve_bars(name, kind, N, T, items):
    """the ratio of every item recorded as the case's largest, then the bar and the bit-for-bit comparison with the restatement"""
    src, tgt, ref, ctl = sb.solve_case(kind, N)
    ratio = max(sb.solve_ratio(T[k], ref[b], ctl[b]) for k, b in enumerate(items))
    failed = []
    try:
        check(f"solve_tps_{name}_max_over_ctl", ratio, sb.SOLVE_BAR, inclusive=True,
              note="e_max(T) / max(e_max(numpy fp64 solve rounded to fp32), 2^-24 max|T_ref|), both against the refined reference (tests/_solve_bounds.py)")
    except AssertionError as e:
        failed.append(str(e))
    for k, b in enumerate(items):
        differ = int((bits(T[k]) != bits(restated(kind, N, b))).sum())
        if differ:
            failed.append(f"item {b}: {differ} of {T[k].size} values of T differ from the restatement of tps_solve_kernel")
    assert not failed, "; ".join(failed)


@pytest.mark.parametrize("case", sb.SOLVE_CASES, ids=cid)
def test_tps_solve_matrix(st, case):
    kind, N, B = case
    src, tgt, _, _ = sb.solve_case(kind, N)
    got = run_tps(st, src[:B], tgt[:B])
    solve_bars(cid(case), kind, N, got["T"], list(range(B)))
    if B > 1:                                                    # batch items are independent: each equals its solo run, bit for bit
        for b in range(B):
            solo = run_tps(st, src[b:b + 1], tgt[b:b + 1])["T"][0]
            assert np.array_equal(bits(solo), bits(got["T"][b])), (case, b)


def test_tps_solve_large(st):
    """N = 1024 (n3 = 1027: a fifth trip of the 256-thread stride begun, an 8 MB work area), the solver alone.  The wall time of the call is
    recorded and held under LARGE_SECONDS: the case is in the suite on the condition that it takes no more than a few seconds (1.1 s when it
    was added, profiles/solve_matrix_measured.json).  N = 4000, the entry's limit, is a single-workgroup elimination of a 4003^2 system whose
    time has not been measured: it is not in the suite."""
    kind, N = "mesh", sb.TPS_N_LARGE
    src, tgt, _, _ = sb.solve_case(kind, N)
    run_tps(st, src[:1], tgt[:1])                                # the first call pays for loading the code object
    got = run_tps(st, src[:1], tgt[:1])
    solve_bars(f"{kind}_{N}_1", kind, N, got["T"], [0])
    check("solve_tps_large_N1024_seconds", got["seconds"], LARGE_SECONDS, note="wall time of one st_tps_solve_grid call, solver only, B = 1; the case's condition for staying in the suite")


# ================================================================================================ 2. the warp
def warp_case_inputs(case):
    N, in_hw, out_hw, Cc = case
    i = sb.WARP_CASES.index(case)
    src, tgt = sb.warp_inputs(N, sb.WARP_B)
    img = np.stack([sb.image(Cc, *in_hw, seed=70000 + 4 * i + b) for b in range(sb.WARP_B)])
    return src, tgt, img


def warp_bars(name, case, src, img, got, items=None):
    """the index rule and the pixel bound of every item from the kernel's own T; the figures are recorded before any is asserted"""
    from oracle import geom
    N, in_hw, out_hw, Cc = case
    oh, ow = out_hw
    worst, left, failed = 0.0, 0.0, []
    for b in (items if items is not None else range(src.shape[0])):
        T = got["T"][b]
        idx = got["idx"][b].reshape(oh * ow, 4)
        res = sb.warp_check(img[b], src[b], T, in_hw, out_hw, idx, got["out"][b].reshape(Cc, oh * ow))
        worst, left = max(worst, res["out_ratio"]), max(left, res["left_out"])
        if not res["idx_ok"]:
            failed.append(f"item {b}: idx differs from the fp64 floor at a sample that is not within E of an integer")
        want = geom.tps_indices(torch.from_numpy(src[b:b + 1]), torch.from_numpy(T[None]), in_hw, out_hw).numpy().reshape(oh * ow, 4)
        keep = ~res["near"]
        if not np.array_equal(idx[keep], want[keep]):
            failed.append(f"item {b}: idx differs from oracle.geom.tps_indices at a sample that is not within E of an integer")
    for nm, val, bound, note in ((f"solve_warp_{name}_err_over_E", worst, 1.0, "|out - fp64 _interpolate| <= E on the samples kept (tests/_solve_bounds.py)"),
                                 (f"solve_warp_{name}_left_out", left, sb.CAP, "share of samples within E of a deciding integer")):
        try:
            check(nm, val, bound, inclusive=True, note=note)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "; ".join(failed)


@pytest.mark.parametrize("case", sb.WARP_CASES, ids=cid)
def test_tps_warp_matrix(st, case):
    N, in_hw, out_hw, Cc = case
    src, tgt, img = warp_case_inputs(case)
    got = run_tps(st, src, tgt, img, out_hw, want_out=True, want_idx=True)
    assert np.isfinite(got["T"]).all() and np.isfinite(got["out"]).all()
    warp_bars(cid(case), case, src, img, got)


# ================================================================================================ 3. the optional forms and the guards
@pytest.mark.parametrize("case", [(4, (2, 2), (5, 65), 1), (254, (32, 40), (5, 65), 3), (510, (32, 40), (3, 129), 4)], ids=cid)
def test_tps_optional_forms(st, case):
    """out = NULL with idx (no image, C = 0), idx = NULL with out, both NULL (solve only: U = NULL, C = 0, no sizes): T, idx and out are
    bit-identical across the forms, and run_tps requires the buffer a form leaves out to keep its fill throughout."""
    N, in_hw, out_hw, Cc = case
    src, tgt = sb.warp_inputs(N, sb.WARP_B)
    img = np.stack([sb.image(Cc, *in_hw, seed=81000 + b) for b in range(sb.WARP_B)])
    both = run_tps(st, src, tgt, img, out_hw, want_out=True, want_idx=True)
    only_idx = run_tps(st, src, tgt, None, out_hw, want_idx=True, in_hw=in_hw)
    only_idx_with_image = run_tps(st, src, tgt, img, out_hw, want_idx=True)
    only_out = run_tps(st, src, tgt, img, out_hw, want_out=True)
    solve_only = run_tps(st, src, tgt)
    for other in (only_idx, only_idx_with_image, only_out, solve_only):
        assert np.array_equal(bits(other["T"]), bits(both["T"]))
    assert np.array_equal(only_idx["idx"], both["idx"]) and np.array_equal(only_idx_with_image["idx"], both["idx"])
    assert np.array_equal(bits(only_out["out"]), bits(both["out"]))
    warp_bars("forms_" + cid(case), case, src, img, both)


def test_tps_guards_reject_before_any_launch(st):
    """N = 0, N = 4001, B = 0, out without U, oh = 0 with idx: each returns ST_EINVAL and no buffer is written"""
    N, B, Cc, H, W, oh, ow = 4, 1, 1, 2, 2, 3, 3
    src, tgt = sb.warp_inputs(N, B)
    s, t = put(torch.from_numpy(src)), put(torch.from_numpy(tgt))
    Ud = put(torch.from_numpy(sb.image(Cc, H, W, 1)[None]))
    bw, work = frame((B * (N + 3) * (N + 5),), torch.float64)
    bT, T = frame((B, 2, N + 3))
    bo, out = frame((B, Cc, oh, ow))
    bi, idx = frame((B, oh, ow, 4), torch.int32)
    p = st.p
    good = dict(U=p(Ud), out=p(out), idx=p(idx), B=B, C=Cc, H=H, W=W, N=N, oh=oh, ow=ow)
    for name, change in (("N = 0", dict(N=0)), ("N = 4001", dict(N=4001)), ("B = 0", dict(B=0)), ("out without U", dict(U=None)),
                         ("oh = 0 with idx", dict(oh=0, out=None)), ("C = 0 with out", dict(C=0))):
        a = dict(good, **change)
        rc = st.lib.st_tps_solve_grid(a["U"], p(s), p(t), p(work), p(T), a["out"], a["idx"], a["B"], a["C"], a["H"], a["W"], a["N"], a["oh"], a["ow"], st.stream())
        torch.cuda.synchronize()
        assert rc == ST_EINVAL, (name, rc)
        assert all_fill(bw) and all_fill(bT) and all_fill(bo) and all_fill(bi), name


# ================================================================================================ 4. singular items
def same_item(a, b, ka, kb):
    return all(np.array_equal(np.ascontiguousarray(a[f][ka]).view(np.uint32), np.ascontiguousarray(b[f][kb]).view(np.uint32)) for f in ("T", "out", "idx"))


@pytest.mark.parametrize("kind", sb.SINGULAR)
@pytest.mark.parametrize("N", [9, 254])
def test_tps_singular_item_leaves_its_neighbours_alone(st, kind, N):
    """B = 3, the middle item singular (two coincident control points: two equal rows; all points on one line: dependent columns): items 0
    and 2 equal their solo runs bit for bit -- T, idx and out -- and every frame is intact.  Nothing is asserted about the singular item's
    values.  This is NaN arithmetic, not a fault: the elimination divides by a zero pivot and T becomes inf / NaN; in tps_warp_kernel a NaN
    position reaches taps_from_normalised, where floorf keeps it NaN, f2i_x86 fails its range test (a NaN compares false) and returns
    INT_MIN, the unsigned + 1 gives INT_MIN + 1, and clampi brings both to index 0 (an infinite or huge position takes the same road), so
    every gather stays inside the image and the NaN weights only reach that item's own pixels.  That path was read before this case was
    written (csrc/geom.hip: f2i_x86, clampi, taps_from_normalised)."""
    in_hw, out_hw, Cc = (32, 40), (5, 65), 3
    src, tgt = sb.warp_inputs(N, 3)
    bad_s, bad_t = sb.solve_inputs(kind, N, 1)
    src, tgt = src.copy(), tgt.copy()
    src[1], tgt[1] = bad_s[0], bad_t[0]
    img = np.stack([sb.image(Cc, *in_hw, seed=82000 + b) for b in range(3)])
    got = run_tps(st, src, tgt, img, out_hw, want_out=True, want_idx=True)
    for b in (0, 2):
        solo = run_tps(st, src[b:b + 1], tgt[b:b + 1], img[b:b + 1], out_hw, want_out=True, want_idx=True)
        assert same_item(got, solo, b, 0), (kind, N, b)
    assert np.isfinite(got["T"][[0, 2]]).all() and np.isfinite(got["out"][[0, 2]]).all()
    assert (got["idx"] >= 0).all() and (got["idx"][..., :2] < in_hw[1]).all() and (got["idx"][..., 2:] < in_hw[0]).all()
    warp_bars(f"singular_{kind}_{N}", (N, in_hw, out_hw, Cc), src, img, got, items=(0, 2))


@pytest.mark.parametrize("N", sb.SINGULAR_N)
def test_tps_fewer_than_three_points(st, N):
    """N = 1 and 2, the smallest systems (n3 = 4, 5): fewer than three points always lie on one line, so [0 | P^T] has rank N < 3 and the
    system is singular whatever the points are.  No value is asserted: every frame intact, every index inside the image, and each item of a
    B = 3 call equal to its solo run bit for bit, NaN payloads included."""
    in_hw, out_hw, Cc = (2, 2), (5, 65), 3
    src, tgt = sb.warp_inputs(N, 3)
    img = np.stack([sb.image(Cc, *in_hw, seed=83000 + b) for b in range(3)])
    got = run_tps(st, src, tgt, img, out_hw, want_out=True, want_idx=True)
    assert (got["idx"] >= 0).all() and (got["idx"] < 2).all()
    for b in range(3):
        solo = run_tps(st, src[b:b + 1], tgt[b:b + 1], img[b:b + 1], out_hw, want_out=True, want_idx=True)
        assert same_item(got, solo, b, 0), (N, b)


# ================================================================================================ 5. dlt4
@pytest.mark.parametrize("case", sb.DLT_CASES, ids=cid)
def test_dlt4_matrix(st, case):
    B, div, with_motion, mscale = case
    src, motion = sb.dlt_inputs(B, mscale, 300 + sb.DLT_CASES.index(case))
    bH, H = frame((B, 3, 3))
    m = put(torch.from_numpy(motion)) if with_motion else None
    st.check(st.lib.st_dlt4(st.p(put(torch.from_numpy(src))), st.p(m), st.p(H), B, mscale[0], mscale[1], div, st.stream()), "st_dlt4")
    torch.cuda.synchronize()
    assert frame_intact(bH, H)
    want = sb.dlt4_ref(src, motion if with_motion else None, mscale, div, B)
    assert np.array_equal(bits(H.cpu().numpy()), bits(want)), case


# ================================================================================================ 6. mat3_sandwich
@pytest.mark.parametrize("case", sb.MAT3_CASES, ids=cid)
def test_mat3_sandwich_matrix(st, case):
    """invert 0 / 1: general matrices between the model's scale pair against oracle.geom.inverse / matmul3; invert 2 (the column-major
    inverse): the recorded set of tests/golden/branches_kernel.npz sliced to B, between identities against the recorded inverses and
    between the scale pair against their products"""
    import torch as th
    from oracle import geom
    B, invert = case
    M = sb.MODEL_M
    Minv = geom.inverse(th.from_numpy(M)).numpy()

    def run(L, X, R):
        bO, O = frame((B, 3, 3))
        st.check(st.lib.st_mat3_sandwich(st.p(put(th.from_numpy(L))), st.p(put(th.from_numpy(np.ascontiguousarray(X)))), st.p(put(th.from_numpy(R))), st.p(O), B, invert,
                                         st.stream()), "st_mat3_sandwich")
        th.cuda.synchronize()
        assert frame_intact(bO, O)
        return O.cpu().numpy()
    if invert < 2:
        X = sb.mat3_inputs(B)
        assert np.array_equal(bits(run(Minv, X, M)), bits(sb.mat3_ref(Minv, X, M, invert))), case
        return
    g = np.load(os.path.join(GOLDEN, "branches_kernel.npz"))
    X, Xi = g["k_cm_in"][:B].astype(np.float32), g["k_cm_inv"][:B].astype(np.float32)
    eye = np.eye(3, dtype=np.float32)
    assert np.array_equal(bits(run(eye, X, eye)), bits(Xi)), case
    assert np.array_equal(bits(run(Minv, X, M)), bits(sb.mat3_ref(Minv, Xi, M, 0))), case
