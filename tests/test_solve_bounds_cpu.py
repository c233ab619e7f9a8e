"""The bars of tests/_solve_bounds.py, shown on the CPU to be neither wrong nor vacuous, and the case tables of
tests/test_solve_matrix_gpu.py.

1. A bar that a correct solver breaks is wrong: solve_kernel, the numpy restatement of tps_solve_kernel (fp64 Gauss-Jordan, the kernel's
   pivot tie order, the f != 0 skip), meets the solve bar at every N of the table and for every kind of control points, and warp_kernel,
   the fp32 restatement of tps_warp_kernel, meets the position bound, the index rule and the pixel bound at every warp case.
2. A bar that a real defect meets is vacuous.  Each planted defect must break a bar in at least one table case, and must change nothing
   where it cannot act.  The contrast that makes the new N values matter: the three defects of the 256-thread stride -- a pivot search
   that sees rows c .. c + 255 only, an elimination that skips rows >= 256, a write-out of T that stops at row 255 -- leave every bit of
   T as it was at N = 169 (n3 = 172, the one size the suite ran before) and at every n3 <= 256, and are caught from n3 = 257 on: the
   last two by the solve bar (T off by 1e7 and more bars, or never written), the first only by the bit-for-bit comparison with the
   restatement, because a narrower pivot search still gives a valid elimination whose T is within rounding of the right one (measured
   here: 0 to 2 of T's 2 n3 fp32 values change).  The ragged-column defect of the warp block changes nothing unless ow % 64 == 1, so it
   too passes at the 24 x 28 and 512 x 512 outputs of the existing tests and is caught at ow = 1, 65 and 129.  The remaining defects (s_T
   at sh + 2 N + 1, the missing + 1e-6, T's rows swapped) act at every N, N = 169 included: they show that the bars bite, not that the
   new sizes are needed.
3. The tables cover their axes, the exclusions stay under their cap for the reference alone, the clamp is exercised on all four sides, the
   inputs keep every logarithm of the system clear of an fp32 rounding midpoint, and the dlt4 / mat3 tables take more than one pivot
   path."""
import functools
import os

import numpy as np
import pytest

import _solve_bounds as sb

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
STRIDE_DEFECTS = ("pivot_window", "elim_256", "write_256")
ALL_N = sb.TPS_N_REGULAR + [sb.TPS_N_LARGE]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def restated(kind, N, b, defect=None):
    src, tgt, _, _ = sb.solve_case(kind, N)
    T, piv = sb.solve_kernel(src[b], tgt[b], defect)
    T.setflags(write=False)
    return T, tuple(piv)


# ================================================================================================ 1. the restatements meet the bars
def test_system_is_stated_as_the_kernel_writes_it():
    src, tgt = sb.solve_inputs("mesh", 9, 1)
    W, rhs = sb.tps_system(src[0], tgt[0])
    N, n3 = 9, 12
    assert W.shape == (n3, n3) and rhs.shape == (n3, 2) and W.dtype == np.float64
    assert np.array_equal(W[:N, 0], np.ones(N)) and np.array_equal(W[:N, 1:3], src[0].astype(np.float64))
    assert np.array_equal(W[N:, :3], np.zeros((3, 3))) and np.array_equal(W[N + 1:, 3:], src[0].T.astype(np.float64)) and np.array_equal(W[N, 3:], np.ones(N))
    R = W[:N, 3:]
    assert np.array_equal(R, R.astype(np.float32).astype(np.float64))                      # fp32 entries, widened
    assert np.array_equal(np.diagonal(R), np.zeros(N))                                     # 0 * log(1e-6): the pivoting is not optional
    assert np.array_equal(rhs[:N], tgt[0].astype(np.float64)) and not rhs[N:].any()
    # the argument of the logarithm is an fp32 sum: stating it in fp64 gives other entries
    s = src[0]
    d2 = ((s[:, None, 0] - s[None, :, 0]) ** 2 + (s[:, None, 1] - s[None, :, 1]) ** 2).astype(np.float32)
    wide = (d2 * np.log(d2.astype(np.float64) + 1e-6).astype(np.float32)).astype(np.float64)
    assert not np.array_equal(wide, R) and np.abs(wide - R).max() < 1e-6
    # and the project's own torch statement of the matrix (oracle.geom.tps_transformer) is this one up to its host's log
    import torch
    p = torch.cat([torch.ones(1, N, 1), torch.from_numpy(s)[None]], 2)
    dd = ((p[:, :, None, :] - p[:, None, :, :]) ** 2).sum(3)
    assert np.abs((dd * torch.log(dd + 1e-6))[0].numpy().astype(np.float64) - R).max() <= 2.0 ** -22


@pytest.mark.parametrize("kind", sb.KINDS)
def test_every_logarithm_is_decided(kind):
    for N in ALL_N:
        src, _ = sb.solve_inputs(kind, N, 3)
        assert all(sb.log_is_decided(src[b]) for b in range(3 if N != sb.TPS_N_LARGE else 1)), (kind, N)
    if kind == "mesh":
        for N in sb.TPS_N:
            assert all(sb.log_is_decided(s) for s in sb.warp_inputs(N, 3)[0]), N


@pytest.mark.parametrize("kind", sb.KINDS)
def test_solve_restatement_meets_the_bar(kind):
    for N in ALL_N:
        for b in range(3 if N != sb.TPS_N_LARGE else 1):
            src, tgt, ref, ctl = sb.solve_case(kind, N)
            r = sb.solve_ratio(restated(kind, N, b)[0], ref[b], ctl[b])
            assert r <= sb.SOLVE_BAR, (kind, N, b, r)
            assert sb.solve_ratio(ctl[b], ref[b], ctl[b]) <= 1.0


def test_reference_converges_and_reproduces_the_system():
    for kind in sb.KINDS:
        for N in (3, 169, 765):
            src, tgt = sb.solve_inputs(kind, N, 1)
            info = {}
            ref = sb.tps_solve_ref(src[0], tgt[0], info)
            assert info["correction"] <= 2.0 ** -36 and ref.dtype == np.longdouble
            W, rhs = sb.tps_system(src[0], tgt[0])
            res = np.abs(W.astype(sb.LD) @ ref.T - rhs).max()
            assert res <= 1e-13 * max(1.0, float(np.abs(ref).max())) * N, (kind, N, float(res))


def test_pivot_tie_order_is_lowest_thread_then_lowest_row():
    """two equal largest candidates in column 0: rows 257 (thread 1, second trip) and 5 (thread 5, first trip) -- thread 1 wins; the plain
    'first largest' rule would take row 5.  The right-hand side makes the system solvable whichever is taken."""
    a = np.abs(np.sin(np.arange(300.0)))
    a[[5, 257]] = 7.0
    assert sb.pick_pivot(a) == 257 and int(np.argmax(a)) == 5
    a[257] = np.nan
    assert sb.pick_pivot(a) == 5 and sb.pick_pivot(np.full(300, np.nan)) == 0 and sb.pick_pivot(np.zeros(300)) == 0
    # in the table's own systems column 0 is all ones: the merge must fall back to row 0 (thread 0, first trip), not the last equal one
    for N in (254, 765):
        assert restated("mesh", N, 0)[1][0] == 0


# ================================================================================================ 2. planted defects
@pytest.mark.parametrize("defect", STRIDE_DEFECTS)
def test_stride_defects_pass_up_to_256_rows_and_are_caught_beyond(defect):
    caught = []
    for kind in sb.KINDS:
        for N in sb.TPS_N_REGULAR:
            if N + 3 <= 256 and (kind != "mesh" and N not in (169, 253)):
                continue                                                   # where it cannot act: the mesh at every such N, the others at 169 and 253
            src, tgt, ref, ctl = sb.solve_case(kind, N)
            good, gp = restated(kind, N, 0)
            T, piv = restated(kind, N, 0, defect)
            same = np.array_equal(bits(T), bits(good))
            if N + 3 <= 256:
                assert same and piv == gp, (defect, kind, N)
                continue
            r = sb.solve_ratio(T, ref[0], ctl[0])
            if r > sb.SOLVE_BAR or not same:
                caught.append((kind, N, "solve bar" if r > sb.SOLVE_BAR else "bit for bit"))
    assert caught, defect
    if defect == "pivot_window":
        assert all(how == "bit for bit" for _, _, how in caught)           # the accuracy bar alone cannot see it (the docstring)
        assert any(restated(k, N, 0, defect)[1] != restated(k, N, 0)[1] for k in sb.KINDS for N in (254, 509, 510, 765))
    else:
        assert [(k, N) for k, N, how in caught if how == "solve bar"] == [(k, N) for k in sb.KINDS for N in sb.TPS_N_REGULAR if N + 3 > 256], caught
        assert caught[0][1] == 254                                         # n3 = 257, the first size with a second trip


def test_missing_epsilon_is_caught_at_every_size():
    for N in (3, 169, 254):
        src, tgt, ref, ctl = sb.solve_case("mesh", N)
        assert sb.solve_ratio(restated("mesh", N, 0, "no_eps")[0], ref[0], ctl[0]) > sb.SOLVE_BAR          # 0 * log(0): NaN on the diagonal


def run_warp(i, case, defect=None, b=0, factor=1.0):
    N, in_hw, out_hw, C = case
    src, tgt = sb.warp_inputs(N, sb.WARP_B)
    T = sb.tps_solve_control(src[b], tgt[b])
    img = sb.image(C, *in_hw, seed=70000 + 4 * i + b)
    pos, idx, out = sb.warp_kernel(img, src[b], T, out_hw, defect)
    return src[b], T, pos, sb.warp_check(img, src[b], T, in_hw, out_hw, idx, out, factor)


def warp_passes(res):
    return res["idx_ok"] and res["out_ratio"] <= 1.0


def test_warp_restatement_meets_its_bounds_and_the_cap_holds():
    for i, case in enumerate(sb.WARP_CASES):
        N, in_hw, out_hw, C = case
        for b in range(sb.WARP_B):
            src, T, pos, res = run_warp(i, case, b=b)
            p64, E = sb.tps_positions_ref(src, T, out_hw)
            assert float((np.abs(pos.astype(np.float64) - p64) / E).max()) <= 1.0, case
            assert warp_passes(res), (case, b, res["idx_ok"], res["out_ratio"])
            # the cap, for the reference alone and with a quarter more than E: the kernel's own T moves a position by far less
            assert run_warp(i, case, b=b, factor=1.25)[3]["left_out"] <= sb.CAP, case
            x, y, _, _ = res["pos"]
            left, right, top, bottom = sb.outside_shares(x, y, in_hw)
            if out_hw[1] >= 28:
                assert left >= 0.08 and right >= 0.08, (case, left, right)
            if out_hw[0] >= 24:
                assert top >= 0.08 and bottom >= 0.08, (case, top, bottom)


@pytest.mark.parametrize("defect", ("lds_shift", "swap_rows", "ragged_ow"))
def test_warp_defects_are_caught(defect):
    caught = []
    for i, case in enumerate(sb.WARP_CASES):
        N, in_hw, out_hw, C = case
        if defect != "ragged_ow" and N not in (3, 169, 254, 765):
            continue
        ok = warp_passes(run_warp(i, case, defect)[3])
        if defect == "ragged_ow":
            assert ok == (out_hw[1] % 64 != 1), case                       # caught at ow = 1, 65, 129 and nowhere else: 24 x 28 passes
        if not ok:
            caught.append(case)
    assert caught, defect
    if defect != "ragged_ow":                                              # these act at every N (three points give a plane: the lost weight is 0)
        assert {c[0] for c in caught} >= {169, 254, 765}, caught


# ================================================================================================ 3. the tables
def test_tables_cover_their_axes():
    n3 = [N + 3 for N in sb.TPS_N]
    assert min(n3) == 4 and {255, 256, 257, 512, 513, 768} <= set(n3) and 172 in n3
    assert {(n - 1) // 256 + 1 for n in n3} == {1, 2, 3}                   # trips of the 256-thread stride; the large case begins a fifth
    assert (sb.TPS_N_LARGE + 3 - 1) // 256 + 1 == 5 and 8.0e6 < (sb.TPS_N_LARGE + 3) * (sb.TPS_N_LARGE + 5) * 8 < 8.5e6
    assert sb.TPS_N_REGULAR == [N for N in sb.TPS_N if N >= 3] and sb.SINGULAR_N == [N for N in sb.TPS_N if N < 3]
    assert {oh % 4 for oh, _ in sb.TPS_OUT_HW} == {0, 1, 2, 3} and {0, 1, 63} <= {ow % 64 for _, ow in sb.TPS_OUT_HW}
    assert any(oh > 4 for oh, _ in sb.TPS_OUT_HW) and any(ow > 128 for _, ow in sb.TPS_OUT_HW) and (24, 28) in sb.TPS_OUT_HW
    assert {(1, 1), (1, 64), (4, 63), (5, 65), (3, 129), (24, 28)} <= set(sb.TPS_OUT_HW)
    for N in sb.TPS_N_REGULAR:
        assert {c[2] for c in sb.WARP_CASES if c[0] == N} == set(sb.TPS_OUT_HW)
    for a, b in ((1, 2), (1, 3), (2, 3)):                                  # every pair of input size, output size and channel count occurs
        want = {(x, y) for x in (sb.TPS_IN_HW, sb.TPS_OUT_HW, sb.TPS_C)[a - 1] for y in (sb.TPS_IN_HW, sb.TPS_OUT_HW, sb.TPS_C)[b - 1]}
        assert {(c[a], c[b]) for c in sb.WARP_CASES} == want, (a, b)
    assert {(k, N, B) for k, N, B in sb.SOLVE_CASES} == {(k, N, B) for k in sb.KINDS for N in sb.TPS_N_REGULAR for B in (1, 3)}
    assert sb.DLT_B == [1, 63, 64, 65, 130] and sb.MAT3_B == sb.DLT_B and sb.DLT_DIV == [1.0, 8.0]
    assert 16 * 4000 + 24 == 64024 < 65536                                  # the warp's LDS at the entry's limit of N, not in the table


def test_the_singular_sets_are_singular_and_the_regular_kinds_are_not():
    for kind in sb.SINGULAR:
        src, tgt = sb.solve_inputs(kind, 9, 1)
        s = np.linalg.svd(sb.tps_system(src[0], tgt[0])[0], compute_uv=False)
        assert s[-1] <= 1e-14 * s[0], (kind, s[-1] / s[0])
    for N in sb.SINGULAR_N:                                                # fewer than three points lie on one line: [0 | P^T] has rank N < 3
        src, tgt = sb.solve_inputs("mesh", N, 1)
        s = np.linalg.svd(sb.tps_system(src[0], tgt[0])[0], compute_uv=False)
        assert s[-1] <= 1e-14 * s[0], N
    cond = {kind: np.linalg.cond(sb.tps_system(*(a[0] for a in sb.solve_inputs(kind, 169, 1)))[0]) for kind in sb.KINDS}
    assert cond["mesh"] < 1e5 < 20 * cond["mesh"] < cond["tight"] < 1e9, cond          # the model's 4e4; badly conditioned, but regular


def test_dlt_table_takes_several_pivot_paths_and_equals_its_oracle_form():
    seqs = set()
    for i, (B, div, with_motion, mscale) in enumerate(sb.DLT_CASES):
        src, motion = sb.dlt_inputs(B, mscale, 300 + i)
        dst = sb.dlt_dst(src, motion if with_motion else None, mscale, B)
        assert np.abs(motion).max() <= 0.3 * 512 and (with_motion or np.array_equal(dst[0], src))
        for b in range(min(B, 8)):
            seqs.add(sb.dlt_pivots((src / np.float32(div)).astype(np.float32), (dst[b] / np.float32(div)).astype(np.float32)))
    assert len(seqs) >= 2, seqs
    src, motion = sb.dlt_inputs(5, (1.0, 1.0), 1)
    H = sb.dlt4_ref(src, None, (1.0, 1.0), 8.0, 5)                         # without motion dst = src: the identity up to the solve's rounding
    assert H.shape == (5, 3, 3) and np.abs(H - np.eye(3)).max() < 1e-3 and np.array_equal(H[0], H[4])


def test_mat3_table_takes_both_sides_of_every_pivot_choice():
    g = np.load(os.path.join(GOLDEN, "branches_kernel.npz"))
    assert g["k_cm_in"].shape[0] >= max(sb.MAT3_B) and g["k_cm_in"].shape == g["k_cm_inv"].shape
    X = sb.mat3_inputs(max(sb.MAT3_B))
    piv = np.array([sb.mat3_pivots(x) for x in X])
    for k in (0, 1):
        stay, swap = int((piv[:, k] == k).sum()), int((piv[:, k] != k).sum())
        assert stay > 0 and swap > 0, (k, stay, swap)
    assert (piv[:, 2] == 2).all()
