"""What tests/test_post_matrix_gpu.py relies on, shown on the CPU: the references of tests/_post_bounds.py are the operations the kernels of
csrc/tps_pipeline.hip, csrc/tps_solve.h and csrc/inpaint.hip state, their tables cover the axes they claim, their bars are neither wrong nor
vacuous, and the entry points reject what their kernels cannot take.

1. Bit-exact bars: torch's own reductions add in the order the kernels add (the in-order restatements give the same bits on every case), and
   the generators reach every threshold the references decide at (>= 3.0, >= 0.5, 0 / 0, 0 and 255), so nothing is left out of torch.equal.
2. A planted defect must fail: for each covered kernel one mutation of its restatement (a bounds test one short, `>=` for `>` in the tie rule,
   a stride loop without its second trip, the ring window on the unwrapped difference, ...) changes a result on a case of the table.
3. The control rule of the solves holds for the reference itself and for the restated elimination, and fails for the planted defects.
4. Host-side rejections: no pointer is dereferenced."""
import itertools

import numpy as np
import pytest
import torch

import _post_bounds as pb

EINVAL = 1001
P0 = 0x7f0000000000                                   # never dereferenced: every call below must return before a launch


def ptrs(n):
    return [P0 + (i << 28) for i in range(n)]


# ================================================================================================ 1. tables and references
def test_shape_tables_cover_their_axes():
    assert {h for h, _ in pb.SHAPES} == {1, 3, 4, 5, 9} and {w for _, w in pb.SHAPES} == {1, 2, 63, 64, 65, 130}
    assert {(1, 1), (5, 65), (9, 130)} <= set(pb.SHAPES) and len(set(pb.SHAPES)) == len(pb.SHAPES)
    assert {255, 256, 257} <= {h * w for h, w in pb.FLAT_SHAPES}
    p = pb.BOXAVG_PARAMS
    assert {q[0] for q in p} == {1, 3, 11} and {q[1][0] * q[1][1] for q in p} == {1, 2, 6} and {q[2] for q in p} == {False, True} == {q[3] for q in p}
    assert any(h < 11 and w < 11 for h, w in pb.SHAPES) and any(h < 3 or w < 3 for h, w in pb.SHAPES)      # windows wider than the image
    for k in (1, 3, 11):
        assert {(q[2], q[3]) for q in p if q[0] == k} == set(itertools.product((False, True), repeat=2)), k
    assert set(pb.MINMAX_K) == {1, 5, 11} and set(pb.MINMAX_PLANES) == {1, 4} and max(pb.MASK_INV_C) > 6
    assert {k for k, _, _ in pb.BOX_GEOM} == {3, 7, 8, 16} and all(pad == k // 2 for k, pad, _ in pb.BOX_GEOM)
    assert {dh for k, _, dh in pb.BOX_GEOM if k % 2 == 0} == {1, 0, -1}                   # the erosion's larger domain, the crops
    got = {(c[0][1], c[0][5]) for s in pb.SHAPES for c in pb.box_cases_of(s)}
    assert got == set(itertools.product((3, 7, 8, 16), (0, 1, 2)))
    assert set(pb.GATHER_P) == {1, 3} and set(pb.GATHER_N) == {1, 255, 257}


def test_reductions_add_in_the_kernels_order():
    """the bit-exact bar of the box mean, the Sobel magnitude, the box sums and the channel means stands on torch adding as the kernels do"""
    for shape in pb.SHAPES:
        for tag, (flow, valid), k, neg in pb.boxavg_cases(shape):
            assert torch.equal(pb.boxavg_ref(flow, valid, k, neg), pb.boxavg_inorder(flow, valid, k, neg)), (shape, tag)
        for tag, img in pb.sobel_cases(shape):
            assert torch.equal(pb.sobel_ref(img), pb.sobel_inorder(img)), (shape, tag)
        for tag, x, k, pad, Ho, Wo, cmp in pb.box_cases_of(shape):
            assert torch.equal(pb.box_ref(x, k, pad, Ho, Wo, cmp), pb.box_inorder(x, k, pad, Ho, Wo, cmp)), (shape, tag)
    for shape in pb.FLAT_SHAPES:
        for tag, wm in pb.mask_inv_cases(shape):
            assert torch.equal(pb.mask_inv_ref(wm), pb.mask_inv_inorder(wm)), (shape, tag)
        for s in (0, 1):
            tps, inv_clean, fw, o1, m1 = pb.mix_blend_inputs(*shape, pb.flat_seed(shape, 6000) + 8 * s)
            fmask, inv1 = pb.mix_blend_means_inorder(fw, m1)
            assert torch.equal(fmask, ((fw >= 3).float().mean(dim=1, keepdim=True) >= 0.5).float())
            assert torch.equal(inv1, ((1 - m1).float().mean(dim=1, keepdim=True) >= 0.5).float())


def test_minmax_reference_is_the_oracles_filter_in_two_passes():
    from oracle import tps_pipeline as otp
    for shape in pb.SHAPES:
        x = pb.minmax_inputs(*shape, 4, 77)
        for k, is_max in itertools.product(pb.MINMAX_K, (False, True)):
            two = pb.minmax_ref(pb.minmax_ref(x, k, is_max, 0), k, is_max, 1)
            assert torch.equal(two, otp._rect_filter(x[None], k, is_max)[0]), (shape, k, is_max)


def test_minmax_restatement_and_its_unclipped_mutant():
    """the filter tap by tap is the reference on every case; taps that leave the row but not the plane's memory (a missing clip) change a result
    at every shape of more than one row"""
    caught = set()
    for shape in pb.SHAPES:
        for (planes, k, is_max, axis), x in pb.minmax_cases(shape):
            want = pb.minmax_ref(x, k, bool(is_max), axis)
            assert torch.equal(pb.minmax_sim(x, k, is_max, axis), want), (shape, planes, k, is_max, axis)
            if axis == 0 and k > 1 and not torch.equal(pb.minmax_sim(x, k, is_max, axis, "no_clip"), want):
                caught.add(shape)
    assert caught == {s for s in pb.SHAPES if s[0] > 1}, caught


def test_generators_reach_every_threshold():
    """the references are exact at their thresholds, so the tables must actually stand on them: each count below is a mutant that would pass
    (`>` for `>=`, a rounding cast for the truncating one, a missing NaN rule, a missing clip) if it were zero"""
    hits = dict(mean_half=0, fw3=0, inv_half=0, zero_div=0, over=0, under=0, frac=0, thr=0, by_half=0, c2=0)
    for shape in pb.FLAT_SHAPES:
        for _, wm in pb.mask_inv_cases(shape):
            hits["mean_half"] += int((wm.mean(1) == 0.5).sum())
        for s in (0, 1):
            tps, inv_clean, fw, o1, m1 = pb.mix_blend_inputs(*shape, pb.flat_seed(shape, 6000) + 8 * s)
            raw = pb.mix_blend_ref(tps, inv_clean, fw, o1, m1)[5]
            hits["fw3"] += int((fw == 3.0).sum())
            hits["inv_half"] += int(((1 - m1).mean(1) == 0.5).sum())
            hits["zero_div"] += int(torch.isnan(raw).sum())
            hits["over"] += int((raw > 255).sum())
            hits["under"] += int((raw < 0).sum())
            hits["frac"] += int(((raw > 0) & (raw < 255) & (raw - raw.floor() > 0.5)).sum())
        a, _ = pb.plane_op_inputs(shape[0] * shape[1], 2, pb.flat_seed(shape, 7000) + 4)
        hits["thr"] += int((a == pb.THR).sum())
        m1 = pb.stage_inputs(*shape, pb.flat_seed(shape, 8000))[2]
        hits["by_half"] += int((m1 == 0.5).sum())
        for c2 in (1, 3):
            o1, b1, o2, b2 = pb.blend_pair_inputs(*shape, c2, pb.flat_seed(shape, 8000) + 10 + c2)
            hits["c2"] += int(torch.isnan(pb.blend_pair_ref(o1, b1, o2, b2)[1]).sum())
    assert all(v > 0 for v in hits.values()), hits
    for H, W in ((5, 65), (3, 2)):                        # gather_points: the corners and the outside points are in every set of n > 1
        planes, pts = pb.gather_inputs(H, W, 3, 255, 1)
        got = {tuple(p) for p in pts.tolist()}
        assert {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (-1, 0), (W, 0), (0, -1), (0, H)} <= got
        ref = pb.gather_ref(planes, pts)
        out = (pts[:, 0] < 0) | (pts[:, 0] >= W) | (pts[:, 1] < 0) | (pts[:, 1] >= H)
        assert bool((ref[out] == 0).all()) and bool((ref[~out] >= 1).all()) and int(out.sum()) >= 8


def test_planted_bounds_defects_change_a_result():
    """a bounds test one short in the window kernels: each must change a value on a case of the table (the first that catches it is named)"""
    caught = {}
    for shape in pb.SHAPES:
        for tag, (flow, valid), k, neg in pb.boxavg_cases(shape):
            if "boxavg" not in caught and not torch.equal(pb.boxavg_ref(flow, valid, k, neg), pb.boxavg_inorder(flow, valid, k, neg, "x_short")):
                caught["boxavg"] = (shape, tag)
        for tag, img in pb.sobel_cases(shape):
            if "sobel" not in caught and not torch.equal(pb.sobel_ref(img), pb.sobel_inorder(img, "y_short")):
                caught["sobel"] = (shape, tag)
        for tag, x, k, pad, Ho, Wo, cmp in pb.box_cases_of(shape):
            if ("box", cmp) not in caught and not torch.equal(pb.box_ref(x, k, pad, Ho, Wo, cmp), pb.box_inorder(x, k, pad, Ho, Wo, cmp, "x_short")):
                caught[("box", cmp)] = (shape, tag)
    assert set(caught) == {"boxavg", "sobel", ("box", 0), ("box", 1), ("box", 2)}, caught
    assert caught["boxavg"][0] == (1, 1)                                                  # the smallest case already tells


# ================================================================================================ 2. range_argmax
def test_argmax_windows_are_what_they_are_called():
    for plane, wins in pb.ARGMAX_WINDOWS.items():
        assert all(r[0] >= 2 and r[1] >= 2 for r in wins.values()), plane
        size = {name: pb.window_size(r, *plane) for name, r in wins.items()}
        for name, n in (("one", 1), ("n255", 255), ("n256", 256), ("n257", 257), ("empty_cols", 0), ("empty_rows", 0), ("past_right", 0), ("last_pixel", 1)):
            assert size.get(name, n) == n, (plane, name, size[name])
        assert size["full"] == plane[0] * plane[1] and pb.window(wins["full"], *plane)[::2] == (0, 0)
    assert pb.window_size(pb.ARGMAX_WINDOWS[(40, 130)]["full"], 40, 130) > 20 * 256 and pb.window_size(pb.ARGMAX_WINDOWS[(40, 130)]["several"], 40, 130) > 4 * 256
    assert {257} <= {pb.window_size(r, 3, 260) for r in pb.ARGMAX_WINDOWS[(3, 260)].values()}
    for plane in ((9, 65), (40, 130)):
        for name in ("clip_right", "clip_bottom", "clip_both"):
            x1, y1, x2, y2 = pb.ARGMAX_WINDOWS[plane][name]
            assert (x2 + 2 > plane[1]) == (name != "clip_bottom") and (y2 + 2 > plane[0]) == (name != "clip_right")
    assert set(pb.ARGMAX_LAUNCH) == {1, 70}


def test_argmax_restatement_is_the_oracle_and_its_mutants_are_not():
    """argmax_sim (range_argmax_kernel thread for thread) equals the oracle's statement on every window and planted tie; each mutant of the tie
    rule, of the tree and of the empty-window sentinel fails one of them"""
    fails = {"ge": [], "no_tie_reduce": [], "no_sentinel": []}
    for i, (plane, name, elems) in enumerate(pb.ARGMAX_TIES):
        grad, rng, first = pb.argmax_planted(plane, name, elems, i)
        assert pb.argmax_ref(grad, [rng]) == [first] == [pb.argmax_sim(grad, rng)], (plane, name, elems)
        for d in fails:
            if pb.argmax_sim(grad, rng, d) != first:
                fails[d].append((plane, name, elems))
    for plane, wins in pb.ARGMAX_WINDOWS.items():
        for q in (True, False):
            grad = pb.argmax_plane(*plane, 11 + plane[0], q)
            for name, rng in wins.items():
                want = pb.argmax_ref(grad, [rng])[0]
                assert pb.argmax_sim(grad, rng) == want, (plane, name, q)
                for d in fails:
                    if pb.argmax_sim(grad, rng, d) != want:
                        fails[d].append((plane, name, q))
    assert ((40, 130), "full", (17, 273)) in fails["ge"] and ((40, 130), "full", (5, 256)) in fails["no_tie_reduce"]
    assert any(n[1].startswith("empty") for n in fails["no_sentinel"]) and all(fails.values())
    # the planted pairs of the issue, as elements of their windows: neighbours, one thread, the wave and half-block seams, first and last
    pairs = {t[2] for t in pb.ARGMAX_TIES if t[2]}
    assert {(300, 301), (17, 273), (63, 64), (127, 128), (0, 5199)} <= pairs and sum(t[2] is None for t in pb.ARGMAX_TIES) == 2


# ================================================================================================ 3. TPS solves
def test_lds_switch_is_134():
    assert pb.lds_limit() == pb.LDS_MAX_N == 134
    assert {134, 135} <= set(pb.SOLVE_N) and {134, 135} <= set(pb.OTHER_N)
    assert set(pb.SOLVE_N) == {3, 4, 5, 64, 134, 135, 141, 142, 253, 254, 300} and set(pb.OTHER_N) == {20, 134, 135, 254}
    assert max(pb.SOLVE_N) + 3 > 256 > 253 + 2                                             # 253: the last single trip; 254, 300: the second trip


@pytest.fixture(scope="module")
def solve_cases():
    return {(kind, n): pb.solve_case(kind, n) for kind, ns in ((0, pb.SOLVE_N), (1, pb.SOLVE_N), ("other", pb.OTHER_N)) for n in ns}


def test_solve_references_are_the_oracles(solve_cases):
    from oracle import tps_pipeline as otp
    import _other_tps_ref as OR
    for n in (5, 64, 135):
        c = solve_cases[(0, n)]
        kw, aw = otp.get_tps_transform(c["sites"][None], c["centers"][None], solve_dtype=torch.float64)
        assert torch.equal(torch.cat([kw[0], aw[0]]), c["w64"].float())
    c = solve_cases[("other", 20)]
    kw, aw = OR.fit(c["c_src"].numpy(), c["c_dst"].numpy())
    assert np.array_equal(np.concatenate([kw, aw]), c["w64"].float().numpy())
    c = solve_cases[(1, 64)]                             # mode 1: the U of warp_by_tps_opencv_like at the float32 sites, in fp32 as tps2_u evaluates it
    a = c["sites"].double().numpy()
    d2 = ((a[:, None, :] - a[None, :, :]) ** 2).sum(-1)
    K64 = d2 * np.log(d2 + 1.1920929e-7)
    assert np.abs(c["L32"][:64, :64].double().numpy() - K64).max() <= 4 * 2.0 ** -24 * np.abs(K64).max() and torch.equal(c["L64"], c["L32"].double())
    # ... and why the fp64-evaluated U is recorded, not asserted: the rounding of K alone moves the solution as far as the fp32 solve errs
    for n in (64, 134, 253, 300):
        c = solve_cases[(1, n)]
        assert pb.rel_err(c["w64"], c["w64_fp64_U"]) > c["ctl"] / 8, n


def test_control_rule_holds_for_the_reference_and_the_restated_elimination(solve_cases):
    """the fp32 reference meets its own rule trivially (ratio 1/4 or less); the elimination of csrc/tps_solve.h, restated in numpy on the system
    the kernel builds, meets it with room at every n -- and reports no singular system"""
    for (kind, n), c in solve_cases.items():
        bound = pb.solve_bound(c)
        assert c["ctl"] <= bound / 4 or c["ctl"] < pb.FLOOR
        L, r = (c["L64"], c["rhs64"]) if kind == "other" else (c["L32"].double(), c["rhs32"].double())     # "other" builds its K in fp64
        w, status, _ = pb.gauss_jordan(L.numpy(), r.numpy())
        assert status == 0 and pb.rel_err(w, c["w64"]) <= bound, (kind, n, pb.rel_err(w, c["w64"]), bound)


def test_planted_elimination_defects_exceed_the_bound_at_300(solve_cases):
    for kind in (0, 1):
        c = solve_cases[(kind, 300)]
        L, r = c["L32"].double().numpy(), c["rhs32"].double().numpy()
        for defect in ("rows256", "swap256"):
            w, _, _ = pb.gauss_jordan(L, r, defect)
            e = pb.rel_err(torch.nan_to_num(w, nan=1e30, posinf=1e30, neginf=-1e30), c["w64"])
            assert e > 100 * pb.solve_bound(c), (kind, defect, e)
        # one trip, the defects are not defects yet: n + 3 = 256 rows at n = 253 (whose n + 5 = 258 columns already take the swap's second
        # trip: 253 and 254 are two different seams), n + 5 <= 256 columns at n = 142
        for n, defect, harmless in ((253, "rows256", True), (142, "swap256", True), (253, "swap256", False), (254, "rows256", False)):
            c = solve_cases[(kind, n)]
            w, _, _ = pb.gauss_jordan(c["L32"].double().numpy(), c["rhs32"].double().numpy(), defect)
            e = pb.rel_err(torch.nan_to_num(w, nan=1e30, posinf=1e30, neginf=-1e30), c["w64"])
            assert (e <= pb.solve_bound(c)) == harmless, (kind, n, defect, e)


def test_lds_limit_off_by_one_changes_no_bit(solve_cases):
    """the two storage layouts run the same arithmetic: were the switch at 135 or at 133, every weight would keep its bits.  So 134 | 135 cannot
    be an accuracy check; the GPU cases there look for a fault, a corrupted workspace frame or a wrong status, and meet the bound"""
    for kind in (0, 1):
        for n in (134, 135):
            c = solve_cases[(kind, n)]
            L, r = c["L32"].double().numpy(), c["rhs32"].double().numpy()
            (wl, sl, bl), (ww, sw, bw) = pb.gauss_jordan(L, r, storage="lds"), pb.gauss_jordan(L, r, storage="work")
            assert torch.equal(wl, ww) and sl == sw == 0
            assert bl.size == (n + 3) * (n + 5) and bw.size == (n + 3) * (n + 6)          # what the entry's LDS bytes / ops.tps2_solve's workspace hold


def test_singular_sets_are_singular_for_the_restated_elimination():
    for n, what in ((134, "dup"), (135, "dup"), (135, "line")):
        src, tgt = pb.singular_sets(n, what)
        L0, r0 = pb.system_kornia(src, tgt)
        L1, r1 = pb.system_pixel(src * pb.PIXELS, tgt * pb.PIXELS, torch.float32)
        for L, r in ((L0, r0), (L1, r1)):
            assert pb.gauss_jordan(L.double().numpy(), r.double().numpy())[1] == 1, (n, what)


# ================================================================================================ 6. guards
def test_post_pipeline_guards():
    from stitch_amd._lib import lib
    a, b, c, d, e, f, g, h, i = ptrs(9)
    for hw in ((0, 8), (8, 0), (-4, 8), (8, -64), (-2, -2)):
        assert lib.st_tps_mask_inv(a, b, 3, *hw, None) == EINVAL, hw
        assert lib.st_tps_mix_blend(a, b, c, d, e, f, g, h, i, *hw, None) == EINVAL, hw
        assert lib.st_mix_stage_a(a, b, c, d, e, f, g, h, *hw, 0, None) == EINVAL, hw
        assert lib.st_mix_stage_b(a, b, c, d, e, f, g, *hw, None) == EINVAL, hw
        assert lib.st_mix_mul_mask(a, b, c, *hw, 0, 0, None) == EINVAL and lib.st_mix_mul_mask(a, None, c, *hw, 0, 1, None) == EINVAL, hw
        assert lib.st_blend_pair(a, b, c, d, 1, e, *hw, None) == EINVAL and lib.st_blend_pair(a, b, c, d, 3, e, *hw, None) == EINVAL, hw
        assert lib.st_gather_points(a, b, c, 4, 2, *hw, None) == EINVAL, hw
    assert lib.st_tps_mask_inv(a, b, 0, 8, 8, None) == EINVAL and lib.st_tps_mask_inv(a, b, -3, 8, 8, None) == EINVAL
    assert lib.st_gather_points(a, b, c, 0, 2, 8, 8, None) == EINVAL and lib.st_gather_points(a, b, c, 4, 0, 8, 8, None) == EINVAL
    for n, P in ((1 << 30, 2), (1 << 16, 1 << 15), (0x7fffffff, 1), (0x7fffffff, 0x7fffffff)):       # n P does not fit the kernel's int index
        assert lib.st_gather_points(a, b, c, n, P, 8, 8, None) == EINVAL, (n, P)
    for B, Cc in ((65536, 1), (1, 65536), (256, 256), (1 << 16, 1 << 16), (0x7fffffff, 2)):           # B C is the grid's z extent
        assert lib.st_flow_boxavg(a, None, b, B, Cc, 8, 8, 3, 1, None) == EINVAL, (B, Cc)
    for planes in (65536, 1 << 20, 0x7fffffff):
        assert lib.st_minmax_filter(a, b, planes, 8, 8, 3, 1, 0, None) == EINVAL, planes


def test_tps2_warp_guards():
    from stitch_amd._lib import lib
    a, b, c, d, e = ptrs(5)

    def call(C_=3, H=8, W=8, n=10, mode=0):
        return lib.st_tps2_warp(a, b, c, d, e, C_, H, W, n, 1.0, 1.0, 0, mode, None)
    for kw in (dict(n=3801), dict(n=0), dict(H=1), dict(H=0), dict(W=1), dict(C_=0), dict(mode=2), dict(mode=4), dict(mode=-1), dict(mode=7)):
        assert call(**kw) == EINVAL, kw


# ================================================================================================ 5. Telea at deep rings
def test_telea_cases_reach_the_depths_they_claim():
    import _telea_ref as R
    dx, dy = R.disc(88)
    assert int((np.abs(dx) + np.abs(dy)).max()) == 124                    # + 1 for the neighbours of q, + 1 for p's own: 126 <= 127
    depth = {}
    for name, (H, W, radius, _, full) in pb.TELEA_CASES.items():
        d = R.ring_distance(pb.telea_fill(name))
        depth[name] = int(d.max())
        if name == "window_r88":
            yy, xx = np.mgrid[0:H, 0:W]
            assert np.array_equal(d, np.maximum(xx - 3, 0) + np.maximum(yy - 3, 0))
            assert set(full) == set(range(120, 137)) | set(range(248, 265))
    assert depth == dict(window_r88=312, wrap_r64=396, strip=1301, strip_t=1301)
    for name in ("strip", "strip_t"):
        H, W = pb.TELEA_CASES[name][:2]
        assert H + W + 1 > 1024 and (H + W + 1 + 1023) // 1024 == 2


def test_tag_window_and_its_mutant():
    """before() on the tag d mod 256 is d(q) < k for every pixel a ring-k target of window_r88 inspects (the disc and its neighbours), on every
    ring; comparing the tag unwrapped is not, from the first ring whose disc straddles a multiple of 256"""
    import _telea_ref as R
    H, W, radius, _, _ = pb.TELEA_CASES["window_r88"]
    d = R.ring_distance(pb.telea_fill("window_r88"))
    dx, dy = R.disc(radius)
    wrong = set()
    for k in range(1, int(d.max()) + 1):
        ys, xs = np.nonzero(d == k)
        for i in (0, len(ys) // 2, len(ys) - 1):
            qy, qx = ys[i] - dy, xs[i] - dx
            ok = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
            dq = d[qy[ok], qx[ok]]
            assert int(np.abs(dq - k).max()) <= 125
            assert np.array_equal(pb.tag_before(dq, k), dq < k), k
            if not np.array_equal(pb.tag_before(dq, k, "unwrapped"), dq < k):
                wrong.add(k)
    assert min(wrong) == 256 - 124 and {132, 136, 256, 264} <= wrong   # from the first ring whose disc reaches a pixel of d = 256 on


def test_ring_histogram_and_scan_and_their_mutants():
    import _telea_ref as R
    for name in ("strip", "strip_t"):
        H, W = pb.TELEA_CASES[name][:2]
        nb = H + W + 1
        d = R.ring_distance(pb.telea_fill(name))
        want = np.bincount(d.ravel(), minlength=nb)
        assert np.array_equal(pb.ring_hist_sim(d, nb), want)
        assert np.array_equal(pb.ring_hist_sim(d, nb, split=1000), want)                  # the split moved down costs atomics, not counts
        assert not np.array_equal(pb.ring_hist_sim(d, nb, split=1100), want)              # moved up: bins 1024.. fall off the LDS histogram
        off = pb.ring_scan_sim(want, nb)
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(np.concatenate([[0], want[1:]]))]))
        assert not np.array_equal(pb.ring_scan_sim(want, nb, one_bucket=True), off)       # buckets 1024.. never get an offset
    d = R.ring_distance(pb.telea_fill("wrap_r64"))                                         # fewer than 1024 buckets: one per thread, the mutants are none
    nb = 96 + 400 + 1
    want = np.bincount(d.ravel(), minlength=nb)
    assert np.array_equal(pb.ring_hist_sim(d, nb, split=1100), want) and np.array_equal(pb.ring_scan_sim(want, nb, one_bucket=True), pb.ring_scan_sim(want, nb))


# ================================================================================================ 4. tps2_warp
WARP_KEYS = ("img", "centers", "kw", "aw", "kscale", "ascale", "align", "mode")


def _errs(x, ref):
    x, ref = x.double().reshape(-1), ref.reshape(-1)
    if not bool(ref.any()):
        e = 0.0 if not bool(x.any()) else float("inf")
        return e, e
    return ((x - ref).norm() / ref.norm()).item(), ((x - ref).abs().max() / ref.abs().max()).item()


def test_warp_table_covers_its_axes():
    c = pb.WARP_CASES
    assert {k[0] for k in c} == {1, 6, 135, 3800} and {k[1] for k in c} == {(2, 2), (4, 64), (5, 65), (9, 130)} and len(c) == 16
    for n in pb.WARP_N:
        rows = [k for k in c if k[0] == n]
        assert {k[2] for k in rows} == {1, 4} and {k[4] for k in rows} == {0, 1} and {k[5] for k in rows} == {"ramps", "random"}, n
        assert any(k[3][0] != 1 and k[3][1] != 1 for k in rows), n
    assert 4 * 3800 * 4 == 60800 and set(pb.WARP_MODES) == {0, 1, 3}
    img = pb.warp_stairs(4, 9, 130)                                        # the quantised mode's image: fractions to truncate, taps to clamp at both ends
    assert bool((img != img.trunc()).any()) and float(img.max()) > 256 and float(img.min()) < 0


def test_warp_fp32_meets_the_rule_and_the_cap():
    """the kernel's arithmetic restated in torch fp32 (the sum over the centres in index order) meets the control rule of modes 0 and 1 on every
    case; in mode 3 the fp32 control alone leaves out at most CAP of a case, and outside that the fp32 restatement rounds as the fp64 one.
    On the ramps image the output is the sampled position wherever the four taps are inside; aw[0] = inf gives zeros"""
    worst = 0.0
    for case in pb.WARP_CASES:
        for mode in pb.WARP_MODES:
            k = pb.warp_case(case, mode)
            args = {key: k[key] for key in WARP_KEYS}
            ref, pre = pb.warp_eval(**args)
            ctl = pb.warp_control(**args)
            sim, _ = pb.warp_eval(**args, dtype=torch.float32, inorder=True)
            if mode == 3:
                near, E = pb.quant_near(pre, ctl)
                assert near.double().mean().item() <= pb.CAP, (case, near.double().mean().item(), E)
                assert torch.equal(sim.double()[~near], ref[~near]), case
                worst = max(worst, near.double().mean().item())
            elif ref.numel() >= 64:
                (hr, hm), (cr, cm) = _errs(sim, ref), _errs(ctl, ref)
                assert hr <= 2 * max(cr, pb.FLOOR) and hm <= 4 * max(cm, pb.FLOOR), (case, mode, hr, cr, hm, cm)
            bad = dict(args, aw=k["aw"].clone())
            bad["aw"][0] = float("inf")
            assert bool((pb.warp_eval(**bad)[0] == 0).all()), (case, mode)
    assert 0 < worst <= pb.CAP
    k = pb.warp_case(pb.WARP_CASES[7], 1)                                  # n = 6, 9 x 130, ramps
    assert pb.WARP_CASES[7][5] == "ramps"
    H, W = 9, 130
    ix, iy = pb.warp_positions(H, W, k["centers"], k["kw"], k["aw"], k["kscale"], k["ascale"], k["align"], 1, torch.float64)
    inside = (ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1)
    ref = pb.warp_eval(**{key: k[key] for key in WARP_KEYS})[0]
    assert int(inside.sum()) > 500 and float((ref[0, 0].reshape(-1)[inside] - ix[inside]).abs().max()) < 1e-9


def test_warp_planted_defects_break_the_rule():
    """the other alignment, and a centre loop one short at the 3800-point limit: each exceeds the rule on a case of the table"""
    hit = {"align": 0, "last_centre": 0}
    for case in pb.WARP_CASES:
        k = pb.warp_case(case, 0)
        args = {key: k[key] for key in WARP_KEYS}
        ref = pb.warp_eval(**args)[0]
        if ref.numel() < 64:
            continue
        cr, cm = _errs(pb.warp_control(**args), ref)
        flipped = pb.warp_eval(**dict(args, align=1 - k["align"]), dtype=torch.float32, inorder=True)[0]
        hit["align"] += _errs(flipped, ref)[1] > 4 * max(cm, pb.FLOOR)
        if case[0] == 3800:
            short = pb.warp_eval(**dict(args, centers=k["centers"][:-1], kw=k["kw"][:-1]), dtype=torch.float32, inorder=True)[0]
            hit["last_centre"] += _errs(short, ref)[1] > 4 * max(cm, pb.FLOOR)
    assert hit["align"] >= 10 and hit["last_centre"] >= 2, hit
