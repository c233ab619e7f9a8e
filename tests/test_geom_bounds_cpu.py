"""The bounds of tests/_geom_bounds.py, shown on the CPU to be neither wrong nor vacuous, the case tables of tests/test_geom_matrix_gpu.py,
and the argument guards of csrc/geom.hip, csrc/flowops.hip and csrc/metrics.hip.

1. A bound that fp32 itself breaks is wrong: torch's CPU fp32 (F.grid_sample, F.interpolate, a 9-term softmax, F.conv2d, a scatter_add
   splat) is held against every E over the whole case table.  err / E <= 1 elementwise.
2. A bound that a real defect meets is vacuous: each planted defect of DEFECTS must give err / E > 1 on at least one case of its table; the
   test names the first (smallest) case that catches it.
3. Every table covers its axes, and every exclusion cap of _geom_bounds.py holds for the reference alone.
4. The entry points reject what their kernels cannot take before any launch: host code only, no pointer is dereferenced."""
import itertools

import pytest
import torch

import _geom_bounds as gb

f32 = torch.float32


def warp_inputs(i, case):
    H, W, B, C, mul = case
    x, flow = gb.image(B, C, H, W, 100 + i), gb.warp_flow(B, H, W, 200 + i)
    m = torch.rand(B, 1, H, W, generator=gb.gen(300 + i)) * 2 - 0.5 if mul else None
    return x, flow, m


def lookup_inputs(i, case):
    H2, W2, r, Nq, _ = case
    return gb.lookup_inputs(Nq, H2, W2, 400 + i)


def resize_inputs(i, case):
    H, W, oh, ow, align, B, C, div, scale = case
    return gb.image(B, C, H, W, 500 + i)


def resize_args(case):
    H, W, oh, ow, align, B, C, div, scale = case
    return dict(oh=oh, ow=ow, align=align, steps=(1.0 / scale, 1.0 / scale) if scale else (1.0, 1.0), div=div)


def convex_inputs(i, case):
    B, H, W, ldm, amp = case
    return gb.convex_inputs(B, H, W, 0.0 if amp == "dominant" else amp, 600 + i, dominant=amp == "dominant")


# ================================================================================================ 1. fp32 meets every E
def test_warp_bound_holds_for_fp32():
    for i, case in enumerate(gb.WARP_CASES):
        x, flow, m = warp_inputs(i, case)
        ref, E = gb.flow_warp_bound(x, flow, m)
        for out in (gb.flow_warp32(x, flow, m), gb.warp_planted(x, flow) * (1 if m is None else m)):
            assert gb.ratio(out, ref, E) <= 1.0, (case, gb.ratio(out, ref, E))
        bad = flow.clone()                                       # the non-finite rule: 0 there, the neighbours as before
        for k, v in enumerate((float("nan"), float("inf"), -float("inf"))):
            bad.view(-1)[(5 * k + 1) % bad.numel()] = v
        rb, Eb = gb.flow_warp_bound(x, bad, m)
        assert gb.ratio(gb.flow_warp32(x, bad, m), rb, Eb) <= 1.0, case
        hit = ~torch.isfinite(bad).all(1, keepdim=True).expand_as(rb)
        assert bool((rb[hit] == 0).all()) and bool((Eb[hit] == 0).all()) and torch.equal(rb[~hit], ref[~hit])


def test_lookup_bound_holds_for_fp32():
    for i, case in enumerate(gb.LOOKUP_CASES):
        H2, W2, r, Nq, _ = case
        maps, coords = lookup_inputs(i, case)
        ref, E = gb.cost_lookup_bound(maps, coords, H2, W2, r)
        for out in (gb.lookup32(maps, coords, H2, W2, r), gb.cost_lookup(maps, coords, H2, W2, r, f32)[0]):
            assert gb.ratio(out, ref, E) <= 1.0, (case, gb.ratio(out, ref, E))


def test_resize_bound_holds_for_fp32():
    for i, case in enumerate(gb.RESIZE_CASES):
        x, a = resize_inputs(i, case), resize_args(case)
        ref, E = gb.resize_bound(x, **a)
        o32 = gb.resize32(x, a["oh"], a["ow"], a["align"], scale=case[8], div=a["div"])
        for out in (o32, gb.resize(x, dtype=f32, **a)[0]):
            assert gb.ratio(out, ref, E) <= 1.0, (case, gb.ratio(out, ref, E))


def test_convex_bound_holds_for_fp32():
    for i, case in enumerate(gb.CONVEX_CASES):
        B, H, W, ldm, amp = case
        coords1, mask = convex_inputs(i, case)
        ref, E = gb.convex_upsample_bound(coords1, mask, B, H, W)
        r = gb.ratio(gb.convex_upsample(coords1, mask, B, H, W, f32), ref, E)
        assert r <= 1.0, (case, r)
        if amp == "dominant":                                    # the reference is the dominant tap's value
            taps = gb.convex_taps(coords1, B, H, W)
            k = mask.view(B, H * W, 9, 64).argmax(2)
            want = torch.gather(taps, 2, k[..., None].expand(-1, -1, -1, 2))        # [B, HW, 64, 2]
            assert (gb.convex_assemble(want, B, H, W) - ref).abs().max().item() < 1e-12


def test_range_map_bound_holds_for_fp32_and_the_exact_patterns():
    from oracle import cgeom
    for i, (H, W, B, pattern) in enumerate(gb.RANGE_CASES):
        flow = gb.range_flow(pattern, B, H, W, 700 + i)
        ref, E = gb.range_map_bound(flow)
        assert gb.ratio(gb.range_map(flow, f32), ref, E) <= 1.0, (H, W, B, pattern)
        assert gb.ratio(torch.from_numpy(cgeom.range_map(flow.numpy())), ref, E) <= 1.0, (H, W, B, pattern)
        if pattern == "zero":
            assert bool((ref == 1).all())
        if pattern == "leave":
            assert bool((ref == 0).all())
        if pattern == "collapse":
            assert bool((ref.flatten(1).amax(1) == H * W).all()) and bool((ref.flatten(1).sum(1) == H * W).all())
        if pattern == "shift":
            assert bool(((ref == 0) | (ref == 1)).all())


def test_flow_encode_bound_holds_for_fp32():
    for i, (Co, H, W, B, _) in enumerate(gb.ENCODE_CASES):
        coords1, w98, bias = gb.flow_encode_inputs(B, H, W, Co, 800 + i)
        ref, E, _ = gb.flow_encode_bound(coords1, w98, bias, B, H, W)
        r = gb.ratio(gb.flow_encode32(coords1, w98, bias, B, H, W), ref, E)
        assert r <= 1.0, (Co, H, W, B, r)


# ================================================================================================ 2. planted defects do not
def first_caught(cases, run):
    """the first case on which run(i, case) -> err / E exceeds 1; None if the defect is never seen"""
    for i, case in enumerate(cases):
        r = run(i, case)
        if r is not None and r > 1.0:
            return case, r
    return None


def warp_defect(**kw):
    def run(i, case):
        x, flow, m = warp_inputs(i, case)
        ref, E = gb.flow_warp_bound(x, flow, m)
        return gb.ratio(gb.warp_planted(x, flow, **kw) * (1 if m is None else m), ref, E)
    return gb.WARP_CASES, run


def warp_item0(i, case):
    x, flow, m = warp_inputs(i, case)
    if x.shape[0] == 1:
        return None
    ref, E = gb.flow_warp_bound(x, flow, m)
    return gb.ratio(gb.warp_planted(x[:1].expand_as(x).contiguous(), flow) * (1 if m is None else m), ref, E)


def warp_last_column(i, case):
    x, flow, m = warp_inputs(i, case)
    if x.shape[-1] < 64:
        return None
    ref, E = gb.flow_warp_bound(x, flow, m)
    out = gb.warp_planted(x, flow) * (1 if m is None else m)
    out[..., 63::64] = float("nan")                             # never written: the NaN the output buffer was filled with
    return gb.ratio(out, ref, E)


def lookup_defect(defect=None, item0=False):
    def run(i, case):
        H2, W2, r, Nq, _ = case
        maps, coords = lookup_inputs(i, case)
        if item0 and Nq == 1:
            return None
        ref, E = gb.cost_lookup_bound(maps, coords, H2, W2, r)
        return gb.ratio(gb.cost_lookup(maps[:1].expand_as(maps) if item0 else maps, coords, H2, W2, r, f32, defect=defect)[0], ref, E)
    return gb.LOOKUP_CASES, run


def resize_defect(defect):
    def run(i, case):
        x, a = resize_inputs(i, case), resize_args(case)
        ref, E = gb.resize_bound(x, **a)
        return gb.ratio(gb.resize(x, dtype=f32, defect=defect, **a)[0], ref, E)
    return gb.RESIZE_CASES, run


def convex_defect(defect):
    def run(i, case):
        B, H, W, ldm, amp = case
        coords1, mask = convex_inputs(i, case)
        ref, E = gb.convex_upsample_bound(coords1, mask, B, H, W)
        return gb.ratio(gb.convex_upsample(coords1, mask, B, H, W, f32, defect=defect), ref, E)
    return gb.CONVEX_CASES, run


def range_drop(i, case):
    H, W, B, pattern = case
    if pattern != "collapse" or H * W < 2:
        return None
    flow = gb.range_flow(pattern, B, H, W, 700 + i)
    ref, E = gb.range_map_bound(flow)
    return gb.ratio(gb.range_map(flow, f32, drop=(B - 1, H * W - 1)), ref, E)


DEFECTS = {
    "lookup_xy_swapped": lookup_defect("swap_xy"),
    "lookup_ne_sw_swapped": lookup_defect("swap_ne_sw"),
    "lookup_taps_clamped": lookup_defect("clamp_taps"),
    "lookup_map_of_query_0": lookup_defect(item0=True),
    "warp_ne_sw_swapped": warp_defect(defect="swap_ne_sw"),
    "warp_taps_clamped": warp_defect(defect="clamp_taps"),
    "warp_wm_hm_swapped": warp_defect(swap_wm=True),
    "warp_batch_stride_of_item_0": (gb.WARP_CASES, warp_item0),
    "warp_last_column_of_a_block_dropped": (gb.WARP_CASES, warp_last_column),
    "resize_other_align_corners": resize_defect("other_align"),
    "resize_mode2_step_from_sizes": resize_defect("step_from_sizes"),
    "resize_div0_div1_swapped": resize_defect("swap_div"),
    "convex_softmax_without_max": convex_defect("no_max"),
    "convex_taps_transposed": convex_defect("transpose_taps"),
    "range_map_one_source_dropped": (gb.RANGE_CASES, range_drop),
}


@pytest.mark.parametrize("name", list(DEFECTS))
def test_planted_defect_exceeds_the_bound(name):
    cases, run = DEFECTS[name]
    hit = first_caught(cases, run)
    assert hit is not None, f"{name}: no case of the table sees it -- the table is missing a case"
    print(f"{name}: caught by {hit[0]} at err / E = {hit[1]:.3g}")


def test_the_no_max_defect_needs_the_large_amplitude():
    """without the max subtraction exp() overflows only at the amplitude-80 cases: those are the ones that catch it"""
    cases, run = convex_defect("no_max")
    caught = {c[4] for i, c in enumerate(cases) if run(i, c) > 1.0}
    assert 80.0 in caught or "dominant" in caught
    assert 1.0 not in caught


# ================================================================================================ 3. tables and caps
def test_the_tables_cover_the_axes():
    assert {(c[0], c[1]) for c in gb.WARP_CASES} == set(itertools.product(gb.TILE_H, gb.TILE_W))
    for ax, vals in ((2, (1, 3)), (3, (1, 3, 6)), (4, (False, True))):
        assert {c[ax] for c in gb.WARP_CASES} == set(vals), ax
    assert {c[0] for c in gb.HOMO_FLOW_CASES} == set(gb.TILE_H) and {c[1] for c in gb.HOMO_FLOW_CASES} == set(gb.TILE_W)
    assert {(c[2], c[3]) for c in gb.HOMO_CASES} == set(itertools.product(gb.TILE_H, gb.TILE_W))
    assert {c[0] for c in gb.HOMO_CASES} == set(gb.TILE_H) and {c[1] for c in gb.HOMO_CASES} == set(gb.TILE_W) and {c[6] for c in gb.HOMO_CASES} == {0, 3}
    rs = gb.RESIZE_CASES
    assert {c[4] for c in rs} == {0, 1, 2}
    for al in (0, 1):
        sub = [c for c in rs if c[4] == al]
        assert {(c[0], c[1]) for c in sub} >= set(itertools.product(gb.TILE_H, gb.TILE_W))
        assert {c[2] for c in sub} == set(gb.TILE_H) and {c[3] for c in sub} >= set(gb.TILE_W)
        kinds = {gb.resize_kind(c) for c in sub}
        assert {"same", "up", "down", "updown"} <= kinds, kinds
        assert any(c[2] == 1 and c[0] > 1 and c[1] > 1 for c in sub) and any(c[3] == 1 and c[0] > 1 and c[1] > 1 for c in sub)
        assert any(c[0] == 1 and c[2] > 1 for c in sub) and any(c[1] == 1 and c[3] > 1 for c in sub)
        assert {c[5] * c[6] for c in sub if c[7] is not None} == {2, 4} and all(c[7][0] != c[7][1] for c in sub if c[7] is not None)
    m2 = [c for c in rs if c[4] == 2]
    assert {c[8] for c in m2} == {0.5, 2.0, 1.5} and any(c[0] * c[8] != int(c[0] * c[8]) for c in m2)
    assert any(c[2] != round(c[0] / (1.0 / c[8])) or c[0] / c[2] != 1.0 / c[8] for c in m2)          # H / oh is not 1 / scale somewhere
    lk = gb.LOOKUP_CASES
    assert {(c[0], c[1]) for c in lk} == {(2, 2), (2, 9), (12, 16), (7, 33)} and {c[2] for c in lk} == {0, 1, 4} and {c[3] for c in lk} == {1, 37, 256}
    assert {(c[3] * (2 * c[2] + 1) ** 2) % 256 == 0 for c in lk} == {True, False} and {c[4] for c in lk} == {0, 3}
    cv = gb.CONVEX_CASES
    assert {(c[1], c[2]) for c in cv} == set(gb.CONVEX_HW) and {c[4] for c in cv} == set(gb.CONVEX_AMPS) and {c[0] for c in cv} == {1, 3} and {c[3] for c in cv} == {576, 580}
    en = gb.ENCODE_CASES
    assert {(c[0], c[1], c[2]) for c in en} == {(co, h, w) for co, (h, w) in itertools.product(gb.ENCODE_CO, gb.ENCODE_HW)}
    assert {c[3] for c in en} == {1, 2} and {c[4] for c in en} == {False, True}
    assert {(c[0], c[1]) for c in gb.RANGE_CASES} == set(gb.RANGE_HW) and {c[3] for c in gb.RANGE_CASES} == set(gb.RANGE_PATTERNS)
    assert [h * w for h, w in gb.PIXEL_HW] == [1, 255, 256, 257, 67 * 131]
    assert all((B * H * W) % 256 for B, H, W, _ in gb.GRID_CASES[:-1]) and {c[3] for c in gb.GRID_CASES} == {2, 4, 8} and any(c[0] == 3 for c in gb.GRID_CASES)


def test_the_warp_flows_reach_every_kind_of_sample():
    """fully inside, two taps out (an edge), three (a corner), four (beyond), exact integers and one ulp either side; one tap out cannot
    happen on a rectangle"""
    seen = set()
    for i, case in enumerate(gb.WARP_CASES):
        H, W = case[:2]
        _, flow, _ = warp_inputs(i, case)
        n = gb.taps_out(flow)
        seen |= set(n.unique().tolist())
        assert 1 not in set(n.unique().tolist()) or min(H, W) == 1
        if H >= 3 and W >= 63:
            assert {0, 2, 3, 4} <= set(n.unique().tolist()), (case, n.unique())
            ix, iy = gb.warp_coords(flow, f32)
            assert bool(((ix == ix.round()) & (ix > 0)).any())
            cx = (gb.pixel_xy(H, W, f32)[0] + flow[:, 0].reshape(flow.shape[0], -1))
            frac = (cx.double() - cx.double().round()).abs()
            assert bool(((frac > 0) & (frac <= 2 * gb.ULP * cx.double().abs())).any())
    assert {0, 2, 3, 4} <= seen


def test_exclusion_caps_hold_for_the_reference_alone():
    for i, (H, W) in enumerate(gb.PIXEL_HW):                    # mean_threshold at 0.5
        for B, C in itertools.product((1, 3), (1, 3, 5)):
            x = gb.mean_inputs((B, C, H, W), 0.5, 900 + i)
            _, near = gb.mean_threshold_bound(x, 0.5)
            assert near.double().mean().item() <= (gb.CAP if H * W > 100 else 0.0), (H, W, B, C)
    for i, (H, W, B, pattern) in enumerate(gb.RANGE_CASES):     # the hard occlusion at 0.5
        ref, E = gb.range_map_bound(gb.range_flow(pattern, B, H, W, 700 + i))
        near = (ref.clamp(0, 1) - 0.5).abs() <= E
        assert near.double().mean().item() <= (gb.CAP if H * W > 100 else 0.0), (H, W, B, pattern)
    for i, (H, W) in enumerate(gb.HOMO_FLOW_CASES):             # overlap: the gathered ones-image against 0.9
        img, H8, flow = gb.homo_flow_inputs(3, H, W, 1000 + i)
        _, ff = gb.homo_flow_final_flow(H8, flow)
        ref, E = gb.flow_warp_bound(torch.ones(3, 1, H, W), ff)
        near = (ref - 0.9).abs() <= E
        assert near.double().mean().item() <= (gb.CAP if H * W > 100 else 0.0), (H, W)


# ================================================================================================ 4. rejected arguments (no launch)
EINVAL = 1001
P0 = 0x7f0000000000                                   # never dereferenced: every call below must return before a launch


def ptrs(n):
    return [P0 + (i << 28) for i in range(n)]


def test_geom_guards():
    from stitch_amd._lib import lib
    a, b, c, d, e, f, g, h = ptrs(8)
    for kw in (dict(B=0), dict(C=0), dict(H=0), dict(W=0), dict(H=-4), dict(W=-64)):
        k = dict(dict(B=2, C=3, H=8, W=8), **kw)
        assert lib.st_flow_warp(a, b, None, c, k["B"], k["C"], k["H"], k["W"], None) == EINVAL, kw
        assert lib.st_grid_sample_blend(a, b, None, c, k["B"], k["C"], k["H"], k["W"], None) == EINVAL, kw
        assert lib.st_mean_threshold(a, b, k["B"], k["C"], k["H"], k["W"], 0.5, None) == EINVAL, kw
        if "C" not in kw:
            assert lib.st_homo_flow_warp(a, b, c, d, e, None, k["B"], k["H"], k["W"], None) == EINVAL, kw
            assert lib.st_range_map(a, b, c, k["B"], k["H"], k["W"], None) == EINVAL, kw
            assert lib.st_morph_open(a, b, c, k["B"], k["H"], k["W"], 3, None) == EINVAL, kw
            assert lib.st_morph_open19(a, b, c, k["B"], k["H"], k["W"], None) == EINVAL, kw
            assert lib.st_eval_finish(a, b, c, k["B"], k["H"], k["W"], None) == EINVAL, kw
        if "B" not in kw and "C" not in kw:
            assert lib.st_blend(a, b, c, d, e, f, g, h, k["H"], k["W"], None) == EINVAL, kw
            assert lib.st_blend_plain(a, b, c, e, f, g, h, k["H"], k["W"], None) == EINVAL, kw
    for ksz in (0, 2, -3):
        assert lib.st_morph_open(a, b, c, 2, 8, 8, ksz, None) == EINVAL, ksz
    assert lib.st_occlusion_from_range(a, b, 0, 0, None) == EINVAL and lib.st_occlusion_from_range(a, b, -5, 1, None) == EINVAL
    for kw in (dict(B=0), dict(C=-1), dict(n1=-1), dict(C=0, n1=0), dict(H=0), dict(W=0), dict(oh=0), dict(ow=0)):
        k = dict(dict(B=2, C=3, n1=0, H=8, W=8, oh=8, ow=8), **kw)
        assert lib.st_homo_warp(a, b, c, None, k["B"], k["C"], k["n1"], k["H"], k["W"], k["oh"], k["ow"], None) == EINVAL, kw
    for kw in (dict(planes=0), dict(H=0), dict(W=0), dict(oh=0), dict(ow=0), dict(al=3), dict(al=-1), dict(nd=1), dict(nd=3), dict(nd=4), dict(nd=2, d0=0.0),
               dict(nd=2, d1=0.0), dict(al=2, d0=0.0), dict(al=2, d1=-1.0), dict(al=2, d0=float("nan")),
               dict(al=2, d0=1.0, d1=0.5, H=2, oh=5),           # mode 2: the last output row would start at source row 4 of 2
               dict(al=2, d0=0.5, d1=1.0, W=2, ow=4)):          # the last output column at source column 3 of 2
        k = dict(dict(planes=4, H=8, W=8, oh=4, ow=4, al=1, d0=0.5, d1=0.5, nd=0), **kw)
        assert lib.st_resize_bilinear(a, b, k["planes"], k["H"], k["W"], k["oh"], k["ow"], k["al"], k["d0"], k["d1"], k["nd"], None) == EINVAL, kw
    assert lib.st_mesh_bounds(a, b, 0, 8.0, 8.0, 3, 3, None) == EINVAL and lib.st_mesh_bounds(a, b, 1, 8.0, 8.0, -1, 3, None) == EINVAL
    for kw in (dict(H=0), dict(W=0), dict(oh=0), dict(ow=-1), dict(C=0), dict(U=None)):      # before the solve is launched
        k = dict(dict(U=a, C=3, H=8, W=8, oh=8, ow=8), **kw)
        assert lib.st_tps_solve_grid(k["U"], b, c, d, e, f, None, 1, k["C"], k["H"], k["W"], 9, k["oh"], k["ow"], None) == EINVAL, kw


def test_flowops_guards():
    from stitch_amd._lib import lib
    a, b, c, d = ptrs(4)
    for B, H, W in ((0, 4, 4), (2, 0, 4), (2, 4, 0), (-1, 4, 4), (2, -4, -4)):
        assert lib.st_coords_grid(a, B, H, W, None) == EINVAL
        assert lib.st_coords_grid_init(a, b, B, H, W, None) == EINVAL
        assert lib.st_flow_from_coords(a, b, 4, c, 2, B, H, W, None) == EINVAL
        assert lib.st_convex_upsample(a, b, 576, c, B, H, W, None) == EINVAL
        assert lib.st_flow_encode(a, b, c, d, 128, None, 0, B, H, W, 128, None) == EINVAL
    assert lib.st_flow_from_coords(a, b, 1, None, 0, 2, 4, 4, None) == EINVAL                # ld4 < 2
    assert lib.st_flow_from_coords(a, None, 0, c, 1, 2, 4, 4, None) == EINVAL                # ld2 < 2
    assert lib.st_convex_upsample(a, b, 575, c, 2, 4, 4, None) == EINVAL                     # ldm < 576
    assert lib.st_convex_upsample(a + 4, b, 576, c, 2, 4, 4, None) == EINVAL                 # coords1 rows are read as float2
    for kw in (dict(Co=0), dict(Co=6), dict(ldo=127), dict(ld2=1), dict(w=b + 4), dict(c1=a + 4)):
        k = dict(dict(Co=128, ldo=128, ld2=2, w=b, c1=a), **kw)
        assert lib.st_flow_encode(k["c1"], k["w"], c, d, k["ldo"], d + 4096, k["ld2"], 2, 4, 4, k["Co"], None) == EINVAL, kw
        if kw != dict(Co=6):
            assert lib.st_flow_encode_split3(k["c1"], k["w"], c, d, k["ldo"], d + 4096, k["ld2"], 2, 4, 4, k["Co"], d + 8192, 1 << 20, 32, None, 0, 0, 0, None) == EINVAL, kw
    assert lib.st_flow_encode_split3(a, b, c, d, 132, None, 0, 2, 4, 4, 132, d + 8192, 1 << 20, 32, None, 0, 0, 0, None) == EINVAL      # Co % 32
    for kw in (dict(Nq=0), dict(H2=1), dict(W2=1), dict(H2=0), dict(W2=-3), dict(r=-1), dict(ldo=80), dict(H2=1 << 16, W2=1 << 16)):
        k = dict(dict(Nq=4, H2=8, W2=8, r=4, ldo=81), **kw)
        assert lib.st_cost_lookup(a, b, c, k["ldo"], k["Nq"], k["H2"], k["W2"], k["r"], None) == EINVAL, kw
        if "r" not in kw:
            assert lib.st_cost_lookup9x9(a, b, c, k["ldo"], k["Nq"], k["H2"], k["W2"], None) == EINVAL, kw


def test_metrics_guards():
    from stitch_amd._lib import lib
    a, b, c, d, e = ptrs(5)
    for B, H, W in ((0, 8, 8), (1, 6, 8), (1, 8, 6), (1, 0, 8), (-2, 8, 8)):
        assert lib.st_masked_psnr_ssim(a, b, 6 * H * W, c, d, e, B, H, W, None) == EINVAL
    assert lib.st_masked_psnr_ssim(a, b, -1, c, d, e, 1, 8, 8, None) == EINVAL and lib.st_masked_psnr_ssim(a, b, 1 << 31, c, d, e, 1, 8, 8, None) == EINVAL
    for B, C, H, W in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, 0)):
        assert lib.st_channel_mean(a, 6 * 64, b, B, C, H, W, None) == EINVAL
    for B, H, W in ((0, 2, 2), (1, 0, 4), (1, 4, 0), (1, 1, 1), (1, 1, 2), (1, 1, 3), (1, 5, 5), (1, 2, 3)):        # h w % 4 != 0 is rejected
        assert lib.st_load_rgb8(a, b, B, H, W, None) == EINVAL
    assert lib.st_load_rgb8(a + 2, b, 1, 2, 2, None) == EINVAL and lib.st_load_rgb8(a, b + 8, 1, 2, 2, None) == EINVAL
