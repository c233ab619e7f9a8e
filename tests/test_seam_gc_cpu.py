"""The seam_gc contract on the CPU (README.md, seam_gc): tests/_seam_gc_ref.py against an enumeration of every labeling on small graphs, the
seed and validity rules on planted cases, the scenes of the issue as orderings, seven planted defects that must each fail an assertion, the C
entries' argument checks and the resource table of csrc/seam_gc.hip (no GPU)."""
import importlib.util
import itertools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _multiband_ref as mb
import _seam_gc_ref as ref
import _seam_ref as dpref
from _multiband_cases import mask_cases, noise_pair, quads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NONE = frozenset()


def scalar_problem(img1, img2, k1, k2):
    """the contract pixel by pixel -> the overlap pixels, S, T (sets of (y, x)) and the arcs {(p, q): capacity}"""
    _, H, W = img1.shape
    a, b = k1[0] > 0.5, k2[0] > 0.5
    trunc = lambda v: int(min(max(float(v), 0.0), 255.0))                  # noqa: E731
    e, S, T = {}, set(), set()
    for y in range(H):
        for x in range(W):
            if a[y, x] and b[y, x]:
                e[y, x] = 1 + sum(abs(trunc(img1[c, y, x]) - trunc(img2[c, y, x])) for c in range(3))
    arcs = {}
    for (y, x) in e:
        near1 = near2 = False
        for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
            qy, qx = y + dy, x + dx
            if not (0 <= qy < H and 0 <= qx < W):
                continue                                                     # the canvas edge seeds nothing
            if (qy, qx) in e:
                arcs[(y, x), (qy, qx)] = e[y, x] + e[qy, qx]
            near1 |= bool(a[qy, qx] and not b[qy, qx])
            near2 |= bool(b[qy, qx] and not a[qy, qx])
        if near1:
            S.add((y, x))
        elif near2:
            T.add((y, x))
    return sorted(e), S, T, arcs


def brute_force(img1, img2, k1, k2):
    """every labeling of the overlap pixels that keeps S on side 1 and T on side 0 -> valid, the minimum cut, and the intersection of the
    side-0 sets of all minimum labelings, as a side plane"""
    _, H, W = img1.shape
    nodes, S, T, arcs = scalar_problem(img1, img2, k1, k2)
    side = np.ones((H, W), np.uint8)
    if not S or not T:
        return 0, 0, side
    free = [p for p in nodes if p not in S and p not in T]
    assert len(free) <= 12
    best, common = None, None
    for bits in itertools.product((1, 0), repeat=len(free)):
        lab = dict(zip(free, bits))
        lab.update({p: 1 for p in S})
        lab.update({p: 0 for p in T})
        cut = sum(c for (p, q), c in arcs.items() if lab[p] == 1 and lab[q] == 0)
        zero = {p for p in nodes if lab[p] == 0}
        if best is None or cut < best:
            best, common = cut, zero
        elif cut == best:
            common &= zero
    for y, x in common:
        side[y, x] = 0
    return 1, best, side


def _assert_equals_brute_force(img1, img2, k1, k2, defects, tag):
    valid, cut, side = brute_force(img1, img2, k1, k2)
    got_side, info = ref.seam(img1, img2, k1, k2, defects=defects)
    assert info.dtype == np.int32 and got_side.dtype == np.uint8
    assert info.tolist() == [valid, 3, 0, cut], (tag, info.tolist(), cut)
    assert np.array_equal(got_side, side), tag
    if valid:
        O, _, _ = ref.regions(k1, k2)
        assert ref.cut_value(ref.cost(img1, img2, k1, k2), O, side) == cut, tag


def _cost_images(rng, H, W, hi):
    """img1 = 0 and img2 with cost - 1 in channel 0: e = 1 + that value.  hi = 1: all costs equal"""
    img2 = np.zeros((3, H, W), f32)
    img2[0] = rng.integers(0, hi, (H, W))
    return np.zeros((3, H, W), f32), img2


def check_cost(defects=NONE):
    """`cost` inside the overlap equals the scalar form on fractional and out-of-range pixels, and what `_seam_ref.cost` (st_seam_cost) gives
    there; it is 0 elsewhere"""
    H, W = 9, 14
    img1, img2 = noise_pair(H, W, 31)
    assert img1.min() < 0 and img1.max() > 255 and (img1 != np.trunc(img1)).any()
    for name, (k1, k2) in mask_cases(H, W).items():
        e = ref.cost(img1, img2, k1, k2, defects)
        O, _, _ = ref.regions(k1, k2)
        nodes, _, _, arcs = scalar_problem(img1, img2, k1, k2)
        assert (e[~O] == 0).all() and np.array_equal(e[O], dpref.cost(img1, img2, k1, k2)[O]), name
        for (p, q), c in arcs.items():
            assert c == e[p] + e[q] and 2 <= c <= 1532, name


def check_grids(defects=NONE):
    """every grid up to 3 x 4 of overlap pixels between a column of E1 and a column of E2 (and transposed), costs from three ranges"""
    rng = np.random.default_rng(61)
    for h in range(1, 4):
        for w in range(1, 5):
            k1, k2 = np.ones((1, h, w + 2), f32), np.ones((1, h, w + 2), f32)
            k2[0, :, 0] = 0
            k1[0, :, -1] = 0
            for hi in (1, 4, 700):
                for rep in range(3):
                    img1, img2 = _cost_images(rng, h, w + 2, hi)
                    _assert_equals_brute_force(img1, img2, k1, k2, defects, (h, w, hi))
                    tr = lambda v: np.ascontiguousarray(v.transpose(0, 2, 1))          # noqa: E731
                    _assert_equals_brute_force(tr(img1), tr(img2), tr(k1), tr(k2), defects, (h, w, hi, "T"))


def check_masks(defects=NONE):
    """seeded small masks with at most 12 overlap pixels: holes, pixels next to both exclusive regions, seedless components"""
    rng = np.random.default_rng(62)
    seen_tie = seen_valid = 0
    for rep in range(160):
        H, W = rng.integers(2, 6), rng.integers(2, 6)
        cls = rng.choice(4, (H, W), p=(0.1, 0.15, 0.15, 0.6))
        if (cls == 3).sum() > 12:
            continue
        k1, k2 = ((cls & 1) > 0)[None].astype(f32), ((cls & 2) > 0)[None].astype(f32)
        img1, img2 = _cost_images(rng, H, W, (1, 4, 700)[rep % 3])
        _, S, T, _ = scalar_problem(img1, img2, k1, k2)
        O, E1, E2 = ref.regions(k1, k2)
        near2 = np.any([ref.shift(E2, dy, dx) for dy, dx in ref.N4], axis=0)
        seen_tie += bool(S and T and any(near2[p] for p in S))
        seen_valid += bool(S and T)
        _assert_equals_brute_force(img1, img2, k1, k2, defects, rep)
    assert seen_tie > 10 and seen_valid > 40


def check_seeds(defects=NONE):
    """S and T on planted masks: the tie goes to S; the canvas edge and a neighbour outside the union seed nothing; diagonal neighbours do not"""
    cls = np.array([[1, 3, 3, 3, 2],
                    [0, 3, 3, 3, 0],
                    [0, 3, 1, 3, 2],
                    [0, 3, 3, 3, 3]])
    O, E1, E2 = ref.regions(((cls & 1) > 0)[None].astype(f32), ((cls & 2) > 0)[None].astype(f32), defects)
    S, T = ref.seeds(O, E1, E2, defects)
    want_S = {(0, 1), (1, 2), (2, 1), (2, 3), (3, 2)}
    want_T = {(0, 3), (3, 4)}                                                 # (2, 3) lies next to both: image 1; (1, 3) has no pixel of the union to its right
    assert {tuple(p) for p in np.argwhere(S)} == want_S
    assert {tuple(p) for p in np.argwhere(T)} == want_T
    full = np.ones((4, 4), bool)
    S, T = ref.seeds(full, ~full, ~full, defects)
    assert not S.any() and not T.any()


def check_ties(defects=NONE):
    """equal images: every cut of the band ties, and the canonical cut sits against image 2's exclusive region"""
    H, W = 6, 12
    k1, k2 = ref.bands(H, W, 0.25, 0.75)
    img = noise_pair(H, W, 63)[0]
    side, info = ref.seam(img, img, k1, k2, defects=defects)
    O, E1, E2 = ref.regions(k1, k2)
    S, T = ref.seeds(O, E1, E2)
    assert info.tolist() == [1, 3, 0, 2 * H] and np.array_equal(side == 0, T)


CHECKS = (check_cost, check_grids, check_masks, check_seeds, check_ties)


def test_cost_is_the_scalar_form_and_seam_cost_inside_the_overlap():
    check_cost()


def test_cut_and_side_equal_the_enumeration_on_small_grids():
    check_grids()


def test_cut_and_side_equal_the_enumeration_on_seeded_small_masks():
    check_masks()


def test_seed_rules():
    check_seeds()


def test_equal_images_put_the_seam_against_image_2():
    check_ties()


@pytest.mark.parametrize("defect", ref.DEFECTS)
def test_a_planted_defect_fails_an_assertion(defect):
    failed = []
    for check in CHECKS:
        try:
            check(frozenset({defect}))
        except AssertionError:
            failed.append(check.__name__)
    assert failed, f"no assertion notices {defect}"


def _scenes():
    out = {f"ghost framed={f}": dpref.ghost_scene(framed=f)[:4] for f in (False, True)}
    out.update({f"serpentine {o}": ref.serpentine_scene(o)[:4] for o in ("vertical", "horizontal")})
    out["L with hole"] = ref.l_hole_scene()
    out["noise quads"] = noise_pair(33, 65, 64) + quads(33, 65)
    return out


def test_dinic_and_edmonds_karp_give_the_same_side():
    for name, scene in _scenes().items():
        a, b = ref.seam(*scene, method="dinic"), ref.seam(*scene, method="edmonds_karp")
        assert np.array_equal(a[0], b[0]) and a[1].tolist() == b[1].tolist() and a[1][0] == 1, name
        O, _, _ = ref.regions(scene[2], scene[3])
        assert ref.cut_value(ref.cost(*scene), O, a[0]) == ref.cut_of(a[1]), name


def test_invalid_arrangements_leave_the_distance_blend():
    H, W = 24, 40
    img1, img2 = noise_pair(H, W, 65)
    cases = mask_cases(H, W)
    for name in ("nested", "identical", "disjoint", "m2_empty", "both_empty"):
        k1, k2 = cases[name]
        for a, b in ((k1, k2), (k2, k1)):
            side, info = ref.seam(img1, img2, a, b)
            assert info.tolist() == [0, 3, 0, 0] and (side == 1).all(), name
            assert np.array_equal(dpref.blend(img1, img2, a, b, 3, (side, info)), mb.blend(img1, img2, a, b, 3)), name
    side, info = ref.seam(img1, img2, *cases["quads"])
    assert info[0] == 1 and (side == 0).any()


def _scene_figures(img1, img2, k1, k2):
    """owner-change discontinuity and seam pixels of the distance seam, seam_dp and seam_gc"""
    _, _, Wd, _ = mb.fields(img1, img2, k1, k2)
    sd = dpref.seam(img1, img2, k1, k2)[:2]
    sg = ref.seam(img1, img2, k1, k2)
    owners = {"distance": Wd, "dp": dpref.fields(img1, img2, k1, k2, sd)[2], "gc": dpref.fields(img1, img2, k1, k2, sg)[2]}
    disc = {n: dpref.owner_change_discontinuity(img1, img2, k1, k2, w > 0.5) for n, w in owners.items()}
    on = {n: dpref.seam_pixels(k1, k2, w) for n, w in owners.items()}
    return sg, owners, disc, on


@pytest.mark.parametrize("framed", [False, True], ids=["quads", "framed"])
def test_cut_avoids_the_ghost_and_shares_the_overlap(framed):
    img1, img2, k1, k2, ghost = dpref.ghost_scene(framed=framed)
    (side, info), owners, disc, on = _scene_figures(img1, img2, k1, k2)
    O, _, _ = ref.regions(k1, k2)
    in_ghost = {n: int((v & ghost).sum()) for n, v in on.items()}
    share = float((owners["gc"][O] > 0.5).mean())
    print(f"ghost scene (framed={framed}): cut {ref.cut_of(info)}, seam pixels inside the ghost {in_ghost}, owner-change discontinuity {disc}, "
          f"image 1's share of the overlap: gc {share:.3f}, dp {float((owners['dp'][O] > 0.5).mean()):.3f}")
    assert info[0] == 1 and in_ghost["gc"] == 0
    assert disc["gc"] <= disc["distance"]
    assert 0 < share < 1
    if framed:
        assert disc["gc"] <= disc["dp"]


@pytest.mark.parametrize("orientation", ["vertical", "horizontal"])
def test_cut_follows_a_corridor_that_doubles_back(orientation):
    img1, img2, k1, k2, corridor = ref.serpentine_scene(orientation)
    (side, info), owners, disc, on = _scene_figures(img1, img2, k1, k2)
    print(f"serpentine ({orientation}): cut {ref.cut_of(info)}, discontinuity {disc}, seam pixels {int(on['gc'].sum())}, off the corridor {int((on['gc'] & ~corridor).sum())}")
    assert info[0] == 1 and disc["gc"] == 0 and on["gc"].any() and not (on["gc"] & ~corridor).any()
    assert disc["dp"] > 0


def test_l_shaped_overlap_with_a_hole_is_shared():
    img1, img2, k1, k2 = ref.l_hole_scene()
    side, info = ref.seam(img1, img2, k1, k2)
    O, E1, E2 = ref.regions(k1, k2)
    m1, m2 = dpref.masks(k1, k2)
    assert (m1 & ~m2)[26:30, 24:31].all()                                     # the hole in mask 2 lies inside image 1
    print(f"L with hole: cut {ref.cut_of(info)}, image 1 owns {int((side[O] == 1).sum())} of {int(O.sum())} overlap pixels")
    assert info[0] == 1 and (side[O] == 1).any() and (side[O] == 0).any()


# ---- entries and binary --------------------------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_touching_the_gpu():
    from stitch_amd._lib import lib
    base = 0x7f0000000000                                                   # never dereferenced on the host
    img1, img2, k1, k2, side, info, ws = (base + (i << 32) for i in range(7))
    H, W = 37, 53
    wsb = lib.st_seam_gc_workspace_bytes
    need = wsb(H, W)
    assert need >= 30 * H * W and need % 16 == 0
    assert wsb(0, 5) == 0 and wsb(5, 0) == 0 and wsb(4097, 5) == 0 and wsb(5, 4097) == 0 and wsb(-1, 5) == 0
    assert 0 < wsb(4096, 4096) < 2 ** 31 and wsb(1, 1) > 0
    big = 1 << 40

    def begin(img1=img1, img2=img2, k1=k1, k2=k2, H=H, W=W, ws=ws, nbytes=need):
        return lib.st_seam_gc_begin(img1, img2, k1, k2, H, W, ws, nbytes, None)
    for name in ("img1", "img2", "k1", "k2", "ws"):
        assert begin(**{name: None}) == 1001, name
    assert begin(H=0) == 1001 and begin(W=0) == 1001 and begin(H=4097, nbytes=big) == 1001 and begin(W=4097, nbytes=big) == 1001 and begin(H=-3) == 1001
    assert begin(nbytes=need - 1) == 1001 and begin(nbytes=0) == 1001 and begin(ws=ws + 8) == 1001 and begin(H=H + 1) == 1001
    for name in ("img1", "img2", "k1", "k2"):                                # an operand inside the workspace
        assert begin(**{name: ws + 64}) == 1001, name
        assert begin(**{name: ws - 16}) == 1001, name

    def rnd(H=H, W=W, ws=ws, nbytes=need):
        return lib.st_seam_gc_round(H, W, ws, nbytes, None)
    assert rnd(ws=None) == 1001 and rnd(H=0) == 1001 and rnd(W=4097, nbytes=big) == 1001 and rnd(nbytes=need - 1) == 1001 and rnd(ws=ws + 4) == 1001

    def relabel(H=H, W=W, ws=ws, nbytes=need):
        return lib.st_seam_gc_relabel(H, W, ws, nbytes, None)
    assert relabel(ws=None) == 1001 and relabel(H=0) == 1001 and relabel(W=4097, nbytes=big) == 1001 and relabel(nbytes=need - 1) == 1001 and relabel(ws=ws + 4) == 1001

    def finish(H=H, W=W, side=side, info=info, ws=ws, nbytes=need):
        return lib.st_seam_gc_finish(H, W, side, info, ws, nbytes, None)
    for name in ("side", "info", "ws"):
        assert finish(**{name: None}) == 1001, name
    assert finish(H=0) == 1001 and finish(W=4097, nbytes=big) == 1001 and finish(nbytes=need - 1) == 1001 and finish(ws=ws + 8) == 1001
    assert finish(side=ws + 32) == 1001 and finish(info=ws + need - 16) == 1001 and finish(info=side + 4) == 1001 and finish(side=info - 8) == 1001


def test_kernels_use_no_scratch_and_the_stated_lds():
    """from the compiler's metadata of csrc/seam_gc.hip, built with the library's own flags (README.md, seam_gc, kernel table)"""
    spec = importlib.util.spec_from_file_location("_stitch_build", os.path.join(ROOT, "seamless-through-breaking-rethinking-image-stitching-for-optimal-alignment_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert build.SOURCES["seam_gc.hip"] == []
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "seam_gc.s")
        subprocess.check_call(build.compile_cmd("seam_gc.hip", out, ["-S", "--cuda-device-only"]), stderr=subprocess.DEVNULL)
        text = open(out).read()
    rep = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+)\n.*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)",
                         text, re.S):
        rep[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    lds = {"gc_class_kernel": 0, "gc_setup_kernel": 64, "gc_begin_kernel": 64, "gc_push_kernel": 0, "gc_gather_kernel": 0, "gc_bfs_kernel": 9840,
           "gc_status_kernel": 64, "gc_side_kernel": 64, "gc_info_kernel": 128}
    assert len(rep) == len(lds), sorted(rep)
    for key, want in lds.items():
        (name, r), = [(n, r) for n, r in rep.items() if key in n]
        assert r["lds"] == want, (name, r)
        assert r["scratch"] == 0 and r["spill"] == 0 and r["vgpr"] <= 64, (name, r)
    # no data-dependent loop, spin or atomic in the device code: the only backward branches are the fixed-count loops
    src = open(os.path.join(ROOT, "seamless-through-breaking-rethinking-image-stitching-for-optimal-alignment_amd", "csrc", "seam_gc.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\batomic\w*\s*\(|\bwhile\s*\(|hipMem(set|cpy)", code)
