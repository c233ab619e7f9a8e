"""The blend stage -- csrc/multiband.hip, csrc/exposure.hip, csrc/seam.hip -- through its C entries at buffer edges, at odd alignments,
with non-finite pixels and with the allowed aliases.  Case tables and helpers: tests/_blend_cases.py; tests/test_blend_bounds_cpu.py
shows on the CPU that the tables cover their axes, that the planted pixels lie where they are said to and that the frame helpers report
a planted overrun.  Every comparison is bit equality.

A. Every operand is a view inside a NaN-filled (floats) or sentinel-filled (integers, bytes) buffer: an output frame must be intact after
   the call, and a read outside an input view would put a NaN or the sentinel into a result.  The workspace is exactly
   st_*_workspace_bytes long, 16-byte aligned inside a sentinel frame and holds 0xFF beforehand.  Results equal the restatements.
B. The result of a call does not depend on where its float operands and `side` start; the table names the kernel each pattern lands on.
C. A non-finite or out-of-range pixel or mask value gives (1) the restatement's bits, finite everywhere, and (2) the bits of the same
   call with that value replaced by its rule value -- which does not lean on the restatement.
D. The allowed aliases (out = img1 or img2 of the blend, in place for exposure) give the bits of the call without them."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _blend_cases as bc  # noqa: E402
import _exposure_ref as er  # noqa: E402
import _multiband_ref as mb  # noqa: E402
import _seam_ref as sr  # noqa: E402
from test_geom_matrix_gpu import _release_frames, frame, ops, st  # noqa: E402,F401  (the fixtures and the frame of the matrix tests)


# ================================================================================================ plumbing
def placed(a, off=0):
    """(buffer, view) of an input: `frame`, or `frame_at` where the start matters"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    return frame(tuple(t.shape), t.dtype, t) if off == 0 else bc.frame_at(tuple(t.shape), t.dtype, t, off)


def inp(a, off=0):
    return placed(a, off)[1]


def outp(shape, dtype=torch.float32, off=0):
    return frame(tuple(shape), dtype) if off == 0 else bc.frame_at(tuple(shape), dtype, None, off)


def P(t):
    return None if t is None else t.data_ptr()


def finish(**frames):
    """synchronise, then every (buffer, view) frame must be intact"""
    torch.cuda.synchronize()
    for name, (buf, view) in frames.items():
        assert bc.intact(buf, view), f"a write outside {name}"


def host(t):
    return None if t is None else t.cpu().numpy()


def run_edt(st, mask, border, with_index, off=0):
    H, W = mask.shape
    m = inp(mask.astype(np.uint8), off)
    fD, fI = outp((H, W), torch.int32), outp((H, W), torch.int32) if with_index else None
    st.check(st.lib.st_edt_sq_u8(P(m), H, W, int(border), P(fD[1]), P(fI[1]) if fI else None, st.stream()), "st_edt_sq_u8")
    finish(D=fD, **({"index": fI} if fI else {}))
    return host(fD[1]), host(fI[1]) if fI else None


def run_blend(st, img1, img2, k1, k2, levels, seam=None, offs=(0, 0, 0, 0, 0), side_off=0, alias=0):
    """st_multiband_blend, or st_multiband_blend_seam with seam = (side, info); offs: the start of img1, img2, mask1, mask2, out in floats
    past a 16-byte boundary; alias 1 / 2: out is img1 / img2"""
    H, W = img1.shape[1:]
    fa, fb = placed(img1, offs[0]), placed(img2, offs[1])
    m1, m2 = inp(k1[0], offs[2]), inp(k2[0], offs[3])
    fo = fa if alias == 1 else fb if alias == 2 else outp((3, H, W), off=offs[4])
    need = st.lib.st_multiband_workspace_bytes(H, W, levels)
    fw = bc.workspace_frame(need)
    if seam is None:
        st.check(st.lib.st_multiband_blend(P(fa[1]), P(fb[1]), P(m1), P(m2), H, W, levels, P(fo[1]), P(fw[1]), need, st.stream()), "st_multiband_blend")
    else:
        side, info = inp(seam[0], side_off), inp(seam[1])
        st.check(st.lib.st_multiband_blend_seam(P(fa[1]), P(fb[1]), P(m1), P(m2), H, W, levels, P(side), P(info), P(fo[1]), P(fw[1]), need, st.stream()),
                 "st_multiband_blend_seam")
    finish(out=fo, workspace=fw)
    return host(fo[1])


def grid(H, W, block):
    return -(-H // block), -(-W // block)


def run_stats(st, img1, img2, k1, k2, block):
    H, W = img1.shape[1:]
    fr = outp(grid(H, W, block) + (9,), torch.int32)
    st.check(st.lib.st_exposure_stats(P(inp(img1)), P(inp(img2)), P(inp(k1[0])), P(inp(k2[0])), H, W, block, P(fr[1]), st.stream()), "st_exposure_stats")
    finish(records=fr)
    return host(fr[1])


def _image_pairs(img1, img2, offs, in_place):
    H, W = img1.shape[1:]
    fa, fb = placed(img1, offs[0]), placed(img2, offs[1])
    f1, f2 = (fa, fb) if in_place else (outp((3, H, W), off=offs[2]), outp((3, H, W), off=offs[3]))
    return fa, fb, f1, f2


def run_apply(st, img1, img2, tables, block, channels, offs=(0, 0, 0, 0), in_place=False):
    H, W = img1.shape[1:]
    fa, fb, f1, f2 = _image_pairs(img1, img2, offs, in_place)
    st.check(st.lib.st_exposure_apply(P(fa[1]), P(fb[1]), P(inp(tables)), tables.shape[2], tables.shape[3], H, W, block, int(channels), P(f1[1]), P(f2[1]),
                                      st.stream()), "st_exposure_apply")
    finish(out1=f1, out2=f2)
    return host(f1[1]), host(f2[1])


def run_compensate(st, img1, img2, k1, k2, mode, block, channels, smooth, offs=(0, 0, 0, 0), in_place=False):
    """-> out1, out2, gains; min_count is the default of ops.exposure_compensate and of the restatement, block^2 / 8"""
    H, W = img1.shape[1:]
    fa, fb, f1, f2 = _image_pairs(img1, img2, offs, in_place)
    th, tw = grid(H, W, block) if mode == "blocks" else (1, 1)
    fg = outp((3 if channels else 1, 2, th, tw))
    need = st.lib.st_exposure_workspace_bytes(H, W, block)
    fw = bc.workspace_frame(need)
    st.check(st.lib.st_exposure_compensate(P(fa[1]), P(fb[1]), P(inp(k1[0])), P(inp(k2[0])), H, W, bc.EXPOSURE_MODES.index(mode), block, int(channels),
                                           block * block // 8, smooth, 10.0, 0.1, P(f1[1]), P(f2[1]), P(fg[1]), P(fw[1]), need, st.stream()),
             "st_exposure_compensate")
    finish(out1=f1, out2=f2, gains_out=fg, workspace=fw)
    return host(f1[1]), host(f2[1]), host(fg[1])


def run_cost(st, img1, img2, k1, k2):
    H, W = img1.shape[1:]
    fc = outp((H, W), torch.int32)
    st.check(st.lib.st_seam_cost(P(inp(img1)), P(inp(img2)), P(inp(k1[0])), P(inp(k2[0])), H, W, P(fc[1]), st.stream()), "st_seam_cost")
    finish(cost=fc)
    return host(fc[1])


def run_dp(st, img1, img2, k1, k2, orientation="auto", first="auto", side_off=0, with_path=True):
    """-> side, info, path (None without path_out)"""
    H, W = img1.shape[1:]
    fs, fi = outp((H, W), torch.uint8, side_off), outp((4,), torch.int32)
    fp = outp((max(H, W),), torch.int32) if with_path else None
    need = st.lib.st_seam_workspace_bytes(H, W)
    fw = bc.workspace_frame(need)
    st.check(st.lib.st_seam_dp(P(inp(img1)), P(inp(img2)), P(inp(k1[0])), P(inp(k2[0])), H, W, sr.ORIENTATIONS[orientation], 0 if first == "auto" else first,
                               P(fs[1]), P(fp[1]) if fp else None, P(fi[1]), P(fw[1]), need, st.stream()), "st_seam_dp")
    finish(side_out=fs, info_out=fi, workspace=fw, **({"path_out": fp} if fp else {}))
    return host(fs[1]), host(fi[1]), host(fp[1]) if fp else None


def same(got, want, what):
    assert bc.same_bits(got, want), f"{what}: {int((np.asarray(got) != np.asarray(want)).sum())} of {np.asarray(want).size} values differ"


def seed_of(*key):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % 100000


# ================================================================================================ A: framed operands
@pytest.mark.parametrize("shape", bc.EDT_SHAPES, ids=str)
def test_edt_framed(st, shape):
    H, W = shape
    rng = np.random.default_rng(seed_of(H, W))
    masks = [bc.scene(H, W, kind, 0)[2][0] > 0.5 for kind in bc.MASK_KINDS] + [rng.random((H, W)) < 0.5, rng.random((H, W)) < 0.95]
    for i, m in enumerate(masks):
        for border in (False, True):
            wantD, wantI = mb.edt_sq(m, border, True)
            for with_index in (False, True):
                D, I = run_edt(st, m, border, with_index)
                same(D, wantD, f"D, mask {i}, border {border}, index {with_index}")
                if with_index:
                    same(I, wantI, f"index, mask {i}, border {border}")


@pytest.mark.parametrize("shape", bc.BASE_SHAPES, ids=str)
def test_blend_framed(st, shape):
    H, W = shape
    for kind in bc.MASK_KINDS:
        img1, img2, k1, k2 = bc.scene(H, W, kind, seed_of(H, W, len(kind)))
        side, info, _ = sr.seam(img1, img2, k1, k2)
        for levels in bc.LEVELS:
            same(run_blend(st, img1, img2, k1, k2, levels), mb.blend(img1, img2, k1, k2, levels), f"st_multiband_blend {kind} levels {levels}")
            same(run_blend(st, img1, img2, k1, k2, levels, seam=(side, info)), sr.blend(img1, img2, k1, k2, levels, seam=(side, info)),
                 f"st_multiband_blend_seam {kind} levels {levels}")


@pytest.mark.parametrize("shape", bc.BASE_SHAPES, ids=str)
def test_exposure_framed(st, shape):
    H, W = shape
    for kind in bc.MASK_KINDS:
        img1, img2, k1, k2 = bc.scene(H, W, kind, seed_of(H, W, len(kind), 1))
        for block in bc.BLOCKS:
            same(run_stats(st, img1, img2, k1, k2, block), er.stats(img1, img2, k1, k2, block).astype(np.int32), f"st_exposure_stats {kind} block {block}")
            for channels in (False, True):
                for mode in bc.EXPOSURE_MODES:
                    for smooth in (bc.SMOOTH if mode == "blocks" else bc.SMOOTH[:1]):
                        what = f"st_exposure_compensate {kind} block {block} channels {channels} {mode} smooth {smooth}"
                        w1, w2, wt = er.compensate(img1, img2, k1, k2, mode, block, channels, None, smooth)
                        o1, o2, g = run_compensate(st, img1, img2, k1, k2, mode, block, channels, smooth)
                        same(g, wt, what + ": gains_out")
                        same(o1, w1, what + ": out1")
                        same(o2, w2, what + ": out2")
                a1, a2 = run_apply(st, img1, img2, wt, block, channels)                     # on the restated tables of "blocks", smooth 2
                same(a1, w1, f"st_exposure_apply {kind} block {block} channels {channels}: out1")
                same(a2, w2, f"st_exposure_apply {kind} block {block} channels {channels}: out2")


@pytest.mark.parametrize("shape", bc.SEAM_SHAPES, ids=str)
def test_seam_framed(st, shape):
    H, W = shape
    for kind in bc.MASK_KINDS:
        img1, img2, k1, k2 = bc.scene(H, W, kind, seed_of(H, W, len(kind), 2))
        same(run_cost(st, img1, img2, k1, k2), sr.cost(img1, img2, k1, k2), f"st_seam_cost {kind}")
        for orientation, first in bc.SEAM_MODES:
            side, info, path = run_dp(st, img1, img2, k1, k2, orientation, first)
            ws, wi, wp = sr.seam(img1, img2, k1, k2, orientation, first)
            what = f"st_seam_dp {kind} {orientation} / {first}"
            same(info, wi, what + ": info_out")
            same(path, wp, what + ": path_out")
            same(side, ws, what + ": side_out")


def test_chain_in_one_arena(st):
    """exposure in place, the seam of the compensated pair, the blend along it: one stream, one arena that holds every operand and the three
    exact-size workspaces back to back, 16 bytes of sentinel (and the padding to the next 16-byte boundary) between any two of them"""
    c = bc.CHAIN
    (H, W), block, levels, sets = c["shape"], c["block"], c["levels"], 3 if c["channels"] else 1
    n, (th, tw) = H * W, grid(H, W, block)
    img1, img2, k1, k2 = bc.scene(H, W, "quads", 11)
    lib = st.lib
    need = dict(ws_exposure=lib.st_exposure_workspace_bytes(H, W, block), ws_seam=lib.st_seam_workspace_bytes(H, W),
                ws_blend=lib.st_multiband_workspace_bytes(H, W, levels))
    sizes = dict(img1=12 * n, img2=12 * n, mask1=4 * n, mask2=4 * n, side=n, path=4 * max(H, W), info=16, out=12 * n, gains=4 * sets * 2 * th * tw, **need)
    at, start = 16, {}
    for name, size in sizes.items():
        start[name] = at
        at = (at + size + 15) // 16 * 16 + 16
    arena = torch.full((at,), bc.SENTINEL[torch.uint8], dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 16 == 0
    part = {name: arena[start[name]:start[name] + size] for name, size in sizes.items()}
    for name, a in (("img1", img1), ("img2", img2), ("mask1", k1[0]), ("mask2", k2[0])):
        part[name].view(torch.float32).copy_(torch.from_numpy(np.ascontiguousarray(a)).reshape(-1))
    for name in need:
        part[name].fill_(bc.WS_FILL)
    p = {name: v.data_ptr() for name, v in part.items()}
    s = st.stream()
    st.check(lib.st_exposure_compensate(p["img1"], p["img2"], p["mask1"], p["mask2"], H, W, bc.EXPOSURE_MODES.index(c["mode"]), block, int(c["channels"]),
                                        block * block // 8, c["smooth"], 10.0, 0.1, p["img1"], p["img2"], p["gains"], p["ws_exposure"], need["ws_exposure"], s),
             "st_exposure_compensate")
    st.check(lib.st_seam_dp(p["img1"], p["img2"], p["mask1"], p["mask2"], H, W, 0, 0, p["side"], p["path"], p["info"], p["ws_seam"], need["ws_seam"], s), "st_seam_dp")
    st.check(lib.st_multiband_blend_seam(p["img1"], p["img2"], p["mask1"], p["mask2"], H, W, levels, p["side"], p["info"], p["out"], p["ws_blend"],
                                         need["ws_blend"], s), "st_multiband_blend_seam")
    torch.cuda.synchronize()
    gap = torch.ones(at, dtype=torch.bool, device="cuda")
    for name, size in sizes.items():
        gap[start[name]:start[name] + size] = False
    assert bool((arena[gap] == bc.SENTINEL[torch.uint8]).all()), "a write into a gap of the arena"
    w1, w2, wt = er.compensate(img1, img2, k1, k2, c["mode"], block, c["channels"], None, c["smooth"])
    ws, wi, wp = sr.seam(w1, w2, k1, k2)
    got = lambda name, dtype, shape: part[name].view(dtype).view(shape).cpu().numpy()       # noqa: E731
    same(got("img1", torch.float32, (3, H, W)), w1, "img1 compensated in place")
    same(got("img2", torch.float32, (3, H, W)), w2, "img2 compensated in place")
    same(got("gains", torch.float32, (sets, 2, th, tw)), wt, "gains_out")
    same(got("info", torch.int32, (4,)), wi, "info_out")
    same(got("path", torch.int32, (max(H, W),)), wp, "path_out")
    same(got("side", torch.uint8, (H, W)), ws, "side_out")
    same(got("out", torch.float32, (3, H, W)), sr.blend(w1, w2, k1, k2, levels, seam=(ws, wi)), "out")
    for name, a in (("mask1", k1[0]), ("mask2", k2[0])):
        same(got(name, torch.float32, (H, W)), a, name)


# ================================================================================================ B: alignment classes
@pytest.mark.parametrize("W", bc.EC_WIDTHS)
def test_exposure_does_not_depend_on_where_the_images_start(st, W):
    H, block, channels = 9, 8, True
    img1, img2, k1, k2 = bc.scene(H, W, "quads", 21 + W)
    w1, w2, wt = er.compensate(img1, img2, k1, k2, "blocks", block, channels, None, 2)
    for Wc, offs, in_place, vec in bc.ec_align_cases():
        if Wc != W:
            continue
        assert bc.ec_vec(W, offs) == vec
        o1, o2, g = run_compensate(st, img1, img2, k1, k2, "blocks", block, channels, 2, offs, in_place)
        a1, a2 = run_apply(st, img1, img2, wt, block, channels, offs, in_place)
        for got, want, what in ((o1, w1, "compensate out1"), (o2, w2, "compensate out2"), (g, wt, "gains_out"), (a1, w1, "apply out1"), (a2, w2, "apply out2")):
            same(got, want, f"{what}, offsets {offs}, in place {in_place}, VEC {vec}")


@pytest.mark.parametrize("shape", bc.SIDE_SHAPES, ids=str)
def test_seam_does_not_depend_on_where_side_starts(st, shape):
    H, W = shape
    scenes = [(bc.scene(H, W, "nested", 31)[:2] + (np.ones((1, H, W), np.float32), np.ones((1, H, W), np.float32)), "vertical", 1)]
    if H * W > 16:
        scenes.append((bc.scene(H, W, "quads", 32), "auto", "auto"))
    for (img1, img2, k1, k2), orientation, first in scenes:
        ws, wi, wp = sr.seam(img1, img2, k1, k2, orientation, first)
        assert wi[0] == 1 or orientation == "auto"
        for off in bc.SIDE_OFFSETS:
            for with_path in (False, True):
                side, info, path = run_dp(st, img1, img2, k1, k2, orientation, first, off, with_path)
                what = f"side_out at byte {off}, path_out {with_path}, {orientation}"
                same(side, ws, what + ": side_out")
                same(info, wi, what + ": info_out")
                if with_path:
                    same(path, wp, what + ": path_out")


def test_blend_and_edt_do_not_depend_on_where_their_operands_start(st):
    H, W = bc.ALIGN_SHAPE
    img1, img2, k1, k2 = bc.scene(H, W, "quads", 41)
    side, info, _ = sr.seam(img1, img2, k1, k2)
    assert info[0] == 1
    want, want_seam = mb.blend(img1, img2, k1, k2, 5), sr.blend(img1, img2, k1, k2, 5, seam=(side, info))
    assert not bc.same_bits(want, want_seam)                                                # (so a `side` read at the wrong byte shows)
    for off in bc.SIDE_OFFSETS:
        same(run_blend(st, img1, img2, k1, k2, 5, seam=(side, info), side_off=off), want_seam, f"st_multiband_blend_seam, side at byte {off}")
    patterns = [tuple(o if i == k else 0 for i in range(5)) for k in range(5) for o in bc.FLOAT_OFFSETS[1:]] + [(0,) * 5, (1, 2, 3, 1, 2), (3, 3, 3, 3, 3)]
    for offs in patterns:
        same(run_blend(st, img1, img2, k1, k2, 5, offs=offs), want, f"st_multiband_blend, float offsets {offs}")
    m = k1[0] > 0.5
    wantD, wantI = mb.edt_sq(m, True, True)
    for off in bc.SIDE_OFFSETS:
        D, I = run_edt(st, m, True, True, off)
        same(D, wantD, f"st_edt_sq_u8 D, mask at byte {off}")
        same(I, wantI, f"st_edt_sq_u8 index, mask at byte {off}")


# ================================================================================================ C: non-finite and extreme values
BLOCK_C, LEVELS_C = 8, 5


@functools.lru_cache(maxsize=None)
def special(shape):
    return bc.special_scene(shape)


def gpu_outputs(st, img1, img2, k1, k2):
    """every output of every entry of the stage on one set of inputs; the blend along the seam takes the seam this very run found"""
    out = {"records": run_stats(st, img1, img2, k1, k2, BLOCK_C), "cost": run_cost(st, img1, img2, k1, k2)}
    for mode in bc.EXPOSURE_MODES:
        out[mode + "_out1"], out[mode + "_out2"], out[mode + "_gains"] = run_compensate(st, img1, img2, k1, k2, mode, BLOCK_C, True, 2)
    out["apply_out1"], out["apply_out2"] = run_apply(st, img1, img2, out["blocks_gains"], BLOCK_C, True)
    out["side"], out["info"], out["path"] = run_dp(st, img1, img2, k1, k2)
    out["blend"] = run_blend(st, img1, img2, k1, k2, LEVELS_C)
    out["blend_seam"] = run_blend(st, img1, img2, k1, k2, LEVELS_C, seam=(out["side"], out["info"]))
    out["blend_0"] = run_blend(st, img1, img2, k1, k2, 0)
    return out


def ref_outputs(img1, img2, k1, k2):
    out = {"records": er.stats(img1, img2, k1, k2, BLOCK_C).astype(np.int32), "cost": sr.cost(img1, img2, k1, k2)}
    for mode in bc.EXPOSURE_MODES:
        out[mode + "_out1"], out[mode + "_out2"], out[mode + "_gains"] = er.compensate(img1, img2, k1, k2, mode, BLOCK_C, True, None, 2)
    out["apply_out1"], out["apply_out2"] = out["blocks_out1"], out["blocks_out2"]
    out["side"], out["info"], out["path"] = sr.seam(img1, img2, k1, k2)
    out["blend"] = mb.blend(img1, img2, k1, k2, LEVELS_C)
    out["blend_seam"] = sr.blend(img1, img2, k1, k2, LEVELS_C, seam=(out["side"], out["info"]))
    out["blend_0"] = mb.blend(img1, img2, k1, k2, 0)
    return out


def check_special(st, planted, replaced, what):
    got, clean, want = gpu_outputs(st, *planted), gpu_outputs(st, *replaced), ref_outputs(*planted)
    assert set(got) == set(want)
    for name in got:
        assert np.isfinite(got[name].astype(np.float64)).all(), f"{what}: {name} is not finite"
        same(got[name], want[name], f"{what}: {name} against the restatement")
        same(got[name], clean[name], f"{what}: {name} against the call on the rule values")


@pytest.mark.parametrize("value", bc.IMAGE_SPECIALS, ids=repr)
@pytest.mark.parametrize("shape", bc.SPECIAL_SHAPES, ids=str)
def test_special_pixels(st, shape, value):
    img1, img2, k1, k2, pk = special(shape)
    planted = bc.plant_pixels(img1, img2, pk, value) + (k1, k2)
    replaced = bc.plant_pixels(img1, img2, pk, bc.pixel_rule(value)) + (k1, k2)
    check_special(st, planted, replaced, f"pixel {value!r}")


@pytest.mark.parametrize("value", bc.MASK_SPECIALS, ids=repr)
@pytest.mark.parametrize("shape", bc.SPECIAL_SHAPES, ids=str)
def test_special_mask_values(st, shape, value):
    img1, img2, k1, k2, pk = special(shape)
    planted = (img1, img2) + bc.plant_masks(k1, k2, pk, value)
    replaced = (img1, img2) + bc.plant_masks(k1, k2, pk, bc.mask_rule(value))
    check_special(st, planted, replaced, f"mask value {value!r}")


# ================================================================================================ D: the allowed aliases
@pytest.mark.parametrize("levels", (0, 5))
def test_blend_may_write_over_either_image(st, levels):
    H, W = 33, 65
    img1, img2, k1, k2 = bc.scene(H, W, "quads", 51)
    side, info, _ = sr.seam(img1, img2, k1, k2)
    for seam in (None, (side, info)):
        plain = run_blend(st, img1, img2, k1, k2, levels, seam=seam)
        same(plain, (sr.blend if seam else mb.blend)(img1, img2, k1, k2, levels, **({"seam": seam} if seam else {})), "the call without an alias")
        for alias in (1, 2):
            same(run_blend(st, img1, img2, k1, k2, levels, seam=seam, alias=alias), plain, f"out = img{alias}, levels {levels}, seam {seam is not None}")
