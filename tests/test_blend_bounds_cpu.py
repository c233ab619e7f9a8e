"""What tests/test_blend_matrix_gpu.py relies on, shown without a GPU: the three restatements read a special pixel or mask value as the
rule says (against a scalar loop written out here), the planted pixels lie in the regions they are named after, the alignment tables reach
every class they claim, the frame helpers report a planted one-element overrun, and the C entries reject a misaligned workspace and every
forbidden overlap before any launch (pointers by arithmetic inside one buffer this test owns: a library without the guard would still touch
nothing else)."""
import itertools
import math

import numpy as np
import pytest
import torch

import _blend_cases as bc
import _exposure_ref as er
import _multiband_ref as mb
import _seam_ref as sr

EINVAL = bc.EINVAL


# ---- C: the rule, value by value -----------------------------------------------------------------------------------------------------------
def scalar_pixel(v):
    """NaN -> 0, -Inf -> 0, +Inf -> 255, a finite value truncated toward zero and clamped; written out, no numpy"""
    v = float(np.float32(v))
    if math.isnan(v):
        return 0
    if math.isinf(v):
        return 255 if v > 0 else 0
    return min(max(math.trunc(v), 0), 255)


ORDINARY = (0.0, 0.999, 1.0, 1.5, 127.5, 254.999, 255.0, 255.5, -1.0, -30.0, 290.0)


@pytest.mark.parametrize("value", bc.IMAGE_SPECIALS + ORDINARY, ids=repr)
def test_each_restatement_reads_a_pixel_as_the_rule_says(value):
    want = scalar_pixel(value)
    assert bc.pixel_rule(value) == want
    x = np.full((3, 2, 2), value, np.float32)
    for got in (mb.to_u8(x), mb.to_u8(x, np.float64), er.to_u8(x), sr.to_int(x)):
        assert got.shape == x.shape and np.isfinite(got.astype(np.float64)).all()
        for g in got.reshape(-1):
            assert float(g) == want and not np.signbit(np.float64(g)), (value, got.dtype)
    # through the entries of the restatements that the GPU is compared with: one pixel pair, both masks set
    one = np.ones((1, 1, 1), np.float32)
    a, b = np.full((3, 1, 1), value, np.float32), np.full((3, 1, 1), 7.0, np.float32)
    assert sr.cost(a, b, one, one)[0, 0] == 1 + 3 * abs(want - 7)
    assert list(er.stats(a, b, one, one, 8)[0, 0, :4]) == [1, want, want, want]
    assert float(mb.blend(a, a, one, one, 0)[0, 0, 0]) == want


@pytest.mark.parametrize("value", bc.MASK_SPECIALS + (0.0, 1.0, 0.49, 0.51, -1.0), ids=repr)
def test_each_restatement_reads_a_mask_value_as_the_rule_says(value):
    v = float(np.float32(value))
    want = (not math.isnan(v)) and v > 0.5                                  # NaN and -Inf unset, +Inf set, 0.5 unset, the next float set
    assert bc.mask_rule(value) == float(want)
    k, one = np.full((1, 1, 1), value, np.float32), np.ones((1, 1, 1), np.float32)
    a, b = np.full((3, 1, 1), 9.0, np.float32), np.full((3, 1, 1), 5.0, np.float32)
    assert bool(sr.masks(k, one)[0][0, 0]) == want
    assert sr.cost(a, b, k, one)[0, 0] == (1 + 12 if want else sr.BIG)
    assert er.stats(a, b, k, one, 8)[0, 0, 0] == int(want)
    assert float(mb.blend(a, b, k, 1 - one, 0)[0, 0, 0]) == (9.0 if want else 0.0)


def test_the_specials_are_the_listed_ones():
    s = bc.IMAGE_SPECIALS
    assert len(s) == 11 and math.isnan(s[0]) and s[1] == math.inf and s[2] == -math.inf and set(s[3:5]) == {1e30, -1e30}
    assert s[5] == 0 and math.copysign(1, s[5]) < 0 and s[6:] == (255.999, 256.0, -0.5, 2.0 ** 31, -2.0 ** 31)
    m = bc.MASK_SPECIALS
    assert len(m) == 5 and math.isnan(m[0]) and m[1:4] == (math.inf, -math.inf, 0.5) and np.float32(m[4]) == np.float32(0.5) + np.float32(2.0 ** -24)
    assert bc.SPECIAL_SHAPES == ((33, 65), (17, 33))


@pytest.mark.parametrize("shape", bc.SPECIAL_SHAPES, ids=str)
def test_the_planted_positions_lie_in_the_named_regions(shape):
    """from the restatements alone: the overlap, both exclusive regions, outside the union, a pixel that an outside pixel extends from, and a
    pixel of the restated seam path"""
    H, W = shape
    img1, img2, k1, k2, pk = bc.special_scene(shape)
    m1, m2 = (k1[0] > 0.5).reshape(-1), (k2[0] > 0.5).reshape(-1)
    U = (m1 | m2).reshape(H, W)
    _, idx = mb.edt_sq(~U, False, True)
    _, info, path = sr.seam(img1, img2, k1, k2)
    assert info[0] == 1
    flat = [p for name in bc.PLACES for p in pk[name]]
    assert len(flat) == len(set(flat)) == 2 * len(bc.PLACES)
    for p in pk["overlap"] + pk["path"]:
        assert m1[p] and m2[p]
    for p in pk["only1"]:
        assert m1[p] and not m2[p]
    for p in pk["only2"]:
        assert m2[p] and not m1[p]
    for p in pk["outside"]:
        assert not m1[p] and not m2[p]
    for p in pk["nearest"]:
        assert (idx[~U] == p).any() and U.reshape(-1)[p]
    for p in pk["path"]:
        y, x = divmod(p, W)
        assert (path[y] == x) if info[1] == sr.VERTICAL else (path[x] == y)
    # and the planting puts the value there, in both images, and nowhere else
    a, b = bc.plant_pixels(img1, img2, pk, np.inf)
    for got, src in ((a, img1), (b, img2)):
        hit = np.argwhere(got.reshape(3, -1) != src.reshape(3, -1))
        assert sorted(int(p) for _, p in hit) == sorted(pk[name][0] for name in bc.PLACES) and np.isinf(got.reshape(3, -1)[tuple(hit.T)]).all()
    ka, kb = bc.plant_masks(k1, k2, pk, np.nan)
    assert sorted(np.flatnonzero(np.isnan(ka))) == sorted(pk[n][0] for n in bc.PLACES) and sorted(np.flatnonzero(np.isnan(kb))) == sorted(pk[n][1] for n in bc.PLACES)


# ---- A, B: the tables --------------------------------------------------------------------------------------------------------------------
def test_the_shape_tables_are_the_listed_ones():
    base = ((1, 1), (1, 5), (5, 1), (3, 7), (17, 33), (32, 64), (33, 65))
    assert bc.BASE_SHAPES == base and bc.SEAM_SHAPES == base + ((5, 257), (66, 9)) and bc.EDT_SHAPES == base + ((2, 257),)
    assert bc.LEVELS == (0, 1, 5, 16) and bc.BLOCKS == (8, 64) and bc.SMOOTH == (0, 2) and bc.EXPOSURE_MODES == ("gain", "blocks")
    assert bc.SEAM_MODES == (("auto", "auto"), ("vertical", 1), ("horizontal", 2)) and bc.MASK_KINDS == ("quads", "nested", "disjoint", "both_empty")
    assert max(h * w for h, w in bc.SEAM_SHAPES + bc.EDT_SHAPES + bc.SIDE_SHAPES + (bc.ALIGN_SHAPE, bc.CHAIN["shape"])) == 33 * 65


def test_the_exposure_alignment_table_reaches_every_class_and_both_kernels():
    cases = bc.ec_align_cases()
    assert {W for W, *_ in cases} == {32, 33, 36}
    patterns = {(0, 0, 0, 0), (1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 1), (1, 2, 3, 1)}
    for W in bc.EC_WIDTHS:
        assert {offs for Wc, offs, in_place, _ in cases if Wc == W and not in_place} == patterns
        assert {offs for Wc, offs, in_place, _ in cases if Wc == W and in_place} == {(1, 1, 1, 1), (0, 0, 0, 0)}
    for W, offs, in_place, vec in cases:
        assert bc.ec_vec(W, offs) == vec, (W, offs)
        assert not in_place or (offs[0] == offs[2] and offs[1] == offs[3])
    # every (W % 4, pointer class) combination: each operand misaligned alone, all of them, none; both kernels at W % 4 == 0, and an aligned
    # call at W % 4 != 0 that must still take VEC = 1
    classes = {(W % 4, tuple(o % 4 != 0 for o in offs)) for W, offs, in_place, _ in cases if not in_place}
    alone = [tuple(i == k for i in range(4)) for k in range(4)]
    assert classes == set(itertools.product({0, 1}, alone + [(False,) * 4, (True,) * 4]))
    assert {vec for W, _, _, vec in cases if W % 4 == 0} == {1, 4} and {vec for W, _, _, vec in cases if W % 4 != 0} == {1}
    assert any(vec == 1 and W % 4 == 0 for W, offs, _, vec in cases) and any(vec == 1 and W % 4 and not any(offs) for W, offs, _, vec in cases)


def test_the_side_table_reaches_the_word_and_the_byte_path_at_every_remainder():
    ns = [h * w for h, w in bc.SIDE_SHAPES]
    assert ns == [1, 3, 4, 5, 7 * 9, 32 * 64] and bc.SIDE_OFFSETS == bc.FLOAT_OFFSETS == (0, 1, 2, 3)
    stores = {(n, off): bc.side_stores(n, off) for n in ns for off in bc.SIDE_OFFSETS}
    assert all(w + b == n and w % 4 == 0 for (n, off), (w, b) in stores.items())
    assert any(w and n % 4 for (n, off), (w, b) in stores.items())                         # words with n % 4 != 0 (5, 63): the tail goes out as bytes
    assert any(w and b == 0 for (n, off), (w, b) in stores.items())                        # words alone (4, 2048)
    assert any(w == 0 and n >= 4 for (n, off), (w, b) in stores.items())                   # bytes with n >= 4: a misaligned side
    assert all(w == 0 for (n, off), (w, b) in stores.items() if n < 4 or off)
    assert {n % 4 for n in ns} == {0, 1, 3}


# ---- the frame helpers report an overrun -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.float32, torch.int32, torch.uint8), ids=str)
@pytest.mark.parametrize("off", (0, 1, 3))
def test_frame_at_reports_a_planted_overrun(dtype, off):
    buf, view = bc.frame_at((3, 5), dtype, None, off, device="cpu")
    size = buf.element_size()
    assert (view.data_ptr() - off * size) % 16 == 0 and view.is_contiguous() and view.shape == (3, 5)
    start = (view.data_ptr() - buf.data_ptr()) // size
    assert start >= bc.MARGIN and buf.numel() - start - 15 >= bc.MARGIN
    view.fill_(1)
    assert bc.intact(buf, view)
    for at in (start - 1, start + 15, 0, buf.numel() - 1):                                   # in front, behind, the far ends
        keep = buf[at].clone()
        buf[at] = 1
        assert not bc.intact(buf, view), at
        buf[at] = keep
        assert bc.intact(buf, view)


def test_an_exact_size_workspace_reports_a_byte_in_front_behind_and_only_there():
    buf, ws = bc.workspace_frame(48, device="cpu")
    assert ws.numel() == 48 and ws.data_ptr() % 16 == 0 and bool((ws == bc.WS_FILL).all()) and bc.intact(buf, ws)
    start = ws.data_ptr() - buf.data_ptr()
    ws[47] = 0                                                                               # the last byte of the workspace is the call's to write
    ws[0] = 0
    assert bc.intact(buf, ws)
    for at in (start - 1, start + 48):
        buf[at] = bc.WS_FILL                                                                 # (what a kernel one byte off would store is not the sentinel)
        assert not bc.intact(buf, ws)
        buf[at] = bc.SENTINEL[torch.uint8]
    assert bc.intact(buf, ws)
    for off in (4, 8):
        assert bc.workspace_frame(48, off, device="cpu")[1].data_ptr() % 16 == off


def test_same_bits_tells_what_value_equality_does_not():
    a = np.array([0.0, 1.0, np.nan], np.float32)
    assert bc.same_bits(a, a.copy()) and not bc.same_bits(a, np.array([-0.0, 1.0, np.nan], np.float32))
    assert not bc.same_bits(a, a.astype(np.float64)) and not bc.same_bits(a, a[:2]) and not bc.same_bits(np.int32([1]), np.int32([2]))


# ---- B, D: the rejections, before any launch ----------------------------------------------------------------------------------------------
H, W, LEVELS, BLOCK = 12, 20, 3, 8
N = H * W
IMG, MSK = 12 * N, 4 * N


@pytest.fixture(scope="module")
def lib():
    from stitch_amd._lib import lib
    return lib


@pytest.fixture(scope="module")
def own(lib):
    """one buffer this test owns, and the start of every operand inside it: 16-byte aligned, each alone in the middle of a slot three times
    the size of the largest operand -- so a range that overlaps one operand by its first or last bytes stays inside the buffer and
    reaches no other operand, and the guard that answers is the one the test names"""
    sizes = dict(img1=IMG, img2=IMG, k1=MSK, k2=MSK, out=IMG, out2=IMG, side=N, path=4 * max(H, W), info=16, cost=4 * N, index=4 * N, mask8=N,
                 gains=4 * 6 * 2 * 3, ws=max(lib.st_multiband_workspace_bytes(H, W, LEVELS), lib.st_seam_workspace_bytes(H, W), lib.st_exposure_workspace_bytes(H, W, BLOCK)))
    slot = (max(sizes.values()) + 15) // 16 * 16
    buf = torch.zeros(3 * slot * len(sizes) + 16, dtype=torch.uint8)
    first = buf.data_ptr() + (-buf.data_ptr()) % 16
    where = {name: first + (3 * i + 1) * slot for i, name in enumerate(sizes)}
    where["_buffer"] = buf
    return where


def overlaps(size, other, other_size):
    """the starts of a `size`-byte range that overlaps [other, other + other_size) by the range's last four bytes, by its first four, and
    from the same start"""
    return other - size + 4, other + other_size - 4, other


def test_a_workspace_off_a_16_byte_boundary_is_rejected(lib, own):
    o = own
    for off in (4, 8):
        ws = o["ws"] + off
        assert lib.st_multiband_blend(o["img1"], o["img2"], o["k1"], o["k2"], H, W, LEVELS, o["out"], ws, 1 << 30, None) == EINVAL
        assert lib.st_multiband_blend_seam(o["img1"], o["img2"], o["k1"], o["k2"], H, W, LEVELS, o["side"], o["info"], o["out"], ws, 1 << 30, None) == EINVAL
        assert lib.st_seam_dp(o["img1"], o["img2"], o["k1"], o["k2"], H, W, 0, 0, o["side"], o["path"], o["info"], ws, 1 << 30, None) == EINVAL
        assert lib.st_exposure_compensate(o["img1"], o["img2"], o["k1"], o["k2"], H, W, 1, BLOCK, 1, 8, 2, 10.0, 0.1, o["out"], o["out2"], o["gains"], ws, 1 << 30,
                                          None) == EINVAL


def test_blend_rejects_every_forbidden_overlap(lib, own):
    o = own
    need = lib.st_multiband_workspace_bytes(H, W, LEVELS)

    def blend(seam, **kw):
        a = dict(o, **kw)
        if seam:
            return lib.st_multiband_blend_seam(a["img1"], a["img2"], a["k1"], a["k2"], H, W, LEVELS, a["side"], a["info"], a["out"], a["ws"], need, None)
        return lib.st_multiband_blend(a["img1"], a["img2"], a["k1"], a["k2"], H, W, LEVELS, a["out"], a["ws"], need, None)
    for seam in (False, True):
        for name, size in (("img1", IMG), ("img2", IMG)):                                   # a shifted view of an image, by one float and by all but one
            for p in (o[name] + 4, o[name] - 4, o[name] + size - 4, o[name] - size + 4):
                assert blend(seam, out=p) == EINVAL, (seam, name, p - o[name])
        for name, size in (("k1", MSK), ("k2", MSK), ("ws", need)) + ((("side", N), ("info", 16)) if seam else ()):
            for p in overlaps(IMG, o[name], size):
                assert blend(seam, out=p) == EINVAL, (seam, name, p - o[name])
        for name, size in (("img1", IMG), ("img2", IMG), ("k1", MSK), ("k2", MSK)) + ((("side", N), ("info", 16)) if seam else ()):
            for p in (o["ws"] + 16, o["ws"] + need - 16):                                    # an input inside the workspace
                assert blend(seam, **{name: p}) == EINVAL, (seam, name)
            assert blend(seam, ws=o[name] + (size - 16) // 16 * 16) == EINVAL, (seam, name)  # the workspace begins in an input's last bytes


def test_edt_rejects_every_forbidden_overlap(lib, own):
    o = own

    def edt(mask=o["mask8"], D=o["cost"], index=o["index"]):
        return lib.st_edt_sq_u8(mask, H, W, 1, D, index, None)
    for p in overlaps(4 * N, o["mask8"], N):
        assert edt(D=p) == EINVAL and edt(index=p) == EINVAL and edt(D=p, index=None) == EINVAL
    for p in overlaps(4 * N, o["cost"], 4 * N):
        assert edt(index=p) == EINVAL
    assert edt(mask=o["cost"] + 4 * N - 1) == EINVAL and edt(mask=o["index"]) == EINVAL


def test_seam_rejects_every_forbidden_overlap(lib, own):
    o = own
    need = lib.st_seam_workspace_bytes(H, W)
    ins = (("img1", IMG), ("img2", IMG), ("k1", MSK), ("k2", MSK))
    outs = (("side", N), ("path", 4 * max(H, W)), ("info", 16))

    def dp(**kw):
        a = dict(o, **kw)
        return lib.st_seam_dp(a["img1"], a["img2"], a["k1"], a["k2"], H, W, 0, 0, a["side"], a["path"], a["info"], a["ws"], need, None)

    def cost(**kw):
        a = dict(o, **kw)
        return lib.st_seam_cost(a["img1"], a["img2"], a["k1"], a["k2"], H, W, a["cost"], None)
    for out, size in outs:
        for name, other in ins + (("ws", need),) + tuple(x for x in outs if x[0] != out):
            for p in overlaps(size, o[name], other):
                assert dp(**{out: p}) == EINVAL, (out, name, p - o[name])
    for name, size in ins:
        assert dp(**{name: o["ws"] + 16}) == EINVAL and dp(ws=o[name] + (size - 16) // 16 * 16) == EINVAL, name
        for p in overlaps(4 * N, o[name], size):
            assert cost(cost=p) == EINVAL, (name, p - o[name])


def test_exposure_rejects_tables_and_gains_over_an_output(lib, own):
    o = own
    need = lib.st_exposure_workspace_bytes(H, W, BLOCK)
    th, tw = -(-H // BLOCK), -(-W // BLOCK)
    assert (th, tw) == (2, 3)

    def comp(mode=1, channels=1, **kw):
        a = dict(o, **kw)
        return lib.st_exposure_compensate(a["img1"], a["img2"], a["k1"], a["k2"], H, W, mode, BLOCK, channels, 8, 2, 10.0, 0.1, a["out"], a["out2"], a["gains"], a["ws"],
                                          need, None)

    def apply(channels=1, **kw):
        a = dict(o, **kw)
        return lib.st_exposure_apply(a["img1"], a["img2"], a["gains"], th, tw, H, W, BLOCK, channels, a["out"], a["out2"], None)
    for channels in (0, 1):
        full = 4 * (3 if channels else 1) * 2 * th * tw                                      # gains_out and the tables at the byte length the call
        for out in ("out", "out2"):                                                          # writes or reads, [sets][2][Th][Tw]
            for p in overlaps(full, o[out], IMG):
                assert comp(channels=channels, gains=p) == EINVAL, (channels, out, p - o[out])
                assert apply(channels=channels, gains=p) == EINVAL, (channels, out, p - o[out])
        for p in (o["out"] - full // (th * tw) + 4, o["out2"] + IMG - 4):                    # mode 0: [sets][2][1][1]
            assert comp(mode=0, channels=channels, gains=p) == EINVAL
        # gains_out or the workspace over an input or an output is rejected too
        for name, size in (("img1", IMG), ("img2", IMG), ("k1", MSK), ("k2", MSK)):
            for p in overlaps(full, o[name], size):
                assert comp(channels=channels, gains=p) == EINVAL, name
            assert comp(ws=o[name] + (size - 16) // 16 * 16) == EINVAL, name
        for p in overlaps(full, o["ws"], need):
            assert comp(channels=channels, gains=p) == EINVAL
    for out in ("out", "out2"):
        assert comp(ws=o[out] + (IMG - 16) // 16 * 16) == EINVAL and comp(**{out: o["ws"] + need - 16}) == EINVAL
