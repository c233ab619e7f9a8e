"""Case tables and helpers of tests/test_blend_matrix_gpu.py and tests/test_blend_bounds_cpu.py: the blend stage (csrc/multiband.hip,
csrc/exposure.hip, csrc/seam.hip) at buffer edges, at odd alignments, with non-finite pixels and with overlapping operands.

Nothing here touches the GPU unless it is asked for a CUDA tensor: `frame_at`, `workspace_frame` and `intact` work on either device, so the
CPU file can show that a planted overrun is reported.  The framing constants are those of tests/test_geom_matrix_gpu.py (imported, as
`frame` is by the GPU file); the references are tests/_multiband_ref.py, tests/_exposure_ref.py and tests/_seam_ref.py."""
import numpy as np
import torch

import _multiband_cases as mc
import _multiband_ref as mb
import _seam_ref as sr
from test_geom_matrix_gpu import _KEEP, MARGIN, NAN, SENTINEL

EINVAL = 1001
WS_FILL = 0xFF                                                     # what an exact-size workspace holds before a call (not the sentinel)

# ---- part A: the smallest sizes at which a tile, wave or word boundary is crossed --------------------------------------------------------
BASE_SHAPES = ((1, 1), (1, 5), (5, 1), (3, 7), (17, 33), (32, 64), (33, 65))
SEAM_SHAPES = BASE_SHAPES + ((5, 257), (66, 9))
EDT_SHAPES = BASE_SHAPES + ((2, 257),)
LEVELS = (0, 1, 5, 16)
BLOCKS = (8, 64)
EXPOSURE_MODES = ("gain", "blocks")
SMOOTH = (0, 2)
SEAM_MODES = (("auto", "auto"), ("vertical", 1), ("horizontal", 2))
MASK_KINDS = ("quads", "nested", "disjoint", "both_empty")
CHAIN = dict(shape=(33, 65), block=8, mode="blocks", channels=True, smooth=2, levels=5)


def scene(H, W, kind, seed):
    """img1, img2 fp32 [3,H,W] in -30..290, mask1, mask2 fp32 [1,H,W]"""
    a, b = mc.noise_pair(H, W, seed)
    k1, k2 = mc.mask_cases(H, W)[kind]
    return a, b, k1.copy(), k2.copy()


# ---- framing ------------------------------------------------------------------------------------------------------------------------------
def frame_at(shape, dtype=torch.float32, fill=None, off=0, device="cuda"):
    """(buffer, view) as `frame` of test_geom_matrix_gpu.py, on `device` and with a chosen start: the view's first element lies `off`
    elements past a 16-byte boundary, at least MARGIN elements of NaN (floats) or of the sentinel (integers) in front of and behind it"""
    n = int(np.prod(shape))
    size = torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + 2 * MARGIN + 16 // size + off,), NAN if dtype.is_floating_point else SENTINEL[dtype], dtype=dtype, device=device)
    start = MARGIN + (-(buf.data_ptr() + MARGIN * size) % 16) // size + off
    view = buf[start:start + n].view(shape)
    assert (view.data_ptr() - off * size) % 16 == 0
    if fill is not None:
        view.copy_(torch.as_tensor(fill))
    if buf.is_cuda:
        _KEEP.append(buf)
    return buf, view


def workspace_frame(nbytes, off=0, device="cuda"):
    """(buffer, view): exactly `nbytes` bytes of WS_FILL, `off` bytes past a 16-byte boundary, inside a sentinel frame"""
    buf, view = frame_at((nbytes,), torch.uint8, None, off, device)
    view.fill_(WS_FILL)
    return buf, view


def intact(buf, view):
    """every element of the flat `buf` outside `view` (of `frame` or `frame_at`) still holds its filler"""
    start = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    edge = torch.cat([buf[:start], buf[start + view.numel():]])
    return bool(torch.isnan(edge).all()) if buf.dtype.is_floating_point else bool((edge == SENTINEL[buf.dtype]).all())


def same_bits(a, b):
    """equal shape, dtype and bits (so -0.0 is not 0.0, and a NaN equals only the same NaN)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool((a.view(np.uint8) == b.view(np.uint8)).all())


# ---- part B: alignment classes ---------------------------------------------------------------------------------------------------------------
# exposure: the start of img1, img2, out1, out2 in floats past a 16-byte boundary, and the VEC of ec_apply_kernel each pattern must land
# on at W % 4 == 0 (at any other W it is 1)
EC_WIDTHS = (32, 33, 36)
EC_PATTERNS = {(0, 0, 0, 0): 4, (1, 0, 0, 0): 1, (0, 2, 0, 0): 1, (0, 0, 3, 0): 1, (0, 0, 0, 1): 1, (1, 2, 3, 1): 1}
EC_IN_PLACE = {(1, 1): 1, (0, 0): 4}                                # out1 is img1, out2 is img2: the start of the two


def ec_vec(W, offsets):
    """the predicate of ec_apply_launch: float4 accesses iff W is a multiple of 4 and all four pointers are 16-byte aligned"""
    return 4 if W % 4 == 0 and all(o % 4 == 0 for o in offsets) else 1


def ec_align_cases():
    """(W, offsets of img1 img2 out1 out2, in place, VEC)"""
    out = []
    for W in EC_WIDTHS:
        out += [(W, p, False, v if W % 4 == 0 else 1) for p, v in EC_PATTERNS.items()]
        out += [(W, (a, b, a, b), True, v if W % 4 == 0 else 1) for (a, b), v in EC_IN_PLACE.items()]
    return out


# seam: side_out at byte offsets 0..3; seam_side_kernel stores words iff side_out is 4-byte aligned, and then only the threads whose four
# pixels all exist: the last n % 4 pixels always go out as bytes
SIDE_OFFSETS = (0, 1, 2, 3)
SIDE_SHAPES = ((1, 1), (3, 1), (2, 2), (1, 5), (7, 9), (32, 64))     # n = 1, 3, 4, 5, 7 * 9, 32 * 64


def side_stores(n, off):
    """(pixels stored as words, pixels stored as bytes) of seam_side_kernel"""
    words = n // 4 * 4 if off % 4 == 0 else 0
    return words, n - words


FLOAT_OFFSETS = (0, 1, 2, 3)
ALIGN_SHAPE = (17, 33)


# ---- part C: non-finite and extreme values ---------------------------------------------------------------------------------------------------
IMAGE_SPECIALS = (float("nan"), float("inf"), -float("inf"), 1e30, -1e30, -0.0, 255.999, 256.0, -0.5, 2.0 ** 31, -2.0 ** 31)
MASK_SPECIALS = (float("nan"), float("inf"), -float("inf"), 0.5, float(np.nextafter(np.float32(0.5), np.float32(1))))
SPECIAL_SHAPES = ((33, 65), (17, 33))
PLACES = ("overlap", "only1", "only2", "outside", "nearest", "path")


def pixel_rule(v):
    """the value a pixel is read as, scalar by scalar: NaN, -Inf and everything below 1 -> 0, +Inf and everything from 255 -> 255, else
    truncated toward zero"""
    v = float(np.float32(v))
    if v != v or v < 1.0:
        return 0.0
    if v >= 255.0:
        return 255.0
    return float(int(v))


def mask_rule(v):
    """1 where a mask value is set (> 0.5; a NaN compares false), else 0"""
    return 1.0 if float(np.float32(v)) > 0.5 else 0.0


def places(img1, img2, k1, k2):
    """{place: flat pixel indices, ascending}, from the restatements alone: the overlap, the two exclusive regions, outside the union, the
    pixels of the union that some outside pixel extends from (`nearest`), and the pixels of the restated seam path inside the overlap"""
    m1, m2 = sr.masks(k1, k2)
    H, W = m1.shape
    U = m1 | m2
    _, idx = mb.edt_sq(~U, False, True)
    _, info, path = sr.seam(img1, img2, k1, k2)
    L = H if info[1] == sr.VERTICAL else W
    on_path = [(l * W + int(path[l])) if info[1] == sr.VERTICAL else (int(path[l]) * W + l) for l in range(L)]
    flat = lambda b: np.flatnonzero(b.reshape(-1))                                          # noqa: E731
    return {"overlap": flat(m1 & m2), "only1": flat(m1 & ~m2), "only2": flat(m2 & ~m1), "outside": flat(~U),
            "nearest": np.unique(idx[~U]), "path": np.array(sorted(p for p in on_path if (m1 & m2).reshape(-1)[p]), np.int64)}


def picks(where, count=2):
    """{place: `count` pixels of it}, spread over the place, no pixel taken twice"""
    taken, out = set(), {}
    for name in PLACES:
        free = [int(p) for p in where[name] if int(p) not in taken]
        assert len(free) >= count, name
        out[name] = [free[(2 * i + 1) * len(free) // (2 * count)] for i in range(count)]
        taken.update(out[name])
    return out


def plant_pixels(img1, img2, pk, value):
    """copies of the images with `value` at the first pick of every place: channel j % 3 of image 1 and channel (j + 1) % 3 of image 2"""
    a, b = img1.copy(), img2.copy()
    for j, name in enumerate(PLACES):
        p = pk[name][0]
        a.reshape(3, -1)[j % 3, p] = value
        b.reshape(3, -1)[(j + 1) % 3, p] = value
    return a, b


def plant_masks(k1, k2, pk, value):
    """copies of the masks with `value` at the first pick of every place in mask 1 and at the second in mask 2"""
    a, b = k1.copy(), k2.copy()
    for name in PLACES:
        a.reshape(-1)[pk[name][0]] = value
        b.reshape(-1)[pk[name][1]] = value
    return a, b


def bands(H, W):
    """two full-height bands [1,H,W] that overlap in the middle, and a corner outside both: every row crosses the overlap and leaving it costs
    2^18 a pixel, so the seam runs inside the overlap (through `quads` it runs down the free column outside the union)"""
    y, x = np.mgrid[:H, :W]
    corner = (y < H // 4) & (x >= W - W // 5)
    return (x < 0.62 * W)[None].astype(np.float32), ((x > 0.33 * W) & ~corner)[None].astype(np.float32)


def special_scene(shape, seed=7):
    """the scene of part C, noise over `bands`, with its places and picks"""
    img1, img2 = mc.noise_pair(shape[0], shape[1], seed)
    k1, k2 = bands(*shape)
    return img1, img2, k1, k2, picks(places(img1, img2, k1, k2))
