"""CPU restatement of the multiband_fusion contract (README.md, multiband_fusion; csrc/multiband.hip): the distance transforms in integer
numpy, the pyramid in numpy float32 operation for operation -- every product and sum below is one array operation, so one fp32 rounding,
in the order the kernels use -- and the same pyramid in float64 (``dtype=np.float64``).

``defects``: a set of names from DEFECTS, each of which plants one deviation from the contract (tests/test_multiband_cpu.py shows that
every one of them fails an assertion).  Production callers pass none."""
import numpy as np

INT32_MAX = 2 ** 31 - 1
G5 = (0.0625, 0.25, 0.375, 0.25, 0.0625)
DEFECTS = ("ring_not_site", "ties_to_image2", "ties_to_highest_index", "no_extension", "reflect_border", "g_03749", "h_before_w",
           "convex_blend", "no_final_clamp")
_RING = 0x1FFF            # row / column field of a site on the ring round the canvas: loses every tie against a canvas pixel
_NO_SITE = np.int64(1) << 40          # column key without a site
_NO_KEY = np.int64(1) << 62           # full key without a site


def edt_sq(mask, border_is_site=True, return_index=False, defects=frozenset()):
    """mask [H,W], nonzero = inside.  D int32 [H,W]: the exact squared Euclidean distance to the nearest site, the sites being the pixels
    with mask == 0 and (``border_is_site``) the one-pixel ring round the canvas; INT32_MAX without any site.  index int32 [H,W]: the lowest
    row-major index among the canvas sites at distance D, -1 when there is none (no site at all, or only the ring is that near).

    Two passes.  Column pass: the nearest site of every pixel within its own column, as the key g << 13 | row (upper site on a tie).  Row pass:
    min over x' of ((x - x')^2 + g(x')^2) << 26 | row << 13 | x'.  A globally nearest site is nearest within its own column, so the smallest
    key names the lowest row-major index among the nearest sites."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    flip = "ties_to_highest_index" in defects
    rows = np.arange(H, dtype=np.int64)[:, None] + np.zeros((1, W), np.int64)
    far = np.int64(1) << 20
    above = np.maximum.accumulate(np.where(~m, rows, -far), axis=0)                 # row of the nearest site at or above, -far: none
    below = np.minimum.accumulate(np.where(~m, rows, far)[::-1], axis=0)[::-1]

    def field(v):
        return (_RING - 1 - v) if flip else v

    def vkey(site_row, g):
        return np.where(np.abs(site_row) >= far, _NO_SITE, g << 13 | field(np.clip(site_row, 0, H - 1)))
    key_v = np.minimum(vkey(above, rows - above), vkey(below, below - rows))
    if border_is_site:
        key_v = np.minimum(key_v, np.minimum(rows + 1, H - rows) << 13 | _RING)
    g = np.where(key_v >= _NO_SITE, 0, key_v >> 13)
    srow = key_v & _RING
    cols = np.arange(W, dtype=np.int64)[None, :] + np.zeros((H, 1), np.int64)
    base = np.where(key_v >= _NO_SITE, _NO_KEY, (g * g) << 26 | srow << 13 | np.where(srow == _RING, _RING, field(cols)))
    best = base.copy()
    if border_is_site:
        e = np.minimum(cols + 1, W - cols)
        best = np.minimum(best, (e * e) << 26 | _RING << 13 | _RING)
    for k in range(1, W):
        if k * k > (best >> 26).max():
            break
        add = np.int64(k * k) << 26
        best[:, k:] = np.minimum(best[:, k:], base[:, :-k] + add)                   # the site column x - k
        best[:, :-k] = np.minimum(best[:, :-k], base[:, k:] + add)                  # x + k
    none = best >= _NO_KEY
    D = np.where(none, INT32_MAX, best >> 26).astype(np.int32)
    if not return_index:
        return D
    r, c = (best >> 13) & _RING, best & _RING
    ring = none | (r == _RING)
    if flip:
        r, c = _RING - 1 - r, _RING - 1 - c
    return D, np.where(ring, -1, r * W + c).astype(np.int32)


def to_u8(img, dtype=np.float32):
    """the saver's rule (`to_pillow_fn`, `st_u8_trunc`): clamp to 0..255, truncate toward zero; NaN -> 0, -Inf -> 0, +Inf -> 255, never -0"""
    x = np.asarray(img, dtype=np.float64)
    x = np.where(np.isnan(x), 0, x)
    return (np.clip(np.trunc(x), 0, 255) + 0.0).astype(dtype)


def fields(img1, img2, mask1, mask2, dtype=np.float32, defects=frozenset(), truncate=True):
    """steps 1-3 of the contract: img [3,H,W], mask [C,H,W] (channel 0 > 0.5) -> I1f [3,H,W], I2f [3,H,W], W [H,W] (0 / 1), U bool [H,W]"""
    m1, m2 = np.asarray(mask1)[0] > 0.5, np.asarray(mask2)[0] > 0.5
    U = m1 | m2
    a = to_u8(img1, dtype) if truncate else np.asarray(img1, dtype)
    b = to_u8(img2, dtype) if truncate else np.asarray(img2, dtype)
    ring = "ring_not_site" not in defects
    D1, D2 = edt_sq(m1, ring).astype(np.int64), edt_sq(m2, ring).astype(np.int64)
    nearer1 = (D1 > D2) if "ties_to_image2" in defects else (D1 >= D2)
    W1 = m1 & (~m2 | nearer1)
    C = np.where(W1[None], a, b)
    Wf = W1.copy()
    if U.any() and "no_extension" not in defects:
        _, idx = edt_sq(~U, False, True, defects=defects)
        q = np.where(U, np.arange(U.size).reshape(U.shape), idx)
        C = C.reshape(3, -1)[:, q]
        Wf = W1.reshape(-1)[q]
    else:
        C = np.where(U[None], C, 0)
        Wf = Wf & U
    return np.where(m1[None], a, C).astype(dtype), np.where(m2[None], b, C).astype(dtype), Wf.astype(dtype), U


def _taps(n, i, defects):
    if "reflect_border" in defects and n > 1:
        i = np.abs(i)
        i = np.where(i > n - 1, 2 * (n - 1) - i, i)
    return np.clip(i, 0, n - 1)


def reduce1(a, axis, defects=frozenset()):
    """REDUCE along one axis: out[i] = sum_k g[k] in[clamp(2 i + k - 2)], added left to right from the k = 0 product"""
    dt = a.dtype.type
    g = [dt(v) for v in G5]
    if "g_03749" in defects:
        g[2] = dt(0.3749)
    a = np.moveaxis(a, axis, -1)
    n = a.shape[-1]
    i = 2 * np.arange((n + 1) // 2)
    acc = g[0] * a[..., _taps(n, i - 2, defects)]
    for k in range(1, 5):
        acc = acc + g[k] * a[..., _taps(n, i + k - 2, defects)]
    return np.moveaxis(acc, -1, axis)


def reduce2(a, defects=frozenset()):
    """along W, the result rounded to the working precision, then along H"""
    if "h_before_w" in defects:
        return reduce1(reduce1(a, -2, defects), -1, defects)
    return reduce1(reduce1(a, -1, defects), -2, defects)


def expand1(a, n, axis, defects=frozenset()):
    """EXPAND along one axis to n samples: even j: (in[c-1] 0.125 + in[c] 0.75) + in[c+1] 0.125; odd j: in[c] 0.5 + in[c+1] 0.5; c = j >> 1"""
    dt = a.dtype.type
    a = np.moveaxis(a, axis, -1)
    m = a.shape[-1]
    j = np.arange(n)
    c = j >> 1
    lo, mid, hi = a[..., _taps(m, c - 1, defects)], a[..., c], a[..., _taps(m, c + 1, defects)]
    even = (lo * dt(0.125) + mid * dt(0.75)) + hi * dt(0.125)
    odd = mid * dt(0.5) + hi * dt(0.5)
    return np.moveaxis(np.where(j & 1, odd, even), -1, axis)


def expand2(a, h, w, defects=frozenset()):
    if "h_before_w" in defects:
        return expand1(expand1(a, h, -2, defects), w, -1, defects)
    return expand1(expand1(a, w, -1, defects), h, -2, defects)


def effective_levels(H, W, levels):
    n = 0
    while n < levels and (H > 1 or W > 1):
        H, W, n = (H + 1) // 2, (W + 1) // 2, n + 1
    return n


def pyramid_blend(I1f, I2f, Wf, levels, defects=frozenset()):
    """steps 4-6: the three Gaussian pyramids, the blend at the top, Laplacians blended on the way down -> R_0 [3,H,W]"""
    H, W = Wf.shape
    Ga, Gb, Gw = [I1f], [I2f], [Wf]
    for _ in range(effective_levels(H, W, levels)):
        Ga.append(reduce2(Ga[-1], defects))
        Gb.append(reduce2(Gb[-1], defects))
        Gw.append(reduce2(Gw[-1], defects))
    convex = "convex_blend" in defects
    one = Wf.dtype.type(1)

    def mix(a, b, g):
        return g * a + (one - g) * b if convex else b + g * (a - b)
    R = mix(Ga[-1], Gb[-1], Gw[-1][None])
    for l in range(len(Ga) - 2, -1, -1):
        h, w = Gw[l].shape
        La = Ga[l] - expand2(Ga[l + 1], h, w, defects)
        Lb = Gb[l] - expand2(Gb[l + 1], h, w, defects)
        R = expand2(R, h, w, defects) + mix(La, Lb, Gw[l][None])
    return R


def blend(img1, img2, mask1, mask2, levels=5, dtype=np.float32, defects=frozenset(), truncate=True):
    """the whole contract: img [3,H,W], mask [1 or 3,H,W] -> [3,H,W] of `dtype`; ``truncate=False`` keeps fractional pixels (the seam-step
    property is stated on a smooth scene)"""
    if not 0 <= levels <= 16:
        raise ValueError(levels)
    I1f, I2f, Wf, U = fields(img1, img2, mask1, mask2, dtype, defects, truncate)
    R = pyramid_blend(I1f, I2f, Wf, levels, defects)
    if "no_final_clamp" not in defects:
        R = np.clip(R, 0, 255)
    return np.where(U[None], R, 0).astype(dtype)
