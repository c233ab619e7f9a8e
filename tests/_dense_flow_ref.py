"""CPU restatement of csrc/dense_flow.hip (README.md, "dense_flow"): a coarse-to-fine, zero-mean Lucas-Kanade flow on integer pyramids,
vectorised numpy.  Everything is int64 except the 2x2 solve, which is fp64 with one rounding per product, difference and quotient (numpy's
element-wise operations never contract).  The contract is this project's own: it is pinned against no library.  `dense_flow` is what
`ops.dense_flow` must equal bit for bit: flow, support, both pyramids and the final flow of every level.  `defects` plants one of DEFECTS,
for tests/test_dense_flow_cpu.py: each of them must break an assertion there.  One item at a time: batch items are independent."""
import numpy as np

from _features_ref import luma, scene  # noqa: F401  (the pixel and luma rules are feature_align's)

MIN_SIDE, MAX_SIDE, MAX_BATCH, MAX_LEVELS, MAX_ITERS, MAX_RADIUS, MAX_DAMPING = 16, 1024, 64, 8, 16, 7, 1 << 24
SPLIT_SIDE, DEN_MIN = 32, 128
DEFAULTS = dict(levels=5, iters=4, radius=4, damping=65536)
G5 = np.array([1, 4, 6, 4, 1], np.int64)
NONE = frozenset()
DEFECTS = ("no_zero_mean", "fx_fy_swapped", "upscale_without_x2", "du_sign", "replicate_window", "m2_ignored", "no_median", "trunc_for_rint", "den_min_127")


# ---- operands and pyramids ---------------------------------------------------------------------------------------------------------------------
def mask_bits(mask, H, W):
    """fp32 [1 or 3,H,W] or None -> int64 [H,W]: set iff channel 0 > 0.5 (NaN is unset)"""
    if mask is None:
        return np.ones((H, W), np.int64)
    return (np.asarray(mask, np.float32)[0] > np.float32(0.5)).astype(np.int64)


def level0(img, mask):
    """-> (V = 16 Y, m) int64 [H,W]"""
    Y = luma(img)
    return 16 * Y, mask_bits(mask, *Y.shape)


def level_sizes(H, W, levels):
    sizes = [(H, W)]
    while len(sizes) < levels and min(sizes[-1]) >= SPLIT_SIDE:
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    return sizes


def down(V, m, defects=NONE):
    """one level down: the 5x5 binomial of m V at (2i, 2j), clamped coordinates, normalised by the same filter of m"""
    H, W = V.shape
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    num, den = np.zeros((Hc, Wc), np.int64), np.zeros((Hc, Wc), np.int64)
    mv = m * V
    for a in range(5):
        yy = np.clip(2 * np.arange(Hc) + a - 2, 0, H - 1)
        for b in range(5):
            xx = np.clip(2 * np.arange(Wc) + b - 2, 0, W - 1)
            g = G5[a] * G5[b]
            num += g * mv[np.ix_(yy, xx)]
            den += g * m[np.ix_(yy, xx)]
    Vc = np.where(den > 0, (2 * num + den) // np.maximum(2 * den, 1), 0)
    return Vc, (den >= (DEN_MIN - 1 if "den_min_127" in defects else DEN_MIN)).astype(np.int64)


def pyramid(V, m, levels, defects=NONE):
    Vs, ms = [V], [m]
    for _ in level_sizes(*V.shape, levels)[1:]:
        Vc, mc = down(Vs[-1], ms[-1], defects)
        Vs.append(Vc), ms.append(mc)
    return Vs, ms


def upscale(Uc, H, W, defects=NONE):
    """U_l(y, x) = 2 U_{l+1}(y >> 1, x >> 1); Uc int64 [2,Hc,Wc]"""
    up = Uc[:, np.arange(H)[:, None] >> 1, np.arange(W)[None, :] >> 1]
    return up if "upscale_without_x2" in defects else 2 * up


# ---- one iteration -----------------------------------------------------------------------------------------------------------------------------
def gradients(V1, m1):
    """(gx, gy, w1): central differences with clamped neighbours (twice the gradient); w1 = m1 at the pixel and its four clamped neighbours"""
    H, W = V1.shape
    xl, xr = np.maximum(np.arange(W) - 1, 0), np.minimum(np.arange(W) + 1, W - 1)
    yu, yd = np.maximum(np.arange(H) - 1, 0), np.minimum(np.arange(H) + 1, H - 1)
    return V1[:, xr] - V1[:, xl], V1[yd, :] - V1[yu, :], m1 & m1[:, xl] & m1[:, xr] & m1[yu, :] & m1[yd, :]


def sample(V2, m2, Ux, Uy, defects=NONE):
    """(J, w2): image 2 at p + U / 256, bilinear in 8.8 fixed point; w2 iff all four taps lie inside and are valid (J is 0 elsewhere)"""
    H, W = V2.shape
    ys, xs = np.mgrid[0:H, 0:W].astype(np.int64)
    sx, sy = 256 * xs + Ux, 256 * ys + Uy
    x0, fx, y0, fy = sx >> 8, sx & 255, sy >> 8, sy & 255
    inside = (x0 >= 0) & (x0 <= W - 2) & (y0 >= 0) & (y0 <= H - 2)
    xc, yc = np.clip(x0, 0, W - 2), np.clip(y0, 0, H - 2)
    w2 = inside & (m2[yc, xc] & m2[yc, xc + 1] & m2[yc + 1, xc] & m2[yc + 1, xc + 1] > 0)
    if "m2_ignored" in defects:
        w2 = inside
    if "fx_fy_swapped" in defects:
        fx, fy = fy, fx
    J = ((256 - fx) * (256 - fy) * V2[yc, xc] + fx * (256 - fy) * V2[yc, xc + 1] + (256 - fx) * fy * V2[yc + 1, xc] + fx * fy * V2[yc + 1, xc + 1] + (1 << 15)) >> 16
    return np.where(w2, J, 0), w2.astype(np.int64)


def window_sum(a, r, defects=NONE):
    """sum over the (2r + 1)^2 window, terms outside the array 0; int64, so the order does not matter"""
    H, W = a.shape
    p = np.pad(a, r, mode="edge") if "replicate_window" in defects else np.pad(a, r)
    c = np.zeros((H + 2 * r + 1, W + 2 * r + 1), np.int64)
    c[1:, 1:] = p.cumsum(0).cumsum(1)
    k = 2 * r + 1
    return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]


def solve(n, Sx, Sy, St, Sxx, Sxy, Syy, Sxt, Syt, r, damping, defects=NONE):
    """(dUx, dUy int64, supported): the zero-mean normal equations exactly in int64, then fp64 with every operation rounded on its own"""
    if "no_zero_mean" in defects:
        Sx = Sy = St = np.zeros_like(n)
    A, Cq = n * Sxx - Sx * Sx + damping * n * n, n * Syy - Sy * Sy + damping * n * n
    Bm, bx, by = n * Sxy - Sx * Sy, n * Sxt - Sx * St, n * Syt - Sy * St
    A, Cq, Bm, bx, by = (v.astype(np.float64) for v in (A, Cq, Bm, bx, by))
    det = A * Cq - Bm * Bm
    ok = (n >= (2 * r + 1) ** 2 // 4) & (det > 0.0)
    safe = np.where(ok, det, 1.0)
    sign = 512.0 if "du_sign" in defects else -512.0
    dx, dy = sign * ((Cq * bx - Bm * by) / safe), sign * ((A * by - Bm * bx) / safe)
    dx, dy = np.clip(dx, -256.0, 256.0), np.clip(dy, -256.0, 256.0)
    rnd = np.trunc if "trunc_for_rint" in defects else np.rint                    # (rint: half to even)
    return np.where(ok, rnd(dx), 0.0).astype(np.int64), np.where(ok, rnd(dy), 0.0).astype(np.int64), ok.astype(np.uint8)


def median3(U):
    """3x3 median with clamped border; int64 [H,W]"""
    H, W = U.shape
    p = np.pad(U, 1, mode="edge")
    st = np.stack([p[a:a + H, b:b + W] for a in range(3) for b in range(3)])
    return np.sort(st, axis=0)[4]


def update(V1, V2, m1, m2, U, r, damping, defects=NONE):
    """the Jacobi update before the median: -> (U + dU int64 [2,H,W], supported uint8 [H,W]); a mask byte is set iff nonzero"""
    m1, m2 = (np.asarray(m1) != 0).astype(np.int64), (np.asarray(m2) != 0).astype(np.int64)
    gx, gy, w1 = gradients(V1, m1)
    J, w2 = sample(V2, m2, U[0], U[1], defects)
    w = w1 & w2
    It = J - V1
    gx, gy, It = w * gx, w * gy, w * It
    S = [window_sum(f, r, defects) for f in (w, gx, gy, It, gx * gx, gx * gy, gy * gy, gx * It, gy * It)]
    dx, dy, ok = solve(*S, r, damping, defects)
    return np.stack([U[0] + dx, U[1] + dy]), ok


def iterate(V1, V2, m1, m2, U, r, damping, defects=NONE):
    """one iteration at one level: -> (U int64 [2,H,W], supported uint8 [H,W])"""
    Un, ok = update(V1, V2, m1, m2, U, r, damping, defects)
    if "no_median" in defects:
        return Un, ok
    return np.stack([median3(Un[0]), median3(Un[1])]), ok


# ---- the whole flow ----------------------------------------------------------------------------------------------------------------------------
def dense_flow(img1, img2, mask1=None, mask2=None, levels=5, iters=4, radius=4, damping=65536, defects=NONE):
    """img1, img2 fp32 [3,H,W]; masks fp32 [1 or 3,H,W] or None -> (flow fp32 [2,H,W], support uint8 [H,W], fields = dict(v1, v2, m1, m2, u:
    lists per level))"""
    V1, m1 = level0(img1, mask1)
    V2, m2 = level0(img2, mask2)
    V1s, m1s = pyramid(V1, m1, levels, defects)
    V2s, m2s = pyramid(V2, m2, levels, defects)
    L = len(V1s)
    us, U, ok = [None] * L, None, None
    for l in range(L - 1, -1, -1):
        H, W = V1s[l].shape
        U = np.zeros((2, H, W), np.int64) if U is None else upscale(U, H, W, defects)
        for _ in range(iters):
            U, ok = iterate(V1s[l], V2s[l], m1s[l], m2s[l], U, radius, damping, defects)
        us[l] = U
    flow = (U.astype(np.float32) / np.float32(256)).astype(np.float32)
    return flow, ok, dict(v1=V1s, v2=V2s, m1=m1s, m2=m2s, u=us)


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------------
def smooth_field(h, w, amp, seed=0):
    """a smooth displacement of amplitude `amp` px: float64 [2,h,w] = (fx, fy), one and a bit periods across the image"""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = 0.7 * seed
    fx = amp * np.sin(2 * np.pi * (0.6 * ys / h + 0.25) + ph) * np.cos(2 * np.pi * 0.5 * xs / w + ph)
    fy = amp * np.cos(2 * np.pi * 0.55 * xs / w + 0.4 + ph) * np.sin(2 * np.pi * (0.45 * ys / h + 0.1))
    return np.stack([fx, fy])


def rgb(g):
    return np.clip(np.stack([g, g * 0.9 + 5, g * 1.05 - 3]), 0, 255).astype(np.float32)


def flow_pair(h, w, amp, seed, gain=0.85, bias=10.0, sigma=3.0, masked=True):
    """-> (img1, img2 fp32 [3,h,w], mask2 fp32 [1,h,w], f float64 [2,h,w]): image 1 is the clean scene sampled at p + f(p), image 2 the scene
    itself with gain, bias and noise, so that img1(p) ~ img2(p + f(p)); the right fifth of image 2 is masked out and black"""
    from scipy import ndimage as ndi
    pad = int(amp) + 4
    big = scene(max(h + 2 * pad, 64), max(w + 2 * pad, 64), seed)              # (the scene's rectangles need 40 px of room)
    f = smooth_field(h, w, amp, seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    im1 = ndi.map_coordinates(big, [ys + f[1] + pad, xs + f[0] + pad], order=1)
    rng = np.random.default_rng(seed + 1000)
    im2 = big[pad:pad + h, pad:pad + w] * gain + bias + rng.normal(0, sigma, (h, w))
    mask2 = np.ones((1, h, w), np.float32)
    if masked:
        mask2[:, :, w - w // 5:] = 0
        im2 = im2 * mask2[0]
    return rgb(im1), rgb(im2) * mask2, mask2, f


def homography_residual_pair(h, w, seed=3, motion=(32, 4, 0, 0, 0), amp=3.0, gain=0.85, bias=10.0, sigma=3.0):
    """-> (img1, img2 fp32 [1,3,h,w]): both cut from one procedural scene, image 2 through a known homography (_features_ref.homography_matrix)
    plus a smooth residual of `amp` px, with gain, bias and noise: what is left for the flow once the homography is found"""
    from scipy import ndimage as ndi
    from _features_ref import homography_matrix
    pad = int(0.3 * max(h, w)) + 8
    big = scene(h + 2 * pad, w + 2 * pad, seed)
    Ht = homography_matrix(h, w, *motion)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    f = smooth_field(h, w, amp, seed)
    d = Ht[2, 0] * xs + Ht[2, 1] * ys + Ht[2, 2]
    u, v = (Ht[0, 0] * xs + Ht[0, 1] * ys + Ht[0, 2]) / d + f[0], (Ht[1, 0] * xs + Ht[1, 1] * ys + Ht[1, 2]) / d + f[1]
    im1 = big[pad:pad + h, pad:pad + w]
    im2 = ndi.map_coordinates(big, [v + pad, u + pad], order=1) * gain + bias + np.random.default_rng(seed + 1000).normal(0, sigma, (h, w))
    return rgb(im1)[None], rgb(im2)[None]


def endpoint_error(flow, support, f, mask2, amp, margin=16):
    """(mean, 99th percentile, mean of a zero flow, pixels): over supported pixels more than `margin` px inside the region where both images are valid"""
    h, w = support.shape
    ys, xs = np.mgrid[0:h, 0:w]
    right = np.flatnonzero(mask2[0, 0] <= 0.5)
    xmax = (right[0] if right.size else w) - margin - int(np.ceil(amp))
    sel = (support > 0) & (ys >= margin) & (ys < h - margin) & (xs >= margin) & (xs < xmax)
    e = np.hypot(flow[0] - f[0], flow[1] - f[1])[sel]
    z = np.hypot(f[0], f[1])[sel]
    return float(e.mean()), float(np.percentile(e, 99)), float(z.mean()), int(sel.sum())
