"""CPU restatement of the tps_method="other" contract (README.md, "tps_method other"; csrc/tps_other.hip): per-axis r^2 ln(r + 1e-6)
splines fitted in fp64, fp64 maps summed in index order, and cv2.remap INTER_CUBIC 8U fixed point with a constant 0 border.
The coefficient table comes from the package (ops.cubic_remap_table): this file restates how it is used, not how it is built."""
import numpy as np

EPS = 1e-6


def normalise(points, out_h, out_w):
    """pixel (x, y) [n,2] -> float32 (x / out_w, y / out_h), divided in float64 (tps_pipline.py:407-415)"""
    p = np.asarray(points, np.float64)
    return np.stack([p[:, 0] / out_w, p[:, 1] / out_h], 1).astype(np.float32)


def dedup_first(c_src, c_dst):
    """coincident sites: keep the first occurrence of each c_dst row, in the original order"""
    _, first = np.unique(c_dst, axis=0, return_index=True)
    keep = np.sort(first)
    return c_src[keep], c_dst[keep]


def u(r):
    return r * r * np.log(r + EPS)


def fit(c_src, c_dst):
    """[[K, P], [P^T, 0]] theta = [delta; 0] in fp64 from the float32 sites; -> (kw [n,2], aw [3,2]) rounded to float32"""
    c = np.asarray(c_dst, np.float32).astype(np.float64)
    delta = (np.asarray(c_src, np.float32) - np.asarray(c_dst, np.float32)).astype(np.float64)
    n = c.shape[0]
    d = np.sqrt((c[:, None, 0] - c[None, :, 0]) ** 2 + (c[:, None, 1] - c[None, :, 1]) ** 2)
    A = np.zeros((n + 3, n + 3))
    A[:n, :n] = u(d)
    A[:n, n] = 1.0
    A[:n, n + 1:] = c
    A[n:, :n] = A[:n, n:].T
    rhs = np.zeros((n + 3, 2))
    rhs[:n] = delta
    theta = np.linalg.solve(A, rhs).astype(np.float32)
    return theta[:n], theta[n:]


def from_reduced(theta, n):
    """the reference's reduced theta [n+2, 2] = (w_1..w_{n-1}, a0, a1, a2) -> (kw [n,2] with w_0 = 0 (replaced), aw [3,2])"""
    theta = np.asarray(theta, np.float32)
    kw = np.zeros((n, 2), np.float32)
    kw[1:] = theta[:n - 1]
    return kw, theta[n - 1:].copy()


def f32_sum(a):
    """numpy's float32 add.reduce of a 1-D array (pairwise_sum: 8 running sums over blocks of up to 128, halves above that)"""
    f = np.float32
    a = np.asarray(a, np.float32)
    n = len(a)
    if n < 8:
        r = f(0)
        for v in a:
            r = f(r + v)
        return r
    if n <= 128:
        r = [a[j] for j in range(8)]
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] = f(r[j] + a[i + j])
            i += 8
        res = f(f(f(r[0] + r[1]) + f(r[2] + r[3])) + f(f(r[4] + r[5]) + f(r[6] + r[7])))
        for v in a[i:]:
            res = f(res + v)
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return f(f32_sum(a[:n2]) + f32_sum(a[n2:]))


def _f32_leaf(a):
    """the block of f32_sum applied to a whole array, whatever its length"""
    f = np.float32
    n = len(a)
    if n < 8:
        r = f(0)
        for v in a:
            r = f(r + v)
        return r
    r = [a[j] for j in range(8)]
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] = f(r[j] + a[i + j])
        i += 8
    res = f(f(f(r[0] + r[1]) + f(r[2] + r[3])) + f(f(r[4] + r[5]) + f(r[6] + r[7])))
    for v in a[i:]:
        res = f(res + v)
    return res


# Three wrong summations, each one way a kernel's copy of f32_sum can go wrong while staying a sum (tests/test_other_tps_cpu.py shows
# that the inputs of `case` tell every one of them from f32_sum; tests/test_other_tps_matrix_gpu.py leans on that).
def sum_in_order(a):
    """WRONG: one running float32 sum in index order.  Defined differently from f32_sum from 8 elements on."""
    r = np.float32(0)
    for v in np.asarray(a, np.float32):
        r = np.float32(r + v)
    return r


def sum_leaf_no_split(a):
    """WRONG: the eight-lane block over the whole array, never halved.  Defined differently from f32_sum above 128 elements."""
    return _f32_leaf(np.asarray(a, np.float32))


def sum_halves_unrounded(a):
    """WRONG: the halving recursion with n2 = n // 2, not rounded down to a multiple of 8.  Defined differently from f32_sum
    wherever unrounded_halves_differ(len(a))."""
    a = np.asarray(a, np.float32)
    n = len(a)
    if n <= 128:
        return _f32_leaf(a)
    return np.float32(sum_halves_unrounded(a[:n // 2]) + sum_halves_unrounded(a[n // 2:]))


def unrounded_halves_differ(m):
    """whether sum_halves_unrounded splits m elements differently from f32_sum at any level (129, 256 and 512 do not)"""
    if m <= 128:
        return False
    h = m // 2
    return h % 8 != 0 or unrounded_halves_differ(h) or unrounded_halves_differ(m - h)


# The control-point counts of the teacher-forced maps tests.  n - 1 elements are summed for w_0: 0, fewer than 8, exactly 8, 8 plus
# a tail (1..17); the 128-element block limit and the first split, 129 = 64 + 65 (129, 130); 136 and 137 elements, whose halves are
# (64 + 72) and are not (64 + 73) multiples of 8; both sides of the staging chunk of 256 centres (255..264) and a partial third chunk
# (513); 2055, the right half of 4095, which itself splits off a 1031; the accepted maximum 4096.
N_TABLE = (1, 2, 3, 8, 9, 10, 17, 128, 129, 130, 137, 138, 255, 256, 257, 264, 300, 512, 513, 1031, 2055, 4095, 4096)
CASE_SEED = {}                      # n -> seed, where 7000 + n does not meet the conditions of tests/test_other_tps_cpu.py (none so far)
PROBE_R = 3.0


def case(n):
    """-> (kw [n,2], aw [3,2], centres [n,2]) float32, seeded by n: weights small enough that the map stays a map, large enough
    that the spline term, not the affine one, decides its last bits"""
    rng = np.random.default_rng(CASE_SEED.get(n, 7000 + n))
    kw = (0.05 * rng.standard_normal((n, 2))).astype(np.float32)
    aw = (0.01 * rng.standard_normal((3, 2))).astype(np.float32)
    centres = rng.uniform(-0.1, 1.1, (n, 2)).astype(np.float32)
    return kw, aw, centres


def probe_case(n):
    """the w_0 probe on a 1 x 1 canvas (x = y = 0): centres 1..n-1 at the origin, where U(0) = 0 exactly, centre 0 at (PROBE_R, 0)
    and no affine part, so that the maps are float32(U(PROBE_R) * w_0[axis]) and nothing else"""
    kw = case(n)[0]
    centres = np.zeros((n, 2), np.float32)
    centres[0, 0] = PROBE_R
    return kw, np.zeros((3, 2), np.float32), centres


def reduce_w0(kw):
    """w_0 = -sum_{i>=1} w_i as the reference computes it: np.sum of the float32 weights (other_tps.py TPS.z)"""
    kw = np.asarray(kw, np.float32).copy()
    for a in range(2):
        kw[0, a] = -f32_sum(kw[1:, a])
    return kw


def grid_axes(H, W):
    return np.linspace(0, 1, W, dtype=np.float32), np.linspace(0, 1, H, dtype=np.float32)


def maps(kw, aw, c_dst, H, W):
    """-> (mapx, mapy) float32 [H,W]: the reduced-form spline on the float32 linspace grid, scaled by W and H (not W-1, H-1)"""
    kw = reduce_w0(kw).astype(np.float64)
    aw = np.asarray(aw, np.float32).astype(np.float64)
    c = np.asarray(c_dst, np.float32).astype(np.float64)
    xs, ys = grid_axes(H, W)
    x = np.broadcast_to(xs.astype(np.float64)[None, :], (H, W))
    y = np.broadcast_to(ys.astype(np.float64)[:, None], (H, W))
    sx, sy = np.zeros((H, W)), np.zeros((H, W))
    for k in range(c.shape[0]):
        r = np.sqrt((x - c[k, 0]) ** 2 + (y - c[k, 1]) ** 2)
        uk = u(r)
        sx = sx + uk * kw[k, 0]
        sy = sy + uk * kw[k, 1]
    dx = ((aw[0, 0] + aw[1, 0] * x) + aw[2, 0] * y) + sx
    dy = ((aw[0, 1] + aw[1, 1] * x) + aw[2, 1] * y) + sy
    return ((x + dx) * W).astype(np.float32), ((y + dy) * H).astype(np.float32)


def quantise(planes):
    """float planes -> the uint8 values cv2 sees (to_pillow_fn): truncate toward zero, clamp to 0..255 (tps2_warp_kernel's rule)"""
    p = np.nan_to_num(np.asarray(planes, np.float32), nan=0.0)
    return np.clip(np.trunc(p), 0, 255).astype(np.int32)


def quantise_map(m):
    """X = cvRound(m * 32) (half to even); -> (sx, fx, ok) with ok False where no tap can be inside (non-finite or |m| >= 2^26)"""
    m = np.asarray(m, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.abs(m) < np.float32(2.0 ** 26)
        X = np.where(ok, np.rint(np.where(ok, m, 0).astype(np.float32) * np.float32(32)), 0).astype(np.int64)
    return X >> 5, X & 31, ok


def remap_cubic(planes_u8, mapx, mapy, table, saturate=True):
    """cv2.remap(INTER_CUBIC, BORDER_CONSTANT 0) on integer planes [P,Hs,Ws] -> int32 [P,H,W] in 0..255
    (saturate=False: the rounded sum before the clamp, to see whether a case reaches it)"""
    src = np.asarray(planes_u8, np.int64)
    P, Hs, Ws = src.shape
    sx, fx, okx = quantise_map(mapx)
    sy, fy, oky = quantise_map(mapy)
    ok = okx & oky
    tab = np.asarray(table, np.int64).reshape(32 * 32, 16)[(fy * 32 + fx)]            # [H,W,16]
    acc = np.zeros((P,) + sx.shape, np.int64)
    for k1 in range(4):
        yy = sy - 1 + k1
        for k2 in range(4):
            xx = sx - 1 + k2
            inside = ok & (yy >= 0) & (yy < Hs) & (xx >= 0) & (xx < Ws)
            v = src[:, np.where(inside, yy, 0), np.where(inside, xx, 0)] * inside
            acc += v * tab[..., k1 * 4 + k2]
    res = (acc + 16384) >> 15
    return (np.clip(res, 0, 255) if saturate else res).astype(np.int32)


def warp_other(H_warp, H_warp_mask, points_src, points_dst, out_h, out_w, table):
    """warp_by_tps(..., "other") on numpy [1,3,H,W] canvases and pixel points [n,2] -> float32 [1,6,H,W]"""
    planes = quantise(np.concatenate([np.asarray(H_warp)[0], np.asarray(H_warp_mask)[0]], 0))
    H, W = planes.shape[-2:]
    cs, cd = dedup_first(normalise(points_src, out_h, out_w), normalise(points_dst, out_h, out_w))
    kw, aw = fit(cs, cd)
    mx, my = maps(kw, aw, cd, H, W)
    return remap_cubic(planes, mx, my, table)[None].astype(np.float32), (mx, my), (kw, aw)
