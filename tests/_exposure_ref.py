"""CPU restatement of the exposure-compensation contract (README.md, exposure compensation; csrc/exposure.hip): the statistics in integer
numpy, the gain solve in float64 operation for operation, the smoothing, interpolation and apply step in numpy float32 -- every product
and sum below is one array operation, so one rounding, in the order the kernels use.

``defects``: a set of names from DEFECTS, each of which plants one deviation from the contract (tests/test_exposure_cpu.py shows that
every one of them fails an assertion).  Production callers pass none."""
import numpy as np

DEFECTS = ("round_p", "y_without_half", "h_before_w", "centre_without_half", "no_edge_clamp", "min_count_ignored", "prior_one",
           "no_final_clamp", "fma_apply")
BLOCKS = (8, 16, 32, 64)
GAIN_MIN, GAIN_MAX = 0.25, 4.0
NONE = frozenset()
f32 = np.float32


def to_u8(img, defects=NONE):
    """the saver's rule: clamp to 0..255, truncate toward zero -> int64; NaN -> 0, -Inf -> 0, +Inf -> 255 (`st_u8_trunc`)"""
    x = np.asarray(img, dtype=np.float64)
    x = np.clip(np.where(np.isnan(x), 0, x), 0, 255)
    return (np.rint(x) if "round_p" in defects else np.trunc(x)).astype(np.int64)


def luma(p, defects=NONE):
    """p int [3,...] -> the integer luma of cv_inpainter (PIL's RGB -> L)"""
    half = 0 if "y_without_half" in defects else 0x8000
    return (19595 * p[0] + 38470 * p[1] + 7471 * p[2] + half) >> 16


def planes(img, defects=NONE):
    """img [3,H,W] -> int64 [4,H,W]: R, G, B, Y"""
    p = to_u8(img, defects)
    return np.concatenate([p, luma(p, defects)[None]])


def grid(H, W, block):
    return -(-H // block), -(-W // block)


def stats(img1, img2, mask1, mask2, block=32, defects=NONE):
    """int64 [Th,Tw,9]: per tile N, S1[R,G,B,Y], S2[R,G,B,Y] over the overlap (channel 0 of both masks > 0.5)"""
    O = (np.asarray(mask1)[0] > 0.5) & (np.asarray(mask2)[0] > 0.5)
    H, W = O.shape
    Th, Tw = grid(H, W, block)
    words = np.concatenate([O[None].astype(np.int64), planes(img1, defects) * O, planes(img2, defects) * O])          # [9,H,W]
    pad = np.zeros((9, Th * block, Tw * block), np.int64)
    pad[:, :H, :W] = words
    rec = pad.reshape(9, Th, block, Tw, block).sum(axis=(2, 4))
    assert rec.max() < 2 ** 32
    return np.moveaxis(rec, 0, -1)


def weights(sigma_n=10.0, sigma_g=0.1):
    return 1.0 / (sigma_n * sigma_n), 1.0 / (sigma_g * sigma_g)


def solve64(N, S1, S2, G1, G2, alpha, beta):
    """the eleven steps of the contract in float64 scalars, before the clamp"""
    N, S1, S2, G1, G2 = (np.float64(v) for v in (N, S1, S2, G1, G2))
    n2 = N * N
    a11 = alpha * (S1 * S1) + beta * n2
    a22 = alpha * (S2 * S2) + beta * n2
    a12 = alpha * (S1 * S2)
    r1 = (beta * n2) * G1
    r2 = (beta * n2) * G2
    det = a11 * a22 - a12 * a12
    return (r1 * a22 + r2 * a12) / det, (r2 * a11 + r1 * a12) / det


def solve(N, S1, S2, G1, G2, alpha, beta):
    """-> (g1, g2) as np.float32: N = 0 gives the prior, else the solve, clamped to [0.25, 4], rounded to fp32"""
    if N == 0:
        return f32(G1), f32(G2)
    g1, g2 = solve64(N, S1, S2, G1, G2, alpha, beta)
    return f32(min(max(g1, GAIN_MIN), GAIN_MAX)), f32(min(max(g2, GAIN_MIN), GAIN_MAX))


def global_gains(rec, alpha, beta):
    """rec [Th,Tw,9] -> fp32 [4,2]: plane R, G, B, Y; (G1, G2) = solve(sum of the tile records, 1, 1)"""
    tot = rec.reshape(-1, 9).astype(np.int64).sum(axis=0)
    return np.array([solve(tot[0], tot[1 + p], tot[5 + p], 1.0, 1.0, alpha, beta) for p in range(4)], dtype=f32)


def tile_gains(rec, G, plane_ids, min_count, alpha, beta, defects=NONE):
    """fp32 [sets,2,Th,Tw]: solve(tile record, G1, G2) of each plane in `plane_ids`; a tile with N < min_count is treated as N = 0"""
    Th, Tw, _ = rec.shape
    out = np.empty((len(plane_ids), 2, Th, Tw), f32)
    for s, p in enumerate(plane_ids):
        prior = (1.0, 1.0) if "prior_one" in defects else (float(G[p, 0]), float(G[p, 1]))
        for i in range(Th):
            for j in range(Tw):
                N = int(rec[i, j, 0])
                if N < min_count and "min_count_ignored" not in defects:
                    N = 0
                out[s, :, i, j] = solve(N, int(rec[i, j, 1 + p]), int(rec[i, j, 5 + p]), prior[0], prior[1], alpha, beta)
    return out


def _take(a, idx, axis, defects):
    """a[..., idx, ...] with the indices clamped to the table (the defect: entries outside the table read as 0)"""
    n = a.shape[axis]
    got = np.take(a, np.clip(idx, 0, n - 1), axis=axis)
    if "no_edge_clamp" in defects:
        shape = [1] * a.ndim
        shape[axis] = len(idx)
        got = np.where(((idx >= 0) & (idx < n)).reshape(shape), got, f32(0))
    return got


def smooth1(t, axis, defects=NONE):
    i = np.arange(t.shape[axis])
    return (f32(0.25) * _take(t, i - 1, axis, defects) + f32(0.5) * t) + f32(0.25) * _take(t, i + 1, axis, defects)


def smooth(t, times, defects=NONE):
    """fp32 [...,Th,Tw]: `times` passes of (0.25, 0.5, 0.25), along W, the result rounded to fp32, then along H"""
    t = np.asarray(t, f32)
    for _ in range(times):
        t = smooth1(smooth1(t, -2, defects), -1, defects) if "h_before_w" in defects else smooth1(smooth1(t, -1, defects), -2, defects)
    return t


def coords(n, block, defects=NONE):
    """pixel centres 0..n-1 -> (i0 int64 [n], f fp32 [n]): u = (x + 0.5) / block - 0.5, i0 = floor(u), f = u - i0"""
    u = (np.arange(n, dtype=f32) + f32(0.5)) / f32(block)
    if "centre_without_half" not in defects:
        u = u - f32(0.5)
    i0 = np.floor(u)
    return i0.astype(np.int64), (u - i0).astype(f32)


def interpolate(table, H, W, block, defects=NONE):
    """fp32 [Th,Tw] -> fp32 [H,W]: g = (g00 (1 - fx) + g01 fx) (1 - fy) + (g10 (1 - fx) + g11 fx) fy, indices clamped to the table"""
    table = np.asarray(table, f32)
    iy, fy = coords(H, block, defects)
    ix, fx = coords(W, block, defects)
    r0, r1 = _take(table, iy, 0, defects), _take(table, iy + 1, 0, defects)
    g00, g01, g10, g11 = _take(r0, ix, 1, defects), _take(r0, ix + 1, 1, defects), _take(r1, ix, 1, defects), _take(r1, ix + 1, 1, defects)
    fx, fy, one = fx[None, :], fy[:, None], f32(1)
    return (g00 * (one - fx) + g01 * fx) * (one - fy) + (g10 * (one - fx) + g11 * fx) * fy


def finish(p, g, defects=NONE):
    """p fp32 (integer-valued), g fp32 -> min(floor(p g + 0.5), 255) as fp32"""
    p, g = np.asarray(p, f32), np.asarray(g, f32)
    if "fma_apply" in defects:                     # one rounding: the product of an 8-bit and a 24-bit number plus 0.5 is exact in float64
        v = (p.astype(np.float64) * g.astype(np.float64) + 0.5).astype(f32)
    else:
        v = p * g + f32(0.5)
    v = np.floor(v)
    return v if "no_final_clamp" in defects else np.minimum(v, f32(255))


def apply(img1, img2, tables, block=32, defects=NONE):
    """tables fp32 [sets,2,th,tw], sets = 1 (all channels) or 3 -> (out1, out2) fp32 [3,H,W]"""
    tables = np.asarray(tables, f32)
    H, W = np.asarray(img1).shape[1:]
    outs = []
    for im, img in enumerate((img1, img2)):
        p = to_u8(img, defects).astype(f32)
        g = np.stack([interpolate(tables[s, im], H, W, block, defects) for s in range(tables.shape[0])])
        outs.append(finish(p, g if len(g) == 3 else g[:1], defects).astype(f32))
    return outs[0], outs[1]


def gain_tables(img1, img2, mask1, mask2, mode="gain", block=32, channels=False, min_count=None, smooth_passes=2, sigma_n=10.0, sigma_g=0.1,
                defects=NONE):
    """the tables the apply step reads: fp32 [sets,2,Th,Tw] in "blocks", [sets,2,1,1] in "gain" """
    if block not in BLOCKS or mode not in ("gain", "blocks") or not 0 <= smooth_passes <= 8:
        raise ValueError((block, mode, smooth_passes))
    alpha, beta = weights(sigma_n, sigma_g)
    rec = stats(img1, img2, mask1, mask2, block, defects)
    G = global_gains(rec, alpha, beta)
    ids = (0, 1, 2) if channels else (3,)
    if mode == "gain":
        return G[list(ids)][:, :, None, None].copy()
    if min_count is None:
        min_count = block * block // 8
    return smooth(tile_gains(rec, G, ids, min_count, alpha, beta, defects), smooth_passes, defects)


def compensate(img1, img2, mask1, mask2, mode="gain", block=32, channels=False, min_count=None, smooth_passes=2, sigma_n=10.0, sigma_g=0.1,
               defects=NONE):
    """the whole contract: img [3,H,W], mask [1 or 3,H,W] -> (out1, out2, tables)"""
    tables = gain_tables(img1, img2, mask1, mask2, mode, block, channels, min_count, smooth_passes, sigma_n, sigma_g, defects)
    out1, out2 = apply(img1, img2, tables, block, defects)
    return out1, out2, tables
