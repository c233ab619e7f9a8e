"""CPU restatement of csrc/features.hip (README.md, "feature_align"): Harris corners, upright BRIEF-256, mutual nearest-neighbour matching
and a RANSAC homography, vectorised numpy.  Corners, descriptors and matching are integers; the RANSAC is fp64, one rounding per product,
sum and quotient (numpy's element-wise operations never contract).  The contract is this project's own: it is pinned against no library.
`homography` is what `ops.feature_homography` must equal bit for bit: keypoints, descriptors, the best / second-best planes, the match list,
the winner, the inlier mask, H, motion and info.  `defects` plants one of DEFECTS, for tests/test_features_cpu.py: each of them must break
an assertion there."""
import numpy as np
from scipy import ndimage as ndi

MIN_SIDE, MAX_SIDE, MAX_BATCH, MAX_HYP = 64, 1024, 64, 65536
CELL, PER_CELL, BORDER = 32, 4, 16
MAX_DIST, RATIO_NUM, RATIO_DEN, NO_DIST = 80, 8, 10, 257
MIN_MATCHES = 8
PIVOT_MIN = 1e-10
PATTERN_KEY = 0x9E3779B9
NONE = frozenset()
DEFECTS = ("nms_ge_lower", "tie_highest_slot", "no_mutual", "ratio_reversed", "bit_order", "draw_without_seed", "two_sided_error", "refit_all_matches",
           "motion_from_w_minus_1")
M32 = np.uint64(0xFFFFFFFF)


def fmix32(x):
    """murmur3's 32-bit finaliser"""
    x = np.asarray(x, np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & M32
    return x ^ (x >> np.uint64(16))


def slots(H, W):
    return PER_CELL * (-(-H // CELL)) * (-(-W // CELL))


# ---- operands --------------------------------------------------------------------------------------------------------------------------------
def pixels(img):
    """fp32 [3,H,W] -> int64: trunc(clamp(x, 0, 255)); NaN and -Inf read 0, +Inf 255"""
    x = np.asarray(img, np.float32)
    x = np.where(np.isnan(x), np.float32(0), x)
    return np.clip(x, 0, 255).astype(np.int64)


def luma(img):
    p = pixels(img)
    return (19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 0x8000) >> 16


# ---- corners ---------------------------------------------------------------------------------------------------------------------------------
def window_sum(a, r):
    """sum over the (2r + 1)^2 window, terms outside the array 0"""
    H, W = a.shape
    p = np.pad(a, r)
    out = np.zeros_like(a)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out += p[dy:dy + H, dx:dx + W]
    return out


def sobel(Y):
    p = np.pad(Y, 1, mode="edge")
    ix = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    iy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    return ix, iy


def harris(Y):
    """R = 16 (A B - C^2) - (A + B)^2 over the 7x7 window of the Sobel gradients of Y (border replicated); int64"""
    ix, iy = sobel(Y)
    A, B, C = window_sum(ix * ix, 3), window_sum(iy * iy, 3), window_sum(ix * iy, 3)
    assert max(A.max(), B.max(), np.abs(C).max()) < 2 ** 31
    return 16 * (A * B - C * C) - (A + B) ** 2


def candidates(R, defects=NONE):
    """at least 16 px from every edge, R > 0, R >= all 8 neighbours and > those with a lower row-major index"""
    H, W = R.shape
    ok = R > 0
    ok[:BORDER] = ok[H - BORDER:] = False
    ok[:, :BORDER] = ok[:, W - BORDER:] = False
    p = np.pad(R, 1, constant_values=np.iinfo(np.int64).max)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            q = p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            lower = dy < 0 or (dy == 0 and dx < 0)
            ok &= (R > q) if lower and "nms_ge_lower" not in defects else (R >= q)
    return ok


def select(R, cand):
    """per 32x32 cell (ragged at the right and bottom) the best 4 candidates by (R descending, index ascending); slot = 4 cell + rank;
    int32 [N,2] = (x, y), (-1, -1) in an unused slot"""
    H, W = R.shape
    CH, CW = -(-H // CELL), -(-W // CELL)
    kp = np.full((PER_CELL * CH * CW, 2), -1, np.int32)
    ys, xs = np.nonzero(cand)
    cell = (ys // CELL) * CW + xs // CELL
    order = np.lexsort((ys * W + xs, -R[ys, xs], cell))
    cell, ys, xs = cell[order], ys[order], xs[order]
    start = np.r_[0, np.nonzero(np.diff(cell))[0] + 1] if len(cell) else np.zeros(0, np.int64)
    rank = np.arange(len(cell)) - np.repeat(start, np.diff(np.r_[start, len(cell)]))
    keep = rank < PER_CELL
    kp[PER_CELL * cell[keep] + rank[keep]] = np.stack([xs[keep], ys[keep]], 1)
    return kp


def detect(img, defects=NONE):
    """-> (kp int32 [N,2], box int64 [H,W])"""
    Y = luma(img)
    R = harris(Y)
    return select(R, candidates(R, defects)), window_sum(Y, 2)


# ---- descriptor ------------------------------------------------------------------------------------------------------------------------------
def brief_pattern():
    """int8 [256,4] = (ax, ay, bx, by): entry i of the flat table is fmix32(key ^ i) mod 25 - 12"""
    return (fmix32(np.uint64(PATTERN_KEY) ^ np.arange(1024, dtype=np.uint64)) % np.uint64(25)).astype(np.int64).reshape(256, 4).astype(np.int8) - np.int8(12)


def describe_bits(box, kp):
    """bool [N,256]: bit k = S(p + a_k) < S(p + b_k); all False for an unused slot"""
    pat = brief_pattern().astype(np.int64)
    valid = kp[:, 0] >= 0
    x, y = np.where(valid, kp[:, 0], BORDER).astype(np.int64)[:, None], np.where(valid, kp[:, 1], BORDER).astype(np.int64)[:, None]
    bits = box[y + pat[None, :, 1], x + pat[None, :, 0]] < box[y + pat[None, :, 3], x + pat[None, :, 2]]
    return bits & valid[:, None]


def pack_bits(bits, defects=NONE):
    """bit k at word k >> 5, position k & 31; uint32 [N,8]"""
    b = bits.reshape(len(bits), 8, 32).astype(np.uint64)
    pos = np.arange(32, dtype=np.uint64)
    if "bit_order" in defects:
        pos = pos[::-1]
    return (b << pos).sum(2).astype(np.uint32)


def describe(box, kp, defects=NONE):
    return pack_bits(describe_bits(box, kp), defects)


# ---- match -----------------------------------------------------------------------------------------------------------------------------------
POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def hamming(dq, dc):
    """int64 [Nq,Nc]"""
    out = np.empty((len(dq), len(dc)), np.int64)
    for i0 in range(0, len(dq), 128):                           # (blocks bound the [Nq,Nc,32] plane)
        x = np.ascontiguousarray(dq[i0:i0 + 128, None, :] ^ dc[None, :, :])
        out[i0:i0 + 128] = POP8[x.view(np.uint8)].sum(2, dtype=np.int64)
    return out


def nearest(kq, dq, kc, dc, defects=NONE):
    """for every valid query slot: (best valid candidate slot, ties to the lowest; d1; d2 = the least distance over the other valid slots or
    257); (-1, 257, 257) for an unused query slot or without any candidate; int32 [N,3]"""
    N = len(kq)
    out = np.tile(np.array([-1, NO_DIST, NO_DIST], np.int32), (N, 1))
    vq, vc = kq[:, 0] >= 0, kc[:, 0] >= 0
    if not vq.any() or not vc.any():
        return out
    D = hamming(dq, dc)
    D[:, ~vc] = 1 << 20
    if "tie_highest_slot" in defects:
        j = N - 1 - np.argmin(D[:, ::-1], 1)
    else:
        j = np.argmin(D, 1)
    d1 = D[np.arange(N), j]
    D[np.arange(N), j] = 1 << 20
    d2 = D.min(1)
    d2 = np.where(d2 >= 1 << 20, NO_DIST, d2)
    out[vq] = np.stack([j, d1, d2], 1)[vq]
    return out


def match(kp1, d1, kp2, d2, defects=NONE):
    """-> (nn int32 [2,N,3], matches int32 [N,2], m): (i, j) iff d1 < 80, 10 d1 < 8 d2 and i is j's best in the reverse direction"""
    N = len(kp1)
    nn = np.stack([nearest(kp1, d1, kp2, d2, defects), nearest(kp2, d2, kp1, d1, defects)])
    j, a, b = nn[0, :, 0].astype(np.int64), nn[0, :, 1].astype(np.int64), nn[0, :, 2].astype(np.int64)
    ratio = (RATIO_DEN * a > RATIO_NUM * b) if "ratio_reversed" in defects else (RATIO_DEN * a < RATIO_NUM * b)
    ok = (j >= 0) & (a < MAX_DIST) & ratio
    if "no_mutual" not in defects:
        ok &= nn[1, np.maximum(j, 0), 0] == np.arange(N)
    i = np.nonzero(ok)[0]
    matches = np.full((N, 2), -1, np.int32)
    matches[:len(i)] = np.stack([i, j[i]], 1)
    return nn, matches, len(i)


# ---- RANSAC ----------------------------------------------------------------------------------------------------------------------------------
def normalise(kp1, kp2, matches, m, H, W):
    """fp64 [m,4] = (x1, y1, x2, y2) as (x - W/2) / (W/2), (y - H/2) / (H/2)"""
    sx, sy = np.float64(0.5 * W), np.float64(0.5 * H)
    a, b = kp1[matches[:m, 0]].astype(np.float64), kp2[matches[:m, 1]].astype(np.float64)
    return np.stack([(a[:, 0] - sx) / sx, (a[:, 1] - sy) / sy, (b[:, 0] - sx) / sx, (b[:, 1] - sy) / sy], 1)


def draws(seed, k, m, defects=NONE):
    """int64 [K,4]: index t of hypothesis k is fmix32(fmix32(seed ^ fmix32(k)) ^ (t + 1)) mod m"""
    s = np.uint64(0 if "draw_without_seed" in defects else int(seed) & 0xFFFFFFFF)
    key = fmix32(s ^ fmix32(np.asarray(k, np.uint64)))
    return (fmix32(key[:, None] ^ np.arange(1, 5, dtype=np.uint64)[None, :]) % np.uint64(m)).astype(np.int64)


def rows(mc):
    """the two rows [.., 2, 9] a match (x, y) -> (u, v) contributes: [x y 1 0 0 0 -ux -uy | u], [0 0 0 x y 1 -vx -vy | v]"""
    x, y, u, v = mc[..., 0], mc[..., 1], mc[..., 2], mc[..., 3]
    o, z = np.ones_like(x), np.zeros_like(x)
    return np.stack([np.stack([x, y, o, z, z, z, -u * x, -u * y, u], -1), np.stack([z, z, z, x, y, o, -v * x, -v * y, v], -1)], -2)


def solve8(A):
    """Gaussian elimination with partial pivoting (first row on ties) of K systems [K,8,9]; a pivot magnitude below 1e-10 (or a NaN) voids
    a system -> (ok bool [K], x fp64 [K,8])"""
    A = np.array(A, np.float64)
    K = len(A)
    ok = np.ones(K, bool)
    ar = np.arange(K)
    with np.errstate(all="ignore"):
        for c in range(8):
            mag = np.abs(A[:, c:, c])
            mag = np.where(np.isnan(mag), -1.0, mag)            # (the device's v > best is false for a NaN)
            piv = c + np.argmax(mag, 1)
            best = np.abs(A[ar, piv, c])
            ok &= best >= PIVOT_MIN
            rc, rp = A[ar, c].copy(), A[ar, piv].copy()
            A[ar, c], A[ar, piv] = rp, rc
            pv = A[:, c, c]
            for r in range(c + 1, 8):
                f = A[:, r, c] / pv
                A[:, r, c + 1:] = A[:, r, c + 1:] - f[:, None] * A[:, c, c + 1:]
        x = np.zeros((K, 8))
        for r in range(7, -1, -1):
            s = A[:, r, 8].copy()
            for k in range(r + 1, 8):
                s = s - A[:, r, k] * x[:, k]
            x[:, r] = s / A[:, r, r]
    return ok, x


def inliers(h, mc, H, W, thr, defects=NONE):
    """bool [K,m]: a positive denominator and a squared one-sided reprojection error, in pixels, below thr^2"""
    h = np.asarray(h, np.float64).reshape(-1, 8)[:, :, None]
    x, y, u, v = (mc[None, :, i] for i in range(4))
    sx, sy = np.float64(0.5 * W), np.float64(0.5 * H)
    thr2 = np.float64(thr) * np.float64(thr)
    with np.errstate(all="ignore"):
        den = (h[:, 6] * x + h[:, 7] * y) + 1.0
        px, py = ((h[:, 0] * x + h[:, 1] * y) + h[:, 2]) / den, ((h[:, 3] * x + h[:, 4] * y) + h[:, 5]) / den
        ex, ey = (px - u) * sx, (py - v) * sy
        e = ex * ex + ey * ey
        if "two_sided_error" in defects:                        # plus the error of the inverse map in image 1
            for hk in range(len(h)):
                a = np.append(h[hk, :, 0], 1.0).reshape(3, 3)
                Hi = np.stack([np.cross(a[1], a[2]), np.cross(a[2], a[0]), np.cross(a[0], a[1])], 1)       # the adjugate: the inverse up to scale
                q = Hi @ np.stack([u[0], v[0], np.ones_like(u[0])])
                e[hk] += ((q[0] / q[2] - x[0]) * sx) ** 2 + ((q[1] / q[2] - y[0]) * sy) ** 2
        return (den > 0.0) & (e < thr2)


def normal_equations(mc, mask):
    """A^T A [8,8] and A^T b [8] as one [8,9] system: every entry is (s0 + s1) + (s2 + s3), s_q the sum over the inliers at list positions
    p = q mod 4 in list order, row 1's product then row 2's"""
    part = []
    for q in range(4):
        sel = mask & (np.arange(len(mask)) % 4 == q)
        r = rows(mc[sel])                                       # [n,2,9]
        terms = (r[:, :, :8, None] * r[:, :, None, :]).reshape(-1, 8, 9)
        part.append(np.add.accumulate(np.concatenate([np.zeros((1, 8, 9)), terms]), 0)[-1])
    return (part[0] + part[1]) + (part[2] + part[3])


def to_pixels(h, H, W, defects=NONE):
    """normalised h [8] -> (H fp32 [3,3] in pixel units with h33 = 1, motion fp32 [4,2], finite)"""
    sx, sy = np.float64(0.5 * W), np.float64(0.5 * H)
    h = np.append(np.asarray(h, np.float64), 1.0).reshape(3, 3)
    with np.errstate(all="ignore"):
        M = np.stack([h[:, 0] / sx, h[:, 1] / sy, (h[:, 2] - h[:, 0]) - h[:, 1]], 1)
        P = np.stack([sx * M[0] + sx * M[2], sy * M[1] + sy * M[2], M[2]])
        Hf = (P / P[2, 2]).astype(np.float32)
        Hf[2, 2] = 1.0
        motion = np.zeros((4, 2), np.float32)
        for q in range(4):
            xn, yn = (1.0 if q & 1 else -1.0), (1.0 if q & 2 else -1.0)
            cx, cy = (float(W) if q & 1 else 0.0), (float(H) if q & 2 else 0.0)
            if "motion_from_w_minus_1" in defects:
                cx, cy = (float(W - 1) if q & 1 else 0.0), (float(H - 1) if q & 2 else 0.0)
                xn, yn = (np.float64(cx) - sx) / sx, (np.float64(cy) - sy) / sy
            den = (h[2, 0] * xn + h[2, 1] * yn) + 1.0
            ux, uy = ((h[0, 0] * xn + h[0, 1] * yn) + h[0, 2]) / den, ((h[1, 0] * xn + h[1, 1] * yn) + h[1, 2]) / den
            motion[q] = np.float32((ux * sx + sx) - cx), np.float32((uy * sy + sy) - cy)
    return Hf, motion, bool(np.isfinite(Hf).all() and np.isfinite(motion).all())


def ransac(kp1, kp2, matches, m, H, W, max_hyp=2048, thr=3.0, min_inliers=12, seed=1, defects=NONE, return_scores=False):
    """-> (motion fp32 [4,2], H fp32 [3,3], info int32 [8], mask uint8 [N])"""
    N = len(kp1)
    n1, n2 = int((kp1[:, 0] >= 0).sum()), int((kp2[:, 0] >= 0).sum())
    mask = np.zeros(N, np.uint8)
    scores = np.full(max_hyp, -1, np.int64)
    winner, have, count, h = -1, False, 0, np.zeros(8)
    if m >= MIN_MATCHES:
        mc = normalise(kp1, kp2, matches, m, H, W)
        idx = draws(seed, np.arange(max_hyp), m, defects)
        s = np.sort(idx, 1)
        void = (s[:, 1:] == s[:, :-1]).any(1)
        ok, hs = solve8(rows(mc[idx]).reshape(max_hyp, 8, 9))
        ok &= ~void
        for k0 in range(0, max_hyp, 256):                       # (blocks bound the [K,m] planes)
            k1 = min(k0 + 256, max_hyp)
            scores[k0:k1] = np.where(ok[k0:k1], inliers(hs[k0:k1], mc, H, W, thr, defects).sum(1), -1)
        if ok.any():
            winner = int(np.argmax(scores))                     # the highest score, ties to the lowest k
            have, h = True, hs[winner]
            inl = inliers(h, mc, H, W, thr, defects)[0]
            for _ in range(2):
                sel = np.ones(m, bool) if "refit_all_matches" in defects else inl
                good, h2 = solve8(normal_equations(mc, sel)[None])
                if good[0]:
                    h = h2[0]
                inl = inliers(h, mc, H, W, thr, defects)[0]
            mask[:m] = inl
            count = int(inl.sum())
    Hf, motion, fin = to_pixels(h, H, W, defects)
    valid = have and fin and count >= min_inliers
    if not valid:
        Hf, motion = np.eye(3, dtype=np.float32), np.zeros((4, 2), np.float32)
    info = np.array([valid, n1, n2, m, winner, count, 0, 0], np.int32)
    return (motion, Hf, info, mask, scores) if return_scores else (motion, Hf, info, mask)


def homography(img1, img2, max_hyp=2048, thr=3.0, min_inliers=12, seed=1, defects=NONE):
    """img1, img2 fp32 [B,3,H,W] -> dict of batched arrays: motion, H, info, kp1, kp2, box1, box2, desc1, desc2, nn [2,B,N,3], matches,
    count, mask"""
    out = {k: [] for k in ("motion", "H", "info", "kp1", "kp2", "box1", "box2", "desc1", "desc2", "nn", "matches", "count", "mask")}
    for a, b in zip(np.asarray(img1), np.asarray(img2)):
        H, W = a.shape[1:]
        kp1, box1 = detect(a, defects)
        kp2, box2 = detect(b, defects)
        d1, d2 = describe(box1, kp1, defects), describe(box2, kp2, defects)
        nn, matches, m = match(kp1, d1, kp2, d2, defects)
        motion, Hf, info, mask = ransac(kp1, kp2, matches, m, H, W, max_hyp, thr, min_inliers, seed, defects)
        for k, v in dict(motion=motion, H=Hf, info=info, kp1=kp1, kp2=kp2, box1=box1, box2=box2, desc1=d1, desc2=d2, nn=nn, matches=matches, count=np.int32(m),
                         mask=mask).items():
            out[k].append(v)
    res = {k: np.stack(v) for k, v in out.items()}
    res["nn"] = res["nn"].transpose(1, 0, 2, 3)
    return res


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------
def scene(h, w, seed):
    """band-limited noise plus rectangles, float64 [h,w] in 0..255"""
    rng = np.random.default_rng(seed)
    s = sum(ndi.gaussian_filter(rng.random((h, w)), sg) * wt for sg, wt in ((1.5, 1.0), (4, 2.0), (12, 4.0)))
    s = (s - s.min()) / (s.max() - s.min())
    for _ in range(max(8, h * w // 11000)):
        y, x = rng.integers(0, h - 40), rng.integers(0, w - 40)
        hh, ww = rng.integers(8, 40, 2)
        s[y:y + hh, x:x + ww] = s[y:y + hh, x:x + ww] * 0.5 + rng.random() * 0.5
    return s * 255.0


def resample(img, Hm, h, w):
    """out(p) = img(Hm p), bilinear, 0 outside; img float64 [H,W]"""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    d = Hm[2, 0] * xs + Hm[2, 1] * ys + Hm[2, 2]
    u, v = (Hm[0, 0] * xs + Hm[0, 1] * ys + Hm[0, 2]) / d, (Hm[1, 0] * xs + Hm[1, 1] * ys + Hm[1, 2]) / d
    return ndi.map_coordinates(img, [v, u], order=1, cval=0.0)


def homography_matrix(h, w, tx, ty, rot, px, py, sc=1.0):
    """about the image centre: rotation by `rot` degrees and scale `sc`, a shift and a perspective row"""
    c, s = np.cos(np.radians(rot)) * sc, np.sin(np.radians(rot)) * sc
    C = np.array([[1, 0, -w / 2], [0, 1, -h / 2], [0, 0, 1.]])
    return np.linalg.inv(C) @ np.array([[c, -s, tx], [s, c, ty], [px, py, 1]]) @ C


# the five motions of the accuracy test, at 512x512: shift up to 150 px, rotation up to 15 degrees, scale up to 1.08, perspective up to 2e-4
MOTIONS = ((80, 10, 0, 0, 0), (120, -30, 3, 1e-4, -5e-5), (60, 40, 8, 2e-4, 1e-4), (150, 0, -5, 1e-4, 0, 1.08), (100, 20, 15, 0, 0))


def pair(h, w, motion, seed, gain=0.85, bias=10.0, sigma=3.0):
    """-> (img1, img2 fp32 [1,3,h,w], Hgt): both cut from one procedural scene, image 2 through the known homography, with gain, bias and
    noise; Hgt maps image-1 pixels onto image-2 pixels"""
    pad = int(0.3 * max(h, w)) + 8
    big = scene(h + 2 * pad, w + 2 * pad, seed)
    T = np.array([[1, 0, pad], [0, 1, pad], [0, 0, 1.]])
    Ht = homography_matrix(h, w, *motion)
    im1 = resample(big, T, h, w)
    im2 = resample(big, T @ Ht, h, w)                          # im2(p) = scene(T Ht p), im1(p) = scene(T p): p1 = Ht p2
    rng = np.random.default_rng(seed + 1000)
    im2 = im2 * gain + bias + rng.normal(0, sigma, im2.shape)
    Hgt = np.linalg.inv(Ht)
    rgb = lambda g: np.clip(np.stack([g, g * 0.9 + 5, g * 1.05 - 3]), 0, 255).astype(np.float32)[None]      # noqa: E731
    return rgb(im1), rgb(im2), Hgt / Hgt[2, 2]


def corner_error(Hf, Hgt, h, w):
    """the largest distance between the images of the four corners under the two matrices"""
    c = np.array([[0, 0, 1], [w, 0, 1], [0, h, 1], [w, h, 1]], np.float64).T
    a, b = np.asarray(Hf, np.float64) @ c, Hgt @ c
    return float(np.hypot(a[0] / a[2] - b[0] / b[2], a[1] / a[2] - b[1] / b[2]).max())


# ---- planted inputs of the tests -------------------------------------------------------------------------------------------------------------
def small_pair(h, w, seed=5, motion=(6, -4, 1.0, 2e-5, -1e-5)):
    """a pair with a large overlap for the small canvases of the tests"""
    return pair(h, w, motion, seed)[:2]


def degenerate(name, h=96, w=128):
    """-> (img1, img2) fp32 [1,3,h,w]: "constant" (no keypoint), "identical", "unrelated" (two scenes: fewer than 8 matches), "checker"
    (equal responses and equal distances everywhere: the tie rules decide), "nonfinite" (NaN, +-Inf and out-of-range pixels planted)"""
    a, b = small_pair(h, w)
    if name == "constant":
        return np.full_like(a, 77.0), np.full_like(b, 77.0)
    if name == "identical":
        return a, a.copy()
    if name == "unrelated":
        return a, small_pair(h, w, seed=99)[0][:, :, ::-1, ::-1].copy()
    if name == "checker":
        yy, xx = np.mgrid[:h, :w]
        c = (((yy // 8) + (xx // 8)) % 2 * 200.0 + 20.0).astype(np.float32)
        img = np.stack([c, c, c])[None]
        return img, np.roll(img, 8, 3).copy()
    if name == "nonfinite":
        rng = np.random.default_rng(11)
        a, b = a.copy(), b.copy()
        for img in (a, b):
            flat = img.reshape(-1)
            idx = rng.choice(flat.size, 400, replace=False)
            flat[idx[:100]] = np.nan
            flat[idx[100:200]] = np.inf
            flat[idx[200:300]] = -np.inf
            flat[idx[300:350]] = -300.5
            flat[idx[350:]] = 1e9
        return a, b
    raise KeyError(name)


DEGENERATE = ("constant", "identical", "unrelated", "checker", "nonfinite")


def planted_matches(name, H=96, W=128):
    """-> (kp1, kp2 int32 [N,2], matches int32 [N,2], m): "m8" (eight points under a homography: most hypotheses repeat an index), "line" (twelve
    points on one line: every system is singular), "few" (seven matches), "outliers" (40 under a homography, 14 of them displaced)"""
    N = slots(H, W)
    rng = np.random.default_rng(21)
    Hm = homography_matrix(H, W, 5, -3, 2.0, 1e-4, -5e-5)
    n = dict(m8=8, line=12, few=7, outliers=40)[name]
    if name == "line":
        p = np.stack([np.arange(n) * 7 + 20, np.full(n, 50)], 1)                # y = 50: a horizontal line
    else:
        p = np.stack([rng.choice(np.arange(16, W - 16), n, replace=False), rng.choice(np.arange(16, H - 16), n, replace=False)], 1)
    q = np.c_[p, np.ones(n)] @ Hm.T
    q = np.rint(q[:, :2] / q[:, 2:]).astype(np.int64)
    if name == "outliers":
        q[:40:3] += rng.integers(8, 20, (14, 2))                                # (14 of them displaced by 8..19 px)
    q = np.clip(q, 0, [W - 1, H - 1])
    kp1, kp2 = np.full((N, 2), -1, np.int32), np.full((N, 2), -1, np.int32)
    s1, s2 = np.sort(rng.choice(N, n, replace=False)), rng.choice(N, n, replace=False)
    kp1[s1], kp2[s2] = p, q
    matches = np.full((N, 2), -1, np.int32)
    matches[:n] = np.stack([s1, s2], 1)
    return kp1, kp2, matches, n


PLANTED = ("m8", "line", "few", "outliers")
