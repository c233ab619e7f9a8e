"""CPU restatement of csrc/features_ms.hip (README.md, "feature_align_ms"): a 5/4 luma pyramid, Harris corners on every level (border 20), a
32-bin orientation from the first moments over a disc of radius 15, the BRIEF-256 pattern of feature_align steered by the bin, then
feature_align's own matching over the slots of all levels and its RANSAC on level-0 coordinates.  Everything is integer up to the match
list and fp64 from there on.  The stages feature_align already has are taken from tests/_features_ref.py as they are.  The contract is this
project's own: it is pinned against no library.  `homography` is what `ops.feature_homography_ms` must equal bit for bit.  `defects` plants
one of DEFECTS, for tests/test_features_ms_cpu.py: each of them must break an assertion there."""
import numpy as np

import _features_ref as ref

MAX_LEVELS, BORDER, RADIUS, BINS = 8, 20, 15, 32
QUARTER = (1024, 1004, 946, 851, 724, 569, 392, 200, 0)
NONE = frozenset()
DEFECTS = ("bins_clockwise", "swap_cs", "tie_highest_bin", "shift_truncates", "corner_aligned", "no_half_pixel", "border_16", "box_from_level0")


# ---- levels and slots ------------------------------------------------------------------------------------------------------------------------
def level_sizes(H, W, levels):
    """[(H_l, W_l)]: level l+1 exists iff l+1 < levels and min(4 H_l div 5, 4 W_l div 5) >= 64, and is that size"""
    out = [(H, W)]
    while len(out) < levels and min(4 * out[-1][0] // 5, 4 * out[-1][1] // 5) >= ref.MIN_SIDE:
        out.append((4 * out[-1][0] // 5, 4 * out[-1][1] // 5))
    return out


def slot_starts(H, W, levels):
    """first slot of every level and, last, N"""
    return np.r_[0, np.cumsum([ref.slots(h, w) for h, w in level_sizes(H, W, levels)])].astype(np.int64)


def slots(H, W, levels):
    return int(slot_starts(H, W, levels)[-1])


def slot_levels(H, W, levels):
    """int64 [N]: the level of every slot"""
    s = slot_starts(H, W, levels)
    return np.searchsorted(s, np.arange(s[-1]), side="right") - 1


# ---- pyramid ---------------------------------------------------------------------------------------------------------------------------------
def downsample(Y, defects=NONE):
    """pixel (i, j) samples Y at (160 (2j + 1) - 128, 160 (2i + 1) - 128) / 256, bilinear with 8-bit weights, the second tap clamped"""
    H, W = Y.shape
    h, w = 4 * H // 5, 4 * W // 5
    sy, sx = 160 * (2 * np.arange(h) + 1) - 128, 160 * (2 * np.arange(w) + 1) - 128
    if "corner_aligned" in defects:
        sy, sx = 320 * np.arange(h), 320 * np.arange(w)
    y0, fy, x0, fx = (sy >> 8)[:, None], (sy & 255)[:, None], (sx >> 8)[None, :], (sx & 255)[None, :]
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    return ((256 - fx) * (256 - fy) * Y[y0, x0] + fx * (256 - fy) * Y[y0, x1] + (256 - fx) * fy * Y[y1, x0] + fx * fy * Y[y1, x1] + (1 << 15)) >> 16


def pyramid(img, levels, defects=NONE):
    """fp32 [3,H,W] -> [Y_l int64 [H_l,W_l]]"""
    out = [ref.luma(img)]
    for _ in level_sizes(*out[0].shape, levels)[1:]:
        out.append(downsample(out[-1], defects))
    return out


# ---- corners and orientation -----------------------------------------------------------------------------------------------------------------
def candidates(R, border):
    """ref.candidates with the border as an argument"""
    H, W = R.shape
    ok = R > 0
    ok[:border] = ok[H - border:] = False
    ok[:, :border] = ok[:, W - border:] = False
    p = np.pad(R, 1, constant_values=np.iinfo(np.int64).max)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                q = p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
                ok &= (R > q) if dy < 0 or (dy == 0 and dx < 0) else (R >= q)
    return ok


def cs_table():
    """int64 [32,2] = (c_b, s_b): the literal first quarter with s_b = c_{8-b}, the other quadrants by (c, s) -> (-s, c)"""
    t = np.zeros((BINS, 2), np.int64)
    for b in range(BINS):
        c, s = QUARTER[b % 8], QUARTER[8 - b % 8]
        for _ in range(b // 8):
            c, s = -s, c
        t[b] = c, s
    return t


def disc():
    """int64 [709,2] = (dx, dy) with dx^2 + dy^2 <= 225"""
    d = np.arange(-RADIUS, RADIUS + 1)
    dy, dx = np.meshgrid(d, d, indexing="ij")
    keep = dx * dx + dy * dy <= RADIUS * RADIUS
    return np.stack([dx[keep], dy[keep]], 1)


def moments(Y, kp):
    """(m10, m01) int64 [N] = sum of dx Y(x + dx, y + dy), of dy Y(..) over the disc; 0 for an unused slot"""
    d = disc()
    valid = kp[:, 0] >= 0
    x, y = np.where(valid, kp[:, 0], RADIUS).astype(np.int64), np.where(valid, kp[:, 1], RADIUS).astype(np.int64)
    v = Y[y[:, None] + d[None, :, 1], x[:, None] + d[None, :, 0]]
    return (v * d[None, :, 0]).sum(1) * valid, (v * d[None, :, 1]).sum(1) * valid


def bins_of(m10, m01, defects=NONE):
    """uint8 [N]: the b that maximises m10 c_b + m01 s_b, ties to the lowest b (a flat patch: bin 0)"""
    t = cs_table()
    s = -t[:, 1] if "bins_clockwise" in defects else t[:, 1]
    v = np.asarray(m10, np.int64)[:, None] * t[None, :, 0] + np.asarray(m01, np.int64)[:, None] * s[None, :]
    if "tie_highest_bin" in defects:
        return (BINS - 1 - np.argmax(v[:, ::-1], 1)).astype(np.uint8)
    return np.argmax(v, 1).astype(np.uint8)


def detect_level(Y, oriented=True, defects=NONE):
    """-> (kp int32 [N_l,2] in the level's pixels, bins uint8 [N_l], box int64 [H_l,W_l])"""
    R = ref.harris(Y)
    kp = ref.select(R, candidates(R, 16 if "border_16" in defects else BORDER))
    bins = bins_of(*moments(np.pad(Y, RADIUS), np.where(kp >= 0, kp + RADIUS, -1)), defects) if oriented else np.zeros(len(kp), np.uint8)
    return kp, bins * (kp[:, 0] >= 0).astype(np.uint8), ref.window_sum(Y, 2)


# ---- descriptor ------------------------------------------------------------------------------------------------------------------------------
def steered(bins, defects=NONE):
    """int64 [N,256,4]: every pattern offset (px, py) as ((px c - py s + 512) >> 10, (px s + py c + 512) >> 10), arithmetic shifts"""
    pat = ref.brief_pattern().astype(np.int64)
    t = cs_table()[np.asarray(bins, np.int64)]
    c, s = (t[:, 1, None], t[:, 0, None]) if "swap_cs" in defects else (t[:, 0, None], t[:, 1, None])
    half = 0 if "shift_truncates" in defects else 512
    out = np.empty((len(t), 256, 4), np.int64)
    for k in (0, 2):
        px, py = pat[None, :, k], pat[None, :, k + 1]
        out[:, :, k], out[:, :, k + 1] = (px * c - py * s + half) >> 10, (px * s + py * c + half) >> 10
    return out


def describe_level(box, kp, bins, defects=NONE):
    """uint32 [N_l,8]: bit k = S(p + a_k) < S(p + b_k) at the steered offsets; zero for an unused slot"""
    o = steered(bins, defects)
    valid = kp[:, 0] >= 0
    x, y = np.where(valid, kp[:, 0], BORDER).astype(np.int64)[:, None], np.where(valid, kp[:, 1], BORDER).astype(np.int64)[:, None]
    bits = box[y + o[:, :, 1], x + o[:, :, 0]] < box[y + o[:, :, 3], x + o[:, :, 2]]
    return ref.pack_bits(bits & valid[:, None])


def features(img, levels=6, oriented=True, defects=NONE):
    """fp32 [3,H,W] -> dict: pyr [Y_l], box [S_l], kp int32 [N,2], bins uint8 [N], desc uint32 [N,8], the slots of all levels concatenated"""
    pyr = pyramid(img, levels, defects)
    per = [detect_level(Y, oriented, defects) for Y in pyr]
    box = [p[2] for p in per]
    desc = [describe_level(box[0][:Y.shape[0], :Y.shape[1]] if "box_from_level0" in defects else b, kp, bins, defects) for Y, (kp, bins, b) in zip(pyr, per)]
    return dict(pyr=pyr, box=box, kp=np.concatenate([p[0] for p in per]), bins=np.concatenate([p[1] for p in per]), desc=np.concatenate(desc))


# ---- level-0 coordinates and RANSAC --------------------------------------------------------------------------------------------------------------
def level0(kp, H, W, levels, defects=NONE):
    """fp64 [N,2]: a slot of level l at (x, y) stands at ((2 x + 1) 5^l) / (2 4^l) - 1/2 (exact in fp64); (-1, -1) for an unused slot"""
    l = slot_levels(H, W, levels)[:, None]
    v = kp.astype(np.int64)
    if "no_half_pixel" in defects:
        out = (v * 5 ** l).astype(np.float64) / (4 ** l).astype(np.float64)
    else:
        out = ((2 * v + 1) * 5 ** l).astype(np.float64) / (2 * 4 ** l).astype(np.float64) - 0.5
    return np.where(kp >= 0, out, -1.0)


def ransac(kp1, kp2, matches, m, H, W, levels, max_hyp=2048, thr=3.0, min_inliers=12, seed=1, defects=NONE):
    """ref.ransac on level-0 coordinates -> (motion fp32 [4,2], H fp32 [3,3], info int32 [8], mask uint8 [N], xy fp64 [2,N,2])"""
    N = len(kp1)
    xy = np.stack([level0(kp1, H, W, levels, defects), level0(kp2, H, W, levels, defects)])
    n1, n2 = int((kp1[:, 0] >= 0).sum()), int((kp2[:, 0] >= 0).sum())
    mask = np.zeros(N, np.uint8)
    winner, have, count, h = -1, False, 0, np.zeros(8)
    if m >= ref.MIN_MATCHES:
        sx, sy = np.float64(0.5 * W), np.float64(0.5 * H)
        a, b = xy[0][matches[:m, 0]], xy[1][matches[:m, 1]]
        mc = np.stack([(a[:, 0] - sx) / sx, (a[:, 1] - sy) / sy, (b[:, 0] - sx) / sx, (b[:, 1] - sy) / sy], 1)
        idx = ref.draws(seed, np.arange(max_hyp), m)
        s = np.sort(idx, 1)
        ok, hs = ref.solve8(ref.rows(mc[idx]).reshape(max_hyp, 8, 9))
        ok &= ~(s[:, 1:] == s[:, :-1]).any(1)
        scores = np.full(max_hyp, -1, np.int64)
        for k0 in range(0, max_hyp, 256):                       # (blocks bound the [K,m] planes)
            k1 = min(k0 + 256, max_hyp)
            scores[k0:k1] = np.where(ok[k0:k1], ref.inliers(hs[k0:k1], mc, H, W, thr).sum(1), -1)
        if ok.any():
            winner = int(np.argmax(scores))                     # the highest score, ties to the lowest k
            have, h = True, hs[winner]
            inl = ref.inliers(h, mc, H, W, thr)[0]
            for _ in range(2):
                good, h2 = ref.solve8(ref.normal_equations(mc, inl)[None])
                if good[0]:
                    h = h2[0]
                inl = ref.inliers(h, mc, H, W, thr)[0]
            mask[:m] = inl
            count = int(inl.sum())
    Hf, motion, fin = ref.to_pixels(h, H, W)
    valid = have and fin and count >= min_inliers
    if not valid:
        Hf, motion = np.eye(3, dtype=np.float32), np.zeros((4, 2), np.float32)
    return motion, Hf, np.array([valid, n1, n2, m, winner, count, 0, 0], np.int32), mask, xy


def homography(img1, img2, levels=6, oriented=True, max_hyp=2048, thr=3.0, min_inliers=12, seed=1, defects=NONE):
    """img1, img2 fp32 [B,3,H,W] -> dict of batched arrays: motion, H, info, kp1, kp2, bins1, bins2, desc1, desc2, nn [2,B,N,3], matches, count,
    mask, xy [2,B,N,2], and pyr1, pyr2, box1, box2: lists of [B,H_l,W_l]"""
    keys = ("motion", "H", "info", "kp1", "kp2", "bins1", "bins2", "desc1", "desc2", "nn", "matches", "count", "mask", "xy")
    out = {k: [] for k in keys}
    planes = {k: [] for k in ("pyr1", "pyr2", "box1", "box2")}
    for a, b in zip(np.asarray(img1), np.asarray(img2)):
        H, W = a.shape[1:]
        f1, f2 = features(a, levels, oriented, defects), features(b, levels, oriented, defects)
        nn, matches, m = ref.match(f1["kp"], f1["desc"], f2["kp"], f2["desc"])
        motion, Hf, info, mask, xy = ransac(f1["kp"], f2["kp"], matches, m, H, W, levels, max_hyp, thr, min_inliers, seed, defects)
        for k, v in dict(motion=motion, H=Hf, info=info, kp1=f1["kp"], kp2=f2["kp"], bins1=f1["bins"], bins2=f2["bins"], desc1=f1["desc"], desc2=f2["desc"], nn=nn,
                         matches=matches, count=np.int32(m), mask=mask, xy=xy).items():
            out[k].append(v)
        for k, v in dict(pyr1=f1["pyr"], pyr2=f2["pyr"], box1=f1["box"], box2=f2["box"]).items():
            planes[k].append(v)
    res = {k: np.stack(v) for k, v in out.items()}
    res["nn"], res["xy"] = res["nn"].transpose(1, 0, 2, 3), res["xy"].transpose(1, 0, 2, 3)
    for k, v in planes.items():
        res[k] = [np.stack(lv) for lv in zip(*v)]
    return res


def pack_levels(planes):
    """[[B,H_l,W_l]] -> the flat buffer of the C entries: level l's planes behind those of the levels before it"""
    return np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in planes])
