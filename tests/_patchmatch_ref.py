"""CPU restatement of csrc/patchmatch.hip (README.md, "patchmatch_inpainter"): exemplar hole filling, PatchMatch (Barnes et al. 2009) inside a
coarse-to-fine vote / search loop (Wexler et al. 2007), all integers, vectorised numpy.  The contract is this project's own: it is pinned
against no library.  `patchmatch` is what `ops.inpaint_patchmatch` must equal bit for bit: the image, info and the level-0 NNF / SAD planes.
`defects` plants one of DEFECTS, for tests/test_patchmatch_cpu.py: each of them must break an assertion there."""
import numpy as np

PATCH, HALF = 7, 3
MIN_SIDE, MAX_SIDE, MAX_LEVELS, AUTO_MIN_SIDE, MAX_ITERS = 15, 4096, 8, 32, 64
INIT_IT = 255                                   # the "iteration" of the initialisation draw
NONE = frozenset()
DEFECTS = ("replace_on_equal", "propagate_without_delta", "in_place_update", "vote_non_interior", "truncate", "all_children", "hash_without_iteration",
           "sad_two_channels", "sources_touch_border")
OY, OX = [a.ravel() for a in np.mgrid[-HALF:HALF + 1, -HALF:HALF + 1]]
M32 = np.uint64(0xFFFFFFFF)
BIG = 1 << 40


def fmix32(x):
    """murmur3's 32-bit finaliser"""
    x = np.asarray(x, np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & M32
    return x ^ (x >> np.uint64(16))


def pm_hash(seed, level, it, k, idx, defects=NONE):
    """fmix32(fmix32(seed ^ fmix32(level * 65536 + it * 256 + k)) ^ idx), idx the row-major pixel index on the level"""
    if "hash_without_iteration" in defects:
        it = 0
    return fmix32(fmix32(np.uint64(int(seed) & 0xFFFFFFFF) ^ fmix32(np.uint64(level * 65536 + it * 256 + k))) ^ np.asarray(idx, np.uint64))


def level_count(H, W, levels=None):
    """auto: a level more while both sides of the next one are >= 32; explicit: cut where the next level would have a side < 15; at most 8"""
    floor, want = (AUTO_MIN_SIDE, MAX_LEVELS) if levels is None else (MIN_SIDE, levels)
    n = 1
    while n < want and min((H + 1) // 2, (W + 1) // 2) >= floor:
        H, W, n = (H + 1) // 2, (W + 1) // 2, n + 1
    return n


def _mean(S, n, defects):
    n = np.maximum(n, 1)
    return S // n if "truncate" in defects else (2 * S + n) // (2 * n)


def down(img, hole, defects=NONE):
    """n -> ceil(n / 2), children at min(2i + a, n - 1): hole iff any child is one, colour the half-up mean of the known children (0: none)"""
    H, W = hole.shape
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    ys = np.minimum(2 * np.arange(h2)[:, None, None, None] + np.arange(2)[None, None, :, None], H - 1)
    xs = np.minimum(2 * np.arange(w2)[None, :, None, None] + np.arange(2)[None, None, None, :], W - 1)
    ys, xs = np.broadcast_arrays(ys, xs)
    known = ~hole[ys, xs]
    n = known.sum((2, 3))
    S = (img[ys, xs].astype(np.int64) * known[..., None]).sum((2, 3))
    colour = _mean(S, n[..., None], defects) * (n > 0)[..., None]
    h = hole[ys, xs]
    return colour.astype(np.uint8), (h.all((2, 3)) if "all_children" in defects else h.any((2, 3)))


def classify(hole, defects=NONE):
    """(source, target) planes: interior centres whose 7x7 box holds no / at least one hole pixel"""
    H, W = hole.shape
    pad = np.pad(hole.astype(np.int64), HALF)
    c = np.zeros((H, W), np.int64)
    for dy in range(PATCH):
        for dx in range(PATCH):
            c += pad[dy:dy + H, dx:dx + W]
    inter = np.zeros((H, W), bool)
    inter[HALF:H - HALF, HALF:W - HALF] = True
    if "sources_touch_border" in defects:
        return (c == 0), inter & (c > 0)
    return inter & (c == 0), inter & (c > 0)


def _at(img, y, x):
    H, W = img.shape[:2]
    return img[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)]        # (the clip only matters under a planted defect)


def sad(img, p, q, defects=NONE):
    """D(p, q): sum over the 49 offsets and 3 channels of |a - b|"""
    a = _at(img, p[:, 0, None] + OY, p[:, 1, None] + OX).astype(np.int64)
    b = _at(img, q[:, 0, None] + OY, q[:, 1, None] + OX).astype(np.int64)
    d = np.abs(a - b)
    if "sad_two_channels" in defects:
        d = d[..., :2]
    return d.sum((1, 2))


def vote(img, hole, tgt, nnf, defects=NONE):
    """every hole pixel x <- half-up mean over the interior target centres p with x in patch(p) of img at NNF(p) + (x - p)"""
    out = img.copy()
    ys, xs = np.nonzero(hole)
    S = np.zeros((len(ys), 3), np.int64)
    n = np.zeros(len(ys), np.int64)
    H, W = hole.shape
    for oy, ox in zip(OY, OX):
        py, px = ys - oy, xs - ox
        ok = (py >= 0) & (py < H) & (px >= 0) & (px < W)
        if "vote_non_interior" in defects:                           # a centre outside the interior votes with the nearest interior one's match
            pyc, pxc = np.clip(py, HALF, H - 1 - HALF), np.clip(px, HALF, W - 1 - HALF)
        else:
            pyc, pxc = np.clip(py, 0, H - 1), np.clip(px, 0, W - 1)
        ok &= tgt[pyc, pxc]
        q = nnf[pyc, pxc]
        S += _at(img, q[:, 0] + oy, q[:, 1] + ox).astype(np.int64) * ok[:, None]
        n += ok
    assert (n > 0).all()
    out[ys, xs] = _mean(S, n[:, None], defects)
    return out


def search(img, src, tgt, nnf, seed, level, it, defects=NONE):
    """one Jacobi sweep -> (NNF_{t+1}, cost plane): the own match recomputed, the eight propagation candidates, the random trials"""
    H, W = tgt.shape
    t = np.argwhere(tgt)
    idx = t[:, 0] * W + t[:, 1]
    read = nnf.copy() if "in_place_update" in defects else nnf
    best = nnf[t[:, 0], t[:, 1]].copy()
    bc = sad(img, t, best, defects)

    def trial(q, ok):
        ok = ok & (q[:, 0] >= 0) & (q[:, 0] < H) & (q[:, 1] >= 0) & (q[:, 1] < W)
        qc = np.clip(q, 0, [H - 1, W - 1])
        ok &= src[qc[:, 0], qc[:, 1]]
        c = np.where(ok, sad(img, t, qc, defects), BIG)
        w = (c <= bc) & ok if "replace_on_equal" in defects else c < bc
        best[w] = qc[w]
        bc[w] = c[w]
        if "in_place_update" in defects:
            read[t[:, 0], t[:, 1]] = best
    for s in (1, 1 << (1 + it % 3)):
        for dy, dx in ((0, -s), (0, s), (-s, 0), (s, 0)):
            n = t + [dy, dx]
            ok = (n[:, 0] >= 0) & (n[:, 0] < H) & (n[:, 1] >= 0) & (n[:, 1] < W)
            nc = np.clip(n, 0, [H - 1, W - 1])
            ok &= tgt[nc[:, 0], nc[:, 1]]
            trial(read[nc[:, 0], nc[:, 1]] - (0 if "propagate_without_delta" in defects else np.array([dy, dx])), ok)
    R, k = max(H, W), 0
    while R >= 1:
        r = pm_hash(seed, level, it, k, idx, defects)
        ry = (r & np.uint64(0xFFFF)).astype(np.int64) % (2 * R + 1) - R
        rx = (r >> np.uint64(16)).astype(np.int64) % (2 * R + 1) - R
        trial(best + np.stack([ry, rx], 1), np.ones(len(t), bool))
        R, k = R // 2, k + 1
    out = nnf.copy()
    out[t[:, 0], t[:, 1]] = best
    cost = np.full((H, W), -1, np.int64)
    cost[t[:, 0], t[:, 1]] = bc
    return out, cost


def init_nnf(src, tgt, seed, level, coarse=None, defects=NONE):
    """NNF of every target: the coarse match doubled when the coarse centre is a target and the result a source, else a draw from the source list"""
    H, W = tgt.shape
    srclist = np.argwhere(src)                                       # row-major: the order is part of the contract
    r = pm_hash(seed, level, INIT_IT, 0, np.arange(H * W), defects).astype(np.int64) % len(srclist)
    nnf = srclist[r].reshape(H, W, 2)
    if coarse is not None:
        nnf_c, tgt_c = coarse
        yy, xx = np.mgrid[0:H, 0:W]
        Hc, Wc = tgt_c.shape
        cy, cx = np.clip(yy >> 1, HALF, Hc - 1 - HALF), np.clip(xx >> 1, HALF, Wc - 1 - HALF)
        up = np.clip(2 * nnf_c[cy, cx] + np.stack([yy & 1, xx & 1], 2), HALF, [H - 1 - HALF, W - 1 - HALF])
        ok = tgt_c[cy, cx] & src[up[..., 0], up[..., 1]]
        nnf = np.where(ok[..., None], up, nnf)
    return np.where(tgt[..., None], nnf, -1)


def pyramid(img, hole, levels=None, defects=NONE):
    pyr = [(img, hole)]
    for _ in range(level_count(*hole.shape, levels) - 1):
        pyr.append(down(*pyr[-1], defects))
    return pyr


def patchmatch(img, mask, levels=None, iters=4, seed=1, defects=NONE, trace=None):
    """img uint8 [H,W,3], mask [H,W] (nonzero = fill) -> (out uint8 [H,W,3], info [valid, start level, level-0 sources, level-0 targets],
    nnf int32 [H,W,2] (-1: no target), sad int32 [H,W] (-1: no target, or no sweep ran)).  `trace`: a list that receives
    (level, stage, image, nnf) after every vote."""
    hole = np.asarray(mask) != 0
    H, W = hole.shape
    assert MIN_SIDE <= min(H, W) and max(H, W) <= MAX_SIDE and 0 <= iters <= MAX_ITERS and img.shape == (H, W, 3) and img.dtype == np.uint8
    pyr = pyramid(img, hole, levels, defects)
    planes = [classify(h, defects) for _, h in pyr]
    nsrc, ntgt = int(planes[0][0].sum()), int(planes[0][1].sum())
    no_nnf, no_sad = np.full((H, W, 2), -1, np.int32), np.full((H, W), -1, np.int32)
    if nsrc == 0 or ntgt == 0:
        return img.copy(), [0, 0, nsrc, ntgt], no_nnf, no_sad
    start = max(l for l, (s, _) in enumerate(planes) if s.any())
    coarse, cost = None, no_sad
    for l in range(start, -1, -1):
        (orig, hole_l), (src, tgt) = pyr[l], planes[l]
        nnf = init_nnf(src, tgt, seed, l, coarse, defects)
        cur = vote(orig, hole_l, tgt, nnf, defects)
        if trace is not None:
            trace.append((l, "init", cur, nnf))
        for it in range(iters):
            nnf, cost = search(cur, src, tgt, nnf, seed, l, it, defects)
            cur = vote(cur, hole_l, tgt, nnf, defects)
            if trace is not None:
                trace.append((l, it, cur, nnf))
        coarse = (nnf, tgt)
    return cur, [1, start, nsrc, ntgt], nnf.astype(np.int32), cost.astype(np.int32)


# ---- the scenes and masks of the tests ----------------------------------------------------------------------------------------------------
def scene(name, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    if name == "stripes":
        sc = np.stack([128 + 100 * np.sin(2 * np.pi * xx / 8), 128 + 100 * np.sin(2 * np.pi * (xx + yy) / 8), 128 + 60 * np.cos(2 * np.pi * yy / 8)], 2)
    elif name == "checker":
        sc = np.stack([((xx // 4 + yy // 4) % 2) * 200 + 20] * 3, 2)
    elif name == "ramp":
        sc = np.stack([128 + 100 * np.sin(2 * np.pi * xx / 8), 128 + 100 * np.sin(2 * np.pi * (xx + yy) / 8), 60 + 2 * xx + yy], 2)
    else:
        sc = np.full((H, W, 3), 77.0)
    return np.clip(sc, 0, 255).astype(np.uint8)


def masks(H, W):
    """corner, border, frame, 2 % noise, thin known strip (8 wide), all-hole, no-hole"""
    yy, xx = np.mgrid[0:H, 0:W]
    return {"corner": (yy < H // 3) & (xx < W // 3), "border": xx >= W - 12, "frame": (yy < 5) | (yy >= H - 5) | (xx < 5) | (xx >= W - 5),
            "noise": np.random.default_rng(0).random((H, W)) < 0.02, "thin_known": ~((xx >= 4) & (xx < 12)), "all": np.ones((H, W), bool),
            "none": np.zeros((H, W), bool)}
