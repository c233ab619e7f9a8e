"""CPU restatement of inner_crop (csrc/crop.hip; README.md, inner_crop), numpy and Python integers.  This project's own contract, pinned
against no library; brute force over all rectangles (`rect_brute`) is the authority the rule is tested against.

Operands: mask1 fp32 [1,H,W] or [3,H,W] (channel 0 is used), mask2 optional, sides 1..4096.  m_i = mask_i > 0.5 (NaN, -Inf and 0.5 are
unset, +Inf is set: `multiband_blend`'s rule); U = m1 or m2, U = m1 without mask2.

A rectangle (top, left, h, w) with h, w >= 1 is inside when every pixel of it is in U.  The result is the inside rectangle that is best in
this order: largest area h w, then lowest top, then lowest left, then smallest h.  info = (valid, top, left, h, w, area), all zeros when U is
empty.

r(y, x) = the number of consecutive U pixels in column x ending at row y going up (0 outside U).  For every (y, x) with v = r(y, x) > 0: L =
the nearest column left of x in row y with r < v, strictly (-1: none), R the same to the right (W: none); the candidate is (y - v + 1, L + 1,
v, R - L - 1).  Every inside rectangle that cannot grow in any direction is a candidate at its bottom row, so the best candidate is the best
rectangle.

`defects`: a set of names from DEFECTS, each a planted mistake that tests/test_crop_cpu.py must notice."""
import numpy as np

NONE = frozenset()
DEFECTS = ("l_le", "r_le", "no_carry", "carry_off_by_one", "ties_highest_top", "ties_largest_h", "bmin_63", "mask_ge", "area_bits")
MAX_SIDE = 4096
SEGS = 16                                # row segments of the run pass
BLOCK = 64                               # positions per block of the row search
SEARCH_BOUND = 1 + 63 + 63 + 63          # LDS reads per side: own minimum, own block, block minima, the block that holds the answer


def union(k1, k2=None, defects=NONE):
    """bool [H,W] from masks [C,H,W] (channel 0)"""
    with np.errstate(invalid="ignore"):
        bit = (lambda k: k[0] >= np.float32(0.5)) if "mask_ge" in defects else (lambda k: k[0] > np.float32(0.5))
        return bit(k1) | bit(k2) if k2 is not None else bit(k1)


def runs(u, defects=NONE):
    """int16 [H,W], in the kernel's form: SEGS segments of S rows per column; a segment's tail = its set rows since the last unset one; the
    carry into a segment = the tails above it, up to and including the first segment that is not wholly set; then a sweep down"""
    H, W = u.shape
    S = -(-H // SEGS)
    bounds = [(min(s * S, H), min(s * S + S, H)) for s in range(SEGS)]
    tails = np.zeros((SEGS, W), np.int64)
    for s, (y0, y1) in enumerate(bounds):
        t = np.zeros(W, np.int64)
        for y in range(y0, y1):
            t = np.where(u[y], t + 1, 0)
        tails[s] = t
    out = np.zeros((H, W), np.int16)
    for s, (y0, y1) in enumerate(bounds):
        if y0 >= y1:
            continue
        v = np.zeros(W, np.int64)
        open_ = np.ones(W, bool)                                   # no segment that is not wholly set met yet
        for a in range(s - 1, -1, -1):
            v += np.where(open_, tails[a], 0)
            open_ &= tails[a] >= S
        if "no_carry" in defects:
            v[:] = 0
        if "carry_off_by_one" in defects:
            v = np.where(v > 0, v - 1, v)
        for y in range(y0, y1):
            v = np.where(u[y], v + 1, 0)
            out[y] = v
    return out


def lr(row, defects=NONE):
    """L and R of every position of a row of runs (lists; positions with r = 0 included), by a monotonic stack: O(W)"""
    row = [int(v) for v in row]
    W = len(row)
    le_l, le_r = "l_le" in defects, "r_le" in defects
    L, R = [-1] * W, [W] * W
    st = []
    for x in range(W):
        while st and not (row[st[-1]] <= row[x] if le_l else row[st[-1]] < row[x]):
            st.pop()
        L[x] = st[-1] if st else -1
        st.append(x)
    st = []
    for x in range(W - 1, -1, -1):
        while st and not (row[st[-1]] <= row[x] if le_r else row[st[-1]] < row[x]):
            st.pop()
        R[x] = st[-1] if st else W
        st.append(x)
    return L, R


def search_reads(row, defects=NONE):
    """The shipped two-level search replayed: (L, R, reads) with reads [W][2] = LDS reads for the left and for the right side of every
    position with r > 0 (the read of the own block's minimum is shared by the two sides and counted in both).  Per side: the own block is
    scanned only when its minimum is below v; then the block minima outward; then the block whose minimum is below v from its near end,
    without reading its far end (when every other position has failed, the far end is the one below v)."""
    row = [int(v) for v in row]
    W = len(row)
    blocks = -(-W // BLOCK)
    span = BLOCK - 1 if "bmin_63" in defects else BLOCK
    bmin = [min(row[b * BLOCK:min(b * BLOCK + span, W)]) for b in range(blocks)]
    lt_l = (lambda a, v: a <= v) if "l_le" in defects else (lambda a, v: a < v)
    lt_r = (lambda a, v: a <= v) if "r_le" in defects else (lambda a, v: a < v)
    L, R, reads = [-1] * W, [W] * W, [[0, 0] for _ in range(W)]
    for x in range(W):
        v = row[x]
        if v == 0:
            continue
        blk = x // BLOCK
        own = bmin[blk] < v
        # left
        n, ans = 1, None
        if own:
            for k in range(x - 1, blk * BLOCK - 1, -1):
                n += 1
                if lt_l(row[k], v):
                    ans = k
                    break
        if ans is None:
            ans = -1
            for b in range(blk - 1, -1, -1):
                n += 1
                if lt_l(bmin[b], v):
                    k = b * BLOCK + BLOCK - 1
                    while k > b * BLOCK:
                        n += 1
                        if lt_l(row[k], v):
                            break
                        k -= 1
                    ans = k
                    break
        L[x], reads[x][0] = ans, n
        # right
        n, ans = 1, None
        if own:
            for k in range(x + 1, min(blk * BLOCK + BLOCK - 1, W - 1) + 1):
                n += 1
                if lt_r(row[k], v):
                    ans = k
                    break
        if ans is None:
            ans = W
            for b in range(blk + 1, blocks):
                n += 1
                if lt_r(bmin[b], v):
                    last = min(b * BLOCK + BLOCK - 1, W - 1)
                    k = b * BLOCK
                    while k < last:
                        n += 1
                        if lt_r(row[k], v):
                            break
                        k += 1
                    ans = k
                    break
        R[x], reads[x][1] = ans, n
    return L, R, reads


def key(top, left, h, w, defects=NONE):
    """the 64-bit key whose unsigned order is the order of the contract: area (25 bits), 4095 - top, 4095 - left (12 bits each), 8191 - h
    (13 bits)"""
    area = h * w
    if "area_bits" in defects:
        area &= (1 << 24) - 1
    t = top if "ties_highest_top" in defects else 4095 - top
    hh = h if "ties_largest_h" in defects else 8191 - h
    return area << 37 | t << 25 | (4095 - left) << 13 | hh


def decode(k, defects=NONE):
    """info (valid, top, left, h, w, area) of a key; 0 = no candidate"""
    if k == 0:
        return [0] * 6
    area, t, left, hh = k >> 37, k >> 25 & 4095, 4095 - (k >> 13 & 4095), k & 8191
    top = t if "ties_highest_top" in defects else 4095 - t
    h = hh if "ties_largest_h" in defects else 8191 - hh
    return [1, top, left, h, area // h, area]


def rect(u, defects=NONE, r=None):
    """info [6] by the candidate rule on the runs of u (``r``: those runs, when the caller has them)"""
    r = runs(u, defects) if r is None else r
    best = 0
    for y in range(r.shape[0]):
        row = r[y].tolist()
        if not any(row):
            continue
        L, R = lr(row, defects)
        for x, v in enumerate(row):
            if v:
                best = max(best, key(y - v + 1, L[x] + 1, v, R[x] - L[x] - 1, defects))
    return decode(best, defects)


def rect_brute(u):
    """info [6] over all rectangles, compared as tuples in the order of the contract"""
    H, W = u.shape
    sat = np.zeros((H + 1, W + 1), np.int64)
    sat[1:, 1:] = np.cumsum(np.cumsum(u.astype(np.int64), axis=0), axis=1)
    sat = sat.tolist()
    best = None
    for top in range(H):
        for left in range(W):
            for h in range(1, H - top + 1):
                for w in range(1, W - left + 1):
                    if sat[top + h][left + w] - sat[top][left + w] - sat[top + h][left] + sat[top][left] == h * w:
                        cand = (-h * w, top, left, h)
                        if best is None or cand < best:
                            best = cand
    if best is None:
        return [0] * 6
    area, top, left, h = -best[0], best[1], best[2], best[3]
    return [1, top, left, h, area // h, area]
