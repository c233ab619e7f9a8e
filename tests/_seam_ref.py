"""CPU restatement of the seam_dp contract (README.md, seam_dp; csrc/seam.hip) in integer numpy, and the multiband blend with the ownership
of the overlap taken from that seam (the pyramid is `_multiband_ref.pyramid_blend`, unchanged).

``defects``: a set of names from DEFECTS, each of which plants one deviation from the contract (tests/test_seam_cpu.py shows that every one
of them fails an assertion).  Production callers pass none."""
import numpy as np

import _multiband_ref as mb

BIG = 1 << 18
INF = np.int64(1) << 40
VERTICAL, HORIZONTAL = 1, 2
ORIENTATIONS = {"auto": 0, "vertical": VERTICAL, "horizontal": HORIZONTAL}
DEFECTS = ("le_for_lt", "minus_first", "last_argmin", "big_outside_u", "no_plus_1", "luma", "ab_swapped", "side_lt", "round")


def masks(mask1, mask2):
    """mask [C,H,W] (channel 0 > 0.5) -> bool m1, m2 [H,W]"""
    return np.asarray(mask1)[0] > 0.5, np.asarray(mask2)[0] > 0.5


def to_int(img, defects=frozenset()):
    """p = trunc(clamp(x, 0, 255)) as int64 [3,H,W]; NaN -> 0, -Inf -> 0, +Inf -> 255 (`st_u8_trunc`)"""
    x = np.asarray(img, dtype=np.float64)
    x = np.clip(np.where(np.isnan(x), 0, x), 0, 255)
    return (np.floor(x + 0.5) if "round" in defects else np.trunc(x)).astype(np.int64)


def cost(img1, img2, mask1, mask2, defects=frozenset()):
    """e int32 [H,W] (canvas layout)"""
    m1, m2 = masks(mask1, mask2)
    a, b = to_int(img1, defects), to_int(img2, defects)
    if "luma" in defects:
        ya, yb = ((p[0] * 19595 + p[1] * 38470 + p[2] * 7471 + 0x8000) >> 16 for p in (a, b))
        d = np.abs(ya - yb)
    else:
        d = np.abs(a - b).sum(0)
    e = np.where(m1 & m2, d + (0 if "no_plus_1" in defects else 1), BIG)
    e = np.where(m1 | m2, e, BIG if "big_outside_u" in defects else 1)
    return e.astype(np.int32)


def decide(m1, m2, orientation="auto", first="auto", defects=frozenset()):
    """-> valid, orientation (1 vertical / 2 horizontal), first (1 / 2), from exact integer sums (Python ints)"""
    E1, E2 = m1 & ~m2, m2 & ~m1
    H, W = m1.shape
    y, x = np.mgrid[:H, :W]
    N1, N2 = int(E1.sum()), int(E2.sum())
    A = int(x[E1].sum()) * N2 - int(x[E2].sum()) * N1
    B = int(y[E1].sum()) * N2 - int(y[E2].sum()) * N1
    if "ab_swapped" in defects:
        A, B = B, A
    automatic = orientation == "auto" or first == "auto"
    orient = ORIENTATIONS[orientation] or (VERTICAL if abs(A) >= abs(B) else HORIZONTAL)
    fst = first if first != "auto" else (1 if (A if orient == VERTICAL else B) <= 0 else 2)
    valid = bool((m1 & m2).any()) and not (automatic and (N1 == 0 or N2 == 0))
    return int(valid), orient, int(fst)


def dp(e, defects=frozenset()):
    """e [L,n] (one row per line) -> s int32 [L], path cost.  M(0) = e; M(l, k) = e + min over the predecessors k, k - 1, k + 1 inside the
    line in that order with strict <; the end is the lowest index among the minima of the last line."""
    e = np.asarray(e, dtype=np.int64)
    L, n = e.shape
    less = (lambda a, b: a <= b) if "le_for_lt" in defects else (lambda a, b: a < b)
    step = np.zeros((L, n), np.int64)                  # predecessor offset of (l, k)
    M = e[0].copy()
    for l in range(1, L):
        left = np.concatenate([[INF], M[:-1]])
        right = np.concatenate([M[1:], [INF]])
        order = ((left, -1), (M, 0), (right, 1)) if "minus_first" in defects else ((M, 0), (left, -1), (right, 1))
        best, off = order[0][0].copy(), np.full(n, order[0][1], np.int64)
        for cand, o in order[1:]:
            take = less(cand, best) & (cand < INF)
            best, off = np.where(take, cand, best), np.where(take, o, off)
        step[l] = off
        M = e[l] + best
    ends = np.flatnonzero(M == M.min())
    k = int(ends[-1] if "last_argmin" in defects else ends[0])
    total = int(M[k])
    s = np.zeros(L, np.int32)
    for l in range(L - 1, -1, -1):
        s[l] = k
        k += int(step[l, k])
    return s, total


def seam(img1, img2, mask1, mask2, orientation="auto", first="auto", defects=frozenset()):
    """the whole contract: img [3,H,W], mask [1 or 3,H,W] -> side uint8 [H,W], info int32 [4] = (valid, orientation, first, path cost),
    path int32 [max(H,W)] (s per line of the decided orientation, -1 behind the last line).  Orientation, first, the path and its cost are
    reported whether or not the seam is valid; only `side` (all ones) depends on that."""
    m1, m2 = masks(mask1, mask2)
    H, W = m1.shape
    valid, orient, fst = decide(m1, m2, orientation, first, defects)
    e = cost(img1, img2, mask1, mask2, defects)
    s, total = dp(e if orient == VERTICAL else e.T, defects)
    y, x = np.mgrid[:H, :W]
    pos, line = (x, y) if orient == VERTICAL else (y, x)
    low = (pos < s[line]) if "side_lt" in defects else (pos <= s[line])
    side = (low == (fst == 1)) if valid else np.ones((H, W), bool)
    path = np.full(max(H, W), -1, np.int32)
    path[:len(s)] = s
    return side.astype(np.uint8), np.array([valid, orient, fst, total], np.int32), path


def fields(img1, img2, mask1, mask2, seam=None, dtype=np.float32):
    """`_multiband_ref.fields` with the ownership override: with a valid seam (side, info), W1 = m1 and (not m2 or side), inside U and,
    through the nearest pixel of U, outside it; else W1 = m1 and (not m2 or D1 >= D2)."""
    m1, m2 = masks(mask1, mask2)
    U = m1 | m2
    a, b = mb.to_u8(img1, dtype), mb.to_u8(img2, dtype)
    if seam is not None and int(seam[1][0]) != 0:
        own = np.asarray(seam[0]) != 0
    else:
        own = mb.edt_sq(m1, True).astype(np.int64) >= mb.edt_sq(m2, True).astype(np.int64)
    W1 = m1 & (~m2 | own)
    C = np.where(W1[None], a, b)
    Wf = W1.copy()
    if U.any():
        _, idx = mb.edt_sq(~U, False, True)
        q = np.where(U, np.arange(U.size).reshape(U.shape), idx)
        C = C.reshape(3, -1)[:, q]
        Wf = W1.reshape(-1)[q]
    else:
        C = np.where(U[None], C, 0)
        Wf = Wf & U
    return np.where(m1[None], a, C).astype(dtype), np.where(m2[None], b, C).astype(dtype), Wf.astype(dtype), U


def blend(img1, img2, mask1, mask2, levels=5, seam=None, dtype=np.float32):
    """`_multiband_ref.blend` along the seam (side, info); seam None or invalid: the distance seam"""
    I1f, I2f, Wf, U = fields(img1, img2, mask1, mask2, seam, dtype)
    R = np.clip(mb.pyramid_blend(I1f, I2f, Wf, levels), 0, 255)
    return np.where(U[None], R, 0).astype(dtype)


def owner_change_discontinuity(img1, img2, mask1, mask2, W1):
    """summed |p1 - p2| (over the channels, at both pixels of the pair) across 4-neighbour pairs inside the overlap whose owner differs"""
    m1, m2 = masks(mask1, mask2)
    O = m1 & m2
    d = np.abs(to_int(img1) - to_int(img2)).sum(0)
    total = 0
    for ax in (0, 1):
        sl0, sl1 = [slice(None)] * 2, [slice(None)] * 2
        sl0[ax], sl1[ax] = slice(None, -1), slice(1, None)
        sl0, sl1 = tuple(sl0), tuple(sl1)
        change = O[sl0] & O[sl1] & (W1[sl0] != W1[sl1])
        total += int((d[sl0] + d[sl1])[change].sum())
    return total


def seam_pixels(mask1, mask2, W1):
    """bool [H,W]: the overlap pixels with a 4-neighbour in the overlap that has the other owner"""
    m1, m2 = masks(mask1, mask2)
    O = m1 & m2
    W1 = np.asarray(W1) > 0.5
    on = np.zeros_like(O)
    for a, b in (((slice(None, -1), slice(None)), (slice(1, None), slice(None))), ((slice(None), slice(None, -1)), (slice(None), slice(1, None)))):
        change = O[a] & O[b] & (W1[a] != W1[b])
        on[a] |= change
        on[b] |= change
    return on


def ghost_scene(H=96, W=160, framed=False):
    """a smooth image, and image 2 = image 1 but for an inverted elliptical blob ("ghost") in the middle of the overlap
    -> img1, img2 [3,H,W] float32, mask1, mask2 [1,H,W] float32, ghost bool [H,W].  Masks: `quads`; ``framed``: two full-height bands
    instead, so that no line of the canvas leaves the union, and image 2 carries a texture of a few grey levels on top."""
    from _multiband_cases import quads
    y, x = np.mgrid[:H, :W]
    if framed:
        k1, k2 = (x < 0.62 * W)[None].astype(np.float32), (x > 0.33 * W)[None].astype(np.float32)
    else:
        k1, k2 = quads(H, W)
    base = np.floor(np.stack([60 + 100 * x / W + 20 * np.sin(y / 7.0), 90 + 80 * y / H, 120 + 40 * np.cos(x / 11.0)])).astype(np.float32)
    O = (k1[0] > 0.5) & (k2[0] > 0.5)
    cy, cx = y[O].mean(), x[O].mean()
    ghost = ((y - cy) / (0.22 * H)) ** 2 + ((x - cx) / (0.07 * W)) ** 2 <= 1.0
    img2 = np.where(ghost[None], 255.0 - base, base + ((x * 7 + y * 13) % 5 if framed else 0)).astype(np.float32)
    return base, img2, k1, k2, ghost


def corridor_scene(L, n, start=3, orientation="vertical"):
    """all-ones masks; the two images differ by 255 in every channel except along a diagonal corridor, one position per line, which moves
    one position per line and turns round at the borders of the line -> img1, img2, mask1, mask2, corridor int [L]"""
    c, k, d = np.zeros(L, np.int64), start, 1
    for l in range(L):
        c[l] = k
        if not 0 <= k + d < n:
            d = -d
        k += d if n > 1 else 0
    img2 = np.full((L, n), 255.0, np.float32)
    img2[np.arange(L), c] = 0
    if orientation == "horizontal":
        img2 = img2.T
    img2 = np.ascontiguousarray(np.broadcast_to(img2, (3,) + img2.shape))
    ones = np.ones((1,) + img2.shape[1:], np.float32)
    return np.zeros_like(img2), img2, ones, ones.copy(), c
