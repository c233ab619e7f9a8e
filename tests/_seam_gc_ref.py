"""CPU restatement of the seam_gc contract (README.md, seam_gc; csrc/seam_gc.hip) in integer numpy over scipy's `maximum_flow`: a minimum
cut over the overlap of two warped images, reported as its one canonical cut -- the overlap pixels that can still reach the sink in the
residual graph of a maximum flow, which is the same set for every maximum flow (the smallest sink side among all minimum cuts).  The
blend that takes the (side, info) pair is `_seam_ref.blend`, unchanged.

``defects``: a set of names from DEFECTS, each of which plants one deviation from the contract (tests/test_seam_gc_cpu.py shows that every
one of them fails an assertion).  Production callers pass none."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import breadth_first_order, maximum_flow

import _seam_ref as dpref

BIG = 1 << 18
DEFECTS = ("cap_single", "eight", "t_keeps_s", "source_side", "e_swapped", "round", "big_nodes")
N4 = ((0, -1), (0, 1), (-1, 0), (1, 0))
N8 = N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def shift(a, dy, dx, fill=False):
    """b[y, x] = a[y + dy, x + dx], `fill` beyond the canvas edge"""
    H, W = a.shape
    b = np.full_like(a, fill)
    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    yd, xd = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
    b[ys, xs] = a[yd, xd]
    return b


def cost(img1, img2, mask1, mask2, defects=frozenset()):
    """e int64 [H,W]: 1 + sum_c |p1 - p2| on the truncated pixels inside O (what `st_seam_cost` gives there), 0 elsewhere"""
    m1, m2 = dpref.masks(mask1, mask2)
    d = np.abs(dpref.to_int(img1, defects) - dpref.to_int(img2, defects)).sum(0)
    return np.where(m1 & m2, d + 1, 0).astype(np.int64)


def regions(mask1, mask2, defects=frozenset()):
    """-> O, E1, E2 bool [H,W]"""
    m1, m2 = dpref.masks(mask1, mask2)
    E1, E2 = m1 & ~m2, m2 & ~m1
    if "e_swapped" in defects:
        E1, E2 = E2, E1
    return m1 & m2, E1, E2


def seeds(O, E1, E2, defects=frozenset()):
    """S = O with a 4-neighbour in E1; T = O with a 4-neighbour in E2, not in S"""
    nb = N8 if "eight" in defects else N4
    near = lambda E: np.any([shift(E, dy, dx) for dy, dx in nb], axis=0)       # noqa: E731
    S, T = O & near(E1), O & near(E2)
    if "t_keeps_s" in defects:
        return S & ~T, T
    return S, T & ~S


def graph(e, N, S, T, defects=frozenset()):
    """the contracted network over the node pixels N: node 0 = all of S, node 1 = all of T, then the other pixels of N -> csr capacities
    int32, node index [H,W] (-1: not a node).  Arcs inside S or inside T vanish; parallel arcs into a terminal add up."""
    H, W = N.shape
    idx = np.full((H, W), -1, np.int64)
    free = N & ~S & ~T
    idx[free] = 2 + np.arange(int(free.sum()))
    idx[S], idx[T] = 0, 1
    n = 2 + int(free.sum())
    rows, cols, caps = [], [], []
    for dy, dx in (N8 if "eight" in defects else N4):
        eq, iq = shift(e, dy, dx, 0), shift(idx, dy, dx, -1)
        c = e if "cap_single" in defects else e + eq
        keep = N & shift(N, dy, dx) & (idx != iq)
        rows.append(idx[keep]); cols.append(iq[keep]); caps.append(c[keep])
    rows, cols, caps = (np.concatenate(v) for v in (rows, cols, caps))
    g = sp.coo_matrix((caps, (rows, cols)), shape=(n, n)).tocsr()             # (duplicates are summed)
    assert g.nnz == 0 or g.max() < 2 ** 31
    return g.astype(np.int32), idx


def seam(img1, img2, mask1, mask2, method="dinic", defects=frozenset()):
    """the whole contract: img [3,H,W], mask [1 or 3,H,W] -> side uint8 [H,W], info int32 [4] = (valid, 3, cut >> 31, cut & (2^31 - 1))"""
    O, E1, E2 = regions(mask1, mask2, defects)
    H, W = O.shape
    e = cost(img1, img2, mask1, mask2, defects)
    S, T = seeds(O, E1, E2, defects)
    side = np.ones((H, W), np.uint8)
    if not (S.any() and T.any()):
        return side, np.array([0, 3, 0, 0], np.int32)
    if "big_nodes" in defects:                                                # the exclusive pixels as nodes of cost BIG: E1 the source, E2 the sink
        g, idx = graph(np.where(E1 | E2, BIG, e), O | E1 | E2, E1, E2, defects)
    else:
        g, idx = graph(e, O, S, T, defects)
    res = maximum_flow(g, 0, 1, method=method)
    residual = (g - res.flow).tocsr()
    residual.data = np.maximum(residual.data, 0)
    residual.eliminate_zeros()
    if "source_side" in defects:
        reached = breadth_first_order(residual, 0, directed=True, return_predecessors=False)
        on = np.ones(g.shape[0], bool)
        on[reached] = False                                                   # the largest sink side instead of the smallest
    else:
        reached = breadth_first_order(residual.T.tocsr(), 1, directed=True, return_predecessors=False)
        on = np.zeros(g.shape[0], bool)
        on[reached] = True
    side[O] = ~on[idx[O]]
    cut = int(res.flow_value)
    return side, np.array([1, 3, cut >> 31, cut & (2 ** 31 - 1)], np.int32)


def cut_of(info):
    return (int(info[2]) << 31) | int(info[3])


def cut_value(e, O, side):
    """the summed capacity e(p) + e(q) of the arcs from side-1 to side-0 overlap pixels"""
    total = 0
    for dy, dx in N4:
        q_in, sq, eq = shift(O, dy, dx), shift(side, dy, dx, 1), shift(e, dy, dx, 0)
        total += int((e + eq)[O & q_in & (side == 1) & (sq == 0)].sum())
    return total


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
def serpentine_scene(orientation="vertical"):
    """44 x 48: full-height bands with a wide overlap; the images differ by 255 in every channel except along a two-pixel-wide corridor that
    runs across the overlap three times (it doubles back twice) -> img1, img2, mask1, mask2, corridor bool [H,W]"""
    H, W = 44, 48
    y, x = np.mgrid[:H, :W]
    k1, k2 = (x < 38), (x >= 10)
    cor = np.zeros((H, W), bool)
    cor[0:14, 14:16] = True
    cor[12:14, 14:34] = True
    cor[12:30, 32:34] = True
    cor[28:30, 14:34] = True
    cor[28:44, 14:16] = True
    img2 = np.where(cor, 0.0, 255.0).astype(np.float32)
    if orientation == "horizontal":
        k1, k2, cor, img2 = k1.T, k2.T, cor.T, img2.T
    img2 = np.ascontiguousarray(np.broadcast_to(img2, (3,) + img2.shape))
    f = lambda b: np.ascontiguousarray(b[None]).astype(np.float32)          # noqa: E731
    return np.zeros_like(img2), img2, f(k1), f(k2), np.ascontiguousarray(cor)


def l_hole_scene(H=40, W=44, seed=5):
    """an L-shaped overlap (image 2 covers the left columns and the bottom rows of image 1's rectangle) with a hole in mask 2 inside it, on
    smooth images with a little texture"""
    y, x = np.mgrid[:H, :W]
    m1 = (y >= 4) & (y < 34) & (x >= 8) & (x < 40)
    m2 = ((x < 18) | (y >= 24)) & (y >= 1) & (x >= 2) & (y < H - 1) & (x < W - 1)
    m2 &= ~((y >= 26) & (y < 30) & (x >= 24) & (x < 31))
    rng = np.random.default_rng(seed)
    base = np.floor(np.stack([80 + 2 * x + y, 60 + 3 * y, 200 - 2 * x])).astype(np.float32)
    img2 = base + rng.integers(0, 12, (3, H, W)).astype(np.float32)
    return base, img2, m1[None].astype(np.float32), m2[None].astype(np.float32)


def bands(H, W, lo=0.3, hi=0.7, transposed=False):
    """two bands across the whole canvas that overlap between lo and hi of the width (of the height when transposed)"""
    y, x = np.mgrid[:H, :W]
    u, n = (y, H) if transposed else (x, W)
    a, b = int(np.floor(lo * n)), int(np.ceil(hi * n))
    return (u < b)[None].astype(np.float32), (u >= a)[None].astype(np.float32)


def smooth_texture_pair(H, W, seed):
    y, x = np.mgrid[:H, :W]
    rng = np.random.default_rng(seed)
    base = np.stack([100 + 60 * np.sin(x / 23.0) + 30 * np.cos(y / 17.0), 90 + 80 * y / H, 120 + 40 * np.cos((x + y) / 31.0)])
    return np.floor(base).astype(np.float32), (np.floor(base) + rng.integers(0, 24, (3, H, W))).astype(np.float32)
