"""CPU restatement of the warm-start splat (``ops.forward_interpolate`` / ``st_flow_forward_interpolate``), numpy only.

Contract.  ``flow`` is [2, H, W] float32 (dx, dy) in low-resolution pixels.  Source pixel s = (i, j) lands at
px = double(j) + double(dx[s]), py = double(i) + double(dy[s]) and is VALID iff 0 < px < W and 0 < py < H (a NaN fails every
comparison, so it is invalid).  Query pixel (qi, qj) takes the flow (dx[s*], dy[s*]) of the valid source whose landing point is
nearest: s* minimises (qj - px)^2 + (qi - py)^2, evaluated in fp64 as two products and one sum.  Two stated deviations from the
scipy ``griddata(method="nearest")`` call this replaces: equal distances go to the LOWEST source index in row-major order (scipy's
order is that of its KD-tree), and a field without any valid source gives zeros (scipy raises).
"""
import numpy as np


def landing(flow):
    """(px, py, valid) as flat fp64 / bool arrays in row-major source order."""
    flow = np.asarray(flow, np.float32)
    _, H, W = flow.shape
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    px = (jj + flow[0].astype(np.float64)).reshape(-1)
    py = (ii + flow[1].astype(np.float64)).reshape(-1)
    with np.errstate(invalid="ignore"):
        valid = (px > 0) & (px < W) & (py > 0) & (py < H)
    return px, py, valid


def _distances(px, py, valid, q0, q1, W):
    """fp64 squared distances [q1 - q0, N] of queries q0..q1 (row-major) to every source; +inf for the invalid ones."""
    q = np.arange(q0, q1)
    qx, qy = (q % W).astype(np.float64)[:, None], (q // W).astype(np.float64)[:, None]
    with np.errstate(invalid="ignore"):
        ex, ey = qx - px[None, :], qy - py[None, :]
        d = ex * ex + ey * ey
    d[:, ~valid] = np.inf
    return d


def nearest_source(flow, chunk=256, want_gap=False):
    """index [H*W] of the chosen source per query (-1 everywhere if no source is valid); with ``want_gap`` also the fp64 difference
    between the second-best and the best squared distance per query (inf with fewer than two valid sources)."""
    flow = np.asarray(flow, np.float32)
    _, H, W = flow.shape
    N = H * W
    px, py, valid = landing(flow)
    if not valid.any():
        return (np.full(N, -1, np.int64), np.full(N, np.inf)) if want_gap else np.full(N, -1, np.int64)
    idx = np.empty(N, np.int64)
    gap = np.full(N, np.inf)
    for q0 in range(0, N, chunk):
        q1 = min(N, q0 + chunk)
        d = _distances(px, py, valid, q0, q1, W)
        best = np.argmin(d, axis=1)                  # first occurrence of the minimum: the lowest source index
        idx[q0:q1] = best
        if want_gap and valid.sum() > 1:
            rows = np.arange(q1 - q0)
            dmin = d[rows, best].copy()
            d[rows, best] = np.inf
            gap[q0:q1] = d.min(axis=1) - dmin
    return (idx, gap) if want_gap else idx


def forward_interpolate(flow):
    """[2, H, W] float32 -> [2, H, W] float32, the contract above; a leading batch dimension is looped over."""
    flow = np.asarray(flow, np.float32)
    if flow.ndim == 4:
        return np.stack([forward_interpolate(f) for f in flow])
    _, H, W = flow.shape
    idx = nearest_source(flow)
    if idx[0] < 0:
        return np.zeros_like(flow)
    return flow.reshape(2, -1)[:, idx].reshape(2, H, W).copy()


def generic_field(H, W, amp, seed):
    """a smooth field plus float noise, amplitude ``amp`` low-res px: no two landing points are equidistant from a pixel centre."""
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    fx = amp * (0.6 * np.sin(jj / 7.3 + ii / 11.9 + seed) + 0.4 * rng.uniform(-1, 1, (H, W)))
    fy = amp * (0.6 * np.cos(ii / 5.7 - jj / 13.1 + 2 * seed) + 0.4 * rng.uniform(-1, 1, (H, W)))
    return np.stack([fx, fy]).astype(np.float32)
