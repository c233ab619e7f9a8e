"""CPU restatement of the Telea inpainting contract (README.md, "cv_inpainter"; csrc/inpaint.hip).  The ring index d and the
arrival time T follow the kernel's fp32 operation order and are bit-exact; the fill is evaluated in float64.  Not OpenCV:
cv2.inpaint's sequential heap order is not reproduced."""
import numpy as np

FAR = 0x3fffffff
LUMA = (19595, 38470, 7471)


def prep_mask(mask):
    """cv_inpainter's mask: float [1 or 3,H,W] -> uint8 [H,W] luma (nonzero = fill)."""
    m = np.asarray(mask, np.float32)
    if m.shape[0] == 1:
        m = np.repeat(m, 3, 0)
    if m.max() <= np.float32(1.1):
        m = np.clip(m * np.float32(255), 0, 255)
    m = np.clip(m, 0, 255).astype(np.uint8).astype(np.uint32)
    return ((m[0] * LUMA[0] + m[1] * LUMA[1] + m[2] * LUMA[2] + 0x8000) >> 16).astype(np.uint8)


def prep_image(img3):
    """float [3,H,W] -> uint8 [H,W,3]: clamp to 0..255, truncate."""
    return np.clip(np.asarray(img3, np.float32), 0, 255).astype(np.uint8).transpose(1, 2, 0).copy()


def ring_distance(fill):
    """4-connected step distance to the pixels where `fill` is False (L1 distance in a rectangle); FAR if there are none."""
    H, W = fill.shape
    g = np.where(fill, FAR, 0).astype(np.int64)
    for x in range(1, W):
        g[:, x] = np.minimum(g[:, x], g[:, x - 1] + 1)
    for x in range(W - 2, -1, -1):
        g[:, x] = np.minimum(g[:, x], g[:, x + 1] + 1)
    for y in range(1, H):
        g[y] = np.minimum(g[y], g[y - 1] + 1)
    for y in range(H - 2, -1, -1):
        g[y] = np.minimum(g[y], g[y + 1] + 1)
    return np.minimum(g, FAR).astype(np.int32)


def _nbrs(d, T, ys, xs, k):
    """T of the 4 neighbours of (ys, xs) that have d < k (inf where absent): left, right, up, down."""
    H, W = d.shape
    out = []
    for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
        yy, xx = ys + dy, xs + dx
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        yc, xc = np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)
        ok &= d[yc, xc] < k
        out.append(np.where(ok, T[yc, xc], np.float32(np.inf)).astype(np.float32))
    return out


def arrival_time(d):
    """T per the contract, float32, ring by ring in the kernel's operation order."""
    T = np.zeros(d.shape, np.float32)
    valid = d[d < FAR]
    for k in range(1, int(valid.max()) + 1 if valid.size else 1):
        ys, xs = np.nonzero(d == k)
        tl, tr, tu, td = _nbrs(d, T, ys, xs, k)
        a, b = np.minimum(tl, tr), np.minimum(tu, td)
        with np.errstate(invalid="ignore", over="ignore"):
            dd = a - b
            sq = np.sqrt(np.maximum(np.float32(2) - dd * dd, np.float32(0)))
            two = ((a + b) + sq) * np.float32(0.5)
        one = np.minimum(a, b) + np.float32(1)
        T[ys, xs] = np.where(np.isinf(a) | np.isinf(b) | (np.abs(dd) >= np.float32(1)), one, two).astype(np.float32)
    return T


def disc(radius):
    dy, dx = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    r2 = dx * dx + dy * dy
    keep = (r2 > 0) & (r2 <= radius * radius)
    return dx[keep], dy[keep]


def _axis_grad(v, has_lo, has_hi, lo, hi, c):
    return np.where(has_lo & has_hi, (hi - lo) / 2, np.where(has_hi, hi - c, np.where(has_lo, c - lo, 0.0)))


def fill_value(img, d, T, y, x, radius, offs=None):
    """float64 [3] the contract assigns to pixel (y, x) of ring k = d[y, x], reading img (uint8 [H,W,3]) only where d < k."""
    H, W = d.shape
    k = int(d[y, x])
    Tf = T.astype(np.float64)
    tl, tr, tu, td = [float(v[0]) for v in _nbrs(d, T, np.array([y]), np.array([x]), k)]
    tp = float(T[y, x])
    nx = (tr - tl) / 2 if np.isfinite(tl) and np.isfinite(tr) else tr - tp if np.isfinite(tr) else tp - tl if np.isfinite(tl) else 0.0
    ny = (td - tu) / 2 if np.isfinite(tu) and np.isfinite(td) else td - tp if np.isfinite(td) else tp - tu if np.isfinite(tu) else 0.0
    n = np.hypot(nx, ny)
    if n > 0:
        nx, ny = nx / n, ny / n
    rx, ry = offs if offs is not None else disc(radius)
    qx, qy = x - rx, y - ry
    ok = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
    rx, ry, qx, qy = rx[ok], ry[ok], qx[ok], qy[ok]
    ok = d[qy, qx] < k
    rx, ry, qx, qy = rx[ok].astype(np.float64), ry[ok].astype(np.float64), qx[ok], qy[ok]
    I = img.astype(np.float64)

    def nb(dy, dx):
        yy, xx = qy + dy, qx + dx
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        yc, xc = np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)
        return inside & (d[yc, xc] < k), I[yc, xc]

    hl, vl = nb(0, -1)
    hr, vr = nb(0, 1)
    hu, vu = nb(-1, 0)
    hd, vd = nb(1, 0)
    c = I[qy, qx]
    gx = _axis_grad(c, hl[:, None], hr[:, None], vl, vr, c)
    gy = _axis_grad(c, hu[:, None], hd[:, None], vu, vd, c)
    r = np.sqrt(rx * rx + ry * ry)
    w = np.maximum(np.abs(nx * rx + ny * ry) / r, 1e-6) / (r * r) / (1.0 + np.abs(tp - Tf[qy, qx]))
    v = c + gx * rx[:, None] + gy * ry[:, None]
    return (w[:, None] * v).sum(0) / w.sum()


def round_u8(v):
    return np.clip(np.floor(np.asarray(v) + 0.5), 0, 255).astype(np.uint8)


def telea(img, fill, radius):
    """Full restatement: uint8 [H,W,3], bool [H,W] -> (uint8 [H,W,3], d, T).  Small images only (one numpy pass per pixel)."""
    out = img.copy()
    d = ring_distance(fill)
    if not fill.any() or (d == FAR).all():
        return out, d, np.zeros(d.shape, np.float32)
    T = arrival_time(d)
    offs = disc(radius)
    for k in range(1, int(d.max()) + 1):
        ys, xs = np.nonzero(d == k)
        vals = [fill_value(out, d, T, y, x, radius, offs) for y, x in zip(ys, xs)]
        for (y, x), v in zip(zip(ys, xs), vals):
            out[y, x] = round_u8(v)
    return out, d, T
