"""fp64 references and first-order worst-case elementwise error bounds for the gather, splat and per-pixel kernels of csrc/geom.hip,
csrc/flowops.hip and csrc/metrics.hip, and the input generators that tests/test_geom_bounds_cpu.py and tests/test_geom_matrix_gpu.py share.
Every reference states the operation in torch fp64 and knows nothing of a kernel's tiling; every bound E is a sum of the roundings the
kernel performs, each taken at its worst, to first order in u = 2^-24.  No constant here comes from a GPU measurement: each is a count
read from the kernel text, given below.  The kernels the project declares bit-exact (homo_warp, morph_open, blend, blend_plain, eval_finish,
mean_threshold, coords_grid(_init), flow_from_coords, load_rgb8, channel_mean, occlusion, the overlap plane, masked_psnr_ssim) have no
bound: the GPU file compares them with their restatements (oracle/cgeom.py, oracle/geom.py, oracle/adapter.py, oracle/metrics.py, torch
fp32 one rounding per operation) bit for bit.

Bilinear gathers   out = sum over the four taps of w_t v_t,  sampled at the pixel coordinate (x, y)
    The sampled surface (the source, zero padded for grid_sample, edge replicated for the resize) is continuous and piecewise bilinear, so a
    coordinate error (dx, dy) moves the value by at most dx Lx + dy Ly, where Lx / Ly is the largest horizontal / vertical difference of
    neighbouring samples of the padded source over the 4 x 4 block around the sample's cell: the cell itself and the cells a small error can
    push the sample into.  An fp32 / fp64 disagreement about floor() at an integer coordinate is a coordinate error like any other and
    needs no exclusion.  To this come the roundings of the weights and of the four-term sum, each relative to T = sum w |v|:

        E = dx Lx + dy Ly + u n_w T (+ u |out| per operation that follows: the multiplier of flow_warp, the divisor of the resize)

    kernel                          dx (dy alike with i, H)                           n_w
    flow_warp, homo_flow_warp       u (5 |a| + (W - 1) / 2),  a = j + fx             6
        flow_tap: a = j + fx (1 rounding, relative to |a|), 2 a / wm (1; the doubling is exact), - 1 (1, relative to |2 a / wm - 1|, which
        in pixels is |a - (W - 1) / 2|), + 1 (1), / 2 exact, * (W - 1) (1): 4 |a| + |a - (W - 1) / 2| <= 5 |a| + (W - 1) / 2.  The weights
        x1f - ix, ix - x0f are exact; each weight is one product (1), each tap one fused multiply-add (4 along the chain), + 1: n_w = 6.
        With W == 1 the divisor is max(W - 1, 1) = 1 and the factor W - 1 = 0: ix = 0 whatever the flow is (and NaN for a non-finite one);
        the reference states exactly that.  A sample whose coordinate is not finite is 0, exactly (E = 0): the project's documented rule.
    cost_lookup                     u (5 |a| + (W2 - 1) / 2),  a = cx + (i - r)      6
        the same chain with the offset added to the query's coordinate; channel i (2r + 1) + j: i moves x, j moves y.
    resize_bilinear, align 1        2 u s,  s = i (H - 1) / (oh - 1)                 6
        the step's division and the product; ly = s - y0 is exact, hy = 1 - ly (1), hx a (1), + lx b (2), hy (.) (1), the last sum (1).
    resize_bilinear, align 0 / 2    3 u (s + 1/2),  s = max(step (i + 1/2) - 1/2, 0)  6
        step = H / oh rounded (mode 0) or handed over as an fp32 (mode 2: the reference uses that fp32 too, as ATen does), the product, the
        subtraction of 1/2 (relative to s + 1/2 at most).  The divisor (ndiv = 2) adds u |out|.

convex_upsample   softmax over 9 logits pooling the tap values 8 (coords - grid), zero outside the image: the softmax-pooling bound of
    tests/_nn_bounds.py with  n_sub = 2, n_exp = 2 (ocml expf, 1 ulp, and its argument), no score term;  n_acc = 9 products + 9 sums + 1 for
    the subtraction coords - grid (relative to the tap value; 8 x is exact) = 19;  n_sum = 9;  + 2 inside the form: the division per tap.

range_map   out(t) = sum over the sources s that reach t of  w_s(t) = hat(cx_s - x_t) hat(cy_s - y_t),  c = pixel + flow
    fp64 splat of fp64 weights.  hat has slope <= 1, so the rounding of cx = j + fx (u |cx|) and of cy move a weight by at most
    u (|cx| + |cy|); 1 - ox, 1 - oy and the product (ox = cx - floor(cx) is exact): <= 3 u more; the fixed point adds 2^-33.  Per contribution
    u (|cx| + |cy| + 3) + 2^-33,
    summed over every source within one pixel of the target in both axes (a source on the edge of a hat has weight 0 in fp64 and may have
    u |cx| in fp32); the final conversion of the sum to fp32: u |out|.  Non-finite coordinates contribute nothing.

flow_encode   relu(b + sum of 98 taps w f),  f = coords1 - grid:  a 98-term fma chain on a rounded difference
        E = u (98 + 2) sum |w| |f| + u |b|          (relu is 1-Lipschitz)

mean_threshold, hard occlusion, overlap against fp64   the comparison may leave out samples whose fp64 value is within the case's E of the
    threshold (E: u (C + 1) mean|x| for the mean; the bounds above for the range map and the gathered ones-image), at most CAP of a case;
    the generators choose inputs for which the reference alone stays under CAP (asserted on the CPU)."""
import itertools

import torch
import torch.nn.functional as F

import _nn_bounds as nb
from _nn_bounds import U, gen, ratio  # noqa: F401

CAP = 0.01
N_W = 6
CONVEX_CONSTS = nb.Consts(0, 2, 2, 19, 9)
FIX = 2.0 ** -33


# ------------------------------------------------------------------------------------------------ the bilinear surface
def bilinear(src, x, y, border="zeros", defect=None):
    """src [B, C, H, W], pixel coordinates x, y [B, N] (any float dtype; the arithmetic is done in src's) -> the samples [B, C, N].
    border: "zeros" (grid_sample: taps outside contribute 0) or "edge" (the resize: taps clamp).  A non-finite coordinate gives 0.
    defect (tests/test_geom_bounds_cpu.py plants these): "swap_ne_sw": the weights of the north-east and south-west taps exchanged;
    "clamp_taps": out-of-range taps of a zero-padded surface read the border instead of 0."""
    B, C, H, W = src.shape
    dt = src.dtype
    x, y = x.to(dt), y.to(dt)
    fin = torch.isfinite(x) & torch.isfinite(y)
    x = torch.where(fin, x, torch.full_like(x, -5.0)).clamp(-1.5, W + 0.5)      # beyond [-1, W] the zero-padded surface is 0; the edge one never gets there
    y = torch.where(fin, y, torch.full_like(y, -5.0)).clamp(-1.5, H + 0.5)
    x0, y0 = torch.floor(x), torch.floor(y)
    lx, ly = x - x0, y - y0
    x0, y0 = x0.long(), y0.long()
    flat = src.reshape(B, C, H * W)

    def tap(yy, xx):
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        v = torch.gather(flat, 2, (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1))[:, None, :].expand(-1, C, -1))
        return v if border == "edge" or defect == "clamp_taps" else v * inside[:, None, :].to(dt)
    nw, ne, sw, se = (1 - lx) * (1 - ly), lx * (1 - ly), (1 - lx) * ly, lx * ly
    if defect == "swap_ne_sw":
        ne, sw = sw, ne
    out = tap(y0, x0) * nw[:, None] + tap(y0, x0 + 1) * ne[:, None] + tap(y0 + 1, x0) * sw[:, None] + tap(y0 + 1, x0 + 1) * se[:, None]
    return out * fin[:, None, :].to(dt)


def bilinear_bound(src, x, y, dx, dy, border="zeros"):
    """-> fp64 (samples, E) [B, C, N]: E = dx Lx + dy Ly + u N_W sum w |v|; Lx, Ly over the 4 x 4 block of the padded source around the cell"""
    src, x, y = src.double(), x.double(), y.double()
    B, C, H, W = src.shape
    ref = bilinear(src, x, y, border)
    T = bilinear(src.abs(), x, y, border)
    P = F.pad(src, (3, 3, 3, 3), mode="constant" if border == "zeros" else "replicate")
    fin = torch.isfinite(x) & torch.isfinite(y)
    x0 = torch.floor(torch.where(fin, x, torch.full_like(x, -5.0)).clamp(-1.5, W + 0.5)).long() + 3
    y0 = torch.floor(torch.where(fin, y, torch.full_like(y, -5.0)).clamp(-1.5, H + 0.5)).long() + 3
    Pf, Wp = P.reshape(B, C, -1), W + 6
    blk = torch.stack([torch.stack([torch.gather(Pf, 2, ((y0 + a) * Wp + (x0 + b))[:, None, :].expand(-1, C, -1)) for b in (-1, 0, 1, 2)], -1)
                       for a in (-1, 0, 1, 2)], -2)                                              # [B, C, N, 4 (y), 4 (x)]
    Lx = (blk[..., :, 1:] - blk[..., :, :-1]).abs().amax((-1, -2))
    Ly = (blk[..., 1:, :] - blk[..., :-1, :]).abs().amax((-1, -2))
    E = (dx[:, None] * Lx + dy[:, None] * Ly + U * N_W * T) * fin[:, None, :].double()
    return ref, E


def pixel_xy(H, W, dtype=torch.float64):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    return xs.reshape(-1), ys.reshape(-1)


# ------------------------------------------------------------------------------------------------ flow_warp / homo_flow_warp
def warp_coords(flow, dtype=torch.float64, swap_wm=False):
    """warp()'s normalisation and grid_sample's un-normalisation: pixel coordinates [B, H W] of the samples.  With W == 1 (H == 1) the
    divisor is 1 and the factor W - 1 is 0."""
    B, _, H, W = flow.shape
    px, py = pixel_xy(H, W, dtype)
    f = flow.to(dtype).reshape(B, 2, H * W)
    wm, hm = max(W - 1, 1), max(H - 1, 1)
    if swap_wm:
        wm, hm = hm, wm
    gx, gy = 2.0 * (px + f[:, 0]) / wm - 1.0, 2.0 * (py + f[:, 1]) / hm - 1.0
    return ((gx + 1.0) / 2.0) * (W - 1), ((gy + 1.0) / 2.0) * (H - 1)


def flow_warp_bound(x, flow, mul=None):
    """x [B, C, H, W], flow [B, 2, H, W], mul [B, 1, H, W] or None -> fp64 (ref, E) [B, C, H, W]"""
    B, C, H, W = x.shape
    ix, iy = warp_coords(flow)
    px, py = pixel_xy(H, W)
    f = flow.double().reshape(B, 2, H * W)
    ax, ay = (px + f[:, 0]).abs(), (py + f[:, 1]).abs()
    dx = U * (5 * ax + (W - 1) / 2) if W > 1 else torch.zeros_like(ax)
    dy = U * (5 * ay + (H - 1) / 2) if H > 1 else torch.zeros_like(ay)
    fin = torch.isfinite(ix) & torch.isfinite(iy)
    dx, dy = (torch.where(fin, d, torch.zeros_like(d)) for d in (dx, dy))
    ref, E = bilinear_bound(x, ix, iy, dx, dy)
    if mul is not None:
        m = mul.double().reshape(B, 1, H * W)
        ref, E = ref * m, E * m.abs() + U * (ref * m).abs()
    return ref.reshape(B, C, H, W), E.reshape(B, C, H, W)


def flow_warp32(x, flow, mul=None):
    """the control: torch CPU fp32 as the reference runs it (core/warp_utils.py:54-80); a non-finite sample set to 0 (the documented rule)"""
    B, _, H, W = flow.shape
    px, py = pixel_xy(H, W, torch.float32)
    g = torch.stack([2.0 * (px.view(H, W) + flow[:, 0]) / max(W - 1, 1) - 1.0, 2.0 * (py.view(H, W) + flow[:, 1]) / max(H - 1, 1) - 1.0], -1)
    out = F.grid_sample(x, g, mode="bilinear", padding_mode="zeros", align_corners=True)
    bad = ~torch.isfinite(((g[..., 0] + 1) / 2) * (W - 1)) | ~torch.isfinite(((g[..., 1] + 1) / 2) * (H - 1))
    out = torch.where(bad[:, None], torch.zeros_like(out), out)
    return out if mul is None else out * mul


def taps_out(flow):
    """how many of the four taps of each sample are outside the image [B, H W] (-1: a non-finite coordinate)"""
    B, _, H, W = flow.shape
    ix, iy = warp_coords(flow)
    fin = torch.isfinite(ix) & torch.isfinite(iy)
    x0, y0 = torch.floor(torch.nan_to_num(ix, 0.0, 0.0, 0.0)), torch.floor(torch.nan_to_num(iy, 0.0, 0.0, 0.0))
    n = torch.zeros_like(ix)
    for a in (0, 1):
        for b in (0, 1):
            n += ((x0 + b < 0) | (x0 + b > W - 1) | (y0 + a < 0) | (y0 + a > H - 1)).double()
    return torch.where(fin, n, torch.full_like(n, -1.0)).long()


ULP = 2.0 ** -23
KINDS = ("inside", "left", "right", "top", "bottom", "corner", "beyond", "far", "integer", "ulp_above", "ulp_below")


def warp_flow(B, H, W, seed, amp=None):
    """flow [B, 2, H, W] fp32 whose targets cycle, pixel by pixel and shifted per batch item, through KINDS: inside the image; straddling
    each of the four borders (two taps out) and a corner (three out; one tap out cannot happen on a rectangle); one to three pixels
    beyond a border (four out); far outside; exact integers; one ulp above and below an integer.  `amp`: a plain random flow of that size."""
    g = gen(seed)
    if amp is not None:
        return (torch.rand(B, 2, H, W, generator=g) * 2 - 1) * amp
    px, py = pixel_xy(H, W)
    r = lambda: torch.rand(B, H * W, generator=g, dtype=torch.float64)      # noqa: E731
    kind = (torch.arange(H * W)[None, :] + 3 * torch.arange(B)[:, None]) % len(KINDS)
    tx, ty = r() * (W - 1), r() * (H - 1)
    side = torch.rand(B, H * W, generator=g) < 0.5
    ix_, iy_ = torch.floor(r() * W), torch.floor(r() * H)
    sel = lambda k, a, b: torch.where(kind == KINDS.index(k), a, b)          # noqa: E731
    tx = sel("left", -r(), tx); tx = sel("right", W - 1 + r(), tx)
    ty = sel("top", -r(), ty); ty = sel("bottom", H - 1 + r(), ty)
    tx = sel("corner", torch.where(side, -r(), W - 1 + r()), tx); ty = sel("corner", torch.where(r() < 0.5, -r(), H - 1 + r()), ty)
    tx = sel("beyond", torch.where(side, -1 - 2 * r(), W + 2 * r()), tx)
    tx = sel("far", torch.where(side, -1e3 - 1e4 * r(), 1e5 + 1e6 * r()), tx); ty = sel("far", 3e4 * (r() - 0.5), ty)
    for k, s in (("integer", 0.0), ("ulp_above", ULP), ("ulp_below", -ULP)):
        tx = sel(k, ix_.clamp_min(1) * (1 + s), tx); ty = sel(k, iy_.clamp_min(1) * (1 + s), ty)
    return torch.stack([tx - px, ty - py], 1).reshape(B, 2, H, W).float()


def image(B, C, H, W, seed, lo=0.0, hi=255.0):
    """content unlike per batch item and per channel (a ramp of its own slope and direction under the noise), so that a wrong stride or a
    swapped axis changes the result"""
    g = gen(seed)
    px, py = pixel_xy(H, W, torch.float32)
    k = torch.arange(B * C, dtype=torch.float32).view(B, C, 1)
    ramp = ((3 + k) * px + (11 + 2 * k) * py) % 97.0 / 97.0
    return (lo + (hi - lo) * (0.5 * ramp + 0.5 * torch.rand(B, C, H * W, generator=g))).reshape(B, C, H, W)


# ------------------------------------------------------------------------------------------------ cost_lookup
def cost_lookup(maps, coords, H2, W2, r, dtype=torch.float64, defect=None):
    """maps [Nq, H2 W2], coords [Nq, 2] -> [Nq, (2r + 1)^2] in `dtype`: channel i (2r + 1) + j samples map n at (cx + i - r, cy + j - r).
    defect "swap_xy": the offsets exchanged; bilinear's defects are handed on"""
    Nq, side = maps.shape[0], 2 * r + 1
    d = torch.arange(side, dtype=dtype) - r
    di, dj = d.repeat_interleave(side), d.repeat(side)
    if defect == "swap_xy":
        di, dj = dj, di
    c = coords.to(dtype)
    x, y = c[:, 0:1] + di[None], c[:, 1:2] + dj[None]
    gx, gy = 2.0 * x / (W2 - 1) - 1.0, 2.0 * y / (H2 - 1) - 1.0
    ix, iy = ((gx + 1.0) / 2.0) * (W2 - 1), ((gy + 1.0) / 2.0) * (H2 - 1)
    return bilinear(maps.to(dtype).reshape(Nq, 1, H2, W2), ix, iy, defect=defect if defect != "swap_xy" else None)[:, 0], (x, y, ix, iy)


def cost_lookup_bound(maps, coords, H2, W2, r):
    Nq = maps.shape[0]
    _, (x, y, ix, iy) = cost_lookup(maps, coords, H2, W2, r)
    dx, dy = U * (5 * x.abs() + (W2 - 1) / 2), U * (5 * y.abs() + (H2 - 1) / 2)
    ref, E = bilinear_bound(maps.reshape(Nq, 1, H2, W2), ix, iy, dx, dy)
    return ref[:, 0], E[:, 0]


def lookup_inputs(Nq, H2, W2, seed):
    """maps with a large gradient in x (40 per pixel) and a small one in y (1 per pixel), different per query; query coordinates from
    one pixel outside to one pixel outside, every fourth an exact integer pair, every seventh far outside"""
    g = gen(seed)
    px, py = pixel_xy(H2, W2, torch.float32)
    n = torch.arange(Nq, dtype=torch.float32)[:, None]
    maps = 40.0 * px[None] + 1.0 * py[None] + 3.0 * n + torch.rand(Nq, H2 * W2, generator=g)
    c = torch.stack([torch.rand(Nq, generator=g) * (W2 + 1) - 1, torch.rand(Nq, generator=g) * (H2 + 1) - 1], 1)
    c[::4] = torch.floor(c[::4])
    c[6::7] = c[6::7] * 1e3 + 500
    return maps, c


# ------------------------------------------------------------------------------------------------ resize_bilinear
def resize_src(n_in, n_out, align, step, dtype):
    """source coordinate of every output index along one axis; `step`: the value the entry is handed in mode 2 (taken as the fp32 it becomes)"""
    i = torch.arange(n_out, dtype=dtype)
    if align == 1:
        return i * torch.tensor((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0, dtype=dtype)
    rh = float(torch.tensor(step, dtype=torch.float32)) if align == 2 else n_in / n_out
    return (torch.tensor(rh, dtype=dtype) * (i + 0.5) - 0.5).clamp_min(0.0)


def resize(x, oh, ow, align, steps=(1.0, 1.0), div=None, dtype=torch.float64, defect=None):
    """x [B, C, H, W] -> [B, C, oh, ow] in `dtype`: F.interpolate(bilinear) with align_corners = 1 / 0, or (align = 2) the scale_factor form
    whose source step is `steps` = (1 / scale_h, 1 / scale_w); div = (div0, div1): plane p divided by div[p % 2] (align 0 / 1).
    defects: "other_align", "step_from_sizes" (mode 2 stepping by H / oh), "swap_div" """
    B, C, H, W = x.shape
    if defect == "other_align":
        align = {0: 1, 1: 0, 2: 1}[align]
    if defect == "step_from_sizes" and align == 2:
        align = 0
    sy, sx = resize_src(H, oh, align, steps[0], dtype), resize_src(W, ow, align, steps[1], dtype)
    X, Y = sx[None, :].expand(oh, ow).reshape(1, -1), sy[:, None].expand(oh, ow).reshape(1, -1)
    out = bilinear(x.to(dtype).reshape(1, B * C, H, W), X, Y, border="edge").reshape(B, C, oh, ow)
    if div is not None and align != 2:
        d = torch.tensor([float(torch.tensor(v, dtype=torch.float32)) for v in (div[::-1] if defect == "swap_div" else div)], dtype=dtype)
        out = out / d[torch.arange(B * C) % 2].view(B, C, 1, 1)
    return out, (X, Y)


def resize_bound(x, oh, ow, align, steps=(1.0, 1.0), div=None):
    B, C, H, W = x.shape
    ref, (X, Y) = resize(x, oh, ow, align, steps, div)
    dx, dy = (2 * U * X, 2 * U * Y) if align == 1 else (3 * U * (X + 0.5), 3 * U * (Y + 0.5))
    raw, E = bilinear_bound(x.reshape(1, B * C, H, W), X, Y, dx, dy, border="edge")
    E = E.reshape(B, C, oh, ow)
    if div is not None and align != 2:
        E = E / _divs(div, B, C) + U * ref.abs()
    return ref, E


def _divs(div, B, C):
    d = torch.tensor([float(torch.tensor(v, dtype=torch.float32)) for v in div], dtype=torch.float64).abs()
    return d[torch.arange(B * C) % 2].view(B, C, 1, 1)


def resize32(x, oh, ow, align, scale=None, div=None):
    """the control: F.interpolate in fp32 as the callers' reference runs it (resize_flow, Resize((512, 512)), out.py's scale_factor form)"""
    if align == 2:
        out = F.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=False)
        assert tuple(out.shape[2:]) == (oh, ow), (out.shape, oh, ow)
        return out
    out = F.interpolate(x, (oh, ow), mode="bilinear", align_corners=bool(align))
    if div is not None:
        B, C = x.shape[:2]
        out = out / torch.tensor(div, dtype=torch.float32)[torch.arange(B * C) % 2].view(B, C, 1, 1)
    return out


# ------------------------------------------------------------------------------------------------ convex_upsample
def convex_taps(coords1, B, H, W, dtype=torch.float64, transpose=False):
    """the nine zero-padded tap values 8 (coords1 - grid) of every pixel: [B, H W, 9, 2]; tap k is the neighbour (k / 3 - 1, k % 3 - 1) in (y, x)"""
    px, py = pixel_xy(H, W, dtype)
    f = 8.0 * (coords1.to(dtype).reshape(B, H * W, 2) - torch.stack([px, py], -1)[None])
    f = F.pad(f.reshape(B, H, W, 2).permute(0, 3, 1, 2), (1, 1, 1, 1))
    taps = [f[:, :, (k % 3 if transpose else k // 3):(k % 3 if transpose else k // 3) + H,
              (k // 3 if transpose else k % 3):(k // 3 if transpose else k % 3) + W] for k in range(9)]
    return torch.stack(taps, -1).permute(0, 2, 3, 4, 1).reshape(B, H * W, 9, 2)


def convex_assemble(o, B, H, W):
    """[B, H W, 64 (i, j), 2] -> NCHW [B, 2, 8H, 8W]"""
    return o.reshape(B, H, W, 8, 8, 2).permute(0, 5, 1, 3, 2, 4).reshape(B, 2, 8 * H, 8 * W)


def convex_upsample(coords1, mask, B, H, W, dtype=torch.float64, defect=None):
    """coords1 [B H W, 2], mask [B H W, 576] (channel k 64 + i 8 + j) -> [B, 2, 8H, 8W].  defects: "no_max" (exp of the raw logits),
    "transpose_taps" """
    s = mask.to(dtype).reshape(B, H * W, 9, 64).transpose(2, 3)                              # [B, HW, 64, 9]
    if defect == "no_max":
        e = torch.exp(s)
        p = e / e.sum(-1, keepdim=True)
    else:
        p = torch.softmax(s, -1)
    return convex_assemble(p @ convex_taps(coords1, B, H, W, dtype, transpose=defect == "transpose_taps"), B, H, W)


def convex_upsample_bound(coords1, mask, B, H, W):
    s = mask.double().reshape(B, H * W, 9, 64).transpose(2, 3)
    ref, E = nb.pool_bound(s, None, convex_taps(coords1, B, H, W), CONVEX_CONSTS)
    return convex_assemble(ref, B, H, W), convex_assemble(E, B, H, W)


def convex_inputs(B, H, W, amp, seed, dominant=False):
    """coords1 = grid + a flow of a few pixels, logits randn * amp; dominant: one tap (its index varies) 200 ahead of the others"""
    g = gen(seed)
    px, py = pixel_xy(H, W, torch.float32)
    coords1 = (torch.stack([px, py], -1)[None] + 4.0 * torch.randn(B, H * W, 2, generator=g)).reshape(-1, 2)
    mask = amp * torch.randn(B * H * W, 576, generator=g)
    if dominant:
        k = (torch.arange(B * H * W)[:, None] + torch.arange(64)[None, :]) % 9
        mask.view(-1, 9, 64).scatter_(1, k[:, None, :], 200.0)
    return coords1, mask


# ------------------------------------------------------------------------------------------------ range_map
def range_map(flow, dtype=torch.float64, drop=None):
    """flow [B, 2, H, W] -> [B, 1, H, W]: bilinear forward splat of ones.  drop: index (b, pixel) of a source left out (a planted defect)"""
    B, _, H, W = flow.shape
    px, py = pixel_xy(H, W, dtype)
    f = flow.to(dtype).reshape(B, 2, H * W)
    cx, cy = px + f[:, 0], py + f[:, 1]
    fin = torch.isfinite(cx) & torch.isfinite(cy)
    if drop is not None:
        fin = fin.clone()
        fin[drop] = False
    cxs, cys = (torch.where(fin, c, torch.full_like(c, -9.0)).clamp(-9.0, 1e6) for c in (cx, cy))
    x0, y0 = torch.floor(cxs), torch.floor(cys)
    ox, oy = cxs - x0, cys - y0
    out = torch.zeros(B, H * W, dtype=dtype)
    for dj, wy in ((0, 1 - oy), (1, oy)):
        for di, wx in ((0, 1 - ox), (1, ox)):
            xi, yj = x0.long() + di, y0.long() + dj
            ok = fin & (xi >= 0) & (xi < W) & (yj >= 0) & (yj < H)
            out.scatter_add_(1, (yj.clamp(0, H - 1) * W + xi.clamp(0, W - 1)), torch.where(ok, wx * wy, torch.zeros_like(wx)))
    return out.reshape(B, 1, H, W)


def range_map_bound(flow):
    B, _, H, W = flow.shape
    ref = range_map(flow)
    px, py = pixel_xy(H, W)
    f = flow.double().reshape(B, 2, H * W)
    cx, cy = px + f[:, 0], py + f[:, 1]
    fin = torch.isfinite(cx) & torch.isfinite(cy)
    cxs, cys = (torch.where(fin, c, torch.full_like(c, -9.0)).clamp(-9.0, 1e6) for c in (cx, cy))
    e = U * (cxs.abs() + cys.abs() + 3) + FIX
    x0, y0 = torch.floor(cxs), torch.floor(cys)
    E = torch.zeros(B, H * W, dtype=torch.float64)
    for dj in (-1, 0, 1, 2):
        for di in (-1, 0, 1, 2):
            xt, yt = x0 + di, y0 + dj
            ok = fin & ((cxs - xt).abs() <= 1) & ((cys - yt).abs() <= 1) & (xt >= 0) & (xt < W) & (yt >= 0) & (yt < H)
            E.scatter_add_(1, (yt.long().clamp(0, H - 1) * W + xt.long().clamp(0, W - 1)), torch.where(ok, e, torch.zeros_like(e)))
    return ref, E.reshape(B, 1, H, W) + U * ref.abs()


RANGE_PATTERNS = ("zero", "shift", "collapse", "leave", "random", "nonfinite")


def range_flow(pattern, B, H, W, seed):
    g = gen(seed)
    px, py = pixel_xy(H, W, torch.float32)
    if pattern == "zero":
        return torch.zeros(B, 2, H, W)
    if pattern == "shift":                                    # an integer shift of its own per batch item: part of the image leaves
        s = torch.stack([torch.arange(B) % 3 - 1, (torch.arange(B) + 1) % 3], 1).float()
        return s.view(B, 2, 1, 1).expand(B, 2, H, W).clone()
    if pattern == "collapse":                                 # every source onto one pixel (its own per batch item): sum = H W exactly
        tx, ty = (torch.arange(B) * 5 + 1) % W, (torch.arange(B) * 3 + 1) % H
        return torch.stack([tx[:, None] - px[None], ty[:, None] - py[None]], 1).reshape(B, 2, H, W)
    if pattern == "leave":
        return torch.full((B, 2, H, W), float(2 * max(H, W) + 3)) * torch.tensor([1.0, -1.0]).view(1, 2, 1, 1)
    f = (torch.rand(B, 2, H, W, generator=g) * 12 - 6)
    if pattern == "nonfinite":
        n = H * W
        for b in range(B):
            for k, v in enumerate((float("nan"), float("inf"), -float("inf"))):
                f.view(B, 2, n)[b, (b + k) % 2, (7 * b + 3 * k) % n] = v
    return f


# ------------------------------------------------------------------------------------------------ flow_encode
def flow_encode_bound(coords1, w98, bias, B, H, W):
    """coords1 [B H W, 2], w98 [98, Co] (tap-major: (ky 7 + kx) 2 + c), bias [Co] -> fp64 (ref, E) [B H W, Co]"""
    Co = w98.shape[1]
    px, py = pixel_xy(H, W)
    f = (coords1.double().reshape(B, H * W, 2) - torch.stack([px, py], -1)[None]).reshape(B, H, W, 2).permute(0, 3, 1, 2)
    wt = w98.double().reshape(7, 7, 2, Co).permute(3, 2, 0, 1)
    ref = F.relu(F.conv2d(f, wt, bias.double(), padding=3))
    S = F.conv2d(f.abs(), wt.abs(), padding=3)
    E = U * (98 + 2) * S + U * bias.double().abs().view(1, Co, 1, 1)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B * H * W, Co)           # noqa: E731
    return rows(ref), rows(E), f.permute(0, 2, 3, 1).reshape(B * H * W, 2)


def flow_encode32(coords1, w98, bias, B, H, W):
    Co = w98.shape[1]
    px, py = pixel_xy(H, W, torch.float32)
    f = (coords1.reshape(B, H * W, 2) - torch.stack([px, py], -1)[None]).reshape(B, H, W, 2).permute(0, 3, 1, 2)
    return F.relu(F.conv2d(f, w98.reshape(7, 7, 2, Co).permute(3, 2, 0, 1), bias, padding=3)).permute(0, 2, 3, 1).reshape(B * H * W, Co)


def flow_encode_inputs(B, H, W, Co, seed):
    g = gen(seed)
    px, py = pixel_xy(H, W, torch.float32)
    coords1 = (torch.stack([px, py], -1)[None] + 4.0 * torch.randn(B, H * W, 2, generator=g)).reshape(-1, 2)
    return coords1, torch.randn(98, Co, generator=g) / 98 ** 0.5, torch.randn(Co, generator=g)


# ------------------------------------------------------------------------------------------------ thresholds with a cap
def mean_threshold_bound(x, thr):
    """x [B, C, H, W] -> (fp64 mean > thr as 0 / 1 [B, 1, H, W], near: within E = u (C + 1) mean|x| of thr)"""
    C = x.shape[1]
    m = x.double().mean(1, keepdim=True)
    return (m > thr).double(), (m - float(torch.tensor(thr, dtype=torch.float32))).abs() <= U * (C + 1) * x.double().abs().mean(1, keepdim=True)


def capped_equal(out, want, near, cap=CAP):
    """out == want wherever `near` is false, and `near` covers at most `cap` of the case"""
    assert near.double().mean().item() <= cap, f"{near.double().mean().item():.4f} of the samples lie within E of the threshold"
    return bool((out.double()[~near] == want.double()[~near]).all())


def mean_inputs(shape, thr, seed):
    """[B, C, H, W] values in [0, 1] with zones of exact 0 and 1 whose channel mean keeps 1e-3 away from thr (a pixel that came closer is
    scaled by 0.9)"""
    g = gen(seed)
    v, z = torch.rand(shape, generator=g), torch.rand(shape[:1] + (1,) + shape[2:], generator=g)
    v = torch.where(z < 0.2, torch.zeros_like(v), torch.where(z > 0.8, torch.ones_like(v), v))
    near = (v.double().mean(1, keepdim=True) - thr).abs() < 1e-3
    return torch.where(near, v * 0.9, v)


# ------------------------------------------------------------------------------------------------ case tables (both files run all of them)
def cyc(seq, i):
    return seq[i % len(seq)]


TILE_H, TILE_W = (1, 2, 3, 4, 5, 37), (1, 2, 63, 64, 65, 130)      # a block takes 4 rows of 64 columns
# flow_warp: (H, W, B, C, mul)
WARP_CASES = [(H, W, cyc((1, 3), a + b), cyc((1, 3, 6), a + 2 * b), bool((a + b // 2) % 2))
              for (a, H), (b, W) in itertools.product(enumerate(TILE_H), enumerate(TILE_W))]
# homo_flow_warp: (H, W), B = 3 with a homography of its own per item
HOMO_FLOW_CASES = [(cyc(TILE_H, i), W) for i, W in enumerate(TILE_W)] + [(H, cyc(TILE_W, i + 3)) for i, H in enumerate(TILE_H)]
# homo_warp: (H, W, oh, ow, B, C, n_ones)
HOMO_CASES = [(cyc(TILE_H, a + 2 * b + 1), cyc(TILE_W, 2 * a + b + 2), oh, ow, cyc((1, 3), a + b), cyc((1, 3, 6), a), cyc((0, 3), b))
              for (a, oh), (b, ow) in itertools.product(enumerate(TILE_H), enumerate(TILE_W))]
# resize_bilinear: (H, W, oh, ow, align, B, C, div, scale); div only with align 1 / 0 on 2 and 4 planes; scale only with align 2
RESIZE_CASES = []
for (_a, _H), (_b, _W), _al in itertools.product(enumerate(TILE_H), enumerate(TILE_W), (0, 1)):
    _B, _C = cyc(((1, 2), (2, 2), (3, 1), (1, 3), (3, 6)), _a + _b + _al)
    _div = (0.75, 1.5) if _B * _C in (2, 4) else None
    RESIZE_CASES.append((_H, _W, cyc(TILE_H, _a + _b + 1 + _al), cyc(TILE_W, 2 * _a + _b + 3 * _al), _al, _B, _C, _div, None))
RESIZE_CASES += [(5, 65, 5, 65, 0, 1, 2, (0.75, 1.5), None), (5, 65, 5, 65, 1, 2, 2, (1.25, 0.5), None), (37, 130, 1, 64, 1, 1, 3, None, None),
                 (37, 130, 4, 1, 0, 1, 3, None, None)]
for _s, (_H, _W), (_B, _C) in itertools.product((0.5, 2.0, 1.5), ((2, 2), (5, 65), (37, 130), (3, 63), (4, 64), (1, 2)), ((1, 3),)):
    if int(_H * _s) >= 1 and int(_W * _s) >= 1:
        RESIZE_CASES.append((_H, _W, int(_H * _s), int(_W * _s), 2, cyc((1, 3), _H), _C, None, _s))
# cost_lookup: (H2, W2, r, Nq, extra columns of ldo)
LOOKUP_CASES = [(H2, W2, r, Nq, cyc((0, 3), a + b + c))
                for (a, (H2, W2)), (b, r), (c, Nq) in itertools.product(enumerate(((2, 2), (2, 9), (12, 16), (7, 33))), enumerate((0, 1, 4)), enumerate((1, 37, 256)))]
# convex_upsample: (B, H, W, ldm, amp) with amp "dominant" = one tap 200 ahead
CONVEX_HW, CONVEX_AMPS = ((1, 1), (1, 7), (5, 1), (3, 5), (12, 16)), (1.0, 20.0, 80.0, "dominant")
CONVEX_CASES = [(cyc((1, 3), a + b), H, W, cyc((576, 580), a + b // 2), amp) for (a, (H, W)), (b, amp) in itertools.product(enumerate(CONVEX_HW), enumerate(CONVEX_AMPS))]
# flow_encode: (Co, H, W, B, flow2 given)
ENCODE_CO, ENCODE_HW = (4, 32, 128, 132, 256), ((1, 1), (3, 7), (4, 8), (5, 9), (13, 22))
ENCODE_CASES = [(Co, H, W, cyc((1, 2), a + b), (a + 2 * b) % 3 != 0) for (a, Co), (b, (H, W)) in itertools.product(enumerate(ENCODE_CO), enumerate(ENCODE_HW))]
# range_map: (H, W, B, pattern)
RANGE_HW = ((1, 1), (2, 3), (5, 65), (37, 70))
RANGE_CASES = [(H, W, B, p) for (H, W), B, p in itertools.product(RANGE_HW, (1, 3), RANGE_PATTERNS)]
MORPH_KSZ, MORPH_HW = (1, 3, 19), ((1, 1), (5, 7), (18, 19), (19, 20), (70, 45))
PIXEL_HW = ((1, 1), (5, 51), (16, 16), (1, 257), (67, 131))          # h w = 1, 255, 256, 257, 67 131
METRIC_HW = ((7, 7), (7, 8), (8, 12), (33, 40))
GRID_CASES = [(3, 5, 7, 2), (3, 1, 1, 4), (1, 13, 22, 8), (3, 9, 19, 4), (2, 16, 16, 4)]      # (B, H, W, ld4): B H W = 105, 3, 286, 513, 512


def resize_kind(c):
    H, W, oh, ow = c[:4]
    return ("same" if (oh, ow) == (H, W) else "") + ("up" if oh > H or ow > W else "") + ("down" if oh < H or ow < W else "")


# ------------------------------------------------------------------------------------------------ controls and restatements in fp32
def lookup32(maps, coords, H2, W2, r):
    """the control: bilinear_sampler + F.grid_sample in torch CPU fp32 (core/utils/utils.py:62-76, decoder.py:242-260): the first axis of
    the window moves x"""
    Nq, side = maps.shape[0], 2 * r + 1
    d = torch.arange(side, dtype=torch.float32) - r
    x = (coords[:, 0, None, None] + d[None, :, None]).expand(Nq, side, side)
    y = (coords[:, 1, None, None] + d[None, None, :]).expand(Nq, side, side)
    g = torch.stack([2.0 * x / (W2 - 1) - 1.0, 2.0 * y / (H2 - 1) - 1.0], -1)
    return F.grid_sample(maps.reshape(Nq, 1, H2, W2), g, mode="bilinear", padding_mode="zeros", align_corners=True).reshape(Nq, side * side)


def warp_planted(x, flow, defect=None, swap_wm=False):
    """flow_warp in fp32 through `bilinear`, with one of its planted defects"""
    B, C, H, W = x.shape
    ix, iy = warp_coords(flow, torch.float32, swap_wm=swap_wm)
    return bilinear(x, ix, iy, defect=defect).reshape(B, C, H, W)


def homo_flow_inputs(B, H, W, seed):
    """image2 with uint8 values, a mild homography of its own per batch item and a residual flow through the KINDS of warp_flow"""
    g = gen(seed)
    H8 = torch.eye(3)[None].repeat(B, 1, 1) + torch.randn(B, 3, 3, generator=g) * torch.tensor([[0.02, 0.02, 2.0], [0.02, 0.02, 2.0], [1e-4, 1e-4, 0.0]])
    return image(B, 3, H, W, seed + 1).round(), H8, warp_flow(B, H, W, seed + 2)


def homo_flow_final_flow(H8, flow):
    """(Hi, final_flow) of the use_combine_h_flow branch in numpy fp32, operation for operation (the restatement that
    tests/test_branches_cpu.py pins to the reference's final_flow bit for bit): Hi = inverse(H8) as MKL runs it on a contiguous operand
    (oracle/cgeom.py), the mesh through inverse(Hi) as it runs on a column-major one, summed x, 1, y unfused."""
    import numpy as np
    from oracle import cgeom
    from oracle.mat3 import F32, inv3_column_major
    B, _, h, w = flow.shape
    Hi = cgeom.inverse(H8.numpy())
    x = torch.linspace(0.0, float(w), w).numpy()[None, :].repeat(h, 0)
    y = torch.linspace(0.0, float(h), h).numpy()[:, None].repeat(w, 1)
    fl, out = flow.numpy(), np.empty((B, 2, h, w), F32)
    for b in range(B):
        p = inv3_column_major(Hi[b]).reshape(-1)
        t = [((p[3 * r] * x).astype(F32) + p[3 * r + 2]).astype(F32) + (p[3 * r + 1] * y).astype(F32) for r in range(3)]
        out[b, 0] = ((t[0] / t[2]).astype(F32) - x).astype(F32) + fl[b, 0]
        out[b, 1] = ((t[1] / t[2]).astype(F32) - y).astype(F32) + fl[b, 1]
    return torch.from_numpy(Hi), torch.from_numpy(out)


def overlap32(ones_plane):
    """eval_finish's mean over three equal planes and the threshold, in fp32: ((o + o) + o) / 3 < 0.9"""
    return ((((ones_plane + ones_plane) + ones_plane) / 3.0) < 0.9).float()
