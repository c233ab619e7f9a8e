"""References, restatements, generators and case tables for the kernels behind the flow network: the per-pixel stages and the arg-max of
csrc/tps_pipeline.hip, the fp64 Gauss-Jordan of csrc/tps_solve.h (st_tps2_solve, st_tps_other_solve) and tps2_warp.  Shared by
tests/test_post_bounds_cpu.py and tests/test_post_matrix_gpu.py; laid out like tests/_geom_bounds.py.

1. Per-pixel kernels: the references are the torch-CPU fp32 expressions of oracle/tps_pipeline.py (one rounding per torch operation, which
   the kernels keep: -ffp-contract=off).  The GPU file asks for torch.equal.  Where a reference reduces (the k x k box sums, the Sobel taps,
   the channel means) the kernel adds in a fixed order; `*_inorder` states that order with one fp32 rounding per addition and the CPU file
   shows on every case of the tables that torch's own reduction gives the same bits -- what the bit-exact bar relies on.
2. range_argmax: the oracle's inner statement (mask, -1 outside, torch.argmax), and `argmax_sim`, a thread-for-thread numpy restatement of
   range_argmax_kernel (stride loop, tie rule, 256-slot tree) in which the CPU file plants the kernel's possible defects.
3. TPS solves: the systems as the kernels build them, their fp64 solutions, the reference's own fp32 torch.linalg.solve as the control, and
   `gauss_jordan`, a numpy restatement of tps_gauss_jordan with its two storage layouts and two planted defects.
4. tps2_warp: the fp64 statement of spline + bilinear sampling (zeros outside), its fp32 twin, and the quantised (mode 3) form.

No bound here is a measured constant: a bar is torch.equal, the control rule err <= 4 max(err of the fp32 reference on the same case, 2^-24)
(rms: 2 x), or a stated cap (CAP of a case may be left out next to a rounding boundary)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import _other_tps_ref as OR
from _geom_bounds import cyc
from _nn_bounds import gen
from oracle import tps_pipeline as otp

FLOOR = 2.0 ** -24
CAP = 0.01
INF = float("inf")

# ================================================================================================ 1. shapes
TILE_H, TILE_W = (1, 3, 4, 5, 9), (1, 2, 63, 64, 65, 130)          # a block takes 4 rows of 64 columns
SHAPES = [(H, W) for a, H in enumerate(TILE_H) for b, W in enumerate(TILE_W) if (a + b) % 2 == 0] + [(5, 65), (9, 130), (4, 64)]
FLAT_SHAPES = SHAPES + [(5, 51), (1, 257)]                          # a flat grid takes 256 pixels: h w = 255, 256 (4 x 64), 257


def values(shape, seed, kind, lo=-16.0, hi=16.0):
    """"float": uniform fp32 in [lo, hi); "dyadic": multiples of 1/8 there, whose sums are exact in any order"""
    v = lo + (hi - lo) * torch.rand(shape, generator=gen(seed))
    return torch.round(v * 8) / 8 if kind == "dyadic" else v


# ------------------------------------------------------------------------------------------------ flow_boxavg
BOXAVG_K, BOXAVG_BC = (1, 3, 11), ((1, 1), (1, 2), (3, 2))          # B C = 1, 2, 6; B = 3 gives `valid` a batch stride
# (k, (B, C), with valid, negate, kind of values)
BOXAVG_PARAMS = [(k, bc, bool((a + b + c) % 2), bool((a + c) % 2), cyc(("float", "dyadic"), b + c))
                 for a, k in enumerate(BOXAVG_K) for b, bc in enumerate(BOXAVG_BC) for c in range(2)]
BOXAVG_PARAMS += [(11, (3, 2), True, True, "float"), (3, (1, 1), False, False, "float"), (1, (3, 2), True, False, "dyadic"), (11, (1, 2), False, True, "float")]


def boxavg_inputs(H, W, B, C, with_valid, kind, seed):
    flow = values((B, C, H, W), seed, kind)
    valid = (torch.rand(B, 1, H, W, generator=gen(seed + 1)) > 0.3).float() if with_valid else None
    return flow, valid


def boxavg_ref(flow, valid, k, negate):
    """preprocess() of the oracle with the grid size whose window is k (min(g, g) // 2 * 2 - 1 == k for g = k + 1)"""
    return otp.preprocess(flow.clone(), valid, True, not negate, k + 1, k + 1)


def boxavg_inorder(flow, valid, k, negate, defect=None):
    """flow_boxavg_kernel: the zero-padded window added row by row, / k^2, negated, * valid.  defect "x_short": the bounds test x < W - 1"""
    B, C, H, W = flow.shape
    r = (k - 1) // 2
    src = flow.clone()
    if defect == "x_short":
        src[..., W - 1] = 0.0
    P = F.pad(src, (r, r, r, r))
    s = torch.zeros_like(flow)
    for dy in range(k):
        for dx in range(k):
            s = s + P[..., dy:dy + H, dx:dx + W]
    v = s / float(k * k)
    v = -v if negate else v
    return v * valid if valid is not None else v


# ------------------------------------------------------------------------------------------------ sobel_magnitude
SOBEL_C = (1, 3, 4)


def sobel_inputs(H, W, C, seed):
    """uint8-like content on even seeds, plain fp32 on odd ones.  With C = 1 always uint8-like: groups = C = 1 is no depthwise convolution,
    torch hands it to another backend whose tap order is not the kernel's, and integer taps sum to the same bits in any order"""
    x = 255.0 * torch.rand(1, C, H, W, generator=gen(seed))
    return x.round() if seed % 2 == 0 or C == 1 else x


def sobel_ref(img):
    return otp.sobel_magnitude(img)[0, 0]


def sobel_inorder(img, defect=None):
    """sobel_mag_kernel: nine taps in row-major order per channel, |.| summed over the channels in order, / C, the two sums added"""
    _, C, H, W = img.shape
    kx = (-1., 0., 1., -2., 0., 2., -1., 0., 1.)
    ky = (-1., -2., -1., 0., 0., 0., 1., 2., 1.)
    src = img.clone()
    if defect == "y_short":
        src[..., H - 1, :] = 0.0
    P = F.pad(src[0], (1, 1, 1, 1))
    sx = sy = None
    for c in range(C):
        gx, gy = torch.zeros(H, W), torch.zeros(H, W)
        for t in range(9):
            v = P[c, t // 3:t // 3 + H, t % 3:t % 3 + W]
            gx, gy = gx + kx[t] * v, gy + ky[t] * v
        sx = gx.abs() if c == 0 else sx + gx.abs()
        sy = gy.abs() if c == 0 else sy + gy.abs()
    return (sx / float(C)).abs() + (sy / float(C)).abs()


# ------------------------------------------------------------------------------------------------ minmax_filter
MINMAX_K, MINMAX_PLANES = (1, 5, 11), (1, 4)


def minmax_inputs(H, W, planes, seed):
    """random values with plateaus of equal ones (a binary mask on every other plane, as the pipeline's erode / dilate sees)"""
    x = values((planes, H, W), seed, "float", -3.0, 3.0)
    x[1::2] = (x[1::2] > -1.0).float()
    return x


def minmax_ref(x, k, is_max, axis):
    """one pass of the filter: F.max_pool2d over (1, k) (axis 0: along x) or (k, 1) with the window clipped to the image"""
    p = k // 2
    y = x if is_max else -x
    r = F.max_pool2d(F.pad(y[None], (p, p, 0, 0) if axis == 0 else (0, 0, p, p), value=-INF), (1, k) if axis == 0 else (k, 1), stride=1)[0]
    return r if is_max else -r


def minmax_sim(x, k, is_max, axis, defect=None):
    """minmax_filter_kernel tap by tap.  defect "no_clip": a tap is skipped only when it leaves the plane's memory, not its row / column"""
    P, H, W = x.shape
    flat = x.reshape(P, H * W)
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    v = torch.full((P, H, W), -INF if is_max else INF)
    for d in range(-(k // 2), k // 2 + 1):
        xx, yy = (xs + d, ys) if axis == 0 else (xs, ys + d)
        idx = yy * W + xx
        ok = (idx >= 0) & (idx < H * W) if defect == "no_clip" else (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        t = flat[:, idx.clamp(0, H * W - 1).reshape(-1)].reshape(P, H, W)
        t = torch.where(ok[None], t, v)
        v = torch.maximum(v, t) if is_max else torch.minimum(v, t)
    return v


# ------------------------------------------------------------------------------------------------ box_sum_cmp
# (k, pad, dh): the output domain is (H + dh) x (W + dh).  pad = k // 2 throughout (dilate_thin_area's geometry): an odd k gives H rows, an
# even k gives H + 1, which the erosion keeps (dh = 1) and the dilations crop (dh = 0; dh = -1 when their input is the erosion's H + 1 rows)
BOX_GEOM = [(3, 1, 0), (7, 3, 0), (8, 4, 1), (8, 4, 0), (8, 4, -1), (16, 8, 1), (16, 8, 0), (16, 8, -1)]
BOX_KINDS = ("mask", "sparse", "dyadic")


def box_inputs(H, W, kind, seed):
    """"mask": ones with a few zeros and a fractional band (sum == k k decides); "sparse": a few tenths on zeros, whose window sums come
    close to 1 (sum >= 1 is decided by the rounding of the row-major sum); "dyadic": multiples of 1/8"""
    g = gen(seed)
    if kind == "mask":
        m = (torch.rand(H, W, generator=g) > 0.03).float()
        m[:, W // 3:W // 3 + 2] = torch.rand(H, min(2, W - W // 3), generator=g)
        return m
    if kind == "sparse":
        tenths = torch.randint(1, 6, (H, W), generator=g).float() * 0.1
        return torch.where(torch.rand(H, W, generator=g) < 0.06, tenths, torch.zeros(H, W))
    return values((H, W), seed, "dyadic", 0.0, 1.0)


def box_kinds(k, cmp):
    """the raw sum (cmp 0) of a 3 x 3 box on fractional values is the one place where torch's convolution does not add row by row (the CPU
    file shows it does everywhere else in the table); there the inputs are the dyadic ones, whose sum has the same bits in any order"""
    return ("dyadic",) if (k == 3 and cmp == 0) else BOX_KINDS


def box_cmp(s, k, cmp):
    return s if cmp == 0 else ((s == float(k * k)).float() if cmp == 1 else (s >= 1.0).float())


def box_ref(x, k, pad, Ho, Wo, cmp):
    """F.conv2d(x, ones(k, k), padding=pad) cropped to the output domain, then the comparison of dilate_thin_area"""
    s = F.conv2d(x[None, None], torch.ones(1, 1, k, k), padding=pad)[0, 0]
    assert s.shape[0] >= Ho and s.shape[1] >= Wo, (tuple(s.shape), Ho, Wo)
    return box_cmp(s[:Ho, :Wo], k, cmp)


def box_inorder(x, k, pad, Ho, Wo, cmp, defect=None):
    """box_sum_cmp_kernel: k x k taps added row by row from the zero-padded plane.  defect "x_short": the bounds test xx < W - 1"""
    H, W = x.shape
    src = x.clone()
    if defect == "x_short":
        src[:, W - 1] = 0.0
    P = F.pad(src, (pad, max(0, Wo + k - 1 - W - pad), pad, max(0, Ho + k - 1 - H - pad)))
    s = torch.zeros(Ho, Wo)
    for dy in range(k):
        for dx in range(k):
            s = s + P[dy:dy + Ho, dx:dx + Wo]
    return box_cmp(s, k, cmp)


def box_cases(H, W):
    """every geometry whose output domain exists at this input size: (k, pad, Ho, Wo)"""
    return [(k, pad, H + dh, W + dh) for k, pad, dh in BOX_GEOM if H + dh >= 1 and W + dh >= 1]


# ------------------------------------------------------------------------------------------------ elementwise stages
NEAR_255 = (-0.5, -1e-6, 0.0, 1e-6, 0.99999994, 254.99998, 255.0, 255.00002, 300.0)
NEAR_3 = (0.0, 2.9999998, 3.0, 3.0000002, 100.5, 255.0, 256.75, -0.25)
NEAR_HALF = (0.0, 1.0, 0.5, 0.49999997, 0.50000006, 0.3, 1.0, 0.0)


def pick(palette, shape, seed, noise=0.0):
    """every element one of `palette`; with `noise`, that share of them a plain random value in [0, 255) instead"""
    g = gen(seed)
    v = torch.tensor(palette, dtype=torch.float32)[torch.randint(0, len(palette), shape, generator=g)]
    if noise:
        v = torch.where(torch.rand(shape, generator=g) < noise, 255.0 * torch.rand(shape, generator=g), v)
    return v


def binary(shape, seed, p=0.5):
    return (torch.rand(shape, generator=gen(seed)) < p).float()


def mask_inv_inputs(H, W, C, seed):
    """channel values from {0, 1/4, .., 1} (means land on 0.5 exactly) on even seeds, near-0.5 fp32 values on odd ones"""
    if seed % 2 == 0:
        return torch.randint(0, 5, (1, C, H, W), generator=gen(seed)).float() / 4
    return 0.5 + 0.02 * (torch.rand(1, C, H, W, generator=gen(seed)) - 0.5)


def mask_inv_ref(wm):
    return 1.0 - (wm.mean(dim=1, keepdim=True) >= 0.5).float()


def mask_inv_inorder(wm):
    s = wm[:, 0:1]
    for c in range(1, wm.shape[1]):
        s = s + wm[:, c:c + 1]
    return 1.0 - ((s / float(wm.shape[1])) >= 0.5).float()


def mix_blend_inputs(H, W, seed):
    """(tps3, inv_clean, final_warp3, output1_3, mask1_3): final_warp on both sides of 3.0, mask1 means on both sides of 0.5, values just
    under and over 0 and 255, and pixels with mask1 + mixmask == 0 (mask1 = 0 where the homography mask is cleaned away and final_warp < 3)"""
    s = (1, 3, H, W)
    tps, o1 = pick(NEAR_255, s, seed, 0.5), pick(NEAR_255, s, seed + 1, 0.5)
    fw, m1 = pick(NEAR_3, s, seed + 2, 0.3), pick(NEAR_HALF, s, seed + 3)
    inv_clean = binary((1, 1, H, W), seed + 4)
    dead = binary((1, 1, H, W), seed + 5, 0.2).bool().expand(s)           # no image anywhere: 0 / 0
    fw, m1 = torch.where(dead, torch.zeros(s), fw), torch.where(dead, torch.zeros(s), m1)
    inv_clean = torch.where(dead[:, :1], torch.ones(1, 1, H, W), inv_clean)
    return tps, inv_clean, fw, o1, m1


def to_u8(x):
    """clip(0, 255), NaN (0 / 0) -> 0, truncation: the CPU cast of the reference"""
    return torch.nan_to_num(x.clip(0, 255), nan=0.0).to(torch.uint8)


def mix_blend_ref(tps, inv_clean, fw, o1, m1):
    """oracle.tps_pipeline.tps_H_warp from `tps = tps * tmask` to the blend -> (tps, tmask, mix, mixmask, blend uint8, the raw quotient)"""
    tmask = 1.0 - inv_clean
    tps = tps * tmask
    fmask = ((fw >= 3).float().mean(dim=1, keepdim=True) >= 0.5).float()
    inv1 = ((1 - m1).float().mean(dim=1, keepdim=True) >= 0.5).float()
    mix = fw * fmask + tps * (1 - fmask) * inv1
    mix_mask = fmask + (1 - fmask) * tmask * inv1
    output2 = mix * mix_mask
    raw = (o1 * m1 + output2 * mix_mask) / (m1 + mix_mask)
    return tps, tmask, output2, mix_mask, to_u8(raw), raw


def mix_blend_means_inorder(fw, m1):
    """the two channel means as tps_mix_blend_kernel adds them: ((c0 + c1) + c2) / 3"""
    f = (fw >= 3).float()
    i = 1.0 - m1
    return (((f[:, 0] + f[:, 1]) + f[:, 2]) / 3.0 >= 0.5).float()[:, None], (((i[:, 0] + i[:, 1]) + i[:, 2]) / 3.0 >= 0.5).float()[:, None]


def plane_op_inputs(n, op, seed):
    a = pick((0.0, 1.0, 0.5, 0.05, 0.050000004, 0.049999997, 1.5, -0.5), (n,), seed)
    b = pick((0.0, 1.0, 0.5, 2.0, -1.0, 0.99999994), (n,), seed + 1)
    return a, b


def plane_op_ref(a, b, op, thr=0.05):
    """dilate_thin_area's middle (op 0), its end with dilate_mask's uint8 truncation (op 1), torch.where(a > thr, 1, 0) (op 2)"""
    if op == 0:
        thick = (a * b).clamp(0, 1)
        return thick, a * (1 - thick)
    if op == 1:
        r = (a + b).clamp(0, 1)
        return r, (r >= 1).float()
    return (a > thr).float(), None


def stage_inputs(H, W, seed):
    """(fw3, occ, m1_3, tps3, tmask, o1_3): images 0..255, mask1 around 0.5 and fractional, binary occlusion and TPS masks"""
    s = (1, 3, H, W)
    return (pick(NEAR_255, s, seed, 0.6), binary((1, 1, H, W), seed + 1, 0.7), pick(NEAR_HALF, s, seed + 2), pick(NEAR_255, s, seed + 3, 0.6),
            binary((1, 1, H, W), seed + 4, 0.7), pick(NEAR_255, s, seed + 5, 0.6))


def stage_a_ref(fw, occ, m1, tps, tm, method):
    """first lines of mix_all_img1_with_inpaint (method 0) / mix_inpaint_all_area (1) -> (tfw, tfwm, channel 0 of the area mask)"""
    if method == 0:
        inv = 1. - torch.where(m1 > 0.5, torch.ones_like(m1), torch.zeros_like(m1))
        tfw, tfwm = fw * occ * m1 + tps * inv, occ * m1 + tm * inv
        return tfw, tfwm, ((1. - tfwm) * m1)[:, 0:1]
    inv = 1. - m1
    tfw, tfwm = fw * occ + tps * inv, occ + tm * inv
    return tfw, tfwm, ((1. - tfwm) * m1 * tm)[:, 0:1]


def stage_b_ref(iam, dil, m1, tfw, o1):
    """mix_all_img1_with_inpaint: border, by1, inpaint_img_by_only_img1 and channel 0 of (1 - by1) * border"""
    border = torch.abs(iam - dil)
    by1 = (1 - border) * dil * m1
    return tfw * (1 - by1) + (o1 * by1) * by1, ((1. - by1) * border)[:, 0:1]


def mul_mask_ref(img, mask, invert, clip):
    v = img.clip(0, 255) if clip else img
    return v if mask is None else v * ((1 - mask) if invert else mask)


def blend_pair_inputs(H, W, c2, seed):
    """mask1 = mask2 = 0 on a fifth of the pixels (0 / 0), values just under and over 0 and 255"""
    s = (1, 3, H, W)
    o1, o2 = pick(NEAR_255, s, seed, 0.5), pick(NEAR_255, s, seed + 1, 0.5)
    m1, m2 = pick(NEAR_HALF, s, seed + 2), pick(NEAR_HALF, (1, c2, H, W), seed + 3)
    dead = binary((1, 1, H, W), seed + 4, 0.2).bool()
    return o1, torch.where(dead.expand(s), torch.zeros(s), m1), o2, torch.where(dead.expand(1, c2, H, W), torch.zeros(1, c2, H, W), m2)


def blend_pair_ref(o1, m1, o2, m2):
    raw = (o1 * m1 + o2 * m2) / (m1 + m2)
    return to_u8(raw), raw


GATHER_P, GATHER_N = (1, 3), (1, 255, 257)


def gather_inputs(H, W, P, n, seed):
    """planes [P, H, W] and n points (x, y) int32: the four corners, points one step and far outside each edge, random ones inside"""
    g = gen(seed)
    planes = 1.0 + torch.rand(P, H, W, generator=g)                    # nothing inside is 0: an outside point is told apart
    pts = torch.stack([torch.randint(0, W, (n,), generator=g), torch.randint(0, H, (n,), generator=g)], 1)
    special = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (-1, 0), (W, 0), (0, -1), (0, H), (W, H - 1), (W - 1, H), (-1, -1), (1 << 20, 0),
               (0, -(1 << 20)), (W - 1 + W, 0), (-W, H - 1)]
    if n == 1:
        pts[0] = torch.tensor((W - 1, H - 1))
    else:
        for i, p in enumerate(special):
            pts[(i * 17 + 3) % n] = torch.tensor(p)
    return planes, pts.int()


def gather_ref(planes, pts):
    P, H, W = planes.shape
    x, y = pts[:, 0].long(), pts[:, 1].long()
    ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    v = planes[:, y.clamp(0, H - 1), x.clamp(0, W - 1)].t()
    return torch.where(ok[:, None], v, torch.zeros_like(v))


# ================================================================================================ 2. range_argmax
ARGMAX_PLANES = ((9, 65), (40, 130), (3, 260))      # the third only for the 1 x 257 window: 257 is prime and no window of the first two has it
# name -> (x1, y1, x2, y2): rows [y1 - 2, y2 + 2) x cols [x1 - 2, x2 + 2), clipped at the right and the bottom; every x1, y1 >= 2
ARGMAX_WINDOWS = {
    (9, 65): dict(one=(5, 4, 2, 1), n255=(4, 3, 51, 4), n256=(2, 3, 62, 3), full=(2, 2, 63, 7), clip_right=(50, 4, 90, 5), clip_bottom=(6, 7, 20, 30),
                  clip_both=(60, 8, 70, 12), origin=(2, 2, 9, 3), empty_cols=(50, 3, 46, 6), empty_rows=(5, 8, 30, 4), past_right=(70, 3, 80, 5)),
    (40, 130): dict(one=(5, 4, 2, 1), n255=(10, 6, 91, 5), n256=(10, 6, 70, 6), full=(2, 2, 128, 38), several=(7, 5, 100, 20), clip_right=(100, 10, 200, 12),
                    clip_bottom=(6, 30, 20, 60), clip_both=(98, 28, 140, 50), origin=(2, 2, 40, 9), empty_cols=(50, 10, 46, 12),
                    empty_rows=(5, 20, 30, 16), last_pixel=(131, 41, 131, 41)),
    (3, 260): dict(n255=(2, 3, 253, 0), n256=(2, 3, 254, 0), n257=(2, 3, 255, 0), full=(2, 2, 258, 1)),
}
# planted ties: (plane, window name, elements (row-major within the window) that share the maximum); None: the whole window is equal
ARGMAX_TIES = [((40, 130), "full", (300, 301)), ((40, 130), "full", (17, 17 + 256)), ((40, 130), "full", (63, 64)), ((40, 130), "full", (127, 128)),
               ((40, 130), "full", (0, 5199)), ((40, 130), "full", (5, 256)), ((40, 130), "several", (255, 256)), ((40, 130), "several", (1, 1 + 512)),
               ((9, 65), "full", (63, 64)), ((9, 65), "full", (127, 128)), ((9, 65), "full", (0, 584)), ((9, 65), "full", (70, 70 + 256)),
               ((9, 65), "n256", (0, 255)), ((3, 260), "n257", (0, 256)), ((3, 260), "n257", (255, 256)), ((9, 65), "one", (0,)),
               ((40, 130), "origin", (0,)), ((9, 65), "origin", (0, 1)), ((40, 130), "full", None), ((9, 65), "n255", None)]
ARGMAX_LAUNCH = (1, 70)


def window(rng, H, W):
    x1, y1, x2, y2 = rng
    return x1 - 2, min(x2 + 2, W), y1 - 2, min(y2 + 2, H)          # xa, xb, ya, yb


def window_size(rng, H, W):
    xa, xb, ya, yb = window(rng, H, W)
    return max(xb - xa, 0) * max(yb - ya, 0)


def argmax_ref(grad, ranges):
    """advanced_uniform_sample_border_points' inner statement for every range: the flat index torch.argmax returns"""
    g = grad[None, None]
    out = []
    for (x1, y1, x2, y2) in ranges:
        mask = torch.zeros_like(g)
        mask[:, :, y1 - 2:y2 + 2, x1 - 2:x2 + 2] = 1
        rg = g * mask + (-1 * torch.ones_like(g)) * (1 - mask)
        out.append(int(torch.argmax(rg)))
    return out


def argmax_sim(grad, rng, defect=None):
    """range_argmax_kernel thread for thread.  defects: "ge": `v >= best` in the stride loop (the later of two equal elements of one thread);
    "no_tie_reduce": the tree keeps the lower thread on a tie, not the lower index; "no_sentinel": an empty window returns the sentinel"""
    g = grad.numpy()
    H, W = g.shape
    xa, xb, ya, yb = window(rng, H, W)
    ww, hh = xb - xa, yb - ya
    sb, si = np.full(256, -2.0, np.float32), np.full(256, 0x7fffffff, np.int64)
    if ww > 0 and hh > 0:
        for t in range(min(256, ww * hh)):
            for e in range(t, ww * hh, 256):
                yy, xx = ya + e // ww, xa + e % ww
                v, idx = g[yy, xx], yy * W + xx
                if v > sb[t] or (v == sb[t] and (defect == "ge" or idx < si[t])):
                    sb[t], si[t] = v, idx
    s = 128
    while s > 0:
        for t in range(s):
            if sb[t + s] > sb[t] or (defect != "no_tie_reduce" and sb[t + s] == sb[t] and si[t + s] < si[t]):
                sb[t], si[t] = sb[t + s], si[t + s]
        s >>= 1
    return int(si[0]) if (si[0] != 0x7fffffff or defect == "no_sentinel") else 0


def argmax_plane(H, W, seed, quantised):
    """a gradient-magnitude plane (>= 0); quantised: one of five levels per pixel, so that every window holds its maximum many times"""
    g = gen(seed)
    return torch.randint(0, 5, (H, W), generator=g).float() / 4 if quantised else torch.rand(H, W, generator=g)


def argmax_planted(plane, name, elems, seed):
    """(grad, range, the flat index that must win): distinct random values below 1 and the value 2 at `elems` of the window; elems None: all equal
    (0.75 on even seeds, 0 on odd ones)"""
    H, W = plane
    rng = ARGMAX_WINDOWS[plane][name]
    xa, xb, ya, yb = window(rng, H, W)
    ww = xb - xa
    if elems is None:
        grad = torch.full((H, W), 0.75 if seed % 2 == 0 else 0.0)
        grad[ya:yb, xa:xb] = 0.5 if seed % 2 == 0 else 0.0            # the frame of the window is LARGER: leaving the window shows
        return grad, rng, ya * W + xa
    grad = torch.rand(H, W, generator=gen(seed)) * 0.9
    for e in elems:
        assert e < ww * (yb - ya), (plane, name, e)
        grad[ya + e // ww, xa + e % ww] = 2.0
    e = min(elems)
    return grad, rng, (ya + e // ww) * W + xa + e % ww


def argmax_ranges(plane, count):
    """`count` ranges cycling through the plane's windows"""
    w = list(ARGMAX_WINDOWS[plane].values())
    return [w[i % len(w)] for i in range(count)]


# ================================================================================================ 3. TPS solves
SOLVE_N = (3, 4, 5, 64, 134, 135, 141, 142, 253, 254, 300)
SOLVE_MODES = (0, 1)
OTHER_N = (20, 134, 135, 254)
PIXELS = 200.0                                        # mode 1 works in pixel units
LDS_MAX_N = 134                                       # (n + 3)(n + 5) 8 <= 150 KiB


def lds_limit():
    return max(n for n in range(3, 400) if (n + 3) * (n + 5) * 8 <= 150 * 1024)


def control_points(n):
    """n cells of a ceil(sqrt n)^2 grid in the unit square, each point at its cell centre +- 0.3 cell; targets = sources +- 0.02.  fp32 [n, 2]"""
    g = gen(7000 + n)
    m = math.ceil(math.sqrt(n))
    cells = torch.randperm(m * m, generator=g)[:n]
    centre = torch.stack([cells % m, cells // m], 1).double() + 0.5
    src = (centre + 0.6 * (torch.rand(n, 2, generator=g, dtype=torch.float64) - 0.5)) / m
    tgt = src + 0.04 * (torch.rand(n, 2, generator=g, dtype=torch.float64) - 0.5)
    return src.float(), tgt.float()


def _assemble(K, P, rhs):
    """[[K, P], [P^T, 0]] and [rhs; 0] in K's dtype"""
    n = K.shape[0]
    L = torch.zeros(n + 3, n + 3, dtype=K.dtype)
    L[:n, :n], L[:n, n:], L[n:, :n] = K, P, P.t()
    return L, torch.cat([rhs.to(K.dtype), torch.zeros(3, 2, dtype=K.dtype)], 0)


def system_kornia(src, dst):
    """mode 0: kornia's get_tps_transform(points_src = src, points_dst = dst) as the oracle builds it in fp32: K_ij = U(src_i, dst_j),
    P = [1, src], right-hand side dst"""
    K = otp._kernel_distance(otp._pair_square_euclidean(src[None], dst[None]))[0]
    return _assemble(K, torch.cat([torch.ones(len(src), 1), src], 1), dst)


def system_pixel(sites, vals, dtype):
    """mode 1: the U = d2 log(d2 + 1.19e-7) system of warp_by_tps_opencv_like at the fp32 sites, evaluated in `dtype`"""
    a = sites.to(dtype)
    d2 = ((a[:, None, :] - a[None, :, :]) ** 2).sum(-1)
    K = d2 * torch.log(d2 + 1.1920929e-7)
    return _assemble(K, torch.cat([torch.ones(len(a), 1, dtype=dtype), a], 1), vals)


def system_other(c_src, c_dst, dtype):
    """tests/_other_tps_ref.fit's system: U = r^2 ln(r + 1e-6) at the fp32 sites c_dst, right-hand side the fp32 difference c_src - c_dst"""
    c = c_dst.to(dtype)
    r = torch.sqrt((c[:, None, 0] - c[None, :, 0]) ** 2 + (c[:, None, 1] - c[None, :, 1]) ** 2)
    K = r * r * torch.log(r + OR.EPS)
    return _assemble(K, torch.cat([torch.ones(len(c), 1, dtype=dtype), c], 1), c_src - c_dst)


def rel_err(w, w64):
    """max |w - w64| / max |w64| over kernel and affine weights together"""
    return ((w.double() - w64).abs().max() / w64.abs().max()).item()


def solve_case(kind, n):
    """kind 0 / 1: the st_tps2_solve modes, "other": st_tps_other_solve.  -> dict(sites, centers, values: the entry's fp32 operands; w64: the
    fp64 solution [n + 3, 2] of the system the kernel builds; w32: the reference's own fp32 torch.linalg.solve; ctl = rel_err(w32);
    L32, rhs32: the fp32 system).  The kernels solve, in fp64, the system they build: st_tps2_solve builds its K in fp32 (tps2_u), so w64 is
    the fp64 solution of the fp32-built system in both of its modes; st_tps_other_solve builds K in fp64.  Mode 1 also carries w64_fp64_U,
    the solution with warp_by_tps_opencv_like's U evaluated in fp64.  It is not a reference for the elimination: rounding every entry of K
    (up to 1e5 in pixel units, cond 1e13 to 1e14) to fp32 moves the solution by 2e-4 to 4e-3 for n >= 64, as much as the fp32 solve's own
    error and a different draw with every libm, so a factor of 4 between the two is chance.  The GPU file records that distance."""
    src, tgt = control_points(n)
    if kind == 0:
        L32, r32 = system_kornia(src, tgt)
        L64, r64 = L32.double(), r32.double()                      # the SAME fp32 system, solved in fp64 (get_tps_transform(solve_dtype=float64))
        ops = dict(sites=src, centers=tgt, values=tgt)
    elif kind == 1:
        a, b = src * PIXELS, tgt * PIXELS
        L32, r32 = system_pixel(a, b, torch.float32)               # the U of warp_by_tps_opencv_like, evaluated in fp32 as tps2_u does
        L64, r64 = L32.double(), r32.double()                      # the same fp32-built system, solved in fp64
        Lu, ru = system_pixel(a, b, torch.float64)                 # that U evaluated in fp64: another system, see w64_fp64_U below
        ops = dict(sites=a, centers=a, values=b, w64_fp64_U=torch.linalg.solve(Lu, ru))
    else:
        L32, r32 = system_other(tgt, src, torch.float32)
        L64, r64 = system_other(tgt, src, torch.float64)
        ops = dict(sites=src, centers=src, values=tgt - src, c_src=tgt, c_dst=src)
    w64 = torch.linalg.solve(L64, r64)
    w32 = torch.linalg.solve(L32, r32)
    return dict(ops, n=n, w64=w64, w32=w32, ctl=rel_err(w32, w64), L32=L32, rhs32=r32, L64=L64, rhs64=r64)


def solve_bound(case):
    """the control rule: 4 x the fp32 reference's own error on the case, floored at one fp32 rounding"""
    return 4.0 * max(case["ctl"], FLOOR)


def gauss_jordan(L, rhs, defect=None, storage="work"):
    """tps_gauss_jordan in numpy fp64 on the system (L, rhs) [n + 3, n + 3], [n + 3, 2] -> (w float32 [n + 3, 2], status).
    storage "lds": the augmented matrix in a buffer of exactly (n + 3)(n + 5) doubles and the factors in a 144-entry array of their own;
    "work": both in one buffer of (n + 3)(n + 6) doubles, the factors behind the matrix (the caller's workspace).  Defects:
    "rows256": the factor loop stops at row 256 (no second stride trip); "swap256": the row swap covers the first 256 columns only."""
    n3 = L.shape[0]
    ld = n3 + 2
    if storage == "lds":
        assert n3 <= 144
        buf, fac = np.full(n3 * ld, np.nan), np.zeros(144)
    else:
        buf = np.full(n3 * (ld + 1), np.nan)
        fac = buf[n3 * ld:]
        fac[:] = 0.0
    work = buf[:n3 * ld].reshape(n3, ld)
    work[:, :n3], work[:, n3:] = np.asarray(L, np.float64), np.asarray(rhs, np.float64)
    pmin, pmax = 1e300, 0.0
    for c in range(n3):
        piv = c + int(np.argmax(np.abs(work[c:, c])))              # the first row on ties, as idamax
        bb = abs(work[piv, c])
        if not bb >= pmin:
            pmin = bb
        pmax = max(pmax, bb)
        if piv != c:
            k = 256 if defect == "swap256" else ld
            work[[c, piv], :k] = work[[piv, c], :k]
        pv = work[c, c]
        inv = 1.0 / (pv if pv != 0.0 else 1.0)
        rows = min(n3, 256) if defect == "rows256" else n3
        fac[:rows] = work[:rows, c] * inv
        if c < rows:
            fac[c] = 0.0
        work[:, c + 1:] -= fac[:n3, None] * work[c, None, c + 1:]
    d = np.diagonal(work)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = (work[:, n3:] / d[:, None]).astype(np.float32)
    status = 0 if (pmin == pmin and pmin > 1e-13 * pmax) else 1
    return torch.from_numpy(w), status, buf


def singular_sets(n, kind):
    """control points [n, 2] in the unit square with no unique spline: "dup": site n - 1 repeats site 0; "line": every site on one line"""
    src, tgt = control_points(n)
    if kind == "dup":
        src[n - 1] = src[0]
    else:
        t = (torch.arange(n, dtype=torch.float32) + 8) / 256          # multiples of 1 / 256: the line is exact in fp32, in both units
        assert float(t.max()) < 1
        src = torch.stack([t, 0.25 + 0.5 * t], 1)
        tgt = src + (tgt - control_points(n)[0])
    return src, tgt


# ================================================================================================ case iterators (both files run all of them)
THR = float(torch.tensor(0.05, dtype=torch.float32))              # the threshold of mix_all_img1_with_inpaint, as the fp32 the entry is handed
MASK_INV_C = (1, 3, 7)


def boxavg_cases(shape):
    H, W = shape
    i = SHAPES.index(shape)
    for j, (k, (B, C), wv, neg, kind) in enumerate(BOXAVG_PARAMS):
        yield (k, B, C, wv, neg, kind), boxavg_inputs(H, W, B, C, wv, kind, 1000 + 50 * i + 2 * j), k, neg


def sobel_cases(shape):
    H, W = shape
    i = SHAPES.index(shape)
    for a, C in enumerate(SOBEL_C):
        for s in (0, 1):
            yield (C, s), sobel_inputs(H, W, C, 2000 + 8 * i + 2 * a + s)


def minmax_cases(shape):
    H, W = shape
    i = SHAPES.index(shape)
    for a, planes in enumerate(MINMAX_PLANES):
        x = minmax_inputs(H, W, planes, 3000 + 4 * i + a)
        for k in MINMAX_K:
            for is_max in (0, 1):
                for axis in (0, 1):
                    yield (planes, k, is_max, axis), x


def box_cases_of(shape):
    """(tag, x, k, pad, Ho, Wo, cmp) for every geometry, comparison and kind of input of one input size"""
    H, W = shape
    i = SHAPES.index(shape)
    planes = {kind: box_inputs(H, W, kind, 4000 + 4 * i + a) for a, kind in enumerate(BOX_KINDS)}
    for (k, pad, Ho, Wo) in box_cases(H, W):
        for cmp in (0, 1, 2):
            for kind in box_kinds(k, cmp):
                yield (kind, k, pad, Ho, Wo, cmp), planes[kind], k, pad, Ho, Wo, cmp


def mask_inv_cases(shape):
    H, W = shape
    i = FLAT_SHAPES.index(shape)
    for a, C in enumerate(MASK_INV_C):
        for s in (0, 1):
            yield (C, s), mask_inv_inputs(H, W, C, 5000 + 8 * i + 2 * a + s)


def flat_seed(shape, base):
    return base + 16 * FLAT_SHAPES.index(shape)


# ================================================================================================ 5. Telea inpainting at deep rings
# name -> (H, W, radius, known set as (rows, cols) slices, rings checked in full)
TELEA_CASES = {
    "window_r88": (160, 160, 88, (slice(0, 4), slice(0, 4)), tuple(range(120, 137)) + tuple(range(248, 265))),
    "wrap_r64": (96, 400, 64, (slice(None), slice(0, 4)), ()),
    "strip": (3, 1300, 3, (slice(0, 1), slice(0, 1)), None),           # None: every pixel
    "strip_t": (1300, 3, 3, (slice(0, 1), slice(0, 1)), None),
}


def telea_fill(name):
    """the hole of a case: everything but its known block"""
    H, W, _, (rows, cols), _ = TELEA_CASES[name]
    fill = np.ones((H, W), bool)
    fill[rows, cols] = False
    return fill


def tag_before(d_q, k, defect=None):
    """inpaint.hip's before(): the packed word keeps d mod 256 and the signed 8-bit difference to the ring index decides `d(q) < k`.
    defect "unwrapped": the tag compared with k as it stands"""
    tag = np.asarray(d_q, np.int64) & 0xff
    if defect == "unwrapped":
        return tag - k < 0
    return ((tag - k) & 0xff).astype(np.uint8).view(np.int8) < 0


def ring_hist_sim(d, nb, split=1024, slots=1024):
    """ring_hist_kernel per 256-pixel block: bins below `split` in a `slots`-entry LDS histogram (a write past it is lost), the others by
    global atomics, then the first min(nb, 1024) LDS bins added to the counts"""
    d = np.asarray(d).reshape(-1)
    counts = np.zeros(nb, np.int64)
    for b0 in range(0, d.size, 256):
        h = np.zeros(slots, np.int64)
        for k in d[b0:b0 + 256]:
            if k < nb:
                if k < split:
                    if k < slots:
                        h[k] += 1
                else:
                    counts[k] += 1
        m = min(nb, 1024, slots)
        counts[:m] += h[:m]
    return counts


def ring_scan_sim(counts, nb, one_bucket=False):
    """ring_scan_kernel: 1024 threads, ceil(nb / 1024) buckets each -> offsets [nb + 1] (exclusive prefix sum of counts[1:]).
    defect one_bucket: every thread takes one bucket whatever nb is"""
    per = 1 if one_bucket else (nb + 1023) // 1024
    part = np.zeros(1024, np.int64)
    for t in range(1024):
        part[t] = sum(int(counts[k]) for k in range(t * per, min(t * per + per, nb)) if k > 0)
    incl = np.cumsum(part)
    offsets = np.full(nb + 1, -1, np.int64)
    for t in range(1024):
        run = int(incl[t - 1]) if t else 0
        for k in range(t * per, min(t * per + per, nb)):
            offsets[k] = run
            run += int(counts[k]) if k > 0 else 0
    offsets[nb] = incl[1023]
    return offsets


# ================================================================================================ 4. tps2_warp
import _geom_bounds as gb  # noqa: E402

WARP_HW, WARP_C, WARP_N = ((2, 2), (4, 64), (5, 65), (9, 130)), (1, 4), (1, 6, 135, 3800)
WARP_SCALES = ((1.0, 1.0), (1.25, 0.9), (0.5, 1.1))                 # (kernel_scale, affine_scale)
WARP_MODES = (0, 1, 3)
# (n, (H, W), C, (kernel_scale, affine_scale), align_corners, image): every n at every size; C, the scales, the alignment and the image cycle
WARP_CASES = [(n, hw, cyc(WARP_C, a + b + 1), cyc(WARP_SCALES, a + 2 * b + 1), (a + b // 2) % 2, cyc(("ramps", "random"), a + b))
              for a, n in enumerate(WARP_N) for b, hw in enumerate(WARP_HW)]


def warp_image(C_, H, W, kind, seed):
    """"ramps": planes x, y, x + 1/4, y + 1/4 ...: wherever all four taps are inside, the output IS the sampled position;
    "random": seeded values in [0, 255) with fractions"""
    if kind == "ramps":
        px, py = gb.pixel_xy(H, W, torch.float32)
        return torch.stack([(px if c % 2 == 0 else py) + 0.25 * (c // 2) for c in range(C_)]).reshape(1, C_, H, W)
    return 255.0 * torch.rand(1, C_, H, W, generator=gen(seed))


def smooth_points(n):
    """the sources of control_points(n) moved by a smooth field of amplitude 0.02: the warp cases want a spline that bends, not one that folds
    (neighbouring sites of the jittered grid pulled apart by independent targets make weights whose fp32 evaluation error hides everything)"""
    src = control_points(n)[0].double()
    x, y = src[:, 0], src[:, 1]
    tgt = src + 0.02 * torch.stack([torch.sin(3 * x + 1) * torch.cos(2 * y), torch.cos(2 * x) * torch.sin(3 * y + 2)], 1)
    return src.float(), tgt.float()


def warp_stairs(C_, H, W):
    """the image of the quantised mode: levels that change by 1 every 32 columns (plane 3: and every 8 rows), with a fraction for the truncation of the
    taps to remove, around 0 on plane 2 and around 255 on plane 1 for the clamp of the taps.  The pixel-unit spline places a sample to about
    1e-4 of the image side in fp32, so on an image with a gradient everywhere (the ramps, the random one) more than 1 % of the values lie
    within that error of a .5 boundary; here only samples next to a level change do"""
    px, py = gb.pixel_xy(H, W, torch.float32)
    sx, sy = torch.floor(px / 32), torch.floor(py / 8)
    planes = [sx + 0.7, torch.full_like(sx, 300.5), sx - 2.0 + 0.5, sx + sy + 0.2]
    return torch.stack([planes[c % 4] for c in range(C_)]).reshape(1, C_, H, W)


def warp_weights(n, H, W, mode, seed):
    """(centers [n, 2], kw [n, 2], aw [3, 2]) fp32.  n = 6, 135: the fp64 solution for smooth_points(n) (normalised mesh units in
    mode 0, pixels of this image in mode 1 / 3), rounded to fp32.  n = 1 has no unique spline and n = 3800 is the entry's limit (60 800 B of
    LDS), not a fit: seeded centres over the mesh, small seeded kernel weights (about 1e-4 in mesh units) and a near-identity affine part."""
    pix = mode != 0
    S = float(max(H, W) - 1)
    if n in (6, 135):
        src, tgt = smooth_points(n)
        if pix:
            box = torch.tensor([W - 1.0, H - 1.0])
            a, b = src * box, tgt * box
            L, r = system_pixel(a, b, torch.float64)
            centers = a
        else:
            a, b = 2 * src - 1, 2 * tgt - 1
            L, r = system_kornia(a, b)
            L, r, centers = L.double(), r.double(), b
        w = torch.linalg.solve(L, r).float()
        return centers.contiguous(), w[:n].contiguous(), w[n:].contiguous()
    g = gen(seed)
    u = torch.rand(n, 2, generator=g)
    centers = u * torch.tensor([W - 1.0, H - 1.0]) if pix else 2 * u - 1
    kw = torch.randn(n, 2, generator=g) * ((1e-2 if n == 1 else 1e-4) / (max(S * S, 1.0) if pix else 1.0))
    aw = torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]) + torch.randn(3, 2, generator=g) * torch.tensor([[0.3 if pix else 0.02], [0.02], [0.02]])
    return centers, kw, aw


def warp_u(cx, cy, centers, mode):
    """U(coord, centre) [N, n] in the dtype of cx: kornia's clamp(-2 a.b + |a|^2 + |b|^2, 0), 0.5 d2 log(d2 + 1e-8) (mode 0); the pixel-unit
    d2 log(d2 + 1.19e-7) (mode 1)"""
    bx, by = centers[:, 0].to(cx.dtype), centers[:, 1].to(cx.dtype)
    if mode == 1:
        d2 = (cx[:, None] - bx[None]) ** 2 + (cy[:, None] - by[None]) ** 2
        return d2 * torch.log(d2 + 1.1920929e-7)
    d2 = (-2 * (cx[:, None] * bx[None] + cy[:, None] * by[None]) + (cx * cx + cy * cy)[:, None] + (bx * bx + by * by)[None]).clamp(min=0)
    return 0.5 * d2 * torch.log(d2 + 1e-8)


def warp_positions(H, W, centers, kw, aw, kscale, ascale, align, mode, dtype, inorder=False):
    """pixel positions (ix, iy) [H W] every output pixel samples at, in `dtype` (mode 3 samples where mode 1 does).  inorder: the kernel sum
    added centre by centre (tps2_warp_kernel's loop), not by torch's reduction"""
    mode &= 1
    px, py = gb.pixel_xy(H, W, dtype)
    if mode == 1:
        cx, cy = px, py
    else:
        cx, cy = (px / (W - 1) - 0.5) * 2, (py / (H - 1) - 0.5) * 2
    sw = (kw * kscale).to(dtype) if dtype == torch.float32 else kw.double() * kscale
    sa = (aw * ascale).to(dtype) if dtype == torch.float32 else aw.double() * ascale
    U = warp_u(cx, cy, centers, mode)
    if inorder:
        kx, ky = torch.zeros_like(cx), torch.zeros_like(cx)
        for i in range(centers.shape[0]):
            kx, ky = kx + U[:, i] * sw[i, 0], ky + U[:, i] * sw[i, 1]
    else:
        kx, ky = U @ sw[:, 0], U @ sw[:, 1]
    gx = (kx + (cx * sa[1, 0] + cy * sa[2, 0])) + sa[0, 0]
    gy = (ky + (cx * sa[1, 1] + cy * sa[2, 1])) + sa[0, 1]
    if mode == 1:
        return gx, gy
    if align:
        return ((gx + 1) / 2) * (W - 1), ((gy + 1) / 2) * (H - 1)
    return ((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2


def u8_trunc(x):
    """what cv2 sees of a float plane: truncated toward zero, clamped to 0..255"""
    return torch.nan_to_num(x, nan=0.0).trunc().clamp(0, 255)


def warp_eval(img, centers, kw, aw, kscale, ascale, align, mode, dtype=torch.float64, inorder=False):
    """the statement of tps2_warp in `dtype`: spline positions, bilinear sampling with zeros outside (a non-finite position gives 0).
    mode 3 -> (rounded half to even and saturated, the value before the rounding); else (value, value)"""
    _, C_, H, W = img.shape
    ix, iy = warp_positions(H, W, centers, kw, aw, kscale, ascale, align, mode, dtype, inorder)
    src = (u8_trunc(img) if mode == 3 else img).to(dtype)
    pre = gb.bilinear(src, ix[None], iy[None]).reshape(1, C_, H, W)
    return (torch.round(pre).clamp(0, 255), pre) if mode == 3 else (pre, pre)


def warp_control(img, centers, kw, aw, kscale, ascale, align, mode):
    """the fp32 control: oracle.tps_pipeline.warp_image_tps on the scaled weights as warp_by_tps hands them over (mode 0); the fp32 evaluation of
    the same formula in torch (mode 1, which has no torch twin; mode 3: before the rounding).  The formula is a sum over the centres in index
    order and the control adds in that order: handed to a matrix product, torch would add in blocks, whose error on the pixel-unit kernel
    (terms of 1e4 cancelling to a few pixels) is half that of any in-order sum, and the rule would measure the blocking."""
    if mode == 0:
        return otp.warp_image_tps(img, centers[None], (kw * kscale)[None], (aw * ascale)[None], align_corners=bool(align))
    return warp_eval(img, centers, kw, aw, kscale, ascale, align, mode, torch.float32, inorder=True)[1]


def warp_case(case, mode):
    """-> dict(img, centers, kw, aw, kscale, ascale, align) of one row of WARP_CASES in one mode"""
    n, (H, W), C_, (kscale, ascale), align, kind = case
    i = WARP_CASES.index(case)
    centers, kw, aw = warp_weights(n, H, W, mode, 9100 + i)
    return dict(img=warp_stairs(C_, H, W) if mode == 3 else warp_image(C_, H, W, kind, 9200 + i), centers=centers, kw=kw, aw=aw, kscale=kscale, ascale=ascale, align=align, mode=mode)


def quant_near(pre64, o32_pre):
    """mode 3: the samples left out: the fp64 value before the rounding lies within E of a .5 boundary, E = 4 x the largest error of the fp32
    control on that plane of the case (what the mode-1 rule grants the kernel), floored at one fp32 rounding of 255.  Per plane because the
    plane that sits at 255 falls to 0 across the image border, a gradient of 255 per pixel that the other planes do not have"""
    E = 4.0 * (o32_pre.double() - pre64).abs().amax((0, 2, 3), keepdim=True).clamp_min(255.0 * FLOOR)        # per plane: [1, C, 1, 1]
    frac = pre64 - torch.floor(pre64)
    return (frac - 0.5).abs() <= E, float(E.max())
