"""Generators, references, bars and case tables for the geometric solvers of csrc/geom.hip: st_tps_solve_grid (tps_solve_kernel and
tps_warp_kernel, the UDIS2 mesh transformer), st_dlt4 and st_mat3_sandwich.  tests/test_solve_bounds_cpu.py shows on the CPU that the
bars hold for a restatement of the kernels, that planted defects break them and that the tables cover their axes;
tests/test_solve_matrix_gpu.py runs the kernels against them.  Nothing here needs a GPU, and no constant comes from a GPU measurement.

The system   tps_system states the matrix exactly as tps_solve_kernel writes it: n3 = N + 3 rows [[1, x, y, R], [0, P^T]] with
    R[i][j] = d2 * float32(log(float64(d2 + 1e-6f))),  d2 = (0 * 0 + dx * dx) + dy * dy,
every operation rounded to fp32 on its own (the file is compiled without contraction).  The argument d2 + 1e-6f is formed in fp32: the
kernel calls st_logf_cr(d2 + 1e-6f) with a float argument, and st_logf_cr (csrc/common.h) widens what it is handed, (float)log((double)x).
The product d2 * log is float * float, rounded to fp32, and only then widened to the fp64 of the work area.  log_is_decided() says whether
every entry's fp64 logarithm keeps clear of an fp32 rounding midpoint by 2^-48 relative, so that any fp64 log of under an ulp (numpy's
here, the device library's there) rounds to the same fp32: the tables use only such inputs (asserted on the CPU).

The solve bar   e_max(T) <= 4 max(e_max(control), 2^-24 max|T_ref|), both errors against tps_solve_ref: the control rule of
tests/test_stage_fp64_gpu.py, the control being numpy's fp64 LAPACK solve of the same system rounded to fp32.  tps_solve_ref is an fp64
solve refined with residuals in np.longdouble (64-bit significand) until the correction is below 2^-60 of max|x| or no longer shrinks:
the residual itself carries n3 2^-64 |W| |x|, which the solve amplifies by the condition number, so a badly conditioned system settles
above 2^-60 (the table's worst: 2^-43).  The level it settles at is required to be below 2^-36, 2^12 below what the bar resolves.

The position bound   tps_positions_ref evaluates  p = T[0] + T[1] gx + T[2] gy + sum_k T[3 + k] r_k  in fp64 from the fp32 T it is handed
and the fp32 grid coordinates, with r_k = d2 log(d2 + 1e-6), d2 = (gx - sx)^2 + (gy - sy)^2 in fp64.  The kernel adds the N + 3 terms along
one chain of fused multiply-adds: each of them rounds a partial sum, and a partial sum is at most S = |T0| + |T1 gx| + |T2 gy| +
sum |T_k r_k|, so the chain costs at most (N + 3) u S, u = 2^-24 -- the form _geom_bounds.py uses for flow_encode.  To this comes the
rounding of each r_k: dx = gx - sx (u |dx|, twice in the square), dx dx (u), the sum of two positive squares (u): 4 u relative in d2; the
argument d2 + 1e-6 (u more, all of it positive): 5 u relative, which moves the logarithm by 5 u absolutely; the logarithm's own
rounding, taken at a whole ulp, 2 u |L|, so that torch's log on the host (oracle.geom.tps_indices) is covered too; the product (u):
    |dr_k| <= u d2 (5 + 7 |L|)          (4 |L| from d2, 2 |L| from the log, |L| from the product, 5 from the argument)
    E = u [ (N + 3) S + sum_k |T[3 + k]| d2_k (5 + 7 |L_k|) ]                  in the normalised coordinates of T.
In pixels x = (p + 1) W / 2: two more roundings relative to |x|, E_px = E W / 2 + 2 u |x|.  An index floor(x) is decided unless an
integer lies within E_px of the fp64 x: those samples are left out, at most CAP of a case.

The pixel bound   `_interpolate` with the kernel's own clamped indices (torch_tps_transform.py:18-94): out = sum over four taps of
a_t b_t v_t, a in {x1 - x, x - x0}, b in {y1 - y, y - y0}.  A position error moves out by at most E_x (|b0| |Ic - Ia| + |b1| |Id - Ib|)
+ E_y (the same in y) + E_x E_y |Ia - Ib - Ic + Id|; the roundings: a (1), b (1), their product (1), the product with v (1), three sums:
N_TAP = 7, relative to sum |a b v|."""
import functools
import itertools
import math

import numpy as np

F32, F64, LD = np.float32, np.float64, np.longdouble
U = 2.0 ** -24
CAP = 0.01
N_TAP = 7
SCALE = 1.27                                     # target = SCALE * source + ...: about a tenth of the positions beyond each side of [-1, 1]
KINDS = ("mesh", "random", "tight")
SINGULAR = ("coincident", "line")


def rng(seed):
    return np.random.default_rng(seed)


# ------------------------------------------------------------------------------------------------ control points
def mesh_points(N, seed, jitter=0.35):
    """N points of the g x g mesh over [-1, 1]^2, g = ceil(sqrt(N)), each moved by up to jitter / 2 of a mesh step and clipped to the
    square; where N < g g the points are a seeded choice of N of them, kept in mesh order.  N = g g, jitter 0.35: the model's case."""
    g = rng(seed)
    n = int(math.ceil(math.sqrt(N)))
    lin = np.linspace(-1.0, 1.0, n) if n > 1 else np.zeros(1)
    step = 2.0 / (n - 1) if n > 1 else 2.0
    pts = np.stack([np.tile(lin, n), np.repeat(lin, n)], 1) + jitter * step * (g.random((n * n, 2)) - 0.5)
    keep = np.sort(g.permutation(n * n)[:N])
    return np.clip(pts[keep], -1.0, 1.0).astype(F32)


def random_points(N, seed):
    return (rng(seed).random((N, 2)) * 2.0 - 1.0).astype(F32)


TIGHT = 1.0 / 16


def tight_points(N, seed):
    """the jittered mesh squeezed towards the line y = 0.3 x to TIGHT of its height: close to the singular set `line`, so the affine
    columns [1, x, y] are nearly dependent -- badly conditioned, but regular"""
    p = mesh_points(N, seed).astype(F64)
    return np.stack([p[:, 0], 0.3 * p[:, 0] + TIGHT * p[:, 1]], 1).astype(F32)


def singular_points(kind, N, seed):
    """`coincident`: the jittered mesh with point 1 a copy of point 0 (two equal rows); `line`: every point on y = x / 2, which fp32 halves
    exactly, so the columns [1, x, y] are dependent to the last bit"""
    p = mesh_points(N, seed)
    if kind == "coincident":
        p[1] = p[0]
        return p
    return np.stack([p[:, 0], F32(0.5) * p[:, 0]], 1).astype(F32)


def points(kind, N, seed):
    return {"mesh": mesh_points, "random": random_points, "tight": tight_points}[kind](N, seed)


def targets(source, seed, rough=True):
    """SCALE * source plus a displacement: `rough`, an independent draw of +-0.04 per point (the solver's cases: every weight of T is
    alive); else a smooth field of +-0.005 (the warp's cases: the weights stay small, so that sum |T_k r_k| and with it E stay small)"""
    s = source.astype(F64)
    g = rng(seed)
    if rough:
        d = 0.08 * (g.random(s.shape) - 0.5)
    else:
        ph = g.random(4) * 6.0
        d = 0.005 * np.stack([np.sin(2.0 * s[:, 0] + ph[0]) * np.cos(1.5 * s[:, 1] + ph[1]), np.cos(1.7 * s[:, 0] + ph[2]) * np.sin(2.2 * s[:, 1] + ph[3])], 1)
    return (SCALE * s + d).astype(F32)


def solve_inputs(kind, N, B=3):
    """(source, target) [B, N, 2] fp32 of a table case: item b has points and targets of its own.  A B = 1 call is item 0 alone."""
    seed = 1000 * (KINDS + SINGULAR).index(kind) + N
    gen = singular_points if kind in SINGULAR else points
    src = np.stack([gen(kind, N, seed + 7919 * b) for b in range(B)])
    return src, np.stack([targets(src[b], seed + 7919 * b + 1) for b in range(B)])


def warp_inputs(N, B):
    """the warp's control points: the jittered mesh with smooth targets"""
    src = np.stack([mesh_points(N, 50000 + N + 7919 * b) for b in range(B)])
    return src, np.stack([targets(src[b], 60000 + N + 7919 * b, rough=False) for b in range(B)])


# ------------------------------------------------------------------------------------------------ the system
def tps_entries(source, eps=True):
    """R [N, N] fp32 as the kernel forms it, and the fp64 logarithms behind it"""
    s = np.asarray(source, F32)
    px, py = s[:, 0], s[:, 1]
    d0 = F32(1.0) - F32(1.0)
    dx, dy = px[:, None] - px[None, :], py[:, None] - py[None, :]
    d2 = (d0 * d0 + dx * dx) + dy * dy                          # fp32, one rounding per operation, the kernel's order
    arg = d2 + F32(1e-6) if eps else d2                         # formed in fp32, then widened
    with np.errstate(divide="ignore", invalid="ignore"):
        L64 = np.log(arg.astype(F64))
        R = d2 * L64.astype(F32)                                # float * float
    assert R.dtype == F32
    return R, L64


def tps_system(source, target, eps=True):
    """-> (W [n3, n3], rhs [n3, 2]) in fp64: [[1, x, y, R], [0, P^T]] and [target; 0].  eps=False plants the missing + 1e-6."""
    s, t = np.asarray(source, F32), np.asarray(target, F32)
    N = s.shape[0]
    n3 = N + 3
    W = np.zeros((n3, n3), F64)
    W[:N, 0], W[:N, 1], W[:N, 2] = 1.0, s[:, 0], s[:, 1]
    W[:N, 3:] = tps_entries(s, eps)[0]
    W[N, 3:], W[N + 1, 3:], W[N + 2, 3:] = 1.0, s[:, 0], s[:, 1]
    rhs = np.zeros((n3, 2), F64)
    rhs[:N] = t
    return W, rhs


def log_is_decided(source):
    """every fp64 logarithm of the system rounds to the same fp32 when moved by 2^-48 relative either way"""
    L = tps_entries(source)[1]
    return bool(np.array_equal((L * (1 - 2.0 ** -48)).astype(F32), (L * (1 + 2.0 ** -48)).astype(F32)))


def tps_solve_ref(source, target, info=None):
    """T [2, n3] in np.longdouble: fp64 solve refined with longdouble residuals (the module docstring).  info: a dict that receives the
    last correction relative to max|x| and the number of refinements."""
    W, rhs = tps_system(source, target)
    Wl, bl = W.astype(LD), rhs.astype(LD)
    x = np.linalg.solve(W, rhs).astype(LD)
    last, rel, it = np.inf, np.inf, 0
    for it in range(1, 13):
        d = np.linalg.solve(W, (bl - Wl @ x).astype(F64))
        rel = float(np.abs(d).max() / np.abs(x).max())
        if rel > 0.5 * last:                                     # no longer shrinking: x is at the level the residual's own rounding allows
            rel = last
            break
        x = x + d
        last = rel
        if rel <= 2.0 ** -60:
            break
    assert rel <= 2.0 ** -36, f"the refinement settles at {rel:.3g} of max|x|: too badly conditioned a case for this table"
    if info is not None:
        info.update(correction=rel, refinements=it)
    return x.T.copy()


def tps_solve_control(source, target):
    """the same system through numpy's fp64 solve, rounded to fp32"""
    W, rhs = tps_system(source, target)
    return np.linalg.solve(W, rhs).T.astype(F32)


def solve_ratio(T, ref, ctl):
    """e_max(T) / max(e_max(control), 2^-24 max|T_ref|); a result that is not finite is infinitely wrong"""
    T = np.asarray(T)
    if not np.isfinite(T).all():
        return float("inf")
    e = float(np.abs(T.astype(LD) - ref).max())
    floor = max(float(np.abs(ctl.astype(LD) - ref).max()), U * float(np.abs(ref).max()))
    return e / floor


SOLVE_BAR = 4.0


@functools.lru_cache(maxsize=None)
def solve_case(kind, N):
    """(source, target, ref, control) of the three items of a table case, each computed once and left unchanged"""
    src, tgt = solve_inputs(kind, N, 3)
    ref = [tps_solve_ref(src[b], tgt[b]) for b in range(3)]
    ctl = [tps_solve_control(src[b], tgt[b]) for b in range(3)]
    for a in (src, tgt, *ref, *ctl):
        a.setflags(write=False)
    return src, tgt, ref, ctl


# ------------------------------------------------------------------------------------------------ tps_solve_kernel restated
def pick_pivot(a):
    """a: |A[c:, c]|.  -> the offset of the kernel's pivot: the largest value; among equal ones the lowest thread (offset % 256), then
    the lowest row of that thread's stride; 0 if nothing compares greater than -1 (all NaN)"""
    a = np.where(np.isnan(a), -1.0, a)
    m = a.max()
    if not m > -1.0:
        return 0
    cand = np.flatnonzero(a == m)
    return int(cand[np.lexsort((cand // 256, cand % 256))[0]])


def solve_kernel(source, target, defect=None, fill=np.nan):
    """tps_solve_kernel in numpy: the fp64 work area [n3, n3 + 2], Gauss-Jordan with partial pivoting, one rounding per operation (a
    product, then a difference: no contraction).  The pivot of column c is the kernel's: thread t looks at rows c + t, c + t + 256, ...
    and keeps the first largest (strict >, from -1: a NaN is never taken), thread 0 merges the 256 with a strict >, so among equal
    candidates the lowest thread wins, then the lowest row of that thread's stride.  A row whose factor is exactly 0 is skipped.
    -> (T [2, n3] fp32, the pivot rows).  T starts as `fill`, what the caller's buffer held.
    defects: "pivot_window" (the search sees rows c .. c + 255 only), "elim_256" (rows >= 256 are never eliminated), "write_256" (T's
    write-out stops at row 255), "no_eps" (the missing + 1e-6)"""
    W, rhs = tps_system(source, target, eps=defect != "no_eps")
    n3 = W.shape[0]
    A = np.concatenate([W, rhs], 1)
    pivots = []
    rows_all = np.arange(n3)
    with np.errstate(all="ignore"):
        for c in range(n3):
            a = np.abs(A[c:, c])
            if defect == "pivot_window":
                a = a[:256]
            piv = c + pick_pivot(a)
            pivots.append(piv)
            if piv != c:
                A[[c, piv]] = A[[piv, c]]
            inv = 1.0 / A[c, c]
            f = A[:, c] * inv
            live = rows_all != c
            if defect == "elim_256":
                live &= rows_all < 256
            upd = live & (f != 0.0)
            A[upd, c + 1:] -= f[upd, None] * A[c, c + 1:][None, :]
            A[live, c] = 0.0
        T = np.full((2, n3), fill, F32)
        stop = min(n3, 256) if defect == "write_256" else n3
        d = np.diagonal(A)[:stop]
        T[0, :stop], T[1, :stop] = (A[:stop, n3] / d).astype(F32), (A[:stop, n3 + 1] / d).astype(F32)
    return T, pivots


# ------------------------------------------------------------------------------------------------ the warp
def linspace32(n):
    """torch.linspace(-1, 1, n) in fp32 as lin_at restates it (oracle/c/geom_oracle.c through cgeom.linspace)"""
    from oracle import cgeom
    return np.asarray(cgeom.linspace(-1.0, 1.0, n), F32)


def grid32(out_hw):
    oh, ow = out_hw
    return np.tile(linspace32(ow), oh), np.repeat(linspace32(oh), ow)


def tps_positions_ref(source, T, out_hw):
    """source [N, 2] fp32, T [2, n3] fp32 -> (p [2, oh ow] fp64: the normalised sample position of every output pixel, E [2, oh ow]: the
    bound of the fp32 chain, derived in the module docstring)"""
    s, T = np.asarray(source, F32).astype(F64), np.asarray(T, F32).astype(F64)
    N = s.shape[0]
    gx, gy = (g.astype(F64) for g in grid32(out_hw))
    d2 = (gx[None, :] - s[:, 0:1]) ** 2 + (gy[None, :] - s[:, 1:2]) ** 2              # [N, P]
    L = np.log(d2 + 1e-6)
    r = d2 * L
    p = T[:, 0:1] + T[:, 1:2] * gx[None] + T[:, 2:3] * gy[None] + T[:, 3:] @ r
    S = np.abs(T[:, 0:1]) + np.abs(T[:, 1:2] * gx[None]) + np.abs(T[:, 2:3] * gy[None]) + np.abs(T[:, 3:]) @ np.abs(r)
    E = U * ((N + 3) * S + np.abs(T[:, 3:]) @ (d2 * (5.0 + 7.0 * np.abs(L))))
    return p, E


def to_pixels(p, E, in_hw):
    """normalised positions [2, P] and their E -> pixel coordinates (x, y) and (E_x, E_y) of `_interpolate`: x = (p + 1) W / 2"""
    H, W = in_hw
    x, y = (p[0] + 1.0) * W / 2.0, (p[1] + 1.0) * H / 2.0
    return x, y, E[0] * W / 2.0 + 2 * U * np.abs(x), E[1] * H / 2.0 + 2 * U * np.abs(y)


def near_integer(x, y, Ex, Ey, in_hw, factor=1.0):
    """an integer k lies within factor E of the coordinate in either axis, and floor() = k - 1 or k gives different clamped indices:
    0 <= k <= W - 1 (below, both indices clamp to 0 either way; above, to W - 1)"""
    H, W = in_hw
    kx, ky = np.round(x), np.round(y)
    return ((np.abs(x - kx) <= factor * Ex) & (kx >= 0) & (kx <= W - 1)) | ((np.abs(y - ky) <= factor * Ey) & (ky >= 0) & (ky <= H - 1))


def taps64(x, y, in_hw):
    """(x0, x1, y0, y1) of `_interpolate` from fp64 coordinates: floor, + 1, clamp; a coordinate that is not finite or beyond int32
    converts to INT_MIN as cvttss2si does, so both of its indices clamp to 0"""
    H, W = in_hw

    def toint(v):
        f = np.floor(v)
        bad = ~((f >= -2147483648.0) & (f < 2147483648.0))
        return np.where(bad, -2147483648, np.where(bad, 0, f).astype(np.int64))
    x0, y0 = toint(x), toint(y)
    return np.stack([np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1), np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)], -1)


def interpolate_bound(U_img, x, y, Ex, Ey):
    """U_img [C, H, W] fp32, pixel coordinates [P] -> (idx [P, 4], out [C, P] fp64, E [C, P]): `_interpolate` in fp64 and its bound"""
    C, H, W = U_img.shape
    idx = taps64(x, y, (H, W))
    x0, x1, y0, y1 = (idx[:, k] for k in range(4))
    fl = U_img.astype(F64).reshape(C, -1)
    Ia, Ib, Ic, Id = fl[:, y0 * W + x0], fl[:, y1 * W + x0], fl[:, y0 * W + x1], fl[:, y1 * W + x1]
    a0, a1, b0, b1 = x1 - x, x - x0, y1 - y, y - y0
    out = a0 * b0 * Ia + a0 * b1 * Ib + a1 * b0 * Ic + a1 * b1 * Id
    mag = np.abs(a0 * b0 * Ia) + np.abs(a0 * b1 * Ib) + np.abs(a1 * b0 * Ic) + np.abs(a1 * b1 * Id)
    E = (Ex * (np.abs(b0) * np.abs(Ic - Ia) + np.abs(b1) * np.abs(Id - Ib)) + Ey * (np.abs(a0) * np.abs(Ib - Ia) + np.abs(a1) * np.abs(Id - Ic))
         + Ex * Ey * np.abs(Ia - Ib - Ic + Id) + N_TAP * U * mag)
    return idx, out, E


def fma32(a, b, c):
    """fp32 fma: the product is exact in fp64; the fp64 sum then rounds twice, which the bound's first order does not see"""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def warp_kernel(U_img, source, T, out_hw, defect=None):
    """tps_warp_kernel for one item in numpy fp32: the dynamic LDS as one array of 4 N + 6 floats (source at 0, T at 2 N), the chain of
    N + 3 fused multiply-adds, `_interpolate`.  -> (positions [2, P] fp32, idx [P, 4] int32, out [C, P] fp32); what a defect leaves
    unwritten keeps the caller's fill: NaN, and INT_MIN + 1 for idx.
    defects: "lds_shift" (s_T at sh + 2 N + 1: its last element falls off the allocation -- the store is dropped, the load gives 0),
    "swap_rows" (T's two rows exchanged), "ragged_ow" (j <= ow - 1 - (ow % 64 == 1): the last column of such a block is lost)"""
    s, T = np.asarray(source, F32), np.asarray(T, F32)
    N = s.shape[0]
    n3 = N + 3
    C, H, W = U_img.shape
    oh, ow = out_hw
    off = 2 * N + (1 if defect == "lds_shift" else 0)
    lds = np.zeros(4 * N + 6 + 1, F32)                                   # one float more than the allocation, never stored to
    lds[:2 * N] = s.reshape(-1)
    flat = (T[::-1] if defect == "swap_rows" else T).reshape(-1)
    lds[off:off + 2 * n3] = flat
    lds[4 * N + 6] = 0.0
    sT = lds[off:off + 2 * n3]
    gx, gy = grid32(out_hw)
    with np.errstate(all="ignore"):
        xs, ys = sT[0] * np.ones_like(gx), sT[n3] * np.ones_like(gx)
        xs, ys = fma32(sT[1], gx, xs), fma32(sT[n3 + 1], gx, ys)
        xs, ys = fma32(sT[2], gy, xs), fma32(sT[n3 + 2], gy, ys)
        for k in range(N):
            dx, dy = gx - lds[2 * k], gy - lds[2 * k + 1]
            d2 = dx * dx + dy * dy
            r = d2 * np.log((d2 + F32(1e-6)).astype(F64)).astype(F32)
            xs, ys = fma32(sT[3 + k], r, xs), fma32(sT[n3 + 3 + k], r, ys)
        x = (xs + F32(1.0)) * F32(W) / F32(2.0)
        y = (ys + F32(1.0)) * F32(H) / F32(2.0)
        idx = taps64(x, y, (H, W))
        x0, x1, y0, y1 = (idx[:, k] for k in range(4))
        x0f, x1f, y0f, y1f = (v.astype(F32) for v in (x0, x1, y0, y1))
        wa, wb, wc, wd = (x1f - x) * (y1f - y), (x1f - x) * (y - y0f), (x - x0f) * (y1f - y), (x - x0f) * (y - y0f)
        fl = U_img.reshape(C, -1)
        out = wa * fl[:, y0 * W + x0]
        out = out + wb * fl[:, y1 * W + x0]
        out = out + wc * fl[:, y0 * W + x1]
        out = out + wd * fl[:, y1 * W + x1]
    assert out.dtype == F32 and x.dtype == F32
    idx = idx.astype(np.int32)
    if defect == "ragged_ow" and ow % 64 == 1:
        lost = (np.arange(oh * ow) % ow) == ow - 1
        out, idx = out.copy(), idx.copy()
        out[:, lost], idx[lost] = np.nan, IDX_FILL
    return np.stack([xs, ys]), idx, out


IDX_FILL = -2147483647


def image(C, H, W, seed):
    """grey levels 0 .. 255, a ramp of its own per channel under noise: a swapped axis or a wrong plane changes the result"""
    g = rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    k = np.arange(C)[:, None, None]
    ramp = ((3 + k) * xs[None] + (11 + 2 * k) * ys[None]) % 97.0 / 97.0
    return (255.0 * (0.5 * ramp + 0.5 * g.random((C, H, W)))).astype(F32)


def warp_check(U_img, source, T, in_hw, out_hw, idx, out, factor=1.0):
    """The bars of one item of a warp case.  T: the fp32 coefficients the positions are taken from (on the GPU the kernel's own);
    idx [P, 4], out [C, P] or None: what the code under test wrote.
    -> dict(left_out: share of samples within factor E of an integer, idx_ok, out_ratio: max |out - ref| / E over the others (inf for
    a value that is not finite), pos: (x, y, Ex, Ey), near)"""
    p, E = tps_positions_ref(source, T, out_hw)
    x, y, Ex, Ey = to_pixels(p, E, in_hw)
    near = near_integer(x, y, Ex, Ey, in_hw, factor)
    res = dict(left_out=float(near.mean()), pos=(x, y, Ex, Ey), near=near, idx_ok=True, out_ratio=0.0)
    keep = ~near
    want_idx, ref, Eo = interpolate_bound(U_img, x, y, Ex, Ey) if U_img is not None else (taps64(x, y, in_hw), None, None)
    if idx is not None:
        res["idx_ok"] = bool(np.array_equal(np.asarray(idx)[keep], want_idx[keep]))
    if out is not None and keep.any():
        o = np.asarray(out, F64)[:, keep]
        with np.errstate(all="ignore"):
            q = np.abs(o - ref[:, keep]) / Eo[:, keep]
        q = np.where(np.abs(o - ref[:, keep]) == 0, 0.0, q)
        res["out_ratio"] = float("inf") if not np.isfinite(o).all() else float(np.nanmax(q)) if q.size else 0.0
    return res


def outside_shares(x, y, in_hw):
    """share of the sample positions left of, right of, above and below the image: the clamp's four sides"""
    H, W = in_hw
    return float((x < 0).mean()), float((x >= W).mean()), float((y < 0).mean()), float((y >= H).mean())


# ------------------------------------------------------------------------------------------------ dlt4, mat3
def dlt_inputs(B, mscale, seed):
    """the four corners of the mscale * 512 image and corner motions of up to +-30 % of the 512 side, so that the pivot order varies"""
    w, h = F32(512.0 * mscale[0]), F32(512.0 * mscale[1])
    src = np.array([[0, 0], [w, 0], [0, h], [w, h]], F32)
    return src, ((rng(seed).random((B, 4, 2)) - 0.5) * 2 * 0.3 * 512.0).astype(F32)


def dlt_dst(src, motion, mscale, B):
    """dst as dlt4_kernel forms it: src + motion * mscale, a product and a sum in fp32; src itself without motion"""
    s = np.broadcast_to(src[None], (B, 4, 2)).astype(F32)
    if motion is None:
        return s.copy()
    return (s + motion * np.array(mscale, F32)[None, None, :]).astype(F32)


def dlt4_ref(src, motion, mscale, div, B):
    """the project's bit-exact restatement (oracle.geom.dlt4) of the kernel's inputs: both point sets divided by div in fp32"""
    import torch
    from oracle import geom
    s = np.broadcast_to(src[None], (B, 4, 2)).astype(F32)
    d = dlt_dst(src, motion, mscale, B)
    return geom.dlt4(torch.from_numpy((s / F32(div)).astype(F32)), torch.from_numpy((d / F32(div)).astype(F32))).numpy()


def dlt_pivots(src4, dst4):
    """the row swaps of dlt4_kernel's LU (of the transposed DLT matrix, partial pivoting, fused trailing update) for one point set"""
    A = np.zeros((8, 8), F32)
    for p in range(4):
        x, y, u, v = src4[p, 0], src4[p, 1], dst4[p, 0], dst4[p, 1]
        A[:, 2 * p] = [x, y, 1, 0, 0, 0, -(u * x), -(u * y)]
        A[:, 2 * p + 1] = [0, 0, 0, x, y, 1, -(v * x), -(v * y)]
    piv = []
    with np.errstate(all="ignore"):
        for k in range(8):
            col = np.abs(A[k:, k])
            p = k + int(np.argmax(col))                              # first largest: the kernel's strict >
            piv.append(p)
            if p != k:
                A[[k, p]] = A[[p, k]]
            r = F32(1.0) / A[k, k]
            A[k + 1:, k] = A[k + 1:, k] * r
            A[k + 1:, k + 1:] = fma32(-A[k + 1:, k:k + 1], A[k:k + 1, k + 1:], A[k + 1:, k + 1:])
    return tuple(piv)


MODEL_M = np.array([[32.0, 0, 32.0], [0, 24.0, 24.0], [0, 0, 1.0]], F32)       # the model's scale pair: L = inverse(M), R = M


def mat3_inputs(B, seed=900):
    """general matrices: the first B of one draw, so that every B of the table shares its pivot paths"""
    return rng(seed).standard_normal((max(MAT3_B), 3, 3)).astype(F32)[:B]


def mat3_ref(L, X, R, invert):
    """L @ (inverse(X) if invert == 1 else X) @ R through the project's bit-exact restatements (oracle.geom.inverse / matmul3)"""
    import torch
    from oracle import geom
    Xt = torch.from_numpy(np.ascontiguousarray(X))
    Lt, Rt = torch.from_numpy(np.ascontiguousarray(L)).expand_as(Xt), torch.from_numpy(np.ascontiguousarray(R)).expand_as(Xt)
    mid = geom.inverse(Xt) if invert == 1 else Xt
    return geom.matmul3(geom.matmul3(Lt, mid), Rt).numpy()


def mat3_pivots(X):
    """the row swaps of mat3_inv for one matrix: it factors the transpose (oracle.mat3._lu3, the restatement of mat3_lu)"""
    from oracle.mat3 import _lu3
    return tuple(_lu3(np.asarray(X, F32).T)[1])


# ------------------------------------------------------------------------------------------------ case tables
def cyc(seq, i):
    return seq[i % len(seq)]


# n3 = N + 3 rows, one workgroup of 256 threads: 4 the smallest system (N = 1 and 2 have fewer than three points, so all of them lie on
# one line: the singular set `line`, run for frames and batch independence only); 5, 6, 7, 12 short of a wave; 172 the model's; 255,
# 256, 257 step across one trip per thread; 512, 513 across two; 768 three full trips
TPS_N = [1, 2, 3, 4, 9, 169, 252, 253, 254, 509, 510, 765]
TPS_N_REGULAR = [N for N in TPS_N if N >= 3]
TPS_N_LARGE = 1024                  # n3 = 1027: a fifth trip begun, an 8 MB work buffer; solver only, kept only if it runs in a few seconds
TPS_B = [1, 3]                      # one workgroup alone; a grid of three whose items must not see each other
TPS_C = [1, 3, 4]                   # one plane; the model's three; one more than it
# (oh, ow) against the warp's 4 x 64 pixel block: one pixel; one full row of a block; a full block's height one column short; one past a
# block in both; three rows, two blocks and a column; the existing test's size; (2, 2): the one remainder of oh the others leave out
TPS_OUT_HW = [(1, 1), (1, 64), (4, 63), (5, 65), (3, 129), (24, 28), (2, 2)]
TPS_IN_HW = [(1, 1), (2, 2), (32, 40)]      # both indices always clamp to 0; every sample touches the border; an image with an inside
SOLVE_CASES = [(kind, N, B) for kind, N, B in itertools.product(KINDS, TPS_N_REGULAR, TPS_B)]
SINGULAR_N = [1, 2]
# the warp: every N against every output size, the input size and the channel count cycling so that each pair of them occurs
WARP_CASES = [(N, cyc(TPS_IN_HW, a + b), out_hw, cyc(TPS_C, a + 2 * b)) for (a, N), (b, out_hw) in itertools.product(enumerate(TPS_N_REGULAR), enumerate(TPS_OUT_HW))]
WARP_B = 2
DLT_B = MAT3_B = [1, 63, 64, 65, 130]       # 64 threads a block: one thread, one short of a block, a block, one past it, two blocks and two
DLT_DIV = [1.0, 8.0]                        # the plain call and the model's
DLT_MSCALE = [(1.0, 1.0), (400.0 / 512.0, 304.0 / 512.0)]
DLT_CASES = list(itertools.product(DLT_B, DLT_DIV, (True, False), DLT_MSCALE))
MAT3_CASES = list(itertools.product(MAT3_B, (0, 1, 2)))
