// multiband_fusion: Laplacian-pyramid seam blend of two warped images (contract in README.md, "multiband_fusion"; CPU restatement
// tests/_multiband_ref.py).  gfx950 only.  Every kernel of a call goes to the caller's stream, in order, inside the caller's workspace:
// no host synchronisation, no allocation, no memset / memcpy, so a call captures into a hipGraph as a linear chain.
//
//   mb_masks_kernel      m1, m2 (mask > 0.5) and not-U as uint8
//   edt_cols_kernel      per column: vertical distance to the nearest site and that site's row, packed (g << 13 | row)      x 3
//   edt_rows_d_kernel    per row: exact squared Euclidean distance from the packed row (m1, m2)                              x 2
//   edt_rows_idx_kernel  the same with the lowest row-major nearest site (not-U)                                             x 1
//   mb_fields_kernel     ownership W1, extension outside U, the seven level-0 planes I1f[3] I2f[3] W
//   mb_reduce_kernel     one REDUCE step of the seven planes, per level
//   mb_top_kernel        R = Gb + Gw (Ga - Gb) at the coarsest level
//   mb_down_kernel       per level, going down: three EXPANDs, two Laplacians, blend, add (the last one: U and the clamp)
//
// Compiled with -ffp-contract=off: every product and sum below is one fp32 rounding, in the order written.
#include "common.h"

#define MB_MAX_SIDE 4096
#define MB_MAX_LEVELS 16
#define EDT_NONE 0x1FFFu                // 13-bit field value "no site" (distance) / "the ring" (row, column)
#define EDT_KEY_NONE (~0ull)

// ---- exact squared Euclidean distance transform, sites = pixels with mask == 0 (and the one-pixel ring round the canvas when `border`) ----
// pass 1: g = distance along the column to the nearest site, row = that site's row (EDT_NONE for the ring), packed as g << 13 | row so that
// the smaller word is the nearer site and, at equal distance, the upper one.  A workgroup takes 64 columns (coalesced across columns) and cuts
// them into EDT_SEGS row segments, one thread each: (1) first and last site row of every segment to LDS, (2) the nearest site above and below
// a segment from the other segments' summaries, (3) a sweep down writing the key of the site above, a sweep up keeping the smaller key.
#define EDT_SEGS 16
__device__ __forceinline__ void edt_step(uint32_t& g, uint32_t& row, bool site, int y) {
    if (site) { g = 0; row = (uint32_t)y; }
    else if (g != EDT_NONE) ++g;
}

__global__ void __launch_bounds__(64 * EDT_SEGS) edt_cols_kernel(const uint8_t* __restrict__ mask, uint32_t* __restrict__ packed, int H, int W, int border) {
    __shared__ int first[EDT_SEGS][64], last[EDT_SEGS][64];
    const int tx = threadIdx.x, seg = threadIdx.y, x = blockIdx.x * 64 + tx;
    const bool act = x < W;
    const int S = (H + EDT_SEGS - 1) / EDT_SEGS, y0 = min(seg * S, H), y1 = min(y0 + S, H);
    int f = -1, l = -1;
    if (act) {
#pragma unroll 8
        for (int y = y0; y < y1; ++y)
            if (mask[(size_t)y * W + x] == 0) { if (f < 0) f = y; l = y; }
    }
    first[seg][tx] = f; last[seg][tx] = l;
    __syncthreads();
    if (!act || y0 >= y1) return;
    // the state one row above the segment
    uint32_t g = border ? (uint32_t)y0 : EDT_NONE, row = EDT_NONE;
    for (int t = seg - 1; t >= 0; --t)
        if (last[t][tx] >= 0) { g = (uint32_t)(y0 - 1 - last[t][tx]); row = (uint32_t)last[t][tx]; break; }
#pragma unroll 8
    for (int y = y0; y < y1; ++y) {
        edt_step(g, row, mask[(size_t)y * W + x] == 0, y);
        packed[(size_t)y * W + x] = g << 13 | row;
    }
    // the state one row below the segment
    g = border ? (uint32_t)(H - y1) : EDT_NONE; row = EDT_NONE;
    for (int t = seg + 1; t < EDT_SEGS; ++t)
        if (first[t][tx] >= 0) { g = (uint32_t)(first[t][tx] - y1); row = (uint32_t)first[t][tx]; break; }
    for (int yb = y1; yb > y0; yb -= 8) {                  // eight rows at a time: their loads first, then the chain
        uint32_t above[8];
        uint8_t mk[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int y = max(yb - 1 - j, y0);
            above[j] = packed[(size_t)y * W + x];
            mk[j] = mask[(size_t)y * W + x];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int y = yb - 1 - j;
            if (y < y0) break;
            edt_step(g, row, mk[j] == 0, y);
            const uint32_t below = g << 13 | row;
            if (below < above[j]) packed[(size_t)y * W + x] = below;
        }
    }
}

// pass 2, one workgroup (up to 1024 threads) per row, the row of pass 1 in LDS (W <= 4096: 16 KB).  Each thread scans outward x' = x -+ k and stops once k * k
// alone reaches its best distance (exact).  `packed` and `D` may be the same buffer: a workgroup reads its row before it writes it.
// Without an index the LDS row holds g * g and the scan is 32-bit: "no site" is 8191^2, above every distance of a 4096 x 4096 canvas.
__global__ void __launch_bounds__(1024) edt_rows_d_kernel(const uint32_t* packed, int32_t* D, int W, int border) {
    __shared__ uint32_t sq[MB_MAX_SIDE];
    const int y = blockIdx.x;
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        const uint32_t g = packed[(size_t)y * W + x] >> 13;
        sq[x] = g * g;
    }
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        uint32_t best = sq[x];
        if (border) {
            const uint32_t e = (uint32_t)min(x + 1, W - x);
            best = min(best, e * e);
        }
        const int kl = x, kr = W - 1 - x, kboth = min(kl, kr), kmax = max(kl, kr);
        int k = 1;
        for (; k <= kboth; ++k) {
            const uint32_t kk = (uint32_t)(k * k);
            if (kk >= best) break;
            best = min(best, min(sq[x - k], sq[x + k]) + kk);
        }
        if (k > kboth) {
            const int dir = kl > kr ? -1 : 1;
            for (; k <= kmax; ++k) {
                const uint32_t kk = (uint32_t)(k * k);
                if (kk >= best) break;
                best = min(best, sq[x + dir * k] + kk);
            }
        }
        D[(size_t)y * W + x] = best >= EDT_NONE * EDT_NONE ? INT32_MAX : (int32_t)best;
    }
}

__device__ __forceinline__ unsigned long long edt_key(uint32_t p, int k, int xs) {
    const uint32_t g = p >> 13, row = p & EDT_NONE;
    if (g == EDT_NONE) return EDT_KEY_NONE;
    const unsigned long long d = (unsigned long long)(k * k) + (unsigned long long)(g * g);
    return d << 26 | (unsigned long long)row << 13 | (row == EDT_NONE ? EDT_NONE : (uint32_t)xs);
}

// pass 2 with the nearest site's index: the winner is the smallest key D << 26 | row << 13 | column, i.e. the lowest row-major index among
// the nearest sites (a globally nearest site is nearest within its own column); ties are still examined, k * k == best can hold a lower index.
__global__ void __launch_bounds__(1024) edt_rows_idx_kernel(const uint32_t* packed, int32_t* D, int32_t* index, int W, int border) {
    __shared__ uint32_t row[MB_MAX_SIDE];
    const int y = blockIdx.x;
    for (int x = threadIdx.x; x < W; x += blockDim.x) row[x] = packed[(size_t)y * W + x];
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        unsigned long long best = edt_key(row[x], 0, x);
        if (border) {
            const long long e = min(x + 1, W - x);
            const unsigned long long kb = (unsigned long long)(e * e) << 26 | (unsigned long long)EDT_NONE << 13 | EDT_NONE;
            best = min(best, kb);
        }
        const int kmax = max(x, W - 1 - x);
        for (int k = 1; k <= kmax; ++k) {
            if ((unsigned long long)(k * k) > (best >> 26)) break;
            if (x - k >= 0) best = min(best, edt_key(row[x - k], k, x - k));
            if (x + k < W) best = min(best, edt_key(row[x + k], k, x + k));
        }
        const uint32_t r = (uint32_t)(best >> 13) & EDT_NONE, c = (uint32_t)best & EDT_NONE;
        D[(size_t)y * W + x] = best == EDT_KEY_NONE ? INT32_MAX : (int32_t)(best >> 26);
        index[(size_t)y * W + x] = r == EDT_NONE ? -1 : (int32_t)(r * (uint32_t)W + c);
    }
}

static int edt_launch(const uint8_t* mask, int H, int W, int border, int32_t* D, int32_t* index, hipStream_t s) {
    edt_cols_kernel<<<(W + 63) / 64, dim3(64, EDT_SEGS), 0, s>>>(mask, (uint32_t*)D, H, W, border);
    ST_CHECK_LAUNCH();
    const int threads = min((W + 63) / 64 * 64, 1024);          // the scan of one pixel is serial: as few pixels per thread as a workgroup allows
    if (index) edt_rows_idx_kernel<<<H, threads, 0, s>>>((const uint32_t*)D, D, index, W, border);
    else edt_rows_d_kernel<<<H, threads, 0, s>>>((const uint32_t*)D, D, W, border);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

static bool mb_overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

// D is written while the mask is still being read, and index while D's row is: the three planes are disjoint
extern "C" int st_edt_sq_u8(const uint8_t* mask, int32_t H, int32_t W, int32_t border_is_site, int32_t* D, int32_t* index, void* stream) {
    if (!mask || !D || H < 1 || W < 1 || H > MB_MAX_SIDE || W > MB_MAX_SIDE) return ST_EINVAL;
    const int64_t n = (int64_t)H * W;
    if (mb_overlap(D, 4 * n, mask, n)) return ST_EINVAL;
    if (index && (mb_overlap(index, 4 * n, mask, n) || mb_overlap(index, 4 * n, D, 4 * n))) return ST_EINVAL;
    return edt_launch(mask, H, W, border_is_site != 0, D, index, (hipStream_t)stream);
}

// ---- the blend ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) mb_masks_kernel(const float* __restrict__ mask1, const float* __restrict__ mask2, uint8_t* __restrict__ m1,
                                                       uint8_t* __restrict__ m2, uint8_t* __restrict__ notu, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint8_t a = mask1[i] > 0.5f, b = mask2[i] > 0.5f;
    m1[i] = a; m2[i] = b; notu[i] = !(a | b);
}

// level 0 of the three pyramids: planes 0-2 I1f, 3-5 I2f, 6 W.  q = the pixel itself inside U, else the nearest pixel of U (`nearest`,
// -1 when U is empty: everything 0).  W1(q) = m1 and (not m2 or D1 >= D2); C = the owner's pixel at q.  With a seam (`side` != NULL and
// info[0] != 0, read here: no host decision) the overlap follows it instead: W1(q) = m1 and (not m2 or side).
__global__ void __launch_bounds__(256) mb_fields_kernel(const float* __restrict__ img1, const float* __restrict__ img2, const uint8_t* __restrict__ m1,
                                                        const uint8_t* __restrict__ m2, const int32_t* __restrict__ D1, const int32_t* __restrict__ D2,
                                                        const int32_t* __restrict__ nearest, const uint8_t* __restrict__ side, const int32_t* __restrict__ info,
                                                        float* __restrict__ G, int n) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const bool a = m1[p], b = m2[p], seam = side && info[0] != 0;
    const int q = (a || b) ? p : nearest[p];
    bool w1 = false;
    float c[3] = {0.f, 0.f, 0.f};
    if (q >= 0) {
        w1 = m1[q] && (!m2[q] || (seam ? side[q] != 0 : D1[q] >= D2[q]));
        const float* src = w1 ? img1 : img2;
        for (int ch = 0; ch < 3; ++ch) c[ch] = st_u8_trunc(src[(size_t)ch * n + q]);
    }
    for (int ch = 0; ch < 3; ++ch) {
        G[(size_t)ch * n + p] = a ? st_u8_trunc(img1[(size_t)ch * n + p]) : c[ch];
        G[(size_t)(3 + ch) * n + p] = b ? st_u8_trunc(img2[(size_t)ch * n + p]) : c[ch];
    }
    G[(size_t)6 * n + p] = w1 ? 1.f : 0.f;
}

__device__ __forceinline__ float mb_reduce5(float a, float b, float c, float d, float e) {
    return (((0.0625f * a + 0.25f * b) + 0.375f * c) + 0.25f * d) + 0.0625f * e;
}

// REDUCE of the seven planes (blockIdx.y): along W at the five source rows, each result one fp32 value, then along H.
__global__ void __launch_bounds__(256) mb_reduce_kernel(const float* __restrict__ in, float* __restrict__ out, int h, int w, int ho, int wo) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= ho * wo) return;
    const int i = o / wo, j = o - i * wo;
    const float* src = in + (size_t)blockIdx.y * h * w;
    int xs[5];
    for (int k = 0; k < 5; ++k) xs[k] = min(max(2 * j + k - 2, 0), w - 1);
    float r[5];
    for (int k = 0; k < 5; ++k) {
        const float* row = src + (size_t)min(max(2 * i + k - 2, 0), h - 1) * w;
        r[k] = mb_reduce5(row[xs[0]], row[xs[1]], row[xs[2]], row[xs[3]], row[xs[4]]);
    }
    out[(size_t)blockIdx.y * ho * wo + o] = mb_reduce5(r[0], r[1], r[2], r[3], r[4]);
}

__device__ __forceinline__ float mb_expand3(float a, float b, float c, int odd) {      // taps c-1, c, c+1 of an even sample; c, c+1 (b, c) of an odd one
    return odd ? b * 0.5f + c * 0.5f : (a * 0.125f + b * 0.75f) + c * 0.125f;
}

// EXPAND of a coarse plane [hc, wc] at the finer position (i, j): along W at the coarse rows the H pass needs, then along H.
__device__ __forceinline__ float mb_expand(const float* __restrict__ pl, int i, int j, int hc, int wc) {
    const int ci = i >> 1, cj = j >> 1, oi = i & 1, oj = j & 1;
    const int x0 = max(cj - 1, 0), x2 = min(cj + 1, wc - 1);
    float r[3];
    for (int k = 0; k < 3; ++k) {
        const float* row = pl + (size_t)min(max(ci + k - 1, 0), hc - 1) * wc;
        r[k] = mb_expand3(row[x0], row[cj], row[x2], oj);
    }
    return mb_expand3(r[0], r[1], r[2], oi);
}

// `final`: U ? clamp(v, 0, 255) : 0
__device__ __forceinline__ float mb_finish(float v, const uint8_t* notu, int p) { return notu[p] ? 0.f : fminf(fmaxf(v, 0.f), 255.f); }

// R = Gb + Gw (Ga - Gb) at the coarsest level; blockIdx.y = channel.  notu != NULL: this is level 0 (levels = 0), finish.
__global__ void __launch_bounds__(256) mb_top_kernel(const float* __restrict__ G, float* __restrict__ R, const uint8_t* __restrict__ notu, int n) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int ch = blockIdx.y;
    const float ga = G[(size_t)ch * n + p], gb = G[(size_t)(3 + ch) * n + p], gw = G[(size_t)6 * n + p];
    const float v = gb + gw * (ga - gb);
    R[(size_t)ch * n + p] = notu ? mb_finish(v, notu, p) : v;
}

// R_l = EXPAND(R_{l+1}) + (Lb + Gw (La - Lb)), Lx = Gx_l - EXPAND(Gx_{l+1}); blockIdx.y = channel.  G: level l [7, h, w]; Gc: level l + 1
// [7, hc, wc]; Rc [3, hc, wc]; R [3, h, w].  notu != NULL: level 0, finish.
__global__ void __launch_bounds__(256) mb_down_kernel(const float* __restrict__ G, const float* __restrict__ Gc, const float* __restrict__ Rc,
                                                      float* __restrict__ R, const uint8_t* __restrict__ notu, int h, int w, int hc, int wc) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int n = h * w, nc = hc * wc;
    if (p >= n) return;
    const int i = p / w, j = p - i * w, ch = blockIdx.y;
    const float la = G[(size_t)ch * n + p] - mb_expand(Gc + (size_t)ch * nc, i, j, hc, wc);
    const float lb = G[(size_t)(3 + ch) * n + p] - mb_expand(Gc + (size_t)(3 + ch) * nc, i, j, hc, wc);
    const float gw = G[(size_t)6 * n + p];
    const float v = mb_expand(Rc + (size_t)ch * nc, i, j, hc, wc) + (lb + gw * (la - lb));
    R[(size_t)ch * n + p] = notu ? mb_finish(v, notu, p) : v;
}

// workspace layout: m1, m2, notu (uint8 [H W]); D1, D2, DN, nearest (int32 [H W]); G_l [7, h_l, w_l] for l = 0..Le; R_l [3, h_l, w_l] for
// l = 1..Le -- each region rounded up to 16 bytes.  Le = the effective level count: REDUCE stops when both sides are 1.
struct mb_layout {
    int Le, h[MB_MAX_LEVELS + 1], w[MB_MAX_LEVELS + 1];
    int64_t m1, m2, notu, D1, D2, DN, nearest, G[MB_MAX_LEVELS + 1], R[MB_MAX_LEVELS + 1], total;
};

static bool mb_plan(int H, int W, int levels, mb_layout& L) {
    if (H < 1 || W < 1 || H > MB_MAX_SIDE || W > MB_MAX_SIDE || levels < 0 || levels > MB_MAX_LEVELS) return false;
    int64_t at = 0;
    auto take = [&](int64_t bytes) { const int64_t o = at; at += (bytes + 15) & ~(int64_t)15; return o; };
    const int64_t n = (int64_t)H * W;
    L.m1 = take(n); L.m2 = take(n); L.notu = take(n);
    L.D1 = take(4 * n); L.D2 = take(4 * n); L.DN = take(4 * n); L.nearest = take(4 * n);
    L.Le = 0; L.h[0] = H; L.w[0] = W;
    while (L.Le < levels && (L.h[L.Le] > 1 || L.w[L.Le] > 1)) {
        L.h[L.Le + 1] = (L.h[L.Le] + 1) >> 1; L.w[L.Le + 1] = (L.w[L.Le] + 1) >> 1; ++L.Le;
    }
    for (int l = 0; l <= L.Le; ++l) L.G[l] = take((int64_t)28 * L.h[l] * L.w[l]);
    L.R[0] = -1;
    for (int l = 1; l <= L.Le; ++l) L.R[l] = take((int64_t)12 * L.h[l] * L.w[l]);
    L.total = at;
    return at <= INT32_MAX;
}

extern "C" int st_multiband_workspace_bytes(int32_t H, int32_t W, int32_t levels) {
    mb_layout L;
    return mb_plan(H, W, levels, L) ? (int)L.total : 0;
}

// out may be img1 or img2 exactly (only the last launch writes it, and that one reads the workspace alone) and nothing else: not a shifted
// view of an image, not a mask, side, info or the workspace; no operand may lie in the workspace
static bool mb_out_ok(const float* img1, const float* img2, const float* mask1, const float* mask2, const uint8_t* side, const int32_t* info,
                      const float* out, const void* workspace, int64_t ws_bytes, int64_t n) {
    const int64_t img = 12 * n, msk = 4 * n;
    if (out != img1 && mb_overlap(out, img, img1, img)) return false;
    if (out != img2 && mb_overlap(out, img, img2, img)) return false;
    if (mb_overlap(out, img, mask1, msk) || mb_overlap(out, img, mask2, msk)) return false;
    if (side && mb_overlap(out, img, side, n)) return false;
    if (info && mb_overlap(out, img, info, 16)) return false;
    if (mb_overlap(workspace, ws_bytes, out, img) || mb_overlap(workspace, ws_bytes, img1, img) || mb_overlap(workspace, ws_bytes, img2, img)) return false;
    if (mb_overlap(workspace, ws_bytes, mask1, msk) || mb_overlap(workspace, ws_bytes, mask2, msk)) return false;
    if (side && mb_overlap(workspace, ws_bytes, side, n)) return false;
    if (info && mb_overlap(workspace, ws_bytes, info, 16)) return false;
    return true;
}

// side, info: the seam of st_seam_dp, or both NULL (the distance seam)
static int mb_blend(const float* img1, const float* img2, const float* mask1, const float* mask2, int32_t H, int32_t W, int32_t levels, const uint8_t* side,
                    const int32_t* info, float* out, void* workspace, int64_t workspace_bytes, void* stream) {
    mb_layout L;
    if (!img1 || !img2 || !mask1 || !mask2 || !out || !workspace || !mb_plan(H, W, levels, L)) return ST_EINVAL;
    if (workspace_bytes < L.total || ((uintptr_t)workspace & 15)) return ST_EINVAL;
    if (!mb_out_ok(img1, img2, mask1, mask2, side, info, out, workspace, L.total, (int64_t)H * W)) return ST_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    uint8_t *m1 = (uint8_t*)(ws + L.m1), *m2 = (uint8_t*)(ws + L.m2), *notu = (uint8_t*)(ws + L.notu);
    int32_t *D1 = (int32_t*)(ws + L.D1), *D2 = (int32_t*)(ws + L.D2), *DN = (int32_t*)(ws + L.DN), *nearest = (int32_t*)(ws + L.nearest);
    const int n = H * W, blocks = (n + 255) / 256;
    mb_masks_kernel<<<blocks, 256, 0, s>>>(mask1, mask2, m1, m2, notu, n);
    ST_CHECK_LAUNCH();
    int rc;
    if ((rc = edt_launch(m1, H, W, 1, D1, nullptr, s)) != ST_OK) return rc;
    if ((rc = edt_launch(m2, H, W, 1, D2, nullptr, s)) != ST_OK) return rc;
    if ((rc = edt_launch(notu, H, W, 0, DN, nearest, s)) != ST_OK) return rc;
    mb_fields_kernel<<<blocks, 256, 0, s>>>(img1, img2, m1, m2, D1, D2, nearest, side, info, (float*)(ws + L.G[0]), n);
    ST_CHECK_LAUNCH();
    for (int l = 0; l < L.Le; ++l) {
        const int no = L.h[l + 1] * L.w[l + 1];
        mb_reduce_kernel<<<dim3((no + 255) / 256, 7), 256, 0, s>>>((const float*)(ws + L.G[l]), (float*)(ws + L.G[l + 1]), L.h[l], L.w[l], L.h[l + 1], L.w[l + 1]);
        ST_CHECK_LAUNCH();
    }
    {
        const int nt = L.h[L.Le] * L.w[L.Le];
        mb_top_kernel<<<dim3((nt + 255) / 256, 3), 256, 0, s>>>((const float*)(ws + L.G[L.Le]), L.Le ? (float*)(ws + L.R[L.Le]) : out, L.Le ? nullptr : notu, nt);
        ST_CHECK_LAUNCH();
    }
    for (int l = L.Le - 1; l >= 0; --l) {
        const int nl = L.h[l] * L.w[l];
        mb_down_kernel<<<dim3((nl + 255) / 256, 3), 256, 0, s>>>((const float*)(ws + L.G[l]), (const float*)(ws + L.G[l + 1]), (const float*)(ws + L.R[l + 1]),
                                                                   l ? (float*)(ws + L.R[l]) : out, l ? nullptr : notu, L.h[l], L.w[l], L.h[l + 1], L.w[l + 1]);
        ST_CHECK_LAUNCH();
    }
    return ST_OK;
}

extern "C" int st_multiband_blend(const float* img1, const float* img2, const float* mask1, const float* mask2, int32_t H, int32_t W, int32_t levels,
                                  float* out, void* workspace, int64_t workspace_bytes, void* stream) {
    return mb_blend(img1, img2, mask1, mask2, H, W, levels, nullptr, nullptr, out, workspace, workspace_bytes, stream);
}

extern "C" int st_multiband_blend_seam(const float* img1, const float* img2, const float* mask1, const float* mask2, int32_t H, int32_t W, int32_t levels,
                                       const uint8_t* side, const int32_t* info, float* out, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!side || !info) return ST_EINVAL;
    return mb_blend(img1, img2, mask1, mask2, H, W, levels, side, info, out, workspace, workspace_bytes, stream);
}
