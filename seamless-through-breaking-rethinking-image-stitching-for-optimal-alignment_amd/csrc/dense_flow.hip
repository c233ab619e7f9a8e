// dense_flow: a weight-free residual flow -- coarse-to-fine, zero-mean Lucas-Kanade on integer pyramids.  Contract in README.md,
// "dense_flow"; CPU restatement tests/_dense_flow_ref.py.  gfx950 only.  Everything is an integer except one 2x2 solve per pixel and
// iteration in fp64 (this file is compiled with -ffp-contract=off: every product, difference and quotient there rounds on its own), so
// every window sum is independent of the order it is formed in.  Every kernel of a call goes to the caller's stream, in order, inside
// the caller's buffers: no host synchronisation, no allocation, no memset / memcpy, no atomics (every word has exactly one writer per
// launch), no buffer needs initialisation, and the launch count and every grid depend on B, H, W, levels and iters alone, so a call
// captures into a hipGraph as a linear chain.
//
//   df_luma_kernel      level 0 of both pyramids: V = 16 Y (int16), m = mask > 0.5 (uint8)
//   df_down_kernel      one level down: the 5x5 binomial of m V, normalised by the same filter of m
//   df_init_kernel      the start of a level: zero, or twice the coarser level's flow at (y >> 1, x >> 1)
//   df_iterate_kernel   one workgroup per 32x16 tile: gx, gy, It (int16) and w (uint8) of the tile and a halo of `radius` into LDS, the nine
//                       window sums separably (rows into LDS as int32, columns in registers as int64), the fp64 solve, the clamped update
//   df_median_kernel    the 3x3 median of each flow component, clamped border; on the last iteration of level 0 also flow = U / 256
#include "common.h"

#define DF_MIN_SIDE 16
#define DF_MAX_SIDE 1024
#define DF_MAX_BATCH 64
#define DF_MAX_LEVELS 8
#define DF_MAX_ITERS 16
#define DF_MAX_RADIUS 7
#define DF_MAX_DAMPING (1 << 24)
#define DF_SPLIT_SIDE 32                // a level is halved while its smaller side is at least this
#define DF_DEN_MIN 128                  // a coarser pixel is valid when half of its 256 binomial weights were
#define DF_TW 32
#define DF_TH 16
#define DF_SW (DF_TW + 2 * DF_MAX_RADIUS)
#define DF_SH (DF_TH + 2 * DF_MAX_RADIUS)
#define DF_THREADS 256

// the saver's pixel: trunc(clamp(x, 0, 255)); NaN and -Inf read 0, +Inf 255
__device__ __forceinline__ int df_pixel(float v) { return (int)fminf(fmaxf(v, 0.f), 255.f); }

// planes z < B come from image 1, the others from image 2; mask: fp32, `mc` channels per item of which channel 0 is read, or null = all set
__global__ void __launch_bounds__(DF_THREADS) df_luma_kernel(const float* __restrict__ img1, const float* __restrict__ img2, const float* __restrict__ mask1, int mc1,
                                                              const float* __restrict__ mask2, int mc2, int B, int hw, int16_t* __restrict__ V, uint8_t* __restrict__ M) {
    const int i = blockIdx.x * DF_THREADS + threadIdx.x, z = blockIdx.y;
    if (i >= hw) return;
    const bool first = z < B;
    const int b = first ? z : z - B;
    const float* img = (first ? img1 : img2) + (size_t)b * 3 * hw;
    const float* mask = first ? mask1 : mask2;
    const int r = df_pixel(img[i]), g = df_pixel(img[(size_t)hw + i]), bl = df_pixel(img[2 * (size_t)hw + i]);
    V[(size_t)z * hw + i] = (int16_t)(16 * ((19595 * r + 38470 * g + 7471 * bl + 0x8000) >> 16));
    M[(size_t)z * hw + i] = mask ? (uint8_t)(mask[(size_t)b * (first ? mc1 : mc2) * hw + i] > 0.5f) : (uint8_t)1;      // (NaN > 0.5 is false)
}

__global__ void __launch_bounds__(DF_THREADS) df_down_kernel(const int16_t* __restrict__ V, const uint8_t* __restrict__ M, int H, int W, int Hc, int Wc,
                                                              int16_t* __restrict__ Vc, uint8_t* __restrict__ Mc) {
    const int i = blockIdx.x * DF_THREADS + threadIdx.x, z = blockIdx.y;
    if (i >= Hc * Wc) return;
    const int y = i / Wc, x = i - y * Wc;
    const int16_t* v = V + (size_t)z * H * W;
    const uint8_t* m = M + (size_t)z * H * W;
    int num = 0, den = 0;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        const int yy = min(max(2 * y + a - 2, 0), H - 1), ga = (a == 0 || a == 4) ? 1 : (a == 2 ? 6 : 4);
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            const int xx = min(max(2 * x + c - 2, 0), W - 1), g = ga * ((c == 0 || c == 4) ? 1 : (c == 2 ? 6 : 4));
            if (m[(size_t)yy * W + xx]) num += g * v[(size_t)yy * W + xx], den += g;
        }
    }
    Vc[(size_t)z * Hc * Wc + i] = (int16_t)(den > 0 ? (2 * num + den) / (2 * den) : 0);
    Mc[(size_t)z * Hc * Wc + i] = (uint8_t)(den >= DF_DEN_MIN);
}

// U int32 [B,2,H,W]; Uc the coarser level's [B,2,Hc,Wc], or null at the coarsest level
__global__ void __launch_bounds__(DF_THREADS) df_init_kernel(const int32_t* __restrict__ Uc, int H, int W, int Hc, int Wc, int32_t* __restrict__ U) {
    const int i = blockIdx.x * DF_THREADS + threadIdx.x, z = blockIdx.y;
    if (i >= H * W) return;
    const int y = i / W, x = i - y * W;
    U[(size_t)z * H * W + i] = Uc ? 2 * Uc[(size_t)z * Hc * Wc + (size_t)(y >> 1) * Wc + (x >> 1)] : 0;
}

__global__ void __launch_bounds__(DF_THREADS) df_iterate_kernel(const int16_t* __restrict__ V1, const int16_t* __restrict__ V2, const uint8_t* __restrict__ M1,
                                                                 const uint8_t* __restrict__ M2, const int32_t* __restrict__ U, int H, int W, int r, long long damping,
                                                                 int32_t* __restrict__ Uout, uint8_t* __restrict__ sup) {
    __shared__ int16_t sgx[DF_SH][DF_SW], sgy[DF_SH][DF_SW], sit[DF_SH][DF_SW];
    __shared__ uint8_t sw[DF_SH][DF_SW];
    __shared__ int32_t hs[9][DF_SH][DF_TW];
    const int t = threadIdx.x, b = blockIdx.z, x0 = blockIdx.x * DF_TW, y0 = blockIdx.y * DF_TH;
    const size_t hw = (size_t)H * W;
    const int16_t *v1 = V1 + b * hw, *v2 = V2 + b * hw;
    const uint8_t *m1 = M1 + b * hw, *m2 = M2 + b * hw;
    const int32_t *ux = U + 2 * b * hw, *uy = ux + hw;
    const int cw = DF_TW + 2 * r, ch = DF_TH + 2 * r, side = 2 * r + 1;
    // ---- gx, gy, It and w of the tile and its halo; a pixel without weight (outside the image included) contributes 0 to every sum
    for (int e = t; e < cw * ch; e += DF_THREADS) {
        const int ty = e / cw, tx = e - ty * cw, y = y0 - r + ty, x = x0 - r + tx;
        int gx = 0, gy = 0, it = 0, w = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t q = (size_t)y * W + x;
            const int xl = max(x - 1, 0), xr = min(x + 1, W - 1), yu = max(y - 1, 0), yd = min(y + 1, H - 1);
            const size_t ql = (size_t)y * W + xl, qr = (size_t)y * W + xr, qu = (size_t)yu * W + x, qd = (size_t)yd * W + x;
            const int sx = 256 * x + ux[q], sy = 256 * y + uy[q];
            const int xs = sx >> 8, fx = sx & 255, ys = sy >> 8, fy = sy & 255;
            w = (m1[q] != 0) & (m1[ql] != 0) & (m1[qr] != 0) & (m1[qu] != 0) & (m1[qd] != 0);   // (a mask byte is set iff nonzero: w is 0 or 1, it is summed below)
            if (w && xs >= 0 && xs <= W - 2 && ys >= 0 && ys <= H - 2) {
                const size_t p = (size_t)ys * W + xs;
                if ((m2[p] != 0) & (m2[p + 1] != 0) & (m2[p + W] != 0) & (m2[p + W + 1] != 0)) {
                    const int J = ((256 - fx) * (256 - fy) * v2[p] + fx * (256 - fy) * v2[p + 1] + (256 - fx) * fy * v2[p + W] + fx * fy * v2[p + W + 1] + (1 << 15)) >> 16;
                    gx = v1[qr] - v1[ql], gy = v1[qd] - v1[qu], it = J - v1[q];
                } else
                    w = 0;
            } else
                w = 0;
        }
        sgx[ty][tx] = (int16_t)gx, sgy[ty][tx] = (int16_t)gy, sit[ty][tx] = (int16_t)it, sw[ty][tx] = (uint8_t)w;
    }
    __syncthreads();
    // ---- row sums over 2r + 1 columns: |term| <= 8160^2, 15 of them stay below 2^30
    for (int e = t; e < ch * DF_TW; e += DF_THREADS) {
        const int ty = e >> 5, cx = e & 31;
        int s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int d = 0; d < side; ++d) {
            const int gx = sgx[ty][cx + d], gy = sgy[ty][cx + d], it = sit[ty][cx + d];
            s[0] += sw[ty][cx + d], s[1] += gx, s[2] += gy, s[3] += it;
            s[4] += gx * gx, s[5] += gx * gy, s[6] += gy * gy, s[7] += gx * it, s[8] += gy * it;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) hs[k][ty][cx] = s[k];
    }
    __syncthreads();
    // ---- column sums, the zero-mean normal equations (exact in int64), the fp64 solve
#pragma unroll
    for (int j = 0; j < DF_TW * DF_TH / DF_THREADS; ++j) {
        const int p = t + DF_THREADS * j, py = p >> 5, px = p & 31, y = y0 + py, x = x0 + px;
        if (y >= H || x >= W) continue;
        long long s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int d = 0; d < side; ++d)
#pragma unroll
            for (int k = 0; k < 9; ++k) s[k] += hs[k][py + d][px];
        const long long n = s[0], Sx = s[1], Sy = s[2], St = s[3];
        const long long A = n * s[4] - Sx * Sx + damping * n * n, Cq = n * s[6] - Sy * Sy + damping * n * n, Bm = n * s[5] - Sx * Sy;
        const long long bx = n * s[7] - Sx * St, by = n * s[8] - Sy * St;
        const double Ad = (double)A, Cd = (double)Cq, Bd = (double)Bm, bxd = (double)bx, byd = (double)by;
        const double det = Ad * Cd - Bd * Bd;
        const bool ok = n >= side * side / 4 && det > 0.0;
        int dx = 0, dy = 0;
        if (ok) {
            const double ddx = -512.0 * ((Cd * bxd - Bd * byd) / det), ddy = -512.0 * ((Ad * byd - Bd * bxd) / det);
            dx = (int)rint(fmin(fmax(ddx, -256.0), 256.0)), dy = (int)rint(fmin(fmax(ddy, -256.0), 256.0));
        }
        const size_t q = (size_t)y * W + x;
        Uout[2 * b * hw + q] = ux[q] + dx, Uout[(2 * b + 1) * hw + q] = uy[q] + dy;
        sup[b * hw + q] = (uint8_t)ok;
    }
}

#define DF_SORT2(a, b)                  \
    do {                                \
        const int lo__ = min(a, b);     \
        b = max(a, b), a = lo__;        \
    } while (0)

// planes = B * 2; flow (fp32, same shape) is null except behind the last iteration of level 0
__global__ void __launch_bounds__(DF_THREADS) df_median_kernel(const int32_t* __restrict__ Uin, int H, int W, int32_t* __restrict__ U, float* __restrict__ flow) {
    const int i = blockIdx.x * DF_THREADS + threadIdx.x, z = blockIdx.y;
    if (i >= H * W) return;
    const int y = i / W, x = i - y * W;
    const int32_t* u = Uin + (size_t)z * H * W;
    int p[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) p[3 * a + c] = u[(size_t)min(max(y + a - 1, 0), H - 1) * W + min(max(x + c - 1, 0), W - 1)];
    DF_SORT2(p[1], p[2]); DF_SORT2(p[4], p[5]); DF_SORT2(p[7], p[8]); DF_SORT2(p[0], p[1]); DF_SORT2(p[3], p[4]); DF_SORT2(p[6], p[7]);
    DF_SORT2(p[1], p[2]); DF_SORT2(p[4], p[5]); DF_SORT2(p[7], p[8]); DF_SORT2(p[0], p[3]); DF_SORT2(p[5], p[8]); DF_SORT2(p[4], p[7]);
    DF_SORT2(p[3], p[6]); DF_SORT2(p[1], p[4]); DF_SORT2(p[2], p[5]); DF_SORT2(p[4], p[7]); DF_SORT2(p[4], p[2]); DF_SORT2(p[6], p[4]);
    DF_SORT2(p[4], p[2]);
    U[(size_t)z * H * W + i] = p[4];
    if (flow) flow[(size_t)z * H * W + i] = (float)p[4] * (1.0f / 256.0f);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct df_region {
    const void* p;
    int64_t bytes;
    bool out;
};

// no null pointer (a region of 0 bytes is an absent optional operand); an output overlaps nothing
static bool df_regions_ok(const df_region* r, int n) {
    for (int i = 0; i < n; ++i)
        if (!r[i].p && r[i].bytes) return false;
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            if ((!r[i].out && !r[j].out) || !r[i].bytes || !r[j].bytes) continue;
            const uintptr_t a = (uintptr_t)r[i].p, b = (uintptr_t)r[j].p;
            if (a < b + (uintptr_t)r[j].bytes && b < a + (uintptr_t)r[i].bytes) return false;
        }
    return true;
}

static bool df_shape_ok(int B, int H, int W) {
    return B >= 1 && B <= DF_MAX_BATCH && H >= DF_MIN_SIDE && H <= DF_MAX_SIDE && W >= DF_MIN_SIDE && W <= DF_MAX_SIDE;
}
static bool df_params_ok(int iters, int radius, int damping) {
    return iters >= 1 && iters <= DF_MAX_ITERS && radius >= 1 && radius <= DF_MAX_RADIUS && damping >= 0 && damping <= DF_MAX_DAMPING;
}
static bool df_mask_ok(const float* mask, int mc) { return !mask || mc == 1 || mc == 3; }

// workspace of st_dense_flow, every region rounded up to 16 bytes.  Per level l of L: V int16 [2,B,Hl,Wl], m uint8 [2,B,Hl,Wl] (image 1's
// planes first), U int32 [B,2,Hl,Wl]; then the flow before the median int32 [B,2,H,W] and the support of an iteration uint8 [B,H,W]
struct df_layout {
    int L, h[DF_MAX_LEVELS], w[DF_MAX_LEVELS];
    int64_t v[DF_MAX_LEVELS], m[DF_MAX_LEVELS], u[DF_MAX_LEVELS], tmp, sup, total;
};
static bool df_plan(int B, int H, int W, int levels, df_layout& P) {
    if (!df_shape_ok(B, H, W) || levels < 1 || levels > DF_MAX_LEVELS) return false;
    int64_t at = 0;
    auto take = [&](int64_t bytes) { const int64_t o = at; at += (bytes + 15) & ~(int64_t)15; return o; };
    P.L = 0;
    for (int l = 0; l < DF_MAX_LEVELS; ++l) P.h[l] = P.w[l] = 0, P.v[l] = P.m[l] = P.u[l] = -1;
    for (int l = 0, h = H, w = W;; ++l) {
        const int64_t px = (int64_t)B * h * w;
        P.h[l] = h, P.w[l] = w, P.L = l + 1;
        P.v[l] = take(4 * px), P.m[l] = take(2 * px), P.u[l] = take(8 * px);
        if (l + 1 >= levels || (h < w ? h : w) < DF_SPLIT_SIDE) break;
        h = (h + 1) / 2, w = (w + 1) / 2;
    }
    P.tmp = take(8 * (int64_t)B * H * W), P.sup = take((int64_t)B * H * W);
    P.total = at;
    return true;
}

static dim3 df_flat_grid(int64_t px, int planes) { return dim3((unsigned)((px + DF_THREADS - 1) / DF_THREADS), planes); }

static int df_launch_pyramid(const float* img1, const float* img2, const float* mask1, int mc1, const float* mask2, int mc2, int B, const df_layout& P, char* ws,
                             hipStream_t s) {
    df_luma_kernel<<<df_flat_grid((int64_t)P.h[0] * P.w[0], 2 * B), DF_THREADS, 0, s>>>(img1, img2, mask1, mc1, mask2, mc2, B, P.h[0] * P.w[0], (int16_t*)(ws + P.v[0]),
                                                                                           (uint8_t*)(ws + P.m[0]));
    ST_CHECK_LAUNCH();
    for (int l = 1; l < P.L; ++l) {
        df_down_kernel<<<df_flat_grid((int64_t)P.h[l] * P.w[l], 2 * B), DF_THREADS, 0, s>>>((const int16_t*)(ws + P.v[l - 1]), (const uint8_t*)(ws + P.m[l - 1]), P.h[l - 1],
                                                                                               P.w[l - 1], P.h[l], P.w[l], (int16_t*)(ws + P.v[l]), (uint8_t*)(ws + P.m[l]));
        ST_CHECK_LAUNCH();
    }
    return ST_OK;
}

// one iteration: u -> tmp (the update), tmp -> u_out (the median); u_out may be u itself
static int df_launch_iterate(const int16_t* v1, const int16_t* v2, const uint8_t* m1, const uint8_t* m2, const int32_t* u, int B, int H, int W, int radius, int damping,
                             int32_t* tmp, int32_t* u_out, uint8_t* sup, float* flow, hipStream_t s) {
    df_iterate_kernel<<<dim3((W + DF_TW - 1) / DF_TW, (H + DF_TH - 1) / DF_TH, B), DF_THREADS, 0, s>>>(v1, v2, m1, m2, u, H, W, radius, (long long)damping, tmp, sup);
    ST_CHECK_LAUNCH();
    df_median_kernel<<<df_flat_grid((int64_t)H * W, 2 * B), DF_THREADS, 0, s>>>(tmp, H, W, u_out, flow);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

extern "C" int st_dense_flow_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t levels, int64_t* bytes_host) {
    df_layout P;
    if (!bytes_host || !df_plan(B, H, W, levels, P)) return ST_EINVAL;
    *bytes_host = P.total;
    return ST_OK;
}

extern "C" int st_dense_flow_workspace_layout(int32_t B, int32_t H, int32_t W, int32_t levels, int64_t* offsets_host) {
    df_layout P;
    if (!offsets_host || !df_plan(B, H, W, levels, P)) return ST_EINVAL;
    offsets_host[0] = P.L;
    for (int l = 0; l < DF_MAX_LEVELS; ++l) offsets_host[1 + l] = P.v[l], offsets_host[9 + l] = P.m[l], offsets_host[17 + l] = P.u[l];
    offsets_host[25] = P.tmp, offsets_host[26] = P.sup, offsets_host[27] = P.total;
    return ST_OK;
}

extern "C" int st_dense_flow_pyramid(const float* img1, const float* img2, const float* mask1, int32_t mask1_channels, const float* mask2, int32_t mask2_channels,
                                     int32_t B, int32_t H, int32_t W, int32_t levels, void* workspace, int64_t workspace_bytes, void* stream) {
    df_layout P;
    if (!df_plan(B, H, W, levels, P) || !df_mask_ok(mask1, mask1_channels) || !df_mask_ok(mask2, mask2_channels)) return ST_EINVAL;
    if (workspace_bytes < P.total || ((uintptr_t)workspace & 15)) return ST_EINVAL;
    const int64_t px = (int64_t)B * H * W;
    const df_region r[5] = {{img1, 12 * px, false}, {img2, 12 * px, false}, {mask1, mask1 ? 4 * mask1_channels * px : 0, false},
                            {mask2, mask2 ? 4 * mask2_channels * px : 0, false}, {workspace, P.total, true}};
    if (!df_regions_ok(r, 5)) return ST_EINVAL;
    return df_launch_pyramid(img1, img2, mask1, mask1_channels, mask2, mask2_channels, B, P, (char*)workspace, (hipStream_t)stream);
}

extern "C" int st_dense_flow_iterate(const int16_t* v1, const int16_t* v2, const uint8_t* m1, const uint8_t* m2, const int32_t* u, int32_t B, int32_t H, int32_t W,
                                     int32_t radius, int32_t damping, int32_t* u_out, uint8_t* support_out, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!df_shape_ok(B, H, W) || !df_params_ok(1, radius, damping)) return ST_EINVAL;
    const int64_t px = (int64_t)B * H * W;
    if (workspace_bytes < 8 * px || ((uintptr_t)workspace & 15)) return ST_EINVAL;
    const df_region r[8] = {{v1, 2 * px, false}, {v2, 2 * px, false}, {m1, px, false}, {m2, px, false}, {u, 8 * px, false}, {u_out, 8 * px, true}, {support_out, px, true},
                            {workspace, 8 * px, true}};
    if (!df_regions_ok(r, 8)) return ST_EINVAL;
    return df_launch_iterate(v1, v2, m1, m2, u, B, H, W, radius, damping, (int32_t*)workspace, u_out, support_out, nullptr, (hipStream_t)stream);
}

extern "C" int st_dense_flow(const float* img1, const float* img2, const float* mask1, int32_t mask1_channels, const float* mask2, int32_t mask2_channels, int32_t B,
                             int32_t H, int32_t W, int32_t levels, int32_t iters, int32_t radius, int32_t damping, float* flow_out, uint8_t* support_out, void* workspace,
                             int64_t workspace_bytes, void* stream) {
    df_layout P;
    if (!df_plan(B, H, W, levels, P) || !df_params_ok(iters, radius, damping) || !df_mask_ok(mask1, mask1_channels) || !df_mask_ok(mask2, mask2_channels)) return ST_EINVAL;
    if (workspace_bytes < P.total || ((uintptr_t)workspace & 15)) return ST_EINVAL;
    const int64_t px = (int64_t)B * H * W;
    const df_region r[7] = {{img1, 12 * px, false}, {img2, 12 * px, false}, {mask1, mask1 ? 4 * mask1_channels * px : 0, false},
                            {mask2, mask2 ? 4 * mask2_channels * px : 0, false}, {flow_out, 8 * px, true}, {support_out, px, true}, {workspace, P.total, true}};
    if (!df_regions_ok(r, 7)) return ST_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int rc = df_launch_pyramid(img1, img2, mask1, mask1_channels, mask2, mask2_channels, B, P, ws, s);
    if (rc) return rc;
    for (int l = P.L - 1; l >= 0; --l) {
        const int h = P.h[l], w = P.w[l];
        const int64_t lpx = (int64_t)B * h * w;
        int32_t* u = (int32_t*)(ws + P.u[l]);
        const bool top = l + 1 == P.L;
        df_init_kernel<<<df_flat_grid((int64_t)h * w, 2 * B), DF_THREADS, 0, s>>>(top ? nullptr : (const int32_t*)(ws + P.u[l + 1]), h, w, top ? 0 : P.h[l + 1],
                                                                                     top ? 0 : P.w[l + 1], u);
        ST_CHECK_LAUNCH();
        const int16_t* v = (const int16_t*)(ws + P.v[l]);
        const uint8_t* m = (const uint8_t*)(ws + P.m[l]);
        for (int k = 0; k < iters; ++k) {
            const bool last = l == 0 && k + 1 == iters;
            rc = df_launch_iterate(v, v + lpx, m, m + lpx, u, B, h, w, radius, damping, (int32_t*)(ws + P.tmp), u, last ? support_out : (uint8_t*)(ws + P.sup),
                                   last ? flow_out : nullptr, s);
            if (rc) return rc;
        }
    }
    return ST_OK;
}
