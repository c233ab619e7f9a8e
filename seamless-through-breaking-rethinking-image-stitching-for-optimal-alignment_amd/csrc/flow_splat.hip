// Warm start across frames: the forward splat of a low-resolution flow (core/utils/utils.py:32-60, RAFT's forward_interpolate) as
// one kernel on the device.  Built with -ffp-contract=off: every fp64 rounding below is part of the contract.
//
// Contract (restated on the CPU in tests/_forward_interp_ref.py).  Source pixel s = (i, j) lands at px = double(j) + double(dx[s]),
// py = double(i) + double(dy[s]); it is valid iff 0 < px < W and 0 < py < H (a NaN fails every comparison).  Query (qi, qj) takes
// (dx, dy) of the valid source minimising (qj - px)^2 + (qi - py)^2 in fp64; equal distances go to the lowest source index; a batch
// element without a valid source gives zeros.
//
// Brute force: N^2 point-query pairs per batch element (N = 4096 at the product's size), exact, no data-dependent structure.  A
// 256-thread workgroup owns 16 queries; lane = (query, slice): each of 16 slices scans 1/16 of every LDS-staged chunk of landing
// points in ascending source order with a strict <, so within a slice the lowest index wins a tie for free; the 16 slices' winners
// are merged on (distance, index).  Invalid sources are staged as px = +inf (distance +inf, never < anything): no compaction pass.
// B * N / 16 workgroups: 512 for the two directions of one 512x512 pair, two per CU.
#include "common.h"
#include "../../include/stitch_gfx950.h"

namespace {

constexpr int SPLAT_THREADS = 256;
constexpr int SPLAT_QUERIES = 16;                                   // per workgroup
constexpr int SPLAT_SLICES = SPLAT_THREADS / SPLAT_QUERIES;         // of the source range, per query
constexpr int SPLAT_CHUNK = 2048;                                   // landing points staged per pass: 32 KB of LDS
constexpr int SPLAT_MAX_N = 1 << 16;

// flow of source s of batch element b: NCHW [B,2,H,W], or the decoder's coords1 rows [B*N,2] minus the pixel grid (decoder.py:344)
template <bool ROWS>
__device__ __forceinline__ void splat_flow_at(const float* __restrict__ src, int b, int s, int N, int W, float& dx, float& dy) {
    if (ROWS) {
        const size_t r = (size_t)b * N + s;
        dx = src[r * 2] - (float)(s % W);
        dy = src[r * 2 + 1] - (float)(s / W);
    } else {
        dx = src[(size_t)b * 2 * N + s];
        dy = src[((size_t)b * 2 + 1) * N + s];
    }
}

template <bool ROWS>
__global__ __launch_bounds__(SPLAT_THREADS) void flow_forward_interpolate_kernel(const float* __restrict__ src, float* __restrict__ out,
                                                                                  int H, int W) {
    __shared__ double2 pos[SPLAT_CHUNK];
    __shared__ double red_d[SPLAT_THREADS];
    __shared__ int red_i[SPLAT_THREADS];
    const int N = H * W, b = blockIdx.y, t = threadIdx.x;
    const int ql = t % SPLAT_QUERIES, sl = t / SPLAT_QUERIES;
    const int q = blockIdx.x * SPLAT_QUERIES + ql;                  // past N in the last workgroup: scanned like any other, never stored
    const double qx = (double)(q % W), qy = (double)(q / W);
    const double inf = __builtin_huge_val();
    double bd = inf;
    int bi = -1;
    for (int c0 = 0; c0 < N; c0 += SPLAT_CHUNK) {
        __syncthreads();                                            // the previous chunk has been scanned
        for (int k = t; k < SPLAT_CHUNK; k += SPLAT_THREADS) {
            const int s = c0 + k;
            double px = inf, py = 0.0;
            if (s < N) {
                float dx, dy;
                splat_flow_at<ROWS>(src, b, s, N, W, dx, dy);
                const double x = (double)(s % W) + (double)dx, y = (double)(s / W) + (double)dy;
                if (x > 0.0 && x < (double)W && y > 0.0 && y < (double)H) { px = x; py = y; }
            }
            pos[k] = make_double2(px, py);
        }
        __syncthreads();
        const int k0 = sl * (SPLAT_CHUNK / SPLAT_SLICES);
#pragma unroll 8
        for (int k = k0; k < k0 + SPLAT_CHUNK / SPLAT_SLICES; ++k) {
            const double2 p = pos[k];
            const double ex = qx - p.x, ey = qy - p.y;
            const double d = ex * ex + ey * ey;
            if (d < bd) { bd = d; bi = c0 + k; }
        }
    }
    red_d[t] = bd;
    red_i[t] = bi;
    __syncthreads();
    if (t >= SPLAT_QUERIES || q >= N) return;
    for (int s2 = 1; s2 < SPLAT_SLICES; ++s2) {
        const double d = red_d[s2 * SPLAT_QUERIES + t];
        const int i = red_i[s2 * SPLAT_QUERIES + t];
        if (i >= 0 && (d < bd || (d == bd && i < bi))) { bd = d; bi = i; }
    }
    float dx = 0.f, dy = 0.f;
    if (bi >= 0) splat_flow_at<ROWS>(src, b, bi, N, W, dx, dy);
    out[(size_t)b * 2 * N + q] = dx;
    out[((size_t)b * 2 + 1) * N + q] = dy;
}

}  // namespace

extern "C" int st_flow_forward_interpolate(const float* src, int32_t src_is_coords_rows, float* out, int32_t B, int32_t H, int32_t W,
                                           void* stream) {
    if (!src || !out || src == out || B < 1 || B > 65535 || H < 1 || W < 1 || (int64_t)H * W > SPLAT_MAX_N) return ST_EINVAL;
    const dim3 grid((H * W + SPLAT_QUERIES - 1) / SPLAT_QUERIES, B);
    if (src_is_coords_rows)
        hipLaunchKernelGGL(flow_forward_interpolate_kernel<true>, grid, dim3(SPLAT_THREADS), 0, (hipStream_t)stream, src, out, H, W);
    else
        hipLaunchKernelGGL(flow_forward_interpolate_kernel<false>, grid, dim3(SPLAT_THREADS), 0, (hipStream_t)stream, src, out, H, W);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
