// exposure compensation: overlap gains of the two warped images in front of multiband_blend (contract in README.md, "exposure
// compensation"; CPU restatement tests/_exposure_ref.py).  gfx950 only.  Every kernel of a call goes to the caller's stream, in order,
// inside the caller's workspace: no host synchronisation, no allocation, no memset / memcpy, no atomics (every word of the workspace has
// exactly one writer), so a call captures into a hipGraph as a linear chain.
//
//   ec_stats_kernel      per tile: N = |O in tile|, S1[R G B Y], S2[R G B Y] over the overlap O, uint32 (exact, order-free)
//   ec_global_kernel     the sum of the tile records in uint64, the four fp64 solves with the prior (1, 1): gains [4 planes][2] fp32
//   ec_tile_gain_kernel  blocks mode: per tile the solve with the global pair as prior, into the fp32 tables [sets][2][Th][Tw]
//   ec_smooth_kernel     blocks mode: one (0.25, 0.5, 0.25) pass along W then H with clamped indices, table A -> table B
//   ec_apply_kernel      g = the table interpolated bilinearly at the pixel, out = min(floor(p g + 0.5), 255) for both images
//
// Compiled with -ffp-contract=off: every product, sum and quotient below is one rounding, in the order written.
#include "common.h"

#define EC_MAX_SIDE 4096
#define EC_WORDS 9                      // a tile record: N, S1[4], S2[4]; planes R, G, B, Y
#define EC_GAIN_MIN 0.25
#define EC_GAIN_MAX 4.0

__device__ __forceinline__ uint32_t ec_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

__device__ __forceinline__ uint64_t ec_wave_sum64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
        v += (uint64_t)hi << 32 | lo;
    }
    return v;
}

// One 256-thread workgroup per tile (blockIdx.x = tile column, blockIdx.y = tile row).  A lane strides over the block x block positions of
// the tile (the row of a position is i >> lb, so a wave reads whole rows of the tile: 32 to 256 contiguous bytes), skips those outside the
// canvas (ragged tiles) and reads the six image samples only inside the overlap; a lane that skips reads pixel 0 instead and drops it.  The largest sum is 64 * 64 * 255 < 2^20.
__global__ void __launch_bounds__(256) ec_stats_kernel(const float* __restrict__ img1, const float* __restrict__ img2, const float* __restrict__ mask1,
                                                       const float* __restrict__ mask2, uint32_t* __restrict__ records, int H, int W, int lb) {
    __shared__ uint32_t part[4][EC_WORDS];
    const int block = 1 << lb, x0 = blockIdx.x << lb, y0 = blockIdx.y << lb;
    const size_t n = (size_t)H * W;
    uint32_t acc[EC_WORDS];
#pragma unroll
    for (int k = 0; k < EC_WORDS; ++k) acc[k] = 0;
    // four positions of a lane at a time, in three phases, so that the loads of a phase are in flight together: the masks, the samples
    // of the positions inside the overlap, the sums
    for (int i0 = threadIdx.x; i0 < block * block; i0 += 4 * 256) {
        size_t p[4];
        bool in[4], ov[4];
        float m1[4], m2[4], a[4][3], b[4][3];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = i0 + k * 256, y = y0 + (i >> lb), x = x0 + (i & (block - 1));
            in[k] = i < block * block && y < H && x < W;
            p[k] = (size_t)y * W + x;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const size_t q = in[k] ? p[k] : 0;              // (pixel 0 always exists: an unconditional load, so that the four are in flight together)
            m1[k] = mask1[q];
            m2[k] = mask2[q];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ov[k] = in[k] && m1[k] > 0.5f && m2[k] > 0.5f;
            const size_t q = ov[k] ? p[k] : 0;              // outside the overlap every lane reads pixel 0 (one cache line) and drops it
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                a[k][c] = img1[c * n + q];
                b[k][c] = img2[c * n + q];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t ua[3], ub[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                ua[c] = (uint32_t)st_u8_trunc(a[k][c]);
                ub[c] = (uint32_t)st_u8_trunc(b[k][c]);
                acc[1 + c] += ov[k] ? ua[c] : 0u;
                acc[5 + c] += ov[k] ? ub[c] : 0u;
            }
            acc[0] += ov[k] ? 1u : 0u;
            acc[4] += ov[k] ? (ua[0] * 19595u + ua[1] * 38470u + ua[2] * 7471u + 0x8000u) >> 16 : 0u;
            acc[8] += ov[k] ? (ub[0] * 19595u + ub[1] * 38470u + ub[2] * 7471u + 0x8000u) >> 16 : 0u;
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < EC_WORDS; ++k) {
        const uint32_t s = ec_wave_sum(acc[k]);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t* rec = records + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * EC_WORDS;
#pragma unroll
        for (int k = 0; k < EC_WORDS; ++k) rec[k] = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
    }
}

// solve(N, S1, S2, G1, G2) of the contract, every operation written out; the result clamped to [0.25, 4] and rounded to fp32
__device__ __forceinline__ void ec_solve(double N, double S1, double S2, double G1, double G2, double alpha, double beta, float& g1, float& g2) {
    if (N == 0.0) { g1 = (float)G1; g2 = (float)G2; return; }
    const double n2 = N * N;
    const double a11 = alpha * (S1 * S1) + beta * n2;
    const double a22 = alpha * (S2 * S2) + beta * n2;
    const double a12 = alpha * (S1 * S2);
    const double r1 = (beta * n2) * G1;
    const double r2 = (beta * n2) * G2;
    const double det = a11 * a22 - a12 * a12;
    const double x1 = (r1 * a22 + r2 * a12) / det;
    const double x2 = (r2 * a11 + r1 * a12) / det;
    g1 = (float)fmin(fmax(x1, EC_GAIN_MIN), EC_GAIN_MAX);
    g2 = (float)fmin(fmax(x2, EC_GAIN_MIN), EC_GAIN_MAX);
}

// One workgroup: the global record in uint64 (integer sums: the order does not matter), then lanes 0..3 solve one plane each.
// gains [4][2] fp32: plane R, G, B, Y; (G1, G2).  copy (may be null): the pairs of the `sets` planes the apply step reads, for the caller.
__global__ void __launch_bounds__(1024) ec_global_kernel(const uint32_t* __restrict__ records, int tiles, double alpha, double beta, float* __restrict__ gains,
                                                         float* __restrict__ copy, int sets) {
    __shared__ uint64_t part[16][EC_WORDS];
    __shared__ uint64_t total[EC_WORDS];
    uint64_t acc[EC_WORDS];
#pragma unroll
    for (int k = 0; k < EC_WORDS; ++k) acc[k] = 0;
    for (int t = threadIdx.x; t < tiles; t += 1024) {
#pragma unroll
        for (int k = 0; k < EC_WORDS; ++k) acc[k] += records[(size_t)t * EC_WORDS + k];
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < EC_WORDS; ++k) {
        const uint64_t s = ec_wave_sum64(acc[k]);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < EC_WORDS) {
        uint64_t s = 0;
        for (int w = 0; w < 16; ++w) s += part[w][threadIdx.x];
        total[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        float g1, g2;
        ec_solve((double)total[0], (double)total[1 + threadIdx.x], (double)total[5 + threadIdx.x], 1.0, 1.0, alpha, beta, g1, g2);
        gains[2 * threadIdx.x] = g1;
        gains[2 * threadIdx.x + 1] = g2;
        if (copy && (sets == 3 ? threadIdx.x < 3 : threadIdx.x == 3)) {       // mode "gain": the caller's copy of the 1 x 1 tables [sets][2]
            const int at = sets == 3 ? 2 * threadIdx.x : 0;
            copy[at] = g1;
            copy[at + 1] = g2;
        }
    }
}

// One thread per tile and set.  sets = 1: plane Y for all channels; sets = 3: planes R, G, B.  table [sets][2][tiles].
__global__ void __launch_bounds__(256) ec_tile_gain_kernel(const uint32_t* __restrict__ records, const float* __restrict__ gains, float* __restrict__ table,
                                                           int tiles, int sets, int min_count, double alpha, double beta) {
    const int t = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (t >= tiles) return;
    const int plane = sets == 1 ? 3 : s;
    const uint32_t* rec = records + (size_t)t * EC_WORDS;
    const uint32_t cnt = rec[0];
    const double N = cnt < (uint32_t)min_count ? 0.0 : (double)cnt;
    float g1, g2;
    ec_solve(N, (double)rec[1 + plane], (double)rec[5 + plane], (double)gains[2 * plane], (double)gains[2 * plane + 1], alpha, beta, g1, g2);
    table[((size_t)s * 2 + 0) * tiles + t] = g1;
    table[((size_t)s * 2 + 1) * tiles + t] = g2;
}

__device__ __forceinline__ float ec_smooth3(float a, float b, float c) { return (0.25f * a + 0.5f * b) + 0.25f * c; }

// One thread per table entry; blockIdx.y = one of the sets * 2 tables.  Along W at the three rows, each result one fp32 value, then along H.
__global__ void __launch_bounds__(256) ec_smooth_kernel(const float* __restrict__ in, float* __restrict__ out, int Th, int Tw) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= Th * Tw) return;
    const int i = t / Tw, j = t - i * Tw;
    const float* src = in + (size_t)blockIdx.y * Th * Tw;
    const int xl = max(j - 1, 0), xr = min(j + 1, Tw - 1);
    float r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* row = src + (size_t)min(max(i + k - 1, 0), Th - 1) * Tw;
        r[k] = ec_smooth3(row[xl], row[j], row[xr]);
    }
    out[(size_t)blockIdx.y * Th * Tw + t] = ec_smooth3(r[0], r[1], r[2]);
}

// the interpolation coordinate of pixel centre x in a table of n entries: clamped indices i0, i1 and the fraction f (all exact in fp32)
__device__ __forceinline__ void ec_coord(int x, float inv_block, int n, int& i0, int& i1, float& f) {
    const float u = ((float)x + 0.5f) * inv_block - 0.5f;
    const float fl = floorf(u);
    f = u - fl;
    const int i = (int)fl;
    i0 = min(max(i, 0), n - 1);
    i1 = min(max(i + 1, 0), n - 1);
}

__device__ __forceinline__ float ec_finish(float x, float g) { return fminf(floorf(st_u8_trunc(x) * g + 0.5f), 255.f); }

// One thread per VEC horizontally adjacent pixels of both images and the three channels.  VEC = 4 (W a multiple of 4, every pointer 16-byte
// aligned): 16-byte loads and stores; the four pixels share their table cell, because a cell boundary (x = block / 2 mod block) is a multiple
// of 4.  VEC = 1: any W.  table [sets][2][Th][Tw]; with sets = 1 the four entries of an image are read once for the three channels.
// In place (out == img) is fine: a thread reads its own pixels before it writes them and no other thread touches them.
template <int VEC>
__global__ void __launch_bounds__(256) ec_apply_kernel(const float* img1, const float* img2, const float* __restrict__ table, float* out1, float* out2,
                                                       int H, int W, int Th, int Tw, int sets, float inv_block) {
    const int wv = W / VEC;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= H * wv) return;
    const int y = t / wv, x = (t - y * wv) * VEC;
    const size_t n = (size_t)H * W, p = (size_t)y * W + x, tiles = (size_t)Th * Tw;
    int iy0, iy1, ix0, ix1;
    float fy, fx0;
    ec_coord(y, inv_block, Th, iy0, iy1, fy);
    ec_coord(x, inv_block, Tw, ix0, ix1, fx0);
    float fx[VEC];
    fx[0] = fx0;
#pragma unroll
    for (int k = 1; k < VEC; ++k) { int a, b; ec_coord(x + k, inv_block, Tw, a, b, fx[k]); }
    float g[2][VEC];
    for (int c = 0; c < 3; ++c) {
        if (c == 0 || sets == 3) {
#pragma unroll
            for (int im = 0; im < 2; ++im) {
                const float* tb = table + ((size_t)(sets == 3 ? c : 0) * 2 + im) * tiles;
                const float g00 = tb[(size_t)iy0 * Tw + ix0], g01 = tb[(size_t)iy0 * Tw + ix1], g10 = tb[(size_t)iy1 * Tw + ix0], g11 = tb[(size_t)iy1 * Tw + ix1];
#pragma unroll
                for (int k = 0; k < VEC; ++k)
                    g[im][k] = (g00 * (1.f - fx[k]) + g01 * fx[k]) * (1.f - fy) + (g10 * (1.f - fx[k]) + g11 * fx[k]) * fy;
            }
        }
        if constexpr (VEC == 4) {
            const float4 a = *reinterpret_cast<const float4*>(img1 + c * n + p), b = *reinterpret_cast<const float4*>(img2 + c * n + p);
            *reinterpret_cast<float4*>(out1 + c * n + p) = make_float4(ec_finish(a.x, g[0][0]), ec_finish(a.y, g[0][1 % VEC]), ec_finish(a.z, g[0][2 % VEC]), ec_finish(a.w, g[0][3 % VEC]));
            *reinterpret_cast<float4*>(out2 + c * n + p) = make_float4(ec_finish(b.x, g[1][0]), ec_finish(b.y, g[1][1 % VEC]), ec_finish(b.z, g[1][2 % VEC]), ec_finish(b.w, g[1][3 % VEC]));
        } else {
            const float a = img1[c * n + p], b = img2[c * n + p];
            out1[c * n + p] = ec_finish(a, g[0][0]);
            out2[c * n + p] = ec_finish(b, g[1][0]);
        }
    }
}

static int ec_log2_block(int block) { return block == 8 ? 3 : block == 16 ? 4 : block == 32 ? 5 : block == 64 ? 6 : -1; }

// workspace layout: records uint32 [Th Tw 9]; gains fp32 [4][2]; tables A and B fp32 [3][2][Th][Tw] -- each region rounded up to 16 bytes
struct ec_layout {
    int lb, Th, Tw;
    int64_t records, gains, table[2], total;
};

static bool ec_plan(int H, int W, int block, ec_layout& L) {
    L.lb = ec_log2_block(block);
    if (H < 1 || W < 1 || H > EC_MAX_SIDE || W > EC_MAX_SIDE || L.lb < 0) return false;
    L.Th = (H + block - 1) >> L.lb; L.Tw = (W + block - 1) >> L.lb;
    int64_t at = 0;
    auto take = [&](int64_t bytes) { const int64_t o = at; at += (bytes + 15) & ~(int64_t)15; return o; };
    const int64_t tiles = (int64_t)L.Th * L.Tw;
    L.records = take(4 * EC_WORDS * tiles);
    L.gains = take(4 * 8);
    L.table[0] = take(4 * 6 * tiles); L.table[1] = take(4 * 6 * tiles);
    L.total = at;
    return true;
}

static bool ec_overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

// an output may be its own input (in place) and nothing else: not a shifted view of it, not the other image, a mask or the other output
static bool ec_outputs_ok(const float* img1, const float* img2, const float* mask1, const float* mask2, const float* out1, const float* out2, int64_t n) {
    const int64_t img = 12 * n, msk = 4 * n;
    if (ec_overlap(out1, img, out2, img)) return false;
    if (out1 != img1 && ec_overlap(out1, img, img1, img)) return false;
    if (out2 != img2 && ec_overlap(out2, img, img2, img)) return false;
    if (ec_overlap(out1, img, img2, img) || ec_overlap(out2, img, img1, img)) return false;
    const float* outs[2] = {out1, out2};
    for (const float* o : outs) {
        if (mask1 && ec_overlap(o, img, mask1, msk)) return false;
        if (mask2 && ec_overlap(o, img, mask2, msk)) return false;
    }
    return true;
}

// the tables, which the apply step reads while it writes, overlap no output (st_exposure_compensate checks its gains_out, written before
// the images are read, against the inputs and the workspace as well); both at the byte length the call reads or writes, [sets][2][Th][Tw]
static bool ec_table_ok(const void* table, int64_t bytes, const float* out1, const float* out2, int64_t n) {
    return !ec_overlap(table, bytes, out1, 12 * n) && !ec_overlap(table, bytes, out2, 12 * n);
}

static int ec_stats_launch(const float* img1, const float* img2, const float* mask1, const float* mask2, int H, int W, const ec_layout& L, uint32_t* records,
                           hipStream_t s) {
    ec_stats_kernel<<<dim3(L.Tw, L.Th), 256, 0, s>>>(img1, img2, mask1, mask2, records, H, W, L.lb);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

static int ec_apply_launch(const float* img1, const float* img2, const float* table, int Th, int Tw, int sets, int H, int W, int lb, float* out1, float* out2,
                           hipStream_t s) {
    const float inv_block = 1.f / (float)(1 << lb);
    const uintptr_t bits = (uintptr_t)img1 | (uintptr_t)img2 | (uintptr_t)out1 | (uintptr_t)out2;
    if (W % 4 == 0 && (bits & 15) == 0)
        ec_apply_kernel<4><<<(H * (W / 4) + 255) / 256, 256, 0, s>>>(img1, img2, table, out1, out2, H, W, Th, Tw, sets, inv_block);
    else
        ec_apply_kernel<1><<<(H * W + 255) / 256, 256, 0, s>>>(img1, img2, table, out1, out2, H, W, Th, Tw, sets, inv_block);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

extern "C" int st_exposure_workspace_bytes(int32_t H, int32_t W, int32_t block) {
    ec_layout L;
    return ec_plan(H, W, block, L) ? (int)L.total : 0;
}

extern "C" int st_exposure_stats(const float* img1, const float* img2, const float* mask1, const float* mask2, int32_t H, int32_t W, int32_t block,
                                 int32_t* records, void* stream) {
    ec_layout L;
    if (!img1 || !img2 || !mask1 || !mask2 || !records || !ec_plan(H, W, block, L)) return ST_EINVAL;
    return ec_stats_launch(img1, img2, mask1, mask2, H, W, L, (uint32_t*)records, (hipStream_t)stream);
}

extern "C" int st_exposure_apply(const float* img1, const float* img2, const float* tables, int32_t Th, int32_t Tw, int32_t H, int32_t W, int32_t block,
                                 int32_t channels, float* out1, float* out2, void* stream) {
    ec_layout L;
    if (!img1 || !img2 || !tables || !out1 || !out2 || !ec_plan(H, W, block, L)) return ST_EINVAL;
    if (Th < 1 || Tw < 1 || Th > EC_MAX_SIDE || Tw > EC_MAX_SIDE) return ST_EINVAL;
    if (!ec_outputs_ok(img1, img2, nullptr, nullptr, out1, out2, (int64_t)H * W)) return ST_EINVAL;
    if (!ec_table_ok(tables, (int64_t)4 * (channels ? 3 : 1) * 2 * Th * Tw, out1, out2, (int64_t)H * W)) return ST_EINVAL;
    return ec_apply_launch(img1, img2, tables, Th, Tw, channels ? 3 : 1, H, W, L.lb, out1, out2, (hipStream_t)stream);
}

extern "C" int st_exposure_compensate(const float* img1, const float* img2, const float* mask1, const float* mask2, int32_t H, int32_t W, int32_t mode,
                                      int32_t block, int32_t channels, int32_t min_count, int32_t smooth, double sigma_n, double sigma_g, float* out1,
                                      float* out2, float* gains_out, void* workspace, int64_t workspace_bytes, void* stream) {
    ec_layout L;
    if (!img1 || !img2 || !mask1 || !mask2 || !out1 || !out2 || !workspace || !ec_plan(H, W, block, L)) return ST_EINVAL;
    if (mode < 0 || mode > 1 || smooth < 0 || smooth > 8 || min_count < 0) return ST_EINVAL;
    if (!(sigma_n > 0.0) || !(sigma_g > 0.0) || __builtin_isinf(sigma_n) || __builtin_isinf(sigma_g)) return ST_EINVAL;
    if (workspace_bytes < L.total || ((uintptr_t)workspace & 15)) return ST_EINVAL;
    if (!ec_outputs_ok(img1, img2, mask1, mask2, out1, out2, (int64_t)H * W)) return ST_EINVAL;
    {
        const int64_t n = (int64_t)H * W, img = 12 * n, msk = 4 * n, gb = (int64_t)4 * (channels ? 3 : 1) * 2 * (mode == 1 ? (int64_t)L.Th * L.Tw : 1);
        const void* ops[6] = {img1, img2, out1, out2, mask1, mask2};
        for (int i = 0; i < 6; ++i) {
            if (ec_overlap(workspace, L.total, ops[i], i < 4 ? img : msk)) return ST_EINVAL;
            if (gains_out && ec_overlap(gains_out, gb, ops[i], i < 4 ? img : msk)) return ST_EINVAL;
        }
        if (gains_out && ec_overlap(gains_out, gb, workspace, L.total)) return ST_EINVAL;
    }
    const double alpha = 1.0 / (sigma_n * sigma_n), beta = 1.0 / (sigma_g * sigma_g);
    if (!(alpha > 0.0) || !(beta > 0.0) || __builtin_isinf(alpha) || __builtin_isinf(beta)) return ST_EINVAL;     // a sigma whose square leaves fp64
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    uint32_t* records = (uint32_t*)(ws + L.records);
    float* gains = (float*)(ws + L.gains);
    float* tab[2] = {(float*)(ws + L.table[0]), (float*)(ws + L.table[1])};
    const int tiles = L.Th * L.Tw, sets = channels ? 3 : 1;
    int rc;
    if ((rc = ec_stats_launch(img1, img2, mask1, mask2, H, W, L, records, s)) != ST_OK) return rc;
    ec_global_kernel<<<1, 1024, 0, s>>>(records, tiles, alpha, beta, gains, mode == 0 ? gains_out : nullptr, sets);
    ST_CHECK_LAUNCH();
    const float* table = channels ? gains : gains + 6;                  // mode "gain": the 1 x 1 tables, [3][2] (R, G, B) or [1][2] (Y)
    int Th = 1, Tw = 1;
    if (mode == 1) {
        // table k of the chain: tile gains (k = 0), then one smoothing pass each; the last one is the caller's gains_out when given
        auto buf = [&](int k) { return k == smooth && gains_out ? gains_out : tab[k & 1]; };
        Th = L.Th; Tw = L.Tw;
        ec_tile_gain_kernel<<<dim3((tiles + 255) / 256, sets), 256, 0, s>>>(records, gains, buf(0), tiles, sets, min_count, alpha, beta);
        ST_CHECK_LAUNCH();
        for (int k = 0; k < smooth; ++k) {
            ec_smooth_kernel<<<dim3((tiles + 255) / 256, sets * 2), 256, 0, s>>>(buf(k), buf(k + 1), Th, Tw);
            ST_CHECK_LAUNCH();
        }
        table = buf(smooth);
    }
    if ((rc = ec_apply_launch(img1, img2, table, Th, Tw, sets, H, W, L.lb, out1, out2, s)) != ST_OK) return rc;
    return ST_OK;
}
