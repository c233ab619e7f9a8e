// What csrc/features.hip (feature_align) and csrc/features_ms.hip (feature_align_ms) both need, written once: the contract's constants, the
// hash and the BRIEF pattern, the fp64 four-point solve, the inlier test, the H / motion / info tail, the argument checks, and the host
// launchers of the kernels of features.hip that the multi-scale front end reuses as they are.  Both files are compiled with
// -ffp-contract=off: every product and sum below rounds on its own.
#pragma once
#include "common.h"

#define FT_MIN_SIDE 64
#define FT_MAX_SIDE 1024
#define FT_MAX_BATCH 64
#define FT_MAX_HYP 65536
#define FT_CELL 32
#define FT_PER_CELL 4
#define FT_BORDER 16
#define FT_WORDS 8
#define FT_MAX_DIST 80                  // a match needs d1 < 80 of 256 bits ...
#define FT_RATIO_NUM 8                  // ... and 10 d1 < 8 d2
#define FT_RATIO_DEN 10
#define FT_NO_DIST 257
#define FT_MIN_MATCHES 8
#define FT_PIVOT_MIN 1e-10
#define FT_PATTERN_KEY 0x9E3779B9u
#define FT_CHUNK 1024                   // candidates / matches staged in LDS at a time
#define FT_THREADS 256

__host__ __device__ constexpr uint32_t ft_fmix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

// pair k compares the box sums at p + (v[4k], v[4k+1]) and p + (v[4k+2], v[4k+3]) (x, y); every offset in -12..12
struct ft_pattern_t {
    int8_t v[1024];
};
constexpr ft_pattern_t ft_make_pattern() {
    ft_pattern_t p{};
    for (int i = 0; i < 1024; ++i) p.v[i] = (int8_t)((int)(ft_fmix32(FT_PATTERN_KEY ^ (uint32_t)i) % 25u) - 12);
    return p;
}

// the saver's pixel: trunc(clamp(x, 0, 255)); NaN and -Inf read 0, +Inf 255
__device__ __forceinline__ int ft_pixel(float v) { return (int)fminf(fmaxf(v, 0.f), 255.f); }

__device__ __forceinline__ long long ft_shfl_xor64(long long v, int o) {
    const int lo = __shfl_xor((int)(v & 0xFFFFFFFFll), o, 64), hi = __shfl_xor((int)(v >> 32), o, 64);
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

// (R descending, index ascending)
__device__ __forceinline__ bool ft_better(long long ra, int ia, long long rb, int ib) { return ra > rb || (ra == rb && ia < ib); }

__device__ __forceinline__ int ft_count(const int32_t* __restrict__ count, int b, int N) { return min(max(count[b], 0), N); }

// element `c` (0..8; 8 = right-hand side) of the two rows a match (x, y) -> (u, v) contributes to the system of h (h33 = 1)
__device__ __forceinline__ double ft_row0(int c, double x, double y, double u) {
    switch (c) {
        case 0: return x;
        case 1: return y;
        case 2: return 1.0;
        case 6: return -u * x;
        case 7: return -u * y;
        case 8: return u;
        default: return 0.0;
    }
}
__device__ __forceinline__ double ft_row1(int c, double x, double y, double v) {
    switch (c) {
        case 3: return x;
        case 4: return y;
        case 5: return 1.0;
        case 6: return -v * x;
        case 7: return -v * y;
        case 8: return v;
        default: return 0.0;
    }
}

// Gaussian elimination with partial pivoting (first row on ties) of the 8 x 9 system at a[(r * 9 + c) * S]; a pivot below FT_PIVOT_MIN
// (or a NaN) voids it
template <int S>
__device__ __forceinline__ bool ft_solve8(double* __restrict__ a, double (&x)[8]) {
    for (int c = 0; c < 8; ++c) {
        int piv = c;
        double best = fabs(a[(c * 9 + c) * S]);
        for (int r = c + 1; r < 8; ++r) {
            const double v = fabs(a[(r * 9 + c) * S]);
            if (v > best) best = v, piv = r;
        }
        if (!(best >= FT_PIVOT_MIN)) return false;
        if (piv != c)
            for (int k = 0; k < 9; ++k) {
                const double tmp = a[(c * 9 + k) * S];
                a[(c * 9 + k) * S] = a[(piv * 9 + k) * S];
                a[(piv * 9 + k) * S] = tmp;
            }
        const double pv = a[(c * 9 + c) * S];
        for (int r = c + 1; r < 8; ++r) {
            const double f = a[(r * 9 + c) * S] / pv;
            for (int k = c + 1; k < 9; ++k) a[(r * 9 + k) * S] = a[(r * 9 + k) * S] - f * a[(c * 9 + k) * S];
        }
    }
#pragma unroll
    for (int r = 7; r >= 0; --r) {
        double s = a[(r * 9 + 8) * S];
#pragma unroll
        for (int k = r + 1; k < 8; ++k) s = s - a[(r * 9 + k) * S] * x[k];
        x[r] = s / a[(r * 9 + r) * S];
    }
    return true;
}

// hypothesis k of an item with m >= 8 matches: four draws, void on a repeat; the 4-point system into a[(.) * S]; solved into h
template <int S>
__device__ __forceinline__ bool ft_hypothesis(const double* __restrict__ mc, int m, uint32_t seed, int k, double* __restrict__ a, double (&h)[8]) {
    const uint32_t key = ft_fmix32(seed ^ ft_fmix32((uint32_t)k));
    int idx[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) idx[t] = (int)(ft_fmix32(key ^ (uint32_t)(t + 1)) % (uint32_t)m);
    if (idx[0] == idx[1] || idx[0] == idx[2] || idx[0] == idx[3] || idx[1] == idx[2] || idx[1] == idx[3] || idx[2] == idx[3]) return false;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const double x = mc[4 * idx[t]], y = mc[4 * idx[t] + 1], u = mc[4 * idx[t] + 2], v = mc[4 * idx[t] + 3];
#pragma unroll
        for (int c = 0; c < 9; ++c) a[((2 * t) * 9 + c) * S] = ft_row0(c, x, y, u), a[((2 * t + 1) * 9 + c) * S] = ft_row1(c, x, y, v);
    }
    return ft_solve8<S>(a, h);
}

// a positive denominator and a squared one-sided reprojection error, in pixels, below thr^2
__device__ __forceinline__ bool ft_inlier(const double (&h)[8], double x, double y, double u, double v, double sx, double sy, double thr2) {
    const double den = (h[6] * x + h[7] * y) + 1.0;
    if (!(den > 0.0)) return false;
    const double px = ((h[0] * x + h[1] * y) + h[2]) / den, py = ((h[3] * x + h[4] * y) + h[5]) / den;
    const double ex = (px - u) * sx, ey = (py - v) * sy;
    return ex * ex + ey * ey < thr2;
}

__device__ __forceinline__ int ft_block_sum(int v, int* part) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}
__device__ __forceinline__ int ft_block_max(int v, int* part) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return max(max(part[0], part[1]), max(part[2], part[3]));
}

// one thread per item: the normalised model sh (h33 = 1) in pixel units, the motion of the four corners, info; the identity without a valid model
__device__ __forceinline__ void ft_write_model(const double (&sh)[8], bool have, int winner, int inliers, int min_inliers, int n1, int n2, int m, int H, int W, double sx,
                                               double sy, int b, float* motion, float* Hout, int32_t* info) {
    double h[9];
#pragma unroll
    for (int c = 0; c < 8; ++c) h[c] = sh[c];
    h[8] = 1.0;
    // pixel units: D Hn Nm with Nm = [[1/sx, 0, -1], [0, 1/sy, -1], [0, 0, 1]], D = [[sx, 0, sx], [0, sy, sy], [0, 0, 1]]
    double M[9], P[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) M[3 * r] = h[3 * r] / sx, M[3 * r + 1] = h[3 * r + 1] / sy, M[3 * r + 2] = (h[3 * r + 2] - h[3 * r]) - h[3 * r + 1];
#pragma unroll
    for (int c = 0; c < 3; ++c) P[c] = sx * M[c] + sx * M[6 + c], P[3 + c] = sy * M[3 + c] + sy * M[6 + c], P[6 + c] = M[6 + c];
    float Hf[9], mo[8];
    bool fin = true;
#pragma unroll
    for (int c = 0; c < 9; ++c) Hf[c] = c == 8 ? 1.f : (float)(P[c] / P[8]), fin = fin && isfinite(Hf[c]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {                        // the corners (0,0), (W,0), (0,H), (W,H): -1 / +1 in normalised units
        const double xn = q & 1 ? 1.0 : -1.0, yn = q & 2 ? 1.0 : -1.0, cx = q & 1 ? (double)W : 0.0, cy = q & 2 ? (double)H : 0.0;
        const double den = (h[6] * xn + h[7] * yn) + 1.0;
        const double ux = ((h[0] * xn + h[1] * yn) + h[2]) / den, uy = ((h[3] * xn + h[4] * yn) + h[5]) / den;
        mo[2 * q] = (float)((ux * sx + sx) - cx), mo[2 * q + 1] = (float)((uy * sy + sy) - cy);
        fin = fin && isfinite(mo[2 * q]) && isfinite(mo[2 * q + 1]);
    }
    const bool valid = have && fin && inliers >= min_inliers;
#pragma unroll
    for (int c = 0; c < 9; ++c) Hout[(size_t)b * 9 + c] = valid ? Hf[c] : (c % 4 == 0 ? 1.f : 0.f);
#pragma unroll
    for (int c = 0; c < 8; ++c) motion[(size_t)b * 8 + c] = valid ? mo[c] : 0.f;
    int32_t* o = info + (size_t)b * 8;
    o[0] = valid, o[1] = n1, o[2] = n2, o[3] = m, o[4] = have ? winner : -1, o[5] = inliers, o[6] = 0, o[7] = 0;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct ft_region {
    const void* p;
    int64_t bytes;
    bool out;
};

// no null pointer; an output overlaps nothing
static inline bool ft_regions_ok(const ft_region* r, int n) {
    for (int i = 0; i < n; ++i)
        if (!r[i].p) return false;
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            if (!r[i].out && !r[j].out) continue;
            const uintptr_t a = (uintptr_t)r[i].p, b = (uintptr_t)r[j].p;
            if (a < b + (uintptr_t)r[j].bytes && b < a + (uintptr_t)r[i].bytes) return false;
        }
    return true;
}

static inline bool ft_shape_ok(int B, int H, int W) {
    return B >= 1 && B <= FT_MAX_BATCH && H >= FT_MIN_SIDE && H <= FT_MAX_SIDE && W >= FT_MIN_SIDE && W <= FT_MAX_SIDE;
}
static inline int ft_cells(int side) { return (side + FT_CELL - 1) / FT_CELL; }
static inline int ft_slots(int H, int W) { return FT_PER_CELL * ft_cells(H) * ft_cells(W); }

static inline bool ft_params_ok(int max_hyp, double thr, int min_inliers) {
    return max_hyp >= 1 && max_hyp <= FT_MAX_HYP && thr > 0.0 && thr <= 1.7e308 && min_inliers >= 0;       // (a NaN thr fails both comparisons)
}

// launchers of features.hip's kernels that take the number of slots N as an argument (defined there): ft_match_kernel + ft_compact_kernel,
// and ft_hyp_kernel on normalised match coordinates
int ft_launch_match(const int32_t* kp1, const uint32_t* desc1, const int32_t* kp2, const uint32_t* desc2, int B, int N, int32_t* nn, int32_t* matches, int32_t* count,
                    hipStream_t s);
int ft_launch_hyp(const double* mc, const int32_t* count, int B, int H, int W, int N, int max_hyp, uint32_t seed, double thr2, int32_t* scores, hipStream_t s);
