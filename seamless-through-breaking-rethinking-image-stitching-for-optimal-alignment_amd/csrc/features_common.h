// What csrc/features.hip (feature_align) and csrc/features_ms.hip (feature_align_ms) both need, written once: the contract's constants, the
// hash and the BRIEF pattern, the corner body of the two detect kernels (ft_corners), the fp64 four-point solve, the inlier test, the body
// of the two refit kernels (ft_refit) with its H / motion / info tail, the argument checks of the match and ransac entries, and the host
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

// The corners of one 32x32 cell at (x0, y0) of an H x W luma plane, from its tile in LDS (clamped to the plane, HALO >= 5 pixels around the
// cell): Sobel (halo 4) -> Harris response (halo 1), the 3x3 non-maximum suppression BORDER pixels inside the plane, the cell's best 4
// corners by (R descending, index ascending) into kp (the cell's 4 slots, (x, y) or (-1, -1)) and, in every thread, into win (y W + x or
// -1); and the 5x5 box sum of the luma into box (the plane).  All FT_THREADS threads call it, behind the barrier that follows the tile load.
template <int HALO, int BORDER>
__device__ __forceinline__ void ft_corners(const uint8_t (&sy)[FT_CELL + 2 * HALO][FT_CELL + 2 * HALO + 2], int x0, int y0, int H, int W, int32_t* __restrict__ kp,
                                           uint16_t* __restrict__ box, int (&win)[FT_PER_CELL]) {
    __shared__ int16_t sgx[40][40], sgy[40][40];
    __shared__ long long sr[34][34];
    __shared__ long long wr[4];
    __shared__ int wi[4];
    constexpr int O = HALO - 5;                              // the 42x42 tile that the response of the cell reads, inside this one
    const int t = threadIdx.x;
    for (int e = t; e < 40 * 40; e += FT_THREADS) {
        const int ty = e / 40, tx = e - ty * 40;
        const int y = y0 - 4 + ty, x = x0 - 4 + tx;
        int gx = 0, gy = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const int a = sy[O + ty][O + tx], b = sy[O + ty][O + tx + 1], c = sy[O + ty][O + tx + 2], d = sy[O + ty + 1][O + tx], f = sy[O + ty + 1][O + tx + 2],
                      g = sy[O + ty + 2][O + tx], h = sy[O + ty + 2][O + tx + 1], i = sy[O + ty + 2][O + tx + 2];
            gx = (c + 2 * f + i) - (a + 2 * d + g);
            gy = (g + 2 * h + i) - (a + 2 * b + c);
        }
        sgx[ty][tx] = (int16_t)gx, sgy[ty][tx] = (int16_t)gy;
    }
    __syncthreads();
    for (int e = t; e < 34 * 34; e += FT_THREADS) {
        const int ty = e / 34, tx = e - ty * 34;
        int a = 0, b = 0, c = 0;
        for (int dy = 0; dy < 7; ++dy)
#pragma unroll
            for (int dx = 0; dx < 7; ++dx) {
                const int gx = sgx[ty + dy][tx + dx], gy = sgy[ty + dy][tx + dx];
                a += gx * gx, b += gy * gy, c += gx * gy;
            }
        const long long A = a, Bq = b, Cq = c;
        sr[ty][tx] = 16 * (A * Bq - Cq * Cq) - (A + Bq) * (A + Bq);
    }
    __syncthreads();
    long long cr[4];
    int ci[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = t + FT_THREADS * j, py = p >> 5, px = p & 31, y = y0 + py, x = x0 + px;
        cr[j] = 0, ci[j] = 0x7FFFFFFF;
        if (y < H && x < W) {
            int s = 0;                                       // 5x5 box sum of the luma, terms outside the plane 0
            for (int dy = -2; dy <= 2; ++dy)
                for (int dx = -2; dx <= 2; ++dx)
                    if (y + dy >= 0 && y + dy < H && x + dx >= 0 && x + dx < W) s += sy[py + HALO + dy][px + HALO + dx];
            box[(size_t)y * W + x] = (uint16_t)s;
            if (y >= BORDER && y < H - BORDER && x >= BORDER && x < W - BORDER) {
                const long long r = sr[py + 1][px + 1];
                bool ok = r > 0;
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (!dy && !dx) continue;
                        const long long q = sr[py + 1 + dy][px + 1 + dx];
                        ok = ok && ((dy < 0 || (dy == 0 && dx < 0)) ? r > q : r >= q);
                    }
                if (ok) cr[j] = r, ci[j] = y * W + x;
            }
        }
    }
#pragma unroll                                               // (so that win[rank] is a register, not scratch)
    for (int rank = 0; rank < FT_PER_CELL; ++rank) {
        long long br = 0;
        int bi = 0x7FFFFFFF;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (ft_better(cr[j], ci[j], br, bi)) br = cr[j], bi = ci[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const long long qr = ft_shfl_xor64(br, o);
            const int qi = __shfl_xor(bi, o, 64);
            if (ft_better(qr, qi, br, bi)) br = qr, bi = qi;
        }
        if ((t & 63) == 0) wr[t >> 6] = br, wi[t >> 6] = bi;
        __syncthreads();
        br = wr[0], bi = wi[0];
#pragma unroll
        for (int v = 1; v < 4; ++v)
            if (ft_better(wr[v], wi[v], br, bi)) br = wr[v], bi = wi[v];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (ci[j] == bi) cr[j] = 0, ci[j] = 0x7FFFFFFF;     // taken (no candidate has the index of "none")
        win[rank] = br > 0 ? bi : -1;
        if (t == 0) kp[2 * rank] = br > 0 ? bi % W : -1, kp[2 * rank + 1] = br > 0 ? bi / W : -1;
    }
}

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

// The body of ft_refit_kernel and ftms_refit_kernel, one workgroup per item: winner, inlier mask, two least-squares refits (four interleaved
// partial sums per entry), H / motion / info.  CAP = the list entries whose inlier flags LDS holds; the entries prove N <= CAP.
template <int CAP>
__device__ __forceinline__ void ft_refit(const int32_t* kp1, const int32_t* kp2, const double* mc, const int32_t* count, const int32_t* scores, int H, int W, int N,
                                         int max_hyp, uint32_t seed, double thr2, int min_inliers, float* motion, float* Hout, int32_t* info, uint8_t* mask) {
    __shared__ uint8_t sm[CAP];                              // inlier flag of every list entry
    __shared__ double sa[72], sh[8], sp[4][44], smc[4 * FT_CHUNK];
    __shared__ int part[4], s_have;
    const int t = threadIdx.x, b = blockIdx.x, m = ft_count(count, b, min(N, CAP));
    const double* mb = mc + (size_t)b * N * 4;
    const double sx = 0.5 * W, sy = 0.5 * H;
    int n1 = 0, n2 = 0, best = -1;
    for (int i = t; i < N; i += FT_THREADS) n1 += kp1[((size_t)b * N + i) * 2] >= 0, n2 += kp2[((size_t)b * N + i) * 2] >= 0;
    n1 = ft_block_sum(n1, part), n2 = ft_block_sum(n2, part);
    // the winner: the highest score, ties to the lowest k
    for (int k = t; k < max_hyp; k += FT_THREADS) {
        const int s = scores[(size_t)b * max_hyp + k];
        if (s >= 0) best = max(best, s * 65536 + (65535 - k));
    }
    best = ft_block_max(best, part);
    const int winner = m >= FT_MIN_MATCHES && best >= 0 ? 65535 - (best & 65535) : -1;
    if (t == 0) {
        double h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const bool ok = winner >= 0 && ft_hypothesis<1>(mb, m, seed, winner, sa, h);
        s_have = ok;
#pragma unroll
        for (int c = 0; c < 8; ++c) sh[c] = h[c];
    }
    __syncthreads();
    const bool have = s_have;
    int inliers = 0;
    for (int round = 0; round <= 2; ++round) {
        if (round && have) {                                 // a refit over the current inliers
            // 36 entries of the upper triangle of A^T A, then the 8 of A^T b.  An entry is (s0 + s1) + (s2 + s3), s_q the sum over the inliers at
            // list positions p = q mod 4 in list order: thread 44 q + e sums s_q of entry e, the matches 1024 at a time in LDS
            const int e = t % 44, q = t / 44;
            int r = 0, c = e;
            if (e >= 36) r = e - 36, c = 8;
            else
                while (c >= 8 - r) c -= 8 - r, ++r;
            if (e < 36) c += r;
            double acc = 0.0;
            for (int c0 = 0; c0 < m; c0 += FT_CHUNK) {
                const int n = min(FT_CHUNK, m - c0);
                __syncthreads();
                for (int i = t; i < 4 * n; i += FT_THREADS) smc[i] = mb[4 * (size_t)c0 + i];
                __syncthreads();
                // The loop below is nearly all of the kernel's time, and its switches diverge in every wave: some 400 instructions with 46 conditional
                // branches, whose cost depends on where they fall in the 64-byte fetch lines.  Measured on the MI355X with the loop's first LDS read at
                // byte 0 / 40 / 12 of a line: 549 / 531 / 529 us for ftms_refit_kernel at 512x512 (README.md, feature_align_ms, Measurements).  So the
                // place is fixed here, 12 as it was before the two kernels shared this body, and no longer moves with the code in front of it.
                // The nine belongs to the blocks the present compiler lays between this point and the loop's header: after a compiler update, or a change
                // to the loop, disassemble the kernel, take the offset of the loop's first ds_read_u8 from the kernel's start modulo 64, and choose the
                // count that makes it 12 again.  (A branch-free loop would not need any of this; that is tuning and a change of its own.)
                asm volatile(".p2align 6\n .rept 9\n s_nop 0\n .endr");
                if (q < 4)
                    for (int p = q; p < n; p += 4) {
                        if (!sm[c0 + p]) continue;
                        const double x = smc[4 * p], y = smc[4 * p + 1], u = smc[4 * p + 2], v = smc[4 * p + 3];
                        acc = acc + ft_row0(r, x, y, u) * ft_row0(c, x, y, u);
                        acc = acc + ft_row1(r, x, y, v) * ft_row1(c, x, y, v);
                    }
            }
            if (q < 4) sp[q][e] = acc;
            __syncthreads();
            if (t < 44) {
                const double total = (sp[0][e] + sp[1][e]) + (sp[2][e] + sp[3][e]);
                sa[r * 9 + c] = total;
                if (c < 8) sa[c * 9 + r] = total;
            }
            __syncthreads();
            if (t == 0) {
                double h[8];
                if (ft_solve8<1>(sa, h))                     // singular: the previous H stays
#pragma unroll
                    for (int c = 0; c < 8; ++c) sh[c] = h[c];
            }
            __syncthreads();
        }
        double h[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) h[c] = sh[c];
        int n = 0;
        for (int p = t; p < m; p += FT_THREADS) {
            const bool in = have && ft_inlier(h, mb[4 * p], mb[4 * p + 1], mb[4 * p + 2], mb[4 * p + 3], sx, sy, thr2);
            sm[p] = in, n += in;
        }
        inliers = ft_block_sum(n, part);                     // (its barriers also order sm and sa between the rounds)
    }
    for (int p = t; p < N; p += FT_THREADS) mask[(size_t)b * N + p] = p < m ? sm[p] : 0;
    if (t == 0) ft_write_model(sh, have, winner, inliers, min_inliers, n1, n2, m, H, W, sx, sy, b, motion, Hout, info);
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

// the operands of the match entries of both paths, N slots per image
static inline bool ft_match_operands_ok(const void* kp1, const void* desc1, const void* kp2, const void* desc2, const void* nn, const void* matches, const void* count, int B,
                                        int64_t N) {
    const int64_t bn = B * N;
    const ft_region r[7] = {{kp1, 8 * bn, false}, {desc1, 32 * bn, false}, {kp2, 8 * bn, false}, {desc2, 32 * bn, false},
                            {nn, 24 * bn, true}, {matches, 8 * bn, true}, {count, 4 * B, true}};
    return ft_regions_ok(r, 7);
}

// those of the ransac entries, xy fp64 [2,B,N,2] where the entry has it; workspace: mc fp64 [B,N,4] then scores int32 [B,max_hyp] = 32 B N +
// 4 B max_hyp bytes
static inline bool ft_ransac_operands_ok(const void* kp1, const void* kp2, const void* matches, const void* count, const void* motion, const void* Hout, const void* info,
                                         const void* mask, const void* xy, bool has_xy, const void* workspace, int64_t workspace_bytes, int B, int64_t N, int max_hyp) {
    const int64_t bn = B * N, need = 32 * bn + 4 * (int64_t)B * max_hyp;
    if (workspace_bytes < need || ((uintptr_t)workspace & 15)) return false;
    const ft_region r[10] = {{kp1, 8 * bn, false}, {kp2, 8 * bn, false}, {matches, 8 * bn, false}, {count, 4 * B, false}, {motion, 32 * B, true},
                             {Hout, 36 * B, true}, {info, 32 * B, true}, {mask, bn, true}, {workspace, need, true}, {xy, 32 * bn, true}};
    return ft_regions_ok(r, has_xy ? 10 : 9);
}

// launchers of features.hip's kernels that take the number of slots N as an argument (defined there): ft_match_kernel + ft_compact_kernel;
// and, behind the path's own norm kernel, ft_hyp_kernel on the normalised match coordinates mc, then the path's refit kernel
typedef void (*ft_refit_fn)(const int32_t* kp1, const int32_t* kp2, const double* mc, const int32_t* count, const int32_t* scores, int H, int W, int N, int max_hyp,
                            uint32_t seed, double thr2, int min_inliers, float* motion, float* Hout, int32_t* info, uint8_t* mask);
int ft_launch_match(const int32_t* kp1, const uint32_t* desc1, const int32_t* kp2, const uint32_t* desc2, int B, int N, int32_t* nn, int32_t* matches, int32_t* count,
                    hipStream_t s);
int ft_launch_hyp_refit(ft_refit_fn refit, const int32_t* kp1, const int32_t* kp2, const double* mc, const int32_t* count, int B, int H, int W, int N, int max_hyp,
                        double thr2, int min_inliers, uint32_t seed, int32_t* scores, float* motion, float* Hout, int32_t* info, uint8_t* mask, hipStream_t s);
