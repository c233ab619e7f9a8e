// fp64 Gauss-Jordan of the TPS systems, shared by csrc/tps_pipeline.hip (kornia / pixel-unit splines) and csrc/tps_other.hip
// (tps_method "other"): the same elimination for every kernel function.  Include after common.h.
#pragma once

// f(A_i) = rhs_i for f(v) = a0 + [ax ay].v + sum_j w_j U(v, Bp_j): L = [[K, P], [P^T, 0]], K_ij = U(A_i, Bp_j), P = [1, A],
// right-hand side [rhs; 0].  kornia's get_tps_transform(points_src = A, points_dst = Bp) puts the kernel centres AND the
// values at Bp (rhs = Bp); the classical spline (OpenCV) has its centres at the sites (Bp = A).  fp64 Gauss-Jordan with partial pivoting on
// work [n+3, n+5]; weights out: kernel [n,2], affine [3,2] fp32.  (The reference solves in fp32 through MKL's blocked LU,
// whose operation order is not reproducible; the fp64 solve is the exact solution of the same fp32 system.)
// Body of a one-block (256 threads) kernel; `ufn(ax, ay, bx, by)` is the kernel function U(A_r, Bp_c), any type convertible
// to double.  Static and dynamic LDS as declared below (the caller launches with the dynamic bytes when use_lds).
template <class UFn>
__device__ __forceinline__ void tps_gauss_jordan(UFn ufn, const float* __restrict__ A, const float* __restrict__ Bp,
                                                 const float* __restrict__ rhs, double* __restrict__ work_g, float* __restrict__ kw,
                                                 float* __restrict__ aw, int n, int use_lds, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double tps2_lds[];
    double* __restrict__ work = use_lds ? tps2_lds : work_g;       // n <= 134 ((n+3)(n+5) doubles <= 150 KiB, the callers' test): the
                                                                   // augmented matrix lives in LDS (91 pivot steps of global round
                                                                   // trips cost 1.9 ms; in LDS 0.2 ms); from n = 135 on in work_g
    const int n3 = n + 3, ld = n + 5;
    __shared__ int s_piv;
    __shared__ double s_pmin, s_pmax;             // smallest / largest pivot magnitude: singular-system detection
    __shared__ double s_best[4];
    __shared__ int s_idx[4];
    __shared__ double s_fac_lds[144];             // per-row elimination factors: LDS mode has n + 3 <= 137
    double* __restrict__ s_fac = use_lds ? s_fac_lds : work_g + (size_t)n3 * ld;   // otherwise behind the matrix ((n+3)*(n+6) scratch)
    for (int e = threadIdx.x; e < n3 * ld; e += 256) {
        const int r = e / ld, c = e % ld;
        double v = 0.0;
        if (r < n) {
            if (c < n) v = ufn(A[2 * r], A[2 * r + 1], Bp[2 * c], Bp[2 * c + 1]);
            else if (c == n) v = 1.0;
            else if (c < n3) v = A[2 * r + (c - n - 1)];
            else v = rhs[2 * r + (c - n3)];
        } else if (c < n) {
            const int k = r - n;
            v = (k == 0) ? 1.0 : A[2 * c + (k - 1)];
        }
        work[e] = v;
    }
    if (threadIdx.x == 0) { s_pmin = 1e300; s_pmax = 0.0; }
    __syncthreads();
    for (int c = 0; c < n3; ++c) {
        double best = -1.0;
        int bi = c;
        for (int r = c + threadIdx.x; r < n3; r += 256) {
            const double a = fabs(work[(size_t)r * ld + c]);
            if (a > best) { best = a; bi = r; }
        }
        // arg-max |a|, first row on ties (LAPACK's idamax): wave shuffles, then the 4 wave results
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if ((threadIdx.x & 63) == 0) { s_best[threadIdx.x >> 6] = best; s_idx[threadIdx.x >> 6] = bi; }
        __syncthreads();
        if (threadIdx.x == 0) {
            double bb = s_best[0];
            int ii = s_idx[0];
            for (int t = 1; t < 4; ++t) if (s_best[t] > bb || (s_best[t] == bb && s_idx[t] < ii)) { bb = s_best[t]; ii = s_idx[t]; }
            s_piv = ii;
            if (!(bb >= s_pmin)) s_pmin = bb;        // (a NaN pivot lands here too)
            if (bb > s_pmax) s_pmax = bb;
        }
        __syncthreads();
        const int piv = s_piv;
        if (piv != c)
            for (int k = threadIdx.x; k < ld; k += 256) {
                const double t = work[(size_t)c * ld + k];
                work[(size_t)c * ld + k] = work[(size_t)piv * ld + k];
                work[(size_t)piv * ld + k] = t;
            }
        __syncthreads();
        // elimination of column c from every other row, parallel over all (row, column) elements of the trailing block:
        // factors first (they read column c, which the update does not touch), then one flat pass
        const double pv = work[(size_t)c * ld + c];
        const double inv = 1.0 / (pv != 0.0 ? pv : 1.0);             // a zero pivot is reported through `status`; keep the sweep finite
        for (int r = threadIdx.x; r < n3; r += 256) s_fac[r] = (r == c) ? 0.0 : work[(size_t)r * ld + c] * inv;
        __syncthreads();
        const int wcols = ld - (c + 1);
        for (int e = threadIdx.x; e < n3 * wcols; e += 256) {
            const int r = e / wcols, k = c + 1 + e % wcols;
            const double f = s_fac[r];
            if (f != 0.0) work[(size_t)r * ld + k] -= f * work[(size_t)c * ld + k];
        }
        __syncthreads();
    }
    for (int r = threadIdx.x; r < n3; r += 256) {
        const double d = work[(size_t)r * ld + r];
        const float wx = (float)(work[(size_t)r * ld + n3] / d), wy = (float)(work[(size_t)r * ld + n3 + 1] / d);
        if (r < n) { kw[2 * r] = wx; kw[2 * r + 1] = wy; }
        else { aw[2 * (r - n)] = wx; aw[2 * (r - n) + 1] = wy; }
    }
    // coincident control points (two equal rows) or fewer than three non-collinear ones: a pivot collapses to rounding level
    if (threadIdx.x == 0 && status) status[0] = (s_pmin == s_pmin && s_pmin > 1e-13 * s_pmax) ? 0 : 1;
}
