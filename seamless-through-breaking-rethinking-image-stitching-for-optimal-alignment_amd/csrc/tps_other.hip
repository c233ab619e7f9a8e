// tps_method="other" of the TPS post-pipeline (reference: core/inference/tps_methods/other_tps.py, tps_pipline.py:405-421).
// gfx950 only.  Compiled with -ffp-contract=off: every fp64 rounding of the maps is the reference's (numpy, one rounding per op).
//
//   tps_other_solve_kernel  the two per-axis splines [[K, P], [P^T, 0]] theta = [delta; 0], K_ij = r^2 ln(r + 1e-6), fp64
//                           Gauss-Jordan (csrc/tps_solve.h) from the float32 sites, theta rounded to float32
//   tps_other_maps_kernel   tps_grid + tps_grid_to_remap: the reduced-form spline on the float32 linspace grid in fp64,
//                           mapx = float32((x + dx) * W), mapy = float32((y + dy) * H)
//   remap_cubic_u8_kernel   cv2.remap(INTER_CUBIC, BORDER_CONSTANT 0) on uint8 data in OpenCV's fixed point: 5-bit map
//                           fractions, the 32 x 32 x 16 int16 coefficient table, int32 sums, (sum + 2^14) >> 15, saturated
#include "common.h"
#include "../../include/stitch_gfx950.h"
#include "tps_solve.h"

// U(r) = r^2 ln(r + 1e-6) of other_tps.py TPS.u, r in fp64 from float32 points (d() subtracts in the points' precision, here fp64:
// the fp64 system is the documented deviation from the reference's float32 sgesv)
__device__ __forceinline__ double other_u(double r) { return r * r * log(r + 1e-6); }

__global__ __launch_bounds__(256) void tps_other_solve_kernel(const float* __restrict__ sites, const float* __restrict__ delta,
                                                              double* __restrict__ work_g, float* __restrict__ kw,
                                                              float* __restrict__ aw, int n, int use_lds, int* __restrict__ status) {
    tps_gauss_jordan(
        [](float ax, float ay, float bx, float by) {
            const double dx = (double)ax - (double)bx, dy = (double)ay - (double)by;
            return other_u(sqrt(dx * dx + dy * dy));
        },
        sites, sites, delta, work_g, kw, aw, n, use_lds, status);
}

extern "C" int st_tps_other_solve(const float* sites, const float* delta, void* work_f64, float* kernel_w, float* affine_w, int32_t n,
                                  int32_t* status, void* stream) {
    if (!sites || !delta || !work_f64 || !kernel_w || !affine_w || !status || n < 3 || n > 4096) return ST_EINVAL;
    const size_t bytes = (size_t)(n + 3) * (n + 5) * sizeof(double);
    const int use_lds = bytes <= 150 * 1024 && n + 3 <= 144;
    if (use_lds && bytes > 48 * 1024)
        (void)hipFuncSetAttribute((const void*)tps_other_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    hipLaunchKernelGGL(tps_other_solve_kernel, dim3(1), dim3(256), use_lds ? bytes : 0, (hipStream_t)stream, sites, delta,
                       (double*)work_f64, kernel_w, affine_w, n, use_lds, status);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// numpy's float32 add.reduce (pairwise_sum) of a[i * stride], 0 <= i < n, n <= 128: eight running sums over whole blocks of 8,
// combined ((0+1)+(2+3))+((4+5)+(6+7)), then the tail in order; below 8 elements a plain in-order sum from 0.
__device__ float np_sum_leaf_f32(const float* __restrict__ a, int stride, int n) {
    if (n < 8) {
        float r = 0.f;
        for (int i = 0; i < n; ++i) r += a[(size_t)i * stride];
        return r;
    }
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = a[(size_t)j * stride];
    int i = 8;
    for (; i < n - n % 8; i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += a[(size_t)(i + j) * stride];
    }
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[(size_t)i * stride];
    return res;
}

// The whole pairwise_sum: above 128 elements the two halves (n2 = n/2 rounded down to a multiple of 8) are summed separately and
// added.  The recursion runs on an explicit stack in LDS (one thread; depth <= 6 for n <= 4096).
__device__ float np_sum_f32(const float* __restrict__ a, int stride, int n, int* st_s, int* st_n, int* st_ph, float* st_l) {
    if (n <= 128) return np_sum_leaf_f32(a, stride, n);
    int sp = 0;
    st_s[0] = 0; st_n[0] = n; st_ph[0] = 0;
    for (;;) {
        const int s = st_s[sp], m = st_n[sp], m2 = m / 2 - (m / 2) % 8;
        const int cs = st_ph[sp] == 0 ? s : s + m2, cm = st_ph[sp] == 0 ? m2 : m - m2;
        if (cm > 128) { ++sp; st_s[sp] = cs; st_n[sp] = cm; st_ph[sp] = 0; continue; }
        float ret = np_sum_leaf_f32(a + (size_t)cs * stride, stride, cm);
        for (;;) {                                     // a child is done: go to the right sibling or finish the parent
            if (st_ph[sp] == 0) { st_l[sp] = ret; st_ph[sp] = 1; break; }
            ret = st_l[sp] + ret;
            if (sp == 0) return ret;
            --sp;
        }
    }
}

// One thread per output pixel (64 x 4 per block).  Centres and weights are staged in LDS as fp64 in chunks of 256, so any n works;
// the sum over the centres runs in index order (w_0 first).  w_0 is the reduced form's -sum_{i>=1} w_i, in float32 as numpy's
// np.sum computes it (other_tps.py TPS.z): kw[0] is ignored.
#define OTHER_CHUNK 256
__global__ __launch_bounds__(256) void tps_other_maps_kernel(const float* __restrict__ centers, const float* __restrict__ kw,
                                                             const float* __restrict__ aw, int n, int H, int W,
                                                             float* __restrict__ mapx, float* __restrict__ mapy) {
    __shared__ double s_cx[OTHER_CHUNK], s_cy[OTHER_CHUNK], s_wx[OTHER_CHUNK], s_wy[OTHER_CHUNK];
    __shared__ float s_w0[2];
    __shared__ int st_s[8], st_n[8], st_ph[8];
    __shared__ float st_l[8];
    if (threadIdx.x == 0) {
        s_w0[0] = -np_sum_f32(kw + 2, 2, n - 1, st_s, st_n, st_ph, st_l);
        s_w0[1] = -np_sum_f32(kw + 3, 2, n - 1, st_s, st_n, st_ph, st_l);
    }
    const int j = blockIdx.x * 64 + (threadIdx.x & 63), i = blockIdx.y * 4 + (threadIdx.x >> 6);
    // numpy.linspace(0, 1, W, dtype=float32): j * (1 / (W - 1)) in fp64, the last sample exactly 1, rounded to float32
    const double x = (W == 1) ? 0.0 : (j == W - 1) ? 1.0 : (double)(float)((double)j * (1.0 / (double)(W - 1)));
    const double y = (H == 1) ? 0.0 : (i == H - 1) ? 1.0 : (double)(float)((double)i * (1.0 / (double)(H - 1)));
    double sx = 0.0, sy = 0.0;
    for (int base = 0; base < n; base += OTHER_CHUNK) {
        __syncthreads();                               // (also orders s_w0 before its first use)
        const int m = min(OTHER_CHUNK, n - base);
        for (int e = threadIdx.x; e < m; e += 256) {
            const int k = base + e;
            s_cx[e] = (double)centers[2 * k];
            s_cy[e] = (double)centers[2 * k + 1];
            s_wx[e] = (double)(k == 0 ? s_w0[0] : kw[2 * k]);
            s_wy[e] = (double)(k == 0 ? s_w0[1] : kw[2 * k + 1]);
        }
        __syncthreads();
        for (int e = 0; e < m; ++e) {
            const double dx = x - s_cx[e], dy = y - s_cy[e];
            const double u = other_u(sqrt(dx * dx + dy * dy));
            sx = sx + u * s_wx[e];
            sy = sy + u * s_wy[e];
        }
    }
    if (i >= H || j >= W) return;
    const double gx = (((double)aw[0] + (double)aw[2] * x) + (double)aw[4] * y) + sx;
    const double gy = (((double)aw[1] + (double)aw[3] * x) + (double)aw[5] * y) + sy;
    mapx[(size_t)i * W + j] = (float)((x + gx) * (double)W);
    mapy[(size_t)i * W + j] = (float)((y + gy) * (double)H);
}

extern "C" int st_tps_other_maps(const float* centers, const float* kernel_w, const float* affine_w, int32_t n, int32_t h, int32_t w,
                                 float* mapx, float* mapy, void* stream) {
    if (!centers || !kernel_w || !affine_w || !mapx || !mapy || n < 1 || n > 4096 || h < 1 || w < 1 || (int64_t)h * w >= (1LL << 31))
        return ST_EINVAL;
    hipLaunchKernelGGL(tps_other_maps_kernel, dim3((w + 63) / 64, (h + 3) / 4), dim3(256), 0, (hipStream_t)stream, centers, kernel_w,
                       affine_w, n, h, w, mapx, mapy);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// One thread per output pixel, every plane: the quantised coordinates and the coefficient row are shared by the planes.
// X = cvRound(map * 32) (v_rndne: half to even), sx = X >> 5, fx = X & 31; taps (sy-1..sy+2) x (sx-1..sx+2), a tap outside the
// source reads 0 (BORDER_CONSTANT).  A non-finite map value or |map| >= 2^26 (where cvRound leaves int32 and OpenCV's int16 tap
// coordinates saturate far outside any accepted source) gives 0.  Planes are float, quantised on load with st_u8_trunc.
__global__ __launch_bounds__(256) void remap_cubic_u8_kernel(const float* __restrict__ src, int P, int Hs, int Ws,
                                                             const float* __restrict__ mapx, const float* __restrict__ mapy, int H,
                                                             int W, const int16_t* __restrict__ table, float* __restrict__ out) {
    const int j = blockIdx.x * 64 + (threadIdx.x & 63), i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= H || j >= W) return;
    const size_t o = (size_t)i * W + j, ohw = (size_t)H * W, shw = (size_t)Hs * Ws;
    const float mx = mapx[o], my = mapy[o];
    if (!(fabsf(mx) < 67108864.f && fabsf(my) < 67108864.f)) {
        for (int p = 0; p < P; ++p) out[p * ohw + o] = 0.f;
        return;
    }
    const int X = (int)rintf(mx * 32.f), Y = (int)rintf(my * 32.f);
    const int sx = (X >> 5) - 1, sy = (Y >> 5) - 1;
    const int4* row = (const int4*)(table + (size_t)(((Y & 31) << 5) | (X & 31)) * 16);
    const int4 t0 = row[0], t1 = row[1];
    const int words[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
    int c[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        c[2 * k] = (int)(int16_t)(words[k] & 0xffff);
        c[2 * k + 1] = words[k] >> 16;
    }
    bool xin[4], yin[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { xin[k] = sx + k >= 0 && sx + k < Ws; yin[k] = sy + k >= 0 && sy + k < Hs; }
    for (int p = 0; p < P; ++p) {
        const float* im = src + p * shw;
        int acc = 0;
#pragma unroll
        for (int k1 = 0; k1 < 4; ++k1) {
            if (!yin[k1]) continue;
            const float* r = im + (size_t)(sy + k1) * Ws;
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2)
                if (xin[k2]) acc += (int)st_u8_trunc(r[sx + k2]) * c[k1 * 4 + k2];
        }
        out[p * ohw + o] = (float)min(max((acc + 16384) >> 15, 0), 255);
    }
}

extern "C" int st_remap_cubic_u8(const float* src, int32_t planes, int32_t src_h, int32_t src_w, const float* mapx, const float* mapy,
                                 int32_t h, int32_t w, const int16_t* table, float* out, void* stream) {
    if (!src || !mapx || !mapy || !table || !out || planes < 1 || planes > 64 || src_h < 1 || src_w < 1 || src_h > 32760 ||
        src_w > 32760 || h < 1 || w < 1 || (int64_t)h * w >= (1LL << 31) || ((uintptr_t)table & 15))
        return ST_EINVAL;
    hipLaunchKernelGGL(remap_cubic_u8_kernel, dim3((w + 63) / 64, (h + 3) / 4), dim3(256), 0, (hipStream_t)stream, src, planes, src_h,
                       src_w, mapx, mapy, h, w, table, out);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
