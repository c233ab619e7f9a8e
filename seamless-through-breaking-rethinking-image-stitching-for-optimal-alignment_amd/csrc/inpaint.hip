// Telea fast-marching inpainting (reference: core/inference/mix_methods/utils/cv_inpainter.py = cv2.inpaint(img, mask, 64,
// cv2.INPAINT_TELEA)) restated in a ring-parallel order (contract: README.md "cv_inpainter", tests/_telea_ref.py):
//   d(p)  4-connected step distance to the known set K0 (mask == 0) = L1 distance, two separable min-plus scans;
//   ring k = {d = k}, filled in increasing k, a ring-k pixel reads only pixels with d < k;
//   T(p)  arrival time, fp32 with IEEE sqrt (sqrtf: __fsqrt_rn is the approximate one here) / division and no contraction (bit-exact against the CPU restatement);
//   I(p)  = sum w (I(q) + grad I(q) . r) / sum w over the disc 0 < |r| <= radius, r = p - q, d(q) < k,
//           w = max(|N . r| / |r|, 1e-6) / |r|^2 / (1 + |T(p) - T(q)|), stored rounded half up to uint8.
// Device state is one packed word per pixel, R | G << 8 | B << 16 | (d mod 256) << 24: the fill reads colour and "known before
// ring k" in one 4-byte load.  Every pixel the fill of ring k inspects lies within L1 distance sqrt(2) radius + 1 of the target,
// and d is 1-Lipschitz in L1, so |d(q) - k| <= 127 for radius <= ST_INPAINT_MAX_RADIUS and the signed 8-bit difference of the tag
// and k is d(q) - k exactly.  A ring-k word may be rewritten by another wave while it is read: its tag still says d = k, so it is
// never used, and which colour a reader sees does not matter.
#include "common.h"

#define ST_INPAINT_MAX_RADIUS 88
#define ST_INPAINT_FAR 0x3fffffff

namespace {

struct Work {                     // carve-up of the caller's workspace (st_inpaint_telea_workspace)
    int* d;
    float* T;
    uint32_t* pk;
    int* list;
    int* offsets;                 // [nb + 1]
    int* cursor;                  // [nb]
    int4* disc;                   // [(2 radius + 1)^2]: (dx, dy, bits(1 / |r|), bits(1 / |r|^2)), row-major, (0, 0) excluded
};

__host__ __device__ inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

__host__ __device__ inline size_t work_bytes(int H, int W, int radius) {
    const size_t n = (size_t)H * W, nb = (size_t)H + W + 1, nd = (size_t)(2 * radius + 1) * (2 * radius + 1);
    return 4 * align256(n * 4) + align256((nb + 1) * 4) + align256(nb * 4) + align256(nd * 16);
}

inline Work carve(void* base, int H, int W, int radius) {
    const size_t n = (size_t)H * W, nb = (size_t)H + W + 1;
    char* p = (char*)base;
    Work w;
    w.d = (int*)p;        p += align256(n * 4);
    w.T = (float*)p;      p += align256(n * 4);
    w.pk = (uint32_t*)p;  p += align256(n * 4);
    w.list = (int*)p;     p += align256(n * 4);
    w.offsets = (int*)p;  p += align256((nb + 1) * 4);
    w.cursor = (int*)p;   p += align256(nb * 4);
    w.disc = (int4*)p;
    (void)radius;
    return w;
}

// ---- mask / image preparation (cv_inpainter.inpaint_cv: to_pillow_fn + .convert('L')) -----------------------------------------
// max of the mask planes as an order-preserving int (negative floats: bits flipped), for the `max <= 1.1` branch
__device__ __forceinline__ int float_order(float v) {
    const int b = __float_as_int(v);
    return b >= 0 ? b : b ^ 0x7fffffff;
}

__global__ __launch_bounds__(256) void mask_max_kernel(const float* __restrict__ mask, int64_t n, int* __restrict__ out) {
    int best = float_order(-INFINITY);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) best = max(best, float_order(mask[i]));
    for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o));
    if ((threadIdx.x & 63) == 0) atomicMax(out, best);
}

// accumulators are set by kernels, not hipMemset / hipMemcpy (the entry points may be captured into a hipGraph)
__global__ __launch_bounds__(256) void fill_i32_kernel(int* __restrict__ p, int n, int v) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

// to(torch.uint8) of a value in [0, 255] truncates; values outside are clamped first (the reference's cast is undefined there)
__device__ __forceinline__ uint32_t trunc_u8(float v) { return (uint32_t)fminf(fmaxf(v, 0.f), 255.f); }

__global__ __launch_bounds__(256) void prep_kernel(const float* __restrict__ img, const float* __restrict__ mask, int mask_planes,
                                                   const int* __restrict__ mask_max, uint8_t* __restrict__ img_hwc,
                                                   uint8_t* __restrict__ mask_u8, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool scale = *mask_max <= float_order(1.1f);
    uint32_t m[3];
    for (int c = 0; c < 3; ++c) {
        float v = mask[(size_t)(mask_planes == 1 ? 0 : c) * n + i];
        if (scale) v = fminf(fmaxf(v * 255.f, 0.f), 255.f);
        m[c] = trunc_u8(v);
        img_hwc[(size_t)3 * i + c] = (uint8_t)trunc_u8(img[(size_t)c * n + i]);
    }
    // PIL's RGB -> L: (R 19595 + G 38470 + B 7471 + 0x8000) >> 16
    mask_u8[i] = (uint8_t)((m[0] * 19595u + m[1] * 38470u + m[2] * 7471u + 0x8000u) >> 16);
}

// ---- rings: d by two min-plus scans, histogram, prefix sum, bucketing ------------------------------------------------------
__global__ __launch_bounds__(256) void dt_rows_kernel(const uint8_t* __restrict__ mask, int* __restrict__ g, int H, int W) {
    const int y = blockIdx.x * 256 + threadIdx.x;
    if (y >= H) return;
    const uint8_t* m = mask + (size_t)y * W;
    int* o = g + (size_t)y * W;
    int run = ST_INPAINT_FAR;
    for (int x = 0; x < W; ++x) {
        run = m[x] == 0 ? 0 : min(run + 1, ST_INPAINT_FAR);
        o[x] = run;
    }
    for (int x = W - 2; x >= 0; --x) {                        // the carry stays in a register: no store -> load chain
        run = min(o[x], min(run + 1, ST_INPAINT_FAR));
        o[x] = run;
    }
}

__global__ __launch_bounds__(256) void dt_cols_kernel(int* __restrict__ d, int H, int W) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    int run = d[x];
    for (int y = 1; y < H; ++y) {
        run = min(d[(size_t)y * W + x], run + 1);
        d[(size_t)y * W + x] = run;
    }
    for (int y = H - 2; y >= 0; --y) {
        run = min(d[(size_t)y * W + x], run + 1);
        d[(size_t)y * W + x] = run;
    }
}

// counts[k] += #{d = k}; bins below 1024 are counted in LDS first (one global atomic per block and bin), the rest directly.
// d = FAR (no known pixel at all) is not counted: counts[0] == 0 tells the caller.
__global__ __launch_bounds__(256) void ring_hist_kernel(const int* __restrict__ d, int n, int nb, int* __restrict__ counts) {
    __shared__ int h[1024];
    for (int i = threadIdx.x; i < 1024; i += 256) h[i] = 0;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const int k = d[i];
        if (k < nb) {
            if (k < 1024) atomicAdd(&h[k], 1);
            else atomicAdd(&counts[k], 1);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < min(nb, 1024); b += 256)
        if (h[b]) atomicAdd(&counts[b], h[b]);
}

// exclusive prefix sum of counts[1..nb) into offsets (offsets[k] = first list slot of ring k; ring 0 is not listed); one block
__global__ __launch_bounds__(1024) void ring_scan_kernel(const int* __restrict__ counts, int nb, int* __restrict__ offsets,
                                                         int* __restrict__ cursor) {
    __shared__ int part[1024];
    const int per = (nb + 1023) / 1024, b0 = threadIdx.x * per;
    int s = 0;
    for (int k = b0; k < min(b0 + per, nb); ++k) s += k > 0 ? counts[k] : 0;
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = threadIdx.x ? part[threadIdx.x - 1] : 0;
    for (int k = b0; k < min(b0 + per, nb); ++k) {
        offsets[k] = run;
        cursor[k] = run;
        run += k > 0 ? counts[k] : 0;
    }
    if (threadIdx.x == 1023) offsets[nb] = part[1023];
}

// list[offsets[k] ..) = the pixels of ring k (order inside a ring is free: its pixels do not read each other); slots are
// reserved per block and bin in LDS as in ring_hist_kernel.  Also writes the packed words and T = 0 (T of d > 0 is set by the fill).
__global__ __launch_bounds__(256) void ring_scatter_kernel(const int* __restrict__ d, const uint8_t* __restrict__ img_hwc, int n, int nb,
                                                           int* __restrict__ cursor, int* __restrict__ list, uint32_t* __restrict__ pk,
                                                           float* __restrict__ T) {
    __shared__ int h[1024];
    for (int i = threadIdx.x; i < 1024; i += 256) h[i] = 0;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    int k = 0, local = -1;
    if (i < n) {
        k = d[i];
        pk[i] = (uint32_t)img_hwc[(size_t)3 * i] | ((uint32_t)img_hwc[(size_t)3 * i + 1] << 8) | ((uint32_t)img_hwc[(size_t)3 * i + 2] << 16) |
                ((uint32_t)(k & 0xff) << 24);
        T[i] = 0.f;
        if (k > 0 && k < 1024 && k < nb) local = atomicAdd(&h[k], 1);
        else if (k >= 1024 && k < nb) list[atomicAdd(&cursor[k], 1)] = i;
    }
    __syncthreads();
    for (int b = threadIdx.x; b < min(nb, 1024); b += 256)
        if (h[b]) h[b] = atomicAdd(&cursor[b], h[b]);
    __syncthreads();
    if (local >= 0) list[h[k] + local] = i;
}

// ---- fill -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void disc_kernel(int4* __restrict__ disc, int radius) {
    const int dy = (int)blockIdx.x * 256 + (int)threadIdx.x - radius;
    if (dy > radius) return;
    int start = 0;                                            // entries of the rows above: 2 floor(sqrt(R^2 - y^2)) + 1 each, minus (0, 0)
    for (int y = -radius; y < dy; ++y) {
        const int r2 = radius * radius - y * y;
        int h = (int)sqrtf((float)r2);                        // integer square root, corrected to be exact
        while (h * h > r2) --h;
        while ((h + 1) * (h + 1) <= r2) ++h;
        start += 2 * h + 1 - (y == 0);
    }
    for (int dx = -radius; dx <= radius; ++dx) {
        const int r2 = dx * dx + dy * dy;
        if (r2 == 0 || r2 > radius * radius) continue;
        const double r = sqrt((double)r2);
        disc[start++] = make_int4(dx, dy, __float_as_int((float)(1.0 / r)), __float_as_int((float)(1.0 / (double)r2)));
    }
}

__device__ __forceinline__ bool before(uint32_t word, int k) { return (int8_t)(uint8_t)((word >> 24) - (uint32_t)k) < 0; }

// gradient along one axis: central if both neighbours are known, one-sided against the centre, else 0 (per colour channel)
__device__ __forceinline__ void grad3(uint32_t c, uint32_t lo, bool has_lo, uint32_t hi, bool has_hi, float g[3]) {
    for (int ch = 0; ch < 3; ++ch) {
        const float vc = (float)((c >> (8 * ch)) & 0xff), vl = (float)((lo >> (8 * ch)) & 0xff), vh = (float)((hi >> (8 * ch)) & 0xff);
        g[ch] = has_lo && has_hi ? (vh - vl) * 0.5f : has_hi ? vh - vc : has_lo ? vc - vl : 0.f;
    }
}

// One wave per target pixel of ring k: T(p) and N(p) from its 4 neighbours (every lane, same loads), then the lanes stride over
// the disc table; weights in fp32, sums in fp64, one wave reduction.  64-thread workgroups: a ring of a few hundred pixels is
// still spread over as many CUs.
__global__ __launch_bounds__(64) void telea_ring_kernel(uint32_t* __restrict__ pk, float* __restrict__ T, const int* __restrict__ list,
                                                        const int4* __restrict__ disc, int ndisc, int H, int W, int k) {
    const int p = list[blockIdx.x];
    const int px = p % W, py = p / W, lane = threadIdx.x;
    const uint32_t wl = px > 0 ? pk[p - 1] : 0u, wr = px < W - 1 ? pk[p + 1] : 0u;
    const uint32_t wu = py > 0 ? pk[p - W] : 0u, wd = py < H - 1 ? pk[p + W] : 0u;
    const bool hl = px > 0 && before(wl, k), hr = px < W - 1 && before(wr, k);
    const bool hu = py > 0 && before(wu, k), hd = py < H - 1 && before(wd, k);
    const float tl = hl ? T[p - 1] : INFINITY, tr = hr ? T[p + 1] : INFINITY, tu = hu ? T[p - W] : INFINITY, td = hd ? T[p + W] : INFINITY;
    const float a = fminf(tl, tr), b = fminf(tu, td);
    float tp;
    if (a == INFINITY || b == INFINITY || fabsf(a - b) >= 1.f) {
        tp = fminf(a, b) + 1.f;
    } else {
        const float dd = a - b;
        tp = ((a + b) + sqrtf(2.f - dd * dd)) * 0.5f;
    }
    float nx = hl && hr ? (tr - tl) * 0.5f : hr ? tr - tp : hl ? tp - tl : 0.f;
    float ny = hu && hd ? (td - tu) * 0.5f : hd ? td - tp : hu ? tp - tu : 0.f;
    const float nn = nx * nx + ny * ny;
    if (nn > 0.f) {
        const float inv = 1.f / sqrtf(nn);
        nx *= inv;
        ny *= inv;
    }
    double sw = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll 2
    for (int i = lane; i < ndisc; i += 64) {
        const int4 e = disc[i];
        const int qx = px - e.x, qy = py - e.y;                 // r = p - q = (e.x, e.y)
        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        const int q = qy * W + qx;
        const uint32_t wq = pk[q];
        if (!before(wq, k)) continue;
        const uint32_t ql = qx > 0 ? pk[q - 1] : 0u, qr = qx < W - 1 ? pk[q + 1] : 0u;
        const uint32_t qu = qy > 0 ? pk[q - W] : 0u, qd = qy < H - 1 ? pk[q + W] : 0u;
        const float tq = T[q];
        float gx[3], gy[3];
        grad3(wq, ql, qx > 0 && before(ql, k), qr, qx < W - 1 && before(qr, k), gx);
        grad3(wq, qu, qy > 0 && before(qu, k), qd, qy < H - 1 && before(qd, k), gy);
        const float rx = (float)e.x, ry = (float)e.y;
        const float dir = fmaxf(fabsf(nx * rx + ny * ry) * __int_as_float(e.z), 1e-6f);
        const float w = dir * __int_as_float(e.w) / (1.f + fabsf(tp - tq));
        const double wd64 = (double)w;
        sw += wd64;
        s0 += wd64 * (double)((float)(wq & 0xff) + (gx[0] * rx + gy[0] * ry));
        s1 += wd64 * (double)((float)((wq >> 8) & 0xff) + (gx[1] * rx + gy[1] * ry));
        s2 += wd64 * (double)((float)((wq >> 16) & 0xff) + (gx[2] * rx + gy[2] * ry));
    }
    for (int o = 32; o > 0; o >>= 1) {
        sw += __shfl_xor(sw, o);
        s0 += __shfl_xor(s0, o);
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
    }
    if (lane == 0) {
        const double inv = 1.0 / sw;
        uint32_t v = (uint32_t)(k & 0xff) << 24;
        const double s[3] = {s0, s1, s2};
        for (int ch = 0; ch < 3; ++ch) v |= (uint32_t)fmin(fmax(floor(s[ch] * inv + 0.5), 0.0), 255.0) << (8 * ch);
        pk[p] = v;
        T[p] = tp;
    }
}

__global__ __launch_bounds__(256) void unpack_kernel(const uint32_t* __restrict__ pk, const int* __restrict__ d, const float* __restrict__ T,
                                                     uint8_t* __restrict__ out_hwc, int* __restrict__ d_out, float* __restrict__ T_out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t w = pk[i];
    out_hwc[(size_t)3 * i] = (uint8_t)w;
    out_hwc[(size_t)3 * i + 1] = (uint8_t)(w >> 8);
    out_hwc[(size_t)3 * i + 2] = (uint8_t)(w >> 16);
    if (d_out) d_out[i] = d[i];
    if (T_out) T_out[i] = T[i];
}

inline bool bad_dims(int32_t H, int32_t W) { return H <= 0 || W <= 0 || (int64_t)H * W > (1 << 28); }

}  // namespace

extern "C" int st_inpaint_telea_workspace(int32_t H, int32_t W, int32_t radius, int64_t* bytes) {
    if (!bytes || bad_dims(H, W) || radius < 1 || radius > ST_INPAINT_MAX_RADIUS) return ST_EINVAL;
    *bytes = (int64_t)work_bytes(H, W, radius);
    return ST_OK;
}

extern "C" int st_inpaint_prep(const float* img3, const float* mask, int32_t mask_planes, uint8_t* img_hwc, uint8_t* mask_u8,
                               int32_t* scratch, int32_t H, int32_t W, void* stream) {
    if (!img3 || !mask || !img_hwc || !mask_u8 || !scratch || (mask_planes != 1 && mask_planes != 3) || bad_dims(H, W)) return ST_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int n = H * W;
    hipLaunchKernelGGL(fill_i32_kernel, dim3(1), dim3(256), 0, s, scratch, 1, (int)0x807fffff);     // float_order(-inf)
    ST_CHECK_LAUNCH();
    const int64_t nm = (int64_t)mask_planes * n;
    hipLaunchKernelGGL(mask_max_kernel, dim3((unsigned)((nm + 255) / 256 < 1024 ? (nm + 255) / 256 : 1024)), dim3(256), 0, s, mask, nm, scratch);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(prep_kernel, dim3((n + 255) / 256), dim3(256), 0, s, img3, mask, mask_planes, scratch, img_hwc, mask_u8, n);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

extern "C" int st_inpaint_telea_rings(const uint8_t* img_hwc, const uint8_t* mask_u8, int32_t H, int32_t W, int32_t radius, void* work,
                                      int64_t work_bytes_, int32_t* ring_counts, void* stream) {
    if (!img_hwc || !mask_u8 || !work || !ring_counts || bad_dims(H, W) || radius < 1 || radius > ST_INPAINT_MAX_RADIUS ||
        work_bytes_ < (int64_t)work_bytes(H, W, radius))
        return ST_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int n = H * W, nb = H + W + 1;
    Work w = carve(work, H, W, radius);
    hipLaunchKernelGGL(fill_i32_kernel, dim3((nb + 255) / 256), dim3(256), 0, s, ring_counts, nb, 0);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(dt_rows_kernel, dim3((H + 255) / 256), dim3(256), 0, s, mask_u8, w.d, H, W);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(dt_cols_kernel, dim3((W + 255) / 256), dim3(256), 0, s, w.d, H, W);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(ring_hist_kernel, dim3((n + 255) / 256), dim3(256), 0, s, w.d, n, nb, ring_counts);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(ring_scan_kernel, dim3(1), dim3(1024), 0, s, ring_counts, nb, w.offsets, w.cursor);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(ring_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, s, w.d, img_hwc, n, nb, w.cursor, w.list, w.pk, w.T);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(disc_kernel, dim3((2 * radius + 1 + 255) / 256), dim3(256), 0, s, w.disc, radius);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

extern "C" int st_inpaint_telea_fill(const int32_t* ring_counts_host, int32_t nrings, int32_t H, int32_t W, int32_t radius, void* work,
                                     int64_t work_bytes_, uint8_t* out_hwc, int32_t* d_out, float* T_out, void* stream) {
    if (!work || !out_hwc || bad_dims(H, W) || radius < 1 || radius > ST_INPAINT_MAX_RADIUS || nrings < 0 || nrings > H + W ||
        (nrings > 0 && !ring_counts_host) || work_bytes_ < (int64_t)work_bytes(H, W, radius))
        return ST_EINVAL;
    int64_t total = 0;
    for (int k = 1; k <= nrings; ++k) {
        if (ring_counts_host[k] <= 0) return ST_EINVAL;          // rings are contiguous: d = k > 0 has a neighbour at k - 1
        total += ring_counts_host[k];
    }
    if (total > (int64_t)H * W) return ST_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    Work w = carve(work, H, W, radius);
    int ndisc = 0;
    for (int dy = -radius; dy <= radius; ++dy)
        for (int dx = -radius; dx <= radius; ++dx) ndisc += dx * dx + dy * dy <= radius * radius;
    ndisc -= 1;
    int off = 0;
    for (int k = 1; k <= nrings; ++k) {
        hipLaunchKernelGGL(telea_ring_kernel, dim3(ring_counts_host[k]), dim3(64), 0, s, w.pk, w.T, w.list + off, w.disc, ndisc, H, W, k);
        ST_CHECK_LAUNCH();
        off += ring_counts_host[k];
    }
    const int n = H * W;
    hipLaunchKernelGGL(unpack_kernel, dim3((n + 255) / 256), dim3(256), 0, s, w.pk, w.d, w.T, out_hwc, d_out, T_out, n);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
