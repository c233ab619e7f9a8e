// feature_align: a weight-free alignment front end -- Harris corners, upright BRIEF-256, mutual nearest-neighbour matching, RANSAC
// homography.  Contract in README.md, "feature_align"; CPU restatement tests/_features_ref.py.  gfx950 only.  Corners, descriptors and
// matching are integers; the RANSAC is fp64 (this file is compiled with -ffp-contract=off: every product and sum below rounds on its own).
// Every kernel of a call goes to the caller's stream, in order, inside the caller's buffers: no host synchronisation, no allocation, no
// memset / memcpy, no atomics (every word has exactly one writer), and the launch count and every grid depend on B, H, W and max_hyp
// alone, so a call captures into a hipGraph as a linear chain.  What depends on the data -- the number of keypoints, of matches, whether a
// hypothesis is void -- is read on the device by the kernels it concerns.
//
//   ft_detect_kernel    one workgroup per 32x32 cell: the luma tile (halo 5) from RGB into LDS, then ft_corners: Sobel (halo 4) -> Harris response
//                       (halo 1), the 3x3 non-maximum suppression, the cell's best 4 corners, and the 5x5 box sum of the luma for the descriptor
//   ft_describe_kernel  one thread per descriptor word: 32 comparisons of box sums
//   ft_match_kernel     both directions: 1024 candidate descriptors at a time in LDS, one wave per query, (distance, slot) reduced over the wave
//   ft_compact_kernel   ratio test, mutual check, the match list in slot order (one workgroup per item: scan)
//   ft_norm_kernel      normalised fp64 coordinates of the matches
//   ft_hyp_kernel       one thread per hypothesis: draw, 8x8 solve in LDS, score against the match list (1024 matches at a time in LDS)
//   ft_refit_kernel     one workgroup per item: ft_refit with the inlier flags of 4096 list entries in LDS
// The bodies ft_corners and ft_refit are in features_common.h, with everything else that features_ms.hip shares: its detect and refit kernels are
// shells around the same two bodies.
#include "features_common.h"

static constexpr ft_pattern_t ft_pattern_host = ft_make_pattern();
__constant__ ft_pattern_t ft_pattern = ft_make_pattern();

__global__ void __launch_bounds__(FT_THREADS) ft_detect_kernel(const float* __restrict__ img1, const float* __restrict__ img2, int B, int H, int W,
                                                                int32_t* __restrict__ kp, uint16_t* __restrict__ box) {
    __shared__ uint8_t sy[42][44];
    const int t = threadIdx.x, z = blockIdx.z, N = FT_PER_CELL * gridDim.x * gridDim.y, cell = blockIdx.y * gridDim.x + blockIdx.x;
    const int x0 = blockIdx.x * FT_CELL, y0 = blockIdx.y * FT_CELL;
    const size_t hw = (size_t)H * W;
    const float* img = (z < B ? img1 + (size_t)z * 3 * hw : img2 + (size_t)(z - B) * 3 * hw);
    for (int e = t; e < 42 * 42; e += FT_THREADS) {
        const int ty = e / 42, tx = e - ty * 42;
        const int y = min(max(y0 - 5 + ty, 0), H - 1), x = min(max(x0 - 5 + tx, 0), W - 1);
        const size_t g = (size_t)y * W + x;
        const int r = ft_pixel(img[g]), gg = ft_pixel(img[hw + g]), b = ft_pixel(img[2 * hw + g]);
        sy[ty][tx] = (uint8_t)((19595 * r + 38470 * gg + 7471 * b + 0x8000) >> 16);
    }
    __syncthreads();
    int win[FT_PER_CELL];                                    // (only ftms_detect_kernel goes on with the winners)
    ft_corners<5, FT_BORDER>(sy, x0, y0, H, W, kp + ((size_t)z * N + FT_PER_CELL * cell) * 2, box + (size_t)z * hw, win);
}

// n2 = number of (item, image) planes; box uint16 [n2, H, W], kp int32 [n2, N, 2] (x, y), desc uint32 [n2, N, 8]
__global__ void __launch_bounds__(FT_THREADS) ft_describe_kernel(const uint16_t* __restrict__ box, const int32_t* __restrict__ kp, int H, int W, int N,
                                                                  uint32_t* __restrict__ desc) {
    const int g = blockIdx.x * FT_THREADS + threadIdx.x, z = blockIdx.y;
    if (g >= N * FT_WORDS) return;
    const int slot = g >> 3, word = g & 7;
    const int x = kp[((size_t)z * N + slot) * 2], y = kp[((size_t)z * N + slot) * 2 + 1];
    uint32_t bits = 0;
    if (x >= FT_BORDER && x < W - FT_BORDER && y >= FT_BORDER && y < H - FT_BORDER) {          // (a valid slot always is; anything else reads nothing)
        const uint16_t* s = box + (size_t)z * H * W;
        for (int b = 0; b < 32; ++b) {
            const int8_t* o = ft_pattern.v + 4 * (word * 32 + b);
            const uint32_t sa = s[(y + o[1]) * W + x + o[0]], sb = s[(y + o[3]) * W + x + o[2]];
            bits |= (uint32_t)(sa < sb) << b;
        }
    }
    desc[((size_t)z * N + slot) * FT_WORDS + word] = bits;
}

// nn int32 [2, B, N, 3]: direction 0 = every slot of image 1 against image 2, direction 1 the reverse; (best slot or -1, d1, d2), 257 = none
__global__ void __launch_bounds__(FT_THREADS) ft_match_kernel(const int32_t* __restrict__ kp1, const uint32_t* __restrict__ desc1, const int32_t* __restrict__ kp2,
                                                               const uint32_t* __restrict__ desc2, int B, int N, int32_t* __restrict__ nn) {
    __shared__ uint32_t cd[FT_WORDS][FT_CHUNK];
    __shared__ uint8_t cv[FT_CHUNK];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, dir = blockIdx.y, b = blockIdx.z;
    const int32_t* kq = (dir ? kp2 : kp1) + (size_t)b * N * 2;
    const int32_t* kc = (dir ? kp1 : kp2) + (size_t)b * N * 2;
    const uint32_t* dq = (dir ? desc2 : desc1) + (size_t)b * N * FT_WORDS;
    const uint32_t* dc = (dir ? desc1 : desc2) + (size_t)b * N * FT_WORDS;
    const int q0 = blockIdx.x * 32 + wave * 8;
    uint32_t key[8], sec[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) key[u] = 0xFFFFFFFFu, sec[u] = FT_NO_DIST;
    for (int c0 = 0; c0 < N; c0 += FT_CHUNK) {
        __syncthreads();
        for (int e = t; e < FT_CHUNK; e += FT_THREADS) {
            const int j = c0 + e;
            const bool ok = j < N && kc[2 * j] >= 0;
            cv[e] = ok;
#pragma unroll
            for (int w = 0; w < FT_WORDS; ++w) cd[w][e] = ok ? dc[(size_t)j * FT_WORDS + w] : 0u;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int qi = q0 + u;
            if (qi >= N || kq[2 * qi] < 0) continue;             // wave-uniform
            uint32_t q[FT_WORDS];
#pragma unroll
            for (int w = 0; w < FT_WORDS; ++w) q[w] = dq[(size_t)qi * FT_WORDS + w];
            for (int e = lane; e < FT_CHUNK; e += 64) {
                if (!cv[e]) continue;
                uint32_t d = 0;
#pragma unroll
                for (int w = 0; w < FT_WORDS; ++w) d += __popc(q[w] ^ cd[w][e]);
                const uint32_t k2 = d << 16 | (uint32_t)(c0 + e);
                if (k2 < key[u]) sec[u] = min(sec[u], key[u] >> 16), key[u] = k2;
                else sec[u] = min(sec[u], d);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int qi = q0 + u;
        if (qi >= N) continue;
        uint32_t k = key[u], s = sec[u];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t ok = (uint32_t)__shfl_xor((int)k, o, 64), os = (uint32_t)__shfl_xor((int)s, o, 64);
            s = min(min(s, os), max(k, ok) >> 16);              // the loser's best is a runner-up (65535 when it has none)
            k = min(k, ok);
        }
        if (lane == 0) {
            int32_t* o = nn + (((size_t)dir * B + b) * N + qi) * 3;
            const bool none = k == 0xFFFFFFFFu;
            o[0] = none ? -1 : (int32_t)(k & 0xFFFF), o[1] = none ? FT_NO_DIST : (int32_t)(k >> 16), o[2] = (int32_t)s;
        }
    }
}

// matches int32 [B, N, 2]: (slot of image 1, slot of image 2) in slot order of image 1, (-1, -1) behind the last; count int32 [B]
__global__ void __launch_bounds__(1024) ft_compact_kernel(const int32_t* __restrict__ nn, int B, int N, int32_t* __restrict__ matches, int32_t* __restrict__ count) {
    __shared__ int ws[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, b = blockIdx.x;
    const int per = (N + 1023) / 1024, i0 = min(t * per, N), i1 = min(i0 + per, N);
    const int32_t* f = nn + (size_t)b * N * 3;
    const int32_t* r = nn + ((size_t)B + b) * N * 3;
    uint32_t flags = 0;
    int c = 0;
    for (int i = i0; i < i1; ++i) {
        const int j = f[3 * i], d1 = f[3 * i + 1], d2 = f[3 * i + 2];
        if (j >= 0 && j < N && d1 < FT_MAX_DIST && FT_RATIO_DEN * d1 < FT_RATIO_NUM * d2 && r[3 * j] == i) flags |= 1u << (i - i0), ++c;
    }
    int inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    int at = inc - c, m = 0;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        if (v < wave) at += ws[v];
        m += ws[v];
    }
    int32_t* o = matches + (size_t)b * N * 2;
    for (int i = i0; i < i1; ++i)
        if (flags >> (i - i0) & 1) o[2 * at] = i, o[2 * at + 1] = f[3 * i], ++at;
    for (int p = m + t; p < N; p += 1024) o[2 * p] = -1, o[2 * p + 1] = -1;
    if (t == 0) count[b] = m;
}

// mc fp64 [B, N, 4]: (x1, y1, x2, y2) of list entry p, normalised as (x - W/2) / (W/2), (y - H/2) / (H/2)
__global__ void __launch_bounds__(FT_THREADS) ft_norm_kernel(const int32_t* __restrict__ kp1, const int32_t* __restrict__ kp2, const int32_t* __restrict__ matches,
                                                              const int32_t* __restrict__ count, int H, int W, int N, double* __restrict__ mc) {
    const int p = blockIdx.x * FT_THREADS + threadIdx.x, b = blockIdx.y;
    if (p >= ft_count(count, b, N)) return;
    const int i = min(max(matches[((size_t)b * N + p) * 2], 0), N - 1), j = min(max(matches[((size_t)b * N + p) * 2 + 1], 0), N - 1);
    const double sx = 0.5 * W, sy = 0.5 * H;
    double* o = mc + ((size_t)b * N + p) * 4;
    o[0] = ((double)kp1[((size_t)b * N + i) * 2] - sx) / sx;
    o[1] = ((double)kp1[((size_t)b * N + i) * 2 + 1] - sy) / sy;
    o[2] = ((double)kp2[((size_t)b * N + j) * 2] - sx) / sx;
    o[3] = ((double)kp2[((size_t)b * N + j) * 2 + 1] - sy) / sy;
}

// scores int32 [B, max_hyp]: inliers of hypothesis k, -1 when it is void (all of them with fewer than 8 matches)
__global__ void __launch_bounds__(64) ft_hyp_kernel(const double* __restrict__ mc, const int32_t* __restrict__ count, int H, int W, int N, int max_hyp, uint32_t seed,
                                                     double thr2, int32_t* __restrict__ scores) {
    __shared__ double sa[72 * 64];                           // the 8 x 9 systems, one column per thread; then 1024 matches at a time
    const int t = threadIdx.x, b = blockIdx.y, k = blockIdx.x * 64 + t, m = ft_count(count, b, N);
    const double* mb = mc + (size_t)b * N * 4;
    double h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool ok = false;
    if (k < max_hyp && m >= FT_MIN_MATCHES) ok = ft_hypothesis<64>(mb, m, seed, k, sa + t, h);
    const double sx = 0.5 * W, sy = 0.5 * H;
    int score = 0;
    for (int c0 = 0; c0 < m; c0 += FT_CHUNK) {
        const int n = min(FT_CHUNK, m - c0);
        __syncthreads();
        for (int e = t; e < 4 * n; e += 64) sa[e] = mb[4 * (size_t)c0 + e];
        __syncthreads();
        if (ok)
            for (int e = 0; e < n; ++e) score += ft_inlier(h, sa[4 * e], sa[4 * e + 1], sa[4 * e + 2], sa[4 * e + 3], sx, sy, thr2);
    }
    if (k < max_hyp) scores[(size_t)b * max_hyp + k] = ok ? score : -1;
}

__global__ void __launch_bounds__(FT_THREADS) ft_refit_kernel(const int32_t* __restrict__ kp1, const int32_t* __restrict__ kp2, const double* __restrict__ mc,
                                                               const int32_t* __restrict__ count, const int32_t* __restrict__ scores, int H, int W, int N, int max_hyp,
                                                               uint32_t seed, double thr2, int min_inliers, float* __restrict__ motion, float* __restrict__ Hout,
                                                               int32_t* __restrict__ info, uint8_t* __restrict__ mask) {
    ft_refit<4 * FT_CHUNK>(kp1, kp2, mc, count, scores, H, W, N, max_hyp, seed, thr2, min_inliers, motion, Hout, info, mask);      // (N <= 4096 by ft_shape_ok)
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// workspace of st_feature_homography, every region rounded up to 16 bytes: box uint16 [2,B,H,W]; kp int32 [2,B,N,2]; desc uint32 [2,B,N,8];
// nn int32 [2,B,N,3]; matches int32 [B,N,2]; count int32 [B]; mc fp64 [B,N,4]; scores int32 [B,max_hyp]; mask uint8 [B,N]
struct ft_layout {
    int N;
    int64_t box, kp, desc, nn, matches, count, mc, scores, mask, total;
};
static bool ft_plan(int B, int H, int W, int max_hyp, ft_layout& L) {
    if (!ft_shape_ok(B, H, W) || max_hyp < 1 || max_hyp > FT_MAX_HYP) return false;
    int64_t at = 0;
    auto take = [&](int64_t bytes) { const int64_t o = at; at += (bytes + 15) & ~(int64_t)15; return o; };
    const int64_t N = L.N = ft_slots(H, W), b = B;
    L.box = take(2 * 2 * b * H * W), L.kp = take(4 * 2 * b * N * 2), L.desc = take(4 * 2 * b * N * 8), L.nn = take(4 * 2 * b * N * 3);
    L.matches = take(4 * b * N * 2), L.count = take(4 * b), L.mc = take(8 * b * N * 4), L.scores = take(4 * b * max_hyp), L.mask = take(b * N);
    L.total = at;
    return true;
}

static int ft_launch_detect(const float* img1, const float* img2, int B, int nimg, int H, int W, int32_t* kp, uint16_t* box, hipStream_t s) {
    ft_detect_kernel<<<dim3(ft_cells(W), ft_cells(H), nimg * B), FT_THREADS, 0, s>>>(img1, img2, B, H, W, kp, box);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
static int ft_launch_describe(const uint16_t* box, const int32_t* kp, int n2, int H, int W, uint32_t* desc, hipStream_t s) {
    const int N = ft_slots(H, W);
    ft_describe_kernel<<<dim3((N * FT_WORDS + FT_THREADS - 1) / FT_THREADS, n2), FT_THREADS, 0, s>>>(box, kp, H, W, N, desc);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
int ft_launch_match(const int32_t* kp1, const uint32_t* desc1, const int32_t* kp2, const uint32_t* desc2, int B, int N, int32_t* nn, int32_t* matches, int32_t* count,
                    hipStream_t s) {
    ft_match_kernel<<<dim3((N + 31) / 32, 2, B), FT_THREADS, 0, s>>>(kp1, desc1, kp2, desc2, B, N, nn);
    ST_CHECK_LAUNCH();
    ft_compact_kernel<<<B, 1024, 0, s>>>(nn, B, N, matches, count);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
int ft_launch_hyp_refit(ft_refit_fn refit, const int32_t* kp1, const int32_t* kp2, const double* mc, const int32_t* count, int B, int H, int W, int N, int max_hyp,
                        double thr2, int min_inliers, uint32_t seed, int32_t* scores, float* motion, float* Hout, int32_t* info, uint8_t* mask, hipStream_t s) {
    ft_hyp_kernel<<<dim3((max_hyp + 63) / 64, B), 64, 0, s>>>(mc, count, H, W, N, max_hyp, seed, thr2, scores);
    ST_CHECK_LAUNCH();
    refit<<<B, FT_THREADS, 0, s>>>(kp1, kp2, mc, count, scores, H, W, N, max_hyp, seed, thr2, min_inliers, motion, Hout, info, mask);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
static int ft_launch_ransac(const int32_t* kp1, const int32_t* kp2, const int32_t* matches, const int32_t* count, int B, int H, int W, int max_hyp, double thr,
                            int min_inliers, uint32_t seed, double* mc, int32_t* scores, float* motion, float* Hout, int32_t* info, uint8_t* mask, hipStream_t s) {
    const int N = ft_slots(H, W);
    ft_norm_kernel<<<dim3((N + FT_THREADS - 1) / FT_THREADS, B), FT_THREADS, 0, s>>>(kp1, kp2, matches, count, H, W, N, mc);
    ST_CHECK_LAUNCH();
    return ft_launch_hyp_refit(ft_refit_kernel, kp1, kp2, mc, count, B, H, W, N, max_hyp, thr * thr, min_inliers, seed, scores, motion, Hout, info, mask, s);
}

extern "C" int st_feature_slots(int32_t H, int32_t W) { return ft_shape_ok(1, H, W) ? ft_slots(H, W) : 0; }

extern "C" int st_feature_brief_pattern(int8_t* out_host) {
    if (!out_host) return ST_EINVAL;
    for (int i = 0; i < 1024; ++i) out_host[i] = ft_pattern_host.v[i];
    return ST_OK;
}

extern "C" int st_feature_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t max_hyp) {
    ft_layout L;
    return ft_plan(B, H, W, max_hyp, L) ? (int)L.total : 0;
}

extern "C" int st_feature_workspace_layout(int32_t B, int32_t H, int32_t W, int32_t max_hyp, int64_t* offsets_host) {
    ft_layout L;
    if (!offsets_host || !ft_plan(B, H, W, max_hyp, L)) return ST_EINVAL;
    const int64_t o[10] = {L.box, L.kp, L.desc, L.nn, L.matches, L.count, L.mc, L.scores, L.mask, L.total};
    for (int i = 0; i < 10; ++i) offsets_host[i] = o[i];
    return ST_OK;
}

extern "C" int st_feature_detect(const float* img, int32_t B, int32_t H, int32_t W, int32_t* kp_out, uint16_t* box_out, void* stream) {
    if (!ft_shape_ok(B, H, W)) return ST_EINVAL;
    const int64_t px = (int64_t)B * H * W, N = ft_slots(H, W);
    const ft_region r[3] = {{img, 12 * px, false}, {kp_out, 8 * B * N, true}, {box_out, 2 * px, true}};
    if (!ft_regions_ok(r, 3)) return ST_EINVAL;
    return ft_launch_detect(img, img, B, 1, H, W, kp_out, box_out, (hipStream_t)stream);
}

extern "C" int st_feature_describe(const uint16_t* box, const int32_t* kp, int32_t B, int32_t H, int32_t W, uint32_t* desc_out, void* stream) {
    if (!ft_shape_ok(B, H, W)) return ST_EINVAL;
    const int64_t px = (int64_t)B * H * W, N = ft_slots(H, W);
    const ft_region r[3] = {{box, 2 * px, false}, {kp, 8 * B * N, false}, {desc_out, 32 * B * N, true}};
    if (!ft_regions_ok(r, 3)) return ST_EINVAL;
    return ft_launch_describe(box, kp, B, H, W, desc_out, (hipStream_t)stream);
}

extern "C" int st_feature_match(const int32_t* kp1, const uint32_t* desc1, const int32_t* kp2, const uint32_t* desc2, int32_t B, int32_t H, int32_t W, int32_t* nn_out,
                                int32_t* matches_out, int32_t* count_out, void* stream) {
    if (!ft_shape_ok(B, H, W)) return ST_EINVAL;
    const int N = ft_slots(H, W);
    if (!ft_match_operands_ok(kp1, desc1, kp2, desc2, nn_out, matches_out, count_out, B, N)) return ST_EINVAL;
    return ft_launch_match(kp1, desc1, kp2, desc2, B, N, nn_out, matches_out, count_out, (hipStream_t)stream);
}

extern "C" int st_feature_ransac(const int32_t* kp1, const int32_t* kp2, const int32_t* matches, const int32_t* count, int32_t B, int32_t H, int32_t W, int32_t max_hyp,
                                 double thr, int32_t min_inliers, int32_t seed, float* motion_out, float* H_out, int32_t* info_out, uint8_t* mask_out, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
    if (!ft_shape_ok(B, H, W) || !ft_params_ok(max_hyp, thr, min_inliers)) return ST_EINVAL;
    const int64_t N = ft_slots(H, W);
    if (!ft_ransac_operands_ok(kp1, kp2, matches, count, motion_out, H_out, info_out, mask_out, nullptr, false, workspace, workspace_bytes, B, N, max_hyp)) return ST_EINVAL;
    return ft_launch_ransac(kp1, kp2, matches, count, B, H, W, max_hyp, thr, min_inliers, (uint32_t)seed, (double*)workspace, (int32_t*)((char*)workspace + 32 * B * N),
                            motion_out, H_out, info_out, mask_out, (hipStream_t)stream);
}

extern "C" int st_feature_homography(const float* img1, const float* img2, int32_t B, int32_t H, int32_t W, int32_t max_hyp, double thr, int32_t min_inliers,
                                     int32_t seed, float* motion_out, float* H_out, int32_t* info_out, void* workspace, int64_t workspace_bytes, void* stream) {
    ft_layout L;
    if (!ft_plan(B, H, W, max_hyp, L) || !ft_params_ok(max_hyp, thr, min_inliers)) return ST_EINVAL;
    if (workspace_bytes < L.total || ((uintptr_t)workspace & 15)) return ST_EINVAL;
    const int64_t px = (int64_t)B * H * W;
    const ft_region r[6] = {{img1, 12 * px, false}, {img2, 12 * px, false}, {motion_out, 32 * B, true}, {H_out, 36 * B, true}, {info_out, 32 * B, true},
                            {workspace, L.total, true}};
    if (!ft_regions_ok(r, 6)) return ST_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int64_t bn = (int64_t)B * L.N;
    int32_t* kp = (int32_t*)(ws + L.kp);
    uint32_t* desc = (uint32_t*)(ws + L.desc);
    int32_t* matches = (int32_t*)(ws + L.matches);
    int32_t* count = (int32_t*)(ws + L.count);
    int rc = ft_launch_detect(img1, img2, B, 2, H, W, kp, (uint16_t*)(ws + L.box), s);
    if (rc) return rc;
    rc = ft_launch_describe((const uint16_t*)(ws + L.box), kp, 2 * B, H, W, desc, s);
    if (rc) return rc;
    rc = ft_launch_match(kp, desc, kp + 2 * bn, desc + 8 * bn, B, L.N, (int32_t*)(ws + L.nn), matches, count, s);
    if (rc) return rc;
    return ft_launch_ransac(kp, kp + 2 * bn, matches, count, B, H, W, max_hyp, thr, min_inliers, (uint32_t)seed, (double*)(ws + L.mc), (int32_t*)(ws + L.scores),
                            motion_out, H_out, info_out, (uint8_t*)(ws + L.mask), s);
}
