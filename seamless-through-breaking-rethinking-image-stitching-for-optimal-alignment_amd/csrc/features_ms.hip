// feature_align_ms: the oriented, multi-scale front end beside feature_align -- a 5/4 luma pyramid, Harris corners on every level, a 32-bin
// orientation from the intensity centroid, the BRIEF-256 pattern steered by it, then feature_align's own matching and RANSAC over the slots
// of all levels in level-0 coordinates.  Contract in README.md, "feature_align_ms"; CPU restatement tests/_features_ms_ref.py.  gfx950 only.
// Everything is integer up to the match list and fp64 from there on (-ffp-contract=off).  Same conventions as features.hip: the caller's
// stream and buffers, no host synchronisation, allocation, memset / memcpy or atomics, one writer per word, and a launch count and grids
// that depend on B, H, W, levels and max_hyp alone.  The match, compaction and hypothesis kernels are those of features.hip, launched with
// the total number of slots.
//
//   ftms_luma_kernel      one thread per pixel: level 0 of the pyramid, the luma as uint8
//   ftms_down_kernel      one thread per coarser pixel: level l+1 from level l, centre-aligned x 5/4, bilinear in 1/256 px
//   ftms_detect_kernel    one workgroup per 32x32 cell, all levels in one launch: ft_detect_kernel's corner body (ft_corners) on a luma tile with a halo of
//                         15, border 20, then one wave per winner: the two first moments over the disc of radius 15 from the tile, the best of 32 bins
//   ftms_describe_kernel  one thread per descriptor word: 32 comparisons of box sums of the slot's level at offsets steered by its bin
//   ftms_norm_kernel      level-0 coordinates of every slot and the normalised fp64 coordinates of the matches
//   ftms_refit_kernel     ft_refit_kernel's body (ft_refit) with the inlier flags of FTMS_MAX_SLOTS list entries in LDS
#include "features_common.h"

#define FTMS_MAX_LEVELS 8
#define FTMS_BORDER 20                  // steered offsets reach 17, the box sum 2 more
#define FTMS_RADIUS 15
#define FTMS_TILE (FT_CELL + 2 * FTMS_RADIUS)
#define FTMS_BINS 32
#define FTMS_MAX_SLOTS 11520            // 1024 x 1024 at 8 levels has 11508

// level l is H[l] x W[l] and owns the slots slot0[l] .. slot0[l+1] - 1 (slot0[k] = N for k > L); pix0[l] pixels of one plane lie before it
struct ftms_levels {
    int L, N;
    int H[FTMS_MAX_LEVELS], W[FTMS_MAX_LEVELS], slot0[FTMS_MAX_LEVELS + 1];
    long long pix0[FTMS_MAX_LEVELS + 1];
};

__constant__ ft_pattern_t ftms_pattern = ft_make_pattern();

// (c, s) of bin b, 1024 (cos, sin)(b * 11.25 degrees) rounded: the literal first quarter, the others by (c, s) -> (-s, c)
struct ftms_cs_t {
    int16_t v[2 * FTMS_BINS];
};
constexpr ftms_cs_t ftms_make_cs() {
    constexpr int q[9] = {1024, 1004, 946, 851, 724, 569, 392, 200, 0};
    ftms_cs_t t{};
    for (int b = 0; b < FTMS_BINS; ++b) {
        int c = q[b % 8], s = q[8 - b % 8];
        for (int r = 0; r < b / 8; ++r) {
            const int nc = -s;
            s = c, c = nc;
        }
        t.v[2 * b] = (int16_t)c, t.v[2 * b + 1] = (int16_t)s;
    }
    return t;
}
__constant__ ftms_cs_t ftms_cs = ftms_make_cs();

// planes z < B of img1, the others of img2; y uint8 [planes, H, W]
__global__ void __launch_bounds__(FT_THREADS) ftms_luma_kernel(const float* __restrict__ img1, const float* __restrict__ img2, int B, int H, int W, uint8_t* __restrict__ y) {
    const int z = blockIdx.y;
    const size_t hw = (size_t)H * W, g = (size_t)blockIdx.x * FT_THREADS + threadIdx.x;
    if (g >= hw) return;
    const float* img = (z < B ? img1 + (size_t)z * 3 * hw : img2 + (size_t)(z - B) * 3 * hw);
    const int r = ft_pixel(img[g]), gg = ft_pixel(img[hw + g]), b = ft_pixel(img[2 * hw + g]);
    y[(size_t)z * hw + g] = (uint8_t)((19595 * r + 38470 * gg + 7471 * b + 0x8000) >> 16);
}

// dst (i, j) samples src at (160 (2j + 1) - 128, 160 (2i + 1) - 128) / 256; Hd = 4 Hs div 5, so the first tap is at most Hs - 2
__global__ void __launch_bounds__(FT_THREADS) ftms_down_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, uint8_t* __restrict__ dst, int Hd, int Wd) {
    const int g = blockIdx.x * FT_THREADS + threadIdx.x, z = blockIdx.y;
    if (g >= Hd * Wd) return;
    const int i = g / Wd, j = g - i * Wd;
    const int sx = 160 * (2 * j + 1) - 128, sy = 160 * (2 * i + 1) - 128;
    const int x0 = sx >> 8, fx = sx & 255, y0 = sy >> 8, fy = sy & 255, x1 = min(x0 + 1, Ws - 1), y1 = min(y0 + 1, Hs - 1);
    const uint8_t* s = src + (size_t)z * Hs * Ws;
    const int a = s[y0 * Ws + x0], b = s[y0 * Ws + x1], c = s[y1 * Ws + x0], d = s[y1 * Ws + x1];
    dst[(size_t)z * Hd * Wd + g] = (uint8_t)(((256 - fx) * (256 - fy) * a + fx * (256 - fy) * b + (256 - fx) * fy * c + fx * fy * d + (1 << 15)) >> 16);
}

// the level of a slot and its size and plane offset, without indexing the argument struct by a run-time value
__device__ __forceinline__ int ftms_level_of(const ftms_levels& V, int slot, int& Hl, int& Wl, int& slot0, long long& pix0) {
    int l = 0;
#pragma unroll
    for (int k = 1; k < FTMS_MAX_LEVELS; ++k) l += slot >= V.slot0[k];
    Hl = V.H[0], Wl = V.W[0], slot0 = 0, pix0 = 0;
#pragma unroll
    for (int k = 1; k < FTMS_MAX_LEVELS; ++k)
        if (l == k) Hl = V.H[k], Wl = V.W[k], slot0 = V.slot0[k], pix0 = V.pix0[k];
    return l;
}

// all levels in one launch, workgroup c = the cell of the slots 4 c .. 4 c + 3: pyr uint8 and box uint16 hold level l's [n2, H_l, W_l] planes at
// pix0[l] n2; kp int32 [n2, N, 2], bins uint8 [n2, N]
__global__ void __launch_bounds__(FT_THREADS) ftms_detect_kernel(const uint8_t* __restrict__ pyr, ftms_levels V, int n2, int oriented, int32_t* __restrict__ kp,
                                                                  uint8_t* __restrict__ bins, uint16_t* __restrict__ box_all) {
    __shared__ uint8_t sy[FTMS_TILE][FTMS_TILE + 2];
    __shared__ int swin[FT_PER_CELL];
    const int t = threadIdx.x, z = blockIdx.y, N = V.N;
    int H, W, slot0;
    long long pix0;
    ftms_level_of(V, FT_PER_CELL * blockIdx.x, H, W, slot0, pix0);
    const int CW = (W + FT_CELL - 1) / FT_CELL, cell = blockIdx.x - slot0 / FT_PER_CELL, cy = cell / CW;
    const int x0 = (cell - cy * CW) * FT_CELL, y0 = cy * FT_CELL;
    const size_t hw = (size_t)H * W, slot = (size_t)z * N + FT_PER_CELL * blockIdx.x;
    const uint8_t* img = pyr + (size_t)pix0 * n2 + (size_t)z * hw;
    for (int e = t; e < FTMS_TILE * FTMS_TILE; e += FT_THREADS) {
        const int ty = e / FTMS_TILE, tx = e - ty * FTMS_TILE;
        const int y = min(max(y0 - FTMS_RADIUS + ty, 0), H - 1), x = min(max(x0 - FTMS_RADIUS + tx, 0), W - 1);
        sy[ty][tx] = img[(size_t)y * W + x];
    }
    __syncthreads();
    int won[FT_PER_CELL];
    ft_corners<FTMS_RADIUS, FTMS_BORDER>(sy, x0, y0, H, W, kp + slot * 2, box_all + (size_t)pix0 * n2 + (size_t)z * hw, won);
    if (t == 0)                                              // (every thread holds won[]; a wave picks its own through LDS as it always did, which keeps the 19680 bytes)
#pragma unroll
        for (int r = 0; r < FT_PER_CELL; ++r) swin[r] = won[r];
    __syncthreads();
    // wave `rank` takes winner `rank`: m10 = sum dx Y, m01 = sum dy Y over the disc (a winner is 20 px inside the level: the disc lies in the
    // tile and in the image), then the bin that maximises m10 c + m01 s, ties to the lowest
    const int rank = t >> 6, lane = t & 63, win = swin[rank];
    int bin = 0;
    if (oriented && win >= 0) {                              // wave-uniform
        const int wy = win / W, py = wy - y0, px = win - wy * W - x0;
        int m10 = 0, m01 = 0;
        for (int e = lane; e < (2 * FTMS_RADIUS + 1) * (2 * FTMS_RADIUS + 1); e += 64) {
            const int ey = e / (2 * FTMS_RADIUS + 1), dy = ey - FTMS_RADIUS, dx = e - ey * (2 * FTMS_RADIUS + 1) - FTMS_RADIUS;
            if (dx * dx + dy * dy <= FTMS_RADIUS * FTMS_RADIUS) {
                const int v = sy[py + FTMS_RADIUS + dy][px + FTMS_RADIUS + dx];
                m10 += dx * v, m01 += dy * v;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m10 += __shfl_xor(m10, o, 64), m01 += __shfl_xor(m01, o, 64);
        const int b = lane & (FTMS_BINS - 1);                // (lanes 32..63 repeat the bins: the reduction below is indifferent to that)
        long long best = (long long)m10 * ftms_cs.v[2 * b] + (long long)m01 * ftms_cs.v[2 * b + 1];
        bin = b;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const long long qv = ft_shfl_xor64(best, o);
            const int qb = __shfl_xor(bin, o, 64);
            if (ft_better(qv, qb, best, bin)) best = qv, bin = qb;
        }
    }
    if (lane == 0) bins[slot + rank] = (uint8_t)bin;
}

// box uint16: level l's [n2, H_l, W_l] planes at pix0[l] n2; kp int32 [n2, N, 2]; bins uint8 [n2, N]; desc uint32 [n2, N, 8]
__global__ void __launch_bounds__(FT_THREADS) ftms_describe_kernel(const uint16_t* __restrict__ box, const int32_t* __restrict__ kp, const uint8_t* __restrict__ bins,
                                                                    ftms_levels V, int n2, uint32_t* __restrict__ desc) {
    const int g = blockIdx.x * FT_THREADS + threadIdx.x, z = blockIdx.y, N = V.N;
    if (g >= N * FT_WORDS) return;
    const int slot = g >> 3, word = g & 7;
    int Hl, Wl, slot0;
    long long pix0;
    ftms_level_of(V, slot, Hl, Wl, slot0, pix0);
    const int x = kp[((size_t)z * N + slot) * 2], y = kp[((size_t)z * N + slot) * 2 + 1];
    uint32_t bits = 0;
    if (x >= FTMS_BORDER && x < Wl - FTMS_BORDER && y >= FTMS_BORDER && y < Hl - FTMS_BORDER) {   // (a valid slot always is; anything else reads nothing)
        const int bin = bins[(size_t)z * N + slot] & (FTMS_BINS - 1), c = ftms_cs.v[2 * bin], sn = ftms_cs.v[2 * bin + 1];
        const uint16_t* s = box + (size_t)pix0 * n2 + (size_t)z * Hl * Wl;
        for (int b = 0; b < 32; ++b) {
            const int8_t* o = ftms_pattern.v + 4 * (word * 32 + b);
            const int ax = (o[0] * c - o[1] * sn + 512) >> 10, ay = (o[0] * sn + o[1] * c + 512) >> 10;
            const int bx = (o[2] * c - o[3] * sn + 512) >> 10, by = (o[2] * sn + o[3] * c + 512) >> 10;
            const uint32_t sa = s[(y + ay) * Wl + x + ax], sb = s[(y + by) * Wl + x + bx];
            bits |= (uint32_t)(sa < sb) << b;
        }
    }
    desc[((size_t)z * N + slot) * FT_WORDS + word] = bits;
}

// level-0 position of pixel v of level l: ((2 v + 1) 5^l) / (2 4^l) - 1/2, every step exact in fp64
__device__ __forceinline__ double ftms_level0(int v, int p5, int p4) { return (double)((2 * v + 1) * p5) / (double)(2 * p4) - 0.5; }

__device__ __forceinline__ void ftms_coords(const ftms_levels& V, const int32_t* __restrict__ kp, int slot, double& X, double& Y) {
    int Hl, Wl, slot0, p5 = 1, p4 = 1;
    long long pix0;
    const int l = ftms_level_of(V, slot, Hl, Wl, slot0, pix0), x = kp[2 * slot], y = kp[2 * slot + 1];
    for (int k = 0; k < l; ++k) p5 *= 5, p4 *= 4;
    X = x >= 0 ? ftms_level0(x, p5, p4) : -1.0, Y = x >= 0 ? ftms_level0(y, p5, p4) : -1.0;
}

// xy fp64 [2, B, N, 2]: the level-0 coordinates of every slot of both images, (-1, -1) in an unused one; mc fp64 [B, N, 4] as ft_norm_kernel's
__global__ void __launch_bounds__(FT_THREADS) ftms_norm_kernel(const int32_t* __restrict__ kp1, const int32_t* __restrict__ kp2, const int32_t* __restrict__ matches,
                                                                const int32_t* __restrict__ count, ftms_levels V, int B, int H, int W, double* __restrict__ xy,
                                                                double* __restrict__ mc) {
    const int p = blockIdx.x * FT_THREADS + threadIdx.x, b = blockIdx.y, N = V.N;
    if (p >= N) return;
    const int32_t* k1 = kp1 + (size_t)b * N * 2;
    const int32_t* k2 = kp2 + (size_t)b * N * 2;
    double X, Y;
    ftms_coords(V, k1, p, X, Y);
    xy[((size_t)b * N + p) * 2] = X, xy[((size_t)b * N + p) * 2 + 1] = Y;
    ftms_coords(V, k2, p, X, Y);
    xy[(((size_t)B + b) * N + p) * 2] = X, xy[(((size_t)B + b) * N + p) * 2 + 1] = Y;
    if (p >= ft_count(count, b, N)) return;
    const int i = min(max(matches[((size_t)b * N + p) * 2], 0), N - 1), j = min(max(matches[((size_t)b * N + p) * 2 + 1], 0), N - 1);
    const double sx = 0.5 * W, sy = 0.5 * H;
    double* o = mc + ((size_t)b * N + p) * 4;
    ftms_coords(V, k1, i, X, Y);
    o[0] = (X - sx) / sx, o[1] = (Y - sy) / sy;
    ftms_coords(V, k2, j, X, Y);
    o[2] = (X - sx) / sx, o[3] = (Y - sy) / sy;
}

__global__ void __launch_bounds__(FT_THREADS) ftms_refit_kernel(const int32_t* __restrict__ kp1, const int32_t* __restrict__ kp2, const double* __restrict__ mc,
                                                                 const int32_t* __restrict__ count, const int32_t* __restrict__ scores, int H, int W, int N, int max_hyp,
                                                                 uint32_t seed, double thr2, int min_inliers, float* __restrict__ motion, float* __restrict__ Hout,
                                                                 int32_t* __restrict__ info, uint8_t* __restrict__ mask) {
    ft_refit<FTMS_MAX_SLOTS>(kp1, kp2, mc, count, scores, H, W, N, max_hyp, seed, thr2, min_inliers, motion, Hout, info, mask);    // (N <= FTMS_MAX_SLOTS by ftms_levels_plan)
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
static bool ftms_levels_plan(int H, int W, int levels, ftms_levels& V) {
    if (!ft_shape_ok(1, H, W) || levels < 1 || levels > FTMS_MAX_LEVELS) return false;
    V = ftms_levels{};
    int h = H, w = W, l = 0;
    for (;;) {
        V.H[l] = h, V.W[l] = w, V.slot0[l + 1] = V.slot0[l] + ft_slots(h, w), V.pix0[l + 1] = V.pix0[l] + (long long)h * w;
        ++l;
        const int nh = 4 * h / 5, nw = 4 * w / 5;
        if (l >= levels || (nh < nw ? nh : nw) < FT_MIN_SIDE) break;
        h = nh, w = nw;
    }
    V.L = l, V.N = V.slot0[l];
    for (int k = l + 1; k <= FTMS_MAX_LEVELS; ++k) V.slot0[k] = V.N, V.pix0[k] = V.pix0[l];
    return V.N <= FTMS_MAX_SLOTS;
}

// workspace of st_feature_ms_homography, every region rounded up to 16 bytes (P pixels of one plane over all levels, level l's planes at P_l n2):
// pyr uint8 [2B P]; box uint16 [2B P]; kp int32 [2,B,N,2]; bins uint8 [2,B,N]; desc uint32 [2,B,N,8]; nn int32 [2,B,N,3]; matches int32 [B,N,2];
// count int32 [B]; xy fp64 [2,B,N,2]; mc fp64 [B,N,4]; scores int32 [B,max_hyp]; mask uint8 [B,N]
struct ftms_layout {
    ftms_levels V;
    int64_t pyr, box, kp, bins, desc, nn, matches, count, xy, mc, scores, mask, total;
};
static bool ftms_plan(int B, int H, int W, int levels, int max_hyp, ftms_layout& L) {
    if (!ft_shape_ok(B, H, W) || max_hyp < 1 || max_hyp > FT_MAX_HYP || !ftms_levels_plan(H, W, levels, L.V)) return false;
    int64_t at = 0;
    auto take = [&](int64_t bytes) { const int64_t o = at; at += (bytes + 15) & ~(int64_t)15; return o; };
    const int64_t N = L.V.N, P = L.V.pix0[L.V.L], b = B;
    L.pyr = take(2 * b * P), L.box = take(2 * 2 * b * P), L.kp = take(4 * 2 * b * N * 2), L.bins = take(2 * b * N), L.desc = take(4 * 2 * b * N * 8);
    L.nn = take(4 * 2 * b * N * 3), L.matches = take(4 * b * N * 2), L.count = take(4 * b), L.xy = take(8 * 2 * b * N * 2), L.mc = take(8 * b * N * 4);
    L.scores = take(4 * b * max_hyp), L.mask = take(b * N);
    L.total = at;
    return at < ((int64_t)1 << 31);
}

static int ftms_launch_pyramid(const float* img1, const float* img2, int B, int nimg, const ftms_levels& V, uint8_t* pyr, hipStream_t s) {
    const int n2 = nimg * B;
    ftms_luma_kernel<<<dim3((V.H[0] * V.W[0] + FT_THREADS - 1) / FT_THREADS, n2), FT_THREADS, 0, s>>>(img1, img2, B, V.H[0], V.W[0], pyr);
    ST_CHECK_LAUNCH();
    for (int l = 1; l < V.L; ++l) {
        ftms_down_kernel<<<dim3((V.H[l] * V.W[l] + FT_THREADS - 1) / FT_THREADS, n2), FT_THREADS, 0, s>>>(pyr + V.pix0[l - 1] * n2, V.H[l - 1], V.W[l - 1],
                                                                                                       pyr + V.pix0[l] * n2, V.H[l], V.W[l]);
        ST_CHECK_LAUNCH();
    }
    return ST_OK;
}
static int ftms_launch_detect(const uint8_t* pyr, int n2, const ftms_levels& V, int oriented, int32_t* kp, uint8_t* bins, uint16_t* box, hipStream_t s) {
    ftms_detect_kernel<<<dim3(V.N / FT_PER_CELL, n2), FT_THREADS, 0, s>>>(pyr, V, n2, oriented, kp, bins, box);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
static int ftms_launch_describe(const uint16_t* box, const int32_t* kp, const uint8_t* bins, int n2, const ftms_levels& V, uint32_t* desc, hipStream_t s) {
    ftms_describe_kernel<<<dim3((V.N * FT_WORDS + FT_THREADS - 1) / FT_THREADS, n2), FT_THREADS, 0, s>>>(box, kp, bins, V, n2, desc);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
static int ftms_launch_ransac(const int32_t* kp1, const int32_t* kp2, const int32_t* matches, const int32_t* count, int B, int H, int W, const ftms_levels& V, int max_hyp,
                              double thr, int min_inliers, uint32_t seed, double* xy, double* mc, int32_t* scores, float* motion, float* Hout, int32_t* info,
                              uint8_t* mask, hipStream_t s) {
    const int N = V.N;
    ftms_norm_kernel<<<dim3((N + FT_THREADS - 1) / FT_THREADS, B), FT_THREADS, 0, s>>>(kp1, kp2, matches, count, V, B, H, W, xy, mc);
    ST_CHECK_LAUNCH();
    return ft_launch_hyp_refit(ftms_refit_kernel, kp1, kp2, mc, count, B, H, W, N, max_hyp, thr * thr, min_inliers, seed, scores, motion, Hout, info, mask, s);
}

extern "C" int st_feature_ms_level_sizes(int32_t H, int32_t W, int32_t levels, int32_t* sizes_host) {
    ftms_levels V;
    if (!ftms_levels_plan(H, W, levels, V)) return 0;
    if (sizes_host)
        for (int l = 0; l < FTMS_MAX_LEVELS; ++l) sizes_host[2 * l] = V.H[l], sizes_host[2 * l + 1] = V.W[l];
    return V.L;
}

extern "C" int st_feature_ms_slots(int32_t H, int32_t W, int32_t levels) {
    ftms_levels V;
    return ftms_levels_plan(H, W, levels, V) ? V.N : 0;
}

extern "C" int st_feature_ms_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t levels, int32_t max_hyp) {
    ftms_layout L;
    return ftms_plan(B, H, W, levels, max_hyp, L) ? (int)L.total : 0;
}

extern "C" int st_feature_ms_workspace_layout(int32_t B, int32_t H, int32_t W, int32_t levels, int32_t max_hyp, int64_t* offsets_host) {
    ftms_layout L;
    if (!offsets_host || !ftms_plan(B, H, W, levels, max_hyp, L)) return ST_EINVAL;
    const int64_t o[13] = {L.pyr, L.box, L.kp, L.bins, L.desc, L.nn, L.matches, L.count, L.xy, L.mc, L.scores, L.mask, L.total};
    for (int i = 0; i < 13; ++i) offsets_host[i] = o[i];
    return ST_OK;
}

extern "C" int st_feature_ms_pyramid(const float* img, int32_t B, int32_t H, int32_t W, int32_t levels, uint8_t* pyr_out, void* stream) {
    ftms_levels V;
    if (!ft_shape_ok(B, H, W) || !ftms_levels_plan(H, W, levels, V)) return ST_EINVAL;
    const int64_t P = V.pix0[V.L];
    const ft_region r[2] = {{img, 12 * (int64_t)B * H * W, false}, {pyr_out, B * P, true}};
    if (!ft_regions_ok(r, 2)) return ST_EINVAL;
    return ftms_launch_pyramid(img, img, B, 1, V, pyr_out, (hipStream_t)stream);
}

extern "C" int st_feature_ms_detect(const uint8_t* pyr, int32_t B, int32_t H, int32_t W, int32_t levels, int32_t oriented, int32_t* kp_out, uint8_t* bins_out,
                                    uint16_t* box_out, void* stream) {
    ftms_levels V;
    if (!ft_shape_ok(B, H, W) || !ftms_levels_plan(H, W, levels, V) || (oriented != 0 && oriented != 1)) return ST_EINVAL;
    const int64_t P = V.pix0[V.L], bn = (int64_t)B * V.N;
    const ft_region r[4] = {{pyr, B * P, false}, {kp_out, 8 * bn, true}, {bins_out, bn, true}, {box_out, 2 * B * P, true}};
    if (!ft_regions_ok(r, 4)) return ST_EINVAL;
    return ftms_launch_detect(pyr, B, V, oriented, kp_out, bins_out, box_out, (hipStream_t)stream);
}

extern "C" int st_feature_ms_describe(const uint16_t* box, const int32_t* kp, const uint8_t* bins, int32_t B, int32_t H, int32_t W, int32_t levels, uint32_t* desc_out,
                                      void* stream) {
    ftms_levels V;
    if (!ft_shape_ok(B, H, W) || !ftms_levels_plan(H, W, levels, V)) return ST_EINVAL;
    const int64_t P = V.pix0[V.L], bn = (int64_t)B * V.N;
    const ft_region r[4] = {{box, 2 * B * P, false}, {kp, 8 * bn, false}, {bins, bn, false}, {desc_out, 32 * bn, true}};
    if (!ft_regions_ok(r, 4)) return ST_EINVAL;
    return ftms_launch_describe(box, kp, bins, B, V, desc_out, (hipStream_t)stream);
}

extern "C" int st_feature_ms_match(const int32_t* kp1, const uint32_t* desc1, const int32_t* kp2, const uint32_t* desc2, int32_t B, int32_t H, int32_t W, int32_t levels,
                                   int32_t* nn_out, int32_t* matches_out, int32_t* count_out, void* stream) {
    ftms_levels V;
    if (!ft_shape_ok(B, H, W) || !ftms_levels_plan(H, W, levels, V)) return ST_EINVAL;
    if (!ft_match_operands_ok(kp1, desc1, kp2, desc2, nn_out, matches_out, count_out, B, V.N)) return ST_EINVAL;
    return ft_launch_match(kp1, desc1, kp2, desc2, B, V.N, nn_out, matches_out, count_out, (hipStream_t)stream);
}

extern "C" int st_feature_ms_ransac(const int32_t* kp1, const int32_t* kp2, const int32_t* matches, const int32_t* count, int32_t B, int32_t H, int32_t W, int32_t levels,
                                    int32_t max_hyp, double thr, int32_t min_inliers, int32_t seed, float* motion_out, float* H_out, int32_t* info_out, uint8_t* mask_out,
                                    double* xy_out, void* workspace, int64_t workspace_bytes, void* stream) {
    ftms_levels V;
    if (!ft_shape_ok(B, H, W) || !ftms_levels_plan(H, W, levels, V) || !ft_params_ok(max_hyp, thr, min_inliers)) return ST_EINVAL;
    if (!ft_ransac_operands_ok(kp1, kp2, matches, count, motion_out, H_out, info_out, mask_out, xy_out, true, workspace, workspace_bytes, B, V.N, max_hyp)) return ST_EINVAL;
    return ftms_launch_ransac(kp1, kp2, matches, count, B, H, W, V, max_hyp, thr, min_inliers, (uint32_t)seed, xy_out, (double*)workspace,
                              (int32_t*)((char*)workspace + 32 * (int64_t)B * V.N), motion_out, H_out, info_out, mask_out, (hipStream_t)stream);
}

extern "C" int st_feature_ms_homography(const float* img1, const float* img2, int32_t B, int32_t H, int32_t W, int32_t levels, int32_t oriented, int32_t max_hyp, double thr,
                                        int32_t min_inliers, int32_t seed, float* motion_out, float* H_out, int32_t* info_out, void* workspace, int64_t workspace_bytes,
                                        void* stream) {
    ftms_layout L;
    if (!ftms_plan(B, H, W, levels, max_hyp, L) || !ft_params_ok(max_hyp, thr, min_inliers) || (oriented != 0 && oriented != 1)) return ST_EINVAL;
    if (workspace_bytes < L.total || ((uintptr_t)workspace & 15)) return ST_EINVAL;
    const int64_t px = (int64_t)B * H * W;
    const ft_region r[6] = {{img1, 12 * px, false}, {img2, 12 * px, false}, {motion_out, 32 * B, true}, {H_out, 36 * B, true}, {info_out, 32 * B, true},
                            {workspace, L.total, true}};
    if (!ft_regions_ok(r, 6)) return ST_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int64_t bn = (int64_t)B * L.V.N;
    uint8_t* pyr = (uint8_t*)(ws + L.pyr);
    uint16_t* box = (uint16_t*)(ws + L.box);
    int32_t* kp = (int32_t*)(ws + L.kp);
    uint8_t* bins = (uint8_t*)(ws + L.bins);
    uint32_t* desc = (uint32_t*)(ws + L.desc);
    int32_t* matches = (int32_t*)(ws + L.matches);
    int32_t* count = (int32_t*)(ws + L.count);
    int rc = ftms_launch_pyramid(img1, img2, B, 2, L.V, pyr, s);
    if (rc) return rc;
    rc = ftms_launch_detect(pyr, 2 * B, L.V, oriented, kp, bins, box, s);
    if (rc) return rc;
    rc = ftms_launch_describe(box, kp, bins, 2 * B, L.V, desc, s);
    if (rc) return rc;
    rc = ft_launch_match(kp, desc, kp + 2 * bn, desc + 8 * bn, B, L.V.N, (int32_t*)(ws + L.nn), matches, count, s);
    if (rc) return rc;
    return ftms_launch_ransac(kp, kp + 2 * bn, matches, count, B, H, W, L.V, max_hyp, thr, min_inliers, (uint32_t)seed, (double*)(ws + L.xy), (double*)(ws + L.mc),
                              (int32_t*)(ws + L.scores), motion_out, H_out, info_out, (uint8_t*)(ws + L.mask), s);
}
