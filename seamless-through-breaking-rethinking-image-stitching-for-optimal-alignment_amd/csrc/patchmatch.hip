// patchmatch_inpainter: exemplar hole filling -- PatchMatch (Barnes et al. 2009) inside a coarse-to-fine vote / search loop (Wexler et al.
// 2007).  Contract in README.md, "patchmatch_inpainter"; CPU restatement tests/_patchmatch_ref.py.  gfx950 only.  Everything is integers.
// Every kernel of a call goes to the caller's stream, in order, inside the caller's workspace: no host synchronisation, no allocation, no
// memset / memcpy, no atomics (every word has exactly one writer), and the launch count and every grid depend on H, W, levels and iters
// alone, so a call captures into a hipGraph as a linear chain.  What depends on the data -- how many sources and targets a level has,
// the level the fill starts at, whether there is anything to fill at all -- is read on the device by the kernels it concerns.
//
//   pm_pack_kernel      level 0: one RGBX word per pixel (X = 0) and the hole plane
//   pm_down_kernel      level l + 1 from level l: hole iff any child is one, colour the half-up mean of the known children
//   pm_classify_kernel  kind plane (0 / source / target) of a level and the counts of every block of 1024 pixels
//   pm_scan_kernel      one workgroup: exclusive scan of the block counts, the level's totals
//   pm_compact_kernel   the row-major source and target lists (y << 16 | x)
//   pm_decide_kernel    one thread: valid, start level -> ctl and info
//   pm_init_kernel      NNF of every target: the coarse match doubled, or a hash draw from the source list
//   pm_vote_kernel      every hole pixel <- half-up mean of the pixels its <= 49 covering target patches map onto it (a gather)
//   pm_sweep_kernel     one Jacobi search sweep over the target list: own match, 8 propagation candidates, random trials; v_sad_u8 per pixel pair
//   pm_output_kernel    level 0 unpacked to uint8 RGB; optionally the level-0 NNF and SAD planes
#include "common.h"

#define PM_HALF 3
#define PM_MIN_SIDE 15
#define PM_MAX_SIDE 4096
#define PM_MAX_LEVELS 8
#define PM_AUTO_MIN_SIDE 32
#define PM_MAX_ITERS 64
#define PM_INIT_IT 255
#define PM_THREADS 256
#define PM_CHUNK 1024                   // pixels per block of the compaction = 4 per thread
#define PM_SCAN_THREADS 1024
#define PM_KIND_SOURCE 1
#define PM_KIND_TARGET 2

__device__ __forceinline__ uint32_t pm_fmix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

// the part of the hash that is uniform over a launch, and the draw of a pixel
__device__ __forceinline__ uint32_t pm_hash_key(uint32_t seed, int level, int it, int k) { return pm_fmix32(seed ^ pm_fmix32((uint32_t)(level * 65536 + it * 256 + k))); }
__device__ __forceinline__ uint32_t pm_hash(uint32_t key, int idx) { return pm_fmix32(key ^ (uint32_t)idx); }

// half-up mean of n >= 1 bytes per channel, packed
__device__ __forceinline__ uint32_t pm_mean(uint32_t r, uint32_t g, uint32_t b, uint32_t n) {
    return (2 * r + n) / (2 * n) | (2 * g + n) / (2 * n) << 8 | (2 * b + n) / (2 * n) << 16;
}

// ctl = (valid, start level): a level above the start, or any level of a call with nothing to fill, is skipped by every kernel
__device__ __forceinline__ bool pm_skip(const int32_t* __restrict__ ctl, int level) { return !ctl[0] || level > ctl[1]; }

__global__ void __launch_bounds__(PM_THREADS) pm_pack_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask, uint32_t* __restrict__ pix,
                                                             uint8_t* __restrict__ hole, int n) {
    const int g = blockIdx.x * PM_THREADS + threadIdx.x;
    if (g >= n) return;
    const uint8_t* p = img + (size_t)3 * g;
    pix[g] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    hole[g] = mask[g] != 0;
}

__global__ void __launch_bounds__(PM_THREADS) pm_down_kernel(const uint32_t* __restrict__ pix, const uint8_t* __restrict__ hole, int h, int w,
                                                             uint32_t* __restrict__ pix2, uint8_t* __restrict__ hole2, int h2, int w2) {
    const int g = blockIdx.x * PM_THREADS + threadIdx.x;
    if (g >= h2 * w2) return;
    const int y = g / w2, x = g - y * w2;
    uint32_t r = 0, gg = 0, b = 0, n = 0, any = 0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int q = min(2 * y + a, h - 1) * w + min(2 * x + c, w - 1);
            if (hole[q]) {
                any = 1;
            } else {
                const uint32_t v = pix[q];
                r += v & 255, gg += v >> 8 & 255, b += v >> 16 & 255, ++n;
            }
        }
    pix2[g] = n ? pm_mean(r, gg, b, n) : 0;
    hole2[g] = (uint8_t)any;
}

// a block's count of sources (low half) and targets (high half): at most 1024 each
__device__ __forceinline__ uint32_t pm_block_sum(uint32_t v, uint32_t* part) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor((int)v, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}

__global__ void __launch_bounds__(PM_THREADS) pm_classify_kernel(const uint8_t* __restrict__ hole, uint8_t* __restrict__ kind, uint32_t* __restrict__ bcnt, int h, int w) {
    __shared__ uint32_t part[PM_THREADS / 64];
    const int n = h * w, g0 = blockIdx.x * PM_CHUNK + threadIdx.x * 4;
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int g = g0 + j;
        if (g >= n) break;
        const int y = g / w, x = g - y * w;
        int k = 0;
        if (y >= PM_HALF && y < h - PM_HALF && x >= PM_HALF && x < w - PM_HALF) {
            uint32_t holes = 0;
            const uint8_t* p = hole + (y - PM_HALF) * w + (x - PM_HALF);
#pragma unroll
            for (int dy = 0; dy < 7; ++dy)
#pragma unroll
                for (int dx = 0; dx < 7; ++dx) holes |= p[dy * w + dx];
            k = holes ? PM_KIND_TARGET : PM_KIND_SOURCE;
            cnt += holes ? 1u << 16 : 1u;
        }
        kind[g] = (uint8_t)k;
    }
    const uint32_t total = pm_block_sum(cnt, part);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = total;
}

// exclusive scan of nb block counts (two int32 lanes: sources, targets) by one workgroup; lv = the level's (sources, targets)
__global__ void __launch_bounds__(PM_SCAN_THREADS) pm_scan_kernel(const uint32_t* __restrict__ bcnt, int32_t* __restrict__ boff, int nb, int32_t* __restrict__ lv) {
    __shared__ int ws[PM_SCAN_THREADS / 64], wt[PM_SCAN_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per = (nb + PM_SCAN_THREADS - 1) / PM_SCAN_THREADS, b0 = min(t * per, nb), b1 = min(b0 + per, nb);
    int s = 0, g = 0;
    for (int b = b0; b < b1; ++b) s += (int)(bcnt[b] & 0xFFFF), g += (int)(bcnt[b] >> 16);
    int is = s, ig = g;                                    // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int us = __shfl_up(is, o, 64), ug = __shfl_up(ig, o, 64);
        if (lane >= o) is += us, ig += ug;
    }
    if (lane == 63) ws[wave] = is, wt[wave] = ig;
    __syncthreads();
    int os = 0, og = 0, ts = 0, tg = 0;
#pragma unroll
    for (int v = 0; v < PM_SCAN_THREADS / 64; ++v) {
        if (v < wave) os += ws[v], og += wt[v];
        ts += ws[v], tg += wt[v];
    }
    os += is - s, og += ig - g;
    for (int b = b0; b < b1; ++b) {
        boff[2 * b] = os, boff[2 * b + 1] = og;
        os += (int)(bcnt[b] & 0xFFFF), og += (int)(bcnt[b] >> 16);
    }
    if (t == 0) lv[0] = ts, lv[1] = tg;
}

__global__ void __launch_bounds__(PM_THREADS) pm_compact_kernel(const uint8_t* __restrict__ kind, const int32_t* __restrict__ boff, uint32_t* __restrict__ src,
                                                                uint32_t* __restrict__ tgt, int h, int w) {
    __shared__ uint32_t part[PM_THREADS / 64];
    const int n = h * w, g0 = blockIdx.x * PM_CHUNK + threadIdx.x * 4, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int k[4];
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        k[j] = g0 + j < n ? kind[g0 + j] : 0;
        cnt += k[j] == PM_KIND_SOURCE ? 1u : k[j] == PM_KIND_TARGET ? 1u << 16 : 0u;
    }
    uint32_t inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)inc, o, 64);
        if (lane >= o) inc += u;
    }
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    uint32_t ex = inc - cnt;
#pragma unroll
    for (int v = 0; v < PM_THREADS / 64; ++v)
        if (v < wave) ex += part[v];
    int os = boff[2 * blockIdx.x] + (int)(ex & 0xFFFF), og = boff[2 * blockIdx.x + 1] + (int)(ex >> 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int g = g0 + j, y = g / w, x = g - y * w;
        if (k[j] == PM_KIND_SOURCE) src[os++] = (uint32_t)y << 16 | (uint32_t)x;
        if (k[j] == PM_KIND_TARGET) tgt[og++] = (uint32_t)y << 16 | (uint32_t)x;
    }
}

// lv = (sources, targets) per level.  valid: level 0 has a source and a target (a hole pixel always lies in an interior box); the start level is
// the coarsest one with a source (every finer one then has one too)
__global__ void pm_decide_kernel(const int32_t* __restrict__ lv, int nlev, int32_t* __restrict__ ctl, int32_t* __restrict__ info) {
    if (threadIdx.x || blockIdx.x) return;
    const int valid = lv[0] > 0 && lv[1] > 0;
    int start = 0;
    for (int l = 0; l < nlev; ++l)
        if (lv[2 * l] > 0) start = l;
    if (!valid) start = 0;
    ctl[0] = valid, ctl[1] = start;
    info[0] = valid, info[1] = start, info[2] = lv[0], info[3] = lv[1];
}

__global__ void __launch_bounds__(PM_THREADS) pm_init_kernel(const uint32_t* __restrict__ tgt, const uint32_t* __restrict__ src, const uint8_t* __restrict__ kind,
                                                             uint32_t* __restrict__ nnf, const int32_t* __restrict__ lv, const int32_t* __restrict__ ctl, int level,
                                                             const uint32_t* __restrict__ nnf_c, const uint8_t* __restrict__ kind_c, int hc, int wc, int h, int w, uint32_t seed) {
    if (pm_skip(ctl, level)) return;
    const int i = blockIdx.x * PM_THREADS + threadIdx.x;
    if (i >= lv[2 * level + 1]) return;
    const uint32_t p = tgt[i];
    const int py = (int)(p >> 16), px = (int)(p & 0xFFFF), g = py * w + px;
    if (level < ctl[1]) {                                  // a coarser level ran: its match, doubled
        const int cy = min(max(py >> 1, PM_HALF), hc - 1 - PM_HALF), cx = min(max(px >> 1, PM_HALF), wc - 1 - PM_HALF);
        if (kind_c[cy * wc + cx] == PM_KIND_TARGET) {
            const uint32_t c = nnf_c[cy * wc + cx];
            const int qy = min(max(2 * (int)(c >> 16) + (py & 1), PM_HALF), h - 1 - PM_HALF), qx = min(max(2 * (int)(c & 0xFFFF) + (px & 1), PM_HALF), w - 1 - PM_HALF);
            if (kind[qy * w + qx] == PM_KIND_SOURCE) {
                nnf[g] = (uint32_t)qy << 16 | (uint32_t)qx;
                return;
            }
        }
    }
    nnf[g] = src[pm_hash(pm_hash_key(seed, level, PM_INIT_IT, 0), g) % (uint32_t)lv[2 * level]];
}

// one thread per pixel of the level; a hole pixel x gathers, over the interior centres p = x + d with |d| <= 3 (each holds x in its box, so
// each is a target), the pixel at NNF(p) - d: a pixel of a source patch, wholly known, so nothing read here is written here
__global__ void __launch_bounds__(PM_THREADS) pm_vote_kernel(uint32_t* __restrict__ pix, const uint8_t* __restrict__ hole, const uint32_t* __restrict__ nnf,
                                                             const int32_t* __restrict__ ctl, int level, int h, int w) {
    if (pm_skip(ctl, level)) return;
    const int g = blockIdx.x * PM_THREADS + threadIdx.x;
    if (g >= h * w || !hole[g]) return;
    const int y = g / w, x = g - y * w;
    uint32_t r = 0, gg = 0, b = 0, n = 0;
    const int y0 = max(y - PM_HALF, PM_HALF), y1 = min(y + PM_HALF, h - 1 - PM_HALF), x0 = max(x - PM_HALF, PM_HALF), x1 = min(x + PM_HALF, w - 1 - PM_HALF);
    for (int py = y0; py <= y1; ++py)
        for (int px = x0; px <= x1; ++px) {
            const uint32_t q = nnf[py * w + px];
            const uint32_t v = pix[((int)(q >> 16) - (py - y)) * w + (int)(q & 0xFFFF) - (px - x)];
            r += v & 255, gg += v >> 8 & 255, b += v >> 16 & 255, ++n;
        }
    pix[g] = pm_mean(r, gg, b, n);
}

// D(p, q) against the target patch in registers; stops after a row once the sum has reached `bound` (such a candidate cannot replace the best)
__device__ __forceinline__ uint32_t pm_sad(const uint32_t (&tp)[49], const uint32_t* __restrict__ pix, int w, int qy, int qx, uint32_t bound) {
    const uint32_t* r = pix + (qy - PM_HALF) * w + (qx - PM_HALF);
    uint32_t acc = 0;
#pragma unroll
    for (int dy = 0; dy < 7; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 7; ++dx) acc = __builtin_amdgcn_sad_u8(tp[dy * 7 + dx], r[dx], acc);
        if (acc >= bound) return acc;
        r += w;
    }
    return acc;
}

__global__ void __launch_bounds__(PM_THREADS) pm_sweep_kernel(const uint32_t* __restrict__ pix, const uint8_t* __restrict__ kind, const uint32_t* __restrict__ tgt,
                                                              const uint32_t* __restrict__ nnf_in, uint32_t* __restrict__ nnf_out, uint32_t* __restrict__ cost,
                                                              const int32_t* __restrict__ lv, const int32_t* __restrict__ ctl, int level, int it, uint32_t seed, int h, int w) {
    if (pm_skip(ctl, level)) return;
    const int i = blockIdx.x * PM_THREADS + threadIdx.x;
    if (i >= lv[2 * level + 1]) return;
    const uint32_t p = tgt[i];
    const int py = (int)(p >> 16), px = (int)(p & 0xFFFF), g = py * w + px;
    uint32_t tp[49];
    {
        const uint32_t* r = pix + (py - PM_HALF) * w + (px - PM_HALF);
#pragma unroll
        for (int dy = 0; dy < 7; ++dy)
#pragma unroll
            for (int dx = 0; dx < 7; ++dx) tp[dy * 7 + dx] = r[dy * w + dx];
    }
    uint32_t best = nnf_in[g];
    uint32_t bc = pm_sad(tp, pix, w, (int)(best >> 16), (int)(best & 0xFFFF), 0xFFFFFFFFu);
    // a candidate counts only if it is a source (the kind plane is 0 outside the interior); strict <: the earlier candidate wins a tie
#define PM_TRY(cy_, cx_)                                                                          \
    do {                                                                                          \
        const int cy = (cy_), cx = (cx_);                                                         \
        if (cy >= 0 && cy < h && cx >= 0 && cx < w && kind[cy * w + cx] == PM_KIND_SOURCE) {      \
            const uint32_t d_ = pm_sad(tp, pix, w, cy, cx, bc);                                   \
            if (d_ < bc) bc = d_, best = (uint32_t)cy << 16 | (uint32_t)cx;                       \
        }                                                                                         \
    } while (0)
    for (int j = 0; j < 2; ++j) {
        const int s = j ? 1 << (1 + it % 3) : 1;
        for (int d = 0; d < 4; ++d) {
            const int dy = d == 2 ? -s : d == 3 ? s : 0, dx = d == 0 ? -s : d == 1 ? s : 0;
            const int ny = py + dy, nx = px + dx;
            if (ny < 0 || ny >= h || nx < 0 || nx >= w || kind[ny * w + nx] != PM_KIND_TARGET) continue;
            const uint32_t c = nnf_in[ny * w + nx];
            PM_TRY((int)(c >> 16) - dy, (int)(c & 0xFFFF) - dx);
        }
    }
    int k = 0;
    for (int R = max(h, w); R >= 1; R >>= 1, ++k) {
        const uint32_t r = pm_hash(pm_hash_key(seed, level, it, k), g), m = 2 * (uint32_t)R + 1;
        PM_TRY((int)(best >> 16) + (int)((r & 0xFFFF) % m) - R, (int)(best & 0xFFFF) + (int)((r >> 16) % m) - R);
    }
#undef PM_TRY
    nnf_out[g] = best;
    cost[g] = bc;
}

__global__ void __launch_bounds__(PM_THREADS) pm_output_kernel(const uint32_t* __restrict__ pix, const uint8_t* __restrict__ kind, const uint32_t* __restrict__ nnf,
                                                               const uint32_t* __restrict__ cost, const int32_t* __restrict__ ctl, int have_cost, uint8_t* __restrict__ out,
                                                               int32_t* __restrict__ nnf_out, int32_t* __restrict__ sad_out, int n) {
    const int g = blockIdx.x * PM_THREADS + threadIdx.x;
    if (g >= n) return;
    const uint32_t v = pix[g];
    uint8_t* o = out + (size_t)3 * g;
    o[0] = (uint8_t)v, o[1] = (uint8_t)(v >> 8), o[2] = (uint8_t)(v >> 16);
    const bool t = ctl[0] && kind[g] == PM_KIND_TARGET;
    if (nnf_out) {
        const uint32_t q = t ? nnf[g] : 0;
        nnf_out[2 * (size_t)g] = t ? (int32_t)(q >> 16) : -1;
        nnf_out[2 * (size_t)g + 1] = t ? (int32_t)(q & 0xFFFF) : -1;
    }
    if (sad_out) sad_out[g] = t && have_cost ? (int32_t)cost[g] : -1;
}

// workspace layout, every region rounded up to 16 bytes.  Per level: pix uint32 [h, w]; hole, kind uint8 [h, w]; src, tgt uint32 [(h - 6)(w - 6)];
// nnf uint32 2 x [h, w]; cost uint32 [h, w]; bcnt uint32 [nb]; boff int32 [nb, 2].  Then lv int32 [8, 2] and ctl int32 [2].
struct pm_level {
    int h, w, nb;
    int64_t pix, hole, kind, src, tgt, nnf[2], cost, bcnt, boff;
};
struct pm_layout {
    int nlev;
    pm_level lv[PM_MAX_LEVELS];
    int64_t lvinfo, ctl, total;
};

static bool pm_plan(int H, int W, int levels, pm_layout& L) {
    if (H < PM_MIN_SIDE || W < PM_MIN_SIDE || H > PM_MAX_SIDE || W > PM_MAX_SIDE || levels < 0 || levels > PM_MAX_LEVELS) return false;
    const int floor = levels ? PM_MIN_SIDE : PM_AUTO_MIN_SIDE, want = levels ? levels : PM_MAX_LEVELS;
    int64_t at = 0;
    auto take = [&](int64_t bytes) { const int64_t o = at; at += (bytes + 15) & ~(int64_t)15; return o; };
    int h = H, w = W, n = 0;
    for (;;) {
        pm_level& v = L.lv[n++];
        const int64_t px = (int64_t)h * w, in = (int64_t)(h - 6) * (w - 6);
        v.h = h, v.w = w, v.nb = (int)((px + PM_CHUNK - 1) / PM_CHUNK);
        v.pix = take(4 * px), v.hole = take(px), v.kind = take(px), v.src = take(4 * in), v.tgt = take(4 * in);
        v.nnf[0] = take(4 * px), v.nnf[1] = take(4 * px), v.cost = take(4 * px), v.bcnt = take(4 * (int64_t)v.nb), v.boff = take(8 * (int64_t)v.nb);
        if (n >= want || min((h + 1) / 2, (w + 1) / 2) < floor) break;
        h = (h + 1) / 2, w = (w + 1) / 2;
    }
    L.nlev = n;
    L.lvinfo = take(8 * PM_MAX_LEVELS);
    L.ctl = take(8);
    L.total = at;
    return true;
}

static bool pm_overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

extern "C" int st_patchmatch_levels(int32_t H, int32_t W, int32_t levels) {
    pm_layout L;
    return pm_plan(H, W, levels, L) ? L.nlev : 0;
}

extern "C" int st_patchmatch_workspace_bytes(int32_t H, int32_t W, int32_t levels) {
    pm_layout L;
    return pm_plan(H, W, levels, L) ? (int)L.total : 0;
}

extern "C" int st_patchmatch_fill(const uint8_t* img, const uint8_t* mask, int32_t H, int32_t W, int32_t levels, int32_t iters, int32_t seed, uint8_t* out,
                                  int32_t* info_out, int32_t* nnf_out, int32_t* sad_out, void* workspace, int64_t workspace_bytes, void* stream) {
    pm_layout L;
    if (!img || !mask || !out || !info_out || !workspace || !pm_plan(H, W, levels, L)) return ST_EINVAL;
    if (iters < 0 || iters > PM_MAX_ITERS || workspace_bytes < L.total || ((uintptr_t)workspace & 15)) return ST_EINVAL;
    const int64_t n = (int64_t)H * W;
    // an output overlaps nothing: no input (out may not alias img: the kernels between read img first, but the contract stays simple), no other
    // output, not the workspace; no input lies in the workspace
    const void* outs[4] = {out, info_out, nnf_out, sad_out};
    const int64_t out_bytes[4] = {3 * n, 16, 8 * n, 4 * n};
    const void* ins[2] = {img, mask};
    const int64_t in_bytes[2] = {3 * n, n};
    for (int i = 0; i < 4; ++i) {
        if (!outs[i]) continue;
        for (int j = 0; j < 2; ++j)
            if (pm_overlap(outs[i], out_bytes[i], ins[j], in_bytes[j])) return ST_EINVAL;
        for (int j = i + 1; j < 4; ++j)
            if (outs[j] && pm_overlap(outs[i], out_bytes[i], outs[j], out_bytes[j])) return ST_EINVAL;
        if (pm_overlap(outs[i], out_bytes[i], workspace, L.total)) return ST_EINVAL;
    }
    for (int j = 0; j < 2; ++j)
        if (pm_overlap(ins[j], in_bytes[j], workspace, L.total)) return ST_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int32_t* lvinfo = (int32_t*)(ws + L.lvinfo);
    int32_t* ctl = (int32_t*)(ws + L.ctl);
    auto blocks = [](int64_t items) { return (unsigned)((items + PM_THREADS - 1) / PM_THREADS); };
#define PM_AT(T, l, field) ((T*)(ws + L.lv[l].field))
    pm_pack_kernel<<<blocks(n), PM_THREADS, 0, s>>>(img, mask, PM_AT(uint32_t, 0, pix), PM_AT(uint8_t, 0, hole), (int)n);
    ST_CHECK_LAUNCH();
    for (int l = 0; l < L.nlev; ++l) {
        const pm_level& v = L.lv[l];
        if (l) {
            const pm_level& f = L.lv[l - 1];
            pm_down_kernel<<<blocks((int64_t)v.h * v.w), PM_THREADS, 0, s>>>(PM_AT(uint32_t, l - 1, pix), PM_AT(uint8_t, l - 1, hole), f.h, f.w, PM_AT(uint32_t, l, pix),
                                                                             PM_AT(uint8_t, l, hole), v.h, v.w);
            ST_CHECK_LAUNCH();
        }
        pm_classify_kernel<<<v.nb, PM_THREADS, 0, s>>>(PM_AT(uint8_t, l, hole), PM_AT(uint8_t, l, kind), PM_AT(uint32_t, l, bcnt), v.h, v.w);
        ST_CHECK_LAUNCH();
        pm_scan_kernel<<<1, PM_SCAN_THREADS, 0, s>>>(PM_AT(uint32_t, l, bcnt), PM_AT(int32_t, l, boff), v.nb, lvinfo + 2 * l);
        ST_CHECK_LAUNCH();
        pm_compact_kernel<<<v.nb, PM_THREADS, 0, s>>>(PM_AT(uint8_t, l, kind), PM_AT(int32_t, l, boff), PM_AT(uint32_t, l, src), PM_AT(uint32_t, l, tgt), v.h, v.w);
        ST_CHECK_LAUNCH();
    }
    pm_decide_kernel<<<1, 64, 0, s>>>(lvinfo, L.nlev, ctl, info_out);
    ST_CHECK_LAUNCH();
    const int last = iters & 1;                            // the buffer a level's final NNF lies in: init writes 0, sweep `it` reads it & 1
    for (int l = L.nlev - 1; l >= 0; --l) {
        const pm_level& v = L.lv[l];
        const bool top = l == L.nlev - 1;
        const pm_level& c = L.lv[top ? l : l + 1];
        const unsigned tb = blocks((int64_t)(v.h - 6) * (v.w - 6)), pb = blocks((int64_t)v.h * v.w);
        pm_init_kernel<<<tb, PM_THREADS, 0, s>>>(PM_AT(uint32_t, l, tgt), PM_AT(uint32_t, l, src), PM_AT(uint8_t, l, kind), PM_AT(uint32_t, l, nnf[0]), lvinfo, ctl, l,
                                                 top ? nullptr : (const uint32_t*)(ws + c.nnf[last]), top ? nullptr : (const uint8_t*)(ws + c.kind), c.h, c.w, v.h, v.w,
                                                 (uint32_t)seed);
        ST_CHECK_LAUNCH();
        pm_vote_kernel<<<pb, PM_THREADS, 0, s>>>(PM_AT(uint32_t, l, pix), PM_AT(uint8_t, l, hole), PM_AT(uint32_t, l, nnf[0]), ctl, l, v.h, v.w);
        ST_CHECK_LAUNCH();
        for (int it = 0; it < iters; ++it) {
            pm_sweep_kernel<<<tb, PM_THREADS, 0, s>>>(PM_AT(uint32_t, l, pix), PM_AT(uint8_t, l, kind), PM_AT(uint32_t, l, tgt), PM_AT(uint32_t, l, nnf[it & 1]),
                                                      PM_AT(uint32_t, l, nnf[(it + 1) & 1]), PM_AT(uint32_t, l, cost), lvinfo, ctl, l, it, (uint32_t)seed, v.h, v.w);
            ST_CHECK_LAUNCH();
            pm_vote_kernel<<<pb, PM_THREADS, 0, s>>>(PM_AT(uint32_t, l, pix), PM_AT(uint8_t, l, hole), PM_AT(uint32_t, l, nnf[(it + 1) & 1]), ctl, l, v.h, v.w);
            ST_CHECK_LAUNCH();
        }
    }
    pm_output_kernel<<<blocks(n), PM_THREADS, 0, s>>>(PM_AT(uint32_t, 0, pix), PM_AT(uint8_t, 0, kind), PM_AT(uint32_t, 0, nnf[last]), PM_AT(uint32_t, 0, cost), ctl,
                                                      iters > 0, out, nnf_out, sad_out, (int)n);
    ST_CHECK_LAUNCH();
#undef PM_AT
    return ST_OK;
}
