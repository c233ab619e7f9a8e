// seam_dp: a minimum-difference seam through the overlap of two warped images, for the ownership of multiband_blend (contract in
// README.md, "seam_dp"; CPU restatement tests/_seam_ref.py).  gfx950 only.  Everything is integers.  Every kernel of a call goes to the
// caller's stream, in order, inside the caller's workspace: no host synchronisation, no allocation, no memset / memcpy, no atomics (every
// word has exactly one writer), and the launch count and every grid depend on H and W alone -- the orientation is decided on the device --
// so a call captures into a hipGraph as a linear chain.
//
//   seam_stats_kernel      per workgroup of 4096 pixels: |E1|, |E2|, |O| and the coordinate sums of E1 and E2, uint32
//   seam_decide_kernel     the sum of the records in int64, A and B, info = (valid, orientation, first, -)
//   seam_cost_kernel       e per pixel, written line-major for the decided orientation (32 x 32 tiles, transposed through LDS)
//   seam_dp_kernel         one workgroup walks the lines: four positions per thread in registers, edge values through LDS, one barrier
//                          per line; predecessor codes as bytes; the argmin of the last line
//   seam_backtrack_kernel  one workgroup: per chunk of 64 lines one lane walks a window of codes in LDS while three waves load the next one
//   seam_side_kernel       side per canvas pixel, four pixels per thread
#include "common.h"
#include <algorithm>

#define SM_MAX_SIDE 4096
#define SM_BIG (1 << 18)
#define SM_INF 0x7fffffff
#define SM_AUTO 0
#define SM_VERTICAL 1                   // lines are rows, a position is a column
#define SM_HORIZONTAL 2                 // lines are columns, a position is a row
#define SM_STAT_WORDS 7                 // N1, N2, NO, Sx1, Sy1, Sx2, Sy2
#define SM_STAT_PIXELS 4096             // pixels per workgroup of the statistics: a coordinate sum stays below 4096 * 4095 < 2^24
#define SM_PER 4                        // positions per thread of the DP
#define SM_CHUNK 64                     // lines per backtrack chunk

__device__ __forceinline__ int sm_stride(int n) { return (n + 3) & ~3; }      // a line of costs / codes: padded to 16 / 4 bytes

__device__ __forceinline__ uint32_t sm_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

__device__ __forceinline__ unsigned long long sm_shfl_xor64(unsigned long long v, int o) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    return (unsigned long long)hi << 32 | lo;
}

// ---- 1: region statistics.  256 threads, 16 pixels each (coalesced: pixel = base + j * 256 + thread), one storing lane.
__global__ void __launch_bounds__(256) seam_stats_kernel(const float* __restrict__ mask1, const float* __restrict__ mask2, uint32_t* __restrict__ records,
                                                         int W, int n) {
    __shared__ uint32_t part[4][SM_STAT_WORDS];
    uint32_t acc[SM_STAT_WORDS];
#pragma unroll
    for (int k = 0; k < SM_STAT_WORDS; ++k) acc[k] = 0;
    const int base = blockIdx.x * SM_STAT_PIXELS + threadIdx.x;
#pragma unroll 4
    for (int j = 0; j < SM_STAT_PIXELS / 256; ++j) {
        const int p = base + j * 256;
        if (p >= n) break;
        const bool a = mask1[p] > 0.5f, b = mask2[p] > 0.5f;
        const uint32_t y = (uint32_t)(p / W), x = (uint32_t)p - y * (uint32_t)W;
        const bool e1 = a && !b, e2 = b && !a;
        acc[0] += e1; acc[1] += e2; acc[2] += a && b;
        acc[3] += e1 ? x : 0u; acc[4] += e1 ? y : 0u;
        acc[5] += e2 ? x : 0u; acc[6] += e2 ? y : 0u;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < SM_STAT_WORDS; ++k) {
        const uint32_t s = sm_wave_sum(acc[k]);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t* rec = records + (size_t)blockIdx.x * SM_STAT_WORDS;
#pragma unroll
        for (int k = 0; k < SM_STAT_WORDS; ++k) rec[k] = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
    }
}

// ---- 2: decide.  One workgroup; info[0..2] = valid, orientation, first (info[3], the path cost, is the DP's word).
__global__ void __launch_bounds__(1024) seam_decide_kernel(const uint32_t* __restrict__ records, int groups, int orientation, int first, int32_t* __restrict__ info) {
    __shared__ unsigned long long part[16][SM_STAT_WORDS];
    unsigned long long acc[SM_STAT_WORDS];
#pragma unroll
    for (int k = 0; k < SM_STAT_WORDS; ++k) acc[k] = 0;
    for (int g = threadIdx.x; g < groups; g += 1024) {
#pragma unroll
        for (int k = 0; k < SM_STAT_WORDS; ++k) acc[k] += records[(size_t)g * SM_STAT_WORDS + k];
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < SM_STAT_WORDS; ++k) {
        unsigned long long s = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += sm_shfl_xor64(s, o);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t[SM_STAT_WORDS];
        for (int k = 0; k < SM_STAT_WORDS; ++k) {
            unsigned long long s = 0;
            for (int w = 0; w < 16; ++w) s += part[w][k];
            t[k] = (long long)s;
        }
        const long long N1 = t[0], N2 = t[1], NO = t[2];
        const long long A = t[3] * N2 - t[5] * N1, B = t[4] * N2 - t[6] * N1;             // below 2^36 * 2^24
        const long long absA = A < 0 ? -A : A, absB = B < 0 ? -B : B;
        const int orient = orientation != SM_AUTO ? orientation : (absA >= absB ? SM_VERTICAL : SM_HORIZONTAL);
        const int fst = first != SM_AUTO ? first : ((orient == SM_VERTICAL ? A : B) <= 0 ? 1 : 2);
        const bool automatic = orientation == SM_AUTO || first == SM_AUTO;
        info[0] = NO != 0 && !(automatic && (N1 == 0 || N2 == 0));
        info[1] = orient;
        info[2] = fst;
    }
}

// ---- 3: cost.  A 32 x 32 canvas tile per workgroup of 256 threads; reads are row-major, the store is line-major for the orientation in
// info (through an LDS transpose for column lines).  info == NULL: canvas layout [H, W] (st_seam_cost).
__device__ __forceinline__ int sm_absdiff(float a, float b) {
    const int d = (int)st_u8_trunc(a) - (int)st_u8_trunc(b);
    return d < 0 ? -d : d;
}

__global__ void __launch_bounds__(256) seam_cost_kernel(const float* __restrict__ img1, const float* __restrict__ img2, const float* __restrict__ mask1,
                                                        const float* __restrict__ mask2, const int32_t* __restrict__ info, int32_t* __restrict__ cost,
                                                        int H, int W) {
    __shared__ int32_t tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 32;
    const size_t n = (size_t)H * W;
    const bool columns = info && info[1] == SM_HORIZONTAL;
    const int stride = info ? sm_stride(columns ? H : W) : W;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int yy = ty + r * 8, y = y0 + yy, x = x0 + tx;
        int e = 0;
        if (y < H && x < W) {
            const size_t p = (size_t)y * W + x;
            const bool a = mask1[p] > 0.5f, b = mask2[p] > 0.5f;
            if (a && b) e = 1 + sm_absdiff(img1[p], img2[p]) + sm_absdiff(img1[n + p], img2[n + p]) + sm_absdiff(img1[2 * n + p], img2[2 * n + p]);
            else e = (a || b) ? SM_BIG : 1;
            if (!columns) cost[(size_t)y * stride + x] = e;
        }
        tile[yy][tx] = e;
    }
    if (!columns) return;                   // (uniform over the grid)
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int xx = ty + r * 8, x = x0 + xx, y = y0 + tx;
        if (x < W && y < H) cost[(size_t)x * stride + y] = tile[tx][xx];
    }
}

// ---- 4: the DP.  One workgroup of `blockDim.x` >= ceil(n / 4) threads; thread t owns positions 4 t .. 4 t + 3 of every line in registers.
// Per line: one barrier, then every thread reads its neighbours' edge values from LDS, takes per position the minimum of the predecessors
// k, k - 1, k + 1 and publishes its own two new edge values for the next line (two buffers, by line parity: a buffer is written again only
// after the barrier that follows its last read).  The predecessor codes -- k, k - 1, k + 1 in that order with strict < -- are worked out
// after that, off the chain.  Positions outside the line hold SM_INF and are never added to; a real value is at most 4096 * 2^18 = 2^30.
// Costs are prefetched four lines ahead as one 16-byte load per line; codes go out as one 4-byte store per line; neither is waited for at
// the barrier.

// a workgroup barrier that orders LDS traffic alone: it waits for this wave's LDS operations, not for its global loads and stores, so the
// prefetched costs and the code stores stay in flight across it (__syncthreads() would drain them on every line)
__device__ __forceinline__ void sm_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ int4 sm_load_costs(const int32_t* __restrict__ cost, int line, int stride, int k0) {
    return *reinterpret_cast<const int4*>(cost + (size_t)line * stride + k0);
}

__global__ void __launch_bounds__(1024) seam_dp_kernel(const int32_t* __restrict__ cost, uint8_t* __restrict__ codes, int32_t* __restrict__ info,
                                                       int32_t* __restrict__ end, int H, int W) {
    __shared__ int32_t edge_lo[2][1024 + 1], edge_hi[2][1 + 1024];   // edge_lo[.][t]: thread t's position 0; edge_hi[.][1 + t]: its position 3
    __shared__ unsigned long long best_key[16];
    const bool columns = info[1] == SM_HORIZONTAL;
    const int L = columns ? W : H, n = columns ? H : W, stride = sm_stride(n);
    const int t = threadIdx.x, k0 = t * SM_PER;
    const bool holds = k0 < stride;                                  // this thread's 16 bytes lie inside the line
    const int kl = holds ? k0 : 0;                                   // (a thread past the line loads position 0 and drops it)
    bool in[SM_PER];
#pragma unroll
    for (int j = 0; j < SM_PER; ++j) in[j] = k0 + j < n;
    int m[SM_PER];
    {
        const int4 c = sm_load_costs(cost, 0, stride, kl);
        m[0] = in[0] ? c.x : SM_INF; m[1] = in[1] ? c.y : SM_INF; m[2] = in[2] ? c.z : SM_INF; m[3] = in[3] ? c.w : SM_INF;
    }
    if (t == 0) {                                                    // what lies left of the first and right of the last thread, never written again
        edge_hi[0][0] = edge_hi[1][0] = SM_INF;
        edge_lo[0][blockDim.x] = edge_lo[1][blockDim.x] = SM_INF;
    }
    edge_lo[1][t] = m[0];                                            // line 1 reads buffer 1
    edge_hi[1][1 + t] = m[SM_PER - 1];
    int4 cur[4], nxt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) cur[j] = sm_load_costs(cost, min(1 + j, L - 1), stride, kl);
    for (int l0 = 1; l0 < L; l0 += 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) nxt[j] = sm_load_costs(cost, min(l0 + 4 + j, L - 1), stride, kl);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int l = l0 + j;
            if (l >= L) break;                                       // (uniform over the workgroup)
            const int buf = l & 1;
            sm_lds_barrier();
            int prev[SM_PER + 2];
            prev[0] = edge_hi[buf][t];
            prev[SM_PER + 1] = edge_lo[buf][t + 1];
#pragma unroll
            for (int i = 0; i < SM_PER; ++i) prev[1 + i] = m[i];
            // the chain from line to line is short: the new values (the minimum is the same in any order) and their edges, published for
            // the next line at once; the codes, which need the order of the contract, follow while those LDS stores are under way
            const int c[SM_PER] = {cur[j].x, cur[j].y, cur[j].z, cur[j].w};
#pragma unroll
            for (int i = 0; i < SM_PER; ++i) m[i] = in[i] ? c[i] + min(min(prev[i], prev[1 + i]), prev[2 + i]) : SM_INF;
            edge_lo[buf ^ 1][t] = m[0];
            edge_hi[buf ^ 1][1 + t] = m[SM_PER - 1];
            uint32_t word = 0;
#pragma unroll
            for (int i = 0; i < SM_PER; ++i) {
                int best = prev[1 + i];
                uint32_t code = 0;
                if (prev[i] < best) { best = prev[i]; code = 1; }
                if (prev[2 + i] < best) code = 2;
                word |= code << (8 * i);
            }
            if (holds) *reinterpret_cast<uint32_t*>(codes + (size_t)l * stride + k0) = word;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
    }
    // the lowest index among the minima of the last line: the smallest key value << 12 | position
    unsigned long long key = ~0ull;
#pragma unroll
    for (int i = SM_PER - 1; i >= 0; --i)
        if (in[i]) key = min(key, (unsigned long long)(uint32_t)m[i] << 12 | (unsigned long long)(k0 + i));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = min(key, sm_shfl_xor64(key, o));
    if ((t & 63) == 0) best_key[t >> 6] = key;
    __syncthreads();
    if (t == 0) {
        const int waves = (blockDim.x + 63) >> 6;
        for (int w = 1; w < waves; ++w) key = min(key, best_key[w]);
        end[0] = (int32_t)(key & 4095);
        info[3] = (int32_t)(key >> 12);
    }
}

// ---- 5: backtrack.  One workgroup of 256 threads.  codes[l][k] names the predecessor of (l, k) in line l - 1, so the path moves at most
// one position per line: a chunk of 64 lines that starts at position k stays inside k - 63 .. k + 63.  From the last line up, per chunk:
// lane 0 walks the chunk's window of codes in LDS while waves 1-3 load the next chunk's window into the other buffer.  That window is
// centred on the position the current chunk starts from, which the next chunk's start is within 64 of, so it is 4 * 64 + 8 bytes wide: 66
// aligned words per line from base = (centre - 128) rounded down to 4, which cover every position the next walk can reach (centre - 127 ..
// centre + 127).  Then all threads store the chunk's 64 positions.  path [max(H, W)]: s[l], -1 past the last line.  Finally info is
// copied to the caller.
#define SM_WIN_WORDS (SM_CHUNK + 2)

__device__ __forceinline__ int sm_win_base(int centre) { return (centre - 2 * SM_CHUNK) & ~3; }       // (two's complement: rounds down below 0 too)

// rows r = 0 .. SM_CHUNK - 1 of the window = lines top - r; lines below 1 (line 0 has no predecessor) and words outside the line read 0
__device__ __forceinline__ void sm_load_window(const uint8_t* __restrict__ codes, uint32_t (*win)[SM_WIN_WORDS], int top, int centre, int stride, int i0, int step) {
    const int base = sm_win_base(centre);
    for (int i = i0; i < SM_CHUNK * SM_WIN_WORDS; i += step) {
        const int r = i / SM_WIN_WORDS, w = i - r * SM_WIN_WORDS, line = top - r, p = base + 4 * w;
        win[r][w] = (line >= 1 && p >= 0 && p + 3 < stride) ? *reinterpret_cast<const uint32_t*>(codes + (size_t)line * stride + p) : 0u;
    }
}

__global__ void __launch_bounds__(256) seam_backtrack_kernel(const uint8_t* __restrict__ codes, const int32_t* __restrict__ info, const int32_t* __restrict__ end,
                                                             int32_t* __restrict__ path, int32_t* __restrict__ path_out, int32_t* __restrict__ info_out,
                                                             int H, int W) {
    __shared__ uint32_t win[2][SM_CHUNK][SM_WIN_WORDS];
    __shared__ int32_t walked[SM_CHUNK];
    __shared__ int32_t at;
    const bool columns = info[1] == SM_HORIZONTAL;
    const int L = columns ? W : H, n = columns ? H : W, stride = sm_stride(n);
    const int t = threadIdx.x;
    for (int l = L + t; l < max(H, W); l += 256) {
        path[l] = -1;
        if (path_out) path_out[l] = -1;
    }
    int k_start = end[0], centre = k_start;                            // (uniform over the workgroup, as L and every `top` are)
    sm_load_window(codes, win[0], L - 1, centre, stride, t, 256);
    __syncthreads();
    for (int top = L - 1, b = 0; top >= 0; top -= SM_CHUNK, b ^= 1) {
        const int cnt = min(SM_CHUNK, top + 1);
        if (t == 0) {
            const uint8_t* bytes = reinterpret_cast<const uint8_t*>(&win[b][0][0]);
            const int base = sm_win_base(centre);
            int k = k_start;
            for (int r = 0; r < cnt; ++r) {
                walked[r] = k;
                const int code = bytes[r * (4 * SM_WIN_WORDS) + (k - base)];       // k - base is in 1 .. 258
                k += code == 1 ? -1 : code == 2 ? 1 : 0;
            }
            at = k;
        } else if (t >= 64 && top - SM_CHUNK >= 0) {
            sm_load_window(codes, win[b ^ 1], top - SM_CHUNK, k_start, stride, t - 64, 192);
        }
        __syncthreads();
        if (t < cnt) {
            path[top - t] = walked[t];
            if (path_out) path_out[top - t] = walked[t];
        }
        centre = k_start;
        k_start = at;
        __syncthreads();                                               // walked and at are written again by the next chunk
    }
    if (t < 4) info_out[t] = info[t];
}

// ---- 6: side.  side(p) = 1 iff (position of p <= s[line of p]) == (first == 1); all ones without a valid seam.  Four pixels per thread,
// stored as one word where the plane allows it.
__global__ void __launch_bounds__(256) seam_side_kernel(const int32_t* __restrict__ info, const int32_t* __restrict__ path, uint8_t* __restrict__ side,
                                                        int W, int n, int words_ok) {
    const int p0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= n) return;
    const bool valid = info[0] != 0, columns = info[1] == SM_HORIZONTAL, low1 = info[2] == 1;
    uint32_t word = 0;
    uint8_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = min(p0 + j, n - 1), y = p / W, x = p - y * W;
        const int pos = columns ? y : x, line = columns ? x : y;
        v[j] = !valid || ((pos <= path[line]) == low1);
        word |= (uint32_t)v[j] << (8 * j);
    }
    if (words_ok && p0 + 3 < n) *reinterpret_cast<uint32_t*>(side + p0) = word;
    else
        for (int j = 0; j < 4 && p0 + j < n; ++j) side[p0 + j] = v[j];
}

// workspace layout: records uint32 [groups, 7]; info int32 [4]; end int32 [1]; path int32 [max(H, W)]; cost int32 [lines, stride]; codes
// uint8 [lines, stride] -- the last two sized for the larger of the two orientations, each region rounded up to 16 bytes
struct sm_layout {
    int groups;
    int64_t records, info, end, path, cost, codes, total;
};

static bool sm_plan(int H, int W, sm_layout& L) {
    if (H < 1 || W < 1 || H > SM_MAX_SIDE || W > SM_MAX_SIDE) return false;
    int64_t at = 0;
    auto take = [&](int64_t bytes) { const int64_t o = at; at += (bytes + 15) & ~(int64_t)15; return o; };
    const int64_t cells = std::max((int64_t)H * ((W + 3) & ~3), (int64_t)W * ((H + 3) & ~3));
    L.groups = (int)(((int64_t)H * W + SM_STAT_PIXELS - 1) / SM_STAT_PIXELS);
    L.records = take((int64_t)4 * SM_STAT_WORDS * L.groups);
    L.info = take(16); L.end = take(4);
    L.path = take((int64_t)4 * std::max(H, W));
    L.cost = take(4 * cells); L.codes = take(cells);
    L.total = at;
    return true;
}

static int sm_cost_launch(const float* img1, const float* img2, const float* mask1, const float* mask2, const int32_t* info, int32_t* cost, int H, int W,
                          hipStream_t s) {
    seam_cost_kernel<<<dim3((W + 31) / 32, (H + 31) / 32), 256, 0, s>>>(img1, img2, mask1, mask2, info, cost, H, W);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

static bool sm_overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

// an output overlaps nothing: no input (the kernels that write side, path and info run after others that read the images and masks, but the
// cost plane is written while they are read), no other output, not the workspace; no input lies in the workspace.  ws may be NULL (st_seam_cost).
static bool sm_operands_ok(const float* img1, const float* img2, const float* mask1, const float* mask2, int64_t n, const void* const* outs,
                           const int64_t* out_bytes, int count, const void* ws, int64_t ws_bytes) {
    const void* ins[4] = {img1, img2, mask1, mask2};
    const int64_t in_bytes[4] = {12 * n, 12 * n, 4 * n, 4 * n};
    for (int i = 0; i < count; ++i) {
        if (!outs[i]) continue;
        for (int j = 0; j < 4; ++j)
            if (sm_overlap(outs[i], out_bytes[i], ins[j], in_bytes[j])) return false;
        for (int j = i + 1; j < count; ++j)
            if (outs[j] && sm_overlap(outs[i], out_bytes[i], outs[j], out_bytes[j])) return false;
        if (ws && sm_overlap(outs[i], out_bytes[i], ws, ws_bytes)) return false;
    }
    for (int j = 0; ws && j < 4; ++j)
        if (sm_overlap(ins[j], in_bytes[j], ws, ws_bytes)) return false;
    return true;
}

extern "C" int st_seam_workspace_bytes(int32_t H, int32_t W) {
    sm_layout L;
    return sm_plan(H, W, L) ? (int)L.total : 0;
}

extern "C" int st_seam_cost(const float* img1, const float* img2, const float* mask1, const float* mask2, int32_t H, int32_t W, int32_t* cost, void* stream) {
    sm_layout L;
    if (!img1 || !img2 || !mask1 || !mask2 || !cost || !sm_plan(H, W, L)) return ST_EINVAL;
    const void* outs[1] = {cost};
    const int64_t out_bytes[1] = {(int64_t)4 * H * W};
    if (!sm_operands_ok(img1, img2, mask1, mask2, (int64_t)H * W, outs, out_bytes, 1, nullptr, 0)) return ST_EINVAL;
    return sm_cost_launch(img1, img2, mask1, mask2, nullptr, cost, H, W, (hipStream_t)stream);
}

extern "C" int st_seam_dp(const float* img1, const float* img2, const float* mask1, const float* mask2, int32_t H, int32_t W, int32_t orientation,
                          int32_t first, uint8_t* side_out, int32_t* path_out, int32_t* info_out, void* workspace, int64_t workspace_bytes, void* stream) {
    sm_layout L;
    if (!img1 || !img2 || !mask1 || !mask2 || !side_out || !info_out || !workspace || !sm_plan(H, W, L)) return ST_EINVAL;
    if (orientation < SM_AUTO || orientation > SM_HORIZONTAL || first < 0 || first > 2) return ST_EINVAL;
    if (workspace_bytes < L.total || ((uintptr_t)workspace & 15)) return ST_EINVAL;
    const void* outs[3] = {side_out, path_out, info_out};
    const int64_t out_bytes[3] = {(int64_t)H * W, (int64_t)4 * std::max(H, W), 16};
    if (!sm_operands_ok(img1, img2, mask1, mask2, (int64_t)H * W, outs, out_bytes, 3, workspace, L.total)) return ST_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    uint32_t* records = (uint32_t*)(ws + L.records);
    int32_t *info = (int32_t*)(ws + L.info), *end = (int32_t*)(ws + L.end), *path = (int32_t*)(ws + L.path), *cost = (int32_t*)(ws + L.cost);
    uint8_t* codes = (uint8_t*)(ws + L.codes);
    const int n = H * W;
    seam_stats_kernel<<<L.groups, 256, 0, s>>>(mask1, mask2, records, W, n);
    ST_CHECK_LAUNCH();
    seam_decide_kernel<<<1, 1024, 0, s>>>(records, L.groups, orientation, first, info);
    ST_CHECK_LAUNCH();
    int rc;
    if ((rc = sm_cost_launch(img1, img2, mask1, mask2, info, cost, H, W, s)) != ST_OK) return rc;
    const int threads = ((std::max(H, W) + SM_PER - 1) / SM_PER + 63) / 64 * 64;         // covers a line of either orientation
    seam_dp_kernel<<<1, threads, 0, s>>>(cost, codes, info, end, H, W);
    ST_CHECK_LAUNCH();
    seam_backtrack_kernel<<<1, 256, 0, s>>>(codes, info, end, path, path_out, info_out, H, W);
    ST_CHECK_LAUNCH();
    seam_side_kernel<<<((n + 3) / 4 + 255) / 256, 256, 0, s>>>(info, path, side_out, W, n, ((uintptr_t)side_out & 3) == 0);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
