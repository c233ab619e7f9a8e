// inner_crop: the largest axis-aligned rectangle that lies wholly inside the union of the two warp masks (contract in README.md,
// "inner_crop"; CPU restatement tests/_crop_ref.py).  gfx950 only.  Everything is integers.  Every kernel of a call goes to the caller's
// stream, in order, inside the caller's workspace: no host synchronisation, no allocation, no memset / memcpy, no atomics (every element has
// exactly one writer), and the launch count and every grid depend on H and W alone, so a call captures into a hipGraph as a linear chain.
//
//   crop_runs_kernel   r(y, x) = set pixels of U in column x ending at row y, int16 (64 columns x 16 row segments per workgroup)
//   crop_rows_kernel   one workgroup per row: the candidate of every position -- the widest span round x whose runs reach r(y, x) -- from a
//                      two-level search over the row and its block minima in LDS; the row's best candidate as one 64-bit key
//   crop_pick_kernel   one workgroup: the best of the H row keys, decoded into info = (valid, top, left, height, width, area)
#include "common.h"

#define CR_MAX_SIDE 4096
#define CR_SEGS 16                      // row segments per column of the run pass
#define CR_BLOCK 64                     // positions per block of the row search = one wave
#define CR_ROW_THREADS 256
#define CR_PICK_THREADS 1024

// U = m1 or m2, m = mask > 0.5 (NaN, -Inf and 0.5 are unset, +Inf is set); mask2 may be NULL (uniform over the grid)
__device__ __forceinline__ bool cr_set(const float* __restrict__ mask1, const float* __restrict__ mask2, size_t p) {
    const bool a = mask1[p] > 0.5f, b = mask2 ? mask2[p] > 0.5f : false;
    return a || b;
}

__device__ __forceinline__ unsigned long long cr_shfl_xor64(unsigned long long v, int o) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    return (unsigned long long)hi << 32 | lo;
}

__device__ __forceinline__ unsigned long long cr_wave_max(unsigned long long key) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = cr_shfl_xor64(key, o);
        key = other > key ? other : key;
    }
    return key;
}

// ---- 1: runs.  A workgroup takes 64 columns (coalesced across columns) and cuts them into CR_SEGS row segments of S rows, one thread each:
// (1) every segment publishes the set rows since its last unset pixel (S when the whole segment is set), (2) a thread's carry is the sum of
// those over the segments above it, up to and including the first one that is not wholly set, (3) a sweep down from that carry.
__global__ void __launch_bounds__(64 * CR_SEGS) crop_runs_kernel(const float* __restrict__ mask1, const float* __restrict__ mask2, int16_t* __restrict__ runs,
                                                                 int H, int W) {
    __shared__ int tail[CR_SEGS][64];
    const int tx = threadIdx.x, seg = threadIdx.y, x = blockIdx.x * 64 + tx;
    const bool act = x < W;
    const int S = (H + CR_SEGS - 1) / CR_SEGS, y0 = min(seg * S, H), y1 = min(y0 + S, H);
    int t = 0;
    if (act) {
#pragma unroll 8
        for (int y = y0; y < y1; ++y) t = cr_set(mask1, mask2, (size_t)y * W + x) ? t + 1 : 0;
    }
    tail[seg][tx] = t;
    __syncthreads();
    if (!act || y0 >= y1) return;
    int v = 0;                                             // (every segment above a non-empty one holds S rows)
    for (int s = seg - 1; s >= 0; --s) {
        const int tl = tail[s][tx];
        v += tl;
        if (tl < S) break;
    }
#pragma unroll 8
    for (int y = y0; y < y1; ++y) {
        v = cr_set(mask1, mask2, (size_t)y * W + x) ? v + 1 : 0;
        runs[(size_t)y * W + x] = (int16_t)v;
    }
}

// ---- 2: rows.  The row of r in LDS with the minimum of every block of 64 positions (a wave loads a block, so the minimum is one wave
// reduction at load time).  For a position x with v = r(y, x) > 0, L = the nearest column on the left with r < v (-1: none), R the same on
// the right (W: none).  Two levels, at most 1 + 63 + 63 + 63 LDS reads per side whatever the data:
//   the own block's minimum (one read, shared by the two sides): only when it is below v can the own block hold the answer, and only then
//   is it scanned (<= 63); then the block minima outward (<= 63); then the one block whose minimum is below v, from its near end: its far
//   end is not read, for when every other position has failed the far end is the one that made the minimum (<= 63).
// The outward scan this replaces reads W values per position on a row of equal runs, the commonest row of a union mask.
__device__ __forceinline__ int cr_left(const uint16_t* row, const uint16_t* bmin, int x, int v, bool own) {
    const int blk = x / CR_BLOCK;
    if (own)
        for (int k = x - 1; k >= blk * CR_BLOCK; --k)
            if (row[k] < v) return k;
    for (int b = blk - 1; b >= 0; --b)
        if (bmin[b] < v) {
            int k = b * CR_BLOCK + CR_BLOCK - 1;
            while (k > b * CR_BLOCK && row[k] >= v) --k;
            return k;
        }
    return -1;
}

__device__ __forceinline__ int cr_right(const uint16_t* row, const uint16_t* bmin, int x, int v, bool own, int W) {
    const int blk = x / CR_BLOCK, blocks = (W + CR_BLOCK - 1) / CR_BLOCK;
    if (own)
        for (int k = x + 1; k <= min(blk * CR_BLOCK + CR_BLOCK - 1, W - 1); ++k)
            if (row[k] < v) return k;
    for (int b = blk + 1; b < blocks; ++b)
        if (bmin[b] < v) {
            const int last = min(b * CR_BLOCK + CR_BLOCK - 1, W - 1);
            int k = b * CR_BLOCK;
            while (k < last && row[k] >= v) ++k;
            return k;
        }
    return W;
}

// the key of a candidate: its unsigned order is largest area, then lowest top, then lowest left, then smallest height.  area <= 2^24 takes
// 25 bits, 4095 - top and 4095 - left 12 each, 8191 - h 13: 62 bits; 0 = no candidate (a real one has area >= 1).
__device__ __forceinline__ unsigned long long cr_key(int top, int left, int h, int w) {
    return (unsigned long long)(uint32_t)(h * w) << 37 | (unsigned long long)(uint32_t)(4095 - top) << 25 | (unsigned long long)(uint32_t)(4095 - left) << 13 |
           (unsigned long long)(uint32_t)(8191 - h);
}

__global__ void __launch_bounds__(CR_ROW_THREADS) crop_rows_kernel(const int16_t* __restrict__ runs, unsigned long long* __restrict__ records, int W) {
    __shared__ uint16_t row[CR_MAX_SIDE];
    __shared__ uint16_t bmin[CR_MAX_SIDE / CR_BLOCK];
    __shared__ unsigned long long part[CR_ROW_THREADS / 64];
    const int y = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int padded = (W + CR_BLOCK - 1) / CR_BLOCK * CR_BLOCK;
    for (int x = t; x < padded; x += CR_ROW_THREADS) {               // (a wave is inside the loop or outside it as a whole)
        const int v = x < W ? (int)(uint16_t)runs[(size_t)y * W + x] : 0xFFFF;
        row[x] = (uint16_t)v;
        int m = v;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o, 64));
        if (lane == 0) bmin[x / CR_BLOCK] = (uint16_t)m;
    }
    __syncthreads();
    unsigned long long key = 0;
    for (int x = t; x < W; x += CR_ROW_THREADS) {
        const int v = row[x];
        if (v == 0) continue;
        const bool own = bmin[x / CR_BLOCK] < v;
        const int L = cr_left(row, bmin, x, v, own), R = cr_right(row, bmin, x, v, own, W);
        const unsigned long long k = cr_key(y - v + 1, L + 1, v, R - L - 1);
        key = k > key ? k : key;
    }
    key = cr_wave_max(key);
    if (lane == 0) part[wave] = key;
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int w = 1; w < CR_ROW_THREADS / 64; ++w) key = part[w] > key ? part[w] : key;
        records[y] = key;
    }
}

// ---- 3: pick.  One workgroup; info = (valid, top, left, height, width, area), all zeros when no row has a candidate.
__global__ void __launch_bounds__(CR_PICK_THREADS) crop_pick_kernel(const unsigned long long* __restrict__ records, int H, int32_t* __restrict__ info) {
    __shared__ unsigned long long part[CR_PICK_THREADS / 64];
    unsigned long long key = 0;
    for (int y = threadIdx.x; y < H; y += CR_PICK_THREADS) key = records[y] > key ? records[y] : key;
    key = cr_wave_max(key);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CR_PICK_THREADS / 64; ++w) key = part[w] > key ? part[w] : key;
        const int valid = key != 0;
        const int area = (int)(key >> 37), top = 4095 - (int)(key >> 25 & 4095), left = 4095 - (int)(key >> 13 & 4095), h = 8191 - (int)(key & 8191);
        info[0] = valid;
        info[1] = valid ? top : 0;
        info[2] = valid ? left : 0;
        info[3] = valid ? h : 0;
        info[4] = valid ? area / h : 0;
        info[5] = area;
    }
}

// workspace layout: runs int16 [H, W]; records uint64 [H] -- each region rounded up to 16 bytes
struct cr_layout {
    int64_t runs, records, total;
};

static bool cr_plan(int H, int W, cr_layout& L) {
    if (H < 1 || W < 1 || H > CR_MAX_SIDE || W > CR_MAX_SIDE) return false;
    int64_t at = 0;
    auto take = [&](int64_t bytes) { const int64_t o = at; at += (bytes + 15) & ~(int64_t)15; return o; };
    L.runs = take((int64_t)2 * H * W);
    L.records = take((int64_t)8 * H);
    L.total = at;
    return true;
}

static bool cr_overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

extern "C" int st_inner_rect_workspace_bytes(int32_t H, int32_t W) {
    cr_layout L;
    return cr_plan(H, W, L) ? (int)L.total : 0;
}

extern "C" int st_inner_rect(const float* mask1, const float* mask2, int32_t H, int32_t W, int32_t* info_out, int16_t* runs_out, void* workspace,
                             int64_t workspace_bytes, void* stream) {
    cr_layout L;
    if (!mask1 || !info_out || !workspace || !cr_plan(H, W, L)) return ST_EINVAL;
    if (workspace_bytes < L.total || ((uintptr_t)workspace & 15)) return ST_EINVAL;
    const int64_t n = (int64_t)H * W;
    // an output overlaps nothing: no mask (runs is written while the masks are read), not the other output, not the workspace; no mask lies
    // in the workspace
    const void* outs[2] = {info_out, runs_out};
    const int64_t out_bytes[2] = {24, 2 * n};
    const void* masks[2] = {mask1, mask2};
    for (int i = 0; i < 2; ++i) {
        if (!outs[i]) continue;
        for (int j = 0; j < 2; ++j)
            if (masks[j] && cr_overlap(outs[i], out_bytes[i], masks[j], 4 * n)) return ST_EINVAL;
        if (cr_overlap(outs[i], out_bytes[i], workspace, L.total)) return ST_EINVAL;
    }
    if (runs_out && cr_overlap(info_out, 24, runs_out, 2 * n)) return ST_EINVAL;
    for (int j = 0; j < 2; ++j)
        if (masks[j] && cr_overlap(masks[j], 4 * n, workspace, L.total)) return ST_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int16_t* runs = runs_out ? runs_out : (int16_t*)(ws + L.runs);
    unsigned long long* records = (unsigned long long*)(ws + L.records);
    crop_runs_kernel<<<(W + 63) / 64, dim3(64, CR_SEGS), 0, s>>>(mask1, mask2, runs, H, W);
    ST_CHECK_LAUNCH();
    crop_rows_kernel<<<H, CR_ROW_THREADS, 0, s>>>(runs, records, W);
    ST_CHECK_LAUNCH();
    crop_pick_kernel<<<1, CR_PICK_THREADS, 0, s>>>(records, H, info_out);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
