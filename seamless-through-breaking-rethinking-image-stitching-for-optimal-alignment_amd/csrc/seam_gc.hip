// seam_gc: a minimum cut over the overlap of two warped images, for the ownership of multiband_blend (contract in README.md, "seam_gc"; CPU
// restatement tests/_seam_gc_ref.py).  gfx950 only.  Everything is integers.  Push-relabel with a periodic exact global relabel; what makes
// the result exact is the termination test, not the validity of the labels: the preflow is maximum exactly when, after a global relabel (a
// backward BFS from the sink over residual arcs), no pixel with excess and no source pixel has a finite distance, and the finite-distance
// set of that same relabel is the side-0 plane.  One writer per word, no atomics, no memset / memcpy; every grid and the launch count of
// every entry depend on H and W alone, no kernel loops on data: the data-dependent loop is the caller's, round by round, on the status
// record at the head of the workspace.
//
//   gc_class_kernel    per pixel: none / E1 / E2 / O and, inside O, e = 1 + sum_c |p1 - p2| (1..766)
//   gc_setup_kernel    seeds S and T, the four residuals r = e(p) + e(q), zero outbox and excess, both label planes; |S|, |T| per tile
//   gc_begin_kernel    one workgroup: valid = S and T non-empty; the status record
//   gc_push_kernel     a pixel with excess pushes to lower neighbours (left, right, up, down) what their residuals take, into its outbox;
//                      in the first sweep of a round a source pixel saturates every arc to a finite-distance neighbour outside S
//   gc_gather_kernel   adds the four neighbours' outboxes to the excess and to the reverse residuals; then, as a phase of its own on the
//                      previous labels (a second label plane), lifts a pixel that still has excess to 1 + its lowest residual neighbour
//   gc_bfs_kernel      a 32 x 32 tile and its halo of labels in LDS, GC_LOCAL min-plus sweeps on it; the last launch of an entry also
//                      counts, per tile, the changed labels, the pixels with excess and a finite label and the source pixels with one
//   gc_status_kernel   one workgroup: sums the tiles' records into the status record
//   gc_side_kernel     side per canvas pixel; the excess collected in T per tile
//   gc_info_kernel     one workgroup: the cut, info
#include "common.h"
#include <algorithm>

#define GC_MAX_SIDE 4096
#define GC_INF 0x3fffffff
#define GC_O 1
#define GC_S 2
#define GC_T 4
#define GC_TILE 32
#define GC_LOCAL 64                     // label sweeps inside a tile per launch of gc_bfs_kernel (a path across a tile is at most 62 steps long)
#define GC_PUSH_SWEEPS 32               // push / gather sweeps per round (even: the labels end in plane 0)
#define GC_BFS_LAUNCHES 8               // gc_bfs_kernel launches per round (even, likewise); st_seam_gc_relabel makes twice as many
#define GC_REC_WORDS 4
// status record, int32 [8] at the head of the workspace
#define GC_ST_ACTIVE 0                  // pixels with excess > 0 and a finite label, outside S and T
#define GC_ST_CHANGING 1                // the last label launch still changed a label: the relabel goes on in the next round
#define GC_ST_ROUNDS 2
#define GC_ST_DONE 3
#define GC_ST_SOURCES 4                 // source pixels with a finite label
#define GC_ST_VALID 5
#define GC_ST_SWEEPS 6                  // push / gather sweeps done
#define GC_ST_LABEL_LAUNCHES 7

struct alignas(8) gc_q { int16_t v[4]; };      // per direction: 0 left, 1 right, 2 up, 3 down; the opposite of d is d ^ 1

__device__ __forceinline__ int gc_step(int d, int W) { return d == 0 ? -1 : d == 1 ? 1 : d == 2 ? -W : W; }

__device__ __forceinline__ int gc_absdiff(float a, float b) {
    const int d = (int)st_u8_trunc(a) - (int)st_u8_trunc(b);
    return d < 0 ? -d : d;
}

__device__ __forceinline__ uint32_t gc_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// the sum of `v` over a workgroup of 1024 threads, in thread 0 (part: 16 words of LDS)
__device__ __forceinline__ uint32_t gc_block_sum(uint32_t v, uint32_t* part) {
    const int t = threadIdx.y * blockDim.x + threadIdx.x;
    const uint32_t s = gc_wave_sum(v);
    __syncthreads();                                                      // part may still be read from the previous sum
    if ((t & 63) == 0) part[t >> 6] = s;
    __syncthreads();
    uint32_t total = 0;
    if (t == 0)
        for (int w = 0; w < 16; ++w) total += part[w];
    return total;
}

// ---- 1: classes and costs
__global__ void __launch_bounds__(256) gc_class_kernel(const float* __restrict__ img1, const float* __restrict__ img2, const float* __restrict__ mask1,
                                                       const float* __restrict__ mask2, uint8_t* __restrict__ cls, int16_t* __restrict__ cost, int n) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const bool a = mask1[p] > 0.5f, b = mask2[p] > 0.5f;
    int e = 0;
    if (a && b) e = 1 + gc_absdiff(img1[p], img2[p]) + gc_absdiff(img1[(size_t)n + p], img2[(size_t)n + p]) + gc_absdiff(img1[2 * (size_t)n + p], img2[2 * (size_t)n + p]);
    cls[p] = (uint8_t)((a ? 1 : 0) | (b ? 2 : 0));                        // 1: E1, 2: E2, 3: O
    cost[p] = (int16_t)e;
}

// ---- 2: seeds, capacities, the initial state.  One 32 x 32 tile per workgroup of 1024 threads (the tiling of gc_bfs_kernel: one record each).
__global__ void __launch_bounds__(1024) gc_setup_kernel(const uint8_t* __restrict__ cls, const int16_t* __restrict__ cost, uint8_t* __restrict__ flags,
                                                        gc_q* __restrict__ res, gc_q* __restrict__ outbox, int32_t* __restrict__ excess,
                                                        int32_t* __restrict__ x0, int32_t* __restrict__ x1, int32_t* __restrict__ records, int H, int W) {
    __shared__ uint32_t part[16];
    const int x = blockIdx.x * GC_TILE + threadIdx.x, y = blockIdx.y * GC_TILE + threadIdx.y;
    const bool inside = x < W && y < H;
    uint32_t f = 0;
    if (inside) {
        const int p = y * W + x;
        const bool o = cls[p] == 3;
        const int e = cost[p];
        const bool has[4] = {x > 0, x + 1 < W, y > 0, y + 1 < H};
        bool near1 = false, near2 = false;
        gc_q r;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            int c = 0;
            if (has[d]) {
                const int q = p + gc_step(d, W);
                const int cq = cls[q];
                near1 |= cq == 1; near2 |= cq == 2;
                if (o && cq == 3) c = e + cost[q];
            }
            r.v[d] = (int16_t)c;
        }
        if (o) f = GC_O | (near1 ? GC_S : near2 ? GC_T : 0);
        flags[p] = (uint8_t)f;
        res[p] = r;
        gc_q zero;
        zero.v[0] = zero.v[1] = zero.v[2] = zero.v[3] = 0;
        outbox[p] = zero;
        excess[p] = 0;
        x0[p] = x1[p] = (f & GC_T) ? 0 : GC_INF;
    }
    const uint32_t ns = gc_block_sum((f & GC_S) != 0, part), nt = gc_block_sum((f & GC_T) != 0, part);
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        int32_t* rec = records + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * GC_REC_WORDS;
        rec[0] = (int32_t)ns; rec[1] = (int32_t)nt; rec[2] = 0;
    }
}

// the sums of words 0 .. 2 of the tiles' records, in thread 0 (one workgroup of 1024 threads; a count is at most 2^24)
__device__ __forceinline__ void gc_sum_records(const int32_t* __restrict__ records, int tiles, uint32_t* part, uint32_t total[3]) {
    uint32_t acc[3] = {0, 0, 0};
    for (int g = threadIdx.x; g < tiles; g += 1024) {
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] += (uint32_t)records[(size_t)g * GC_REC_WORDS + k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) total[k] = gc_block_sum(acc[k], part);
}

// ---- 3: the status record of a call.  Without a source or a sink there is nothing to cut: done, not valid.  Else a relabel is under way.
__global__ void __launch_bounds__(1024) gc_begin_kernel(const int32_t* __restrict__ records, int tiles, int32_t* __restrict__ st) {
    __shared__ uint32_t part[16];
    uint32_t total[3];
    gc_sum_records(records, tiles, part, total);
    if (threadIdx.x == 0) {
        const bool valid = total[0] != 0 && total[1] != 0;
        st[GC_ST_ACTIVE] = 0; st[GC_ST_CHANGING] = valid; st[GC_ST_ROUNDS] = 0; st[GC_ST_DONE] = !valid;
        st[GC_ST_SOURCES] = 0; st[GC_ST_VALID] = valid; st[GC_ST_SWEEPS] = 0; st[GC_ST_LABEL_LAUNCHES] = 0;
    }
}

// ---- 4: push.  32 x 8 pixels per workgroup.  Nothing happens while a relabel is under way or after the end (uniform over the grid).  A
// residual > 0 names a neighbour inside O, so inside the canvas.  T never pushes: its outbox stays zero from the setup.
__global__ void __launch_bounds__(256) gc_push_kernel(const int32_t* __restrict__ st, const uint8_t* __restrict__ flags, const int32_t* __restrict__ h,
                                                      gc_q* __restrict__ res, gc_q* __restrict__ outbox, int32_t* __restrict__ excess, int H, int W, int first) {
    if (st[GC_ST_DONE] || st[GC_ST_CHANGING]) return;
    const int x = blockIdx.x * 32 + threadIdx.x, y = blockIdx.y * 8 + threadIdx.y;
    if (x >= W || y >= H) return;
    const int p = y * W + x;
    const uint32_t f = flags[p];
    if (!(f & GC_O) || (f & GC_T)) return;
    gc_q r = res[p], out;
    out.v[0] = out.v[1] = out.v[2] = out.v[3] = 0;
    bool pushed = false;
    if (f & GC_S) {
        if (first) {
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                if (r.v[d] <= 0) continue;
                const int q = p + gc_step(d, W);
                if (h[q] < GC_INF && !(flags[q] & GC_S)) { out.v[d] = r.v[d]; r.v[d] = 0; pushed = true; }
            }
        }
    } else {
        int ex = excess[p];
        const int hp = h[p];
        if (ex > 0 && hp < GC_INF) {
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                if (r.v[d] <= 0 || ex <= 0) continue;
                if (h[p + gc_step(d, W)] < hp) {
                    const int delta = min(ex, (int)r.v[d]);
                    out.v[d] = (int16_t)delta; r.v[d] = (int16_t)(r.v[d] - delta); ex -= delta; pushed = true;
                }
            }
            if (pushed) excess[p] = ex;
        }
    }
    outbox[p] = out;
    if (pushed) res[p] = r;
}

// ---- 5: gather, then relabel.  The outbox of a pixel outside O is zero.  `last`: the round's sweeps end here and its relabel starts from
// scratch: 0 in T, infinite elsewhere.
__global__ void __launch_bounds__(256) gc_gather_kernel(const int32_t* __restrict__ st, const uint8_t* __restrict__ flags, const gc_q* __restrict__ outbox,
                                                        gc_q* __restrict__ res, int32_t* __restrict__ excess, const int32_t* __restrict__ hin,
                                                        int32_t* __restrict__ hout, int H, int W, int last) {
    if (st[GC_ST_DONE] || st[GC_ST_CHANGING]) return;
    const int x = blockIdx.x * 32 + threadIdx.x, y = blockIdx.y * 8 + threadIdx.y;
    if (x >= W || y >= H) return;
    const int p = y * W + x;
    const uint32_t f = flags[p];
    if (!(f & GC_O)) return;
    const bool has[4] = {x > 0, x + 1 < W, y > 0, y + 1 < H};
    gc_q r = res[p];
    int ex = excess[p], got = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        if (!has[d]) continue;
        const int inc = outbox[p + gc_step(d, W)].v[d ^ 1];
        r.v[d] = (int16_t)(r.v[d] + inc);
        got += inc;
    }
    ex = (f & GC_S) ? 0 : ex + got;
    if (got) { res[p] = r; excess[p] = ex; }
    int hn = hin[p];
    if (!(f & (GC_S | GC_T)) && ex > 0 && hn < GC_INF) {
        int m = GC_INF;
#pragma unroll
        for (int d = 0; d < 4; ++d)
            if (r.v[d] > 0) m = min(m, hin[p + gc_step(d, W)]);
        hn = max(hn, m >= GC_INF ? GC_INF : m + 1);
    }
    hout[p] = last ? ((f & GC_T) ? 0 : GC_INF) : hn;
}

// ---- 6: the global relabel: d(T) = 0, d(p) = 1 + min over the residual arcs p -> q of d(q), downwards from infinity.  A 32 x 32 tile per
// workgroup of 1024 threads, its labels and a halo of one pixel in LDS; GC_LOCAL Jacobi sweeps between barriers with the halo held fixed, then
// the tile goes to the other plane.  Labels only fall and are path lengths at all times, so a launch that changes nothing anywhere has
// reached the exact distances.  Pixels outside O hold infinity in both planes from the setup.
__global__ void __launch_bounds__(1024) gc_bfs_kernel(const int32_t* __restrict__ st, const uint8_t* __restrict__ flags, const gc_q* __restrict__ res,
                                                      const int32_t* __restrict__ excess, const int32_t* __restrict__ din, int32_t* __restrict__ dout,
                                                      int32_t* __restrict__ records, int H, int W, int last) {
    __shared__ int32_t lab[2][GC_TILE + 2][GC_TILE + 3];                  // two buffers by sweep parity: one barrier per sweep
    __shared__ uint32_t part[16];
    if (st[GC_ST_DONE]) return;
    const int tx = threadIdx.x, ty = threadIdx.y, t = ty * GC_TILE + tx;
    const int x0 = blockIdx.x * GC_TILE, y0 = blockIdx.y * GC_TILE, x = x0 + tx, y = y0 + ty;
    const bool inside = x < W && y < H;
    const int p = inside ? y * W + x : 0;
    const uint32_t f = inside ? flags[p] : 0;
    const bool live = (f & GC_O) != 0;
    int32_t* rec = records + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * GC_REC_WORDS;
    if (!__syncthreads_or(live)) {                                        // a tile without an overlap pixel has no label to move (uniform over the workgroup)
        if (last && t == 0) rec[0] = rec[1] = rec[2] = 0;
        return;
    }
    const int first = inside ? din[p] : GC_INF;
    lab[0][ty + 1][tx + 1] = first;
    if (t < 4 * GC_TILE) {                                                // the halo: above, below, left, right; it stays what it is in both buffers
        const int side = t >> 5, i = t & 31;
        const int hx = side == 0 || side == 1 ? x0 + i : side == 2 ? x0 - 1 : x0 + GC_TILE;
        const int hy = side == 0 ? y0 - 1 : side == 1 ? y0 + GC_TILE : y0 + i;
        const int v = (hx >= 0 && hx < W && hy >= 0 && hy < H) ? din[hy * W + hx] : GC_INF;
        const int ly = side == 0 ? 0 : side == 1 ? GC_TILE + 1 : i + 1, lx = side == 2 ? 0 : side == 3 ? GC_TILE + 1 : i + 1;
        lab[0][ly][lx] = lab[1][ly][lx] = v;
    }
    bool arc[4] = {false, false, false, false};
    if (live && !(f & GC_T)) {
        const gc_q r = res[p];
#pragma unroll
        for (int d = 0; d < 4; ++d) arc[d] = r.v[d] > 0;
    }
    int m = first;
    __syncthreads();
#pragma unroll 2
    for (int it = 0; it < GC_LOCAL; ++it) {
        const int32_t (*cur)[GC_TILE + 3] = lab[it & 1];
        if (arc[0]) m = min(m, cur[ty + 1][tx] + 1);                      // (infinity + 1 stays above every label)
        if (arc[1]) m = min(m, cur[ty + 1][tx + 2] + 1);
        if (arc[2]) m = min(m, cur[ty][tx + 1] + 1);
        if (arc[3]) m = min(m, cur[ty + 2][tx + 1] + 1);
        lab[(it & 1) ^ 1][ty + 1][tx + 1] = m;                            // (read again only after the next barrier, written again only after the one behind it)
        __syncthreads();
    }
    if (live) dout[p] = m;
    if (!last) return;                                                    // (uniform over the grid)
    const bool finite = live && m < GC_INF;
    const uint32_t changed = gc_block_sum(live && m != first, part);
    const uint32_t active = gc_block_sum(finite && !(f & (GC_S | GC_T)) && excess[p] > 0, part);
    const uint32_t sources = gc_block_sum(finite && (f & GC_S), part);
    if (t == 0) { rec[0] = (int32_t)changed; rec[1] = (int32_t)active; rec[2] = (int32_t)sources; }
}

// ---- 7: the status record after an entry: `round` = 0 after the relabel of the begin entry; `sweeps`: the push / gather sweeps the entry
// launched, `launches` its label launches
__global__ void __launch_bounds__(1024) gc_status_kernel(const int32_t* __restrict__ records, int tiles, int32_t* __restrict__ st, int round, int sweeps,
                                                         int launches) {
    __shared__ uint32_t part[16];
    if (st[GC_ST_DONE]) return;
    uint32_t total[3];
    gc_sum_records(records, tiles, part, total);
    if (threadIdx.x == 0) {
        if (!st[GC_ST_CHANGING]) st[GC_ST_SWEEPS] += sweeps;                  // (the sweeps ran only with the relabel before them complete)
        st[GC_ST_LABEL_LAUNCHES] += launches;
        st[GC_ST_ROUNDS] += round;
        st[GC_ST_CHANGING] = total[0] != 0;
        st[GC_ST_ACTIVE] = (int32_t)total[1];
        st[GC_ST_SOURCES] = (int32_t)total[2];
        st[GC_ST_DONE] = total[0] == 0 && total[1] == 0 && total[2] == 0;
    }
}

// ---- 8: side: 0 iff the cut is there (done and valid), p is in O and its label is finite.  The excess of T per tile (at most 1024 * 6128).
__global__ void __launch_bounds__(1024) gc_side_kernel(const int32_t* __restrict__ st, const uint8_t* __restrict__ flags, const int32_t* __restrict__ excess,
                                                       const int32_t* __restrict__ d, uint8_t* __restrict__ side, int32_t* __restrict__ records, int H, int W) {
    __shared__ uint32_t part[16];
    const int x = blockIdx.x * GC_TILE + threadIdx.x, y = blockIdx.y * GC_TILE + threadIdx.y;
    const bool ok = st[GC_ST_DONE] && st[GC_ST_VALID];
    uint32_t flow = 0;
    if (x < W && y < H) {
        const int p = y * W + x;
        const uint32_t f = flags[p];
        side[p] = !(ok && (f & GC_O) && d[p] < GC_INF);
        if (ok && (f & GC_T)) flow = (uint32_t)excess[p];
    }
    const uint32_t total = gc_block_sum(flow, part);
    if (threadIdx.x == 0 && threadIdx.y == 0) records[(size_t)(blockIdx.y * gridDim.x + blockIdx.x) * GC_REC_WORDS] = (int32_t)total;
}

// ---- 9: info = (valid, 3, cut >> 31, cut & (2^31 - 1))
__global__ void __launch_bounds__(1024) gc_info_kernel(const int32_t* __restrict__ st, const int32_t* __restrict__ records, int tiles, int32_t* __restrict__ info) {
    __shared__ unsigned long long part[16];
    unsigned long long acc = 0;
    for (int g = threadIdx.x; g < tiles; g += 1024) acc += (uint32_t)records[(size_t)g * GC_REC_WORDS];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)acc, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(acc >> 32), o, 64);
        acc += (unsigned long long)hi << 32 | lo;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long cut = 0;
        for (int w = 0; w < 16; ++w) cut += part[w];
        const bool ok = st[GC_ST_DONE] && st[GC_ST_VALID];
        info[0] = ok; info[1] = 3;
        info[2] = ok ? (int32_t)(cut >> 31) : 0;
        info[3] = ok ? (int32_t)(cut & 0x7fffffffull) : 0;
    }
}

// workspace layout: status int32 [8]; records int32 [tiles, 4]; classes uint8 [n]; flags uint8 [n]; costs int16 [n]; residuals and outbox
// int16 [n, 4] each; excess int32 [n]; two label planes int32 [n] -- each region rounded up to 16 bytes
struct gc_layout {
    int tiles, gx, gy;
    int64_t status, records, cls, flags, cost, res, outbox, excess, x0, x1, total;
};

static bool gc_plan(int H, int W, gc_layout& L) {
    if (H < 1 || W < 1 || H > GC_MAX_SIDE || W > GC_MAX_SIDE) return false;
    int64_t at = 0;
    auto take = [&](int64_t bytes) { const int64_t o = at; at += (bytes + 15) & ~(int64_t)15; return o; };
    const int64_t n = (int64_t)H * W;
    L.gx = (W + GC_TILE - 1) / GC_TILE; L.gy = (H + GC_TILE - 1) / GC_TILE; L.tiles = L.gx * L.gy;
    L.status = take(32);
    L.records = take((int64_t)4 * GC_REC_WORDS * L.tiles);
    L.cls = take(n); L.flags = take(n); L.cost = take(2 * n);
    L.res = take(8 * n); L.outbox = take(8 * n);
    L.excess = take(4 * n); L.x0 = take(4 * n); L.x1 = take(4 * n);
    L.total = at;
    return true;
}

static bool gc_overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

static bool gc_workspace_ok(const void* workspace, int64_t workspace_bytes, const gc_layout& L) {
    return workspace && workspace_bytes >= L.total && !((uintptr_t)workspace & 15);
}

// the label launches of an entry and the status record after them
static int gc_relabel(const gc_layout& L, char* ws, int H, int W, int round, int sweeps, int launches, hipStream_t s) {
    int32_t* st = (int32_t*)(ws + L.status);
    int32_t* records = (int32_t*)(ws + L.records);
    int32_t* x[2] = {(int32_t*)(ws + L.x0), (int32_t*)(ws + L.x1)};
    for (int j = 0; j < launches; ++j) {
        gc_bfs_kernel<<<dim3(L.gx, L.gy), dim3(GC_TILE, GC_TILE), 0, s>>>(st, (const uint8_t*)(ws + L.flags), (const gc_q*)(ws + L.res), (const int32_t*)(ws + L.excess),
                                                                          x[j & 1], x[(j + 1) & 1], records, H, W, j == launches - 1);
        ST_CHECK_LAUNCH();
    }
    gc_status_kernel<<<1, 1024, 0, s>>>(records, L.tiles, st, round, sweeps, launches);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

extern "C" int st_seam_gc_workspace_bytes(int32_t H, int32_t W) {
    gc_layout L;
    return gc_plan(H, W, L) ? (int)L.total : 0;
}

extern "C" int st_seam_gc_begin(const float* img1, const float* img2, const float* mask1, const float* mask2, int32_t H, int32_t W, void* workspace,
                                int64_t workspace_bytes, void* stream) {
    gc_layout L;
    if (!img1 || !img2 || !mask1 || !mask2 || !gc_plan(H, W, L) || !gc_workspace_ok(workspace, workspace_bytes, L)) return ST_EINVAL;
    const int64_t n = (int64_t)H * W;
    const void* ins[4] = {img1, img2, mask1, mask2};
    const int64_t in_bytes[4] = {12 * n, 12 * n, 4 * n, 4 * n};
    for (int j = 0; j < 4; ++j)
        if (gc_overlap(ins[j], in_bytes[j], workspace, L.total)) return ST_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int32_t* records = (int32_t*)(ws + L.records);
    gc_class_kernel<<<(int)((n + 255) / 256), 256, 0, s>>>(img1, img2, mask1, mask2, (uint8_t*)(ws + L.cls), (int16_t*)(ws + L.cost), (int)n);
    ST_CHECK_LAUNCH();
    gc_setup_kernel<<<dim3(L.gx, L.gy), dim3(GC_TILE, GC_TILE), 0, s>>>((const uint8_t*)(ws + L.cls), (const int16_t*)(ws + L.cost), (uint8_t*)(ws + L.flags),
                                                                        (gc_q*)(ws + L.res), (gc_q*)(ws + L.outbox), (int32_t*)(ws + L.excess),
                                                                        (int32_t*)(ws + L.x0), (int32_t*)(ws + L.x1), records, H, W);
    ST_CHECK_LAUNCH();
    gc_begin_kernel<<<1, 1024, 0, s>>>(records, L.tiles, (int32_t*)(ws + L.status));
    ST_CHECK_LAUNCH();
    return gc_relabel(L, ws, H, W, 0, 0, GC_BFS_LAUNCHES, s);
}

extern "C" int st_seam_gc_round(int32_t H, int32_t W, void* workspace, int64_t workspace_bytes, void* stream) {
    gc_layout L;
    if (!gc_plan(H, W, L) || !gc_workspace_ok(workspace, workspace_bytes, L)) return ST_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int32_t* st = (const int32_t*)(ws + L.status);
    const uint8_t* flags = (const uint8_t*)(ws + L.flags);
    gc_q *res = (gc_q*)(ws + L.res), *outbox = (gc_q*)(ws + L.outbox);
    int32_t* excess = (int32_t*)(ws + L.excess);
    int32_t* x[2] = {(int32_t*)(ws + L.x0), (int32_t*)(ws + L.x1)};
    const dim3 grid((W + 31) / 32, (H + 7) / 8), block(32, 8);
    for (int k = 0; k < GC_PUSH_SWEEPS; ++k) {
        gc_push_kernel<<<grid, block, 0, s>>>(st, flags, x[k & 1], res, outbox, excess, H, W, k == 0);
        ST_CHECK_LAUNCH();
        gc_gather_kernel<<<grid, block, 0, s>>>(st, flags, outbox, res, excess, x[k & 1], x[(k + 1) & 1], H, W, k == GC_PUSH_SWEEPS - 1);
        ST_CHECK_LAUNCH();
    }
    return gc_relabel(L, ws, H, W, 1, GC_PUSH_SWEEPS, GC_BFS_LAUNCHES, s);
}

// a round without its sweeps, for the caller to make while the status record says that the relabel is still changing (gc_push_kernel and
// gc_gather_kernel would do nothing then): twice the label launches of a round, then the status record
extern "C" int st_seam_gc_relabel(int32_t H, int32_t W, void* workspace, int64_t workspace_bytes, void* stream) {
    gc_layout L;
    if (!gc_plan(H, W, L) || !gc_workspace_ok(workspace, workspace_bytes, L)) return ST_EINVAL;
    return gc_relabel(L, (char*)workspace, H, W, 1, 0, 2 * GC_BFS_LAUNCHES, (hipStream_t)stream);
}

extern "C" int st_seam_gc_finish(int32_t H, int32_t W, uint8_t* side_out, int32_t* info_out, void* workspace, int64_t workspace_bytes, void* stream) {
    gc_layout L;
    if (!side_out || !info_out || !gc_plan(H, W, L) || !gc_workspace_ok(workspace, workspace_bytes, L)) return ST_EINVAL;
    const int64_t n = (int64_t)H * W;
    if (gc_overlap(side_out, n, info_out, 16) || gc_overlap(side_out, n, workspace, L.total) || gc_overlap(info_out, 16, workspace, L.total)) return ST_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int32_t* st = (const int32_t*)(ws + L.status);
    int32_t* records = (int32_t*)(ws + L.records);
    gc_side_kernel<<<dim3(L.gx, L.gy), dim3(GC_TILE, GC_TILE), 0, s>>>(st, (const uint8_t*)(ws + L.flags), (const int32_t*)(ws + L.excess), (const int32_t*)(ws + L.x0),
                                                                       side_out, records, H, W);
    ST_CHECK_LAUNCH();
    gc_info_kernel<<<1, 1024, 0, s>>>(st, records, L.tiles, info_out);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
