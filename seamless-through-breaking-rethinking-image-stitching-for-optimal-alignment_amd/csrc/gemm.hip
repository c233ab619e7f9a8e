// fp32 implicit-GEMM on the gfx950 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 fmaf chain).
//
//   C[m, n] = epilogue( alpha * sum_k A(m, k) * Wt[n, k] + bias[n] )
//
// A is an NHWC activation read through convolution addressing (kh x kw window, stride, zero
// padding); a plain row-major matrix is the 1x1 case.  Wt is [N, K] row-major with
// K = kh*kw*Cin ordered (ky, kx, c) -- the layout nn.Linear already has and the layout the host
// prepacks conv weights into.  Both operand tiles are K-contiguous in LDS; each lane fetches 4 consecutive k
// of its row with one ds_read_b128 and feeds them to 4 consecutive MFMAs, lane half h taking k = 8j+4h+t for
// both operands so the contraction pairs up without any transposition.
//
// This file is the fp32 family and the dispatcher; the exact-split bf16 kernels (gemm_split3.h) are launched from gemm_split3.hip, the
// C = 128 row kernels (rowchain128 / rowmlp128, mlp_split3.h) from gemm_rows.hip; what the three share -- the descriptor checks among it -- is gemm_common.h.
// Dispatch (conv_gemm_launch): check_f32 -> for_each_row_chunk if the rows are beyond one launch -> plan_f32, a pure function -> launch_f32, a switch on
// the plan; st_gemm_plan runs the first three alone.  Kernels in this file:
//   conv_gemm_dma_kernel   Cin % 32 == 0 (the default): global -> LDS DMA ring, VALU-free K loop, optional persistent walk
//                          over M tiles; tiles 64x64 / 128x64 / 128x32
//   conv_gemm_kernel       any Cin % 4 == 0 (or scalar gather otherwise): register-staged, [rows][BK+4] padded LDS tiles
//   rowstream_gemm_kernel  plain matrices with K = 64 / 128 and many rows: weights resident in LDS, A rows in registers
//   skinny_gemm_kernel (M <= 8), narrow_conv_kernel / narrow_conv3x3_kernel (N <= 4), splitk_reduce_kernel
// and one epilogue (bias, alpha, row-mapped addend, activation, residual / gate / GRU / axpy / fused z|r) shared by all (gemm_common.h).
//
// Replaces (reference, /root/reference): every F.conv2d / nn.Linear / einsum contraction on the
// FlowHomoAdpater path, e.g. core/FlowFormer/PerCostFormer3/encoder.py:359-369 (all-pairs corr),
// gru.py:44-59 (SepConvGRU), core/UDIS2/Homography/network.py:103-137 (ResNet-50 + regressor).
#include "gemm_common.h"

// optional profiling observer (st_set_gemm_observer) and the launch plan of the calling thread's last launch (st_gemm_last_plan)
typedef void (*st_gemm_observer_fn)(const st_gemm_desc*, void* stream, int32_t phase, void* user);
static st_gemm_observer_fn g_observer = nullptr;
static void* g_observer_user = nullptr;
static thread_local int32_t g_last_plan[4] = {-1, 0, 0, 0};

// the only way in for the launchers of the family, here and in the other translation units (declared in gemm_common.h)
void st_plan_set(int kernel, int tile, int split_k, int persistent) {
    g_last_plan[0] = kernel; g_last_plan[1] = tile; g_last_plan[2] = split_k; g_last_plan[3] = persistent;
}
bool st_observer_installed(void) { return g_observer != nullptr; }
bool st_observe(const st_gemm_desc* od, void* stream, int phase) {
    st_gemm_observer_fn obs = g_observer;
    if (!obs) return false;
    obs(od, stream, phase, g_observer_user);
    return true;
}

#define BK 32
#define LDS_LD (BK + 4)

template <int WARPS_M, int WARPS_N, int TM, int TN, bool VEC>
__global__ __launch_bounds__(256) void conv_gemm_kernel(const st_gemm_desc d) {
    constexpr int BM = WARPS_M * TM * 32;
    constexpr int BN = WARPS_N * TN * 32;
    static_assert(WARPS_M * WARPS_N == 4, "4 waves per workgroup");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                      // [2][BM][LDS_LD]
    float* Bs = smem + 2 * BM * LDS_LD;    // [2][BN][LDS_LD]

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WARPS_N, wn = wave % WARPS_N;

    // grid.z is either the batch index or, for split-K launches (batch == 1), the K slice
    const int split = d.split_k > 1 ? d.split_k : 1;
    const int bz = split > 1 ? 0 : blockIdx.z;
    const int kz = split > 1 ? blockIdx.z : 0;
    const float* __restrict__ X = d.a + (size_t)bz * d.batch_stride_a;
    const float* __restrict__ Wt = d.w + (size_t)bz * d.batch_stride_w;
    float* __restrict__ C = d.c + (size_t)bz * d.batch_stride_c;

    // XCD-aware tile order: consecutive block ids are dealt round-robin over the 8 XCDs, so give
    // each XCD a contiguous run of tiles (neighbouring tiles share operand panels in its L2).
    const int ntm = (d.M + BM - 1) / BM, ntn = (d.N + BN - 1) / BN;
    const int nwg = ntm * ntn;
    int bid = blockIdx.x;
    {
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int tile_n = bid % ntn, tile_m = bid / ntn;
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    const int K = d.K;
    const int dil_h = d.dh > 1 ? d.dh : 1, dil_w = d.dw > 1 ? d.dw : 1;      // conv dilation (0 / 1 = dense)
    const int kcol = (tid & 7) * 4;   // this thread's float4 column inside a BK chunk
    const int rrow = tid >> 3;        // 0..31

    // per-thread A rows: decode m -> (b, oy, ox) once
    constexpr int AP = BM / 32, BP = BN / 32;
    int a_pix[AP];      // pixel index of (b, iy0, ix0) top-left, or <0 row invalid
    int a_iy0[AP], a_ix0[AP], a_b[AP];
#pragma unroll
    for (int p = 0; p < AP; ++p) {
        const int m = m0 + rrow + 32 * p;
        if (m < d.M) {
            const int hw = d.Ho * d.Wo;
            const int b = m / hw, r = m - b * hw;
            const int oy = r / d.Wo, ox = r - oy * d.Wo;
            a_b[p] = b; a_iy0[p] = oy * d.sh - d.ph; a_ix0[p] = ox * d.sw - d.pw;
            a_pix[p] = 0;
        } else { a_pix[p] = -1; a_b[p] = 0; a_iy0[p] = 0; a_ix0[p] = 0; }
    }

    // descriptors over the whole A / W extents of this batch slice (wave-uniform: kernel args + blockIdx)
    const __amdgpu_buffer_rsrc_t rsrcA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(X), 0, (int)d.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrcW = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Wt), 0, (int)d.w_bytes, 0x00020000);
    float4 ra[AP], rb[BP];
    // VEC path state: this thread's (ky, kx, c) for the tile being loaded, advanced incrementally
    // (one integer division per kernel instead of two per K step); loads are branch-free -- an
    // out-of-range tap / row / k reads a safe address and is zeroed by a select, so the compiler
    // can issue all of a step's global loads back to back.
    int t_ky = 0, t_kx = 0, t_c = 0, t_kt = -2;   // -2: the first tile always decodes by division
    auto load_tile = [&](int kt) {
        const int k = kt * BK + kcol;
        if constexpr (VEC) {
            if (d.kh * d.kw > 1) {
                if (t_kt + 1 == kt && d.Cin >= BK) {
                    t_c += BK;
                    if (t_c >= d.Cin) { t_c -= d.Cin; if (++t_kx == d.kw) { t_kx = 0; ++t_ky; } }
                } else {
                    const int kyx = k / d.Cin;
                    t_c = k - kyx * d.Cin; t_ky = kyx / d.kw; t_kx = kyx - t_ky * d.kw;
                }
                t_kt = kt;
            } else { t_c = k; }
            const bool kin = k < K;
#pragma unroll
            for (int p = 0; p < AP; ++p) {
                const int iy = a_iy0[p] + t_ky * dil_h, ix = a_ix0[p] + t_kx * dil_w;
                const bool ok = kin && a_pix[p] >= 0 && iy >= 0 && iy < d.H && ix >= 0 && ix < d.W;
                const unsigned off = ok ? (unsigned)(((a_b[p] * d.H + iy) * d.W + ix) * d.ldx + t_c) * 4u : ST_OOB;
                ra[p] = buf_load16(rsrcA, off);
            }
#pragma unroll
            for (int p = 0; p < BP; ++p) {
                const int n = n0 + rrow + 32 * p;
                const bool ok = kin && n < d.N;
                const unsigned off = ok ? (unsigned)(n * d.ldw + k) * 4u : ST_OOB;
                rb[p] = buf_load16(rsrcW, off);
            }
        } else {
#pragma unroll
            for (int p = 0; p < AP; ++p) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int ke = k + e;
                    float x = 0.f;
                    if (a_pix[p] >= 0 && ke < K) {
                        const int kyx = ke / d.Cin, c = ke - kyx * d.Cin;
                        const int ky = kyx / d.kw, kx = kyx - ky * d.kw;
                        const int iy = a_iy0[p] + ky * dil_h, ix = a_ix0[p] + kx * dil_w;
                        if (iy >= 0 && iy < d.H && ix >= 0 && ix < d.W)
                            x = X[((size_t)(a_b[p] * d.H + iy) * d.W + ix) * d.ldx + c];
                    }
                    v[e] = x;
                }
                ra[p] = make_float4(v[0], v[1], v[2], v[3]);
            }
#pragma unroll
            for (int p = 0; p < BP; ++p) {
                const int n = n0 + rrow + 32 * p;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (n < d.N && k + e < K) ? Wt[(size_t)n * d.ldw + k + e] : 0.f;
                rb[p] = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int p = 0; p < AP; ++p)
            *reinterpret_cast<float4*>(As + ((size_t)buf * BM + rrow + 32 * p) * LDS_LD + kcol) = ra[p];
#pragma unroll
        for (int p = 0; p < BP; ++p)
            *reinterpret_cast<float4*>(Bs + ((size_t)buf * BN + rrow + 32 * p) * LDS_LD + kcol) = rb[p];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    f32x16 tot[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) tot[i][j][r] = 0.f;
    const int nkt_all = (K + BK - 1) / BK;
    const int per = (nkt_all + split - 1) / split;
    const int kt0 = kz * per;
    const int nkt = min(nkt_all, kt0 + per);
    const int li = lane & 31, lh = lane >> 5;
    if (kt0 < nkt) {
        load_tile(kt0);
        store_tile(kt0 & 1);
    }
    __syncthreads();
    for (int kt = kt0; kt < nkt; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nkt) load_tile(kt + 1);   // global loads in flight under the MFMAs
        const float* Ab = As + ((size_t)buf * BM + wm * TM * 32 + li) * LDS_LD + 4 * lh;
        const float* Bb = Bs + ((size_t)buf * BN + wn * TN * 32 + li) * LDS_LD + 4 * lh;
#pragma unroll
        for (int j = 0; j < BK / 8; ++j) {
            float4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const float4*>(Ab + i * 32 * LDS_LD + 8 * j);
#pragma unroll
            for (int i = 0; i < TN; ++i) bf[i] = *reinterpret_cast<const float4*>(Bb + i * 32 * LDS_LD + 8 * j);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int jn = 0; jn < TN; ++jn) {
                    acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].x, bf[jn].x, acc[i][jn], 0, 0, 0);
                    acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].y, bf[jn].y, acc[i][jn], 0, 0, 0);
                    acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].z, bf[jn].z, acc[i][jn], 0, 0, 0);
                    acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].w, bf[jn].w, acc[i][jn], 0, 0, 0);
                }
        }
        if (kt + 1 < nkt) store_tile(buf ^ 1);
        // K-blocked accumulation, same block boundaries as conv_gemm_dma_kernel (every 8 K steps = 256 k): see there
        if (((kt - kt0 + 1) & 7) == 0 && kt + 1 < nkt) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int jn = 0; jn < TN; ++jn) {
                    tot[i][jn] = tot[i][jn] + acc[i][jn];
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][jn][r] = 0.f;
                }
        }
        __syncthreads();
    }
    if (nkt - kt0 > 8) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int jn = 0; jn < TN; ++jn) acc[i][jn] = acc[i][jn] + tot[i][jn];
    }

    gemm_tile_epilogue<TM, TN>(d, C, acc, m0, n0, wm, wn, li, lh, split, kz);
}

// ---------------------------------------------------------------------------------------------
// Deep-pipelined variant of the same contraction: operand tiles go global -> LDS directly
// (buffer_load_dwordx4 ... lds, no VGPR staging, no ds_write), STAGES tiles deep, one raw s_barrier per
// K step with a counted s_waitcnt vmcnt so that STAGES-2 tiles stay in flight across every barrier.
// This is what keeps a workgroup's MFMAs fed when it is alone on its CU (the M = 8192 decoder GEMMs launch
// 256..512 workgroups): the register-staged kernel above can hold one tile in flight, whose L2 latency is
// longer than the 16 MFMAs of a K step.
//   LDS image of a stage: (BM + BN) rows x 128 B (32 k), unpadded -- one DMA wave-instruction writes 1 KiB
//   = 8 whole rows, lane l -> row l/8, 16-B slot l%8.  Bank conflicts are avoided by an XOR swizzle applied
//   on the SOURCE side: slot s of row r holds k-chunk s ^ ((r >> 1) & 7); the fragment reads
//   (32 rows x one chunk per ds_read_b128) then hit 16 distinct bank quads in each hardware lane group.
//   Out-of-image taps use an offset past the descriptor's num_records: the DMA writes zeros (probed on gfx950).
//   The DMA is issued from inline asm: hipcc treats the builtin form as a pending LDS write and puts
//   s_waitcnt vmcnt(0) in front of the next ds_read, which would drain the whole pipeline every K step.
// Preconditions (checked by the host): 16-B aligned operands, Cin % 32 == 0 (a K step never straddles taps).

// The K loop is written around one measured fact (tools/probes/mfma_gap.hip: v_mfma_f32_32x32x2_f32 shares the fp32 FMA
// datapath with the VALU): every VALU instruction issued between two MFMAs costs 4-8 cycles of matrix time
// (2 VALU per MFMA: 67 -> 89 cycles per MFMA at one wave per SIMD), while SALU (<= 4 per MFMA), ds_read and
// buffer_load...lds issue for free.  So the loop body contains NO per-tile VALU work:
//   - fragment reads use loop-invariant address VGPRs + immediate offsets (the loop is unrolled by STAGES so the
//     stage offset is a literal);
//   - DMA source addresses are loop-invariant VGPR offsets + an SGPR offset advanced on the SALU; the only VALU
//     left is the padding test, redone when the (ky, kx) tap changes (every Cin/32 tiles), never for 1x1;
//   - waits, barrier, loop control are scalar.
// PERSIST (plain matrices, K % (32*STAGES) == 0, no split-K): a workgroup walks M tiles g, g+G, g+2G, ... of its
// column tile with ONE continuous DMA ring, so the operand tiles of the next M tile stream in under the epilogue
// of the current one (short-K GEMMs -- K = 128 has four K steps per tile -- are otherwise all load latency).
template <int WM, int WN, int TM, int TN, int STAGES, bool PERSIST, bool CT = false>
__device__ __forceinline__ void conv_gemm_dma_body(const st_gemm_desc& d, const int block_id) {
    static_assert(WM * WN == 4, "4 waves per workgroup");
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32, ROWS = BM + BN;
    constexpr int PA = BM / 32, PB = BN / 32;      // 1-KiB pieces (8 rows x 128 B) per wave and K step
    constexpr int PPW = PA + PB;
    constexpr int STAGE_FLOATS = ROWS * 32;
    extern __shared__ __attribute__((aligned(1024))) float smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int split = d.split_k > 1 ? d.split_k : 1;
    const int bz = split > 1 ? 0 : blockIdx.z;
    const int kz = split > 1 ? blockIdx.z : 0;
    const float* __restrict__ X = d.a + (size_t)bz * d.batch_stride_a;
    const float* __restrict__ Wt = d.w + (size_t)bz * d.batch_stride_w;
    float* __restrict__ C = d.c + (size_t)bz * d.batch_stride_c;

    const int ntm = (d.M + BM - 1) / BM, ntn = (d.N + BN - 1) / BN;
    const int nwg = PERSIST ? (int)gridDim.x : ntm * ntn;
    int bid = block_id;
    {
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int tile_n = bid % ntn, tile_m = bid / ntn;        // PERSIST: tile_m = first M tile, stride G
    const int G = PERSIST ? nwg / ntn : 1;
    const int nmt = PERSIST ? (ntm - tile_m + G - 1) / G : 1;
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    const i32x4 rsrcA = make_rsrc(X, d.a_bytes), rsrcW = make_rsrc(Wt, d.w_bytes);
    // optional second A source (same geometry): channels below a2_channels come from it -- a wave-uniform descriptor
    // choice per issued piece, on the SALU
    const i32x4 rsrcA2 = make_rsrc(d.a2 ? d.a2 : X, d.a_bytes);
    const int a2c = (!PERSIST && d.a2) ? d.a2_channels : 0;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) float*)smem;   // LDS byte address

    // staging slots of this lane: wave w stages A rows [8*PA*w, 8*PA*(w+1)) and B rows [8*PB*w, 8*PB*(w+1)),
    // 8 rows per piece, lane l -> row l/8 of the piece, 16-B slot l%8 holding k-chunk (l%8) ^ ((row>>1)&7)
    int a_base[PA], a_iy0[PA], a_ix0[PA];
    unsigned voffA[PA], voffB[PB];
    auto set_mtile = [&](int mbase) {               // per-lane decomposition (image, oy, ox) of the A rows of the M tile starting at mbase
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            const int r = 8 * (wave * PA + i) + (lane >> 3);
            const int chunk4 = (((lane & 7) ^ ((r >> 1) & 7)) << 2);
            const int m = min(mbase + r, d.M - 1);                              // rows past M: any valid row (never stored)
            const int hw = d.Ho * d.Wo;
            const int b = m / hw, rr = m - b * hw;
            const int oy = rr / d.Wo, ox = rr - oy * d.Wo;
            a_iy0[i] = oy * d.sh - d.ph; a_ix0[i] = ox * d.sw - d.pw;
            a_base[i] = ((b * d.H + a_iy0[i]) * d.W + a_ix0[i]) * d.ldx + chunk4;
        }
    };
    set_mtile(m0);
    // PERSIST walks plain matrices only (rows are contiguous: set_rows).  (Round 5 also let convolutions walk that way, re-deriving the tap
    // addresses at every M-tile change: measured -1.9 % in the product, DESIGN.md section 5, and removed again in round 6 -- ADVICE r5.)
#pragma unroll
    for (int i = 0; i < PB; ++i) {
        const int r = 8 * (wave * PB + i) + (lane >> 3);                    // row inside the B part; BM % 16 == 0
        const int chunk4 = (((lane & 7) ^ ((r >> 1) & 7)) << 2);
        voffB[i] = (unsigned)(min(n0 + r, d.N - 1) * d.ldw + chunk4) * 4u;
    }

    const int nkt_all = d.K / 32;
    const int per = (nkt_all + split - 1) / split;
    const int kt0 = kz * per;
    const int nkt = min(nkt_all, kt0 + per) - kt0;          // K steps per output tile
    const int ntiles = PERSIST ? nmt * nkt : nkt;           // flat (M tile, K step) sequence of this workgroup

    // wave-uniform state of the next tile to issue: tap (ky, kx), channel offset c0; byte offsets for the SGPR operand
    int i_c0, i_ky, i_kx, i_kt = 0, i_m0 = m0;
    {
        const int k = kt0 * 32, tap = k / d.Cin;
        i_c0 = k - tap * d.Cin; i_ky = tap / d.kw; i_kx = tap - i_ky * d.kw;
    }
    unsigned soffA = (unsigned)i_c0 * 4u, soffB = (unsigned)kt0 * 128u;
    auto set_tap = [&]() {                          // per-lane source offsets of the A pieces for tap (i_ky, i_kx)
        const int ty = i_ky * (d.dh > 1 ? d.dh : 1), tx = i_kx * (d.dw > 1 ? d.dw : 1);      // dilated tap offset
        const int tapbase = (ty * d.W + tx) * d.ldx;
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            const bool ok = (unsigned)(a_iy0[i] + ty) < (unsigned)d.H && (unsigned)(a_ix0[i] + tx) < (unsigned)d.W;
            voffA[i] = ok ? (unsigned)(a_base[i] + tapbase) * 4u : ST_OOB;
        }
    };
    auto set_rows = [&]() {                         // PERSIST: A rows of the M tile starting at i_m0 (plain matrix)
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            const int r = 8 * (wave * PA + i) + (lane >> 3);
            voffA[i] = (unsigned)(min(i_m0 + r, d.M - 1) * d.ldx + (((lane & 7) ^ ((r >> 1) & 7)) << 2)) * 4u;
        }
    };
    if (PERSIST) set_rows(); else set_tap();
    auto issue_a = [&](int stage, int i) {
        lds_dma16(i_c0 < a2c ? rsrcA2 : rsrcA, lds0 + (unsigned)(stage * STAGE_FLOATS + (wave * PA + i) * 256) * 4u, voffA[i], soffA);
    };
    auto issue_b = [&](int stage, int i) {
        lds_dma16(rsrcW, lds0 + (unsigned)(stage * STAGE_FLOATS + BM * 32 + (wave * PB + i) * 256) * 4u, voffB[i], soffB);
    };
    auto advance = [&]() {                          // scalar, except the address refresh at a tap / M-tile change
        soffB += 128u; soffA += 128u;
        if (PERSIST) {
            if (++i_kt == nkt) {
                i_kt = 0; soffA = 0; soffB = 0; i_m0 += G * BM;
                set_rows();
            }
        } else {
            i_c0 += 32;
            if (i_c0 >= d.Cin) {
                i_c0 = 0; soffA = 0;
                if (++i_kx == d.kw) { i_kx = 0; ++i_ky; }
                set_tap();
            }
        }
    };
    // wait until at most `tiles` whole tiles of this wave's DMA pieces are still in flight (wave-uniform)
    auto wait_tiles = [&](int tiles) {
        if (tiles >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * PPW) : "memory");
        else if (tiles == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PPW) : "memory");
        else if (tiles == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPW) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // K-blocked accumulation: one fmaf chain over all of K has a rounding error that grows like sqrt(K); the reference's
    // CPU GEMM (MKL) accumulates in K blocks of a few hundred, and at K >= 512 a single chain is measurably worse than it
    // (rms 5.7e-7 vs 3.4e-7 at K = 1024, 8.6e-7 vs 3.1e-7 at K = 2304; profiles/r2_parity_trace_*.txt).  So the chain is
    // cut every KBLK K steps (256 k): the running tile is folded into `tot` and restarted from zero.  16 v_add per
    // 32x32 sub-tile every 128 MFMAs; K <= 256 never folds.
    constexpr int KBLK = 8;                         // K steps per block (256 k), whatever the ring depth
    f32x16 tot[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) tot[i][j][r] = 0.f;
    auto fold = [&]() {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                tot[i][j] = tot[i][j] + acc[i][j];
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
            }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto unfold = [&]() {                           // result of a blocked tile back into acc (epilogue operand)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                acc[i][j] = acc[i][j] + tot[i][j];
#pragma unroll
                for (int r = 0; r < 16; ++r) tot[i][j][r] = 0.f;
            }
        __builtin_amdgcn_sched_barrier(0);
    };

    const int li = lane & 31, lh = lane >> 5;
    const int swz = (li >> 1) & 7;
    // loop-invariant fragment pointers (one per 8-k step: the XOR swizzle is lane dependent); stage / sub-tile
    // offsets are literals folded into the ds_read offset field
    const float* pa[4];
    const float* pb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int foff = ((2 * j + lh) ^ swz) << 2;
        pa[j] = smem + (wm * TM * 32 + li) * 32 + foff;
        pb[j] = smem + (BM + wn * TN * 32 + li) * 32 + foff;
    }

    float4 fa[2][TM], fb[2][TN];                   // fragment ping-pong: step j+1 is read under the MFMAs of step j
    auto read_frags = [&](int buf, int stage, int j) {
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[buf][i] = *reinterpret_cast<const float4*>(pa[j] + stage * STAGE_FLOATS + i * 1024);
#pragma unroll
        for (int i = 0; i < TN; ++i) fb[buf][i] = *reinterpret_cast<const float4*>(pb[j] + stage * STAGE_FLOATS + i * 1024);
    };
    auto comp = [](const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; };
    auto mfma_k = [&](int buf, int e) {            // the TM*TN MFMAs of one k (k = 8j + 4*lane_half + e)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int jn = 0; jn < TN; ++jn)
                acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(comp(fa[buf][i], e), comp(fb[buf][jn], e), acc[i][jn], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
#define ST_GAP(stmt) do { stmt; __builtin_amdgcn_sched_barrier(0); } while (0)

    // epilogue operands are fetched ahead of the K loop (ordinary loads, older than every DMA of the ring: the
    // counted vmcnt waits below only ever over-wait because of them)
    EpiOperands<TM, TN> eop;
    gemm_epilogue_consts<TM, TN>(d, eop, n0, wn, li, split);                 // once per workgroup (also for every M tile of PERSIST)
    if (!PERSIST) gemm_epilogue_load<TM, TN>(d, eop, m0, n0, wm, wn, li, lh, split);
    __builtin_amdgcn_sched_barrier(0);

    if (ntiles > 0) {
#pragma unroll
        for (int t = 0; t < STAGES - 1; ++t)
            if (t < ntiles) {
#pragma unroll
                for (int i = 0; i < PA; ++i) issue_a(t, i);
#pragma unroll
                for (int i = 0; i < PB; ++i) issue_b(t, i);
                advance();
            }
        wait_tiles(min(STAGES - 2, ntiles - 1));    // tile 0 landed (this wave's pieces) ...
        asm volatile("s_barrier" ::: "memory");     // ... and everybody else's
        read_frags(0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        // one tile: stage s (literal), tile index t.  FULL = steady state (tile t+STAGES-1 exists): no branches at all.
        auto tile_body = [&](auto full_c, int s, int t) {
            constexpr bool FULL = decltype(full_c)::value;
            const bool more = FULL || t + 1 < ntiles, feed = FULL || t + STAGES - 1 < ntiles;
            const int fstage = (s + STAGES - 1) % STAGES, nstage = (s + 1) % STAGES;
            // ---- k-step 0 (fragments in buffer 0)
            mfma_k(0, 0); ST_GAP(read_frags(1, s, 1));
            mfma_k(0, 1);
            // tile t+1 has landed everywhere and every wave is past tile t-1, whose stage is therefore free
            if (FULL) ST_GAP(wait_tiles(STAGES - 3); asm volatile("s_barrier" ::: "memory"));
            else ST_GAP(if (more) { wait_tiles(min(STAGES - 3, ntiles - 2 - t)); asm volatile("s_barrier" ::: "memory"); });
            mfma_k(0, 2); ST_GAP(if (feed) issue_a(fstage, 0));
            mfma_k(0, 3); ST_GAP(if (feed) { _Pragma("unroll") for (int i = 1; i < PA; ++i) issue_a(fstage, i); });
            // ---- k-step 1 (buffer 1)
            mfma_k(1, 0); ST_GAP(read_frags(0, s, 2));
            mfma_k(1, 1); ST_GAP(if (feed) issue_b(fstage, 0));
            mfma_k(1, 2); ST_GAP(if (feed) { _Pragma("unroll") for (int i = 1; i < PB; ++i) issue_b(fstage, i); });
            mfma_k(1, 3); ST_GAP(if (feed) advance());
            // ---- k-step 2 (buffer 0)
            mfma_k(0, 0); ST_GAP(read_frags(1, s, 3));
            mfma_k(0, 1); mfma_k(0, 2); mfma_k(0, 3);
            // ---- k-step 3 (buffer 1); step 0 of the next tile is read under it (a stale read after the last tile)
            mfma_k(1, 0); ST_GAP(read_frags(0, nstage, 0));
            mfma_k(1, 1); mfma_k(1, 2); mfma_k(1, 3);
            if (STAGES != 4 && (t & (KBLK - 1)) == KBLK - 1 && t + 1 < ntiles) fold();    // (4-deep ring: folded by the callers, at block ends)
        };
        // (round 4 measured ONE barrier per two K steps -- the ring used in stage pairs, an even tile issuing the whole next pair's DMA, the odd
        // tile closing the pair with vmcnt(0) + s_barrier: bit-identical, 81.85 -> 81.65 pairs/s and 72.0 -> 71.2 with one pair in flight: what
        // this loop waits for is the DMA's distance ahead (3 tiles here, 2 in the pair scheme), not the barrier itself)
        if (PERSIST) {
            for (int mt = 0; mt < nmt; ++mt) {
                gemm_epilogue_load<TM, TN>(d, eop, (tile_m + mt * G) * BM, n0, wm, wn, li, lh, 1);   // lands under the MFMAs
                __builtin_amdgcn_sched_barrier(0);
                for (int tb = mt * nkt, kb = STAGES; tb < (mt + 1) * nkt; tb += STAGES, kb += STAGES) {    // nkt % STAGES == 0: stage == s
                    if (tb + 2 * STAGES - 1 <= ntiles) {
#pragma unroll
                        for (int s = 0; s < STAGES; ++s) tile_body(st_true{}, s, tb + s);
                    } else {
#pragma unroll
                        for (int s = 0; s < STAGES; ++s) tile_body(st_false{}, s, tb + s);
                    }
                    if (kb % KBLK == 0 && kb < nkt) fold();
                }
                if (nkt > KBLK) unfold();
                gemm_epilogue_store<TM, TN, false, CT>(d, C, acc, eop, (tile_m + mt * G) * BM, n0, wm, wn, li, lh, 1, 0);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
            }
        } else {
            int tb = 0;
            for (; tb + 2 * STAGES - 1 <= ntiles; tb += STAGES) {       // every tile of the block still feeds a new one
#pragma unroll
                for (int s = 0; s < STAGES; ++s) tile_body(st_true{}, s, tb + s);
                if (STAGES == 4 && (tb + STAGES) % KBLK == 0) fold();
            }
            for (; tb < ntiles; tb += STAGES) {
#pragma unroll
                for (int s = 0; s < STAGES; ++s)
                    if (tb + s < ntiles) tile_body(st_false{}, s, tb + s);
                if (STAGES == 4 && (tb + STAGES) % KBLK == 0 && tb + STAGES < ntiles) fold();
            }
            if (ntiles > KBLK) unfold();
        }
    }
#undef ST_GAP

    if (!PERSIST) gemm_epilogue_store<TM, TN, false, CT>(d, C, acc, eop, m0, n0, wm, wn, li, lh, split, kz);
}

template <int WM, int WN, int TM, int TN, int STAGES, bool PERSIST, bool CT = false>
__global__ __launch_bounds__(256) void conv_gemm_dma_kernel(const st_gemm_desc d) {
    conv_gemm_dma_body<WM, WN, TM, TN, STAGES, PERSIST, CT>(d, (int)blockIdx.x);
}

template <int WM, int WN, int TM, int TN, int STAGES>
__global__ __launch_bounds__(256) void conv_gemm_dma_pair_kernel(const st_gemm_pair_args g) {
    const bool second = (int)blockIdx.x >= g.tiles0;             // workgroup-uniform
    conv_gemm_dma_body<WM, WN, TM, TN, STAGES, false>(second ? g.d[1] : g.d[0], second ? (int)blockIdx.x - g.tiles0 : (int)blockIdx.x);
}

// ---------------------------------------------------------------------------------------------
// Row-streaming GEMM for the short-K linears (K = 64 / 128: the Twins / latent / vertical-layer linears at
// M = 32768 ... 524288: twins.py:253-304,336-392,785, encoder.py:156-172, crossattentionlayer.py:37-56).  Those shapes are
// MFMA-bound and HBM-bound at once (64 MFMAs per 64x64 tile against 48 KB of traffic), so the tiled kernels pay for
// every barrier and for fetching A once per column tile.  Here:
//   - the weight slice of the workgroup (<= 8 chunks of 32 columns x K) is staged into LDS ONCE and stays there
//     ([n][K + 4] padded rows: the 16 lanes of a ds_read_b128 group hit 16 distinct bank quads), with its bias;
//   - a wave owns whole 32-row blocks of A and keeps a block in REGISTERS (K / 2 floats per lane, loaded straight from
//     global memory with 16-byte buffer loads; lane (li, lh) holds k = 8j + 4lh + t of row li -- the same k pairing and
//     the same summation order as the tiled kernels, so results are bit-identical to theirs); for K <= 128 the next
//     block is prefetched under the MFMAs of the current one (in two halves, each issued AFTER the epilogue operand
//     loads of its chunk: vmcnt retires in order, so an epilogue must never have to wait for the prefetch);
//   - so the main loop has no barrier, no LDS traffic for A, and each wave runs independently: for every 32-column
//     chunk, K/2 MFMAs fed by K/8 ds_read_b128, then the shared epilogue (a half-chunk start delay for waves 4-7, so
//     that the two waves of a SIMD do not run their epilogues side by side, was measured neutral to slightly worse);
//   - because a lane pair holds a complete row, LayerNorm of the A rows (d.a_ln) is two in-register reductions and one
//     cross-half exchange: the LayerNorm kernel in front of these linears, its write and its re-read disappear.
// Column slices (more chunks than a workgroup keeps, or too few row blocks to give every wave one) are separate
// workgroups that walk the same rows; the slices of a row group get block ids that land on the same XCD (shared L2).
template <int KC, bool PREFETCH>
__global__ __launch_bounds__(512) void rowstream_gemm_kernel(const st_gemm_desc d, const int chunks_per_slice, const int nslices) {
    constexpr int K = 32 * KC, LDW = K + 4, NJ = 4 * KC, NW = 8;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int S = nslices, G = (int)gridDim.x / S;
    const int q = (int)blockIdx.x >> 3, xcd = (int)blockIdx.x & 7;
    const int sl = q % S, g = (q / S) * 8 + xcd;                 // slice, workgroup index inside the slice (0 .. G-1)
    const int n_base = sl * chunks_per_slice * 32;
    const int ncols = min(d.N - n_base, chunks_per_slice * 32);
    const int nch = (ncols + 31) >> 5;
    const int nblk = (d.M + 31) >> 5;
    const int stride = G * NW;
    float* bias_lds = smem + chunks_per_slice * 32 * LDW;

    const __amdgpu_buffer_rsrc_t rsrcA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.a), 0, (int)d.a_bytes, 0x00020000);
    auto row_off = [&](int blk) {
        const int row = blk * 32 + li;
        return (blk < nblk && row < d.M) ? (unsigned)(row * d.ldx + 4 * lh) * 4u : ST_OOB;
    };
    int blk = g * NW + wave;
    float4 a[NJ], an[PREFETCH ? NJ : 1];
    {
        const unsigned off = row_off(blk);                       // in flight while the weight slice is staged
#pragma unroll
        for (int j = 0; j < NJ; ++j) a[j] = buf_load16(rsrcA, off + 32u * j);
    }
    {
        // weight slice -> LDS, 8 float4 per thread in flight at a time
        const int total = nch * 32 * (K / 4);
        for (int f0 = 0; f0 < total; f0 += 512 * 8) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int f = f0 + u * 512 + tid, r = f / (K / 4), c4 = f - r * (K / 4);
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (f < total && r < ncols) v[u] = *reinterpret_cast<const float4*>(d.w + (size_t)(n_base + r) * d.ldw + c4 * 4);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int f = f0 + u * 512 + tid, r = f / (K / 4), c4 = f - r * (K / 4);
                if (f < total) *reinterpret_cast<float4*>(smem + r * LDW + c4 * 4) = v[u];
            }
        }
        if (tid < nch * 32) bias_lds[tid] = (d.bias && tid < ncols) ? d.bias[n_base + tid] : 0.f;
    }
    const float sc = d.scale_ptr ? *d.scale_ptr : 1.0f;
    __syncthreads();

    const float* wl = smem + li * LDW + 4 * lh;
    EpiOperands<1, 1> e;
    e.sc = sc;
    for (; blk < nblk; blk += stride) {
        const int m0 = blk * 32;
        const unsigned noff = PREFETCH ? row_off(blk + stride) : 0u;
        if (d.a_ln) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) s += (a[j].x + a[j].y) + (a[j].z + a[j].w);
            s += __shfl_xor(s, 32, 64);
            const float mean = s * (1.0f / K);
            float v = 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                a[j].x -= mean; a[j].y -= mean; a[j].z -= mean; a[j].w -= mean;
                v += (a[j].x * a[j].x + a[j].y * a[j].y) + (a[j].z * a[j].z + a[j].w * a[j].w);
            }
            v += __shfl_xor(v, 32, 64);
            const float rstd = 1.0f / sqrtf(v * (1.0f / K) + d.a_ln_eps);
#pragma unroll
            for (int j = 0; j < NJ; ++j) { a[j].x *= rstd; a[j].y *= rstd; a[j].z *= rstd; a[j].w *= rstd; }
        }
        for (int c = 0; c < nch; ++c) {
            const int n0 = n_base + c * 32;
            e.bv[0] = bias_lds[c * 32 + li];
            gemm_epilogue_load<1, 1, true>(d, e, m0, n0, 0, 0, li, lh, 1);
            if (PREFETCH) {
                if (c == 0) {
#pragma unroll
                    for (int j = 0; j < NJ / 2; ++j) an[j] = buf_load16(rsrcA, noff + 32u * j);
                }
                if (c == 1 || nch == 1) {
#pragma unroll
                    for (int j = NJ / 2; j < NJ; ++j) an[PREFETCH ? j : 0] = buf_load16(rsrcA, noff + 32u * j);
                }
            }
            f32x16 acc[1][1];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.f;
            const float* wb = wl + c * 32 * LDW;
            float4 b = *reinterpret_cast<const float4*>(wb);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                // the fragment of step j+1 is read under the MFMAs of step j
                const float4 bn = *reinterpret_cast<const float4*>(wb + 8 * (j + 1 < NJ ? j + 1 : j));
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].x, b.x, acc[0][0], 0, 0, 0);
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].y, b.y, acc[0][0], 0, 0, 0);
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].z, b.z, acc[0][0], 0, 0, 0);
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].w, b.w, acc[0][0], 0, 0, 0);
                b = bn;
                __builtin_amdgcn_sched_barrier(0);
            }
            gemm_epilogue_store<1, 1, true>(d, d.c, acc, e, m0, n0, 0, 0, li, lh, 1, 0);
        }
        if (PREFETCH) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) a[j] = an[j];
        } else if (blk + stride < nblk) {
            const unsigned off = row_off(blk + stride);
#pragma unroll
            for (int j = 0; j < NJ; ++j) a[j] = buf_load16(rsrcA, off + 32u * j);
        }
    }
}

// split-K tail: sum the K-slice slabs [split][M][N] in slice order (deterministic) + epilogue.
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const st_gemm_desc d) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)d.M * d.N) return;
    const int m = idx / d.N, n = idx % d.N;
    float acc = 0.f;
    for (int z = 0; z < d.split_k; ++z) acc += d.workspace[((size_t)z * d.M + m) * d.N + n];
    const float sc = d.scale_ptr ? *d.scale_ptr : 1.0f;
    gemm_store(d, d.c, m, n, acc, sc);
}
void splitk_reduce_launch(const st_gemm_desc& d, hipStream_t s) {
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(((size_t)d.M * d.N + 255) / 256), dim3(256), 0, s, d);
}

// Skinny GEMM (M <= 8 rows, e.g. the batch-1 regression head): weight-read bound, one wave per
// output column, K split across the lanes with 16-B loads, wave-shuffle reduction.
template <int MR>
__global__ __launch_bounds__(256) void skinny_gemm_kernel(const st_gemm_desc d) {
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= d.N) return;
    const float* w = d.w + (size_t)wave * d.ldw;
    float acc[MR];
#pragma unroll
    for (int m = 0; m < MR; ++m) acc[m] = 0.f;
    for (int k = lane * 4; k < d.K; k += 256) {
        const float4 wv = *reinterpret_cast<const float4*>(w + k);
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            if (m < d.M) {
                const float4 av = *reinterpret_cast<const float4*>(d.a + (size_t)m * d.ldx + k);
                acc[m] = fmaf(av.x, wv.x, acc[m]); acc[m] = fmaf(av.y, wv.y, acc[m]);
                acc[m] = fmaf(av.z, wv.z, acc[m]); acc[m] = fmaf(av.w, wv.w, acc[m]);
            }
        }
    }
#pragma unroll
    for (int m = 0; m < MR; ++m) acc[m] = wave_sum(acc[m]);
    if (lane == 0) {
        const float bv = d.bias ? d.bias[wave] : 0.f;
        for (int m = 0; m < d.M && m < MR; ++m) d.c[(size_t)m * d.ldc + wave] = st_act(acc[m] * d.alpha + bv, d.act);
    }
}

// Very narrow outputs (N <= 4: the flow head's 2-channel 3x3 conv, gru.py:5-13): an MFMA tile would be > 90 % padding.
// One wave per output pixel; lanes stride the channels of each tap with float4 loads, N running dot products,
// one wave reduction at the end.  Pure L2 bandwidth (every input row is re-read kh*kw times).
template <int NMAX>
__global__ __launch_bounds__(256) void narrow_conv_kernel(const st_gemm_desc d) {
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (m >= d.M) return;
    const int hw = d.Ho * d.Wo;
    const int b = m / hw, rr = m - b * hw;
    const int oy = rr / d.Wo, ox = rr - oy * d.Wo;
    float acc[NMAX];
#pragma unroll
    for (int n = 0; n < NMAX; ++n) acc[n] = 0.f;
    for (int ky = 0; ky < d.kh; ++ky) {
        const int iy = oy * d.sh - d.ph + ky * (d.dh > 1 ? d.dh : 1);
        if (iy < 0 || iy >= d.H) continue;
        for (int kx = 0; kx < d.kw; ++kx) {
            const int ix = ox * d.sw - d.pw + kx * (d.dw > 1 ? d.dw : 1);
            if (ix < 0 || ix >= d.W) continue;
            const float* xr = d.a + ((size_t)(b * d.H + iy) * d.W + ix) * d.ldx;
            const float* wr = d.w + (size_t)(ky * d.kw + kx) * d.Cin;
            for (int c = lane * 4; c < d.Cin; c += 256) {
                const float4 xv = *reinterpret_cast<const float4*>(xr + c);
#pragma unroll
                for (int n = 0; n < NMAX; ++n) {
                    if (n < d.N) {
                        const float4 wv = *reinterpret_cast<const float4*>(wr + (size_t)n * d.ldw + c);
                        acc[n] = fmaf(xv.x, wv.x, acc[n]); acc[n] = fmaf(xv.y, wv.y, acc[n]);
                        acc[n] = fmaf(xv.z, wv.z, acc[n]); acc[n] = fmaf(xv.w, wv.w, acc[n]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int n = 0; n < NMAX; ++n) acc[n] = wave_sum(acc[n]);
    if (lane == 0) {
        const float sc = d.scale_ptr ? *d.scale_ptr : 1.0f;
        for (int n = 0; n < d.N && n < NMAX; ++n) d.c[(size_t)m * d.ldc + n] = gemm_epilogue(d, m, n, acc[n], sc);
    }
}

// The flow head's second conv (gru.py:5-13: Conv2d(256, 2, 3, padding=1)) and its like: 3x3, stride 1, pad 1, Cin = 256,
// N <= 2.  A lane owns 4 input channels and keeps its 9 x N weight quads in registers; a wave produces 8 consecutive
// output pixels of one image row: per kernel row it loads the 10 input pixels it needs once (whole 1-KiB channel
// rows), 9 x 8 x N dot-4 updates, then ONE transposing butterfly reduces the 8 x N partial sums across the wave
// (17 shuffles instead of 6 per value).  Input pixels are fetched 30 times per wave instead of 72, weights once
// instead of once per pixel (narrow_conv_kernel: 17 us at M = 8192; this: ~5 us).
template <int NOUT>
__global__ __launch_bounds__(256) void narrow_conv3x3_kernel(const st_gemm_desc d) {
    constexpr int NV = 8 * NOUT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int segs = (d.W + 7) >> 3;
    const int wid = blockIdx.x * 4 + wave;
    const int nimg = d.M / (d.H * d.W);
    if (wid >= nimg * d.H * segs) return;
    const int b = wid / (d.H * segs), r = wid - b * d.H * segs;
    const int y = r / segs, x0 = (r - y * segs) * 8;
    const __amdgpu_buffer_rsrc_t rsrcW = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.w), 0, (int)d.w_bytes, 0x00020000);
    float4 wv[NOUT][9];
#pragma unroll
    for (int n = 0; n < NOUT; ++n)
#pragma unroll
        for (int t = 0; t < 9; ++t)
            wv[n][t] = buf_load16(rsrcW, n < d.N ? (unsigned)(n * d.ldw + t * 256 + 4 * lane) * 4u : ST_OOB);   // (a conditional global load made
    //                                                       hipcc wait for each of the 18 loads in turn: 18 dependent L2 round trips per wave)
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
    // all 30 input rows are requested before the first is used (raw buffer loads: a tap outside the image gets an offset past
    // num_records and reads zeros, so there is no branch between the loads): one memory round trip per wave instead of three
    // dependent ones -- with one wave per SIMD nothing else hides them
    const __amdgpu_buffer_rsrc_t rsrcA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.a), 0, (int)d.a_bytes, 0x00020000);
    float4 in[3][10];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = y + ky - 1;
        const bool yok = iy >= 0 && iy < d.H;
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            const int ix = x0 - 1 + i;
            const unsigned off = (yok && ix >= 0 && ix < d.W) ? (unsigned)(((b * d.H + iy) * d.W + ix) * d.ldx + 4 * lane) * 4u : ST_OOB;
            in[ky][i] = buf_load16(rsrcA, off);
        }
    }
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
            for (int p = 0; p < 8; ++p)
#pragma unroll
                for (int n = 0; n < NOUT; ++n) {
                    const float4 xv = in[ky][p + kx], w4 = wv[n][ky * 3 + kx];
                    float a = acc[p * NOUT + n];
                    a = fmaf(xv.x, w4.x, a); a = fmaf(xv.y, w4.y, a); a = fmaf(xv.z, w4.z, a); a = fmaf(xv.w, w4.w, a);
                    acc[p * NOUT + n] = a;
                }
    // transposing butterfly: each step halves the number of values a lane carries; after log2(NV) steps lane l holds the
    // 64 / NV-lane partial sum of value v(l), v's bits taken from the lane bits used so far (high bits first)
    int cnt = NV / 2;
#pragma unroll
    for (int s = 32; cnt >= 1; s >>= 1, cnt >>= 1) {
        const bool hi = lane & s;
#pragma unroll
        for (int i = 0; i < NV / 2; ++i)
            if (i < cnt) {
                const float send = hi ? acc[i] : acc[i + cnt], keep = hi ? acc[i + cnt] : acc[i];
                acc[i] = keep + __shfl_xor(send, s, 64);
            }
    }
    constexpr int STEPS = NOUT == 1 ? 3 : NOUT == 2 ? 4 : 5;          // log2(NV)
    float v = acc[0];
#pragma unroll
    for (int s = 32 >> STEPS; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    if ((lane & ((64 >> STEPS) - 1)) == 0) {
        int idx = 0, c = NV / 2;
#pragma unroll
        for (int s = 32; c >= 1; s >>= 1, c >>= 1) idx += (lane & s) ? c : 0;
        const int p = idx / NOUT, n = idx - p * NOUT;
        const int x = x0 + p;
        if (x < d.W && n < d.N) {
            const int m = (b * d.H + y) * d.W + x;
            const float sc = d.scale_ptr ? *d.scale_ptr : 1.0f;
            d.c[(size_t)m * d.ldc + n] = gemm_epilogue(d, m, n, v, sc);
        }
    }
}


template <int WARPS_M, int WARPS_N, int TM, int TN>
static int launch_cfg(const st_gemm_desc& d, bool vec, hipStream_t s) {
    constexpr int BM = WARPS_M * TM * 32, BN = WARPS_N * TN * 32;
    const int ntm = (d.M + BM - 1) / BM, ntn = (d.N + BN - 1) / BN;
    dim3 grid(ntm * ntn, 1, d.split_k > 1 ? d.split_k : (d.batch > 0 ? d.batch : 1));
    const size_t lds = (size_t)2 * (BM + BN) * LDS_LD * sizeof(float);
    if (vec) {
        auto k = conv_gemm_kernel<WARPS_M, WARPS_N, TM, TN, true>;
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k, grid, dim3(256), lds, s, d);
    } else {
        auto k = conv_gemm_kernel<WARPS_M, WARPS_N, TM, TN, false>;
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k, grid, dim3(256), lds, s, d);
    }
    if (d.split_k > 1) splitk_reduce_launch(d, s);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

static const int f32_bms[6] = {0, 128, 128, 64, 128, 64}, f32_bns[6] = {0, 128, 64, 64, 32, 128};      // tile by tile_cfg (register-staged 1-4) or tile_cfg - 10 (LDS-DMA 12-15)
#define DMA_STAGES 4            // ring depth of every LDS-DMA instantiation launch_f32 uses
// 512 workgroup slots = both of a CU's slots for the LDS-DMA kernel's footprint.  One slot per CU (a workgroup walking >= 2 M tiles, the second slot
// left to another stream's kernel) was measured in round 5 and not adopted: faster on uniform GEMMs alone, slower in the product (bench.py,
// 3 pairs in flight, same box A/B/A: 82.66 / 82.58 -> 81.09 / 80.67 pairs/s; one pair in flight 72.4 -> 69.0).
#define DMA_SLOTS 512
template <int WM, int WN, int TM, int TN, int STAGES>
static int launch_dma(const st_gemm_desc& d, bool persist, hipStream_t s) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const int ntm = (d.M + BM - 1) / BM, ntn = (d.N + BN - 1) / BN;
    const int batch = d.batch > 0 ? d.batch : 1;
    const size_t lds = (size_t)STAGES * (BM + BN) * 32 * sizeof(float);
    const int slots = DMA_SLOTS / batch;
    if (persist) {                                  // persistent walk over M tiles (plan_f32)
        int G = slots / ntn;
        if (G > ntm) G = ntm;
        auto k = d.c_t ? conv_gemm_dma_kernel<WM, WN, TM, TN, STAGES, true, true> : conv_gemm_dma_kernel<WM, WN, TM, TN, STAGES, true>;
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k, dim3(G * ntn, 1, batch), dim3(256), lds, s, d);
        ST_CHECK_LAUNCH();
        return ST_OK;
    }
    dim3 grid(ntm * ntn, 1, d.split_k > 1 ? d.split_k : batch);
    auto k = d.c_t ? conv_gemm_dma_kernel<WM, WN, TM, TN, STAGES, false, true> : conv_gemm_dma_kernel<WM, WN, TM, TN, STAGES, false>;
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, grid, dim3(256), lds, s, d);
    if (d.split_k > 1) splitk_reduce_launch(d, s);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// row-streaming kernel: S column slices of `cps` 32-column chunks, G workgroups (512 threads, one per CU) per slice.
// S is the smallest power of two that (a) keeps a slice within `max_cps` chunks and (b) yields at least one (row block,
// slice) item per wave of the chip; G * S = 256, G a multiple of 8 (one run of workgroups per XCD).
// (the slicing is host arithmetic only: plan_f32 runs it to reject what no slicing fits, the launcher to size its grid)
static int rowstream_slices(const st_gemm_desc& d, int KC, int& cps, int& S) {
    const int nchunks = (d.N + 31) / 32, nblk = (d.M + 31) / 32;
    const int lds_cap = (160 * 1024 - 1024) / (32 * (32 * KC + 4) * 4);
    const int max_cps = lds_cap < 8 ? lds_cap : 8;      // 8-chunk slices (4-chunk ones, which would let a 64-KiB GEMM workgroup co-reside, measured 0.3 % slower with 3 pairs in flight)
    S = 1;
    while (S < 32 && ((nchunks + S - 1) / S > max_cps || ((long)nblk * S < 2048 && 2 * S <= nchunks))) S *= 2;
    cps = (nchunks + S - 1) / S;
    if (cps > lds_cap) return ST_EINVAL;
    S = (nchunks + cps - 1) / cps;                 // drop empty slices
    return ST_OK;
}

template <int KC>
static int launch_rowstream(const st_gemm_desc& d, hipStream_t s) {
    const int nblk = (d.M + 31) / 32;
    int cps, S;
    if (rowstream_slices(d, KC, cps, S)) return ST_EINVAL;
    int G = (256 / S) / 8 * 8;                      // (G * S <= 256)
    if (G < 8) G = 8;
    const int need = ((nblk + 7) / 8 + 7) / 8 * 8;
    if (G > need) G = need;
    const size_t lds = ((size_t)cps * 32 * (32 * KC + 4) + cps * 32) * sizeof(float);
    auto k = rowstream_gemm_kernel<KC, true>;
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, dim3(G * S), dim3(512), lds, s, d, cps, S);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// ---- fp32 dispatch: check, chunk if needed, plan, launch -- the first three without a HIP call, so st_gemm_plan answers from the same code ----
// The fp32 path's own rules on top of desc_common_check.  `chunked`: the rows must run in pieces (for_each_row_chunk).
static int check_f32(const st_gemm_desc& d, bool& chunked) {
    // a_ln belongs to the row-streaming kernel, c_t to the LDS-DMA kernels (plan_f32 would refuse the combination as well; the rule stays where it was)
    if (!desc_common_check(d) || (d.c_t && d.a_ln)) return ST_EINVAL;
    const f32_extent e = desc_f32_extent(d);
    if (e.w_bytes >= (int64_t)ST_OOB) return ST_EINVAL;         // (W is never cut)
    chunked = e.a_bytes >= (int64_t)ST_OOB || !desc_epi_reach_ok(d);
    return ST_OK;
}

// Larger than the 32-bit offsets reach (whole-batch PatchEmbed maps at B >= 4, ...): run the rows in chunks.  A chunk is a whole number of images (convs)
// and of aux0 mapping periods, so every operand just shifts its base.  piece(chunk descriptor) is called in row order; a non-zero return ends the walk.
template <class F>
static int for_each_row_chunk(const st_gemm_desc& d, F&& piece) {
    if ((d.batch > 1) || d.split_k > 1 || d.c_t || d.c_planes) return ST_EINVAL;
    const bool plain_mat = desc_is_plain_matrix(d);
    const f32_extent e = desc_f32_extent(d);
    const int64_t hw = e.hw, img_rows = e.img_rows, lim = (int64_t)1 << 31, ldmax = desc_epi_ldmax(d);
    const int64_t div = d.aux0_row_div > 1 ? d.aux0_row_div : 1, mod = d.aux0_row_mod > 0 ? d.aux0_row_mod : 1;
    int64_t a = hw, b = div * mod;                               // rows per indivisible unit: lcm(hw, aux0 period) via gcd
    while (b) { const int64_t t = a % b; a = b; b = t; }
    const int64_t unit = hw / a * (div * mod);
    const int64_t in_rows_per_unit = unit / hw * img_rows;
    int64_t per_out = (lim / 4 / ldmax - 256) / unit, per_in = ((int64_t)ST_OOB / 4 / d.ldx) / in_rows_per_unit;
    int64_t units = per_out < per_in ? per_out : per_in;
    // strictly inside both limits (check_f32's tests, on the chunk)
    while (units > 0 && (((units * in_rows_per_unit - 1) * d.ldx + d.Cin) * 4 >= (int64_t)ST_OOB || (units * unit + 256) * ldmax * 4 >= lim)) --units;
    if (units < 1 || d.M % unit || units * unit >= d.M) return ST_EINVAL;      // (a chunk must be a strict part)
    const int64_t total = d.M / unit, nchunks = (total + units - 1) / units;      // equal-sized chunks
    const int64_t chunk = (total + nchunks - 1) / nchunks * unit;
    for (int64_t m0 = 0; m0 < d.M; m0 += chunk) {
        st_gemm_desc c = d;
        c.M = (int32_t)((d.M - m0) < chunk ? (d.M - m0) : chunk);
        c.a = d.a + m0 / hw * img_rows * d.ldx;
        if (d.a2) c.a2 = d.a2 + m0 / hw * img_rows * d.ldx;
        c.c = d.c + m0 * d.ldc;
        if (d.c2) c.c2 = d.c2 + m0 * d.ldc2;
        if (d.aux1) c.aux1 = d.aux1 + m0 * d.ld_aux1;
        if (d.aux2) c.aux2 = d.aux2 + m0 * d.ld_aux2;
        if (d.aux0 && d.aux0_row_mod <= 0) c.aux0 = d.aux0 + m0 / div * d.ld_aux0;   // with a modulus the chunk starts a period
        if (plain_mat) { c.H = 1; c.W = c.M; c.Ho = 1; c.Wo = c.M; }
        const int rc = piece(c);
        if (rc) return rc;
    }
    return ST_OK;
}

// What a descriptor that passed check_f32 in one piece launches: kernel family, tile, split-K, persistent walk.  Every threshold is a measured choice
// (the comments say where); tests/test_gemm_plan_cpu.py pins both sides of each at the workload's shapes.
static int plan_f32(const st_gemm_desc& d, gemm_plan& p) {
    const f32_extent e = desc_f32_extent(d);
    p = gemm_plan{0, 0, 0, 0, false, false, (uint32_t)e.a_bytes, (uint32_t)e.w_bytes};
    auto chosen = [&p](int family, int tile, int split, int walk) { p.family = family; p.tile_cfg = tile; p.split = split; p.persistent = walk; return ST_OK; };
    const bool aligned = ((uintptr_t)d.a % 16 == 0) && ((uintptr_t)d.w % 16 == 0) && (d.ldx % 4 == 0) && (d.ldw % 4 == 0) && (d.Cin % 4 == 0) &&
                         (d.batch_stride_a % 4 == 0) && (d.batch_stride_w % 4 == 0);
    const int batch = d.batch > 0 ? d.batch : 1;
    if (d.M <= 8 && d.kh == 1 && d.kw == 1 && aligned && batch == 1 && d.epi == ST_EPI_STORE && !d.aux0 && d.H * d.W == d.M && !d.a2 && !d.c_t && !d.c_planes)
        return chosen(0, 0, 1, 0);
    if (d.N <= 4 && aligned && batch == 1 && d.epi != ST_EPI_ZR && d.M >= 1024 && d.tile_cfg == 0 && d.split_k <= 1 && !d.a2 && !d.c_t && !d.c_planes) {
        p.narrow3x3 = d.N <= 2 && d.Cin == 256 && d.kh == 3 && d.kw == 3 && d.sh == 1 && d.sw == 1 && d.ph == 1 && d.pw == 1 && d.dh <= 1 && d.dw <= 1 && d.Ho == d.H && d.Wo == d.W;
        return chosen(1, 0, 1, 0);
    }
    // row-streaming kernel (weights resident in LDS, A rows in registers): plain matrices with K = 64 / 128 and enough
    // 32-row blocks to give every wave of the chip at least one
    const bool map_ok = (d.aux0_row_div <= 1 && (d.aux0_row_mod <= 0 || d.aux0_row_mod % 32 == 0)) || (d.aux0_row_div == 8 && d.aux0_row_mod <= 0) || !d.aux0;
    const bool rs_ok = desc_is_plain_input(d) && aligned && batch == 1 && !d.a2 && !d.c_t && !d.c_planes && d.split_k <= 1 && (d.K == 64 || d.K == 128) &&
                       d.epi != ST_EPI_ZR && d.epi != ST_EPI_GRU && map_ok;
    // measured on MI355X, in the pipeline and stand-alone (tools/rowstream_bench.py): ahead of the LDS-DMA kernel for K = 64,
    // for M >= 262144 and for N >= 384; behind it by ~2 us per launch at M <= 65536, N = 128 (one block per wave: all
    // start-up); K = 256 (no room for the prefetch) was 10-30 % slower everywhere and is not instantiated
    const bool rs_want = d.tile_cfg == 20 || (d.tile_cfg == 0 && d.M >= 16384 && (d.K == 64 || d.M >= 262144 || (d.N >= 384 && d.M >= 32768)));
    if (d.a_ln && !(rs_ok && (d.tile_cfg == 0 || d.tile_cfg == 20))) return ST_EINVAL;
    if (rs_ok && (rs_want || d.a_ln)) {
        int cps, S;
        return rowstream_slices(d, d.K == 64 ? 2 : 4, cps, S) ? ST_EINVAL : chosen(4, 20, 1, 1);
    }
    if (d.tile_cfg >= 20) return ST_EINVAL;
    int cfg = d.tile_cfg;
    // the LDS-DMA pipelined kernel needs whole 32-channel K steps inside one tap
    const bool dma_ok = aligned && d.Cin % 32 == 0;
    if (cfg == 0) {
        // measured on MI355X (tools/tile_sweep.py, tools/dma_sweep.py): the 64x64 tile wins for every short-K /
        // mid-size shape of this path (more resident workgroups); 128-wide tiles stay selectable through tile_cfg.
        // K >= 128 (four K steps): the DMA ring already beats the register-staged kernel by 25-35 % per launch
        // (graph replay, tools/shortk_bench.py: 8192x256x160 14.4 -> 10.6 us, 8192x128x192 10.9 -> 7.6, 4096x128x128 7.8 -> 5.9)
        const bool dma = dma_ok && d.K >= 128;
        if (d.N <= 32) cfg = dma ? 14 : 4;
        else cfg = dma ? 13 : 3;
        // (64x128, tile_cfg 15, one workgroup per CU with two accumulator tiles per wave, stays selectable but is not chosen: round 4
        // measured it equal on the real z|r launches (67.0 / 65.3 vs 66.6 / 64.7 us, tools/tile15_bench.py, bit-identical) and 0.8 % slower
        // in the pipeline, 82.7 -> 82.0 pairs/s; it wins 2-5 % only on plain N = 256 long-K convs, which the path does not have)
    }
    if (!(cfg >= 1 && cfg <= 4) && !(cfg >= 12 && cfg <= 15)) return ST_EINVAL;
    if (cfg > 10 && !dma_ok) return ST_EINVAL;
    if ((d.a2 || d.c_t) && cfg <= 10) return ST_EINVAL;        // second A source / transposed copy: LDS-DMA kernels only
    // split-K: a launch that cannot fill the 256 CUs (M = 4096-pixel maps x 64..256 channels) is cut
    // along K into slabs reduced by a second tiny kernel (deterministic order; no atomics).
    const int bm = f32_bms[cfg > 10 ? cfg - 10 : cfg], bn = f32_bns[cfg > 10 ? cfg - 10 : cfg];
    const int ntm = (d.M + bm - 1) / bm, ntn = (d.N + bn - 1) / bn;
    const long tiles = (long)ntm * ntn * batch;
    int split = d.split_k;
    if (split == 0) {
        split = 1;
        if (batch == 1 && d.workspace && d.K >= 512 && !d.c_t) {
            if (cfg > 10) {
                // the pipelined kernel runs near its steady-state rate with ONE workgroup per CU, so it only needs
                // every CU covered; 257..511 tiles leave half the chip with twice the work of the other half
                if (tiles < 256) split = (int)((256 + tiles - 1) / tiles);
                else if (tiles < 512 && tiles % 256 && d.K >= 1024) split = 2;
            } else if (tiles < 256) {
                split = (int)((512 + tiles - 1) / tiles);
            }
            if (split > d.K / 256) split = d.K / 256;
            if (split > 16) split = 16;
            if (split < 1) split = 1;
            while (split > 1 && (int64_t)split * d.M * d.N > d.workspace_floats) --split;
        }
    }
    if (split > 1 && (batch != 1 || !d.workspace || (int64_t)split * d.M * d.N > d.workspace_floats)) return ST_EINVAL;
    p.vec = aligned;
    // persistent walk over M tiles (LDS-DMA kernels): plain matrices whose K is a whole number of ring turns and whose grid would
    // otherwise be many short workgroups (two resident per CU with this LDS footprint)
    const int slots = DMA_SLOTS / batch;
    const bool walk = cfg > 10 && desc_is_plain_matrix(d) && !d.a2 && split <= 1 && (d.K / 32) % DMA_STAGES == 0 && (long)ntm * ntn > slots && ntn <= slots && slots > 0;
    return chosen(cfg > 10 ? 3 : 2, cfg, split, walk);
}

static int launch_f32(st_gemm_desc d, const gemm_plan& p, hipStream_t s) {
    d.a_bytes = p.a_bytes; d.w_bytes = p.w_bytes;
    if (p.family == 4) return d.K == 64 ? launch_rowstream<2>(d, s) : launch_rowstream<4>(d, s);
    if (p.family <= 1) {
        if (p.family == 0) hipLaunchKernelGGL(skinny_gemm_kernel<8>, dim3((d.N * 64 + 255) / 256), dim3(256), 0, s, d);
        else if (p.narrow3x3) {
            const int waves = (d.M / (d.H * d.W)) * d.H * ((d.W + 7) / 8);
            hipLaunchKernelGGL(narrow_conv3x3_kernel<2>, dim3((waves + 3) / 4), dim3(256), 0, s, d);
        } else hipLaunchKernelGGL(narrow_conv_kernel<4>, dim3((d.M + 3) / 4), dim3(256), 0, s, d);
        ST_CHECK_LAUNCH();
        return ST_OK;
    }
    d.split_k = p.split;
    switch (p.tile_cfg) {
        case 12: return launch_dma<2, 2, 2, 1, 4>(d, p.persistent, s);
        // (a 3-deep ring -- 48 KB, three workgroups per CU -- is correct with this body (the K-block fold is independent of the ring depth) and
        // was measured: kernels of different pairs overlap better (3-in-flight / 1-in-flight 1.18 instead of 1.135) but a tile then has ONE K
        // step to land and every kernel slows down: 71.9 -> 67.9 pairs/s with one pair in flight, 81.6 -> 80.2 with three; a 5-deep ring
        // -- 80 KB, four tiles ahead -- for the convs and K >= 1024, round 4: 82.65 -> 81.5 / 72.5 -> 71.6: two workgroups no longer share a CU)
        case 13: return launch_dma<2, 2, 1, 1, 4>(d, p.persistent, s);
        case 15: return launch_dma<2, 2, 1, 2, 4>(d, p.persistent, s);      // 64x128: selectable only (see the tile choice in plan_f32)
        case 14: return launch_dma<4, 1, 1, 1, 4>(d, p.persistent, s);      // (80 KB of LDS; a 3-deep ring, 60 KB, measured neutral: PatchEmbed's 6x3 conv is not occupancy-bound)
        case 1: return launch_cfg<2, 2, 2, 2>(d, p.vec, s);
        case 2: return launch_cfg<2, 2, 2, 1>(d, p.vec, s);
        case 3: return launch_cfg<2, 2, 1, 1>(d, p.vec, s);
        case 4: return launch_cfg<4, 1, 1, 1>(d, p.vec, s);
        default: return ST_EINVAL;
    }
}

// check, chunk if needed, plan; `go(descriptor, plan)` is what happens to each planned piece (st_conv_gemm: launch it, st_gemm_plan: note the plan)
template <class Go>
static int dispatch_f32(const st_gemm_desc& d, Go& go) {
    bool chunked;
    if (check_f32(d, chunked)) return ST_EINVAL;
    if (chunked) return for_each_row_chunk(d, [&go](const st_gemm_desc& c) { return dispatch_f32(c, go); });
    gemm_plan p;
    return plan_f32(d, p) ? ST_EINVAL : go(d, p);
}

static int conv_gemm_launch(const st_gemm_desc* desc, void* stream) {
    if (desc->split3) return conv_gemm_split3_launch(desc, stream);
    auto go = [stream](const st_gemm_desc& d, const gemm_plan& p) { st_plan_set(p); return launch_f32(d, p, (hipStream_t)stream); };
    return dispatch_f32(*desc, go);
}

// An fp32 member of st_conv_gemm_pair (which = 0 / 1): one piece on the plain (non-persistent, unsplit) 64x64 LDS-DMA kernel.
static int plan_f32_pair_member(const st_gemm_desc& d, int which, gemm_plan& p) {
    if (!desc_common_check(d)) return ST_EINVAL;
    // both members share one grid of one tile shape: no batches, no split-K slabs, tile_cfg 13 only -- and nothing only another kernel carries
    if (d.split3 || d.c_t || d.a_ln || d.batch > 1 || d.split_k > 1 || (d.tile_cfg != 0 && d.tile_cfg != 13)) return ST_EINVAL;
    // the LDS-DMA kernel's preconditions, which plan_f32 answers by choosing another kernel: whole 32-channel K steps, a full ring, 16-byte rows
    if (d.K < 128 || d.Cin % 32 || ((uintptr_t)d.a & 15) || ((uintptr_t)d.w & 15) || (d.ldx & 3) || (d.ldw & 3)) return ST_EINVAL;
    const f32_extent e = desc_f32_extent(d);
    if (e.w_bytes >= (int64_t)ST_OOB || e.a_bytes >= (int64_t)ST_OOB || !desc_epi_reach_ok(d)) return ST_EINVAL;   // (no row chunking here)
    p = gemm_plan{3, 13, 1, 2 + which, false, false, (uint32_t)e.a_bytes, (uint32_t)e.w_bytes};
    return ST_OK;
}

extern "C" int st_conv_gemm_pair(const st_gemm_desc* desc0, const st_gemm_desc* desc1, void* stream) {
    if (!desc0 || !desc1) return ST_EINVAL;
    if (desc0->split3 || desc1->split3) return conv_gemm_split3_pair_launch(desc0, desc1, stream);
    gemm_plan p[2];
    if (plan_f32_pair_member(*desc0, 0, p[0]) || plan_f32_pair_member(*desc1, 1, p[1])) return ST_EINVAL;
    return launch_pair(conv_gemm_dma_pair_kernel<2, 2, 1, 1, 4>, 256, (size_t)4 * (64 + 64) * 32 * sizeof(float), desc0, desc1, p, stream);
}

// What st_conv_gemm(desc) -- or, with pair_with, st_conv_gemm_pair(desc, pair_with) -- would do, from the functions they run themselves: ST_EINVAL, or
// ST_OK and the four values st_gemm_last_plan reports after that call.  Launches nothing, follows no pointer, leaves the thread's last plan alone.
extern "C" int st_gemm_plan(const st_gemm_desc* desc, const st_gemm_desc* pair_with, int32_t* plan4) {
    if (!desc || !plan4) return ST_EINVAL;
    gemm_plan p[2];                                             // p[1]: the plan reported last
    auto go = [&p](const st_gemm_desc&, const gemm_plan& q) { p[1] = q; return ST_OK; };
    const int rc = !pair_with ? (desc->split3 ? conv_gemm_split3_plan(*desc, p[1]) : dispatch_f32(*desc, go))
                   : (desc->split3 || pair_with->split3) ? conv_gemm_split3_pair_plan(*desc, *pair_with, p)
                   : (plan_f32_pair_member(*desc, 0, p[0]) || plan_f32_pair_member(*pair_with, 1, p[1])) ? ST_EINVAL : ST_OK;
    if (rc) return rc;
    plan4[0] = p[1].family; plan4[1] = p[1].tile_cfg; plan4[2] = p[1].split; plan4[3] = p[1].persistent;
    return ST_OK;
}

// All-pairs correlation volume = batched A . B^T on the same MFMA core (K = C = 256 at 512^2).
extern "C" int st_corr_volume(const float* f1, const float* f2, float* vol, int32_t B, int32_t N1, int32_t N2,
                              int32_t C, void* stream) {
    if (!f1 || !f2 || !vol || B <= 0 || N1 <= 0 || N2 <= 0 || C <= 0) return ST_EINVAL;
    return Gemm(f1, C, f2, C, vol, N2, N1, N2, C).batched(B, (int64_t)N1 * C, (int64_t)N2 * C, (int64_t)N1 * N2).run(stream);
}

// 1 = one product with a transposed second store, 0 = two products.  The transposed store needs a shape of the LDS-DMA kernel
// (N % 4 == 0, C % 32 == 0, C >= 128, 16-byte aligned operands) AND a volume that the 32-bit buffer offsets reach in one piece:
// N * N * 4 < 2^31 for the transposed copy (desc_common_check rejects c_t otherwise) and (N + 256) * N * 4 < 2^31, f1 / f2 extents
// < 2^31 for the row-chunked path, which cannot carry c_t (N > ~23 000, i.e. flow grids beyond ~1 200 x 1 200 pixels / 8).
extern "C" int st_corr_volume_both_plan(int32_t B, int32_t N, int32_t C, int32_t aligned16) {
    if (B <= 0 || N <= 0 || C <= 0) return 0;
    if ((N & 3) || C % 32 || C < 128 || !aligned16) return 0;
    const int64_t lim = (int64_t)1 << 31;
    if ((int64_t)N * N * 4 >= lim || ((int64_t)N + 256) * N * 4 >= lim || ((int64_t)(N - 1) * C + C) * 4 >= (int64_t)ST_OOB) return 0;
    return 1;
}

extern "C" int st_corr_volume_both(const float* f1, const float* f2, float* vol12, float* vol21, int32_t B, int32_t N, int32_t C,
                                   void* stream) {
    if (!f1 || !f2 || !vol12 || !vol21 || B <= 0 || N <= 0 || C <= 0) return ST_EINVAL;
    if (!st_corr_volume_both_plan(B, N, C, (int32_t)((((uintptr_t)f1 | (uintptr_t)f2 | (uintptr_t)vol21) & 15) == 0))) {
        // not a shape of the LDS-DMA kernel's transposed store: two products
        const int rc = st_corr_volume(f1, f2, vol12, B, N, N, C, stream);
        return rc ? rc : st_corr_volume(f2, f1, vol21, B, N, N, C, stream);
    }
    return Gemm(f1, C, f2, C, vol12, N, N, N, C).transposed(vol21, N).batched(B, (int64_t)N * C, (int64_t)N * C, (int64_t)N * N).run(stream);
}

extern "C" int st_gemm_last_plan(int32_t* plan4) {
    if (!plan4) return ST_EINVAL;
    for (int i = 0; i < 4; ++i) plan4[i] = g_last_plan[i];
    return ST_OK;
}

// ABI self-check for bindings: size of st_gemm_desc as this library was compiled.
extern "C" int st_abi_gemm_desc_size(void) { return (int)sizeof(st_gemm_desc); }


// Optional profiling observer (bench.py's live roofline): called on the launching thread before (phase 0)
// and after (phase 1) the kernels of every st_conv_gemm are enqueued -- including the launches made by the
// operator-level entry points -- so the caller can record HIP events on `stream`.  NULL (default) = off.

extern "C" int st_set_gemm_observer(void* callback, void* user) {
    g_observer = (st_gemm_observer_fn)callback;
    g_observer_user = user;
    return ST_OK;
}

extern "C" int st_conv_gemm(const st_gemm_desc* desc, void* stream) {
    if (!desc) return ST_EINVAL;
    if (!st_observe(desc, stream, 0)) return conv_gemm_launch(desc, stream);
    const int rc = conv_gemm_launch(desc, stream);
    st_observe(desc, stream, 1);
    return rc;
}
