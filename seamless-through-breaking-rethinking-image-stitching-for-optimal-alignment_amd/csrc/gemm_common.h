// What the three translation units of the implicit-GEMM family share: gemm.hip (the fp32-MFMA kernels and their dispatcher),
// gemm_split3.hip (the exact-split bf16 kernels of gemm_split3.h) and gemm_rows.hip (the C = 128 row kernels, mlp_split3.h).
//   device side: the vector types, the raw-buffer / LDS-DMA loaders and the one epilogue every tiled kernel ends with;
//   host side:   the descriptor checks every path opens with, the launch plan, the plain-GEMM descriptor builder, the pair launcher, and declarations
//                of the few internals that cross the files (each defined once, in the file named beside it).
// Templates, __forceinline__ / inline functions, types and macros only -- no __global__ and no non-inline definition: the library is
// built without relocatable device code, every .hip is its own code object.  Macros of one family stay in that family's file.
#pragma once
#include "common.h"
#include <string.h>
#include <algorithm>
#include "../../include/stitch_gfx950.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Operand tiles are fetched with raw buffer loads: a lane whose tap / row / k is out of range gets an
// offset past the descriptor's num_records and the hardware returns zeros -- no branch and, crucially, no
// select on the loaded data (a select makes the compiler wait for the load right after issuing it, which
// serialises L2 latency with the MFMA block; measured: 3000 instead of ~1300 cycles per K step).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#define ST_OOB 0x80000000u

__device__ __forceinline__ float4 buf_load16(__amdgpu_buffer_rsrc_t rsrc, unsigned byte_off) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)byte_off, 0, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

// v = act(alpha*acc + bias[n] + aux0) followed by the combine mode; shared by the GEMM epilogue and
// the split-K reducer.
__device__ __forceinline__ float gemm_epilogue(const st_gemm_desc& d, int m, int n, float acc, float sc) {
    float v = fmaf(acc, d.alpha, d.bias ? d.bias[n] : 0.f);      // explicit fma everywhere: every kernel's epilogue rounds alike
    if (d.aux0) {
        int ar = m;
        if (d.aux0_row_div > 1) ar = m / d.aux0_row_div;
        if (d.aux0_row_mod > 0) ar = ar % d.aux0_row_mod;
        v += d.aux0[(size_t)ar * d.ld_aux0 + n];
    }
    v = st_act(v, d.act);
    switch (d.epi) {
        case ST_EPI_ADD: v += d.aux1[(size_t)m * d.ld_aux1 + n]; break;
        case ST_EPI_MUL: v *= d.aux1[(size_t)m * d.ld_aux1 + n]; break;
        case ST_EPI_GRU: {
            const float z = d.aux1[(size_t)m * d.ld_aux1 + n], h = d.aux2[(size_t)m * d.ld_aux2 + n];
            v = (1.0f - z) * h + z * v;
        } break;
        case ST_EPI_AXPY: v = fmaf(sc, v, d.aux1[(size_t)m * d.ld_aux1 + n]); break;
        default: break;
    }
    return v;
}

// st_gemm_desc.c_planes: element (m, col) of the plane-carrying output into the three blocked bf16 planes (scalar form: split-K reducer)
// (consecutive threads of the reducer own consecutive columns of a row -- N is even -- so lane ^ 1 holds the neighbouring column: dword stores)
__device__ __forceinline__ void gemm_store_planes(const st_gemm_desc& d, int m, int col, float v) {
    __bf16 h, mi, lo;
    st_split3(v, h, mi, lo);
    const unsigned ph = st_bf16_bits(h), pm = st_bf16_bits(mi), pl = st_bf16_bits(lo);
    const unsigned nh = (unsigned)__builtin_amdgcn_update_dpp(0, (int)ph, 0xB1, 0xF, 0xF, false);
    const unsigned nm = (unsigned)__builtin_amdgcn_update_dpp(0, (int)pm, 0xB1, 0xF, 0xF, false);
    const unsigned nl = (unsigned)__builtin_amdgcn_update_dpp(0, (int)pl, 0xB1, 0xF, 0xF, false);
    if (col & 1) return;
    const int cc = d.c_plane_col0 + col;
    unsigned* p = reinterpret_cast<unsigned*>(reinterpret_cast<__bf16*>(d.c_planes) + ((size_t)(cc >> 5) * d.c_plane_rows + d.c_plane_row0 + m) * 32 + (cc & 31));
    p[0] = ph | (nh << 16); p[d.c_plane_stride / 2] = pm | (nm << 16); p[d.c_plane_stride] = pl | (nl << 16);
}

// epilogue + store.  ST_EPI_ZR (fused GRU gates, gru.py:47-49): columns [0, N/2) are z -> C,
// columns [N/2, N) are r and leave as r*h -> c2 (aux1 = h).
__device__ __forceinline__ void gemm_store(const st_gemm_desc& d, float* __restrict__ C, int m, int n, float acc, float sc) {
    if (d.epi == ST_EPI_ZR) {
        const int half = d.N >> 1;
        float v = fmaf(acc, d.alpha, d.bias ? d.bias[n] : 0.f);
        if (d.aux0) v += d.aux0[(size_t)m * d.ld_aux0 + n];
        v = st_act(v, d.act);
        if (n < half) C[(size_t)m * d.ldc + n] = v;
        else {
            const float rh = v * d.aux1[(size_t)m * d.ld_aux1 + (n - half)];
            if (!d.c_no_f32) d.c2[(size_t)m * d.ldc2 + (n - half)] = rh;
            if (d.c_planes) gemm_store_planes(d, m, n - half, rh);
        }
        return;
    }
    const float o = gemm_epilogue(d, m, n, acc, sc);
    if (!d.c_no_f32) C[(size_t)m * d.ldc + n] = o;
    if (d.c_planes) gemm_store_planes(d, m, n, o);
}

// Epilogue shared by the fp32 and the split-bf16 kernels, in two halves so that the operand loads (bias, the
// pre-activation addend, residual / gate operands) can be issued BEFORE the K loop and land under its MFMAs:
// issued after it, they are two or three dependent L2 round trips that a short-K tile (K = 128: 64 MFMAs) cannot hide.
// acc[r] is C[row = (r&3) + 8*(r>>2) + 4*lh][col = li] of the 32x32 tile.
// Everything goes through raw buffer instructions: the per-lane offset (first row of the lane, its column) is
// computed once per 32x32 sub-tile, the 16 row steps are SGPR offsets, and the hardware range check (which
// includes the SGPR offset on gfx950 -- probed) drops rows >= M; absent operands get a zero-record descriptor, so the
// loads are unconditional, return 0 and touch no memory.  Result: no per-element address arithmetic or predication
// on the VALU, which v_mfma_f32_32x32x2_f32 shares its datapath with.
template <int TM, int TN>
struct EpiOperands {
    float sc;
    float bv[TN];
    float a0[TM][TN][16];      // aux0 (pre-activation addend)
    float x1[TM][TN][16];      // aux1
    float x2[TM][TN][16];      // aux2 (GRU state)
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t epi_rsrc(const float* p, long long bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, p ? (int)bytes : 0, 0x00020000);
}
__device__ __forceinline__ float buf_ld(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0));
}
__device__ __forceinline__ void buf_st(float v, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, (int)voff, (int)soff, 0);
}
// st_gemm_desc.c_planes: the lane's value of accumulator row r into the three blocked bf16 planes.  Lanes li = 0..31 of a sub-tile are the 32
// channels of one chunk row; neighbouring lanes exchange their halves (one DPP move per plane) and the EVEN lane stores the pair as a dword
// (vp of the odd lanes is the out-of-range sentinel): 16 dword lanes = one 64-byte chunk row per wave half, no sub-dword store anywhere.
__device__ __forceinline__ void buf_st_planes(float v, __amdgpu_buffer_rsrc_t r, unsigned vp_even, unsigned soff, unsigned plane_b) {
    __bf16 h, mi, lo;
    st_split3(v, h, mi, lo);
    const unsigned ph = st_bf16_bits(h), pm = st_bf16_bits(mi), pl = st_bf16_bits(lo);
    const unsigned nh = (unsigned)__builtin_amdgcn_update_dpp(0, (int)ph, 0xB1, 0xF, 0xF, false);     // quad_perm [1, 0, 3, 2]: lane ^ 1
    const unsigned nm = (unsigned)__builtin_amdgcn_update_dpp(0, (int)pm, 0xB1, 0xF, 0xF, false);
    const unsigned nl = (unsigned)__builtin_amdgcn_update_dpp(0, (int)pl, 0xB1, 0xF, 0xF, false);
    __builtin_amdgcn_raw_buffer_store_b32(ph | (nh << 16), r, (int)vp_even, (int)soff, 0);
    __builtin_amdgcn_raw_buffer_store_b32(pm | (nm << 16), r, (int)vp_even, (int)(soff + plane_b), 0);
    __builtin_amdgcn_raw_buffer_store_b32(pl | (nl << 16), r, (int)vp_even, (int)(soff + 2u * plane_b), 0);
}
// row r of a lane's 16 accumulator registers, relative to the lane's first row
#define ST_EPI_ROW(r) (((r) & 3) + 8 * ((r) >> 2))

// per-workgroup constants of the epilogue: bias of the lane's columns, the device scalar of ST_EPI_AXPY
template <int TM, int TN>
__device__ __forceinline__ void gemm_epilogue_consts(const st_gemm_desc& d, EpiOperands<TM, TN>& e, int n0, int wn, int li, int split) {
    const bool raw = split > 1;
    e.sc = (d.scale_ptr && !raw) ? *d.scale_ptr : 1.0f;
    const __amdgpu_buffer_rsrc_t rb = epi_rsrc(raw ? nullptr : d.bias, (long long)d.N * 4);
#pragma unroll
    for (int jn = 0; jn < TN; ++jn) {
        const int n = n0 + wn * TN * 32 + jn * 32 + li;
        e.bv[jn] = buf_ld(rb, (unsigned)(n < d.N ? n : d.N - 1) * 4u, 0);
    }
}

// LITE (row-streaming kernel; the host checks the descriptor): no per-element row mapping, no GRU / z|r modes -- their
// operand registers and code are not instantiated.
template <int TM, int TN, bool LITE = false>
__device__ __forceinline__ void gemm_epilogue_load(const st_gemm_desc& d, EpiOperands<TM, TN>& e, int m0, int n0, int wm, int wn,
                                                   int li, int lh, int split) {
    const bool raw = split > 1;                                // raw partial sums: nothing to fetch
    const int half = d.N >> 1;
    const bool zr = !LITE && d.epi == ST_EPI_ZR;
    const long long M = d.M;
    // aux0 row = (m / div) % mod.  div == 8 without mod (one table row per pixel, 8 latent rows each -- the vertical
    // layers' q / k tables) keeps the SGPR-step form: a lane's rows m0' + (r&3) + 8*(r>>2), m0' % 4 == 0, map to
    // table rows m0'/8 + (r>>2), i.e. four loads.  Other mappings are computed per element (small GEMMs only).
    // mod % 32 == 0 without div (a table of `mod` rows repeated down the matrix -- PatchEmbed's per-patch position table):
    // a 32-row sub-tile never wraps, so it is the identity form started at row (sub-tile start) % mod.
    const bool div8 = d.aux0_row_div == 8 && d.aux0_row_mod <= 0;
    const bool mod32 = d.aux0_row_div <= 1 && d.aux0_row_mod > 0 && (d.aux0_row_mod & 31) == 0;
    const bool mapped = !LITE && !div8 && !mod32 && (d.aux0_row_div > 1 || d.aux0_row_mod > 0);
    const __amdgpu_buffer_rsrc_t r0 = epi_rsrc(raw ? nullptr : d.aux0, mapped ? 0x7fffffffLL
                                               : div8 ? (((M + 7) / 8 - 1) * d.ld_aux0 + d.N) * 4
                                               : mod32 ? ((long long)(d.aux0_row_mod - 1) * d.ld_aux0 + d.N) * 4 : ((M - 1) * d.ld_aux0 + d.N) * 4);
    const float* aux1 = d.aux1 ? d.aux1 + (size_t)(d.batch > 1 ? blockIdx.z : 0) * d.batch_stride_aux1 : nullptr;
    const __amdgpu_buffer_rsrc_t r1 = epi_rsrc((raw || d.epi == ST_EPI_STORE) ? nullptr : aux1, ((M - 1) * d.ld_aux1 + (zr ? half : d.N)) * 4);
    const __amdgpu_buffer_rsrc_t r2 = epi_rsrc((raw || d.epi != ST_EPI_GRU) ? nullptr : d.aux2, ((M - 1) * d.ld_aux2 + d.N) * 4);
#pragma unroll
    for (int jn = 0; jn < TN; ++jn) {
        const int n = n0 + wn * TN * 32 + jn * 32 + li;
        const int nc = n < d.N ? n : d.N - 1;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int row0 = m0 + wm * TM * 32 + i * 32 + 4 * lh;              // this lane's first row
            // aux0: identity rows, or the (row / div) % mod table mapping (per element; small tables).  Operands the
            // mode does not use are not fetched (wave-uniform branches; their registers stay undefined and unread).
            if (!raw && d.aux0) {
                if (mapped) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        int ar = min(row0 + ST_EPI_ROW(r), d.M - 1);
                        if (d.aux0_row_div > 1) ar = ar / d.aux0_row_div;
                        if (d.aux0_row_mod > 0) ar = ar % d.aux0_row_mod;
                        e.a0[i][jn][r] = buf_ld(r0, (unsigned)(ar * d.ld_aux0 + nc) * 4u, 0);
                    }
                } else if (div8) {
                    const unsigned v0 = (unsigned)((row0 >> 3) * d.ld_aux0 + nc) * 4u;
                    float t4[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) t4[q] = buf_ld(r0, v0, (unsigned)(q * d.ld_aux0) * 4u);
#pragma unroll
                    for (int r = 0; r < 16; ++r) e.a0[i][jn][r] = t4[r >> 2];
                } else {
                    const unsigned v0 = (unsigned)((mod32 ? row0 % d.aux0_row_mod : row0) * d.ld_aux0 + nc) * 4u;
#pragma unroll
                    for (int r = 0; r < 16; ++r) e.a0[i][jn][r] = buf_ld(r0, v0, (unsigned)(ST_EPI_ROW(r) * d.ld_aux0) * 4u);
                }
            }
            if (!raw && d.epi != ST_EPI_STORE) {
                const int c1 = zr ? (nc >= half ? nc - half : 0) : nc;
                const unsigned v1 = (unsigned)(row0 * d.ld_aux1 + c1) * 4u;
#pragma unroll
                for (int r = 0; r < 16; ++r) e.x1[i][jn][r] = buf_ld(r1, v1, (unsigned)(ST_EPI_ROW(r) * d.ld_aux1) * 4u);
                if (!LITE && d.epi == ST_EPI_GRU) {
                    const unsigned v2 = (unsigned)(row0 * d.ld_aux2 + nc) * 4u;
#pragma unroll
                    for (int r = 0; r < 16; ++r) e.x2[i][jn][r] = buf_ld(r2, v2, (unsigned)(ST_EPI_ROW(r) * d.ld_aux2) * 4u);
                }
            }
        }
    }
}

template <int TM, int TN, bool LITE = false, bool CT = false>
__device__ __forceinline__ void gemm_epilogue_store(const st_gemm_desc& d, float* __restrict__ C, f32x16 (&acc)[TM][TN],
                                                    const EpiOperands<TM, TN>& e, int m0, int n0, int wm, int wn, int li, int lh,
                                                    int split, int kz) {
    const int half = d.N >> 1;
    const long long M = d.M;
    if (split > 1) {                                           // raw partial sums -> slab kz of the workspace
        const __amdgpu_buffer_rsrc_t rw = epi_rsrc(d.workspace + (size_t)kz * d.M * d.N, M * d.N * 4);
#pragma unroll
        for (int jn = 0; jn < TN; ++jn) {
            const int n = n0 + wn * TN * 32 + jn * 32 + li;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row0 = m0 + wm * TM * 32 + i * 32 + 4 * lh;
                const unsigned vo = n < d.N ? (unsigned)(row0 * d.N + n) * 4u : ST_OOB;
#pragma unroll
                for (int r = 0; r < 16; ++r) buf_st(acc[i][jn][r], rw, vo, (unsigned)(ST_EPI_ROW(r) * d.N) * 4u);
            }
        }
        return;
    }
    const bool zr = !LITE && d.epi == ST_EPI_ZR;
    // c_no_f32: the plane-carrying output (c, or c2 in z|r mode) is not stored as fp32 (zero-record descriptor: the stores are dropped)
    const __amdgpu_buffer_rsrc_t rc = epi_rsrc((d.c_no_f32 && !zr) ? nullptr : C, ((M - 1) * d.ldc + (zr ? half : d.N)) * 4);
    const __amdgpu_buffer_rsrc_t rc2 = epi_rsrc((zr && !d.c_no_f32) ? d.c2 : nullptr, ((M - 1) * d.ldc2 + half) * 4);
    // optional plane copy of the result (st_gemm_desc.c_planes): host-checked M % 32 == 0, c_plane_col0 % 32 == 0, extents < 2 GiB
    const bool planes = !LITE && d.c_planes != nullptr;
    const unsigned plane_b = (unsigned)(d.c_plane_stride * 2);
    const __amdgpu_buffer_rsrc_t rp = epi_rsrc(planes ? reinterpret_cast<const float*>(d.c_planes) : nullptr, 0x7fffffffLL);
    const long long prow0 = d.c_plane_row0 + (long long)(d.batch > 1 ? blockIdx.z : 0) * d.c_plane_batch_rows;
#pragma unroll
    for (int jn = 0; jn < TN; ++jn) {
        const int n = n0 + wn * TN * 32 + jn * 32 + li;
        const bool ncol = n < d.N;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int row0 = m0 + wm * TM * 32 + i * 32 + 4 * lh;
            float v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = fmaf(acc[i][jn][r], d.alpha, e.bv[jn]);
            if (d.aux0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] += e.a0[i][jn][r];
            }
            switch (d.act) {                                   // wave-uniform, outside the register loop
                case ST_ACT_RELU:
#pragma unroll
                    for (int r = 0; r < 16; ++r) v[r] = fmaxf(v[r], 0.f);
                    break;
                case ST_ACT_GELU:
#pragma unroll
                    for (int r = 0; r < 16; ++r) v[r] = st_act(v[r], ST_ACT_GELU);
                    break;
                case ST_ACT_SIGMOID:
#pragma unroll
                    for (int r = 0; r < 16; ++r) v[r] = st_act(v[r], ST_ACT_SIGMOID);
                    break;
                case ST_ACT_TANH:
#pragma unroll
                    for (int r = 0; r < 16; ++r) v[r] = st_act(v[r], ST_ACT_TANH);
                    break;
                case ST_ACT_LRELU:
#pragma unroll
                    for (int r = 0; r < 16; ++r) v[r] = st_act(v[r], ST_ACT_LRELU);
                    break;
                default: break;
            }
            // plane copy: byte offset of (this lane's first row, its channel) inside plane 0; a 32-row sub-tile is wholly inside M
            unsigned vp = ST_OOB;
            if (planes) {
                const int pcol = d.c_plane_col0 + (zr ? n - half : n);
                // (even lane: its column and the next are both inside -- the plane-carrying output has an even number of columns, host-checked)
                if (!(li & 1) && ncol && (!zr || n >= half) && row0 < d.M)
                    vp = (unsigned)((((long long)(pcol >> 5) * d.c_plane_rows + prow0 + row0) * 32 + (pcol & 31)) * 2);
            }
            if (zr) {
                const unsigned vc = (ncol && n < half) ? (unsigned)(row0 * d.ldc + n) * 4u : ST_OOB;
                const unsigned vc2 = (ncol && n >= half) ? (unsigned)(row0 * d.ldc2 + n - half) * 4u : ST_OOB;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    buf_st(v[r], rc, vc, (unsigned)(ST_EPI_ROW(r) * d.ldc) * 4u);
                    const float rh = v[r] * e.x1[i][jn][r];
                    buf_st(rh, rc2, vc2, (unsigned)(ST_EPI_ROW(r) * d.ldc2) * 4u);
                    if (planes) buf_st_planes(rh, rp, vp, (unsigned)(ST_EPI_ROW(r) * 64), plane_b);
                }
            } else {
                const unsigned vc = ncol ? (unsigned)(row0 * d.ldc + n) * 4u : ST_OOB;
                if (d.epi == ST_EPI_STORE) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) buf_st(v[r], rc, vc, (unsigned)(ST_EPI_ROW(r) * d.ldc) * 4u);
                    if (planes) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) buf_st_planes(v[r], rp, vp, (unsigned)(ST_EPI_ROW(r) * 64), plane_b);
                    }
                    if (CT && d.c_t) {                           // (only the CT instantiations carry this code)
                        // transposed copy: the lane's 16 values are 4 runs of 4 consecutive rows of column n -> 4 x 16-byte stores
                        // into row n of c_t (M % 4 == 0: a run is inside the matrix or wholly outside)
                        float* ctb = d.c_t + (size_t)(d.batch > 1 ? blockIdx.z : 0) * d.batch_stride_c;
                        const __amdgpu_buffer_rsrc_t rt = epi_rsrc(ctb, ((long long)(d.N - 1) * d.ld_ct + M) * 4);
#pragma unroll
                        for (int q4 = 0; q4 < 4; ++q4) {
                            const unsigned vt = (ncol && row0 + 8 * q4 < d.M) ? (unsigned)(n * d.ld_ct + row0 + 8 * q4) * 4u : ST_OOB;
                            const u32x4 pk = {__float_as_uint(v[4 * q4]), __float_as_uint(v[4 * q4 + 1]), __float_as_uint(v[4 * q4 + 2]),
                                              __float_as_uint(v[4 * q4 + 3])};
                            __builtin_amdgcn_raw_buffer_store_b128(pk, rt, (int)vt, 0, 0);
                        }
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float x1 = e.x1[i][jn][r];
                        float o = v[r] + x1;                                   // ST_EPI_ADD
                        if (d.epi == ST_EPI_MUL) o = v[r] * x1;
                        else if (!LITE && d.epi == ST_EPI_GRU) o = (1.0f - x1) * e.x2[i][jn][r] + x1 * v[r];
                        else if (d.epi == ST_EPI_AXPY) o = fmaf(e.sc, v[r], x1);
                        buf_st(o, rc, vc, (unsigned)(ST_EPI_ROW(r) * d.ldc) * 4u);
                        if (planes) buf_st_planes(o, rp, vp, (unsigned)(ST_EPI_ROW(r) * 64), plane_b);
                    }
                }
            }
        }
    }
}

template <int TM, int TN>
__device__ __forceinline__ void gemm_tile_epilogue(const st_gemm_desc& d, float* __restrict__ C, f32x16 (&acc)[TM][TN], int m0, int n0,
                                                   int wm, int wn, int li, int lh, int split, int kz) {
    EpiOperands<TM, TN> e;
    gemm_epilogue_consts<TM, TN>(d, e, n0, wn, li, split);
    gemm_epilogue_load<TM, TN>(d, e, m0, n0, wm, wn, li, lh, split);
    gemm_epilogue_store<TM, TN>(d, C, acc, e, m0, n0, wm, wn, li, lh, split, kz);
}

typedef int i32x4 __attribute__((ext_vector_type(4)));
struct st_true { static constexpr bool value = true; };
struct st_false { static constexpr bool value = false; };

// M0 is not used by anything else in these kernels (gfx9 DS ops do not need it), so it is simply overwritten.
__device__ __forceinline__ void lds_dma16(i32x4 rsrc, unsigned lds_byte_addr, unsigned voff, unsigned soff) {
    asm volatile(
        "s_mov_b32 m0, %0\n\t"
        "s_nop 0\n\t"
        "buffer_load_dwordx4 %1, %2, %3 offen lds"
        :
        : "s"(lds_byte_addr), "v"(voff), "s"(rsrc), "s"(soff)
        : "memory");
}

__device__ __forceinline__ i32x4 make_rsrc(const void* base, unsigned bytes) {
    const unsigned long long a = (unsigned long long)base;
    i32x4 r;
    r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
    r.y = __builtin_amdgcn_readfirstlane((int)(unsigned)((a >> 32) & 0xffffu));   // stride 0, no swizzle
    r.z = __builtin_amdgcn_readfirstlane((int)bytes);
    r.w = 0x00020000;
    return r;
}

// Two independent contractions in ONE launch (st_conv_gemm_pair): workgroups [0, tiles0) run d[0], the rest d[1].  For pairs of
// mid-size convs that are ready at the same time and each fill only part of the chip (BasicMotionEncoder's convc2: 384 tiles, and
// convf2: 128 tiles, gru.py:252-253): together they give every CU two workgroups without split-K slabs or a second launch.
struct st_gemm_pair_args {
    st_gemm_desc d[2];
    int32_t tiles0;
};

// st_gemm_desc.c_planes: what every kernel that can emit planes needs checked
inline bool c_planes_ok(const st_gemm_desc& d) {
    if (d.reserved4 != 0) return false;
    if (!d.c_planes) return d.c_no_f32 == 0;
    const int batch = d.batch > 0 ? d.batch : 1;
    const int ncols = d.epi == ST_EPI_ZR ? d.N / 2 : d.N;
    if ((d.M & 31) || (ncols & 1) || (d.c_plane_col0 & 31) || d.c_plane_col0 < 0 || d.c_plane_row0 < 0 || d.c_plane_stride <= 0 || (d.c_plane_stride & 7) || d.c_plane_rows <= 0 ||
        ((uintptr_t)d.c_planes & 15) || d.c_t)
        return false;
    const int64_t last_row = d.c_plane_row0 + (int64_t)(batch - 1) * d.c_plane_batch_rows + d.M;
    if (last_row > d.c_plane_rows) return false;
    const int64_t chunks = (d.c_plane_col0 + ncols + 31) / 32;
    return 2 * (2 * d.c_plane_stride + chunks * d.c_plane_rows * 32) < ((int64_t)1 << 31);
}

// ---- descriptor checks, written once: the fp32 path, the fp32 pair members (gemm.hip) and the split3 path (gemm_split3.hip) each add their own rules ----
// a 1x1 window, unit stride, no padding over an input of exactly M pixels: A is read as M rows.  (Says nothing about Ho / Wo: the row-streaming
// kernel's test, which never looks at them -- a descriptor with Ho * Wo a proper divisor of M passes the common checks and takes that kernel.)
inline bool desc_is_plain_input(const st_gemm_desc& d) { return d.kh == 1 && d.kw == 1 && d.sh == 1 && d.sw == 1 && d.ph == 0 && d.pw == 0 && (int64_t)d.H * d.W == d.M; }
// a matrix: every row is its own "image".  (Products in 64 bits at every site; the LDS-DMA walk's copy took them in 32, which differs only where H * W
// overflows int32 -- undefined there, and with ldx >= 1 such an input has already failed the 2 GiB test of its A extent.)
inline bool desc_is_plain_matrix(const st_gemm_desc& d) { return desc_is_plain_input(d) && (int64_t)d.Ho * d.Wo == d.M; }

// the epilogue addresses C / aux operands with 32-bit buffer offsets (first row of a lane + SGPR row step): the largest leading dimension it uses ...
inline int64_t desc_epi_ldmax(const st_gemm_desc& d) {
    const int64_t ld[6] = {d.ldc, d.N, d.aux0 ? d.ld_aux0 : 0, d.aux1 ? d.ld_aux1 : 0, d.aux2 ? d.ld_aux2 : 0, d.c2 ? d.ldc2 : 0};
    return *std::max_element(ld, ld + 6);
}
inline bool desc_epi_reach_ok(const st_gemm_desc& d) { return ((int64_t)d.M + 256) * desc_epi_ldmax(d) * 4 < ((int64_t)1 << 31); }     // ... and whether it reaches every row
inline bool desc_common_check(const st_gemm_desc& d) {           // what every path checks
    if (!d.a || !d.w || !d.c || d.M <= 0 || d.N <= 0 || d.K <= 0) return false;
    if (d.kh <= 0 || d.kw <= 0 || d.K != d.kh * d.kw * d.Cin) return false;
    if (d.Ho <= 0 || d.Wo <= 0 || d.M % (d.Ho * d.Wo)) return false;
    if (d.epi != ST_EPI_STORE && !d.aux1) return false;
    if (d.epi == ST_EPI_GRU && !d.aux2) return false;
    if (d.epi == ST_EPI_ZR && (!d.c2 || (d.N & 1))) return false;
    if (d.reserved0 != 0 || d.reserved1 != 0 || d.reserved2 != 0 || d.reserved3 != 0) return false;
    // transposed second store: 16-byte runs of four rows, inside the 32-bit offsets, never from split-K slabs
    if (d.c_t && (d.epi != ST_EPI_STORE || (d.M & 3) || (d.ld_ct & 3) || d.ld_ct < d.M || ((uintptr_t)d.c_t & 15) || d.split_k > 1 ||
                  (int64_t)d.N * d.ld_ct * 4 >= ((int64_t)1 << 31)))
        return false;
    // second A source: whole 32-channel K steps, one batch (the pair members reject batch > 1 outright, so the batch half is moot there)
    if (d.a2 && (d.a2_channels <= 0 || d.a2_channels % 32 || d.a2_channels > d.Cin || d.batch > 1 || ((uintptr_t)d.a2 & 15))) return false;
    return c_planes_ok(d);
}

// byte extents of one batch slice of the fp32 operands A and W for the buffer descriptors (both must stay below 2 GiB so that the out-of-range
// sentinel offset is always past num_records); hw / img_rows = output / input rows per image (1 / 1 for a matrix)
struct f32_extent { int64_t hw, img_rows, a_bytes, w_bytes; };
inline f32_extent desc_f32_extent(const st_gemm_desc& d) {
    const bool plain_mat = desc_is_plain_matrix(d);
    const int64_t hw = plain_mat ? 1 : (int64_t)d.Ho * d.Wo, img_rows = plain_mat ? 1 : (int64_t)d.H * d.W;
    return {hw, img_rows, ((d.M / hw * img_rows - 1) * d.ldx + d.Cin) * 4, ((int64_t)(d.N - 1) * d.ldw + d.K) * 4};
}

// What a checked descriptor launches.  The first four are st_gemm_last_plan's values, in its order; plan_f32 (gemm.hip) and plan_split3
// (gemm_split3.hip) fill one without a HIP call or a global, the launchers switch on it.
struct gemm_plan {
    int32_t family, tile_cfg, split, persistent;
    bool vec, narrow3x3;        // family 2: the register-staged kernel's 16-byte loads (VEC), not its scalar gather; family 1: narrow_conv3x3_kernel, not narrow_conv_kernel
    uint32_t a_bytes, w_bytes;  // st_gemm_desc.a_bytes / w_bytes of the launch
};

// The plain A . B^T descriptor and what the callers put on top of it (the operator entry points, st_corr_volume*, the row launchers' observer image)
struct Gemm {
    st_gemm_desc d;
    Gemm(const float* a, int32_t lda, const float* w, int32_t ldw, float* c, int32_t ldc, int32_t M, int32_t N, int32_t Cin) {
        memset(&d, 0, sizeof(d));
        d.a = a; d.w = w; d.c = c; d.M = M; d.N = N; d.K = Cin; d.ldx = lda; d.ldw = ldw; d.ldc = ldc;
        d.H = 1; d.W = M; d.Cin = Cin; d.kh = d.kw = d.sh = d.sw = 1; d.Ho = 1; d.Wo = M;
        d.alpha = 1.f; d.batch = 1;
    }
    Gemm& conv(int32_t B, int32_t H, int32_t W, int32_t kh, int32_t kw, int32_t sh, int32_t sw, int32_t ph, int32_t pw, int32_t Ho = -1, int32_t Wo = -1) {
        d.H = H; d.W = W; d.kh = kh; d.kw = kw; d.sh = sh; d.sw = sw; d.ph = ph; d.pw = pw;
        d.Ho = Ho >= 0 ? Ho : (H + 2 * ph - kh) / sh + 1; d.Wo = Wo >= 0 ? Wo : (W + 2 * pw - kw) / sw + 1;
        d.M = B * d.Ho * d.Wo; d.K = kh * kw * d.Cin;
        return *this;
    }
    Gemm& bias(const float* b) { d.bias = b; return *this; }
    Gemm& act(int a) { d.act = a; return *this; }
    Gemm& alpha(float a) { d.alpha = a; return *this; }
    Gemm& aux0(const float* p, int32_t ld, int32_t row_div = 0, int32_t row_mod = 0) { d.aux0 = p; d.ld_aux0 = ld; d.aux0_row_div = row_div; d.aux0_row_mod = row_mod; return *this; }
    Gemm& epi(int e, const float* a1, int32_t ld1, const float* a2 = nullptr, int32_t ld2 = 0) { d.epi = e; d.aux1 = a1; d.ld_aux1 = ld1; d.aux2 = a2; d.ld_aux2 = ld2; return *this; }
    Gemm& scale(const float* s) { d.scale_ptr = s; return *this; }
    Gemm& out2(float* c2, int32_t ld) { d.c2 = c2; d.ldc2 = ld; return *this; }
    Gemm& a2(const float* p, int32_t channels) { d.a2 = p; d.a2_channels = channels; return *this; }
    Gemm& batched(int32_t n, int64_t sa, int64_t sw, int64_t sc) { d.batch = n; d.batch_stride_a = sa; d.batch_stride_w = sw; d.batch_stride_c = sc; return *this; }
    Gemm& transposed(float* c_t, int32_t ld) { d.c_t = c_t; d.ld_ct = ld; return *this; }
    Gemm& work(void* ws, int64_t floats) { d.workspace = (float*)ws; d.workspace_floats = floats; return *this; }
    int run(void* stream) { return st_conv_gemm(&d, stream); }
};

// ---- host-side internals that cross the translation units (not part of the C ABI) ---------------------------------------------------
// The profiling observer (st_set_gemm_observer) and the calling thread's last launch plan (st_gemm_last_plan).  The state is private to
// gemm.hip; every launcher of the family, in whichever file, reports through these.
void st_plan_set(int kernel, int tile, int split_k, int persistent);      // the calling thread's last plan (st_gemm_last_plan's four values)
inline void st_plan_set(const gemm_plan& p) { st_plan_set(p.family, p.tile_cfg, p.split, p.persistent); }
bool st_observer_installed(void);                                          // lets a launcher build a descriptor for the observer only when one listens
bool st_observe(const st_gemm_desc* od, void* stream, int phase);         // phase 0 before a launch, 1 after it; false when no observer is installed
void splitk_reduce_launch(const st_gemm_desc& d, hipStream_t s);          // gemm.hip: the split-K tail (splitk_reduce_kernel) behind a launch with d.split_k > 1
// gemm_split3.hip: st_conv_gemm / st_conv_gemm_pair with split3 set, and what each would launch (checks + plan_split3, no HIP call: st_gemm_plan)
int conv_gemm_split3_launch(const st_gemm_desc* desc, void* stream);
int conv_gemm_split3_pair_launch(const st_gemm_desc* desc0, const st_gemm_desc* desc1, void* stream);
int conv_gemm_split3_plan(const st_gemm_desc& desc, gemm_plan& p);
int conv_gemm_split3_pair_plan(const st_gemm_desc& desc0, const st_gemm_desc& desc1, gemm_plan (&p)[2]);

// One launch for both members of a pair (fp32: conv_gemm_dma_pair_kernel, split3: conv_gemm_split3_pair_kernel): workgroups [0, tiles0) of 64x64 tiles
// run desc0, the rest desc1.  p: the members' plans; plan[3] = 2 for the first member (no dispatch of its own: the observer sees an empty bracket),
// 3 for the second (the pair's single dispatch and all of its time).
template <class K>
inline int launch_pair(K k, int block, size_t lds, const st_gemm_desc* desc0, const st_gemm_desc* desc1, const gemm_plan (&p)[2], void* stream) {
    st_gemm_pair_args g;
    for (int i = 0; i < 2; ++i) {
        g.d[i] = i ? *desc1 : *desc0;
        g.d[i].a_bytes = p[i].a_bytes; g.d[i].w_bytes = p[i].w_bytes; g.d[i].split_k = 1; g.d[i].batch = 1;
    }
    auto tiles = [](const st_gemm_desc& d) { return ((d.M + 63) / 64) * ((d.N + 63) / 64); };
    g.tiles0 = tiles(g.d[0]);
    const int total = g.tiles0 + tiles(g.d[1]);
    st_plan_set(p[0]);
    const bool obs = st_observe(desc0, stream, 0);
    if (obs) { st_observe(desc0, stream, 1); st_observe(desc1, stream, 0); }
    st_plan_set(p[1]);
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, dim3(total), dim3(block), lds, (hipStream_t)stream, g);
    if (obs) st_observe(desc1, stream, 1);                      // (the pair's time is attributed to its second member)
    ST_CHECK_LAUNCH();
    return ST_OK;
}
