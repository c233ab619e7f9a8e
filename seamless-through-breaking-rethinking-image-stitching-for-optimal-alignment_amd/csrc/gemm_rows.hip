// The C = 128 row kernels of the implicit-GEMM family and their entry points: a wave owns 32-row blocks that stay in registers in the MFMA
// operand layout while several layers are applied, so the intermediate activations never leave the CU.
//   rowchain128_kernel   st_linear_chain128: up to three Linear(128 -> 128) layers (fp32 MFMA)
//   rowmlp128_kernel     st_mlp128: [projection + residual ->] LayerNorm -> fc1 + GELU -> fc2 + residual(s) (fp32 MFMA)
//   mlp_split3.h         the same block tail, LayerNorm -> Linear(128 -> N), the latent self-attention (LayerNorm -> q | k | v -> 8 x 8 attention) and
//                        PatchEmbed's tail on the exact-split bf16 contraction (rowmlp128_split3_kernel, rowlin128_split3_kernel,
//                        latent_self_attn_split3_kernel, pe_tail_split3_kernel and their weight-image pack kernels)
// The loaders and vector types they share with the tiled kernels of gemm.hip / gemm_split3.hip are in gemm_common.h.
#include "gemm_common.h"

// One launch of this file as the rest of the family sees it.  The calling thread's plan (st_gemm_last_plan) becomes (kernel, tile, 1, 1); an installed
// profiling observer gets the launch as ONE GEMM of the family, M x N x 128 (N chosen by the caller so that 2 M N 128 is the launch's FLOPs; the
// A + W + C byte formula of the tools then counts the intermediate activations that these kernels do NOT move).  The descriptor is only built when
// an observer is installed; returns whether phase 0 was reported, i.e. whether the caller owes st_observe(&od, stream, 1) behind its launch.
static bool row_launch_begin(st_gemm_desc& od, int kernel, int tile, void* stream, const float* a, int lda, float* c, int ldc, const void* w, int M, int N,
                             int split3) {
    bool obs = st_observer_installed();
    if (obs) {
        od = Gemm(a, lda, (const float*)w, 128, c, ldc, M, N, 128).d;
        od.split3 = split3;
        obs = st_observe(&od, stream, 0);
    }
    st_plan_set(kernel, tile, 1, 1);
    return obs;
}

// ---------------------------------------------------------------------------------------------
// Row chain: up to three Linear(128 -> 128) layers applied to 32-row blocks that never leave the CU (st_linear_chain128).
// Built on the row-streaming kernel: a wave keeps its block in registers in the A-operand layout (lane (li, lh) holds
// k = 8j + 4lh + t of row li); a layer is four 32-column chunks of 64 MFMAs computed as the TRANSPOSED product (weights first
// operand, activations second): a chunk's accumulators are then row li's output features 8 jj + 4 lh + t, i.e. four more float4 of
// the NEXT layer's A operand -- bias, activation, LayerNorm and the residual adds happen in that layout, in registers, and nothing
// crosses LDS between layers.  Weights stream through a 3-stage LDS ring of 32-row chunks shared by the waves of the workgroup
// (LDS DMA, XOR-swizzled 128-B-row image as in conv_gemm_dma_kernel; one barrier per chunk; the DMA of chunk q + 2 is issued at the
// start of step q, but every step opens with s_waitcnt vmcnt(0), so a chunk has ONE step -- 64 MFMAs per wave -- to land, not two).
// Per layer the k pairing and summation order are those of the other kernels: bit-identical.
#define RC_NW 4                                                  // waves per workgroup, two workgroups per CU (starting half of them half a
                                                                 // step late so that co-resident waves run out of phase: measured neutral)
__global__ __launch_bounds__(256, 2) void rowchain128_kernel(const st_chain_desc d) {
    constexpr int NJ = 16, NW = RC_NW;
    extern __shared__ __attribute__((aligned(1024))) float smem[];
    float* ring = smem;                                        // [3][32 rows][128 k] unpadded, 16-B slots XOR-swizzled by (row & 15)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int nblk = (d.M + 31) >> 5;
    const int G = (int)gridDim.x;
    const int blk0 = (int)blockIdx.x * NW;
    const int rounds = blk0 < nblk ? (nblk - blk0 + G * NW - 1) / (G * NW) : 0;
    const int L = d.nlayers, steps = 4 * L, total = rounds * steps;
    if (total == 0) return;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) float*)smem;

    // weight chunk q of the (round-periodic) sequence = rows [32c, 32c + 32) of layer (q % steps) / 4 -> ring stage q % 3, by LDS DMA:
    // 16 pieces of 1 KiB (two rows each), 16 / NW per wave; lane l of a piece writes slot l & 31 of row 2p + (l >> 5), which holds
    // k-chunk slot ^ (row & 15) (the swizzle is applied on the source side)
    auto dma_chunk = [&](int q) {
        const int qq = q % steps, l = qq >> 2, c = qq & 3;
        const i32x4 rs = make_rsrc(d.layer[l].w, 128 * 128 * 4);
#pragma unroll
        for (int u = 0; u < 16 / NW; ++u) {
            const int p = wave * (16 / NW) + u, r = 2 * p + (lane >> 5);
            const unsigned voff = (unsigned)(((c * 32 + r) * 128 + (((lane & 31) ^ (r & 15)) << 2)) * 4);
            lds_dma16(rs, lds0 + (unsigned)(((q % 3) * 32 * 128 + p * 256) * 4), voff, 0u);
        }
    };
    dma_chunk(0);
    if (total > 1) dma_chunk(1);
    // fragment slot offsets (floats) of this lane: 16-B slot (2j + lh) ^ (li & 15) -- the XOR touches the low four bits only
    int foff[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) foff[j] = (((2 * j + lh) ^ (li & 15)) << 2);

    float4 a[NJ], an[NJ], sv[NJ];
    int q = 0;
    for (int rd = 0; rd < rounds; ++rd) {
        const int blk = blk0 + wave + rd * G * NW;
        const bool active = blk < nblk;                         // wave-uniform; idle waves still load weights and meet the barriers
        const int row = blk * 32 + li;
        const bool rok = active && row < d.M;
        if (active) {
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                a[j] = rok ? *reinterpret_cast<const float4*>(d.a + (size_t)row * d.lda + 8 * j + 4 * lh) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        for (int l = 0; l < L; ++l) {
            const st_chain_layer& Ly = d.layer[l];
            if (active) {
                // a later layer adds THIS layer's input (before its LN) as residual: keep a copy (parking it in the block's rows of `out`
                // instead frees 64 registers and removes the ~30 spilled ones, but its 67 MB of extra traffic cost 5 us per launch: measured)
                bool keep = false;
                for (int m = l; m < L; ++m) keep = keep || (d.layer[m].res == 2 && d.layer[m].res_layer == l);
                if (keep) {
#pragma unroll
                    for (int j = 0; j < NJ; ++j) sv[j] = a[j];
                }
                if (Ly.ln) {
                    float s = 0.f;
#pragma unroll
                    for (int j = 0; j < NJ; ++j) s += (a[j].x + a[j].y) + (a[j].z + a[j].w);
                    s += __shfl_xor(s, 32, 64);
                    const float mean = s * (1.0f / 128.0f);
                    float v = 0.f;
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        a[j].x -= mean; a[j].y -= mean; a[j].z -= mean; a[j].w -= mean;
                        v += (a[j].x * a[j].x + a[j].y * a[j].y) + (a[j].z * a[j].z + a[j].w * a[j].w);
                    }
                    v += __shfl_xor(v, 32, 64);
                    const float rstd = 1.0f / sqrtf(v * (1.0f / 128.0f) + Ly.ln_eps);
#pragma unroll
                    for (int j = 0; j < NJ; ++j) { a[j].x *= rstd; a[j].y *= rstd; a[j].z *= rstd; a[j].w *= rstd; }
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c, ++q) {
                // chunk q (DMA issued two steps ago; the vmcnt(0) below also drains chunk q + 1, issued one step ago, so the ring's
                // effective lead is one step) is in the ring once every wave's pieces have landed; everyone is past chunk q - 1,
                // whose stage chunk q + 2 may now overwrite
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (q + 2 < total) dma_chunk(q + 2);
                if (active) {
                    const float* wb = ring + (q % 3) * 32 * 128 + li * 128;
                    // bias of the 16 output features this lane ends up holding (see below): four runs of four
                    float4 bv[4];
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj)
                        bv[jj] = Ly.bias ? *reinterpret_cast<const float4*>(Ly.bias + c * 32 + 8 * jj + 4 * lh) : make_float4(0.f, 0.f, 0.f, 0.f);
                    f32x16 acc;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                    float4 b = *reinterpret_cast<const float4*>(wb + foff[0]);
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        const int jn = j + 1 < NJ ? j + 1 : j;
                        const float4 bn = *reinterpret_cast<const float4*>(wb + foff[jn & 7] + (jn >> 3) * 64);
                        // TRANSPOSED product D[n][m] = sum_k W[n][k] X[m][k]: the weight fragment is the first MFMA operand, the
                        // activations the second (same products, same k order: the same bits as X . W^T).  Lane (li, lh) then holds
                        // row m = li and output features n = (r & 3) + 8 (r >> 2) + 4 lh, r = 0..15 -- which IS the A-operand layout
                        // of the next layer (k = 8 j + 4 lh + t with j = r >> 2, t = r & 3): no trip through LDS between layers.
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.x, a[j].x, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.y, a[j].y, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.z, a[j].z, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.w, a[j].w, acc, 0, 0, 0);
                        b = bn;
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    float v[16];
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        v[4 * jj] = acc[4 * jj] + bv[jj].x; v[4 * jj + 1] = acc[4 * jj + 1] + bv[jj].y;
                        v[4 * jj + 2] = acc[4 * jj + 2] + bv[jj].z; v[4 * jj + 3] = acc[4 * jj + 3] + bv[jj].w;
                    }
                    if (Ly.act == ST_ACT_GELU) {                 // wave-uniform, outside the register loop (none / relu / gelu only)
#pragma unroll
                        for (int r = 0; r < 16; ++r) v[r] = st_gelu(v[r]);
                    } else if (Ly.act == ST_ACT_RELU) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) v[r] = fmaxf(v[r], 0.f);
                    }
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) an[4 * c + jj] = make_float4(v[4 * jj], v[4 * jj + 1], v[4 * jj + 2], v[4 * jj + 3]);
                }
            }
            if (active) {
                if (Ly.res == 1) {
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        const float4 x = rok ? *reinterpret_cast<const float4*>(Ly.res_ptr + (size_t)row * Ly.ld_res + 8 * j + 4 * lh) : make_float4(0.f, 0.f, 0.f, 0.f);
                        an[j].x += x.x; an[j].y += x.y; an[j].z += x.z; an[j].w += x.w;
                    }
                } else if (Ly.res == 2) {
#pragma unroll
                    for (int j = 0; j < NJ; ++j) { an[j].x += sv[j].x; an[j].y += sv[j].y; an[j].z += sv[j].z; an[j].w += sv[j].w; }
                }
                if (l == L - 1) {
                    if (rok) {
#pragma unroll
                        for (int j = 0; j < NJ; ++j) *reinterpret_cast<float4*>(d.out + (size_t)row * d.ldo + 8 * j + 4 * lh) = an[j];
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < NJ; ++j) a[j] = an[j];
                }
            }
        }
    }
}

extern "C" int st_abi_chain_desc_size(void) { return (int)sizeof(st_chain_desc); }

extern "C" int st_linear_chain128(const st_chain_desc* desc, void* stream) {
    if (!desc) return ST_EINVAL;
    const st_chain_desc& d = *desc;
    if (!d.a || !d.out || d.M <= 0 || d.nlayers < 1 || d.nlayers > 3 || d.lda < 128 || d.ldo < 128 || (d.lda & 3) || (d.ldo & 3) ||
        ((uintptr_t)d.a & 15) || ((uintptr_t)d.out & 15) || (int64_t)d.M * (d.lda > d.ldo ? d.lda : d.ldo) >= ((int64_t)1 << 40))
        return ST_EINVAL;
    for (int l = 0; l < d.nlayers; ++l) {
        const st_chain_layer& y = d.layer[l];
        if (!y.w || ((uintptr_t)y.w & 15) || y.act < 0 || y.act > ST_ACT_GELU || y.res < 0 || y.res > 2) return ST_EINVAL;
        if (y.res == 1 && (!y.res_ptr || y.ld_res < 128 || (y.ld_res & 3) || ((uintptr_t)y.res_ptr & 15))) return ST_EINVAL;
        if (y.res == 2 && (y.res_layer < 0 || y.res_layer > l)) return ST_EINVAL;
        if (y.bias && ((uintptr_t)y.bias & 15)) return ST_EINVAL;        // read with 16-byte loads
    }
    {
        // the kernel keeps ONE saved layer input (`sv`): every res == 2 layer must name the same res_layer -- a second one would
        // overwrite the copy a later layer still needs and silently add the wrong tensor
        int saved = -1;
        for (int l = 0; l < d.nlayers; ++l)
            if (d.layer[l].res == 2) {
                if (saved >= 0 && d.layer[l].res_layer != saved) return ST_EINVAL;
                saved = d.layer[l].res_layer;
            }
    }
    const int nblk = (d.M + 31) / 32;
    int G = (nblk + RC_NW - 1) / RC_NW;
    if (G > 512) G = 512;                                       // two workgroups per CU
    const size_t lds = (size_t)(3 * 32 * 128) * sizeof(float);
    (void)hipFuncSetAttribute((const void*)rowchain128_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    // the profiling observer sees the chain as one launch of the family: M x (128 * nlayers) x 128 (its FLOPs; the A + W + C byte
    // formula of the tools then counts the intermediate activations that this kernel does NOT move)
    st_gemm_desc od;
    const bool obs = row_launch_begin(od, 5, 30, stream, d.a, d.lda, d.out, d.ldo, d.layer[0].w, d.M, 128 * d.nlayers, 0);
    hipLaunchKernelGGL(rowchain128_kernel, dim3(G), dim3(64 * RC_NW), lds, (hipStream_t)stream, d);
    if (obs) st_observe(&od, stream, 1);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// ---------------------------------------------------------------------------------------------
// The Twins MLP (timm Mlp, twins.py:785-790: x + fc2(GELU(fc1(LN(x)))), C = 128, hidden = 512) as ONE launch: the hidden
// activations never leave the CU.  Unfused, fc1's [M, 512] tensor is written and read back: 268 MB per MLP at M = 65536, and fc1
// and fc2 are two K = 128 / N = 128 launches at 0.53 / 0.66 of the fp32-MFMA peak (profiles/r3_gemm_shapes.csv).
// Structure = rowchain128_kernel's: a wave owns a 32-row block whose LayerNorm'ed rows sit in registers in the MFMA operand
// layout; the hidden dimension is walked in chunks of 32 features:
//   stage A   h = GELU(W1[32 hc .. +32, :] . x^T + b1)     64 MFMAs, TRANSPOSED product (weights first): lane (li, lh) then holds
//             row li's hidden features 8 j + 4 lh + t of the chunk -- the operand layout of the k slice [32 hc, 32 hc + 32) of fc2
//   stage B   o[oc] += W2[32 oc .. +32, 32 hc .. +32] . h^T, oc = 0..3     64 MFMAs, transposed again: four accumulator tiles whose
//             layout is the block's own row layout, so bias, the residual x (re-read: it is L2-warm) and the optional second
//             residual are added in registers and stored as 16-byte runs.
// Per step the workgroup's four waves share W1's chunk (32 x 128) and W2's slice (128 x 32) through a 2-stage LDS ring filled by
// LDS-DMA one step ahead (32 KB per stage, 64 KB per workgroup, two workgroups per CU), one barrier per step.  k pairing and order
// inside both products are those of the other kernels (k = 8 j + 4 lane_half + t); fc1 is bit-identical to the unfused launch,
// fc2 accumulates its 512 k in ONE chain (the unfused kernels fold at k = 256; holding that fold would need 64 more registers
// per lane than two waves per SIMD have) -- same products, the sum differs in the last bits.
#define MLP_NW 4
template <bool PROJ>
__global__ __launch_bounds__(256, 2) void rowmlp128_kernel(const st_mlp_desc d) {
    constexpr int NJ = 16, NW = MLP_NW, STAGE = 2 * 32 * 128;   // floats per ring stage: [W1 chunk 32 x 128 | W2 slice 128 x 32]
    extern __shared__ __attribute__((aligned(1024))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int nblk = (d.M + 31) >> 5;
    const int G = (int)gridDim.x;
    const int blk0 = (int)blockIdx.x * NW;
    const int rounds = blk0 < nblk ? (nblk - blk0 + G * NW - 1) / (G * NW) : 0;
    // optional leading layer (the attention output projection of the Block, twins.py:622-623 / 676-677): x = a . wp^T + bp + res0,
    // four more steps of 32 output features each in front of the hidden chunks; x then takes a's place
    constexpr bool proj = PROJ;
    const int npre = proj ? 4 : 0;
    const int nhc = d.hidden >> 5, spr = npre + nhc, total = rounds * spr;
    if (total == 0) return;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) float*)smem;
    const i32x4 rs1 = make_rsrc(d.w1, (unsigned)d.hidden * 128u * 4u), rs2 = make_rsrc(d.w2, 128u * (unsigned)d.hidden * 4u);
    const i32x4 rsp = make_rsrc(proj ? d.wp : d.w1, 128u * 128u * 4u);

    // step q = step s = q % spr of a round -> ring stage q & 1.  s < npre: chunk s of wp (image of a W1 chunk); otherwise hidden chunk
    // hc = s - npre.  W1 chunk: 16 pieces of 1 KiB = two 512-B rows, slot t of row r holds k-chunk t ^ (r & 15) (rowchain128's image).
    // W2 slice: 16 pieces of 1 KiB = eight 128-B rows, slot t of row r holds k-chunk t ^ ((r >> 1) & 7) (conv_gemm_dma's image).
    // The swizzles are applied on the source side; 8 (4 for a wp step) pieces per wave and step.
    auto dma_step = [&](int q) {
        const int s = __builtin_amdgcn_readfirstlane(q % spr);
        const bool pre = PROJ && s < npre;
        const int hc = pre ? s : s - npre;
        const unsigned st = lds0 + (unsigned)((q & 1) * STAGE * 4);
        if (pre) {                                              // (a scalar branch: the descriptor operand of the DMA must be an SGPR quad)
#pragma unroll
            for (int u = 0; u < 16 / NW; ++u) {
                const int p = wave * (16 / NW) + u, r = 2 * p + (lane >> 5);
                lds_dma16(rsp, st + (unsigned)(p * 1024), (unsigned)((((hc << 5) + r) * 128 + (((lane & 31) ^ (r & 15)) << 2)) * 4), 0u);
            }
        } else {
#pragma unroll
            for (int u = 0; u < 16 / NW; ++u) {
                const int p = wave * (16 / NW) + u, r = 2 * p + (lane >> 5);
                lds_dma16(rs1, st + (unsigned)(p * 1024), (unsigned)((((hc << 5) + r) * 128 + (((lane & 31) ^ (r & 15)) << 2)) * 4), 0u);
            }
        }
        if (!pre) {
#pragma unroll
            for (int u = 0; u < 16 / NW; ++u) {
                const int p = wave * (16 / NW) + u, r = 8 * p + (lane >> 3);
                const unsigned voff = (unsigned)((r * d.hidden + (((lane & 7) ^ ((r >> 1) & 7)) << 2)) * 4);
                lds_dma16(rs2, st + (unsigned)(32 * 128 * 4 + p * 1024), voff, (unsigned)(hc << 7));
            }
        }
    };
    dma_step(0);
    if (total > 1) dma_step(1);                                 // both stages are free at the start
    int foff[8], goff[4];
#pragma unroll
    for (int j = 0; j < 8; ++j) foff[j] = (((2 * j + lh) ^ (li & 15)) << 2);
#pragma unroll
    for (int j = 0; j < 4; ++j) goff[j] = li * 32 + (((2 * j + lh) ^ ((li >> 1) & 7)) << 2);

    // one K = 128 product of the block with the 32-row weight chunk in ring stage (q & 1): TRANSPOSED (weights first), so lane (li, lh)
    // ends up with row li's output features 8 jj + 4 lh + t of the chunk
    float4 a[NJ];
    auto chunk128 = [&](const float* ws) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        float4 b = *reinterpret_cast<const float4*>(ws + foff[0]);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int jn = j + 1 < NJ ? j + 1 : j;
            const float4 bn = *reinterpret_cast<const float4*>(ws + foff[jn & 7] + (jn >> 3) * 64);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.x, a[j].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.y, a[j].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.z, a[j].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.w, a[j].w, acc, 0, 0, 0);
            b = bn;
            __builtin_amdgcn_sched_barrier(0);
        }
        return acc;
    };
    auto step_sync = [&](int q) {
        // step q's weights (DMA issued one step ago; steps 0 and 1 before the loop) are in the ring once every wave's pieces have
        // landed; everyone is past step q - 1, whose stage step q + 1 may now overwrite
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (q > 0 && q + 1 < total) dma_step(q + 1);
    };

    const float* xres = proj ? d.out : d.a;                      // where the rows the MLP adds back live (x is parked in `out` when computed here)
    const int ld_xres = proj ? d.ldo : d.lda;
    int q = 0;
    for (int rd = 0; rd < rounds; ++rd) {
        const int blk = blk0 + wave + rd * G * NW;
        const bool active = blk < nblk;                         // wave-uniform; idle waves still load weights and meet the barriers
        const int row = blk * 32 + li;
        const bool rok = active && row < d.M;
        const size_t rowc = (size_t)(row < d.M ? row : d.M - 1);   // rows past M (last block only) read a valid row and are never stored:
        if (active) {                                           // unconditional loads, no per-lane branches around them
#pragma unroll
            for (int j = 0; j < NJ; ++j) a[j] = *reinterpret_cast<const float4*>(d.a + rowc * d.lda + 8 * j + 4 * lh);
        }
        if (proj) {
            // x = a . wp^T + bp + res0, 32 features per step, written straight to the block's rows of `out` and read back below: x is
            // needed twice (as this MLP's input and as its residual) and holding both a and x in registers next to the accumulators
            // does not fit two waves per SIMD (hipcc spilled 55 registers); the rows are L2-warm when they come back
#pragma unroll 1
            for (int c = 0; c < 4; ++c, ++q) {
                step_sync(q);
                if (active) {
                    // bias and residual of the 16 features this lane ends up holding: requested before the MFMAs, used after them
                    float4 bv[4], ev[4];
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        const int col = (c << 5) + 8 * jj + 4 * lh;
                        // (wave-uniform conditions: scalar branches, no exec masking)
                        bv[jj] = d.bp ? *reinterpret_cast<const float4*>(d.bp + col) : make_float4(0.f, 0.f, 0.f, 0.f);
                        ev[jj] = d.res0 ? *reinterpret_cast<const float4*>(d.res0 + rowc * d.ld_res0 + col) : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                    const f32x16 acc = chunk128(smem + (q & 1) * STAGE + li * 128);
                    if (rok) {
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) {
                            // (acc + bias) + residual: the unfused epilogue's order
                            *reinterpret_cast<float4*>(d.out + rowc * d.ldo + (c << 5) + 8 * jj + 4 * lh) =
                                make_float4((acc[4 * jj] + bv[jj].x) + ev[jj].x, (acc[4 * jj + 1] + bv[jj].y) + ev[jj].y,
                                            (acc[4 * jj + 2] + bv[jj].z) + ev[jj].z, (acc[4 * jj + 3] + bv[jj].w) + ev[jj].w);
                        }
                    }
                }
            }
            if (active) {
                // the stores above are complete (written through to L2; the vector L1 does not allocate on a store, and these rows were
                // never read by this CU before) -> read x back in the operand layout
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
                for (int j = 0; j < NJ; ++j) a[j] = *reinterpret_cast<const float4*>(d.out + rowc * d.ldo + 8 * j + 4 * lh);
            }
        }
        if (active && d.ln) {                                   // LayerNorm without affine (gamma / beta are folded into w1 / b1): as rowchain128
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) s += (a[j].x + a[j].y) + (a[j].z + a[j].w);
            s += __shfl_xor(s, 32, 64);
            const float mean = s * (1.0f / 128.0f);
            float v = 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                a[j].x -= mean; a[j].y -= mean; a[j].z -= mean; a[j].w -= mean;
                v += (a[j].x * a[j].x + a[j].y * a[j].y) + (a[j].z * a[j].z + a[j].w * a[j].w);
            }
            v += __shfl_xor(v, 32, 64);
            const float rstd = 1.0f / sqrtf(v * (1.0f / 128.0f) + d.ln_eps);
#pragma unroll
            for (int j = 0; j < NJ; ++j) { a[j].x *= rstd; a[j].y *= rstd; a[j].z *= rstd; a[j].w *= rstd; }
        }
        __builtin_amdgcn_sched_barrier(0);                      // (keeps the 64 accumulator zeros below from being scheduled above the projection)
        f32x16 o[4];
#pragma unroll
        for (int oc = 0; oc < 4; ++oc)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[oc][r] = 0.f;
        for (int hc = 0; hc < nhc; ++hc, ++q) {
            step_sync(q);
            if (active) {
                const float* w2s = smem + (q & 1) * STAGE + 32 * 128;
                float4 bv[4];
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) bv[jj] = *reinterpret_cast<const float4*>(d.b1 + (hc << 5) + 8 * jj + 4 * lh);
                // ---- stage A: hidden chunk, K = 128
                const f32x16 acc = chunk128(smem + (q & 1) * STAGE + li * 128);
                // first W2 fragments of stage B are requested before the GELU arithmetic
                float4 g[4];
#pragma unroll
                for (int oc = 0; oc < 4; ++oc) g[oc] = *reinterpret_cast<const float4*>(w2s + oc * 1024 + goff[0]);
                float4 hq[4];
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    hq[jj].x = st_gelu(acc[4 * jj] + bv[jj].x); hq[jj].y = st_gelu(acc[4 * jj + 1] + bv[jj].y);
                    hq[jj].z = st_gelu(acc[4 * jj + 2] + bv[jj].z); hq[jj].w = st_gelu(acc[4 * jj + 3] + bv[jj].w);
                }
                __builtin_amdgcn_sched_barrier(0);
                // ---- stage B: the chunk is the k slice [32 hc, 32 hc + 32) of fc2; four independent accumulator tiles
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float4 gn[4];
                    const int jn = j + 1 < 4 ? j + 1 : j;
#pragma unroll
                    for (int oc = 0; oc < 4; ++oc) gn[oc] = *reinterpret_cast<const float4*>(w2s + oc * 1024 + goff[jn]);
#pragma unroll
                    for (int oc = 0; oc < 4; ++oc) o[oc] = __builtin_amdgcn_mfma_f32_32x32x2f32(g[oc].x, hq[j].x, o[oc], 0, 0, 0);
#pragma unroll
                    for (int oc = 0; oc < 4; ++oc) o[oc] = __builtin_amdgcn_mfma_f32_32x32x2f32(g[oc].y, hq[j].y, o[oc], 0, 0, 0);
#pragma unroll
                    for (int oc = 0; oc < 4; ++oc) o[oc] = __builtin_amdgcn_mfma_f32_32x32x2f32(g[oc].z, hq[j].z, o[oc], 0, 0, 0);
#pragma unroll
                    for (int oc = 0; oc < 4; ++oc) o[oc] = __builtin_amdgcn_mfma_f32_32x32x2f32(g[oc].w, hq[j].w, o[oc], 0, 0, 0);
#pragma unroll
                    for (int oc = 0; oc < 4; ++oc) g[oc] = gn[oc];
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        if (rok) {
            // out = (fc2 + b2) + x [+ res]: the unfused epilogue's order (fma(acc, 1, bias), + aux0, + aux1).  The pointer is laundered
            // per round: b2's 16 loads are invariant across the rounds loop and hipcc otherwise hoists them to the top of the kernel,
            // where they hold 64 registers for its whole length (the projection variant then spilled 55)
            const float* b2p = d.b2;
            asm volatile("" : "+s"(b2p));
#pragma unroll
            for (int oc = 0; oc < 4; ++oc)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int col = oc * 32 + 8 * jj + 4 * lh;
                    const float4 bb = *reinterpret_cast<const float4*>(b2p + col);
                    const float4 x = *reinterpret_cast<const float4*>(xres + rowc * ld_xres + col);
                    float4 v = make_float4((o[oc][4 * jj] + bb.x) + x.x, (o[oc][4 * jj + 1] + bb.y) + x.y, (o[oc][4 * jj + 2] + bb.z) + x.z,
                                           (o[oc][4 * jj + 3] + bb.w) + x.w);
                    if (d.res) {
                        const float4 e = *reinterpret_cast<const float4*>(d.res + rowc * d.ld_res + col);
                        v.x += e.x; v.y += e.y; v.z += e.z; v.w += e.w;
                    }
                    *reinterpret_cast<float4*>(d.out + rowc * d.ldo + col) = v;
                }
        }
    }
}

extern "C" int st_abi_mlp_desc_size(void) { return (int)sizeof(st_mlp_desc); }

extern "C" int st_mlp128(const st_mlp_desc* desc, void* stream) {
    if (!desc) return ST_EINVAL;
    const st_mlp_desc& d = *desc;
    if (!d.a || !d.out || !d.w1 || !d.b1 || !d.w2 || !d.b2 || d.M <= 0 || d.hidden < 32 || d.hidden > 2048 || (d.hidden & 31) || d.lda < 128 ||
        d.ldo < 128 || (d.lda & 3) || (d.ldo & 3) || d.reserved != 0 || (int64_t)d.M * (d.lda > d.ldo ? d.lda : d.ldo) >= ((int64_t)1 << 40))
        return ST_EINVAL;
    if ((((uintptr_t)d.a | (uintptr_t)d.out | (uintptr_t)d.w1 | (uintptr_t)d.b1 | (uintptr_t)d.w2 | (uintptr_t)d.b2) & 15)) return ST_EINVAL;
    if (d.res && (d.ld_res < 128 || (d.ld_res & 3) || ((uintptr_t)d.res & 15))) return ST_EINVAL;
    if (d.a == d.out) return ST_EINVAL;                        // the residual x is re-read at the end of a block: not in place
    if (d.wp && (((uintptr_t)d.wp & 15) || (d.bp && ((uintptr_t)d.bp & 15)))) return ST_EINVAL;
    if (!d.wp && (d.bp || d.res0)) return ST_EINVAL;           // bias / residual of a projection that is not there
    if (d.wp && d.res == d.out) return ST_EINVAL;              // with a projection the block's rows of `out` hold the parked x until the end
    if (d.res0 && (d.ld_res0 < 128 || (d.ld_res0 & 3) || ((uintptr_t)d.res0 & 15) || d.res0 == d.out)) return ST_EINVAL;
    const int nblk = (d.M + 31) / 32;
    int G = (nblk + MLP_NW - 1) / MLP_NW;
    if (G > 512) G = 512;                                       // two workgroups per CU
    const size_t lds = (size_t)(2 * 2 * 32 * 128) * sizeof(float);
    auto kern = d.wp ? rowmlp128_kernel<true> : rowmlp128_kernel<false>;
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    // the profiling observer sees the MLP as one launch of the family: M x (2 * hidden) x 128 = its FLOPs (2 M 128 hidden per product)
    st_gemm_desc od;
    const bool obs = row_launch_begin(od, 6, 31, stream, d.a, d.lda, d.out, d.ldo, d.w1, d.M, 2 * d.hidden + (d.wp ? 128 : 0), 0);
    hipLaunchKernelGGL(kern, dim3(G), dim3(64 * MLP_NW), lds, (hipStream_t)stream, d);
    if (obs) st_observe(&od, stream, 1);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

#include "mlp_split3.h"

// bytes of the weight image of st_mlp128_split3 (one 49-KiB LDS stage image per step of the walk)
static int64_t mlp_split3_image_bytes(int32_t hidden, bool with_proj) {
    if (hidden < 32 || hidden > 2048 || (hidden & 31)) return 0;
    return (int64_t)((with_proj ? 4 : 0) + hidden / 32) * MS3_STAGE_B;
}
extern "C" int st_mlp128_split3_image_bytes(int32_t hidden, int32_t with_proj, int64_t* bytes) {
    if (!bytes) return ST_EINVAL;
    *bytes = mlp_split3_image_bytes(hidden, with_proj != 0);
    return *bytes ? ST_OK : ST_EINVAL;
}

extern "C" int st_mlp128_split3_pack(const float* w1, const float* b1, const float* w2, const float* wp, const float* bp, int32_t hidden, void* image,
                                     int64_t image_bytes, void* stream) {
    if (!w1 || !b1 || !w2 || !image || hidden < 32 || hidden > 2048 || (hidden & 31) || ((uintptr_t)image & 15) || (!wp && bp)) return ST_EINVAL;
    if (image_bytes < mlp_split3_image_bytes(hidden, wp != nullptr)) return ST_EINVAL;
    const int steps = (wp ? 4 : 0) + hidden / 32;
    hipLaunchKernelGGL(mlp_split3_pack_kernel, dim3(5, steps), dim3(256), 0, (hipStream_t)stream, w1, b1, w2, wp, bp, (int)hidden, (unsigned char*)image);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// st_mlp128 on the exact-split contraction (csrc/mlp_split3.h).  `desc` as for st_mlp128 -- w1 / b1 / w2 / bp are not read (the image holds them),
// wp != NULL says that the image was packed WITH the projection; b2 is read.
extern "C" int st_mlp128_split3(const st_mlp_desc* desc, const void* image, int64_t image_bytes, void* stream) {
    if (!desc || !image) return ST_EINVAL;
    const st_mlp_desc& d = *desc;
    if (!d.a || !d.out || !d.b2 || d.M <= 0 || d.hidden < 32 || d.hidden > 2048 || (d.hidden & 31) || d.lda < 128 || d.ldo < 128 || (d.lda & 3) ||
        (d.ldo & 3) || d.reserved != 0 || (int64_t)d.M * (d.lda > d.ldo ? d.lda : d.ldo) >= ((int64_t)1 << 40))
        return ST_EINVAL;
    if ((((uintptr_t)d.a | (uintptr_t)d.out | (uintptr_t)d.b2 | (uintptr_t)image) & 15)) return ST_EINVAL;
    if (d.res && (d.ld_res < 128 || (d.ld_res & 3) || ((uintptr_t)d.res & 15))) return ST_EINVAL;
    if (d.a == d.out) return ST_EINVAL;
    if (!d.wp && (d.bp || d.res0)) return ST_EINVAL;
    if (d.res0 && (d.ld_res0 < 128 || (d.ld_res0 & 3) || ((uintptr_t)d.res0 & 15) || d.res0 == d.out)) return ST_EINVAL;
    const int64_t need = mlp_split3_image_bytes(d.hidden, d.wp != nullptr);
    if (!need) return ST_EINVAL;
    if (image_bytes < need || need >= ((int64_t)1 << 31)) return ST_EINVAL;
    const int nblk = (d.M + 31) / 32;
    int G = (nblk + MS3_NWAVES - 1) / MS3_NWAVES;
    if (G > 256) G = 256;                                       // 147 KB of LDS: one workgroup per CU
    const size_t lds = (size_t)3 * MS3_STAGE_B;
    auto kern = d.wp ? rowmlp128_split3_kernel<true> : rowmlp128_split3_kernel<false>;
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    st_gemm_desc od;
    const bool obs = row_launch_begin(od, 9, 38, stream, d.a, d.lda, d.out, d.ldo, image, d.M, 2 * d.hidden + (d.wp ? 128 : 0), 1);
    hipLaunchKernelGGL(kern, dim3(G), dim3(64 * MS3_NWAVES), lds, (hipStream_t)stream, d, (const unsigned char*)image, (unsigned)need);
    if (obs) st_observe(&od, stream, 1);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// LayerNorm -> Linear(128 -> N) + bias on the exact-split contraction (csrc/mlp_split3.h, rowlin128_split3_kernel): the weights packed once into
// N / 32 stage images of 25 KiB
extern "C" int st_rowlin128_split3_image_bytes(int32_t N, int64_t* bytes) {
    if (!bytes || N < 32 || N > 4096 || (N & 31)) return ST_EINVAL;
    *bytes = (int64_t)(N / 32) * LS3_STAGE_B;
    return ST_OK;
}
extern "C" int st_rowlin128_split3_pack(const float* w, const float* b, int32_t N, void* image, int64_t image_bytes, void* stream) {
    if (!w || !image || N < 32 || N > 4096 || (N & 31) || ((uintptr_t)image & 15) || image_bytes < (int64_t)(N / 32) * LS3_STAGE_B) return ST_EINVAL;
    hipLaunchKernelGGL(rowlin_split3_pack_kernel, dim3(3, N / 32), dim3(256), 0, (hipStream_t)stream, w, b, (unsigned char*)image);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
extern "C" int st_rowlin128_split3(const float* a, int32_t lda, float* out, int32_t ldo, int32_t M, int32_t N, int32_t ln, float ln_eps, const void* image,
                                   int64_t image_bytes, const float* aux, int32_t ld_aux, int32_t row_div, void* stream) {
    if (aux && (ld_aux < N || (ld_aux & 3) || row_div < 1 || ((uintptr_t)aux & 15) || aux == out)) return ST_EINVAL;
    if (!a || !out || !image || M <= 0 || N < 32 || N > 4096 || (N & 31) || lda < 128 || ldo < N || (lda & 3) || (ldo & 3) || a == out) return ST_EINVAL;
    if ((((uintptr_t)a | (uintptr_t)out | (uintptr_t)image) & 15) || (int64_t)M * (lda > ldo ? lda : ldo) >= ((int64_t)1 << 40)) return ST_EINVAL;
    const int64_t need = (int64_t)(N / 32) * LS3_STAGE_B;
    if (image_bytes < need) return ST_EINVAL;
    const int nblk = (M + 31) / 32;
    int G = (nblk + 3) / 4;
    if (G > 512) G = 512;                                       // 75 KB of LDS: two workgroups per CU
    const size_t lds = (size_t)3 * LS3_STAGE_B;
    auto kern = aux ? rowlin128_split3_kernel<true> : rowlin128_split3_kernel<false>;
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    st_gemm_desc od;
    const bool obs = row_launch_begin(od, 10, 40, stream, a, lda, out, ldo, image, M, N, 1);
    hipLaunchKernelGGL(kern, dim3(G), dim3(256), lds, (hipStream_t)stream, a, (int)lda, out, (int)ldo, (int)M, (int)N, (int)ln, ln_eps,
                       (const unsigned char*)image, (unsigned)need, aux, (int)ld_aux, (int)(row_div > 0 ? row_div : 1));
    if (obs) st_observe(&od, stream, 1);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// The latent self-attention in one launch (csrc/mlp_split3.h, latent_self_attn_split3_kernel): out[M, 128] = attention(LayerNorm(a) . wqkv^T + bqkv) over
// groups of 8 consecutive rows (the 8 latents of a cost map), 8 heads of 16; w [384, 128] = q | k | v rows, packed once into 12 chunk images + the bias
extern "C" int st_latent_self_attn_split3_image_bytes(int64_t* bytes) {
    if (!bytes) return ST_EINVAL;
    *bytes = LA3_IMAGE_B;
    return ST_OK;
}
extern "C" int st_latent_self_attn_split3_pack(const float* w, const float* b, void* image, int64_t image_bytes, void* stream) {
    if (!w || !image || ((uintptr_t)image & 15) || image_bytes != LA3_IMAGE_B) return ST_EINVAL;
    hipLaunchKernelGGL(latent_self_attn_split3_pack_kernel, dim3(3, LA3_STEPS), dim3(256), 0, (hipStream_t)stream, w, b, (unsigned char*)image);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
extern "C" int st_latent_self_attn_split3(const float* a, int32_t lda, float* out, int32_t ldo, int32_t M, int32_t ln, float ln_eps, float scale,
                                          const void* image, int64_t image_bytes, void* stream) {
    if (!a || !out || !image || M <= 0 || (M & 7) || lda < 128 || ldo < 128 || (lda & 3) || (ldo & 3) || a == out) return ST_EINVAL;
    if ((((uintptr_t)a | (uintptr_t)out | (uintptr_t)image) & 15) || (int64_t)M * (lda > ldo ? lda : ldo) >= ((int64_t)1 << 40)) return ST_EINVAL;
    if (image_bytes != LA3_IMAGE_B) return ST_EINVAL;
    const int nblk = (M + 31) / 32;
    int G = (nblk + 3) / 4;
    if (G > 512) G = 512;                                       // 80 KB of LDS: two workgroups per CU
    const size_t lds = (size_t)LA3_LDS_B;
    (void)hipFuncSetAttribute((const void*)latent_self_attn_split3_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    // reported to the observer as the projection it holds: M x 384 x 128
    st_gemm_desc od;
    const bool obs = row_launch_begin(od, 12, 42, stream, a, lda, out, ldo, image, M, 384, 1);
    hipLaunchKernelGGL(latent_self_attn_split3_kernel, dim3(G), dim3(256), lds, (hipStream_t)stream, a, (int)lda, out, (int)ldo, (int)M, (int)ln, ln_eps,
                       scale, (const unsigned char*)image);
    if (obs) st_observe(&od, stream, 1);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// PatchEmbed's tail (csrc/mlp_split3.h, pe_tail_split3_kernel): tokens[R, 128] = LayerNorm(ReLU(x[R, 64] . w1^T + tab[r % P]) . w2^T + b2) in one launch
extern "C" int st_pe_tail_split3_image_bytes(int64_t* bytes) {
    if (!bytes) return ST_EINVAL;
    *bytes = PT3_IMAGE_B;
    return ST_OK;
}
extern "C" int st_pe_tail_split3_pack(const float* w1, int32_t ld1, const float* w2, void* image, int64_t image_bytes, void* stream) {
    if (!w1 || !w2 || !image || ld1 < 64 || ((uintptr_t)image & 15) || image_bytes < PT3_IMAGE_B) return ST_EINVAL;
    hipLaunchKernelGGL(pe_tail_split3_pack_kernel, dim3(3, 4), dim3(256), 0, (hipStream_t)stream, w1, (int)ld1, w2, (unsigned char*)image);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
extern "C" int st_pe_tail_split3(const float* x, const float* tab, int32_t P, const void* image, int64_t image_bytes, const float* b2, const float* gamma,
                                 const float* beta, float eps, float* out, int32_t R, void* stream) {
    if (!x || !tab || !image || !b2 || !gamma || !beta || !out || R <= 0 || P <= 0 || image_bytes < PT3_IMAGE_B || x == out) return ST_EINVAL;
    if ((((uintptr_t)x | (uintptr_t)tab | (uintptr_t)image | (uintptr_t)out) & 15) || (int64_t)R * 128 >= ((int64_t)1 << 40)) return ST_EINVAL;
    const int nblk = (R + 31) / 32;
    int G = (nblk + 3) / 4;
    if (G > 256) G = 256;                                       // 146 KB of LDS: one workgroup per CU
    // a grid whose row stride (G * 128) is a multiple of the table period keeps a wave's table rows the same for all its blocks: the largest such G <= 256
    bool tabinv = false;
    for (int g = G; g >= (G > 8 ? G - G / 8 : 1); --g)
        if (((long)g * 128) % P == 0) { G = g; tabinv = true; break; }
    const size_t lds = (size_t)PT3_IMAGE_B + PT3_VEC_B;
    auto kern = tabinv ? pe_tail_split3_kernel<true> : pe_tail_split3_kernel<false>;
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    st_gemm_desc od;
    const bool obs = row_launch_begin(od, 11, 41, stream, x, 64, out, 128, image, R, 192, 1);      // reported as R x 192 x 128: its FLOPs (2 R (128 . 64 + 128 . 128))
    hipLaunchKernelGGL(kern, dim3(G), dim3(256), lds, (hipStream_t)stream, x, tab, (const unsigned char*)image, b2, gamma, beta, eps, out, (int)R, (int)P);
    if (obs) st_observe(&od, stream, 1);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
