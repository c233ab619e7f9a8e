/* libstitch_gfx950.so -- C-ABI of the MI355X-native stitching hot path.
 *
 * The reference (gargatik/Seamless-Through-Breaking..., 100 % Python) has no native interface for
 * this path: every operator below replaces stock PyTorch ops called from
 * core/flowHomoAdpater.py:FlowHomoAdpater.forward (the drop-in boundary).  Each entry
 * point cites the reference code it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc'd / torch CUDA tensor .data_ptr()), fp32 unless
 *     stated, 16-byte aligned bases; no allocation, no ownership transfer, no global state
 *   - `stream` is a hipStream_t (0 = default stream); all calls are asynchronous on it
 *   - activations are channels-last: [B, H, W, C] with a row stride `ld*` (floats) >= C, so a
 *     channel slice of a wider buffer is addressable (concatenation = column offset)
 *   - return 0 on success, ST_EINVAL (1001) for a rejected argument, otherwise a hipError_t value
 */
#ifndef STITCH_GFX950_H
#define STITCH_GFX950_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- dense contractions -------------------------------------------------------------------- */
typedef struct st_gemm_desc {
    const float* a;        /* activations, NHWC [B,H,W,ldx] (plain matrix: H=1, W=M, kh=kw=1)      */
    const float* w;        /* weights [N, K] row-major, K ordered (ky, kx, c), row stride ldw       */
    float* c;              /* output [M, ldc], M = B*Ho*Wo                                          */
    const float* bias;     /* [N] or NULL                                                           */
    const float* aux0;     /* pre-activation addend [*, ld_aux0] or NULL; row = (m / aux0_row_div) % aux0_row_mod */
    const float* aux1;     /* epilogue operand [M, ld_aux1] or NULL                                 */
    const float* aux2;     /* epilogue operand [M, ld_aux2] or NULL                                 */
    const float* scale_ptr;/* device scalar for ST_EPI_AXPY or NULL                                 */
    int32_t M, N, K;       /* K = kh*kw*Cin                                                         */
    int32_t H, W, Cin, ldx;
    int32_t kh, kw, sh, sw, ph, pw, Ho, Wo;
    int32_t ldw, ldc, ld_aux0, ld_aux1, ld_aux2;
    int32_t aux0_row_div, aux0_row_mod;   /* 0/1 = identity row mapping                            */
    int32_t act;           /* 0 none, 1 relu, 2 gelu(erf), 3 sigmoid, 4 tanh, 5 leaky relu (0.01)   */
    int32_t epi;           /* 0 store, 1 +aux1, 2 *aux1, 3 GRU blend, 4 aux1 + *scale_ptr * v,
                              5 z|r: cols<N/2 -> c, cols>=N/2 -> c2 = v*aux1                        */
    float alpha;           /* v = act(alpha*acc + bias + aux0)                                      */
    int32_t batch;         /* grid.z batches (0/1 = single)                                         */
    int64_t batch_stride_a, batch_stride_w, batch_stride_c;   /* in floats                          */
    int32_t tile_cfg;      /* 0 = auto; register-staged 1: 128x128, 2: 128x64, 3: 64x64, 4: 128x32;
                              LDS-DMA pipelined (Cin % 32 == 0) 12: 128x64, 13: 64x64, 14: 128x32, 15: 64x128 (never auto);
                              row-streaming (plain matrix, K = 64 / 128) 20 */
    int32_t split_k;       /* 0 = auto, 1 = off, >1 = K slices (needs workspace, batch <= 1)        */
    float* workspace;      /* split-K slabs [split_k, M, N] or NULL (then never split)              */
    int64_t workspace_floats;
    float* c2;             /* second output for epi 5 (fused GRU gates): [M, ldc2]                  */
    int32_t ldc2;
    uint32_t a_bytes, w_bytes;  /* filled by the library: extents of A / W for the buffer descriptors  */
    int32_t reserved0;     /* must be 0 (was the selector of an experimental split-bf16 kernel, removed)           */
    int64_t batch_stride_aux1;  /* floats; aux1 of batch z starts at aux1 + z * batch_stride_aux1          */
    int32_t dh, dw;        /* conv dilation (0 / 1 = dense): tap (ky,kx) reads pixel (oy*sh-ph+ky*dh, ox*sw-pw+kx*dw);
                              Ho / Wo are the caller's (PyTorch: H + 2*ph - dh*(kh-1) - 1) / sh + 1)            */
    int32_t a_ln;          /* 1: every row of A is layer-normalised WITHOUT affine, (x - mean) * rstd over its K = Cin
                              entries, before the contraction (nn.LayerNorm in front of a Linear, twins.py:787-790,
                              encoder.py:156-172; the caller folds gamma into W and beta into the bias).  Row-streaming
                              kernel only: plain matrix, K = 64 / 128, batch <= 1; anything else is rejected          */
    float a_ln_eps;
    const float* a2;       /* optional second source of A with the SAME geometry and row stride: input channels c < a2_channels
                              are read from a2, the others from a (SepConvGRU's q conv reads [r*h | x] as r*h from one
                              buffer and x from the other, gru.py:50, without x being copied).  LDS-DMA kernel only
                              (Cin % 32 == 0, a2_channels % 32 == 0, batch <= 1); anything else is rejected                 */
    int32_t a2_channels;
    int32_t reserved1;     /* must be 0 */
    float* c_t;            /* optional TRANSPOSED copy of the result: c_t[n, m] (row stride ld_ct, batch stride batch_stride_c) receives
                              what c[m, n] receives.  ST_EPI_STORE on the LDS-DMA kernels only, M % 4 == 0, ld_ct % 4 == 0, no split-K:
                              the all-pairs volume of the reverse flow direction is the transpose of the forward one
                              (encoder.py:359-369 evaluated for (f2, f1)) and costs a second store instead of a second product */
    int32_t ld_ct;
    int32_t reserved2;     /* must be 0 */
    int32_t split3;        /* 0: a / w are fp32 (everything above).  1: EXACT-SPLIT operands on the bf16 matrix cores (csrc/gemm_split3.h, launched from csrc/gemm_split3.hip):
                              a, w (and a2) point to THREE bf16 planes hi, mid, lo with x == hi + mid + lo exactly (st_split3_pack or a
                              producing kernel's epilogue), each blocked by 32-channel chunks: plane = [C / 32][rows][32] bf16, the planes
                              a_plane_stride / w_plane_stride ELEMENTS apart; a_rows = rows per chunk of the A planes (all pixels B*H*W of the
                              activation, >= what the geometry addresses), w_rows = rows per chunk of the W planes (>= N; W chunks follow the
                              K order (ky, kx, c / 32)).  ldx / ldw are ignored; batch strides are bf16 elements inside each plane, whole rows (multiples of
                              32), and with batch > 1 the last batch's rows must end inside a_rows / w_rows.  The six
                              products hi.hi, hi.mid, mid.hi, mid.mid, hi.lo, lo.hi are accumulated in fp32 (dropped terms <= 2^-23 |a||b|);
                              epilogue, split-K and outputs exactly as the fp32 kernels.  Cin % 32 == 0; tile_cfg 0 = auto, 31: 128x128,
                              32: 128x64, 33: 64x128, 34: 64x64, 37: 64x64 PERSISTENT walk over the tiles (many short tiles; the only one that
                              takes c_t); a_ln is rejected.                                                 */
    int32_t reserved3;     /* must be 0 */
    int64_t a_plane_stride, w_plane_stride, a_rows, w_rows;
    void* c_planes;        /* optional (any kernel of the family, fp32 or split3 operands): the result ALSO leaves as three blocked bf16 planes
                              (the operand format of a split3 consumer), written by the epilogue that produced it -- no separate pass, no split
                              work in any K loop.  Element (m, n) goes to plane p at
                                  c_planes[p * c_plane_stride + (((c_plane_col0 + n) / 32) * c_plane_rows + c_plane_row0 + z * c_plane_batch_rows + m) * 32
                                           + (c_plane_col0 + n) % 32]            (z = batch index)
                              In ST_EPI_ZR mode the planes receive the SECOND output (c2 = r*h, column n - N/2).  M % 32 == 0 and
                              c_plane_col0 % 32 == 0 are required; c_no_f32 = 1 skips the fp32 store of that output (its c / c2 pointer must
                              still be valid: split-K partial sums and the z half are unaffected).                                        */
    int64_t c_plane_stride, c_plane_rows, c_plane_batch_rows;
    int32_t c_plane_col0, c_plane_row0, c_no_f32, reserved4;
} st_gemm_desc;

/* fp32 MFMA implicit GEMM: nn.Linear / F.conv2d / einsum on the path, e.g.
 *   core/FlowFormer/PerCostFormer3/encoder.py:359-369 (corr), :60-95 (PatchEmbed convs),
 *   gru.py:44-59,246-254,5-13 (SepConvGRU, motion encoder, heads), gma.py:54-76,102-115,
 *   twins.py:253-392,587-680 (q/k/v/proj/sr/MLP), core/UDIS2/Homography/network.py:18-46,103-137. */
int st_conv_gemm(const st_gemm_desc* desc, void* stream);

/* fp32 rows [rows, ldx] (C columns, C % 32 == 0) -> the three blocked bf16 planes st_gemm_desc.split3 consumes:
 * planes[p * plane_stride + ((c / 32) * chunk_rows + row) * 32 + c % 32], p = 0 (hi), 1 (mid), 2 (lo); x == hi + mid + lo exactly
 * (+-inf / NaN stay in hi alone).  Used once per weight at pack time and for activations no split3-emitting kernel produced.
 * Operands of: gru.py:44-59,246-254, gma.py:102-115, encoder.py:359-369.                                                   */
/* All-pairs volume(s) from the feature maps' PLANES (st_split3_pack of f1 / f2 rows [B*N, C]; sample b = rows b*N ..): vol12[b] = f1[b] . f2[b]^T and, when vol21
 * is not NULL, its transpose from the same launch -- the split3 form of st_corr_volume / st_corr_volume_both on the persistent 64x64 kernel
 * (tile_cfg 37: a workgroup walks its tiles with one continuous DMA ring).  encoder.py:359-369.                                       */
int st_corr_volume_split3(const void* f1_planes, const void* f2_planes, int64_t pstride, int64_t prows, float* vol12, float* vol21, int32_t B,
                          int32_t N, int32_t C, void* stream);
int st_split3_pack(const float* x, void* planes, int64_t rows, int32_t C, int64_t ldx, int64_t plane_stride, int64_t chunk_rows, void* stream);

/* Two independent contractions in ONE launch: workgroups of both descriptors share the grid, so two mid-size convs that are
 * ready together (BasicMotionEncoder's convc2 and convf2, gru.py:252-253) fill the chip without split-K slabs or a second
 * launch.  Both must be LDS-DMA-kernel shapes (Cin % 32 == 0, K >= 128), batch <= 1, no split-K, no a_ln; results are
 * bit-identical to two st_conv_gemm calls.                                                                            */
int st_conv_gemm_pair(const st_gemm_desc* desc0, const st_gemm_desc* desc1, void* stream);

/* Profiling observer, off by default: `callback` is a
 *   void (*)(const st_gemm_desc*, void* stream, int32_t phase, void* user)
 * invoked on the launching thread before (phase 0) and after (phase 1) every st_conv_gemm enqueues its kernels
 * (also for the GEMMs launched by the operator-level entry points below), so a caller can bracket them with HIP
 * events on `stream`.  NULL switches it off.  Process-wide; do not change it while other threads launch.   */
int st_set_gemm_observer(void* callback, void* user);

/* Profiling aid: the launch plan the library chose for the calling thread's most recent st_conv_gemm:
 *   plan4[0] kernel family (0 skinny_gemm, 1 narrow_conv, 2 conv_gemm_kernel [register-staged], 3 conv_gemm_dma_kernel,
 *            4 rowstream_gemm_kernel, 5 rowchain128_kernel [st_linear_chain128, reported to the observer as M x 128L x 128],
 *            6 rowmlp128_kernel [st_mlp128, reported as M x 2 hidden x 128], 7 patch_c0c2_kernel [st_patch_conv12], 8 conv_gemm_split3_kernel
 *            [st_gemm_desc.split3: tile_cfg 31..37], 9 rowmlp128_split3_kernel [st_mlp128_split3], 10 rowlin128_split3_kernel [st_rowlin128_split3], 11 pe_tail_split3_kernel [st_pe_tail_split3],
 *            12 latent_self_attn_split3_kernel [st_latent_self_attn_split3])
 *   plan4[1] tile_cfg actually used, plan4[2] split_k actually used, plan4[3] 1 = persistent M walk, 2 / 3 = first / second
 *            member of an st_conv_gemm_pair launch (one dispatch, reported with the second member).
 * Used by tools/gemm_shapes_csv.py to label every launch of a step (profiles/r2_gemm_shapes.csv). */
int st_gemm_last_plan(int32_t* plan4);

/* The dispatch decision alone, from the functions st_conv_gemm / st_conv_gemm_pair run themselves.  pair_with == NULL: returns what
 * st_conv_gemm(desc) returns before it launches anything (0, or 1001 for a descriptor it rejects) and, on 0, writes to plan4 the four values
 * st_gemm_last_plan reports after that call (for a descriptor whose rows run in chunks: those of its last chunk).  pair_with != NULL: the same for
 * st_conv_gemm_pair(desc, pair_with).  Host arithmetic only: no launch, no HIP call, none of the descriptor's pointers is followed (their
 * alignment is read), and the calling thread's last plan stays as it is.  For callers that want to know the kernel before they launch
 * and for tests/test_gemm_plan_cpu.py, which pins the dispatch table without a GPU. */
int st_gemm_plan(const st_gemm_desc* desc, const st_gemm_desc* pair_with, int32_t* plan4);

/* sizeof(st_gemm_desc) as compiled into the library (binding self-check; returns the size). */
int st_abi_gemm_desc_size(void);

/* A chain of up to 3 Linear(128 -> 128) layers over the rows of a matrix, evaluated without the intermediate activations
 * leaving the CU (the tail of the latent layers: `proj + residual -> LayerNorm -> ffn.0 + GELU -> ffn.3 + residual`,
 * crossattentionlayer.py:46-56, encoder.py:163-172):
 *   x_0 = a;   x_{l+1} = act_l( LN_l(x_l) . w_l^T + bias_l ) + residual_l ;   out = x_nlayers
 * LN_l (ln = 1): layer norm of the row WITHOUT affine (the caller folds gamma / beta into w_l / bias_l);
 * residual_l: res = 0 none, 1 = rows of the global matrix res_ptr (row stride ld_res), 2 = x_{res_layer} (an earlier
 * layer's input before its LN).  w_l [128,128] row-major contiguous, bias_l [128], both 16-byte aligned.  Same k pairing and
 * summation order per layer as st_conv_gemm (bit-identical to the unfused chain).  The kernel keeps ONE saved layer input:
 * all res = 2 layers of a chain must name the same res_layer (ST_EINVAL otherwise).                                      */
typedef struct st_chain_layer {
    const float* w;
    const float* bias;
    const float* res_ptr;
    int32_t ld_res;
    int32_t act;           /* 0 none, 1 relu, 2 gelu                                                                      */
    int32_t ln;
    float ln_eps;
    int32_t res;
    int32_t res_layer;
} st_chain_layer;
typedef struct st_chain_desc {
    const float* a;        /* [M, lda], 128 columns used                                                                  */
    float* out;            /* [M, ldo]                                                                                    */
    int32_t lda, ldo, M, nlayers;
    st_chain_layer layer[3];
} st_chain_desc;
int st_linear_chain128(const st_chain_desc* desc, void* stream);
int st_abi_chain_desc_size(void);

/* The Twins / vertical-layer MLP of C = 128 rows (timm Mlp inside Block, twins.py:785-790; encoder.py:121-125):
 *   out = a + ( GELU( LN(a) . w1^T + b1 ) . w2^T + b2 ) [+ res]
 * as one launch (rowmlp128_kernel): the [M, hidden] activations never reach HBM.  LN (ln = 1): layer norm WITHOUT affine, the
 * caller folds gamma / beta into w1 / b1.  w1 [hidden, 128], w2 [128, hidden] row-major contiguous; b1 [hidden], b2 [128];
 * hidden % 32 == 0, 32..2048; every pointer 16-byte aligned; out must not alias a.  fc1 + GELU are bit-identical to
 * st_conv_gemm(act = gelu); fc2 sums its `hidden` products in one chain (st_conv_gemm folds every 256 k): same products, the
 * last bits of the sum differ.  plan4[0] = 6; reported to the observer as M x (2 hidden [+ 128 with wp]) x 128.                 */
typedef struct st_mlp_desc {
    const float* a;        /* [M, lda], 128 columns used: input and first residual                                         */
    float* out;            /* [M, ldo]                                                                                    */
    const float* w1;
    const float* b1;
    const float* w2;
    const float* b2;
    const float* res;      /* optional second residual [M, ld_res] (encoder.py:281 short-cut), or NULL                    */
    int32_t lda, ldo, ld_res, M, hidden, ln;
    float ln_eps;
    int32_t reserved;      /* must be 0                                                                                   */
    /* optional leading layer, the Block's attention output projection + residual (twins.py:622-623, 676-677, 790):
     *   x = a . wp^T + bp + res0   takes a's place above (a is then the attention output, x never reaches HBM as a tensor of
     * its own: it is parked in the block's rows of `out` and re-read as the MLP's residual).  wp [128,128]; NULL = absent.   */
    const float* wp;
    const float* bp;
    const float* res0;     /* [M, ld_res0] or NULL; must not alias out                                                    */
    int32_t ld_res0, reserved1;
} st_mlp_desc;
int st_mlp128(const st_mlp_desc* desc, void* stream);
int st_abi_mlp_desc_size(void);
/* st_mlp128 on the exact-split contraction (round 6, csrc/mlp_split3.h in csrc/gemm_rows.hip): every fp32 product of the three GEMMs as six bf16 MFMA
 * products of operand planes (hi / mid / lo), fp32 accumulation; same operator, same `desc`; accuracy against fp64 that of the fp32 MFMA
 * chain or better (tests/test_split3_gpu.py); a non-finite activation gives NaN in its row.  The weights are packed ONCE into an image
 * (one 49-KiB LDS stage per step of the kernel's walk: [wp chunk]* then [w1 chunk | w2 slice | b1 chunk]*):
 *   st_mlp128_split3_image_bytes(hidden, with_proj, &bytes)  size of the image
 *   st_mlp128_split3_pack(w1, b1, w2, wp, bp, hidden, image, image_bytes, stream)   wp / bp NULL = no projection
 *   st_mlp128_split3(desc, image, image_bytes, stream)   desc->w1 / b1 / w2 / bp are not read; desc->wp != NULL <=> the image holds a projection.
 * res may alias out, with the projection as well (x stays in registers; a lane reads its residual values right before it writes the same
 * addresses); st_mlp128 allows that alias without the projection only.  plan4[0] = 9; reported to the observer like st_mlp128 with split3 = 1. */
int st_mlp128_split3_image_bytes(int32_t hidden, int32_t with_proj, int64_t* bytes);
int st_mlp128_split3_pack(const float* w1, const float* b1, const float* w2, const float* wp, const float* bp, int32_t hidden, void* image,
                          int64_t image_bytes, void* stream);
int st_mlp128_split3(const st_mlp_desc* desc, const void* image, int64_t image_bytes, void* stream);
/* out[M, N] = LayerNorm(a)[M, 128] . w^T + b on the exact-split contraction (round 6, csrc/mlp_split3.h, rowlin128_split3_kernel): the q | k | v
 * projections behind norm1 (twins.py:598-600, encoder.py:156-160), i.e. st_conv_gemm with a_ln for K = 128.  ln = 1: layer norm without affine
 * (gamma / beta folded into w / b by the caller), ln = 0: plain rows.  w [N, 128] row-major, b [N] or NULL, N % 32 == 0; weights packed once:
 *   st_rowlin128_split3_image_bytes(N, &bytes), st_rowlin128_split3_pack(w, b, N, image, image_bytes, stream).  aux (or NULL): a table
 * [ceil(M / row_div), ld_aux] whose row (m / row_div) is added to output row m (st_gemm_desc.aux0 with row_div).  plan4[0] = 10.      */
int st_rowlin128_split3_image_bytes(int32_t N, int64_t* bytes);
int st_rowlin128_split3_pack(const float* w, const float* b, int32_t N, void* image, int64_t image_bytes, void* stream);
int st_rowlin128_split3(const float* a, int32_t lda, float* out, int32_t ldo, int32_t M, int32_t N, int32_t ln, float ln_eps, const void* image,
                        int64_t image_bytes, const float* aux, int32_t ld_aux, int32_t row_div, void* stream);
/* The latent self-attention of the cost encoder (encoder.py:156-162) in one launch (csrc/mlp_split3.h, latent_self_attn_split3_kernel):
 *   q | k | v = LayerNorm(a)[M, 128] . w^T + b  (w [384, 128] = the q, k, v rows, b [384] or NULL),  out[M, 128] = softmax(scale q k^T) v per group of
 * 8 consecutive rows (the 8 latents of a cost map) and per head (8 heads of 16 features).  The [M, 384] q | k | v tensor is never written.  The
 * products are st_rowlin128_split3's and the row arithmetic is st_attention_small's (one device function, csrc/attn_small.h): the result equals
 * st_rowlin128_split3 -> st_attention_small(B = M / 8, heads = 8, Nq = Nk = 8, D = 16) bit for bit.  M % 8 == 0; a, out, image 16-byte aligned;
 * lda, ldo >= 128 and multiples of 4; out must not alias a; image_bytes exactly what st_latent_self_attn_split3_image_bytes reports
 * (12 chunk images of 24 KiB in the order q_c, k_c, v_c, c = 0..3, then the 384 bias floats in the same order).  plan4[0] = 12; reported to
 * the observer as M x 384 x 128 with split3 = 1.                                                                                        */
int st_latent_self_attn_split3_image_bytes(int64_t* bytes);
int st_latent_self_attn_split3_pack(const float* w, const float* b, void* image, int64_t image_bytes, void* stream);
int st_latent_self_attn_split3(const float* a, int32_t lda, float* out, int32_t ldo, int32_t M, int32_t ln, float ln_eps, float scale,
                               const void* image, int64_t image_bytes, void* stream);

/* All-pairs correlation volume, MemoryEncoder.corr (encoder.py:359-369):
 *   f1, f2 [B, N, C] channels-last features -> vol [B, N1, N2] = f1 . f2^T (no scaling). */
int st_corr_volume(const float* f1, const float* f2, float* vol, int32_t B, int32_t N1, int32_t N2,
                   int32_t C, void* stream);
/* Both directions at once: vol12 [B, N, N] = f1 . f2^T and vol21 [B, N, N] = f2 . f1^T = vol12^T (bit for bit: products
 * commute, same k order), written by the same launch through a transposed second store (N % 4 == 0, C % 32 == 0, C >= 128;
 * other shapes run as two products).                                                                                  */
int st_corr_volume_both(const float* f1, const float* f2, float* vol12, float* vol21, int32_t B, int32_t N, int32_t C,
                        void* stream);
/* The dispatch decision of st_corr_volume_both, without launching (host only): returns 1 = one product + transposed second store,
 * 0 = two st_corr_volume products (shape / alignment of the LDS-DMA kernel not met, or N * N * 4 >= 2^31: the transposed copy
 * and the row-chunked path exclude each other).  aligned16: all of f1, f2, vol21 are 16-byte aligned.                     */
int st_corr_volume_both_plan(int32_t B, int32_t N, int32_t C, int32_t aligned16);

/* ---- row-wise network ops (channels-last rows) ------------------------------------------------ */
/* nn.LayerNorm over the last dim (encoder.py:58,140-141; twins.py:752-790, eps 1e-5 / 1e-6).        */
int st_layernorm(const float* x, int32_t ldx, const float* w, const float* b, float* out, int32_t ldo,
                 int32_t rows, int32_t C, float eps, void* stream);
/* in-place softmax over rows of length C <= 4096 (gma.py:72 `sim.softmax(dim=-1)`).                */
int st_softmax_rows(float* x, int32_t ld, int32_t rows, int32_t C, void* stream);
/* F.normalize(p=2, dim=C) on NHWC rows (core/UDIS2/Homography/network.py:150-151).                  */
int st_l2norm_rows(const float* x, float* out, int32_t rows, int32_t C, void* stream);
/* nn.MaxPool2d on NHWC (network.py:22,28,34; torchvision resnet maxpool 3/2/1).  torch's limits hold:
 * 0 <= 2 p <= k and H + 2 p >= k, W + 2 p >= k (ST_EINVAL otherwise); out [B, Ho, Wo, C],
 * Ho = floor((H + 2 p - k) / s) + 1.                                                                  */
int st_maxpool_nhwc(const float* x, float* out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k,
                    int32_t s, int32_t p, void* stream);
/* PEG PosConv: depthwise 3x3 + bias + identity (twins.py:793-808); w [9, C].                        */
int st_dwconv3x3_residual(const float* x, const float* w, const float* bias, float* out, int32_t B,
                          int32_t H, int32_t W, int32_t C, void* stream);
/* LinearPositionEmbeddingSine (attention.py:156-161); coords [rows, ldc]=(x,y) or implicit grid
 * (r = row % period; r -> (r % Wg, r / Wg), optionally modulo ws), value*cscale + coff; accumulate: 0 = write,
 * 1 = add to what is there, n > 1 = write columns < n and add to columns >= n.                      */
int st_sine_pe(float* out, int32_t ld, int32_t rows, int32_t dim, const float* coords, int32_t ldc,
               int32_t Wg, int32_t ws, int32_t period, float cscale, float coff, int32_t accumulate,
               void* stream);
/* Multi-head softmax attention, element (b, t, h, e) at base + b*bs + t*ts + h*D + e (floats).
 *   _small : one thread per query, K/V from L2 (attention.py:9-68; 8 latents / 1x8 decoder query)
 *   _kvlds : K/V slab staged in LDS (GSA: twins.py:336-392,633-680); matrix cores for Nk % 16 == 0,
 *            Nk <= 256, otherwise a VALU kernel while 2*Nk*D floats fit in 160 KiB
 * D = 8 (small only), 16 or 32.  Rows move as 16-byte vectors: every base pointer 16-byte aligned and
 * every stride a multiple of 4 floats, else ST_EINVAL (also for _window below and its pad tables). */
int st_attention_small(const float* q, int64_t q_bs, int64_t q_ts, const float* k, int64_t k_bs, int64_t k_ts,
                       const float* v, int64_t v_bs, int64_t v_ts, float* out, int64_t o_bs, int64_t o_ts,
                       int32_t B, int32_t heads, int32_t Nq, int32_t Nk, int32_t D, float scale, void* stream);
int st_attention_kvlds(const float* q, int64_t q_bs, int64_t q_ts, const float* k, int64_t k_bs, int64_t k_ts,
                       const float* v, int64_t v_bs, int64_t v_ts, float* out, int64_t o_bs, int64_t o_ts,
                       int32_t B, int32_t heads, int32_t Nq, int32_t Nk, int32_t D, float scale, void* stream);
/* 7x7-window attention (LSA: twins.py:253-304,587-631); q/k/v pad tables [ws*ws, heads*D] hold the
 * projections of a zero-padded token at each window position.                                      */
int st_window_attention(const float* q, const float* k, const float* v, int64_t bs, int64_t ts,
                        const float* qpad, const float* kpad, const float* vpad, float* out, int64_t o_bs,
                        int64_t o_ts, int32_t B, int32_t H, int32_t W, int32_t heads, int32_t D, int32_t ws,
                        float scale, void* stream);
/* CCL: 3x3 patch correlation + softmax(10 x) + soft-argmax (network.py:147-199) from the all-pairs
 * product G [B, P, P] of the normalised features; out [B, P, ldo] = (flow_w, flow_h, 0...).         */
int st_ccl_softargmax(const float* G, float* out, int32_t ldo, int32_t B, int32_t h, int32_t w, void* stream);
/* PatchEmbed's first conv, Conv2d(1,16,k6,s2,p2)+ReLU on single-channel cost maps (encoder.py:36-37);
 * maps [M,H,W], w [36,16] (tap-major), out [M*Ho*Wo,16]; reads beyond H/W are zero (right/bottom pad). */
int st_patch_conv1(const float* maps, const float* w36x16, const float* bias, float* out, int32_t M, int32_t H,
                   int32_t W, int32_t Ho, int32_t Wo, void* stream);
/* PatchEmbed.proj[0..3] per cost map in ONE launch (encoder.py:36-39,68-72: Conv2d(1,16,6,2,2) + ReLU -> Conv2d(16,32,6,2,2) + ReLU):
 * cost_maps [M, 64*64] -> s2 rows [M*16*16, 32] (channels last), the first feature map never leaving the CU; bit-identical to
 * st_patch_conv1 followed by the (6x3 pixel-pair) st_conv_gemm of st_patch_embed.  H = W = 64 only (ST_EINVAL otherwise: callers take
 * the unfused launches).                                                                              */
int st_patch_conv12(const float* cost_maps, const float* c0_w36x16, const float* c0_b, const float* c2_w32x576,
                    const float* c2_b, float* s2, int32_t M, int32_t H, int32_t W, void* stream);
/* st_patch_conv12 whose result leaves as three blocked bf16 planes [1 chunk][M*256 rows][32] (s2_pstride elements apart) instead of fp32 rows:
 * the operand of the split3 form of PatchEmbed's third convolution (st_patch_embed_split3).  encoder.py:60-75.                    */
int st_patch_conv12_planes(const float* cost_maps, const float* c0_w36x16, const float* c0_b, const float* c2_w32x576, const float* c2_b,
                           void* s2_planes, int64_t s2_pstride, int32_t M, int32_t H, int32_t W, void* stream);
int st_copy2d(const float* src, int32_t lds, float* dst, int32_t ldd, int32_t rows, int32_t cols, void* stream);
/* NCHW image -> channels-last rows with v = mul*(x/div) - sub (flowHomoAdpater.py:55-56,
 * transformer.py:53-54); channels C..ldo-1 are zero.                                               */
int st_prep_image(const float* src, float* dst, int32_t B, int32_t C, int32_t H, int32_t W, int32_t ldo,
                  float mul, float div, float sub, void* stream);

/* Latent cross-attention with the k / v projections folded out (crossattentionlayer.py:37-56, attention.py:9-68; the 8
 * latent queries do not depend on the pixel): per pixel, softmax over its P tokens of the 64 (latent, head) score rows
 * and the pooling z = softmax(S)^T . T.  scores [pixels*P, ld_s>=64] (col = latent*8 + head), tokens [pixels*P, ld_t>=128],
 * z [pixels*64, 128].  P even, <= 64.                                                                        */
int st_latent_pool(const float* scores, int32_t ld_s, const float* tokens, int32_t ld_t, float* z, int32_t pixels,
                   int32_t P, void* stream);

/* ---- FlowFormer decoder gathers --------------------------------------------------------------- */
/* Argument rule of this group and of the geometric and metric groups below: every size (B, H, W, C, planes, Nq, n, h, w) must be
 * positive and every row stride must cover the columns written, else ST_EINVAL and nothing is launched; the further preconditions of
 * an entry stand next to its prototype. */
int st_coords_grid(float* out, int32_t B, int32_t H, int32_t W, void* stream);          /* decoder.py:22-29; B, H, W >= 1 */
/* Warm start (decoder.py:270-272): out rows [B*H*W, 2] = float(grid) + init, init NCHW [B,2,H,W] in low-resolution pixels.     */
int st_coords_grid_init(float* out, const float* init, int32_t B, int32_t H, int32_t W, void* stream);
/* Forward splat of a low-resolution flow, the next frame's flow_init (core/utils/utils.py:32-60 on the device, no host read-back).
 * src: the flow NCHW [B,2,H,W] (src_is_coords_rows = 0) or the decoder's coords1 rows [B*H*W, 2], from which the pixel grid is
 * subtracted (1); out NCHW [B,2,H,W], not aliasing src.  Source (i, j) lands at (j + dx, i + dy) in fp64 and is valid iff
 * 0 < px < W and 0 < py < H (a NaN is invalid); every pixel takes the flow of the valid source that landed nearest to it (fp64
 * squared distance; equal distances: the lowest source index, row-major); no valid source in a batch element: zeros.
 * H*W <= 65536, B <= 65535.                                                                                         */
int st_flow_forward_interpolate(const float* src, int32_t src_is_coords_rows, float* out, int32_t B, int32_t H, int32_t W,
                                void* stream);
/* flow = coords1 - grid (decoder.py:321) into flow4 [B*H*W, ld4] (columns 0..1, zeros up to ld4) and / or columns 0..1 of dst2 rows of
 * stride ld2; either may be NULL.  B, H, W >= 1; ld4 >= 2 where flow4 is given, ld2 >= 2 where dst2 is given.                  */
int st_flow_from_coords(const float* coords1, float* flow4, int32_t ld4, float* dst2, int32_t ld2, int32_t B,
                        int32_t H, int32_t W, void* stream);
/* BasicMotionEncoder flow branch, first layer, fused with the flow computation (gru.py:251, decoder.py:321):
 * out [B*H*W, ldo] (first Co columns) = relu(Conv2d(2, Co, 7, padding=3)(coords1 - coords0)); w98 [49 taps][2][Co]
 * (tap-major: w98[(ky*7+kx)*2 + c][co] = weight[co][c][ky][kx]); flow2 (optional) receives the flow itself in
 * columns 0..1 of rows of stride ld2 (gru.py:254 cat([out, flow])).  B, H, W >= 1; Co >= 4, Co % 4 == 0; ldo >= Co; ld2 >= 2 where
 * flow2 is given; w98 16-byte and coords1 8-byte aligned (its rows are read as float2).                             */
int st_flow_encode(const float* coords1, const float* w98, const float* bias, float* out, int32_t ldo, float* flow2,
                   int32_t ld2, int32_t B, int32_t H, int32_t W, int32_t Co, void* stream);                             /* decoder.py:321   */
/* The same, ALSO leaving both results as blocked bf16 planes (st_gemm_desc.split3 operand format, planes `*_pstride` elements apart,
 * `*_prows` rows per 32-channel chunk): out_planes [3][Co/32][out_prows][32]; channels flow_col, flow_col + 1 (flow_col even) of flow_planes
 * (may be NULL).  Co % 32 == 0, otherwise st_flow_encode's preconditions.  Replaces gru.py:251,254 for a split3 consumer of gru.py:252-253 / 44-59. */
int st_flow_encode_split3(const float* coords1, const float* w98, const float* bias, float* out, int32_t ldo, float* flow2,
                          int32_t ld2, int32_t B, int32_t H, int32_t W, int32_t Co, void* out_planes, int64_t out_pstride,
                          int64_t out_prows, void* flow_planes, int64_t flow_pstride, int64_t flow_prows, int32_t flow_col,
                          void* stream);
/* encode_flow_token + bilinear_sampler (decoder.py:242-260, core/utils/utils.py:62-76): maps [Nq, H2*W2], coords [Nq, 2], out [Nq, ldo],
 * channel i*(2r+1)+j sampled at (x + i - r, y + j - r).  Nq >= 1; 0 <= r <= 64; ldo >= (2r+1)^2; H2, W2 >= 2 (the sampler divides by
 * W2 - 1 and H2 - 1, as the reference's does); H2*W2 < 2^31.                                          */
int st_cost_lookup(const float* maps, const float* coords, float* out, int32_t ldo, int32_t Nq, int32_t H2,
                   int32_t W2, int32_t r, void* stream);
/* One fused launch for the row-local token chain of a refinement iteration: flow_token_encoder
 * (decoder.py:148-152,305) + decoder CrossAttentionLayer (decoder.py:62-109: LN, sine PE of coords1, q, 8-head
 * attention over the pixel's ntok<=8 memory tokens kv [rows*ntok,128]=(k|v), proj + short-cut, FFN).
 * corr [rows, ld>=148]: reads cols 0..83 (cost_forward, 81 + 3 zero), writes cols 84..147 (cost_global).
 * weights16 (host array of 16 device pointers): w0[64,84] b0 w2[64,64] b2 n1w n1b wq bq wp bp n2w n2b wf0 bf0 wf3 bf3. */
int st_decoder_token_chain(float* corr, int32_t ld_corr, const float* coords1, const float* kv,
                           const float* const* weights16, int32_t rows, int32_t ntok, void* stream);
/* upsample_flow (decoder.py:214-225): mask [B*H*W, ldm>=576] -> out NCHW [B,2,8H,8W].  B, H, W >= 1; coords1 8-byte aligned. */
int st_convex_upsample(const float* coords1, const float* mask, int32_t ldm, float* out, int32_t B, int32_t H,
                       int32_t W, void* stream);

/* ---- geometric stage (NCHW images; bit-exact integer sample indices) --------------------------- */
/* tensor_DLT (core/udis_utils/torch_DLT.py:17-45): src [4,2] shared corners, dst = src +
 * motion[B,4,2]*(mscale_x, mscale_y), both divided by `div` -> H [B,3,3].                           */
int st_dlt4(const float* src4x2, const float* motion, float* H, int32_t B, float mscale_x, float mscale_y,
            float div, void* stream);
/* out[b] = L @ (invert ? X[b]^-1 : X[b]) @ R (flowHomoAdpater.py:108,112,226,307).  invert == 1: torch.inverse
 * of a contiguous X; invert == 2: torch.inverse of a column-major X (another torch.inverse's result, warp_utils.py:24). */
int st_mat3_sandwich(const float* L, const float* X, const float* R, float* out, int32_t B, int32_t invert,
                     void* stream);
/* torch_homo_transform.transformer (core/udis_utils/torch_homo_transform.py:5-151); the last n_ones
 * output channels are the warp of an all-ones image; idx (optional) [B,oh,ow,4] = x0,x1,y0,y1.
 * B, H, W, oh, ow >= 1; C, n_ones >= 0 and, where out is given, C + n_ones >= 1; out or idx given.  */
int st_homo_warp(const float* U, const float* theta, float* out, int32_t* idx, int32_t B, int32_t C,
                 int32_t n_ones, int32_t H, int32_t W, int32_t oh, int32_t ow, void* stream);
/* get_rigid_mesh + H2Mesh + min/max (core/warp_utils.py:10-34, flowHomoAdpater.py:254-266).  B >= 1; gw, gh >= 0. */
int st_mesh_bounds(const float* H, float* out4, int32_t B, float width, float height, int32_t gw, int32_t gh,
                   void* stream);
/* warp() = grid_sample(bilinear, zeros, align_corners=True) at pix+flow (core/warp_utils.py:54-80); a sample whose coordinate is not
 * finite is 0.  mul (optional) [B,1,H,W].  B, C, H, W >= 1.                                         */
int st_flow_warp(const float* x, const float* flow, const float* mul, float* out, int32_t B, int32_t C,
                 int32_t H, int32_t W, void* stream);
/* use_combine_h_flow branch of train_eval_foward (flowHomoAdpater.py:150-164): Hi = inverse(H8) (optional output [B,3,3]), mesh of
 * the per-pixel rigid grid through inverse(Hi) (warp_utils.py:10-34), final_flow = mesh - grid + flow, out6 = warp(cat(image2,
 * ones), final_flow) [B,6,H,W], overlap = mean(out6[:,3:6]) < 0.9 [B,H,W].  image2 [B,3,H,W], H8 [B,3,3], flow [B,2,H,W].  B, H, W >= 1. */
int st_homo_flow_warp(const float* image2, const float* H8, const float* flow, float* out6, float* overlap, float* Hi,
                      int32_t B, int32_t H, int32_t W, void* stream);
/* F.interpolate bilinear: resize_flow (warp_utils.py:38-46) / Resize((512,512)) (flowHomoAdpater.py:14);
 * align_corners == 2: scale_factor form of out.py:281 (half-pixel centres, source step (div0, div1) = 1/scale).
 * ndiv == 2 (align_corners 0 / 1): plane p is divided by (p % 2 ? div1 : div0) afterwards.  planes, H, W, oh, ow >= 1; align_corners in
 * {0, 1, 2}; ndiv in {0, 2}, the divisors non-zero when ndiv == 2; align_corners == 2: div0, div1 > 0 and the last output row / column
 * starts inside the source, div0 * (oh - 0.5) - 0.5 < H and div1 * (ow - 0.5) - 0.5 < W (i.e. oh <= H * scale: the lower tap index (int)sy is not clamped). */
int st_resize_bilinear(const float* x, float* out, int32_t planes, int32_t H, int32_t W, int32_t oh, int32_t ow,
                       int32_t align_corners, float div0, float div1, int32_t ndiv, void* stream);
/* compute_range_map (core/warp_utils.py:114-175), deterministic fixed-point splat; scratch: B*H*W uint64.  B, H, W >= 1. */
int st_range_map(const float* flow, void* scratch_u64, float* out, int32_t B, int32_t H, int32_t W, void* stream);
/* 1 - (1 - clamp(range, 0, 1)), thresholded at >= 0.5 when threshold != 0 (warp_utils.py:212-220, flowHomoAdpater.py:181).  n >= 1. */
int st_occlusion_from_range(const float* range, float* out, int64_t n, int32_t threshold, void* stream);
/* preprocess_occlusion_mask (flowHomoAdpater.py:18-35); scratch: 2*N*H*W bytes.  N, H, W >= 1; ksz >= 1 and odd. */
int st_morph_open(const float* mask, float* out, void* scratch_u8x2, int32_t N, int32_t H, int32_t W,
                  int32_t ksz, void* stream);
/* flowHomoAdpater.py:171-183: overlap = mean(final6[:,3:6]) < 0.9, final6 *= occ in place.  B, H, W >= 1. */
int st_eval_finish(float* final6, const float* occ, float* overlap, int32_t B, int32_t H, int32_t W, void* stream);
int st_blend(const float* homo1, const float* homo2, float* fin, const float* occ, float* output2, float* mask1,
             float* mask2, uint8_t* blend, int32_t h, int32_t w, void* stream);          /* :339-360; h, w >= 1 */
/* test_out without the consistency mask (flowHomoAdpater.py:349-360): st_blend's outputs, fin read only, no occlusion and no
 * non_overlap_mask factor.  h, w >= 1. */
int st_blend_plain(const float* homo1, const float* homo2, const float* fin, float* output2, float* mask1, float* mask2,
                   uint8_t* blend, int32_t h, int32_t w, void* stream);
int st_mean_threshold(const float* x, float* out, int32_t B, int32_t C, int32_t H, int32_t W, float thr,
                      void* stream);                                                      /* :233-234; B, C, H, W >= 1 */
/* UDIS2 TPS transformer (core/udis_utils/torch_tps_transform.py:7-190): fp64 solve -> T [B,2,N+3],
 * then grid + 4-tap gather.  work_f64: B*(N+3)*(N+5) doubles.  B >= 1, 1 <= N <= 4000; with out or idx: H, W, oh, ow >= 1, and with
 * out: U given and C >= 1 (checked before the solve is launched).                                    */
int st_tps_solve_grid(const float* U, const float* source, const float* target, void* work_f64, float* T,
                      float* out, int32_t* idx, int32_t B, int32_t C, int32_t H, int32_t W, int32_t N,
                      int32_t oh, int32_t ow, void* stream);

/* ---- evaluation metric ------------------------------------------------------- */
/* Masked PSNR / SSIM per image exactly as evaluate.py:53-65 feeds skimage 0.19.3 (uint8 truncation, mask =
 * uint8(channel-mean mask), 7x7 uniform SSIM, K1=.01 K2=.03, sample covariance, 3-px crop, channel mean).
 * image1 [B,3,H,W]; warped: B images of 3 planes, batch stride in floats (e.g. 6*H*W for final_warp_output);
 * maskmean [B,H,W]; partial_f64: 2*B*ceil(3HW/256) doubles of scratch; out [B,2] fp64 = (psnr, ssim).  B >= 1; H, W >= 7 (one
 * SSIM window); 0 <= warped_batch_stride < 2^31. */
int st_masked_psnr_ssim(const float* image1, const float* warped, int64_t warped_batch_stride, const float* maskmean,
                        void* partial_f64, double* out_psnr_ssim, int32_t B, int32_t H, int32_t W, void* stream);
/* mean over C planes of x[b] (evaluate.py:45).  B, C, H, W >= 1. */
int st_channel_mean(const float* x, int64_t batch_stride, float* out, int32_t B, int32_t C, int32_t H, int32_t W,
                    void* stream);

/* Loader tail of the harnesses (core/datasets.py:383-386 `torch.from_numpy(img).permute(2,0,1).float()`, out.py:137-143):
 * interleaved uint8 [B,H,W,3] -> planar float32 [B,3,H,W] (exact).  H*W must be a multiple of 4, src 4-byte and dst 16-byte
 * aligned (ST_EINVAL otherwise). */
int st_load_rgb8(const void* src_u8_hwc, float* dst_chw, int32_t B, int32_t H, int32_t W, void* stream);

/* Saver tail of out.py (out.py:260-312 `to_pillow_fn(x).save(path)`): the baseline JPEG file Pillow writes at its defaults on libjpeg-turbo
 * (quality 75; RGB: 4:2:0; L: one component; Annex K Huffman tables; JFIF header; integer "islow" DCT), byte for byte, encoded on the device
 * (csrc/jpeg.hip; contract in README.md, CPU restatement tests/_jpeg_ref.py).  src: uint8 [H, W, channels] interleaved, rows row_stride BYTES
 * apart (>= W * channels, < 2^31); channels 3 (RGB) or 1 (L); 1 <= H, W <= 65535 and H * W <= 2^24.  out receives the file (SOI .. EOI),
 * *out_nbytes (device int32) its length; nothing is read back, all launches go to `stream`.  ST_EINVAL before any launch for: a null pointer,
 * other channels, sizes outside those limits, a row_stride below W * channels, a workspace that is not 16-byte aligned or smaller than
 * st_jpeg_workspace_bytes, an out_capacity below st_jpeg_max_bytes -- the worst case of the code tables: header (623 bytes RGB, 328 L) +
 * 2 * ceil(nblocks * (20 + 63 * 26) / 8) + 2, i.e. <= 20 bits of DC and <= 16 + 10 bits per AC coefficient in every block, doubled for byte
 * stuffing, + EOI; nblocks = 6 * ceil(W / 16) * ceil(H / 16) (RGB) or ceil(W / 8) * ceil(H / 8) (L).  The workspace needs no
 * initialisation and may be reused by the next call on the same stream.  The two size queries return 0 for a rejected shape.  The three
 * functions are the _ex ones below at {75, 2, 2, 0} (one channel: {75, 1, 1, 0}): one encoder, same sizes, same launches, same bytes.   */
int st_jpeg_workspace_bytes(int32_t H, int32_t W, int32_t channels);
int st_jpeg_max_bytes(int32_t H, int32_t W, int32_t channels);
int st_jpeg_encode_u8(const void* src, int32_t H, int32_t W, int32_t channels, int64_t row_stride, void* out, int64_t out_capacity,
                      int32_t* out_nbytes, void* workspace, int64_t workspace_bytes, void* stream);

/* The same encoder with Pillow's options: the file `Image.save(path, quality=q, subsampling=s, optimize=o)` writes on libjpeg-turbo, byte for
 * byte (csrc/jpeg.hip; contract in README.md, CPU restatement tests/_jpeg_opts_ref.py).  quality 1..100 (libjpeg's scaling, quantisers
 * clamped to 1..255); (hs, vs) the luma sampling factors, chroma is 1 x 1: (1,1) 4:4:4, (2,1) 4:2:2, (2,2) 4:2:0, one channel: (1,1) only;
 * optimize 1: libjpeg's two-pass optimize_coding -- the symbols are counted, the four code tables are made on the device and the DHT segments
 * list only the symbols that occur, so the header's length and the scan's offset are device values; 0: the Annex K tables.  At
 * {75, 2, 2, 0} (one channel: {75, 1, 1, 0}) the file is st_jpeg_encode_u8's.  Everything else is as for st_jpeg_encode_u8: nothing is read
 * back, all launches (8, with optimize 10) go to `stream`, the workspace needs no initialisation -- the histograms are cleared by the call -- and
 * may be reused by the next call on the same stream; a captured call can be replayed on other pixels.
 * Sizes: codes stay <= 16 bits and at most 12 DC / 162 AC symbols exist, so the header is never longer than 623 bytes (328 for one channel)
 * and a block never longer than 20 + 63 * 26 bits (csrc/jpeg.hip: sizes); st_jpeg_max_bytes_ex is that bound for the blocks of the
 * sampling -- 4 * ceil(W / 16) * ceil(H / 8) at 4:2:2, 3 * ceil(W / 8) * ceil(H / 8) at 4:4:4 -- and equals st_jpeg_max_bytes at 4:2:0 and for
 * one channel.  (st_jpeg_max_bytes itself bounds 4:2:2 and 4:4:4 files of real pictures, which stay far below half of it, but not every input.)
 * st_jpeg_workspace_bytes_ex with optimize 0 is the layout of st_jpeg_workspace_bytes -- no table area, nothing of it is read; optimize 1 adds
 * the area of the four code tables, DHT payloads and histograms (9 312 bytes).  (Before the two encoders became one, optimize 0 reserved that
 * area too: the query now returns 9 312 bytes less there.)
 * ST_EINVAL before any launch for everything st_jpeg_encode_u8 rejects (with the _ex sizes), and for: a null params; quality outside 1..100;
 * sampling other than (1,1), (2,1), (2,2); one channel with sampling other than (1,1); optimize other than 0 / 1; a nonzero reserved[1..3];
 * reserved[0] outside 0..65535.
 * Restart intervals (the jpegr_enc_* kernels of csrc/jpeg.hip; contract in README.md "Restart intervals", CPU restatement tests/_jpeg_rst_ref.py): reserved[0] = Ri > 0
 * writes the file of Pillow's `save(restart_marker_blocks=Ri)` (for `restart_marker_rows=r`: Ri = min(r * MCUs per row, 65535), which
 * ops.jpeg_encode computes), byte for byte: the segment FF DD 00 04 Ri directly in front of SOS; in front of MCU k * Ri (k >= 1) the pending
 * bits padded with 1-bits to a byte (a padded FF is stuffed), then FF D0+((k-1)&7) unstuffed, and every DC prediction back at 0; with
 * optimize 1 the histograms count those reset differences.  With n = ceil(MCUs / Ri) intervals st_jpeg_max_bytes_ex grows by 6 + 4 n -- the
 * DRI segment, and per interval the two marker bytes and at most 7 padding bits, counted as one byte and doubled like every byte of the
 * bound for stuffing -- and st_jpeg_workspace_bytes_ex by the stream's share of that and two 16-byte rounded tables of n + 1 words behind the
 * stream (padding per interval, first byte of every interval).  reserved[0] = 0 is the call, the launches and the sizes without the field.
 * The size queries return 0 for what the entry rejects.                                                                                     */
typedef struct st_jpeg_enc_params {
    int32_t quality;                                /* 1..100                                                                                */
    int32_t hs, vs;                                 /* luma sampling factors                                                                 */
    int32_t optimize;                               /* 0: Annex K tables; 1: tables made from the image's symbol counts                      */
    int32_t reserved[4];                            /* [0]: restart interval Ri in MCUs, 0..65535, 0: none (below); [1..3]: 0                */
} st_jpeg_enc_params;
int st_abi_jpeg_enc_params_size(void);
int st_jpeg_workspace_bytes_ex(int32_t H, int32_t W, int32_t channels, const st_jpeg_enc_params* params);
int st_jpeg_max_bytes_ex(int32_t H, int32_t W, int32_t channels, const st_jpeg_enc_params* params);
int st_jpeg_encode_u8_ex(const void* src, int32_t H, int32_t W, int32_t channels, int64_t row_stride, const st_jpeg_enc_params* params, void* out,
                         int64_t out_capacity, int32_t* out_nbytes, void* workspace, int64_t workspace_bytes, void* stream);

/* Loader head of evaluate.py and out.py (`PIL.Image.open(path)` on the worker threads): the uint8 [H, W, C] array Pillow returns for a baseline
 * JPEG file on libjpeg-turbo at its defaults (Huffman baseline, integer "islow" IDCT, fancy upsampling, jdcolor.c's fixed-point YCbCr -> RGB),
 * bit for bit, decoded on the device (csrc/jpeg_dec.hip; contract in README.md, CPU restatement tests/_jpeg_dec_ref.py).  The HOST parses the
 * markers (ops.jpeg_probe) and fills st_jpeg_dec_params; the quantiser and Huffman tables and the scan are read on the device from the file's
 * bytes at the offsets given there.  file_dev: the whole file, nbytes <= 2^28.  out: uint8 [H, W, ncomp] interleaved, rows row_stride BYTES apart
 * (>= W * ncomp, < 2^31).  *status_dev (device int32) receives 0, 1 when the scan ended before the frame's blocks were decoded, 2 when it held
 * more blocks than the frame; with a nonzero status the pixels are unspecified, every access stays in bounds (bit reads inside the scan, coefficient
 * writes inside the frame's blocks).  Nothing is read back, all launches go to `stream`: 9 + one per 256 subsequences of 1024 scan bits.
 * ST_EINVAL before any launch for: a null pointer; 1 <= H, W <= 65535 and H * W <= 2^24 violated; ncomp other than 1 or 3; (hs, vs) -- the luma
 * sampling factors, chroma is 1 x 1 -- other than (1,1), or with three components (2,1), (2,2); a table index outside 0..1; an offset of a used
 * table below 0 or closer to the end of the file than its fixed part (64 quantiser bytes, 16 code counts); a scan outside the file or empty;
 * a row_stride below W * ncomp; a workspace that is not 16-byte aligned or smaller than st_jpeg_dec_workspace_bytes (0 for a rejected shape).
 * The workspace needs no initialisation and may be reused by the next call on the same stream.                                             */
typedef struct st_jpeg_dec_params {
    int32_t H, W, ncomp, hs, vs;
    int32_t tq[3], td[3], ta[3];                    /* component -> quantiser / DC / AC table index (0..1)                                   */
    int32_t q_off[2], dc_off[2], ac_off[2];         /* byte offsets in the file: the 64 zigzag-ordered quantiser bytes of DQT table i; the 16
                                                     * code counts of DHT table i (its values follow); -1: not defined                       */
    int32_t scan_off, scan_len;                     /* the entropy-coded bytes: behind the SOS header, up to (not including) the EOI marker  */
    int32_t restart_interval, reserved;             /* MCUs per restart interval (the file's DRI), 0: none; reserved: 0                      */
} st_jpeg_dec_params;
int st_abi_jpeg_dec_params_size(void);
int st_jpeg_dec_workspace_bytes(int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs, int64_t scan_len);
/* Restart intervals (the jpegr_* kernels of csrc/jpeg_dec.hip; contract in README.md "Restart intervals", CPU restatement tests/_jpeg_rst_ref.py).  With
 * restart_interval Ri in 1..65535 the scan is n = ceil(MCUs / Ri) intervals with the markers FF D0, FF D1, ... FF D7, FF D0, ... between them
 * (ops.jpeg_probe(data, restart=True) checks their count and order on the host; nothing but the file is uploaded).  The device finds the
 * markers, drops them while it unstuffs, and cuts EVERY INTERVAL into its own subsequences of 1024 bits: an interval's first subsequence starts
 * from a known state (its first bit, DC next, DC predictions 0, block i * Ri * blocks per MCU), so the fixpoint of the entropy decoder runs
 * inside an interval only and a file whose intervals are shorter than 1024 bits needs no repair at all.  *status_dev: 0, or the OR over the
 * intervals of 1 (fewer blocks in the interval's bytes than it has) and 2 (more); coefficient writes of an interval stay inside its own
 * blocks, so every other interval still decodes exactly.  restart_interval 0 makes exactly the launches of the table above.  ST_EINVAL before
 * any launch for a restart_interval outside 0..65535, a nonzero reserved, and a workspace smaller than st_jpeg_dec_workspace_bytes_ex -- the
 * workspace for these params (0 for rejected ones; with restart_interval 0 it equals st_jpeg_dec_workspace_bytes): that of the plain decode
 * plus, with n intervals, c = ceil(scan_len / 2048) chunks and s = ceil(8 * scan_len / 1024) + n subsequences rounded up to 256, the 16-byte
 * rounded tables 2 * 4c (counts) + 3 * 4(n + 1) (marker offsets, interval starts, first subsequences) + 4 * 4s + 4(s + 1) (states, blocks)
 * + boundary states and flags as above.  Launches: 12 + one per 256 of those s subsequences.                                             */
int st_jpeg_dec_workspace_bytes_ex(const st_jpeg_dec_params* params);
int st_jpeg_decode_u8(const void* file_dev, int64_t nbytes, const st_jpeg_dec_params* params, void* out, int64_t row_stride, int32_t* status_dev,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* ---- operator-level entry points (one per reference operator; host-side composition of the kernels
 *      above on the caller's stream, caller-provided scratch, no allocation, no state) ------------------ */
/* encode_flow_token with the reference's 9x9 window (decoder.py:242-260).                            */
int st_cost_lookup9x9(const float* maps, const float* coords, float* out, int32_t ldo, int32_t Nq, int32_t H2,
                      int32_t W2, void* stream);
/* warp(x, flow) [* mask] (core/warp_utils.py:54-80, flowHomoAdpater.py:171-172,339-341).             */
int st_grid_sample_blend(const float* x, const float* flow, const float* mul, float* out, int32_t B, int32_t C,
                         int32_t H, int32_t W, void* stream);
/* preprocess_occlusion_mask, 19x19 structuring element (flowHomoAdpater.py:18-35).                   */
int st_morph_open19(const float* mask, float* out, void* scratch_u8x2, int32_t N, int32_t H, int32_t W,
                    void* stream);
/* PatchEmbed.forward (encoder.py:60-95; patch 8, 'single', linear PE): cost maps [M,H,W] -> tokens
 * [M*P,128], P = ceil(H/8)*ceil(W/8).  weights (host array of 11 device pointers): c0_w[36,16] c0_b
 * c2_w[32,576] c2_b c4_w[64,1152] c4_b f0_w[128,ld_f0] (cols 0..63) f2_w[128,128] f2_b ln_w ln_b;
 * pe_bias [P,128] = f0_w[:,64:] . sinePE(pos) + f0_b.  scratch rows: s1 16, s2 32, s3 64, s4 128 wide.
 * 64x64 maps with 16-byte aligned cost_maps and c2_w run the first two convs as st_patch_conv12 (s1 stays
 * on the CU): s1 may then be NULL (ST_EINVAL when the unfused launches would need it). */
int st_patch_embed(const float* cost_maps, const float* const* weights, int32_t ld_f0, const float* pe_bias,
                   float* s1, float* s2, float* s3, float* s4, float* tokens, int32_t M, int32_t H, int32_t W,
                   void* workspace, int64_t workspace_floats, void* stream);
/* st_patch_embed for 64 x 64 maps with Conv2d(32, 64, 6, 2, 2) -- 77 of the operator's 99 GFLOP per pair -- on exact-split operands
 * (st_gemm_desc.split3): s2_planes scratch [3][1][M*256][32] written by the fused c0 + c2 launch, c4_w_planes = st_split3_pack(c4_w [64, 1152]).
 * M <= 16 384 maps per call (2 GiB buffer offsets).  encoder.py:60-95.                                                              */
int st_patch_embed_split3(const float* cost_maps, const float* const* weights, int32_t ld_f0, const float* pe_bias, void* s2_planes,
                          int64_t s2_pstride, const void* c4_w_planes, int64_t c4_w_pstride, float* s3, float* s4, float* tokens, int32_t M,
                          int32_t H, int32_t W, const void* tail_image, int64_t tail_image_bytes, void* workspace, int64_t workspace_floats, void* stream);
/* PatchEmbed's tail (encoder.py:77-95) as one launch on the exact-split contraction (csrc/mlp_split3.h, pe_tail_split3_kernel):
 *   out[R, 128] = LayerNorm_affine( ReLU( x[R, 64] . w1^T + tab[r mod P] ) . w2^T + b2 )
 * w1 = ffn_with_coord.0's first 64 input columns [128, ld1], tab [P, 128] = its position half + bias (st_patch_embed's pe_bias), w2 [128, 128];
 * both weight matrices are packed once into a 144-KiB image that the kernel holds in LDS (st_pe_tail_split3_image_bytes / _pack).  st_patch_embed_split3
 * takes the image as tail_image (NULL = the three separate launches, s4 [M P, 128] scratch required).  plan4[0] = 11, reported as R x 192 x 128.
 * A non-finite value of x stays in its row but does not show in it: the hidden layer of such a row is NaN, the ReLU is v_max_f32, which returns 0
 * for a NaN (as st_conv_gemm's), and the row leaves as LayerNorm_affine(b2).                                                                          */
int st_pe_tail_split3_image_bytes(int64_t* bytes);
int st_pe_tail_split3_pack(const float* w1, int32_t ld1, const float* w2, void* image, int64_t image_bytes, void* stream);
int st_pe_tail_split3(const float* x, const float* tab, int32_t P, const void* image, int64_t image_bytes, const float* b2, const float* gamma,
                      const float* beta, float eps, float* out, int32_t R, void* stream);
/* GMA Attention.forward (gma.py:54-76), 1 head x 128: attn [B,N,N] = softmax(128^-0.5 q k^T),
 * [q|k] = inp . w_qk^T (w_qk [256,128]); qk scratch [B*N,256].                                        */
int st_gma_attention(const float* inp, int32_t ld_inp, const float* w_qk, float* qk, float* attn, int32_t B,
                     int32_t N, void* workspace, int64_t workspace_floats, void* stream);
/* GMA Aggregate.forward (gma.py:102-115): out = mf + gamma * attn @ (mf . w_v^T); vT scratch [B,128,N]. */
int st_gma_aggregate(const float* attn, const float* mf, int32_t ld_mf, const float* w_v, const float* gamma,
                     float* vT, float* out, int32_t ld_out, int32_t B, int32_t N, void* workspace,
                     int64_t workspace_floats, void* stream);
/* SepConvGRU.forward (gru.py:44-59).  hxA rows [h(128) | x(ld-128)], hxB rows of the same stride [r*h scratch | unused]; the constant
 * `inp` channels arrive folded into tab1/tab2 [rows, ld_tab>=384] = conv_inp([z|r|q]) + bias; w_zr* [256,5*ld],
 * w_q* [128,5*ld] with K ordered (tap, channel); zbuf scratch [rows,128].  h is updated in place in hxA.   */
int st_sepconv_gru(float* hxA, float* hxB, int32_t ld, float* zbuf, const float* tab1, const float* tab2,
                   int32_t ld_tab, const float* w_zr1, const float* w_q1, const float* w_zr2, const float* w_q2,
                   int32_t B, int32_t H, int32_t W, void* workspace, int64_t workspace_floats, void* stream);
/* The same two operators on EXACT-SPLIT operands (st_gemm_desc.split3): every contraction operand is three blocked bf16 planes
 * [C/32][prows][32] (`*_pstride` elements apart) that the producing kernels' epilogues wrote, the six partial products run on the bf16
 * matrix cores with fp32 accumulation (error <= the fp32 chain's, tools/split3_probe.py), epilogue operands and results stay fp32.
 * st_gma_aggregate_split3 (gma.py:102-115): attn_planes [3][N/32][B*N][32] = st_split3_pack of attn, once per pass; vT_planes scratch
 * [3][N/32][B*128][32]; the result also goes to columns out_col..out_col+127 of out_planes.
 * st_sepconv_gru_split3 (gru.py:44-59): hxA_planes / hxB_planes image hxA = [h | x] and hxB = [r*h | -] (ld channels, ld % 32 == 0);
 * r*h exists only as planes; the new h goes to hxA (fp32, in place) and to columns 0..127 of hxA_planes; w_* are st_split3_pack
 * images of the fp32 operator's weight matrices.                                                                                   */
/* st_gma_aggregate whose result ALSO leaves as blocked bf16 planes (columns out_col..out_col+127 of out_planes; st_gemm_desc.c_planes): the
 * aggregate reads the whole attention matrix every call and is HBM-bound on either operand format, so it stays on the fp32 kernel while
 * its consumer (st_sepconv_gru_split3) reads planes.  gma.py:102-115.                                                              */
int st_gma_aggregate_planes(const float* attn, const float* mf, int32_t ld_mf, const float* w_v, const float* gamma, float* vT,
                            float* out, int32_t ld_out, void* out_planes, int64_t out_pstride, int64_t out_prows, int32_t out_col, int32_t B,
                            int32_t N, void* workspace, int64_t workspace_floats, void* stream);
int st_gma_aggregate_split3(const void* attn_planes, int64_t attn_pstride, const float* mf, int32_t ld_mf, const float* w_v, const float* gamma,
                            float* vT, void* vT_planes, int64_t vT_pstride, float* out, int32_t ld_out, void* out_planes, int64_t out_pstride,
                            int64_t out_prows, int32_t out_col, int32_t B, int32_t N, void* workspace, int64_t workspace_floats, void* stream);
int st_sepconv_gru_split3(float* hxA, int32_t ld, void* hxA_planes, void* hxB_planes, int64_t pstride, int64_t prows, float* zbuf,
                          const float* tab1, const float* tab2, int32_t ld_tab, const void* w_zr1, const void* w_q1, const void* w_zr2,
                          const void* w_q2, int64_t w_pstride_zr, int64_t w_pstride_q, int32_t B, int32_t H, int32_t W, void* workspace,
                          int64_t workspace_floats, void* stream);

/* ---- UDIS2 composition stage (the convolutions run on st_conv_gemm with dh/dw) ------------ */
/* F.interpolate(mode='nearest') to (oh, ow), channels-last rows, C % 4 == 0 (Composition/network.py:70).   */
int st_resize_nearest_rows(const float* x, int32_t ldx, float* out, int32_t ldo, int32_t B, int32_t H, int32_t W,
                           int32_t C, int32_t oh, int32_t ow, void* stream);
/* out = a - b on [rows, C] row views (network.py:120-124).                                                 */
int st_sub_rows(const float* a, int32_t lda, const float* b, int32_t ldb, float* out, int32_t ldo, int64_t rows,
                int32_t C, void* stream);
/* build_model (network.py:8-22): NCHW [B,3,H,W] images / masks, net_out rows [B*H*W] with stride ld_net.    */
int st_compose_blend(const float* warp1, const float* warp2, const float* mask1, const float* mask2,
                     const float* net_out, int32_t ld_net, float* learned_mask1, float* learned_mask2,
                     float* stitched, int32_t B, int32_t H, int32_t W, void* stream);
/* out.py:284 normalize_fn: clip(0,255)/127.5 - 1.                                                          */
int st_compose_normalize(const float* x, float* out, int64_t n, void* stream);

/* ---- TPS post-pipeline (the core/inference package, in-tree "kornia" back-end, no inpainter) ---------------- */
/* preprocess (tps_pipline.py:213-244): zero-padded k x k mean of flow [B,C,H,W] (row-major window sum / k^2), optional
 * negation (residual_flow_use_forward = False), optional * valid [B,1,H,W].  One plane per grid layer: B*C <= 65535,
 * ST_EINVAL beyond.                                                                                                      */
int st_flow_boxavg(const float* flow, const float* valid, float* out, int32_t B, int32_t C, int32_t H, int32_t W,
                   int32_t k, int32_t negate, void* stream);
/* advanced_uniform_sample_border_points (sample_point_methods.py:70-90): image [C,H,W] -> grad [H,W] =
 * mean_c |Sobel_x| + mean_c |Sobel_y| (zero padding).                                                                    */
int st_sobel_magnitude(const float* img, float* grad, int32_t C, int32_t H, int32_t W, void* stream);
/* sample_point_methods.py:93-113: for every range (x1,y1,x2,y2) the first arg-max of grad over rows [y1-2, y2+2) x
 * cols [x1-2, x2+2) -> flat index y*W + x.                                                                               */
int st_range_argmax(const float* grad, const int32_t* ranges, int32_t* out_flat_idx, int32_t n_ranges, int32_t H,
                    int32_t W, void* stream);
/* get_point_pairs flow lookup (core/inference/utils.py:61-68) / border_points_mask filter (tps_pipline.py:111-128):
 * out[i, p] = planes[p, y_i, x_i] for integer points (x, y); a point outside the H x W image gives 0.  H, W > 0 and
 * n*P < 2^31 - 255 (computed in 64 bits), ST_EINVAL otherwise.                                                           */
int st_gather_points(const float* planes, const int32_t* points_xy, float* out, int32_t n, int32_t P, int32_t H,
                     int32_t W, void* stream);
/* TPS fit f(sites_i) = values_i, f(v) = a0 + [ax ay].v + sum_j w_j U(|v - centers_j|) -> kernel_w [n,2], affine_w [3,2];
 * work_f64: (n+3)*(n+6) doubles.  mode 0 = kornia get_tps_transform(points_src = sites, points_dst = centers = values) as
 * called by warp_by_tps (tps_pipline.py:362-378, kornia_tps.py:47-112): normalised points, U = 0.5 d2 log(d2 + 1e-8);
 * mode 1 = pixel-unit r^2 log r^2 spline with centers = sites (OpenCV ThinPlateSplineShapeTransformer's formulation,
 * opencv_tps.py:8-18).  status (device int32, may be NULL): 0, or 1 when a pivot collapsed to rounding level (coincident or
 * collinear control points: the reference's torch.linalg.solve raises there) -- the weights are then meaningless.
 * The augmented [n+3, n+5] fp64 matrix is kept in LDS while (n+3)*(n+5)*8 <= 150 KiB, i.e. for n <= 134; from n = 135 on
 * it lives in work_f64 (same arithmetic, same result).                                                                   */
int st_tps2_solve(const float* sites, const float* centers, const float* values, void* work_f64, float* kernel_w,
                  float* affine_w, int32_t n, int32_t mode, int32_t* status, void* stream);
/* warp_image_tps (kornia_tps.py:114-176): img [C,H,W] -> out [C,H,W]; centers [n,2]; grid_sample(bilinear, zeros).  mode 0 =
 * kornia (normalised mesh), 1 = pixel-unit spline sampled directly, 3 = 1 on uint8 data as the reference's OpenCV branch sees it
 * (opencv_tps.py + utils.py:10: taps truncated to 0..255 integers, result rounded half-to-even and saturated).  Any other
 * mode, H or W < 2, n < 1 or n > 3800 (16 n bytes of LDS): ST_EINVAL.                                                     */
int st_tps2_warp(const float* img, const float* centers, const float* kernel_w, const float* affine_w, float* out,
                 int32_t C, int32_t H, int32_t W, int32_t n, float kernel_scale, float affine_scale,
                 int32_t align_corners, int32_t mode, void* stream);
/* cv2.erode / cv2.dilate with a k x k rectangle (tps_pipline.py:143-148) = two 1-D passes of this filter (axis 0: x,
 * axis 1: y), window clipped to the image; in != out.  One plane per grid layer: planes <= 65535, ST_EINVAL beyond.      */
int st_minmax_filter(const float* in, float* out, int32_t planes, int32_t H, int32_t W, int32_t k, int32_t is_max,
                     int32_t axis, void* stream);
/* tps_pipline.py:139-141: inv [h,w] = 1 - (mean_c(warped_mask [C,h,w]) >= 0.5).  This entry and the elementwise ones below
 * (st_tps_mix_blend, st_mix_stage_a, st_mix_stage_b, st_mix_mul_mask, st_blend_pair) return ST_EINVAL for h <= 0 or w <= 0. */
int st_tps_mask_inv(const float* warped_mask, float* inv, int32_t C, int32_t h, int32_t w, void* stream);
/* tps_pipline.py:150-176 with inv_clean = dilate(erode(inv)): tps3 *= tmask (in place), tmask [h,w], mix3 = output2 of
 * the flow/TPS mix, mixmask [h,w], blend3 uint8 [3,h,w] = clip((output1*mask1 + mix*mixmask) / (mask1 + mixmask)).      */
int st_tps_mix_blend(float* tps3, const float* inv_clean, const float* final_warp3, const float* output1_3,
                     const float* mask1_3, float* tmask, float* mix3, float* mixmask, uint8_t* blend3, int32_t h,
                     int32_t w, void* stream);

/* ---- mix_fn plug-ins of the post-pipeline (core/inference/mix_methods/all_img1_with_inpaint.py:8-113,
 *      inpaint_all_area.py:8-73; helpers core/inference/utils.py:125-170): everything but the neural inpainter ----------- */
/* F.conv2d(plane, ones(k,k), padding=pad) on the output domain Ho x Wo (even kernels: the reference crops to [:H,:W]),
 * cmp 0: sum, 1: sum == k*k (erosion of dilate_thin_area), 2: sum >= 1 (its dilations).                                    */
int st_box_sum_cmp(const float* in, int32_t H, int32_t W, float* out, int32_t Ho, int32_t Wo, int32_t k, int32_t pad,
                   int32_t cmp, void* stream);
/* plane ops of dilate_thin_area / thresholds: op 0: o0 = clamp(a*b,0,1), o1 = a*(1-o0); 1: o0 = clamp(a+b,0,1), o1 = (o0>=1);
 * 2: o0 = a > thr.                                                                                                         */
int st_mix_plane_op(const float* a, const float* b, float* o0, float* o1, int64_t n, int32_t op, float thr, void* stream);
/* first lines of mix_fn (method 0: all_img1_with_inpaint.py:44-53, 1: inpaint_all_area.py:43-51): tps_final_warp,
 * tps_final_warp_mask (3 planes each) and channel 0 of the inpaint-area mask before dilate_thin_area.                       */
int st_mix_stage_a(const float* final_warp3, const float* occ, const float* mask1_3, const float* tps3, const float* tmask,
                   float* tfw3, float* tfwm3, float* iam0, int32_t h, int32_t w, int32_t method, void* stream);
/* all_img1_with_inpaint.py:58-77: border / image-1 fill -> inpaint_img_by_only_img1 (3 planes), channel 0 of the
 * "inpaint by other" mask before dilate_thin_area.                                                                          */
int st_mix_stage_b(const float* iam, const float* dil, const float* mask1_3, const float* tfw3, const float* output1_3,
                   float* only_img1_3, float* other0, int32_t h, int32_t w, void* stream);
/* out3 = [clip 0..255](img3) * (invert ? 1 - mask : mask); mask NULL = no mask (all_img1_with_inpaint.py:82,85,101).       */
int st_mix_mul_mask(const float* img3, const float* mask, float* out3, int32_t h, int32_t w, int32_t invert, int32_t clip,
                    void* stream);
/* new_blend_image (tps_pipline.py:186-187): clip((output1*mask1 + output2*mask2)/(mask1+mask2), 0, 255) -> uint8.            */
int st_blend_pair(const float* output1_3, const float* mask1_3, const float* output2_3, const float* mask2, int32_t mask2_planes,
                  uint8_t* blend3, int32_t h, int32_t w, void* stream);

/* ---- Telea inpainting (core/inference/mix_methods/utils/cv_inpainter.py: cv2.inpaint(img, mask, 64, INPAINT_TELEA)), restated
 *      ring by ring (d = L1 distance to the known set mask == 0; contract in README.md, CPU restatement tests/_telea_ref.py) ----- */
/* cv_inpainter's preprocessing: img3 [3,h,w] -> img_hwc uint8 [h,w,3] (clamp to 0..255, truncate); mask [mask_planes,h,w]
 * (1 plane = repeated) scaled by 255 and clamped when its max is <= 1.1 (else clamped), truncated, PIL luma ->
 * mask_u8 [h,w] (nonzero = fill).  scratch: one device int32.                                                             */
int st_inpaint_prep(const float* img3, const float* mask, int32_t mask_planes, uint8_t* img_hwc, uint8_t* mask_u8, int32_t* scratch,
                    int32_t h, int32_t w, void* stream);
/* *bytes (HOST int64) = workspace size of st_inpaint_telea_rings / _fill for h x w and radius (1..88).                     */
int st_inpaint_telea_workspace(int32_t h, int32_t w, int32_t radius, int64_t* bytes);
/* d, ring buckets and packed state in `work`; ring_counts [h + w + 1] (device) = number of pixels per ring k (k = 0: known).
 * counts[0] == 0: no known pixel.  The caller reads ring_counts back once and passes it to st_inpaint_telea_fill.            */
int st_inpaint_telea_rings(const uint8_t* img_hwc, const uint8_t* mask_u8, int32_t h, int32_t w, int32_t radius, void* work,
                           int64_t work_bytes, int32_t* ring_counts, void* stream);
/* one launch per ring 1..nrings (ring_counts_host: HOST copy of ring_counts, nrings + 1 entries, each ring nonempty), then
 * out_hwc uint8 [h,w,3]; d_out int32 [h,w] and T_out fp32 [h,w] (ring index and arrival time) may be NULL.                 */
int st_inpaint_telea_fill(const int32_t* ring_counts_host, int32_t nrings, int32_t h, int32_t w, int32_t radius, void* work,
                          int64_t work_bytes, uint8_t* out_hwc, int32_t* d_out, float* T_out, void* stream);

/* ---- tps_method "other" of the post-pipeline (core/inference/tps_methods/other_tps.py, tps_pipline.py:405-421): per-axis
 *      r^2 ln(r + 1e-6) splines in normalised coordinates and cv2.remap INTER_CUBIC in 8U fixed point (contract in README.md,
 *      CPU restatement tests/_other_tps_ref.py) ----------------------------------------------------------------------- */
/* fit of the two splines f(sites_i) = delta_i (sites = c_dst, delta = c_src - c_dst, both [n,2] float32, 3 <= n <= 4096):
 * [[K, P], [P^T, 0]] theta = [delta; 0], K_ij = U(|sites_i - sites_j|), U(r) = r^2 ln(r + 1e-6), P = [1, x, y], in fp64 ->
 * kernel_w [n,2], affine_w [3,2] float32.  work_f64: (n+3)*(n+6) doubles.  status (device int32, required): 0, or 1 when a
 * pivot collapsed to rounding level (coincident or collinear sites).  LDS for n <= 134, work_f64 from n = 135 on, as for
 * st_tps2_solve.                                                                                                          */
int st_tps_other_solve(const float* sites, const float* delta, void* work_f64, float* kernel_w, float* affine_w, int32_t n,
                       int32_t* status, void* stream);
/* remap maps [h,w] float32 of the fitted splines (centers = sites [n,2], 1 <= n <= 4096): on the numpy.linspace(0, 1) float32
 * grid x_j, y_i, dx = a0 + a1 x + a2 y + sum_k U(r_k) w_k in fp64 (index order, w_0 replaced by numpy's float32
 * -np.sum(w_1..w_{n-1}): kernel_w[0] is ignored), mapx = float32((x + dx) * w), mapy = float32((y + dy) * h).              */
int st_tps_other_maps(const float* centers, const float* kernel_w, const float* affine_w, int32_t n, int32_t h, int32_t w,
                      float* mapx, float* mapy, void* stream);
/* cv2.remap(src, mapx, mapy, INTER_CUBIC) with BORDER_CONSTANT 0 on uint8 data: src [planes,src_h,src_w] float32, each value
 * truncated toward zero and clamped to 0..255 on load; maps [h,w]; out [planes,h,w] float32 holding 0..255.  table: the
 * int16 [1024,16] coefficient table of ops.cubic_remap_table() in device memory, 16-byte aligned.  planes 1..64, src sides
 * 1..32760.                                                                                                              */
int st_remap_cubic_u8(const float* src, int32_t planes, int32_t src_h, int32_t src_w, const float* mapx, const float* mapy,
                      int32_t h, int32_t w, const int16_t* table, float* out, void* stream);

/* ---- TransRef inpainter (core/inference/mix_methods/utils/transref_inpainter.py, TransRef/models/*.py; csrc/transref.hip) -------- */
/* softmax(scale Q K^T) V per head, flash style on the fp32 matrix cores: q [Nq, ldq], k [Nk, ldk], v [Nk, ldv], out [Nq, ldo] row-major,
 * head h in columns [h D, (h + 1) D).  D in {32, 64, 80, 128, 160, 256}, heads, Nq, Nk >= 1 (any Nq, Nk: ragged tiles are masked).
 * q and k 16-byte aligned, ldq and ldk multiples of 4 (float4 loads; h D is a multiple of 8 for every admitted D); v and out need
 * 4-byte alignment only and any ldv, ldo; every ld >= heads D.  out must not overlap q, k or v.  Anything else: ST_EINVAL, no launch. */
int st_tr_attention(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, float* out, int64_t ldo,
                    int32_t heads, int32_t Nq, int32_t Nk, int32_t D, float scale, void* stream);
/* mmcv DeformConv2d 3x3 / pad 1 / one deformable group, sampling part: x channels-last [H W, ldx], off [H W, ldoff] (channel 2k = dy,
 * 2k + 1 = dx of tap k = 3 ky + kx) -> cols [H W, 9 C] dense ((ky, kx, c) order, for a plain-matrix st_conv_gemm).  H, W, C >= 1,
 * ldx >= C, ldoff >= 18.  The sample point is the fp32 sum (oy - 1 + ky) + dy; outside (-1, H) x (-1, W), any magnitude, it gives 0. */
int st_tr_deform_im2col(const float* x, int64_t ldx, const float* off, int64_t ldoff, float* cols, int32_t H, int32_t W, int32_t C,
                        void* stream);
/* stride-2 transposed convolution, last step: phases [4, H W, C] dense (phase 2 py + px) -> out [(2H)(2W), ldo] (+ res, row stride ldr,
 * one fp32 add; res may be null).  H, W, C >= 1, ldo >= C, ldr >= C when res is given.                                             */
int st_tr_phase_interleave(const float* phases, float* out, int64_t ldo, const float* res, int64_t ldr, int32_t H, int32_t W, int32_t C,
                           void* stream);
/* out = GELU(erf)(depthwise 3x3 pad 1 conv of x + bias): x / out channels-last [H W, ld], w9c [9, C] (tap-major) and bias [C] dense.
 * H, W, C >= 1, ldx >= C, ldo >= C; out must not overlap x.                                                                        */
int st_tr_dwconv3x3_gelu(const float* x, int64_t ldx, const float* w9c, const float* bias, float* out, int64_t ldo, int32_t H, int32_t W,
                         int32_t C, void* stream);
/* out = a + b over [rows, C] row-major views: rows, C >= 1, every ld >= C.  out may be a or b (same view); no other overlap.            */
int st_tr_add(const float* a, int64_t lda, const float* b, int64_t ldb, float* out, int64_t ldo, int64_t rows, int32_t C, void* stream);
/* wrapper, steps 1-2: img3 / ctl3 [3, hw] -> out6 [6, hw] = ((trunc-clamp-u8(x) / 255) - 0.5) / 0.5, each operation rounded to fp32 as
 * torch's CPU does (no contraction); all dense, hw >= 1.                                                                           */
int st_tr_prep(const float* img3, const float* ctl3, float* out6, int64_t hw, void* stream);
/* steps 4-6: rs6 [6, n] (resized out6), mask [n] (resized mask plane 0) -> x6 [n, 6], ref3 [n, 3], detail3 [3, n], all dense, n >= 1.
 * byte = (int)mask & 255 (mask.byte()); where it is nonzero the image channels hold the fill colour; the three mask channels hold
 * 1 - byte as TransRef.set_input builds them (1 / 0 for a 0 / 1 mask, -254 for 255).                                              */
int st_tr_pack(const float* rs6, const float* mask, float* x6, float* ref3, float* detail3, int64_t n, void* stream);
/* step 7: fake3 [3, n] = out3 [n, 3] * mask + detail3 * (1 - mask), one fp32 rounding per operation; mask [mask_planes, n], mask_planes
 * 1 (broadcast) or 3, any other count is ST_EINVAL; all dense, n >= 1.                                                             */
int st_tr_blend(const float* out3, const float* detail3, const float* mask, int32_t mask_planes, float* fake3, int64_t n, void* stream);
/* step 8: uint8 (x * 127.5 + 127.5).round() (halves to even) clamped to 0..255; dense, n >= 1.                                        */
int st_tr_to_u8(const float* x, uint8_t* out, int64_t n, void* stream);

/* ---- multiband_fusion: Laplacian-pyramid seam blend of the two warped images (csrc/multiband.hip; contract in README.md, CPU restatement
 *      tests/_multiband_ref.py; this project's own contract, unpinned against OpenCV's detail::MultiBandBlender) -------------------------- */
/* Non-finite and out-of-range values, for every entry of the blend stage (st_multiband_*, st_exposure_*, st_seam_*): a pixel is read as
 * min(max(trunc(x), 0), 255), which takes NaN -> 0, -Inf -> 0, +Inf -> 255 and truncates any finite value toward zero and clamps it (-0.5
 * and -0.0 -> 0, 255.999 -> 255, +-1e30 -> 255 / 0).  A mask value is set iff > 0.5: NaN, -Inf and 0.5 are unset, +Inf is set.  So a call
 * with a non-finite pixel or mask value gives the bits of the same call with that value replaced by its rule value, and every output is
 * finite everywhere (st_exposure_apply: for finite tables).
 * Aliasing: inputs may overlap each other freely (they are only read).  Whatever else may overlap is said at each entry; everything that
 * is not allowed there is rejected with ST_EINVAL before any launch, each operand taken at its full byte length.                        */
/* exact squared Euclidean distance transform: mask uint8 [H,W], sites = the pixels with mask == 0 and, with border_is_site != 0, the
 * one-pixel ring round the canvas.  D int32 [H,W] = squared distance to the nearest site (INT32_MAX when there is none); index (may be
 * NULL) int32 [H,W] = the lowest row-major index among the canvas sites at that distance, -1 when there is none or only the ring is that
 * near.  D doubles as the scratch of the column pass.  mask, D and index must not overlap one another.  ST_EINVAL before any launch: mask
 * or D null, a side outside 1..4096, an overlap.  Two launches.                                                                       */
int st_edt_sq_u8(const uint8_t* mask, int32_t H, int32_t W, int32_t border_is_site, int32_t* D, int32_t* index, void* stream);
/* bytes of workspace st_multiband_blend needs; 0 for a side outside 1..4096 or levels outside 0..16.                                 */
int st_multiband_workspace_bytes(int32_t H, int32_t W, int32_t levels);
/* img1, img2 float32 [3,H,W] (clamped to 0..255 and truncated on load); mask1, mask2 float32 [H,W] (plane 0 of the mask tensor; set where
 * > 0.5); levels = requested REDUCE steps (0 = hard seam along the distance partition; capped where both sides reach 1); out float32
 * [3,H,W], 0 outside the union of the masks.  9 + 2 x (effective levels) launches on `stream`, nothing else: no synchronisation, no
 * allocation, the workspace needs no initialisation and may be reused by the next call on the same stream.  ST_EINVAL before any
 * launch: a null pointer, a side outside 1..4096, levels outside 0..16, a workspace smaller than st_multiband_workspace_bytes or not
 * 16-byte aligned, a forbidden overlap.  out may be img1 or img2 exactly (only the last launch writes out, and it reads the workspace
 * alone); it must not overlap an image in any other way (a shifted view), a mask, or (st_multiband_blend_seam) side or info.  The
 * workspace (its first st_multiband_workspace_bytes bytes) must not overlap any operand.                                             */
int st_multiband_blend(const float* img1, const float* img2, const float* mask1, const float* mask2, int32_t H, int32_t W, int32_t levels,
                       float* out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- exposure compensation: overlap gains of the two warped images in front of st_multiband_blend (csrc/exposure.hip; contract in
 *      README.md, CPU restatement tests/_exposure_ref.py; this project's own contract, unpinned against OpenCV's detail::GainCompensator /
 *      BlocksGainCompensator).  Operands as st_multiband_blend: img float32 [3,H,W] (clamped to 0..255 and truncated on load), mask float32
 *      [H,W] (set where > 0.5); block in {8, 16, 32, 64}; the tile grid is Th = ceil(H / block) by Tw = ceil(W / block). ------------------- */
/* bytes of workspace st_exposure_compensate needs; 0 for a side outside 1..4096 or a block outside the list.                          */
int st_exposure_workspace_bytes(int32_t H, int32_t W, int32_t block);
/* the first kernel alone: records int32 [Th,Tw,9] = per tile N, S1[R,G,B,Y], S2[R,G,B,Y] over the overlap.  ST_EINVAL before the launch: a
 * null pointer, a side outside 1..4096, a block outside the list.                                                                     */
int st_exposure_stats(const float* img1, const float* img2, const float* mask1, const float* mask2, int32_t H, int32_t W, int32_t block,
                      int32_t* records, void* stream);
/* the last kernel alone on the caller's tables: float32 [sets,2,Th,Tw], sets = 3 with channels != 0 (R, G, B) else 1, (image 1, image 2),
 * any Th, Tw in 1..4096 (indices are clamped to the table).  out = min(floor(p g + 0.5), 255), g = the table interpolated bilinearly at
 * the pixel (tile centres at (t + 0.5) block - 0.5).  out may be its own img (in place).  ST_EINVAL before the launch: a null pointer, a
 * side or table side outside 1..4096, a block outside the list, an out that overlaps anything but its own img exactly -- the other
 * image, the other out, or the tables (the [sets,2,Th,Tw] floats the call reads).                                                     */
int st_exposure_apply(const float* img1, const float* img2, const float* tables, int32_t Th, int32_t Tw, int32_t H, int32_t W, int32_t block,
                      int32_t channels, float* out1, float* out2, void* stream);
/* mode 0 "gain": one pair of gains from the global overlap sums; mode 1 "blocks": a pair per tile with the global pair as prior (tiles with
 * N < min_count keep it), smoothed `smooth` (0..8) times with (0.25, 0.5, 0.25).  channels != 0: R, G, B each get their own gains, else the
 * integer luma's serve all three.  sigma_n, sigma_g: the weights 1 / sigma^2 of the data and the prior term.  out1, out2 float32 [3,H,W],
 * integer-valued, every pixel written; gains_out (may be NULL) float32 [sets,2,Th,Tw] ([sets,2,1,1] in mode 0): the tables the apply step
 * read.  3 (mode 0) or 4 + smooth (mode 1) launches on `stream`, nothing else: no synchronisation, no allocation, the workspace needs no
 * initialisation and may be reused by the next call on the same stream.  ST_EINVAL before any launch: a null pointer (but gains_out), a side
 * outside 1..4096, a block outside the list, a mode outside 0..1, smooth outside 0..8, a negative min_count, a sigma that is not positive and
 * finite (or whose 1 / sigma^2 is not), a workspace smaller than st_exposure_workspace_bytes or not 16-byte aligned, an out that overlaps
 * anything but its own img exactly, a gains_out (the [sets,2,Th,Tw] floats the call writes, [sets,2,1,1] in mode 0) that overlaps an
 * image, a mask, an out or the workspace, a workspace (its first st_exposure_workspace_bytes bytes) that overlaps an image, a mask or an
 * out.                                                                                                                                */
int st_exposure_compensate(const float* img1, const float* img2, const float* mask1, const float* mask2, int32_t H, int32_t W, int32_t mode,
                           int32_t block, int32_t channels, int32_t min_count, int32_t smooth, double sigma_n, double sigma_g, float* out1,
                           float* out2, float* gains_out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- seam_dp: a minimum-difference seam through the overlap, between st_exposure_compensate and the blend (csrc/seam.hip; contract in
 *      README.md, seam_dp; CPU restatement tests/_seam_ref.py; this project's own contract, unpinned against OpenCV's detail::DpSeamFinder /
 *      GraphCutSeamFinder).  Operands as st_multiband_blend.  All integers: p = trunc(clamp(x, 0, 255)), m = mask > 0.5, O = m1 and m2,
 *      E1 / E2 = the exclusive regions.  Cost e int32: in O 1 + sum_c |p1 - p2|, outside m1 or m2 1, in E1 or E2 2^18.  orientation: 0 auto,
 *      1 vertical (lines are rows, one column per row), 2 horizontal (lines are columns); first: 0 auto, 1 or 2 = the image that owns the
 *      low-coordinate side.  Auto, from N_i = |E_i| and the coordinate sums Sx_i, Sy_i: A = Sx1 N2 - Sx2 N1, B = Sy1 N2 - Sy2 N1; vertical iff
 *      |A| >= |B|; first = 1 iff (vertical ? A : B) <= 0.  M(0, k) = e, M(l, k) = e + min over the predecessors k, k - 1, k + 1 inside the
 *      line, in that order with strict <; the path ends at the lowest index among the minima of the last line.  ------------------------- */
/* bytes of workspace st_seam_dp needs; 0 for a side outside 1..4096.                                                                  */
int st_seam_workspace_bytes(int32_t H, int32_t W);
/* the cost plane alone, int32 [H,W] (canvas layout); it must not overlap an image or a mask.  ST_EINVAL before the launch: a null
 * pointer, a side outside 1..4096, such an overlap.                                                                                   */
int st_seam_cost(const float* img1, const float* img2, const float* mask1, const float* mask2, int32_t H, int32_t W, int32_t* cost, void* stream);
/* side_out uint8 [H,W]: 1 iff (position <= s[line]) == (first == 1), for every canvas pixel; all ones when info[0] == 0.  path_out (may be
 * NULL) int32 [max(H,W)]: s[l] for the lines of the decided orientation, -1 behind them.  info_out int32 [4]: valid, orientation (1 / 2),
 * first (1 / 2), path cost; valid = 0 when O is empty, or when an argument is auto and E1 or E2 is empty (orientation, first, the path and
 * its cost are reported all the same).  6 launches on `stream` whose grids depend on H and W alone, nothing else: no synchronisation, no
 * allocation, no atomics; the workspace needs no initialisation and may be reused by the next call on the same stream.  ST_EINVAL before any
 * launch: a null pointer (but path_out), a side outside 1..4096, orientation or first outside 0..2, a workspace smaller than
 * st_seam_workspace_bytes or not 16-byte aligned, an overlap: no output (side_out, path_out, info_out) may overlap an image, a mask,
 * another output or the workspace (its first st_seam_workspace_bytes bytes), and no image or mask may lie in the workspace.            */
int st_seam_dp(const float* img1, const float* img2, const float* mask1, const float* mask2, int32_t H, int32_t W, int32_t orientation,
               int32_t first, uint8_t* side_out, int32_t* path_out, int32_t* info_out, void* workspace, int64_t workspace_bytes, void* stream);
/* st_multiband_blend with the ownership of the overlap taken from a seam: W1 = m1 and (not m2 or side) where info[0] != 0, else the distance
 * rule, decided on the device.  side uint8 [H,W], info int32 [4] as st_seam_dp wrote them (device pointers).  Everything else, the
 * workspace (st_multiband_workspace_bytes) and the rejections as st_multiband_blend; a null side or info is rejected too.             */
int st_multiband_blend_seam(const float* img1, const float* img2, const float* mask1, const float* mask2, int32_t H, int32_t W, int32_t levels,
                            const uint8_t* side, const int32_t* info, float* out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- seam_gc: a minimum cut over the overlap, for the same place as seam_dp (csrc/seam_gc.hip; contract in README.md, seam_gc; CPU
 *      restatement tests/_seam_gc_ref.py over scipy's maximum_flow; this project's own contract, unpinned against OpenCV's
 *      detail::GraphCutSeamFinder).  Operands, pixel and mask rules as st_seam_dp.  Nodes: the pixels of O; every 4-neighbour pair inside O
 *      is joined by an arc in each direction of capacity e(p) + e(q), e = 1 + sum_c |p1 - p2|.  S = O with a 4-neighbour in E1 is the
 *      source, T = O with a 4-neighbour in E2 and not in S the sink.  side = 0 exactly on the overlap pixels that can reach T along residual
 *      arcs under a maximum flow (the smallest sink side among the minimum cuts), 1 everywhere else; all ones without both S and T.
 *      Push-relabel with an exact global relabel per round; no atomics, one writer per word, no kernel loops on data.  The number of rounds
 *      depends on the data, so the caller drives them: begin, then round until the status record says done, then finish.
 *      The status record is int32 [8] at the head of the workspace: pixels with excess and a finite label, relabel still changing, rounds
 *      done, done, source pixels with a finite label, valid (S and T non-empty), push sweeps done, label launches done.            ------- */
/* bytes of workspace the three entries need; 0 for a side outside 1..4096.                                                            */
int st_seam_gc_workspace_bytes(int32_t H, int32_t W);
/* masks, seeds, capacities and the first global relabel: 12 launches on `stream`, nothing else.  The workspace needs no initialisation.
 * ST_EINVAL before any launch: a null pointer, a side outside 1..4096, a workspace smaller than st_seam_gc_workspace_bytes or not 16-byte
 * aligned, an image or a mask that lies in the workspace (its first st_seam_gc_workspace_bytes bytes).                                */
int st_seam_gc_begin(const float* img1, const float* img2, const float* mask1, const float* mask2, int32_t H, int32_t W, void* workspace,
                     int64_t workspace_bytes, void* stream);
/* one round on the workspace of st_seam_gc_begin with the same H and W: the sources saturate their arcs to finite-label neighbours, 32 push /
 * gather-relabel sweeps, then 8 launches of the global relabel (64 label sweeps inside a tile each) and the status record: 73 launches.
 * While a relabel has not reached its fixpoint (status word 1) the sweeps of a round do nothing and the round only continues the relabel;
 * st_seam_gc_relabel is that round without the idle launches: 16 launches of the relabel and the status record, 17 launches.  After done
 * neither changes anything.  Both count as a round in the status record.
 * PRECONDITION (not checked: the state lives in device memory): the workspace holds what st_seam_gc_begin and the rounds since wrote for
 * this H and W, untouched by anyone else.  A positive residual names a neighbour, and the setup gives none across the canvas edge; a
 * workspace that st_seam_gc_begin never initialised may hold one there, and the push and gather kernels of st_seam_gc_round would follow it
 * up to W words outside a label plane.  st_seam_gc_relabel and st_seam_gc_finish form no address from the workspace's contents, but what
 * they compute on such a workspace is undefined.                                                                                     */
int st_seam_gc_round(int32_t H, int32_t W, void* workspace, int64_t workspace_bytes, void* stream);
int st_seam_gc_relabel(int32_t H, int32_t W, void* workspace, int64_t workspace_bytes, void* stream);
/* side_out uint8 [H,W], info_out int32 [4] = (valid, 3, cut >> 31, cut & (2^31 - 1)); when the status record does not say done: valid =
 * 0, cut = 0, side all ones.  2 launches.  ST_EINVAL: as above; side_out and info_out may overlap neither each other nor the workspace.  */
int st_seam_gc_finish(int32_t H, int32_t W, uint8_t* side_out, int32_t* info_out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- inner_crop: the largest hole-free rectangle of the stitch (csrc/crop.hip; contract in README.md, inner_crop; CPU restatement
 *      tests/_crop_ref.py; this project's own contract, pinned against no library).  Masks as st_multiband_blend: float32 [H,W] (plane 0 of
 *      the mask tensor), set where > 0.5 (NaN, -Inf and 0.5 unset, +Inf set); U = m1 or m2, U = m1 with mask2 NULL.  A rectangle (top, left,
 *      h, w), h, w >= 1, is inside when every pixel of it is in U; the result is the inside rectangle with the largest area h w, then the
 *      lowest top, then the lowest left, then the smallest h.  All integers.  ------------------------------------------------------------ */
/* bytes of workspace st_inner_rect needs; 0 for a side outside 1..4096.                                                               */
int st_inner_rect_workspace_bytes(int32_t H, int32_t W);
/* info_out int32 [6]: valid, top, left, height, width, area; all zeros when U is empty.  runs_out (may be NULL) int16 [H,W]: r(y, x) = the
 * number of consecutive pixels of U in column x ending at row y going up (0 outside U), the plane the rectangle is searched in.  3 launches
 * on `stream` whose grids depend on H and W alone, nothing else: no synchronisation, no allocation, no atomics; the workspace needs no
 * initialisation and may be reused by the next call on the same stream.  ST_EINVAL before any launch: a null mask1, info_out or workspace,
 * a side outside 1..4096, a workspace smaller than st_inner_rect_workspace_bytes or not 16-byte aligned, an overlap: neither output
 * (info_out, its 24 bytes; runs_out) may overlap a mask, the other output or the workspace (its first st_inner_rect_workspace_bytes
 * bytes), and no mask may lie in the workspace.  mask1 and mask2 may overlap each other freely (they are only read).                     */
int st_inner_rect(const float* mask1, const float* mask2, int32_t H, int32_t W, int32_t* info_out, int16_t* runs_out, void* workspace,
                  int64_t workspace_bytes, void* stream);

/* ---- patchmatch_inpainter: exemplar hole filling (csrc/patchmatch.hip; contract in README.md, patchmatch_inpainter; CPU restatement
 *      tests/_patchmatch_ref.py; this project's own contract, pinned against no library).  PatchMatch (Barnes et al. 2009) inside a
 *      coarse-to-fine vote / search loop (Wexler et al. 2007): 7x7 patches, sum of absolute differences over R, G, B, a stateless counter
 *      hash for every random draw.  All integers.  img uint8 [H,W,3], mask uint8 [H,W] (nonzero = fill), sides 15..4096.
 *      levels: 0 = auto (a level more while both sides of the next one are >= 32, at most 8), 1..8 = at most that many (cut where the next
 *      level would have a side < 15).  ---------------------------------------------------------------------------------------------------- */
/* the number of levels a call runs on; 0 for a side outside 15..4096 or levels outside 0..8.                                            */
int st_patchmatch_levels(int32_t H, int32_t W, int32_t levels);
/* bytes of workspace st_patchmatch_fill needs (below 2^31 for every accepted shape); 0 where st_patchmatch_levels is 0.                 */
int st_patchmatch_workspace_bytes(int32_t H, int32_t W, int32_t levels);
/* out uint8 [H,W,3]: the image with the hole filled, every known pixel byte for byte; the input itself when the mask is empty or level 0
 * has no source patch.  info_out int32 [4]: valid, start level, level-0 sources, level-0 targets.  nnf_out (may be NULL) int32 [H,W,2]:
 * the level-0 match (y, x) of every target centre after the last sweep, -1 elsewhere; sad_out (may be NULL) int32 [H,W]: its cost, -1
 * elsewhere and everywhere with iters = 0.  iters 0..64 search sweeps per level.  2 + (6 + 2 iters) levels launches on
 * `stream` whose grids depend on H, W, levels and iters alone, nothing else: no synchronisation, no allocation, no atomics; the workspace
 * needs no initialisation and may be reused by the next call on the same stream.  ST_EINVAL before any launch: a null img, mask, out,
 * info_out or workspace, a rejected shape, levels or iters, a workspace smaller than st_patchmatch_workspace_bytes or not 16-byte
 * aligned, an overlap: no output may overlap an input, another output or the workspace (its first st_patchmatch_workspace_bytes bytes),
 * and no input may lie in the workspace.  img and mask may overlap each other freely (they are only read).                              */
int st_patchmatch_fill(const uint8_t* img, const uint8_t* mask, int32_t H, int32_t W, int32_t levels, int32_t iters, int32_t seed, uint8_t* out,
                       int32_t* info_out, int32_t* nnf_out, int32_t* sad_out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- feature_align: a weight-free alignment front end (csrc/features.hip; contract in README.md, feature_align; CPU restatement
 *      tests/_features_ref.py; this project's own contract, pinned against no library).  Harris corners (k = 1/16, 7x7 window, the best 4 per
 *      32x32 cell), upright BRIEF-256 on 5x5 box sums, mutual nearest neighbours under a ratio test, RANSAC homography in fp64.  Images
 *      float32 [B,3,H,W], pixel = trunc(clamp(x, 0, 255)); B 1..64, sides 64..1024.  N = 4 ceil(H/32) ceil(W/32) keypoint slots per image,
 *      slot = 4 cell + rank; keypoints int32 [B,N,2] = (x, y), (-1, -1) in an unused slot; descriptors uint32 [B,N,8].  No call
 *      synchronises, allocates or uses atomics; the launch count and every grid depend on B, H, W and max_hyp alone; no buffer needs
 *      initialisation.  Every entry returns ST_EINVAL before any launch for a null pointer, a rejected shape or parameter, and an output
 *      that overlaps any other operand of the call (inputs may overlap each other freely).  -------------------------------------------- */
/* N; 0 for a side outside 64..1024.                                                                                                     */
int st_feature_slots(int32_t H, int32_t W);
/* the BRIEF pattern into HOST memory, int8 [256,4] = (ax, ay, bx, by) of pair k: bit k = S(p + a) < S(p + b).                             */
int st_feature_brief_pattern(int8_t* out_host);
/* bytes of workspace st_feature_homography needs (below 2^31 for every accepted shape); 0 for a rejected B, H, W or max_hyp.             */
int st_feature_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t max_hyp);
/* the regions of that workspace, byte offsets into HOST memory int64 [10]: box uint16 [2,B,H,W], keypoints int32 [2,B,N,2], descriptors
 * uint32 [2,B,N,8], nn int32 [2,B,N,3], matches int32 [B,N,2], count int32 [B], normalised match coordinates fp64 [B,N,4], scores int32
 * [B,max_hyp], inlier mask uint8 [B,N], total.  After a call they hold that call's intermediate data.                                    */
int st_feature_workspace_layout(int32_t B, int32_t H, int32_t W, int32_t max_hyp, int64_t* offsets_host);
/* kp_out int32 [B,N,2]; box_out uint16 [B,H,W], the 5x5 box sum of the luma (terms outside the image 0).  1 launch.                      */
int st_feature_detect(const float* img, int32_t B, int32_t H, int32_t W, int32_t* kp_out, uint16_t* box_out, void* stream);
/* desc_out uint32 [B,N,8] from the box sums and keypoints of st_feature_detect; all zero for a slot that is not a keypoint.  1 launch.    */
int st_feature_describe(const uint16_t* box, const int32_t* kp, int32_t B, int32_t H, int32_t W, uint32_t* desc_out, void* stream);
/* nn_out int32 [2,B,N,3]: per direction (0: image 1 -> 2, 1: the reverse) and slot (best slot or -1, d1, d2), 257 = no such distance;
 * matches_out int32 [B,N,2] = (slot 1, slot 2) in slot order of image 1, (-1, -1) behind the last; count_out int32 [B].  2 launches.      */
int st_feature_match(const int32_t* kp1, const uint32_t* desc1, const int32_t* kp2, const uint32_t* desc2, int32_t B, int32_t H, int32_t W, int32_t* nn_out,
                     int32_t* matches_out, int32_t* count_out, void* stream);
/* motion_out float32 [B,4,2], H_out float32 [B,3,3], info_out int32 [B,8] = (valid, keypoints 1, keypoints 2, matches, winner k or -1,
 * inliers, 0, 0), mask_out uint8 [B,N]: inlier flag of every list entry.  max_hyp 1..65536, thr finite and > 0, min_inliers >= 0.
 * workspace: at least 32 B N + 4 B max_hyp bytes, 16-byte aligned.  3 launches.                                                          */
int st_feature_ransac(const int32_t* kp1, const int32_t* kp2, const int32_t* matches, const int32_t* count, int32_t B, int32_t H, int32_t W, int32_t max_hyp,
                      double thr, int32_t min_inliers, int32_t seed, float* motion_out, float* H_out, int32_t* info_out, uint8_t* mask_out, void* workspace,
                      int64_t workspace_bytes, void* stream);
/* the four stages on both images inside `workspace` (st_feature_workspace_bytes, 16-byte aligned): 7 launches.                           */
int st_feature_homography(const float* img1, const float* img2, int32_t B, int32_t H, int32_t W, int32_t max_hyp, double thr, int32_t min_inliers,
                          int32_t seed, float* motion_out, float* H_out, int32_t* info_out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- feature_align_ms: the oriented, multi-scale front end beside feature_align (csrc/features_ms.hip; contract in README.md,
 *      feature_align_ms; CPU restatement tests/_features_ms_ref.py; this project's own contract, pinned against no library).  Operands as
 *      feature_align's; levels 1..8 (capped: level l+1 exists iff l+1 < levels and min(4 H_l div 5, 4 W_l div 5) >= 64, and is that size),
 *      oriented 0 / 1.  The slots of all levels are concatenated, level 0 first: N = sum of 4 ceil(H_l/32) ceil(W_l/32); keypoints int32
 *      (x, y) in their level's pixels, one orientation bin 0..31 (uint8) per slot.  A pyramid or box-sum buffer of n planes holds level l's
 *      [n, H_l, W_l] planes behind those of the levels before it.  Same conventions as st_feature_*: no call synchronises, allocates or uses
 *      atomics; the launch count and every grid depend on B, H, W, levels and max_hyp alone; no buffer needs initialisation; ST_EINVAL
 *      before any launch for a null pointer, a rejected shape or parameter, a small or misaligned workspace, and an output that overlaps
 *      any other operand of the call.  --------------------------------------------------------------------------------------------------- */
/* the number of levels L (0 for a rejected H, W or levels); sizes_host (may be null) int32 [8,2] = (H_l, W_l), 0 for l >= L.              */
int st_feature_ms_level_sizes(int32_t H, int32_t W, int32_t levels, int32_t* sizes_host);
/* N over all levels; 0 for a rejected H, W or levels.                                                                                    */
int st_feature_ms_slots(int32_t H, int32_t W, int32_t levels);
/* bytes of workspace st_feature_ms_homography needs (below 2^31 for every accepted shape); 0 for a rejected argument.                    */
int st_feature_ms_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t levels, int32_t max_hyp);
/* the regions of that workspace, byte offsets into HOST memory int64 [13]: pyramids uint8 (2B planes, image 1's first), box sums uint16
 * (2B planes), keypoints int32 [2,B,N,2], bins uint8 [2,B,N], descriptors uint32 [2,B,N,8], nn int32 [2,B,N,3], matches int32 [B,N,2],
 * count int32 [B], level-0 coordinates fp64 [2,B,N,2], normalised match coordinates fp64 [B,N,4], scores int32 [B,max_hyp], inlier mask
 * uint8 [B,N], total.  After a call they hold that call's intermediate data.                                                             */
int st_feature_ms_workspace_layout(int32_t B, int32_t H, int32_t W, int32_t levels, int32_t max_hyp, int64_t* offsets_host);
/* pyr_out uint8, B planes per level: level 0 the luma, level l+1 the centre-aligned x 5/4 bilinear resample of level l.  L launches.      */
int st_feature_ms_pyramid(const float* img, int32_t B, int32_t H, int32_t W, int32_t levels, uint8_t* pyr_out, void* stream);
/* kp_out int32 [B,N,2], bins_out uint8 [B,N] (all 0 with oriented = 0), box_out uint16 (B planes per level): the 5x5 box sum of each level.
 * 1 launch over the cells of all levels.                                                                                                  */
int st_feature_ms_detect(const uint8_t* pyr, int32_t B, int32_t H, int32_t W, int32_t levels, int32_t oriented, int32_t* kp_out, uint8_t* bins_out,
                         uint16_t* box_out, void* stream);
/* desc_out uint32 [B,N,8]: the BRIEF pattern steered by the slot's bin on the box sums of the slot's level; zero for an unused slot.  1 launch. */
int st_feature_ms_describe(const uint16_t* box, const int32_t* kp, const uint8_t* bins, int32_t B, int32_t H, int32_t W, int32_t levels, uint32_t* desc_out,
                           void* stream);
/* st_feature_match over the N slots of all levels.  2 launches.                                                                          */
int st_feature_ms_match(const int32_t* kp1, const uint32_t* desc1, const int32_t* kp2, const uint32_t* desc2, int32_t B, int32_t H, int32_t W, int32_t levels,
                        int32_t* nn_out, int32_t* matches_out, int32_t* count_out, void* stream);
/* st_feature_ransac on level-0 coordinates: xy_out fp64 [2,B,N,2], the level-0 position ((2 x + 1) 5^l) / (2 4^l) - 1/2 of every slot of
 * both images, (-1, -1) for an unused one.  workspace: at least 32 B N + 4 B max_hyp bytes, 16-byte aligned.  3 launches.                  */
int st_feature_ms_ransac(const int32_t* kp1, const int32_t* kp2, const int32_t* matches, const int32_t* count, int32_t B, int32_t H, int32_t W, int32_t levels,
                         int32_t max_hyp, double thr, int32_t min_inliers, int32_t seed, float* motion_out, float* H_out, int32_t* info_out, uint8_t* mask_out,
                         double* xy_out, void* workspace, int64_t workspace_bytes, void* stream);
/* all stages on both images inside `workspace` (st_feature_ms_workspace_bytes, 16-byte aligned): L + 7 launches.                         */
int st_feature_ms_homography(const float* img1, const float* img2, int32_t B, int32_t H, int32_t W, int32_t levels, int32_t oriented, int32_t max_hyp, double thr,
                             int32_t min_inliers, int32_t seed, float* motion_out, float* H_out, int32_t* info_out, void* workspace, int64_t workspace_bytes,
                             void* stream);

/* ---- dense_flow: a weight-free residual flow (csrc/dense_flow.hip; contract in README.md, dense_flow; CPU restatement
 *      tests/_dense_flow_ref.py; this project's own contract, pinned against no library).  Coarse-to-fine, zero-mean Lucas-Kanade on integer
 *      pyramids: V = 16 luma (int16) and a validity mask (uint8) per level, the flow state int32 (Ux, Uy) in 1/256 px of its level.  Images
 *      float32 [B,3,H,W], pixel = trunc(clamp(x, 0, 255)); B 1..64, sides 16..1024.  A mask is float32 with 1 or 3 channels per item
 *      (mask*_channels; channel 0 is read, set iff > 0.5), or a null pointer for all set.  levels 1..8 (capped: level l+1 exists iff
 *      l+1 < levels and min(H_l, W_l) >= 32; it is ceil(H_l/2) x ceil(W_l/2)), iters 1..16, radius 1..7, damping 0..2^24.  No call
 *      synchronises, allocates or uses atomics; the launch count and every grid depend on B, H, W, levels and iters alone; no buffer needs
 *      initialisation.  Every entry returns ST_EINVAL before any launch for a null pointer (other than a mask), a rejected shape or
 *      parameter, a small or misaligned workspace, and an output that overlaps any other operand of the call.                             */
/* *bytes_host = bytes of workspace st_dense_flow needs.                                                                                  */
int st_dense_flow_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t levels, int64_t* bytes_host);
/* the regions of that workspace into HOST memory int64 [28]: [0] the number of levels L; [1+l], [9+l], [17+l] the byte offsets of level
 * l's V int16 [2,B,Hl,Wl], m uint8 [2,B,Hl,Wl] (image 1's planes first) and U int32 [B,2,Hl,Wl] (-1 for l >= L); [25] the flow before the
 * median int32 [B,2,H,W]; [26] the support of an iteration uint8 [B,H,W]; [27] total.  After a call they hold that call's data.            */
int st_dense_flow_workspace_layout(int32_t B, int32_t H, int32_t W, int32_t levels, int64_t* offsets_host);
/* both pyramids into the V and m regions of `workspace` (at least the total above, 16-byte aligned).  L launches.                         */
int st_dense_flow_pyramid(const float* img1, const float* img2, const float* mask1, int32_t mask1_channels, const float* mask2, int32_t mask2_channels,
                          int32_t B, int32_t H, int32_t W, int32_t levels, void* workspace, int64_t workspace_bytes, void* stream);
/* one iteration at one level of H x W (sides 16..1024): v1, v2 int16 [B,H,W], m1, m2 uint8 [B,H,W] (set iff nonzero), u int32 [B,2,H,W]
 * -> u_out int32 [B,2,H,W] (the update, then the 3x3 median), support_out uint8 [B,H,W].  workspace: at least 8 B H W bytes, 16-byte
 * aligned.  2 launches.  u is data: a sample position outside 0..W-2 x 0..H-2 reads nothing and the pixel carries no weight; the result is
 * defined for |u| <= 2^31 - 1 - 256 * 1023 - 256 (256 x + u and u + du stay inside int32).                                              */
int st_dense_flow_iterate(const int16_t* v1, const int16_t* v2, const uint8_t* m1, const uint8_t* m2, const int32_t* u, int32_t B, int32_t H, int32_t W,
                          int32_t radius, int32_t damping, int32_t* u_out, uint8_t* support_out, void* workspace, int64_t workspace_bytes, void* stream);
/* flow_out float32 [B,2,H,W] = (dx, dy) with img1(p) ~ img2(p + flow(p)), exactly U / 256 of level 0; support_out uint8 [B,H,W]: the
 * supported flag of the last iteration at level 0.  2 L + 2 L iters launches.                                                            */
int st_dense_flow(const float* img1, const float* img2, const float* mask1, int32_t mask1_channels, const float* mask2, int32_t mask2_channels, int32_t B,
                  int32_t H, int32_t W, int32_t levels, int32_t iters, int32_t radius, int32_t damping, float* flow_out, uint8_t* support_out, void* workspace,
                  int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
