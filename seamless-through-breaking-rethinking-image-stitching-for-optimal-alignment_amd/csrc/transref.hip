// TransRef inpainting network (reference: core/inference/mix_methods/utils/transref_inpainter.py, TransRef/models/TransRef.py,
// base_networks.py, RefPA/*.py): the kernels its layers need beyond the implicit-GEMM family of gemm.hip -- flash attention of any
// key count on the fp32 matrix cores, mmcv's DeformConv2d sampling (bilinear im2col), the output-phase interleave of a transposed
// convolution, depthwise 3x3 + bias + GELU, and the wrapper's pre / post steps.  Built without fp contraction (build.py): the
// wrapper steps restate torch-CPU fp32 expressions operation by operation.
#include "common.h"

#include <math.h>

typedef float floatx16 __attribute__((ext_vector_type(16)));

// ---- flash attention -------------------------------------------------------------------------------------------------------
// One wave owns 32 queries of one head and walks the keys 32 at a time.  It forms S^T = K Q^T (v_mfma_f32_32x32x2f32: lane l holds
// S^T[key = (r & 3) + 8 (r >> 2) + 4 (l >> 5)][query = l & 31] in register r), so a query's scores sit in one lane pair (l, l ^ 32):
// the running max needs one cross-half exchange, and the probabilities are already the B operand of O^T += V^T P^T -- the lane
// supplies its own register r for its own key, and V's A operand is read for that key.  Q stays in registers for the whole walk;
// each 8-column group of the QK^T contraction is one 16-byte load per lane (lanes < 32: columns 0..3 of the group, lanes >= 32:
// 4..7).  Keys past Nk score -inf (their rows are clamped to Nk - 1 for the loads, their probability is exactly 0).  The softmax
// is the reference's exp(s * scale - max) with ocml's expf; the row sum keeps one partial per register (rescaled with the outputs,
// summed pairwise at the end) so its rounding chain grows with the number of key tiles only; one IEEE division per output.
template <int D>
__global__ __launch_bounds__(256) void tr_attention_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k, int64_t ldk,
                                                           const float* __restrict__ v, int64_t ldv, float* __restrict__ out, int64_t ldo,
                                                           int Nq, int Nk, float scale) {
    constexpr int NG = D / 8;
    constexpr int NT = (D + 31) / 32;
    const int lane = threadIdx.x & 63, c = lane & 31, hf = lane >> 5;
    const int q0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
    if (q0 >= Nq) return;
    const size_t hoff = (size_t)blockIdx.y * D;
    const int qi = q0 + c;
    float4 qr[NG];
    {
        const float* qp = q + (size_t)min(qi, Nq - 1) * ldq + hoff + 4 * hf;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            qr[g] = *(const float4*)(qp + 8 * g);
            if (qi >= Nq) qr[g] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    floatx16 o[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
    float m = -INFINITY;
    float lp[16];                                    // per-register partial sums of the probabilities: a chain of one term per key tile
#pragma unroll
    for (int r = 0; r < 16; ++r) lp[r] = 0.f;
    const float* kh = k + hoff + 4 * hf;
    const float* vh = v + hoff;
    for (int k0 = 0; k0 < Nk; k0 += 32) {
        floatx16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        const float* kp = kh + (size_t)min(k0 + c, Nk - 1) * ldk;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const float4 kv = *(const float4*)(kp + 8 * g);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.x, qr[g].x, s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.y, qr[g].y, s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.z, qr[g].z, s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.w, qr[g].w, s, 0, 0, 0);
        }
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * hf;
            const float sv = key < Nk ? s[r] * scale : -INFINITY;
            s[r] = sv;
            mx = fmaxf(mx, sv);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m, mx);
        const float alpha = expf(m - mn);            // 0 on the first tile (m = -inf, mn finite: every tile holds a key < Nk)
        m = mn;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = expf(s[r] - mn);
            s[r] = p;
            lp[r] = lp[r] * alpha + p;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[t][r] *= alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = min(k0 + (r & 3) + 8 * (r >> 2) + 4 * hf, Nk - 1);
            const float* vp = vh + (size_t)key * ldv;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int d = 32 * t + c;
                const float vv = (D % 32 == 0 || d < D) ? vp[min(d, D - 1)] : 0.f;
                o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv, s[r], o[t], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int w = 8; w > 0; w >>= 1)                  // pairwise over the 16 registers, then across the lane pair
#pragma unroll
        for (int r = 0; r < w; ++r) lp[r] += lp[r + w];
    const float lsum = lp[0] + __shfl_xor(lp[0], 32, 64);
    if (qi >= Nq) return;
    float* op = out + (size_t)qi * ldo + hoff;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int d = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hf;
            if (D % 32 == 0 || d < D) op[d] = o[t][r] / lsum;
        }
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int st_tr_attention(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, float* out, int64_t ldo,
                               int32_t heads, int32_t Nq, int32_t Nk, int32_t D, float scale, void* stream) {
    if (!q || !k || !v || !out || heads <= 0 || Nq <= 0 || Nk <= 0) return ST_EINVAL;
    if (!al16(q) || !al16(k) || (ldq & 3) || (ldk & 3) || ldq < (int64_t)heads * D || ldk < (int64_t)heads * D || ldv < (int64_t)heads * D ||
        ldo < (int64_t)heads * D)
        return ST_EINVAL;
    dim3 grid((Nq + 127) / 128, heads);
    hipStream_t s = (hipStream_t)stream;
#define TR_ATT(DD)                                                                                                            \
    case DD: hipLaunchKernelGGL(tr_attention_kernel<DD>, grid, dim3(256), 0, s, q, ldq, k, ldk, v, ldv, out, ldo, Nq, Nk, scale); \
        break;
    switch (D) {
        TR_ATT(32) TR_ATT(64) TR_ATT(80) TR_ATT(128) TR_ATT(160) TR_ATT(256)
        default: return ST_EINVAL;
    }
#undef TR_ATT
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// ---- mmcv DeformConv2d (3x3, stride 1, pad 1, dilation 1, one deformable group): bilinear im2col --------------------------------
// cols[p][k * C + c] = x sampled at (oy - 1 + ky + off[p][2k], ox - 1 + kx + off[p][2k + 1]), tap k = 3 ky + kx; mmcv's
// deformable_im2col_bilinear: 0 when h <= -1, h >= H, w <= -1 or w >= W, else bilinear with every outside corner reading 0.
// A plain-matrix st_conv_gemm with the [Cout, 9 Cin] (ky, kx, cin) weight finishes the convolution.
__global__ __launch_bounds__(256) void tr_deform_im2col_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ off,
                                                               int64_t ldoff, float* __restrict__ cols, int H, int W, int C) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)H * W * 9 * C;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const int64_t t = idx / C;
    const int kk = (int)(t % 9);
    const int64_t p = t / 9;
    const int oy = (int)(p / W), ox = (int)(p % W), ky = kk / 3, kx = kk % 3;
    const float h = (float)(oy - 1 + ky) + off[p * ldoff + 2 * kk];
    const float w = (float)(ox - 1 + kx) + off[p * ldoff + 2 * kk + 1];
    float val = 0.f;
    if (h > -1.f && w > -1.f && h < (float)H && w < (float)W) {
        const float hl = floorf(h), wl = floorf(w);
        const int h_low = (int)hl, w_low = (int)wl, h_high = h_low + 1, w_high = w_low + 1;
        const float lh = h - hl, lw = w - wl, hh = 1.f - lh, hw = 1.f - lw;
        const float v1 = (h_low >= 0 && w_low >= 0) ? x[((int64_t)h_low * W + w_low) * ldx + c] : 0.f;
        const float v2 = (h_low >= 0 && w_high <= W - 1) ? x[((int64_t)h_low * W + w_high) * ldx + c] : 0.f;
        const float v3 = (h_high <= H - 1 && w_low >= 0) ? x[((int64_t)h_high * W + w_low) * ldx + c] : 0.f;
        const float v4 = (h_high <= H - 1 && w_high <= W - 1) ? x[((int64_t)h_high * W + w_high) * ldx + c] : 0.f;
        const float w1 = hh * hw, w2 = hh * lw, w3 = lh * hw, w4 = lh * lw;
        val = w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4;
    }
    cols[p * 9 * C + kk * C + c] = val;
}

extern "C" int st_tr_deform_im2col(const float* x, int64_t ldx, const float* off, int64_t ldoff, float* cols, int32_t H, int32_t W, int32_t C,
                                   void* stream) {
    if (!x || !off || !cols || H <= 0 || W <= 0 || C <= 0 || ldx < C || ldoff < 18) return ST_EINVAL;
    const int64_t total = (int64_t)H * W * 9 * C;
    hipLaunchKernelGGL(tr_deform_im2col_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, off, ldoff,
                       cols, H, W, C);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// ---- transposed convolution, stride 2: interleave of the four output phases ---------------------------------------------------
// phases [4][H * W][C] (phase 2 py + px = the stride-1 GEMM of the taps that reach output rows 2a + py, columns 2b + px, bias and
// activation already applied) -> out[(2a + py) * 2W + 2b + px][c] (row stride ldo), plus res (same geometry, row stride ldr) if given.
__global__ __launch_bounds__(256) void tr_phase_interleave_kernel(const float* __restrict__ ph, float* __restrict__ out, int64_t ldo,
                                                                  const float* __restrict__ res, int64_t ldr, int H, int W, int C) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)4 * H * W * C;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const int64_t op = idx / C;
    const int oy = (int)(op / (2 * W)), ox = (int)(op % (2 * W));
    const int phase = 2 * (oy & 1) + (ox & 1);
    float val = ph[(((int64_t)phase * H + (oy >> 1)) * W + (ox >> 1)) * C + c];
    if (res) val = val + res[op * ldr + c];
    out[op * ldo + c] = val;
}

extern "C" int st_tr_phase_interleave(const float* phases, float* out, int64_t ldo, const float* res, int64_t ldr, int32_t H, int32_t W,
                                      int32_t C, void* stream) {
    if (!phases || !out || H <= 0 || W <= 0 || C <= 0 || ldo < C || (res && ldr < C)) return ST_EINVAL;
    const int64_t total = (int64_t)4 * H * W * C;
    hipLaunchKernelGGL(tr_phase_interleave_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, phases, out, ldo,
                       res, ldr, H, W, C);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// ---- depthwise 3x3 (pad 1) + bias + GELU(erf): the Mix-FFN middle of TransRef.py's Mlp (DWConv, then nn.GELU) ----------------------
__global__ __launch_bounds__(256) void tr_dwconv3x3_gelu_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ w9c,
                                                                const float* __restrict__ bias, float* __restrict__ out, int64_t ldo, int H,
                                                                int W, int C) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)H * W * C) return;
    const int c = (int)(idx % C);
    const int64_t p = idx / C;
    const int oy = (int)(p / W), ox = (int)(p % W);
    float acc = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int yy = oy + ky - 1;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int xx = ox + kx - 1;
            if (xx < 0 || xx >= W) continue;
            acc = fmaf(x[((int64_t)yy * W + xx) * ldx + c], w9c[(ky * 3 + kx) * C + c], acc);
        }
    }
    const float v = acc + bias[c];
    out[p * ldo + c] = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
}

extern "C" int st_tr_dwconv3x3_gelu(const float* x, int64_t ldx, const float* w9c, const float* bias, float* out, int64_t ldo, int32_t H,
                                    int32_t W, int32_t C, void* stream) {
    if (!x || !w9c || !bias || !out || H <= 0 || W <= 0 || C <= 0 || ldx < C || ldo < C) return ST_EINVAL;
    const int64_t total = (int64_t)H * W * C;
    hipLaunchKernelGGL(tr_dwconv3x3_gelu_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, w9c, bias,
                       out, ldo, H, W, C);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// ---- elementwise sum of two row-major [rows, C] views (the stage joins x1 = patch_embed(x1) + x2 of EncoderTransformer) ----------
__global__ __launch_bounds__(256) void tr_add_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ b, int64_t ldb,
                                                     float* __restrict__ out, int64_t ldo, int64_t rows, int C) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * C) return;
    const int64_t r = idx / C;
    const int c = (int)(idx % C);
    out[r * ldo + c] = a[r * lda + c] + b[r * ldb + c];
}

extern "C" int st_tr_add(const float* a, int64_t lda, const float* b, int64_t ldb, float* out, int64_t ldo, int64_t rows, int32_t C,
                         void* stream) {
    if (!a || !b || !out || rows <= 0 || C <= 0 || lda < C || ldb < C || ldo < C) return ST_EINVAL;
    hipLaunchKernelGGL(tr_add_kernel, dim3((unsigned)((rows * C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, lda, b, ldb, out, ldo,
                       rows, C);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// ---- wrapper steps (transref_inpainter.py:37-70, TransRef.set_input / forward) ---------------------------------------------------
// 1-2: to_pillow_fn (truncate toward zero, clamp 0..255), ToTensor (/ 255), Normalize(0.5, 0.5): planes 0..2 from img, 3..5 from ctl.
__global__ __launch_bounds__(256) void tr_prep_kernel(const float* __restrict__ img, const float* __restrict__ ctl, float* __restrict__ out6,
                                                      int64_t hw) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 6 * hw) return;
    const float v = idx < 3 * hw ? img[idx] : ctl[idx - 3 * hw];
    const float t = st_u8_trunc(v) / 255.0f;
    out6[idx] = (t - 0.5f) / 0.5f;
}

extern "C" int st_tr_prep(const float* img3, const float* ctl3, float* out6, int64_t hw, void* stream) {
    if (!img3 || !ctl3 || !out6 || hw <= 0) return ST_EINVAL;
    hipLaunchKernelGGL(tr_prep_kernel, dim3((unsigned)((6 * hw + 255) / 256)), dim3(256), 0, (hipStream_t)stream, img3, ctl3, out6, hw);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// 4-6: mask_process (mask[0][0].byte(): truncation), the fill colours 2 {123, 104, 117} / 255 - 1 where that byte is nonzero, the
// 6-channel network input cat([input_DE, 1 - byte]) and the reference, channels-last; detail3 = input_DE as planes (the same tensor
// as `detail` in the reference, so the final blend sees the fill).  rs6: the resized planes of st_tr_prep, mask: its resize.
__global__ __launch_bounds__(256) void tr_pack_kernel(const float* __restrict__ rs6, const float* __restrict__ mask, float* __restrict__ x6,
                                                      float* __restrict__ ref3, float* __restrict__ detail3, int64_t n) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int byte = ((int)mask[p]) & 255;
    const bool hole = byte != 0;
    const float fill[3] = {(float)(2.0 * 123.0 / 255.0 - 1.0), (float)(2.0 * 104.0 / 255.0 - 1.0), (float)(2.0 * 117.0 / 255.0 - 1.0)};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float d = hole ? fill[c] : rs6[c * n + p];
        x6[p * 6 + c] = d;
        x6[p * 6 + 3 + c] = 1.f - (float)byte;
        detail3[c * n + p] = d;
        ref3[p * 3 + c] = rs6[(3 + c) * n + p];
    }
}

extern "C" int st_tr_pack(const float* rs6, const float* mask, float* x6, float* ref3, float* detail3, int64_t n, void* stream) {
    if (!rs6 || !mask || !x6 || !ref3 || !detail3 || n <= 0) return ST_EINVAL;
    hipLaunchKernelGGL(tr_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rs6, mask, x6, ref3, detail3, n);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// 7: fake = out * mask + detail * (1 - mask) (out channels-last [n,3]; mask planes [mask_planes, n], one plane = broadcast) -> planes.
__global__ __launch_bounds__(256) void tr_blend_kernel(const float* __restrict__ out3, const float* __restrict__ detail3,
                                                       const float* __restrict__ mask, int mask_planes, float* __restrict__ fake3, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 3 * n) return;
    const int c = (int)(idx / n);
    const int64_t p = idx % n;
    const float m = mask[(mask_planes == 1 ? 0 : c) * n + p];
    const float a = out3[p * 3 + c] * m;
    const float inv = 1.0f - m;
    fake3[idx] = a + detail3[idx] * inv;
}

extern "C" int st_tr_blend(const float* out3, const float* detail3, const float* mask, int32_t mask_planes, float* fake3, int64_t n, void* stream) {
    if (!out3 || !detail3 || !mask || !fake3 || n <= 0 || (mask_planes != 1 && mask_planes != 3)) return ST_EINVAL;
    hipLaunchKernelGGL(tr_blend_kernel, dim3((unsigned)((3 * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out3, detail3, mask,
                       mask_planes, fake3, n);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// 8: (x * 127.5 + 127.5).round() (half to even), clamp(0, 255), uint8.
__global__ __launch_bounds__(256) void tr_to_u8_kernel(const float* __restrict__ x, uint8_t* __restrict__ out, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const float a = x[idx] * 127.5f;
    const float v = rintf(a + 127.5f);
    out[idx] = (uint8_t)fminf(fmaxf(v, 0.f), 255.f);
}

extern "C" int st_tr_to_u8(const float* x, uint8_t* out, int64_t n, void* stream) {
    if (!x || !out || n <= 0) return ST_EINVAL;
    hipLaunchKernelGGL(tr_to_u8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out, n);
    ST_CHECK_LAUNCH();
    return ST_OK;
}
