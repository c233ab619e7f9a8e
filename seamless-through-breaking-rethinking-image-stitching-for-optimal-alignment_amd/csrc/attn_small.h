// ---------------------------------------------------------------------------------------------
// The arithmetic of one (query row, head) of the small multi-head attention, written ONCE: attention_small_kernel (csrc/nn.hip, keys / values
// from global memory) and latent_self_attn_split3_kernel (csrc/mlp_split3.h, keys / values from the wave's LDS slab) both call it, so the two
// give the same bits for the same q / k / v values by construction.
//   q      the row's D query values, unscaled
//   kf, vf (j, e) -> float4: elements e .. e + 3 (e a multiple of 4) of key / value row j
//   o      the D outputs
// Order of operations (every step of it is pinned by tests/test_nn_matrix_gpu.py and the seeded end-to-end tests):
//   * scale goes into q first: both passes below then run the SAME fma chain and the row maximum is one of the scores the second pass
//     exponentiates.  With `s * scale` taken after the chain the compiler contracted the second pass to fma(s, scale, -mx) against a maximum of
//     rounded products, so the top key's weight was exp(rounding residual) instead of 1 whenever scale is not a power of two (D = 8, 32): Nk = 1
//     did not return the V row.
//   * two passes over the keys, e ascending inside a score; fmaxf for the maximum; __expf(s - mx); sum += p in key order; fmaf accumulation of
//     v; acc * (1 / sum) at the end.
#pragma once

template <int D, class KF, class VF>
__device__ __forceinline__ void st_attn_small_row(const float (&q)[D], const float scale, const int Nk, KF kf, VF vf, float (&o)[D]) {
    float qr[D], acc[D];
#pragma unroll
    for (int e = 0; e < D; ++e) qr[e] = q[e] * scale;
    float mx = -INFINITY;
    for (int j = 0; j < Nk; ++j) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < D; e += 4) {
            const float4 t = kf(j, e);
            s = fmaf(qr[e], t.x, s); s = fmaf(qr[e + 1], t.y, s); s = fmaf(qr[e + 2], t.z, s); s = fmaf(qr[e + 3], t.w, s);
        }
        mx = fmaxf(mx, s);
    }
#pragma unroll
    for (int e = 0; e < D; ++e) acc[e] = 0.f;
    float sum = 0.f;
    for (int j = 0; j < Nk; ++j) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < D; e += 4) {
            const float4 t = kf(j, e);
            s = fmaf(qr[e], t.x, s); s = fmaf(qr[e + 1], t.y, s); s = fmaf(qr[e + 2], t.z, s); s = fmaf(qr[e + 3], t.w, s);
        }
        const float p = __expf(s - mx);
        sum += p;
#pragma unroll
        for (int e = 0; e < D; e += 4) {
            const float4 t = vf(j, e);
            acc[e] = fmaf(p, t.x, acc[e]); acc[e + 1] = fmaf(p, t.y, acc[e + 1]);
            acc[e + 2] = fmaf(p, t.z, acc[e + 2]); acc[e + 3] = fmaf(p, t.w, acc[e + 3]);
        }
    }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int e = 0; e < D; ++e) o[e] = acc[e] * inv;
}
