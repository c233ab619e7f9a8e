// Host side of the exact-split fp32 contraction on the bf16 matrix cores ("split3": every fp32 operand as three bf16 planes, six bf16 MFMA
// products per fp32 product -- the kernels and their story are in gemm_split3.h, the epilogue they share with the fp32 kernels in
// gemm_common.h): the split3 rules on top of the common descriptor checks (check_split3), the tile / split-K / persistent-walk plan as a pure
// function (plan_split3), the launches by a switch on that plan.  Reached from st_conv_gemm / st_conv_gemm_pair / st_gemm_plan (gemm.hip) for
// descriptors with split3 set, and through st_split3_pack and st_corr_volume_split3.
#include "gemm_split3.h"

// KPAR: two consumer groups per workgroup (csrc/gemm_split3.h): 768 threads, same tiles, same ring
template <int WM, int WN, int TM, int TN, int STAGES, bool KPAR = false>
static int launch_split3(const st_gemm_desc& d, hipStream_t s) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const int ntm = (d.M + BM - 1) / BM, ntn = (d.N + BN - 1) / BN;
    const int batch = d.batch > 0 ? d.batch : 1;
    const size_t lds = (size_t)STAGES * 3 * (BM + BN) * 64;
    void (*k)(const st_gemm_desc) = conv_gemm_split3_kernel<WM, WN, TM, TN, STAGES>;
    if constexpr (KPAR) k = conv_gemm_split3_kpar_kernel<WM, WN, TM, TN, STAGES>;
    else if constexpr (TM * TN == 1 && WM == 2 && WN == 2 && STAGES == 3) k = conv_gemm_split3_kernel64<STAGES>;
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, dim3(ntm * ntn, 1, d.split_k > 1 ? d.split_k : batch), dim3(KPAR ? 768 : 512), lds, s, d);
    if (d.split_k > 1) splitk_reduce_launch(d, s);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// tile_cfg 37: up to 512 / batch workgroups walk the 64x64 tiles
static int launch_split3_persist(const st_gemm_desc& d, hipStream_t s) {
    const int batch = d.batch > 0 ? d.batch : 1;
    const long ntl64 = (long)((d.M + 63) / 64) * ((d.N + 63) / 64);
    int G = 512 / batch;
    if (G < 1) G = 1;
    if (G > ntl64) G = (int)ntl64;
    const size_t lds = (size_t)3 * 3 * 128 * 64;
    void (*k)(const st_gemm_desc) = d.c_t ? conv_gemm_split3_persist_kernel<true> : conv_gemm_split3_persist_kernel<false>;
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, dim3(G, 1, batch), dim3(512), lds, s, d);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// The split3 path's own rules on top of desc_common_check, and the extents of its operands (shared by st_conv_gemm and st_conv_gemm_pair)
static int check_split3(const st_gemm_desc& d, gemm_plan& p) {
    if (!desc_common_check(d)) return ST_EINVAL;
    // the operands are planes of whole 32-channel chunks; LayerNorm of the A rows is the fp32 row-streaming kernel's
    if (d.split3 != 1 || d.Cin % 32 || d.a_ln) return ST_EINVAL;
    // transposed second store: the persistent 64x64 kernel only, which reads one A source (plan_split3 refuses a2 on tile 37 as well, and
    // c_planes_ok refuses c_t beside c_planes: both halves are kept as the rule stood)
    if (d.c_t && (d.a2 || d.c_planes)) return ST_EINVAL;
    if (d.a_plane_stride <= 0 || d.w_plane_stride <= 0 || d.a_rows <= 0 || d.w_rows < d.N) return ST_EINVAL;
    if ((((uintptr_t)d.a | (uintptr_t)d.w) & 15) || ((d.a_plane_stride | d.w_plane_stride | d.batch_stride_a | d.batch_stride_w) & 7)) return ST_EINVAL;
    const int64_t nimg = d.M / ((int64_t)d.Ho * d.Wo), in_rows = desc_is_plain_matrix(d) ? d.M : nimg * d.H * d.W;
    if (in_rows > d.a_rows) return ST_EINVAL;
    // batch b reads rows b * batch_stride / 32 onwards of every chunk (the kernels shift the base, not the buffer extents): the last batch's
    // planes must end inside the caller's
    if (d.batch > 1 && (d.batch_stride_a < 0 || d.batch_stride_w < 0 || (d.batch_stride_a & 31) || (d.batch_stride_w & 31) ||
                        (int64_t)(d.batch - 1) * (d.batch_stride_a / 32) + in_rows > d.a_rows ||
                        (int64_t)(d.batch - 1) * (d.batch_stride_w / 32) + d.N > d.w_rows))
        return ST_EINVAL;
    // extents (bytes) from the plane-0 base to the end of plane 2; the 32-bit buffer offsets and the out-of-range sentinel need < 2 GiB
    const int64_t ab = 2 * (2 * d.a_plane_stride + (int64_t)(d.Cin / 32) * d.a_rows * 32);
    const int64_t wb = 2 * (2 * d.w_plane_stride + (int64_t)(d.K / 32) * d.w_rows * 32);
    if (ab >= (int64_t)ST_OOB || wb >= (int64_t)ST_OOB || !desc_epi_reach_ok(d)) return ST_EINVAL;      // (no row chunking on this path)
    p = gemm_plan{8, 0, 0, 0, false, false, (uint32_t)ab, (uint32_t)wb};
    return ST_OK;
}

// What a descriptor that passed check_split3 launches (family 8): tile, split-K, persistent walk.  No HIP call, no global.  Every threshold is a
// measured choice; tests/test_gemm_plan_cpu.py pins both sides of each at the workload's shapes.
static int plan_split3(const st_gemm_desc& d, gemm_plan& p) {
    const int batch = d.batch > 0 ? d.batch : 1;
    int cfg = d.tile_cfg;
    // measured (tools/split3_probe.py, profiles/r6_split3_probe.json): 128x64 tiles on a 4-stage ring win when they still give every CU a
    // workgroup (N = 256 at M = 8 192: 41.8 vs 44.2 us), 64x64 tiles (two workgroups per CU) otherwise; 128x128 never
    if (cfg == 0) cfg = (long)((d.M + 127) / 128) * ((d.N + 63) / 64) * batch >= 256 ? 32 : 34;
    // many short tiles (>= 4 per workgroup slot, K <= 2 048): the persistent 64x64 walk (tile_cfg 37) -- the all-pairs volume, PatchEmbed's third conv
    const long ntl64 = (long)((d.M + 63) / 64) * ((d.N + 63) / 64);
    if (d.tile_cfg == 0 && !d.a2 && d.split_k <= 1 && d.K <= 2048 && ntl64 * batch >= 2048) cfg = 37;
    if (d.c_t) cfg = 37;
    // two consumer groups per workgroup (csrc/gemm_split3.h KPAR; tile_cfg 39: 64x64 tiles, 38: 128x64) for a launch of exactly one 64x64 tile per CU and
    // a long K -- the N = 128 shapes at M = 8 192 (SepConvGRU's q convolutions, the motion encoder's 126-channel conv).  Measured (tools/split3_probe.py,
    // 8192 x 128 x 1920): 23.9 us against 29.1 for the four-consumer tile and 33.9 + a 7.4 us reducer launch for the split-K-2 form it replaces.  The
    // 128x64 form (tile_cfg 38, never chosen here) is SLOWER than its four-consumer twin on the N = 256 shapes (47.7 against 42.7 us): three waves per
    // SIMD and twelve waves per barrier cost more than the second MFMA issuer returns there.
    if (d.tile_cfg == 0 && cfg == 34 && ntl64 == 256 && batch == 1 && d.split_k <= 1 && d.K >= 1024) cfg = 39;
    static const int bms[10] = {0, 128, 128, 64, 64, 128, 64, 64, 128, 64}, bns[10] = {0, 128, 64, 128, 64, 64, 64, 64, 64, 64};
    if (cfg < 31 || cfg > 39) return ST_EINVAL;
    if (cfg >= 38 && (d.split_k > 1 || batch != 1)) return ST_EINVAL;
    if (cfg == 37 && (d.a2 || d.split_k > 1)) return ST_EINVAL;
    const long tiles = (long)((d.M + bms[cfg - 30] - 1) / bms[cfg - 30]) * ((d.N + bns[cfg - 30] - 1) / bns[cfg - 30]) * batch;
    int split = d.split_k;
    if (cfg >= 37) split = 1;
    if (split == 0) {
        split = 1;
        if (batch == 1 && d.workspace && d.K >= 512 && tiles < 256) split = (int)((256 + tiles - 1) / tiles);
        // exactly one workgroup per CU (N = 128 at M = 8 192) leaves every SIMD with ONE consumer wave -- two K halves give it two
        // (measured: decoder chain 5.36 -> 5.23 ms, tools/decoder_bench.py)
        if (batch == 1 && d.workspace && d.K >= 1024 && tiles == 256 && cfg == 34) split = 2;
        if (split > d.K / 256) split = d.K / 256;
        if (split > 16) split = 16;
        if (split < 1) split = 1;
        while (split > 1 && (int64_t)split * d.M * d.N > d.workspace_floats) --split;
    }
    if (split > 1) {
        if (batch != 1 || !d.workspace || (int64_t)split * d.M * d.N > d.workspace_floats) return ST_EINVAL;
        const int nkt = d.K / 32, per = (nkt + split - 1) / split;
        split = (nkt + per - 1) / per;                     // no empty slice
    }
    p.tile_cfg = cfg; p.split = split; p.persistent = cfg == 37;
    return ST_OK;
}

int conv_gemm_split3_plan(const st_gemm_desc& desc, gemm_plan& p) {
    const int rc = check_split3(desc, p);
    return rc ? rc : plan_split3(desc, p);
}

int conv_gemm_split3_launch(const st_gemm_desc* desc, void* stream) {
    gemm_plan p;
    if (conv_gemm_split3_plan(*desc, p)) return ST_EINVAL;
    st_gemm_desc d = *desc;
    d.a_bytes = p.a_bytes; d.w_bytes = p.w_bytes; d.split_k = p.split;
    st_plan_set(p);
    hipStream_t s = (hipStream_t)stream;
    switch (p.tile_cfg) {
        case 37: return launch_split3_persist(d, s);
        case 38: return launch_split3<2, 2, 2, 1, 4, true>(d, s);
        case 39: return launch_split3<2, 2, 1, 1, 4, true>(d, s);
        case 31: return launch_split3<2, 2, 2, 2, 3>(d, s);
        case 32: return launch_split3<2, 2, 2, 1, 4>(d, s);
        case 33: return launch_split3<2, 2, 1, 2, 4>(d, s);
        case 35: return launch_split3<2, 2, 2, 1, 3>(d, s);
        case 36: return launch_split3<2, 2, 1, 1, 4>(d, s);
        default: return launch_split3<2, 2, 1, 1, 3>(d, s);
    }
}

// fp32 [rows, ldx] (C columns) -> three blocked bf16 planes [C/32][chunk_rows][32], plane_stride elements apart (csrc/gemm_split3.h)
extern "C" int st_split3_pack(const float* x, void* planes, int64_t rows, int32_t C, int64_t ldx, int64_t plane_stride, int64_t chunk_rows,
                              void* stream) {
    if (!x || !planes || rows <= 0 || C <= 0 || C % 32 || ldx < C || (ldx & 3) || chunk_rows < rows || ((uintptr_t)x & 15) ||
        ((uintptr_t)planes & 15) || (plane_stride & 7) || plane_stride < (int64_t)(C / 32) * chunk_rows * 32)
        return ST_EINVAL;
    const long long n = (long long)rows * (C / 8);
    hipLaunchKernelGGL(split3_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (__bf16*)planes, (long long)rows, (int)C,
                       (long long)ldx, (long long)plane_stride, (long long)chunk_rows);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

// st_conv_gemm_pair with split3 members (both must be): 64x64 tiles (tile_cfg 34), no batches, no split-K -- one grid of one tile shape for both
int conv_gemm_split3_pair_plan(const st_gemm_desc& desc0, const st_gemm_desc& desc1, gemm_plan (&p)[2]) {
    if (!desc0.split3 || !desc1.split3) return ST_EINVAL;
    for (int i = 0; i < 2; ++i) {
        const st_gemm_desc& di = i ? desc1 : desc0;
        if (di.batch > 1 || di.split_k > 1 || (di.tile_cfg != 0 && di.tile_cfg != 34)) return ST_EINVAL;
        const int rc = check_split3(di, p[i]);
        if (rc) return rc;
        p[i].tile_cfg = 34; p[i].split = 1; p[i].persistent = 2 + i;
    }
    return ST_OK;
}

// one launch of 8-wave workgroups; plan[3] and the observer's brackets as in the fp32 pair (launch_pair, gemm_common.h)
int conv_gemm_split3_pair_launch(const st_gemm_desc* desc0, const st_gemm_desc* desc1, void* stream) {
    gemm_plan p[2];
    const int rc = conv_gemm_split3_pair_plan(*desc0, *desc1, p);
    if (rc) return rc;
    return launch_pair(conv_gemm_split3_pair_kernel<2, 2, 1, 1, 3>, 512, (size_t)3 * 3 * 128 * 64, desc0, desc1, p, stream);
}

// All-pairs volume(s) from the feature maps' planes (st_gemm_desc.split3; planes [3][C/32][rows][32], sample b = rows b*N ..): vol12[b] = f1[b] . f2[b]^T and,
// when vol21 is given, vol21[b] = its transpose from the same launch (encoder.py:359-369 for both flow directions).
extern "C" int st_corr_volume_split3(const void* f1_planes, const void* f2_planes, int64_t pstride, int64_t prows, float* vol12, float* vol21, int32_t B,
                                     int32_t N, int32_t C, void* stream) {
    if (!f1_planes || !f2_planes || !vol12 || B <= 0 || N <= 0 || C <= 0 || (C & 31) || prows < (int64_t)B * N) return ST_EINVAL;
    Gemm g((const float*)f1_planes, C, (const float*)f2_planes, C, vol12, N, N, N, C);
    g.transposed(vol21, N).batched(B, (int64_t)N * 32, (int64_t)N * 32, (int64_t)N * N);
    g.d.split3 = 1; g.d.a_plane_stride = pstride; g.d.w_plane_stride = pstride; g.d.a_rows = prows; g.d.w_rows = prows;
    g.d.tile_cfg = 37;
    return g.run(stream);
}
