"""The descriptors that pin the GEMM dispatch table on the CPU (tests/test_gemm_plan_cpu.py, tools/make_gemm_plan_golden.py).

Every case is (name, tags, fields of the descriptor, fields of the pair's second member or None).  The addresses are made up -- 16-byte aligned
unless a case is about alignment -- so a case may be handed to ``st_gemm_plan`` only, which follows no pointer: never to an entry that launches.

Tags say what a case is for: ``plan`` (a reportable plan), ``thr:<threshold>:<side>`` (one side of a measured dispatch threshold at a shape of the
workload: M = 4 096 / 8 192 / 32 768 rows, K = 128 ... 2 304), ``chunk:matrix`` / ``chunk:conv`` (rows run in chunks), ``reject:<function>:<operand>``
(the accepted base case of that path with exactly that operand of that ``return ST_EINVAL`` violated).  The function names are those the rejections
had when the table was first recorded, one copy of the checks per path; their rules now live in desc_common_check / c_planes_ok (csrc/gemm_common.h),
check_f32, for_each_row_chunk and plan_f32 (conv_gemm_launch, launch_rowstream), plan_f32_pair_member (pair_member_prepare), check_split3
(split3_prepare), plan_split3 (conv_gemm_split3_launch) and conv_gemm_split3_pair_plan (conv_gemm_split3_pair_launch)."""
import copy

# made-up device addresses, 1 GiB apart
_B = 0x7F0000000000
PTR = {n: _B + (i << 30) for i, n in enumerate(("a", "w", "c", "bias", "aux0", "aux1", "aux2", "scale_ptr", "workspace", "c2", "a2", "c_t", "c_planes"))}
WS_FLOATS = 16 * 1024 * 1024        # what ops.conv_gemm attaches
ACT = dict(none=0, relu=1, gelu=2, sigmoid=3, tanh=4, lrelu=5)
EPI = dict(store=0, add=1, mul=2, gru=3, axpy=4, zr=5)


def mat(M, N, K, **over):
    """plain matrix C[M, N] = A[M, K] . W[N, K]^T with a workspace, auto tile and auto split"""
    f = dict(a=PTR["a"], w=PTR["w"], c=PTR["c"], M=M, N=N, K=K, H=1, W=M, Cin=K, ldx=K, kh=1, kw=1, sh=1, sw=1, ph=0, pw=0, Ho=1, Wo=M,
             ldw=K, ldc=N, alpha=1.0, batch=1, workspace=PTR["workspace"], workspace_floats=WS_FLOATS)
    f.update(over)
    return f


def conv(B, H, W, Cin, N, kh, kw, sh=1, sw=1, ph=0, pw=0, **over):
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    f = mat(B * Ho * Wo, N, kh * kw * Cin)
    f.update(H=H, W=W, Cin=Cin, ldx=Cin, kh=kh, kw=kw, sh=sh, sw=sw, ph=ph, pw=pw, Ho=Ho, Wo=Wo)
    f.update(over)
    return f


def s3(f, **over):
    """the same contraction on exact-split planes (st_gemm_desc.split3)"""
    f = dict(f)
    rows_a = f["M"] // (f["Ho"] * f["Wo"]) * f["H"] * f["W"] * max(f["batch"], 1)
    rows_w = f["N"] * max(f["batch"], 1)
    f.update(split3=1, a_rows=rows_a, w_rows=rows_w, a_plane_stride=f["Cin"] * rows_a, w_plane_stride=f["K"] * rows_w)
    f.update(over)
    return f


def planes(f, **over):
    """the result also leaves as planes (st_gemm_desc.c_planes)"""
    f = dict(f)
    ncols = f["N"] // 2 if f.get("epi") == EPI["zr"] else f["N"]
    f.update(c_planes=PTR["c_planes"], c_plane_rows=f["M"], c_plane_stride=(ncols + 31) // 32 * f["M"] * 32)
    f.update(over)
    return f


def needs_chunks(f):
    """check_f32's test (csrc/gemm.hip): an fp32 descriptor beyond the 32-bit buffer offsets"""
    plain = (f["kh"], f["kw"], f["sh"], f["sw"], f["ph"], f["pw"]) == (1, 1, 1, 1, 0, 0) and f["H"] * f["W"] == f["M"] == f["Ho"] * f["Wo"]
    hw, img = (1, 1) if plain else (f["Ho"] * f["Wo"], f["H"] * f["W"])
    ab = ((f["M"] // hw * img - 1) * f["ldx"] + f["Cin"]) * 4
    ldmax = max([f["ldc"], f["N"]] + [f.get(ld, 0) for p, ld in (("aux0", "ld_aux0"), ("aux1", "ld_aux1"), ("aux2", "ld_aux2"), ("c2", "ldc2")) if f.get(p)])
    return ab >= 1 << 31 or (f["M"] + 256) * ldmax * 4 >= 1 << 31


CASES = []


def add(name, f, pair=None, tags=()):
    CASES.append((name, tuple(tags), copy.deepcopy(f), copy.deepcopy(pair)))


def mut(f, **over):
    g = dict(f)
    g.update(over)
    return g


# ---- every reportable plan ---------------------------------------------------------------------------------------------------------
add("skinny", mat(8, 1000, 2048), tags=["plan", "thr:skinny_M:lo"])
add("skinny_M9", mat(9, 1000, 2048), tags=["thr:skinny_M:hi"])
add("narrow", conv(2, 64, 64, 128, 4, 3, 3, ph=1, pw=1), tags=["plan", "thr:narrow_N:lo", "thr:narrow_M:hi"])
add("narrow_N5", conv(2, 64, 64, 128, 5, 3, 3, ph=1, pw=1), tags=["thr:narrow_N:hi"])
add("narrow_M1023", mat(1023, 4, 256), tags=["thr:narrow_M:lo"])
add("narrow_M1024", mat(1024, 4, 256), tags=["thr:narrow_M:hi"])
add("narrow3x3", conv(2, 64, 64, 256, 2, 3, 3, ph=1, pw=1), tags=["plan"])
for t in (1, 2, 3, 4):
    add(f"reg_tile{t}", conv(2, 64, 64, 36, 96, 3, 3, ph=1, pw=1, tile_cfg=t), tags=["plan"])
add("reg_scalar_gather", conv(2, 64, 64, 3, 64, 7, 7, 2, 2, 3, 3), tags=["plan"])
add("reg_misaligned_a", mat(8192, 128, 256, a=PTR["a"] + 4), tags=["plan"])
add("reg_split", mat(4096, 64, 528), tags=["plan"])                      # Cin % 32 != 0, 64 tiles, K >= 512
for t in (12, 13, 14, 15):
    add(f"dma_tile{t}", conv(2, 64, 64, 128, 256, 3, 3, ph=1, pw=1, tile_cfg=t), tags=["plan"])
add("dma_auto_conv", conv(2, 64, 64, 128, 256, 1, 5, pw=2), tags=["plan"])
add("dma_split", mat(4096, 128, 1024), tags=["plan"])
add("dma_persistent", mat(32768, 512, 256), tags=["plan"])
add("dma_persistent_ct", mat(4096, 4096, 256, c_t=PTR["c_t"], ld_ct=4096, batch=2, batch_stride_a=4096 * 256, batch_stride_w=4096 * 256,
                             batch_stride_c=4096 * 4096, workspace=0, workspace_floats=0), tags=["plan"])
add("dma_batched", mat(4096, 128, 4096, batch=2, batch_stride_a=4096 * 4096, batch_stride_w=128 * 4096, batch_stride_c=4096 * 128, workspace=0,
                       workspace_floats=0), tags=["plan"])
add("dma_a2", conv(1, 64, 128, 384, 128, 1, 5, pw=2, a2=PTR["a2"], a2_channels=128, epi=EPI["gru"], aux1=PTR["aux1"], ld_aux1=128,
                   aux2=PTR["aux2"], ld_aux2=384, act=ACT["tanh"]), tags=["plan"])
add("dma_zr_planes", planes(conv(1, 64, 128, 384, 256, 1, 5, pw=2, epi=EPI["zr"], aux1=PTR["aux1"], ld_aux1=384, c2=PTR["c2"], ldc2=384,
                                 act=ACT["sigmoid"])), tags=["plan"])
add("rowstream_K64", mat(32768, 256, 64), tags=["plan"])
add("rowstream_K128_ln", mat(4096, 128, 128, a_ln=1, a_ln_eps=1e-5), tags=["plan"])
add("rowstream_tile20", mat(4096, 128, 128, tile_cfg=20), tags=["plan"])
add("rowstream_mod32", mat(65536, 128, 64, aux0=PTR["aux0"], ld_aux0=128, aux0_row_mod=64, act=ACT["relu"]), tags=["plan"])
# row chunks: a whole-batch PatchEmbed tail (plain matrix, aux0 table of 64 rows) and its 6x6 stride-2 conv
add("chunk_matrix", mat(64 * 65536, 128, 64, aux0=PTR["aux0"], ld_aux0=128, aux0_row_mod=64), tags=["plan", "chunk:matrix"])
add("chunk_matrix_div8", mat(8 * 1048576, 128, 128, aux0=PTR["aux0"], ld_aux0=128, aux0_row_div=8), tags=["chunk:matrix"])
add("chunk_conv", conv(65536, 16, 16, 32, 64, 6, 6, 2, 2, 2, 2, Ho=8, Wo=8, M=65536 * 64), tags=["plan", "chunk:conv"])
add("chunk_conv_input", conv(32768, 32, 16, 32, 32, 6, 3, 2, 1, 2, 1, Ho=16, Wo=16, M=32768 * 256), tags=["chunk:conv"])

S3_CONV = s3(conv(2, 64, 64, 256, 256, 1, 5, pw=2))             # 8192 x 256 x 1280
for t in (31, 32, 33, 34, 35, 36, 37, 38, 39):
    add(f"s3_tile{t}", mut(S3_CONV, tile_cfg=t), tags=["plan"])
add("s3_auto_32", S3_CONV, tags=["plan"])
add("s3_auto_34_split", s3(conv(1, 64, 64, 384, 128, 1, 5, pw=2)), tags=["plan"])
add("s3_auto_39", s3(conv(2, 64, 64, 384, 128, 1, 5, pw=2)), tags=["plan"])
add("s3_auto_37", s3(mat(4096, 4096, 256, tile_cfg=0, batch=2, batch_stride_a=4096 * 32, batch_stride_w=4096 * 32, batch_stride_c=4096 * 4096)), tags=["plan"])
add("s3_ct", s3(mat(4096, 4096, 256, tile_cfg=37, c_t=PTR["c_t"], ld_ct=4096)), tags=["plan"])
add("s3_split_explicit", mut(S3_CONV, tile_cfg=34, split_k=4), tags=["plan"])
add("s3_a2_planes", planes(s3(conv(2, 64, 64, 384, 128, 1, 5, pw=2, a2=PTR["a2"], a2_channels=128, batch=1, epi=EPI["gru"], aux1=PTR["aux1"], ld_aux1=128,
                                   aux2=PTR["aux2"], ld_aux2=384))), tags=["plan"])

# ---- pairs (BasicMotionEncoder's convc2 / convf2) --------------------------------------------------------------------------------
P0 = conv(2, 64, 64, 256, 192, 3, 3, ph=1, pw=1, act=ACT["relu"])
P1 = conv(2, 64, 64, 128, 64, 3, 3, ph=1, pw=1, act=ACT["relu"])
add("pair_f32", P0, P1, tags=["plan"])
add("pair_s3", s3(P0), s3(P1), tags=["plan"])
add("pair_f32_tile13", mut(P0, tile_cfg=13), mut(P1, tile_cfg=13))
add("pair_s3_tile34", s3(mut(P0, tile_cfg=34)), s3(mut(P1, tile_cfg=34)))

# ---- both sides of every measured threshold, at the workload's shapes ---------------------------------------------------------------
for M in (16383, 16384):
    add(f"thr_rs_K64_M{M}", mat(M, 256, 64), tags=[f"thr:rowstream_K64_M16384:{'lo' if M < 16384 else 'hi'}"])
for M in (262143, 262144):
    add(f"thr_rs_K128_M{M}", mat(M, 128, 128), tags=[f"thr:rowstream_M262144:{'lo' if M < 262144 else 'hi'}"])
for N in (383, 384):
    add(f"thr_rs_N{N}_M32768", mat(32768, N, 128, ldc=384), tags=[f"thr:rowstream_N384:{'lo' if N < 384 else 'hi'}"])
for M in (32767, 32768):
    add(f"thr_rs_N384_rows{M}", mat(M, 384, 128), tags=[f"thr:rowstream_N384_M32768:{'lo' if M < 32768 else 'hi'}"])
for K in (64, 96, 128, 160, 256):
    add(f"thr_dma_K{K}", mat(8192, 160, K), tags=[f"thr:dma_K128:{'lo' if K < 128 else 'hi'}"] if K in (96, 128) else [])
for N in (32, 33):
    add(f"thr_narrow_tile_N{N}", mat(8192, N, 256), tags=[f"thr:tile_N32:{'lo' if N <= 32 else 'hi'}"])
    add(f"thr_narrow_tile_reg_N{N}", mat(8192, N, 100))
for tiles in (255, 256, 257, 511, 512, 513):
    for K in (480, 512, 992, 1024):
        add(f"thr_dma_tiles{tiles}_K{K}", mat(64 * tiles, 64, K), tags=[f"thr:dma_tiles:{tiles}", f"thr:dma_K:{K}"])
    add(f"thr_reg_tiles{tiles}", mat(64 * tiles, 64, 528), tags=[f"thr:reg_tiles:{tiles}"])
    add(f"thr_dma_walk_tiles{tiles}", mat(64 * tiles, 64, 128), tags=[f"thr:walk_tiles:{tiles}"])
    add(f"thr_dma_walk_ring_tiles{tiles}", mat(64 * tiles, 64, 160))
for K in (511, 512, 1023, 1024):
    add(f"thr_K{K}_tiles128", mat(8192, 64, K), tags=[f"thr:K:{K}"])
    add(f"thr_K{K}_tiles384", mat(8192, 192, K), tags=[f"thr:K:{K}"])
add("thr_split_clamp_16", mat(64, 64, 8192))
add("thr_split_clamp_K", mat(640, 64, 768))
add("thr_split_small_ws", mat(4096, 128, 1024, workspace_floats=2 * 4096 * 128 + 1))
add("thr_split_no_ws", mat(4096, 128, 1024, workspace=0, workspace_floats=0))
add("thr_split_off", mat(4096, 128, 1024, split_k=1))
add("thr_split_explicit", mat(4096, 128, 1024, split_k=3))
for b, tag in ((2047, "lo"), (2048, "hi")):
    add(f"thr_s3_walk_{b}", s3(mat(64 * b, 64, 256)), tags=[f"thr:s3_ntl64_2048:{tag}"])
    Mb, nb = (64 * 89, 23) if b == 2047 else (64 * 128, 16)
    add(f"thr_s3_walk_batched_{b}", s3(mat(Mb, 64, 256, batch=nb, batch_stride_a=Mb * 32, batch_stride_w=64 * 32, batch_stride_c=Mb * 64)),
        tags=[f"thr:s3_ntl64_2048:{tag}"])
for K in (2048, 2080):
    add(f"thr_s3_walk_K{K}", s3(mat(64 * 2048, 64, K)), tags=[f"thr:s3_walk_K2048:{'lo' if K <= 2048 else 'hi'}"])
for t128 in (255, 256):
    add(f"thr_s3_tile32_{t128}", s3(mat(128 * t128, 64, 1280)), tags=[f"thr:s3_tiles128_256:{'lo' if t128 < 256 else 'hi'}"])
for t64 in (255, 256, 257):
    for K in (992, 1024):
        add(f"thr_s3_kpar_{t64}_K{K}", s3(mat(64 * t64, 64, K)), tags=[f"thr:s3_ntl64_256:{t64}", f"thr:s3_kpar_K1024:{'lo' if K < 1024 else 'hi'}"])
    add(f"thr_s3_split_{t64}_K480", s3(mat(64 * t64, 64, 480)), tags=["thr:s3_split_K512:lo"])
    add(f"thr_s3_split_{t64}_K512", s3(mat(64 * t64, 64, 512)), tags=["thr:s3_split_K512:hi", f"thr:s3_tiles_256:{t64}"])
    add(f"thr_s3_split2_{t64}", s3(mat(64 * t64, 64, 1024, tile_cfg=34)), tags=[f"thr:s3_split2_256:{t64}"])
add("thr_s3_split2_K992", s3(mat(64 * 256, 64, 992, tile_cfg=34)))
add("thr_s3_no_ws", s3(mat(4096, 128, 1920, workspace=0, workspace_floats=0)))

# ---- the contractions of the workload (decoder at 64 x 64 and 64 x 128 maps, the Twins stages): what each gets today ----------------------------
for M in (4096, 8192, 32768):
    for N in (64, 128, 256, 384):
        for K in (128, 256, 512, 1024):
            add(f"work_f32_{M}x{N}x{K}", mat(M, N, K))
            if M <= 8192:
                add(f"work_s3_{M}x{N}x{K}", s3(mat(M, N, K)))

# ---- rejections: the accepted base of a path with ONE operand of ONE `return ST_EINVAL` violated ------------------------------------
F32 = conv(2, 64, 64, 128, 256, 3, 3, ph=1, pw=1)                      # LDS-DMA 64x64
F32_CT = mat(4096, 4096, 256, c_t=PTR["c_t"], ld_ct=4096, workspace=0, workspace_floats=0)
F32_A2 = mut(F32, a2=PTR["a2"], a2_channels=64)
F32_PL = planes(F32)
S3 = s3(F32)
S3_CT = s3(F32_CT, tile_cfg=37)
S3_A2 = s3(F32_A2)
S3_B = s3(mat(4096, 128, 4096, batch=2, batch_stride_a=4096 * 32, batch_stride_w=128 * 32, batch_stride_c=4096 * 128, workspace=0, workspace_floats=0))
for n, f in (("f32", F32), ("f32_ct", F32_CT), ("f32_a2", F32_A2), ("f32_planes", F32_PL), ("s3", S3), ("s3_ct", S3_CT), ("s3_a2", S3_A2), ("s3_batched", S3_B)):
    add(f"base_{n}", f, tags=["base"])
add("base_pair_f32_a2", mut(P0, a2=PTR["a2"], a2_channels=64), P1, tags=["base"])
add("base_pair_s3_a2", s3(mut(P0, a2=PTR["a2"], a2_channels=64)), s3(P1), tags=["base"])

COMMON = [       # (operand, mutation); what conv_gemm_launch, pair_member_prepare and split3_prepare all open with
    ("a", dict(a=0)), ("w", dict(w=0)), ("c", dict(c=0)), ("M", dict(M=0)), ("N", dict(N=0)), ("K", dict(K=0)),
    ("kh", dict(kh=0)), ("kw", dict(kw=0)), ("K_ne_khkwCin", dict(K=128 * 9 + 32)),
    ("Ho", dict(Ho=0)), ("Wo", dict(Wo=0)), ("M_mod_HoWo", dict(Ho=63)),
    ("epi_aux1", dict(epi=EPI["add"])), ("gru_aux2", dict(epi=EPI["gru"], aux1=PTR["aux1"], ld_aux1=256)),
    ("zr_c2", dict(epi=EPI["zr"], aux1=PTR["aux1"], ld_aux1=256)), ("zr_N_odd", dict(epi=EPI["zr"], aux1=PTR["aux1"], ld_aux1=256, c2=PTR["c2"], ldc2=256, N=191, w_rows=191)),
    ("reserved0", dict(reserved0=1)), ("reserved1", dict(reserved1=1)), ("reserved2", dict(reserved2=1)), ("reserved3", dict(reserved3=1)),
]
A2_OPS = [("a2_channels_le0", dict(a2_channels=0)), ("a2_channels_mod32", dict(a2_channels=48)), ("a2_channels_gt_Cin", dict(a2_channels=288)),
          ("a2_align", dict(a2=PTR["a2"] + 8))]
CT_OPS = [("ct_epi", dict(epi=EPI["add"], aux1=PTR["aux1"], ld_aux1=4096)), ("ct_M_mod4", dict(M=4094, W=4094, Wo=4094, a_rows=4094)),
          ("ct_ld_mod4", dict(ld_ct=4098)), ("ct_ld_lt_M", dict(ld_ct=4092)), ("ct_align", dict(c_t=PTR["c_t"] + 8)),
          ("ct_split_k", dict(split_k=2, workspace=PTR["workspace"], workspace_floats=1 << 40)),
          ("ct_reach", dict(N=131072 + 64, ldc=131072 + 64, w_rows=131072 + 64))]
PLANE_OPS = [("reserved4", dict(reserved4=1)), ("no_f32_without_planes", dict(c_planes=0, c_no_f32=1)), ("M_mod32", dict(M=8176, H=73, W=56, Ho=73, Wo=56, c_plane_rows=8192)),
             ("ncols_odd", dict(N=255)), ("col0_mod32", dict(c_plane_col0=16)), ("col0_neg", dict(c_plane_col0=-32)), ("row0_neg", dict(c_plane_row0=-1)),
             ("stride_le0", dict(c_plane_stride=0)), ("stride_mod8", dict(c_plane_stride=8 * 8192 * 32 + 4)), ("rows_le0", dict(c_plane_rows=0)),
             ("align", dict(c_planes=PTR["c_planes"] + 8)), ("c_t", dict(c_t=PTR["c_t"], ld_ct=8192)), ("last_row", dict(c_plane_row0=1)),
             ("extent", dict(c_plane_rows=1 << 22, c_plane_stride=8 * (1 << 22) * 32))]


def reject(fn, op, f, pair=None):
    add(f"rej_{fn}_{op}", f, pair, tags=[f"reject:{fn}:{op}"])


for op, m in COMMON:
    reject("conv_gemm_launch", op, mut(F32, **m))
    reject("pair_member_prepare", op, P0, mut(P1, **dict({k: v for k, v in m.items() if k != "w_rows"}, **({"N": 63} if "N" in m and m["N"] else {}))))
    reject("split3_prepare", op, mut(S3, **m))
for op, m in A2_OPS:
    reject("conv_gemm_launch", op, mut(F32_A2, **m))
    reject("pair_member_prepare", op, mut(P0, **dict(dict(a2=PTR["a2"], a2_channels=64), **m)), P1)
    reject("split3_prepare", op, mut(S3_A2, **m))
reject("conv_gemm_launch", "a2_batch", mut(F32_A2, batch=2))
reject("split3_prepare", "a2_batch", mut(S3_A2, batch=2, a_rows=2 * S3_A2["a_rows"], w_rows=512))
for op, m in CT_OPS:
    reject("conv_gemm_launch", op, mut(F32_CT, **{k: v for k, v in m.items() if k not in ("a_rows", "w_rows")}))
    reject("split3_prepare", op, mut(S3_CT, **m))
reject("conv_gemm_launch", "ct_a_ln", mut(F32_CT, a_ln=1))
reject("split3_prepare", "ct_a2", mut(S3_CT, a2=PTR["a2"], a2_channels=64))
reject("split3_prepare", "ct_c_planes", planes(S3_CT))
for op, m in PLANE_OPS:
    reject("c_planes_ok", op, mut(F32_PL, **m))
reject("c_planes_ok", "via_pair", P0, planes(P1, c_plane_col0=16))
reject("c_planes_ok", "via_split3", planes(S3, c_plane_col0=16))
# conv_gemm_launch: extents, row chunks, kernel preconditions
BIG = mat(1 << 21, 128, 128, ldc=256, workspace=0, workspace_floats=0)             # beyond the epilogue's reach: chunked
add("base_f32_chunked", BIG, tags=["base", "chunk:matrix"])
reject("conv_gemm_launch", "w_bytes", mat(4096, 1 << 20, 512, workspace=0, workspace_floats=0))
reject("conv_gemm_launch", "chunk_batch", mut(BIG, batch=2))
reject("conv_gemm_launch", "chunk_split_k", mut(BIG, split_k=2, workspace=PTR["workspace"], workspace_floats=1 << 40))
reject("conv_gemm_launch", "chunk_c_t", mut(BIG, c_t=PTR["c_t"], ld_ct=1 << 21))
reject("conv_gemm_launch", "chunk_c_planes", planes(mut(BIG, N=32, K=128)))
reject("conv_gemm_launch", "chunk_units_lt1", mat(64, 64, 128, ldc=1 << 27))
reject("conv_gemm_launch", "chunk_M_mod_unit", mut(BIG, aux0=PTR["aux0"], ld_aux0=128, aux0_row_mod=1000))
reject("conv_gemm_launch", "a_ln_kernel", mat(4096, 128, 256, a_ln=1))
reject("conv_gemm_launch", "a_ln_tile", mat(4096, 128, 128, a_ln=1, tile_cfg=13))
reject("conv_gemm_launch", "tile_ge20", mat(4096, 128, 256, tile_cfg=20))
reject("conv_gemm_launch", "dma_tile_not_ok", conv(2, 64, 64, 36, 96, 3, 3, ph=1, pw=1, tile_cfg=13))
reject("conv_gemm_launch", "a2_reg_tile", mut(F32_A2, tile_cfg=3))
reject("conv_gemm_launch", "ct_reg_tile", mut(F32_CT, tile_cfg=3))
reject("conv_gemm_launch", "split_batch", mat(4096, 128, 4096, batch=2, split_k=2))
reject("conv_gemm_launch", "split_no_workspace", mat(4096, 128, 1024, split_k=2, workspace=0))
reject("conv_gemm_launch", "split_workspace_small", mat(4096, 128, 1024, split_k=2, workspace_floats=2 * 4096 * 128 - 1))
for t in (5, 11):      # (6..10, 16..19 and negative values indexed past the tile table before this refactor: no recorded answer to compare with)
    reject("conv_gemm_launch", f"tile_{t}", mut(F32, tile_cfg=t))
reject("launch_rowstream", "slices", mat(1024, 9248, 128, tile_cfg=20))
# pair_member_prepare: its own rules (violations alternate between the members)
reject("pair_member_prepare", "K_lt128", P0, conv(2, 64, 64, 32, 64, 1, 3, pw=1))
reject("pair_member_prepare", "Cin_mod32", conv(2, 64, 64, 48, 192, 3, 3, ph=1, pw=1), P1)
reject("pair_member_prepare", "c_t", P0, mut(P1, c_t=PTR["c_t"], ld_ct=8192))
reject("pair_member_prepare", "a_ln", mut(P0, a_ln=1), P1)
reject("pair_member_prepare", "batch", P0, mut(P1, batch=2))
reject("pair_member_prepare", "split_k", mut(P0, split_k=2), P1)
reject("pair_member_prepare", "tile_cfg", P0, mut(P1, tile_cfg=12))
reject("pair_member_prepare", "a_align", mut(P0, a=PTR["a"] + 8), P1)
reject("pair_member_prepare", "w_align", P0, mut(P1, w=PTR["w"] + 8))
reject("pair_member_prepare", "ldx_mod4", mut(P0, ldx=258), P1)
reject("pair_member_prepare", "ldw_mod4", P0, mut(P1, ldw=128 * 9 + 2))
reject("pair_member_prepare", "w_bytes", P0, mut(P1, ldw=1 << 24))
reject("pair_member_prepare", "a_bytes", mut(P0, ldx=1 << 17), P1)
reject("pair_member_prepare", "reach", P0, mut(P1, ldc=1 << 17))
# split3_prepare: its own rules
reject("split3_prepare", "Cin_mod32", s3(conv(2, 64, 64, 48, 256, 3, 3, ph=1, pw=1)))
reject("split3_prepare", "a_ln", mut(S3, a_ln=1))
reject("split3_prepare", "split3_ne1", mut(S3, split3=2))
reject("split3_prepare", "a_plane_stride_le0", mut(S3, a_plane_stride=0))
reject("split3_prepare", "w_plane_stride_le0", mut(S3, w_plane_stride=0))
reject("split3_prepare", "a_rows_le0", mut(S3, a_rows=0))
reject("split3_prepare", "w_rows_lt_N", mut(S3, w_rows=255))
reject("split3_prepare", "a_align", mut(S3, a=PTR["a"] + 8))
reject("split3_prepare", "w_align", mut(S3, w=PTR["w"] + 8))
reject("split3_prepare", "a_plane_stride_mod8", mut(S3, a_plane_stride=S3["a_plane_stride"] + 4))
reject("split3_prepare", "w_plane_stride_mod8", mut(S3, w_plane_stride=S3["w_plane_stride"] + 4))
reject("split3_prepare", "batch_stride_a_mod8", mut(S3, batch_stride_a=4))
reject("split3_prepare", "batch_stride_w_mod8", mut(S3, batch_stride_w=4))
reject("split3_prepare", "in_rows_gt_a_rows", mut(S3, a_rows=8191))
reject("split3_prepare", "batch_stride_a_neg", mut(S3_B, batch_stride_a=-4096 * 32))
reject("split3_prepare", "batch_stride_w_neg", mut(S3_B, batch_stride_w=-128 * 32))
reject("split3_prepare", "batch_stride_a_mod32", mut(S3_B, batch_stride_a=4096 * 32 + 8))
reject("split3_prepare", "batch_stride_w_mod32", mut(S3_B, batch_stride_w=128 * 32 + 8))
reject("split3_prepare", "batch_a_rows", mut(S3_B, a_rows=8191))
reject("split3_prepare", "batch_w_rows", mut(S3_B, w_rows=255))
reject("split3_prepare", "a_bytes", mut(S3, a_rows=1 << 23, a_plane_stride=(1 << 23) * 128))
reject("split3_prepare", "w_bytes", mut(S3, w_rows=1 << 20, w_plane_stride=(1 << 20) * 1152))
reject("split3_prepare", "reach", mut(S3, ldc=1 << 17))
# conv_gemm_split3_launch
reject("conv_gemm_split3_launch", "tile_lt31", mut(S3, tile_cfg=13))
reject("conv_gemm_split3_launch", "tile_gt39", mut(S3, tile_cfg=40))
reject("conv_gemm_split3_launch", "kpar_split_k", mut(S3, tile_cfg=39, split_k=2))
reject("conv_gemm_split3_launch", "kpar_batch", mut(S3_B, tile_cfg=38))
reject("conv_gemm_split3_launch", "walk_a2", mut(S3_A2, tile_cfg=37))
reject("conv_gemm_split3_launch", "walk_split_k", mut(S3, tile_cfg=37, split_k=2))
reject("conv_gemm_split3_launch", "split_batch", mut(S3_B, split_k=2, workspace=PTR["workspace"], workspace_floats=WS_FLOATS))
reject("conv_gemm_split3_launch", "split_no_workspace", mut(S3, split_k=2, workspace=0))
reject("conv_gemm_split3_launch", "split_workspace_small", mut(S3, split_k=2, workspace_floats=2 * 8192 * 256 - 1))
# conv_gemm_split3_pair_launch
reject("conv_gemm_split3_pair_launch", "desc0_fp32", P0, s3(P1))
reject("conv_gemm_split3_pair_launch", "desc1_fp32", s3(P0), P1)
reject("conv_gemm_split3_pair_launch", "batch", s3(P0), s3(mut(P1, batch=2)))
reject("conv_gemm_split3_pair_launch", "split_k", s3(mut(P0, split_k=2)), s3(P1))
reject("conv_gemm_split3_pair_launch", "tile_cfg", s3(P0), s3(mut(P1, tile_cfg=32)))

# Two operands of the parent's rejections that no descriptor can violate alone, so they have no row:
#   conv_gemm_launch `units * unit >= d.M` -- the chunk passes the very tests the whole descriptor failed, so a chunk as large as M cannot pass;
#   pair_member_prepare `d.split3` -- st_conv_gemm_pair hands every pair with a split3 member to the split3 launcher first.
UNREACHABLE = ("conv_gemm_launch:chunk_units_ge_M", "pair_member_prepare:split3")

assert len({c[0] for c in CASES}) == len(CASES), "case names must be unique"


def desc(fields):
    """the st_gemm_desc of a case (stitch_amd._lib.GemmDesc)"""
    from stitch_amd._lib import GemmDesc
    d = GemmDesc()
    for k, v in fields.items():
        setattr(d, k, v)
    return d
