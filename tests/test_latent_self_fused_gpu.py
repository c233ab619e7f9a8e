"""st_latent_self_attn_split3 (csrc/mlp_split3.h, latent_self_attn_split3_kernel): LayerNorm -> q | k | v -> the 8-latent, 8-head, D = 16 attention
of every cost map in one launch, against the two launches it replaces, st_rowlin128_split3 -> st_attention_small, on the same inputs and weights.

The bar is torch.equal, no tolerance: the products are the same MFMA chains (the pack kernel permutes weight rows, which moves a product to another
accumulator slot and changes nothing else) and the row arithmetic is one device function (csrc/attn_small.h) that both attention kernels call.

Row counts: 8 (one cost map, a partial block), 32 (one block), 40 (a block and a partial one), 8 * 257 (several workgroups, partial last block),
8 * 4099 (32 792 rows = 1 025 blocks: a launch of 257 workgroups; the ring runs 12 steps per block) and 65 536 + 8 * 5 (2 050 blocks against the
grid cap of 512 workgroups x 4 waves: a second round, so the block loop and its prefetch across rounds run, with idle waves in the last round).
Input patterns: normal data; rows scaled by 1e4 (the softmax maximum decides everything); a cost map of 8 identical rows (tied scores); one NaN and
one +inf element (same non-finite pattern, equal finite values)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

EINVAL = 1001
ROWS = [8, 32, 40, 8 * 257, 8 * 4099, 65536 + 8 * 5]
PATTERNS = ["normal", "scaled_1e4", "tied_map", "nonfinite"]


@pytest.fixture(scope="module")
def ops():
    import stitch_amd
    assert torch.cuda.is_available()
    return stitch_amd.ops


@pytest.fixture(scope="module")
def weights(ops):
    """non-trivial LayerNorm weight / bias folded into random q | k | v weights, and the two images of them"""
    g = torch.Generator().manual_seed(20261)
    gamma = (1.0 + 0.3 * torch.randn(128, generator=g)).cuda()
    beta = (0.2 * torch.randn(128, generator=g)).cuda()
    w = (torch.randn(384, 128, generator=g) / 128 ** 0.5).cuda()
    b = (0.1 * torch.randn(384, generator=g)).cuda()
    wf, bf = ops.fold_layernorm(gamma, beta, w, b)
    wf, bf = wf.contiguous(), bf.contiguous()
    return dict(w=wf, b=bf, lin=ops.rowlin128_split3_pack(wf, bf), fused=ops.latent_self_attn_split3_pack(wf, bf))


def make_rows(M, pattern):
    g = torch.Generator().manual_seed(1000 + M)
    x = torch.randn(M, 128, generator=g)
    if pattern == "scaled_1e4":
        x *= 1e4
    elif pattern == "tied_map":
        m = (M // 8) // 2
        x[8 * m:8 * m + 8] = x[8 * m].clone()
    elif pattern == "nonfinite":
        x[M // 2, 5] = float("nan")
        x[M - 1, 77] = float("inf")
        if M > 8:
            x[3, 0] = float("inf")
    return x.cuda()


def unfused(ops, x, weights, ln_eps):
    M = x.shape[0]
    qkv = torch.empty(M, 384, device="cuda")
    ops.rowlin128_split3(x, qkv, weights["lin"], ln_eps=ln_eps)
    att = torch.empty(M, 128, device="cuda")
    ops.attention_small(qkv[:, :128], (8 * 384, 384), qkv[:, 128:256], (8 * 384, 384), qkv[:, 256:], (8 * 384, 384), att, (8 * 128, 128),
                        M // 8, 8, 8, 8, 16, 16 ** -0.5)
    return att


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("M", ROWS)
def test_fused_equals_the_two_launches(ops, weights, M, pattern):
    x = make_rows(M, pattern)
    # scaled rows run twice: through LayerNorm as every other pattern (which takes the factor out again), and without it, so that the 1e4 reaches
    # q and k and the scores of a row lie ~1e8 apart
    if pattern == "scaled_1e4":
        run_case(ops, weights, x, pattern, None)
    run_case(ops, weights, x, pattern, 1e-5)


def run_case(ops, weights, x, pattern, ln_eps):
    M = x.shape[0]
    ref = unfused(ops, x, weights, ln_eps)
    wide = torch.full((M, 136), float("nan"), device="cuda")          # the output as a column slice: row stride 136, the frame stays NaN
    out = wide[:, 4:132]
    ops.latent_self_attn_split3(x, out, weights["fused"], ln_eps=ln_eps)
    torch.cuda.synchronize()
    assert bool(torch.isnan(wide[:, :4]).all()) and bool(torch.isnan(wide[:, 132:]).all())
    if pattern == "nonfinite":
        assert torch.equal(torch.isnan(out), torch.isnan(ref)) and torch.equal(torch.isinf(out), torch.isinf(ref))
        # a non-finite element makes its whole cost map NaN (its k and v rows reach all 8 queries): 8 rows are one map; from 32 rows on a map stays clean
        assert bool(torch.isnan(ref).any()) and (M < 32 or bool(torch.isfinite(ref).any()))
        assert torch.equal(torch.nan_to_num(out, nan=0.0), torch.nan_to_num(ref, nan=0.0))
    else:
        assert bool(torch.isfinite(ref).all())
        assert torch.equal(out, ref)
    # rerun into the same buffer: same bits
    ops.latent_self_attn_split3(x, out, weights["fused"], ln_eps=ln_eps)
    assert torch.equal(torch.nan_to_num(out, nan=0.0), torch.nan_to_num(ref, nan=0.0))


def test_input_row_stride(ops, weights):
    """rows as a column slice of a wider buffer (lda = 136)"""
    M = 8 * 37
    x = make_rows(M, "normal")
    wide = torch.full((M, 136), float("nan"), device="cuda")
    wide[:, 4:132] = x
    out = torch.empty(M, 128, device="cuda")
    ops.latent_self_attn_split3(wide[:, 4:132], out, weights["fused"], ln_eps=1e-5)
    assert torch.equal(out, unfused(ops, x, weights, 1e-5))


def test_rejections_leave_the_output_alone(ops, weights):
    from stitch_amd._lib import lib
    M = 16
    x = make_rows(M, "normal")
    buf = torch.full((M * 128 + 8,), -7.0, device="cuda")
    out = buf[:M * 128].view(M, 128)
    img = weights["fused"]
    p = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731

    def call(a=x, o=out, rows=M, image=p(img), nbytes=img.numel(), lda=128, ldo=128):
        return lib.st_latent_self_attn_split3(p(a), lda, p(o) if o is not None else None, ldo, rows, 1, 1e-5, 0.25, image, nbytes, None)

    assert call(rows=12) == EINVAL                                   # not whole cost maps
    assert call(o=buf[1:1 + M * 128].view(M, 128)) == EINVAL         # output 4 bytes off a 16-byte boundary
    assert call(image=None) == EINVAL
    assert call(nbytes=img.numel() - 1536) == EINVAL and call(nbytes=img.numel() + 16) == EINVAL
    assert call(o=None) == EINVAL and call(rows=0) == EINVAL and call(ldo=126) == EINVAL and call(lda=64) == EINVAL and call(o=x) == EINVAL
    torch.cuda.synchronize()
    assert bool((buf == -7.0).all())
    nb = C.c_int64(0)
    assert lib.st_latent_self_attn_split3_image_bytes(C.byref(nb)) == 0 and nb.value == img.numel() == 12 * 24576 + 1536
    assert lib.st_latent_self_attn_split3_pack(p(weights["w"]), p(weights["b"]), p(img), img.numel() - 16, None) == EINVAL
    assert lib.st_latent_self_attn_split3_pack(None, p(weights["b"]), p(img), img.numel(), None) == EINVAL
    assert call() == 0                                               # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert torch.equal(out, unfused(ops, x, weights, 1e-5))


def test_model_latent_self_with_and_without_the_image(seeded_sd):
    """FlowFormer._latent_self on M = 64 cost maps: the fused entry against the layer with its packed image removed (the unfused path)"""
    import stitch_amd
    cfg, _ = stitch_amd.load_inference_config("all_img1_with_inpaint_g12_transRef")
    m = stitch_amd.build_model(cfg)
    m.load_state_dict(seeded_sd, strict=True)
    fb = m.cuda().eval().flow_backbone
    fb.pack()
    x = torch.randn(64 * 8, 128, generator=torch.Generator().manual_seed(5)).cuda()
    for L in fb._pk["self"]:
        assert L.get("attn_s3") is not None
        fused = fb._latent_self(L, x, 64).clone()
        plain = fb._latent_self({k: v for k, v in L.items() if k != "attn_s3"}, x, 64).clone()
        assert bool(torch.isfinite(fused).all()) and torch.equal(fused, plain)
