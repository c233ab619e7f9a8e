"""The warp, resize, splat, lookup and per-pixel kernels of csrc/geom.hip, csrc/flowops.hip and csrc/metrics.hip over the shapes at which a
64 x 4-pixel block, a 256-thread grid or a channel block can go wrong (H, W of 1 and 2, one short of, equal to and one past a block, several
blocks), over batch and channel strides, over the borders of the sampled image and over the numerics the single-shape tests of
test_ops_gpu.py never reach.  The references, bounds, generators and case tables are those of tests/_geom_bounds.py;
tests/test_geom_bounds_cpu.py shows on the CPU that fp32 meets the bounds, that planted defects do not, and that the tables cover their axes.

Bounded kernels (flow_warp, homo_flow_warp's image planes, resize_bilinear, cost_lookup, convex_upsample, range_map, flow_encode), per case:
(a) elementwise |out - ref| <= E against the fp64 statement of the operation, recorded as max err / E through _measure.check;
(b) the control rule of tests/test_stage_fp64_gpu.py against torch's CPU fp32 on the same inputs: e_rms(HIP) <= 2 max(e_rms(o32), 2^-24) and
    e_max(HIP) <= 4 max(e_max(o32), 2^-24), both recorded for every case.  They are asserted from MIN_SAMPLES outputs on (below that the two
    rms figures are estimates from too few draws to differ by a factor of 2 only for a reason, the argument of test_nn_matrix_gpu.py), and
    not for flow_encode, whose reason stands at CONTROL_OFF_FLOW_ENCODE.
Bit-exact kernels (homo_warp values and indices, morph_open, blend, blend_plain, eval_finish, mean_threshold, coords_grid(_init),
flow_from_coords, occlusion, load_rgb8, channel_mean, the overlap plane, masked_psnr_ssim to its existing bar) equal their restatements bit
for bit at every shape; where an fp64 reference is compared through a threshold, samples within E of it are left out, at most 1 % of a case.

Every operand sits at an offset inside a NaN-filled buffer (a sentinel byte / integer for the integer ones): an output buffer must be
untouched outside its view afterwards, and a read outside an input view would put a NaN into a result.  The entries are called through
lib.st_* directly where ops.py would allocate the output itself."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _geom_bounds as gb  # noqa: E402
from _measure import check  # noqa: E402
from test_split3_matrix_gpu import nan_wide, untouched  # noqa: E402

NAN = float("nan")
FLOOR = 2.0 ** -24
MARGIN = 8                                                        # elements of NaN in front of and behind every placed operand
MIN_SAMPLES = 64
CONTROL_OFF_FLOW_ENCODE = ("flow_encode_kernel adds its 98 products along ONE fma chain per output; torch's convolution sums in vector lanes and "
                           "blocks, so the control's accumulation error is that of a much shorter chain (the reason of the VALU attention case in "
                           "test_nn_matrix_gpu.py); bar (a), whose 98 is that chain, stands alone")


@pytest.fixture(scope="module")
def ops():
    import stitch_amd
    assert torch.cuda.is_available()
    return stitch_amd.ops


@pytest.fixture(scope="module")
def st(ops):
    """the C entry points, the error check and the two helpers of ops.py that turn a tensor into a pointer and name the stream"""
    from stitch_amd._lib import check as rc_check
    from stitch_amd._lib import lib

    class St:
        pass
    s = St()
    s.lib, s.check, s.p, s.stream = lib, rc_check, ops._p, ops._stream
    return s


# ================================================================================================ plumbing
SENTINEL = {torch.uint8: 0xA5, torch.int32: -0x5A5A5A5B, torch.int64: -0x5A5A5A5A5A5A5A5B}
_KEEP = []                                                        # every framed buffer of the running test: an entry is handed a bare pointer, so the
                                                                  # tensor behind it must outlive the call (a dropped one goes back to the allocator)


@pytest.fixture(autouse=True)
def _release_frames():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def frame(shape, dtype=torch.float32, fill=None):
    """(buffer, view): a contiguous `shape` view MARGIN elements inside a flat buffer of NaN (floats) or of a sentinel (integers);
    `fill`: a CPU tensor copied into the view"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * MARGIN,), NAN if dtype.is_floating_point else SENTINEL[dtype], device="cuda", dtype=dtype)
    view = buf[MARGIN:MARGIN + n].view(shape)
    if fill is not None:
        view.copy_(fill)
    _KEEP.append(buf)
    return buf, view


def frame_intact(buf, view):
    n = view.numel()
    edge = torch.cat([buf[:MARGIN], buf[MARGIN + n:]])
    return bool(torch.isnan(edge).all()) if buf.dtype.is_floating_point else bool((edge == SENTINEL[buf.dtype]).all())


def put(t):
    """an input: the view of `frame`"""
    return frame(tuple(t.shape), t.dtype, t)[1]


def rows_frame(rows, cols, ld, fill=None):
    """(buffer, view): [rows, cols] with row stride ld >= cols inside a flat NaN buffer -- ld == cols included, which nan_wide cannot give"""
    buf = torch.full((rows * ld + 2 * MARGIN,), NAN, device="cuda")
    view = buf.as_strided((rows, cols), (ld, 1), MARGIN)
    if fill is not None:
        view.copy_(fill)
    _KEEP.append(buf)
    return buf, view


def rows_intact(buf, view):
    keep = view.clone()
    view.fill_(NAN)
    ok = bool(torch.isnan(buf).all())
    view.copy_(keep)
    return ok


def errs(x, ref):
    x, ref = x.double().reshape(-1), ref.reshape(-1)
    if not bool(ref.any()):                                   # an exactly zero answer: only an exact zero is right
        e = 0.0 if not bool(x.any()) else float("inf")
        return e, e
    return ((x - ref).norm() / ref.norm()).item(), ((x - ref).abs().max() / ref.abs().max()).item()


def bars(name, out, ref, E, o32, control=True):
    """bar (a) and bar (b); every figure is recorded before any is asserted"""
    out, ref, E = out.detach().cpu(), ref.cpu(), E.cpu()
    assert out.shape == ref.shape == E.shape == o32.shape, (out.shape, ref.shape, E.shape, o32.shape)
    todo = [(f"geom_{name}_err_over_E", gb.ratio(out, ref, E), 1.0, "|out - ref| <= E elementwise, fp64 reference (tests/_geom_bounds.py)")]
    control = control and out.numel() >= MIN_SAMPLES
    hr, hm = errs(out, ref)
    cr, cm = errs(o32, ref)
    note = "torch CPU fp32 on the same inputs; multiples of tests/test_stage_fp64_gpu.py bar (a)" + ("" if control else "; recorded, not asserted")
    todo += [(f"geom_{name}_rms_over_ctl", hr / max(cr, FLOOR), 2.0 if control else float("inf"), note),
             (f"geom_{name}_max_over_ctl", hm / max(cm, FLOOR), 4.0 if control else float("inf"), note)]
    failed = []
    for nm, val, bound, nt in todo:
        try:
            check(nm, val, bound, inclusive=True, note=nt)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "; ".join(failed)


def cid(c):
    return "_".join(str(v).replace(" ", "").replace(".", "p") for v in c)


# ================================================================================================ flow_warp
def run_flow_warp(st, x, flow, mul):
    B, Cc, H, W = x.shape
    buf, out = frame((B, Cc, H, W))
    st.check(st.lib.st_flow_warp(st.p(put(x)), st.p(put(flow)), st.p(put(mul)) if mul is not None else None, st.p(out), B, Cc, H, W, st.stream()), "st_flow_warp")
    torch.cuda.synchronize()
    assert frame_intact(buf, out), "a write outside the output view"
    return out.cpu()


@pytest.mark.parametrize("case", gb.WARP_CASES, ids=cid)
def test_flow_warp_matrix(st, case):
    H, W, B, Cc, with_mul = case
    i = gb.WARP_CASES.index(case)
    x, flow = gb.image(B, Cc, H, W, 100 + i), gb.warp_flow(B, H, W, 200 + i)
    mul = torch.rand(B, 1, H, W, generator=gb.gen(300 + i)) * 2 - 0.5 if with_mul else None
    out = run_flow_warp(st, x, flow, mul)
    ref, E = gb.flow_warp_bound(x, flow, mul)
    bars("flow_warp_" + cid(case), out, ref, E, gb.flow_warp32(x, flow, mul))
    # the non-finite rule: a NaN / +-inf flow gives 0 there and leaves every other pixel's bits as they were
    bad = flow.clone()
    for k, v in enumerate((NAN, float("inf"), -float("inf"))):
        bad.view(-1)[(5 * k + 1) % bad.numel()] = v
    ob = run_flow_warp(st, x, bad, mul)
    hit = ~torch.isfinite(bad).all(1, keepdim=True).expand_as(ob)
    assert bool(torch.isfinite(ob).all()) and bool((ob[hit] == 0).all()) and torch.equal(ob[~hit], out[~hit])


# ================================================================================================ homo_flow_warp
@pytest.mark.parametrize("case", gb.HOMO_FLOW_CASES, ids=cid)
def test_homo_flow_warp_matrix(st, case):
    """B = 3, a homography of its own per item.  Hi and the overlap plane bit for bit against their restatements, the image planes and the
    ones planes within the gather's bound at the restated final flow."""
    H, W = case
    B, i = 3, gb.HOMO_FLOW_CASES.index(case)
    img, H8, flow = gb.homo_flow_inputs(B, H, W, 1000 + i)
    Hi_want, ff = gb.homo_flow_final_flow(H8, flow)
    b6, out6 = frame((B, 6, H, W))
    bo, ov = frame((B, H, W))
    bh, Hi = frame((B, 3, 3))
    st.check(st.lib.st_homo_flow_warp(st.p(put(img)), st.p(put(H8)), st.p(put(flow)), st.p(out6), st.p(ov), st.p(Hi), B, H, W, st.stream()), "st_homo_flow_warp")
    torch.cuda.synchronize()
    assert frame_intact(b6, out6) and frame_intact(bo, ov) and frame_intact(bh, Hi)
    out6, ov = out6.cpu(), ov.cpu()
    assert torch.equal(Hi.cpu(), Hi_want)
    x6 = torch.cat([img, torch.ones_like(img)], 1)
    ref, E = gb.flow_warp_bound(x6, ff)
    bars("homo_flow_warp_" + cid(case), out6, ref, E, gb.flow_warp32(x6, ff))
    assert torch.equal(out6[:, 3], out6[:, 4]) and torch.equal(out6[:, 3], out6[:, 5])
    assert torch.equal(ov, gb.overlap32(out6[:, 3]))                                         # the fp32 restatement: no exclusion
    near = (ref[:, 3] - 0.9).abs() <= E[:, 3]
    assert gb.capped_equal(ov, (ref[:, 3] < 0.9), near, cap=gb.CAP if H * W > 100 else 0.0)
    # the non-finite rule on this path: a NaN / +-inf residual flow gives 0 in all six planes (overlap 1) and leaves every other pixel's bits
    bad = flow.clone()
    for k, v in enumerate((NAN, float("inf"), -float("inf"))):
        bad.view(-1)[(5 * k + 1) % bad.numel()] = v
    b6n, out6n = frame((B, 6, H, W))
    bon, ovn = frame((B, H, W))
    st.check(st.lib.st_homo_flow_warp(st.p(put(img)), st.p(put(H8)), st.p(put(bad)), st.p(out6n), st.p(ovn), None, B, H, W, st.stream()), "st_homo_flow_warp")
    torch.cuda.synchronize()
    assert frame_intact(b6n, out6n) and frame_intact(bon, ovn)
    hit1 = ~torch.isfinite(bad).all(1)
    hit = hit1[:, None].expand(B, 6, H, W)
    o6n, on = out6n.cpu(), ovn.cpu()
    assert bool(torch.isfinite(o6n).all()) and bool((o6n[hit] == 0).all()) and torch.equal(o6n[~hit], out6[~hit])
    assert bool((on[hit1] == 1).all()) and torch.equal(on[~hit1], ov[~hit1])
    # without Hi: the same bits
    b6b, out6b = frame((B, 6, H, W))
    st.check(st.lib.st_homo_flow_warp(st.p(put(img)), st.p(put(H8)), st.p(put(flow)), st.p(out6b), st.p(frame((B, H, W))[1]), None, B, H, W, st.stream()), "st_homo_flow_warp")
    assert torch.equal(out6b.cpu(), out6) and frame_intact(b6b, out6b)


# ================================================================================================ homo_warp
@pytest.mark.parametrize("case", gb.HOMO_CASES, ids=cid)
def test_homo_warp_matrix(st, case):
    from oracle import cgeom
    H, W, oh, ow, B, Cc, n1 = case
    i = gb.HOMO_CASES.index(case)
    U = gb.image(B, Cc, H, W, 1100 + i)
    theta = (torch.eye(3)[None] + torch.randn(B, 3, 3, generator=gb.gen(1200 + i)) * torch.tensor([[0.1, 0.05, 0.1], [0.05, 0.1, 0.1], [0.03, 0.03, 0.0]])).reshape(B, 9)
    bo, out = frame((B, Cc + n1, oh, ow))
    bi, idx = frame((B, oh, ow, 4), torch.int32)
    st.check(st.lib.st_homo_warp(st.p(put(U)), st.p(put(theta)), st.p(out), st.p(idx), B, Cc, n1, H, W, oh, ow, st.stream()), "st_homo_warp")
    torch.cuda.synchronize()
    assert frame_intact(bo, out) and frame_intact(bi, idx)
    full = torch.cat([U, torch.ones(B, n1, H, W)], 1) if n1 else U
    ref_out, ref_idx = cgeom.homo_warp(full.numpy(), theta.numpy(), (oh, ow))
    assert np.array_equal(idx.cpu().numpy(), ref_idx)
    assert np.array_equal(out.cpu().numpy(), ref_out)


# ================================================================================================ resize_bilinear
@pytest.mark.parametrize("case", gb.RESIZE_CASES, ids=cid)
def test_resize_bilinear_matrix(st, case):
    H, W, oh, ow, align, B, Cc, div, scale = case
    i = gb.RESIZE_CASES.index(case)
    x = gb.image(B, Cc, H, W, 500 + i)
    steps = (1.0 / scale, 1.0 / scale) if scale else (1.0, 1.0)
    d0, d1, nd = (div[0], div[1], 2) if div else ((steps[0], steps[1], 0) if align == 2 else (1.0, 1.0, 0))
    buf, out = frame((B, Cc, oh, ow))
    st.check(st.lib.st_resize_bilinear(st.p(put(x)), st.p(out), B * Cc, H, W, oh, ow, align, d0, d1, nd, st.stream()), "st_resize_bilinear")
    torch.cuda.synchronize()
    assert frame_intact(buf, out)
    ref, E = gb.resize_bound(x, oh, ow, align, steps, div)
    bars(f"resize_{gb.resize_kind(case)}_" + cid(case), out, ref, E, gb.resize32(x, oh, ow, align, scale=scale, div=div))
    if (oh, ow) == (H, W) and div is None:
        assert torch.equal(out.cpu(), x)                                                      # the identity, bit for bit


# ================================================================================================ cost_lookup
@pytest.mark.parametrize("case", gb.LOOKUP_CASES, ids=cid)
def test_cost_lookup_matrix(st, case):
    H2, W2, r, Nq, extra = case
    i, nch = gb.LOOKUP_CASES.index(case), (2 * r + 1) ** 2
    maps, coords = gb.lookup_inputs(Nq, H2, W2, 400 + i)
    buf, out = rows_frame(Nq, nch, nch + extra)
    st.check(st.lib.st_cost_lookup(st.p(put(maps)), st.p(put(coords)), st.p(out), nch + extra, Nq, H2, W2, r, st.stream()), "st_cost_lookup")
    torch.cuda.synchronize()
    assert rows_intact(buf, out), "a write outside the output columns"
    ref, E = gb.cost_lookup_bound(maps, coords, H2, W2, r)
    bars("cost_lookup_" + cid(case), out, ref, E, gb.lookup32(maps, coords, H2, W2, r))


# ================================================================================================ convex_upsample
@pytest.mark.parametrize("case", gb.CONVEX_CASES, ids=cid)
def test_convex_upsample_matrix(st, case):
    B, H, W, ldm, amp = case
    i = gb.CONVEX_CASES.index(case)
    coords1, mask = gb.convex_inputs(B, H, W, 0.0 if amp == "dominant" else amp, 600 + i, dominant=amp == "dominant")
    _, mv = rows_frame(B * H * W, 576, ldm, mask)
    buf, out = frame((B, 2, 8 * H, 8 * W))
    st.check(st.lib.st_convex_upsample(st.p(put(coords1)), st.p(mv), ldm, st.p(out), B, H, W, st.stream()), "st_convex_upsample")
    torch.cuda.synchronize()
    assert frame_intact(buf, out)
    ref, E = gb.convex_upsample_bound(coords1, mask, B, H, W)
    bars("convex_upsample_" + cid(case), out, ref, E, gb.convex_upsample(coords1, mask, B, H, W, torch.float32))
    if amp == "dominant":                                       # every other weight underflows to an exact zero: the tap's value in fp32, bit for bit
        k = mask.view(B, H * W, 9, 64).argmax(2)
        want = torch.gather(gb.convex_taps(coords1, B, H, W, torch.float32), 2, k[..., None].expand(-1, -1, -1, 2))
        assert torch.equal(out.cpu(), gb.convex_assemble(want, B, H, W))


# ================================================================================================ flow_encode
@pytest.mark.parametrize("case", gb.ENCODE_CASES, ids=cid)
def test_flow_encode_matrix(st, ops, case):
    Co, H, W, B, with_flow2 = case
    i, R = gb.ENCODE_CASES.index(case), B * H * W
    coords1, w98, bias = gb.flow_encode_inputs(B, H, W, Co, 800 + i)
    c1, wd, bd = put(coords1), put(w98), put(bias)
    wide, out = nan_wide(R, Co, off=3, pad=5)                   # ldo = Co + 8 > Co
    wide2, f2 = nan_wide(R, 2, off=5, pad=1)                    # ld2 = 8 > 2
    ld2 = f2.stride(0) if with_flow2 else 0
    st.check(st.lib.st_flow_encode(st.p(c1), st.p(wd), st.p(bd), st.p(out), out.stride(0), st.p(f2) if with_flow2 else None, ld2, B, H, W, Co, st.stream()), "st_flow_encode")
    torch.cuda.synchronize()
    assert untouched(wide, 3, Co)
    ref, E, _ = gb.flow_encode_bound(coords1, w98, bias, B, H, W)
    bars("flow_encode_" + cid(case), out, ref, E, gb.flow_encode32(coords1, w98, bias, B, H, W), control=False)      # CONTROL_OFF_FLOW_ENCODE
    px, py = gb.pixel_xy(H, W, torch.float32)
    f32 = (coords1.view(B, H * W, 2) - torch.stack([px, py], -1)[None]).reshape(R, 2)
    if with_flow2:
        assert untouched(wide2, 5, 2) and torch.equal(f2.cpu(), f32)                          # one fp32 subtraction
    else:
        assert bool(torch.isnan(wide2).all())
    if Co % 32 == 0 and Co >= 32:                               # the split3 entry: the same fp32 bits, and planes that are st_split3 of them
        wide3, out3 = nan_wide(R, Co, off=3, pad=5)
        wide4, f4 = nan_wide(R, 2, off=5, pad=1)
        pl, fp = ops.Planes(R, Co, "cuda"), ops.Planes(R, 64, "cuda")
        fp.t.zero_()
        ops.flow_encode_split3(c1, wd, bd, out3, f4, B, H, W, pl, (fp, 34))
        torch.cuda.synchronize()
        assert untouched(wide3, 3, Co) and untouched(wide4, 5, 2)
        assert torch.equal(out3, out) and torch.equal(f4.cpu(), f32)
        assert torch.equal(pl.t, ops.split3_pack(out3.clone(memory_format=torch.contiguous_format).reshape(R, Co)).t)
        got = fp.t.double().sum(0).permute(1, 0, 2).reshape(R, 64).cpu()
        assert torch.equal(got[:, 34:36], f32.double()) and bool((got[:, :34] == 0).all()) and bool((got[:, 36:] == 0).all())


# ================================================================================================ coords_grid(_init), flow_from_coords
@pytest.mark.parametrize("case", gb.GRID_CASES, ids=cid)
def test_coords_grid_and_flow_from_coords(st, case):
    B, H, W, ld4 = case
    R = B * H * W
    px, py = gb.pixel_xy(H, W, torch.float32)
    grid = torch.stack([px, py], -1)[None].expand(B, -1, -1).reshape(R, 2)
    buf, cg = frame((R, 2))
    st.check(st.lib.st_coords_grid(st.p(cg), B, H, W, st.stream()), "st_coords_grid")
    torch.cuda.synchronize()
    assert frame_intact(buf, cg) and torch.equal(cg.cpu(), grid)
    init = gb.warp_flow(B, H, W, 1300 + R)                                                   # the same per-pixel kinds, different per item
    buf, ci = frame((R, 2))
    st.check(st.lib.st_coords_grid_init(st.p(ci), st.p(put(init)), B, H, W, st.stream()), "st_coords_grid_init")
    torch.cuda.synchronize()
    want = grid + init.reshape(B, 2, H * W).transpose(1, 2).reshape(R, 2)                     # one fp32 addition
    assert frame_intact(buf, ci) and torch.equal(ci.cpu(), want)
    flow = want - grid                                                                       # one fp32 subtraction
    for give4, give2 in ((True, True), (True, False), (False, True)):
        b4, f4 = rows_frame(R, ld4, ld4)
        wide2, d2 = nan_wide(R, 2, off=6, pad=3)
        st.check(st.lib.st_flow_from_coords(st.p(ci), st.p(f4) if give4 else None, ld4 if give4 else 0, st.p(d2) if give2 else None,
                                            d2.stride(0) if give2 else 0, B, H, W, st.stream()), "st_flow_from_coords")
        torch.cuda.synchronize()
        if give4:
            assert rows_intact(b4, f4) and torch.equal(f4[:, :2].cpu(), flow) and bool((f4[:, 2:] == 0).all())
        else:
            assert bool(torch.isnan(b4).all())
        if give2:
            assert untouched(wide2, 6, 2) and torch.equal(d2.cpu(), flow)
        else:
            assert bool(torch.isnan(wide2).all())


# ================================================================================================ range_map, occlusion
def run_range_map(st, flow):
    B, _, H, W = flow.shape
    bs, scratch = frame((B * H * W,), torch.int64)
    bo, out = frame((B, 1, H, W))
    st.check(st.lib.st_range_map(st.p(put(flow)), st.p(scratch), st.p(out), B, H, W, st.stream()), "st_range_map")
    torch.cuda.synchronize()
    assert frame_intact(bo, out) and frame_intact(bs, scratch)
    return out


@pytest.mark.parametrize("hw", gb.RANGE_HW, ids=cid)
def test_range_map_and_occlusion_matrix(st, hw):
    from oracle import cgeom
    H, W = hw
    for B, pattern in itertools.product((1, 3), gb.RANGE_PATTERNS):
        i = gb.RANGE_CASES.index((H, W, B, pattern))
        flow = gb.range_flow(pattern, B, H, W, 700 + i)
        out = run_range_map(st, flow)
        assert torch.equal(run_range_map(st, flow), out)                                     # two launches: the same bits
        ref, E = gb.range_map_bound(flow)
        bars(f"range_map_{H}x{W}_b{B}_{pattern}", out, ref, E, gb.range_map(flow, torch.float32))
        o = out.cpu()
        assert (o - torch.from_numpy(cgeom.range_map(flow.numpy()))).abs().max().item() < 1e-5   # the project's bar against its C restatement
        if pattern == "zero":
            assert bool((o == 1).all())
        if pattern == "leave":
            assert bool((o == 0).all())
        if pattern in ("collapse", "shift"):
            assert torch.equal(o.double(), ref)                                              # integer targets: exact, H W on one pixel
        # occlusion: soft = 1 - (1 - clamp) in fp32, exactly; hard = the soft output thresholded at 0.5, bit for bit
        bsf, soft = frame(tuple(out.shape))
        bh, hard = frame(tuple(out.shape))
        n = out.numel()
        st.check(st.lib.st_occlusion_from_range(st.p(out), st.p(soft), n, 0, st.stream()), "st_occlusion_from_range")
        st.check(st.lib.st_occlusion_from_range(st.p(out), st.p(hard), n, 1, st.stream()), "st_occlusion_from_range")
        torch.cuda.synchronize()
        assert frame_intact(bsf, soft) and frame_intact(bh, hard)
        assert torch.equal(soft.cpu(), 1.0 - (1.0 - o.clamp(0.0, 1.0)))
        assert torch.equal(hard.cpu(), (soft.cpu() >= 0.5).float())
        near = (ref.clamp(0, 1) - 0.5).abs() <= E
        assert gb.capped_equal(hard.cpu(), ref.clamp(0, 1) >= 0.5, near, cap=gb.CAP if H * W > 100 else 0.0)


def test_occlusion_on_the_threshold(st):
    """range values exactly 0.5, one ulp below and above, negative, above 1: n = 257 (a ragged second block)"""
    r = torch.rand(257, generator=gb.gen(5)) * 1.4 - 0.2
    r[:6] = torch.tensor([0.5, 0.5 - 2.0 ** -25, 0.5 + 2.0 ** -24, -0.0, 1.0, 1.0 + 2.0 ** -23])
    for thr in (0, 1):
        buf, out = frame((257,))
        st.check(st.lib.st_occlusion_from_range(st.p(put(r)), st.p(out), 257, thr, st.stream()), "st_occlusion_from_range")
        torch.cuda.synchronize()
        soft = 1.0 - (1.0 - r.clamp(0.0, 1.0))
        assert frame_intact(buf, out) and torch.equal(out.cpu(), (soft >= 0.5).float() if thr else soft)


# ================================================================================================ morph_open
@pytest.mark.parametrize("ksz", gb.MORPH_KSZ)
def test_morph_open_matrix(st, ksz):
    """ksz larger than, equal to and smaller than the image; N = B C of 1 and 6; densities near 0, near 1 and 0.5; input values exactly 0.5
    (set) and just below it (clear): bit for bit against the C restatement"""
    from oracle import cgeom
    for (H, W), N, dens in itertools.product(gb.MORPH_HW, (1, 6), (0.02, 0.5, 0.98)):
        g = gb.gen(1400 + 100 * H + W + N)
        on = torch.rand(N, 1, H, W, generator=g) < dens
        lvl = torch.rand(N, 1, H, W, generator=g)
        m = torch.where(on, torch.where(lvl < 0.5, torch.full_like(lvl, 0.5), 0.5 + lvl / 2), torch.where(lvl < 0.5, torch.full_like(lvl, 0.5 - 2.0 ** -25), lvl / 2))
        bs, scratch = frame((2 * N * H * W,), torch.uint8)
        bo, out = frame((N, 1, H, W))
        st.check(st.lib.st_morph_open(st.p(put(m)), st.p(out), st.p(scratch), N, H, W, ksz, st.stream()), "st_morph_open")
        torch.cuda.synchronize()
        assert frame_intact(bo, out) and frame_intact(bs, scratch)
        assert np.array_equal(out.cpu().numpy(), cgeom.morph_open(m.numpy(), ksz)), (H, W, N, dens)
        if ksz == 1:
            assert torch.equal(out.cpu(), (m >= 0.5).float())


# ================================================================================================ blend, blend_plain, eval_finish, mean_threshold
def canvas_inputs(h, w, seed):
    """[image | mask] triples as the canvas holds them: fractional masks with zones of exact 0 and 1 (0 / 0 -> byte 0), and pixels whose blend
    lands on x.0 and x.999 before the uint8 cast (equal images under a fractional mask give the image back up to a rounding)"""
    g = gb.gen(seed)
    t = [torch.rand(1, 6, h, w, generator=g) * 255 for _ in range(3)]
    for k, x in enumerate(t):
        x[:, 3:] = gb.mean_inputs((1, 1, h, w), 0.5, seed + 1 + k).expand(-1, 3, -1, -1)
    homo1, homo2, fin = t
    whole = (torch.rand(1, 1, h, w, generator=g) < 0.3).expand(-1, 3, -1, -1)                 # every view shows the same integer there
    v = torch.randint(0, 256, (1, 3, h, w), generator=g).float()
    for x in t:
        x[:, :3] = torch.where(whole, v, x[:, :3])
    occ = (torch.rand(1, 1, h, w, generator=g) > 0.3).float()
    return homo1, homo2, fin, occ


@pytest.mark.parametrize("hw", gb.PIXEL_HW, ids=cid)
def test_blend_family_matrix(st, hw):
    from oracle import adapter as oadapter
    h, w = hw
    homo1, homo2, fin, occ = canvas_inputs(h, w, 1500 + h)
    f = fin * occ
    _, o2r, m1r, m2r, bl = oadapter.blend_canvas(homo1, homo2, f)
    outs = [frame((1, 3, h, w)) for _ in range(3)] + [frame((1, 3, h, w), torch.uint8)]
    find = put(fin)
    st.check(st.lib.st_blend(st.p(put(homo1)), st.p(put(homo2)), st.p(find), st.p(put(occ)), *(st.p(v) for _, v in outs), h, w, st.stream()), "st_blend")
    torch.cuda.synchronize()
    assert all(frame_intact(b, v) for b, v in outs)
    for (_, got), want in zip(outs, (o2r, m1r, m2r, bl)):
        assert torch.equal(got.cpu(), want)
    assert torch.equal(find.cpu(), f)
    # blend_plain: no occlusion and no non-overlap factor, fin read only (the numpy statement of tests/test_branches_gpu.py, in torch)
    m1, m2 = homo1[:, 3:6], fin[:, 3:6]
    o2 = homo2[:, 0:3] * (1 - m2) + fin[:, 0:3] * m2
    mm2 = homo2[:, 3:6] * (1 - m2) + m2 * m2
    blp = torch.nan_to_num(((homo1[:, 0:3] * m1 + o2 * mm2) / (m1 + mm2)).clip(0, 255), nan=0.0).to(torch.uint8)
    wants = (o2, m1.mean(1, keepdim=True).clip(0, 1).repeat(1, 3, 1, 1), mm2.mean(1, keepdim=True).clip(0, 1).repeat(1, 3, 1, 1), blp)
    outs = [frame((1, 3, h, w)) for _ in range(3)] + [frame((1, 3, h, w), torch.uint8)]
    find = put(fin)
    st.check(st.lib.st_blend_plain(st.p(put(homo1)), st.p(put(homo2)), st.p(find), *(st.p(v) for _, v in outs), h, w, st.stream()), "st_blend_plain")
    torch.cuda.synchronize()
    assert all(frame_intact(b, v) for b, v in outs) and torch.equal(find.cpu(), fin)
    for (_, got), want in zip(outs, wants):
        assert torch.equal(got.cpu(), want)
    for B in (1, 3):
        # eval_finish: overlap = mean(final[:, 3:6]) < 0.9 as ((a + b) + c) / 3 in fp32, final *= occ in place
        fin6 = torch.cat([gb.image(B, 3, h, w, 1600 + h), gb.mean_inputs((B, 3, h, w), 0.9, 1601 + h)], 1)
        occ2 = (torch.rand(B, 1, h, w, generator=gb.gen(1602 + h)) > 0.5).float()
        b6, f6 = frame((B, 6, h, w), fill=fin6)
        bo, ov = frame((B, h, w))
        st.check(st.lib.st_eval_finish(st.p(f6), st.p(put(occ2)), st.p(ov), B, h, w, st.stream()), "st_eval_finish")
        torch.cuda.synchronize()
        mean3 = ((fin6[:, 3] + fin6[:, 4]) + fin6[:, 5]) / 3.0
        assert frame_intact(b6, f6) and frame_intact(bo, ov)
        assert torch.equal(ov.cpu(), (mean3 < 0.9).float()) and torch.equal(f6.cpu(), fin6 * occ2)
        for Cc in (1, 3, 5):
            x = gb.mean_inputs((B, Cc, h, w), 0.5, 1700 + h + Cc)
            x[:, :, 0, 0] = 0.5                                                              # the mean exactly on the threshold: not above it
            bm, mt = frame((B, 1, h, w))
            st.check(st.lib.st_mean_threshold(st.p(put(x)), st.p(mt), B, Cc, h, w, 0.5, st.stream()), "st_mean_threshold")
            torch.cuda.synchronize()
            s = torch.zeros(B, h, w)
            for c in range(Cc):
                s = s + x[:, c]
            assert frame_intact(bm, mt) and torch.equal(mt.cpu()[:, 0], ((s / float(Cc)) > 0.5).float())
            want, near = gb.mean_threshold_bound(x, 0.5)
            near[:, :, 0, 0] = True                                                          # the planted tie
            assert gb.capped_equal(mt.cpu(), want, near, cap=B / near.numel() + (gb.CAP if h * w > 100 else 0.0))


# ================================================================================================ metrics
@pytest.mark.parametrize("hw", gb.METRIC_HW, ids=cid)
def test_metrics_matrix(st, hw):
    """masked_psnr_ssim to its existing bar against the fp64 oracle (one SSIM window at 7 x 7), channel_mean bit for bit; the 6-channel
    input is a view whose batch stride is larger than 6 H W; masks all 1, all 0 (PSNR +inf, SSIM 1, as the oracle gives) and mixed"""
    from oracle import metrics
    H, W = hw
    for B, kind in itertools.product((1, 3), ("ones", "zeros", "mixed")):
        g = gb.gen(1800 + H + W + B)
        img = (torch.rand(B, 3, H, W, generator=g) * 255).round()
        warped = (img + torch.randn(B, 3, H, W, generator=g) * 10).clamp(-20, 280)
        mask3 = torch.ones(B, 3, H, W) if kind != "zeros" else torch.zeros(B, 3, H, W)
        if kind == "mixed":
            mask3[:, :, :, W // 2:] = 0
            mask3[B - 1, 0, 1:3, 0:2] = 0.5
        stride = 6 * H * W + 12
        buf = torch.full((B * stride + 2 * MARGIN,), NAN, device="cuda")
        fwo = buf.as_strided((B, 6, H, W), (stride, H * W, W, 1), MARGIN)
        fwo.copy_(torch.cat([warped, mask3], 1))
        bv, valid = frame((B, H, W))
        st.check(st.lib.st_channel_mean(st.p(fwo[:, 3:6]), stride, st.p(valid), B, 3, H, W, st.stream()), "st_channel_mean")
        nblk = (3 * H * W + 255) // 256
        bp, partial = frame((2 * B * nblk,), torch.float64)
        bo, out = frame((B, 2), torch.float64)
        st.check(st.lib.st_masked_psnr_ssim(st.p(put(img)), st.p(fwo), stride, st.p(valid), st.p(partial), st.p(out), B, H, W, st.stream()), "st_masked_psnr_ssim")
        torch.cuda.synchronize()
        assert frame_intact(bv, valid) and frame_intact(bp, partial) and frame_intact(bo, out)
        vm = ((mask3[:, 0] + mask3[:, 1]) + mask3[:, 2]) / 3.0
        assert torch.equal(valid.cpu(), vm)
        got = out.cpu().numpy()
        for b in range(B):
            with np.errstate(divide="ignore"):
                p, s = metrics.pair_metrics(img[b].numpy(), warped[b].numpy(), vm[b:b + 1].numpy())
            assert (np.isinf(p) and got[b, 0] == p) or abs(got[b, 0] - p) < 1e-9 * max(1.0, abs(p)), (kind, got[b, 0], p)
            assert abs(got[b, 1] - s) < 1e-9, (kind, got[b, 1], s)
        if kind == "zeros":
            assert np.isposinf(got[:, 0]).all() and (got[:, 1] == 1.0).all()


@pytest.mark.parametrize("hw", [(2, 2), (2, 4), (26, 30)], ids=cid)
def test_load_rgb8_matrix(st, hw):
    """h w = 4, 8, 260 * 3; B = 1 and 3; bit for bit against the host-side conversion"""
    H, W = hw
    for B in (1, 3):
        src = torch.randint(0, 256, (B, H, W, 3), generator=gb.gen(1900 + H + B), dtype=torch.uint8)
        bo, out = frame((B, 3, H, W))
        st.check(st.lib.st_load_rgb8(st.p(put(src)), st.p(out), B, H, W, st.stream()), "st_load_rgb8")
        torch.cuda.synchronize()
        assert frame_intact(bo, out) and torch.equal(out.cpu(), src.permute(0, 3, 1, 2).float())


# ================================================================================================ mesh_bounds
def test_mesh_bounds_matrix(ops):
    """the loop of test_ops_gpu.py::test_mesh_bounds, with one-point, four-point and tall meshes and B = 4; the second call goes into the
    same buffer.  The contract stays: min / max exact up to the fp32 evaluation of the mesh, and equal int() canvas bounds."""
    from oracle import geom
    gen = gb.gen(77)
    buf, out = frame((4,))
    for trial, (gw, gh, B) in enumerate([(0, 0, 1), (1, 1, 4), (3, 600, 2), (0, 0, 4), (3, 600, 4), (12, 7, 4)]):
        Hm = torch.eye(3)[None].repeat(B, 1, 1) + torch.randn(B, 3, 3, generator=gen) * torch.tensor([[0.05, 0.05, 60.0], [0.05, 0.05, 60.0], [1e-4, 1e-4, 0.0]])
        w, h = 37 + 10 * trial, 29
        mesh = geom.h2mesh(Hm, geom.rigid_mesh(B, h, w, gh, gw))
        want = torch.stack([mesh[..., 0].min(), mesh[..., 0].max(), mesh[..., 1].min(), mesh[..., 1].max()])
        for rep in range(2):
            ops.mesh_bounds(put(Hm), out, w, h, gw, gh)
            got = out.cpu()
            assert frame_intact(buf, out)
            assert (got - want).abs().max() <= 1e-3 * max(1.0, want.abs().max().item()), (trial, got, want)
            assert torch.equal(got.int(), want.int()) or (got - want).abs().max() < 1e-4, (trial, got, want)


# ================================================================================================ rejected arguments (no launch)
def test_rejections_on_device_tensors(ops):
    """what the kernels cannot take comes back as an error from the host, on real device tensors too: zero sizes, a row stride below the
    columns written, a cost map of one row or column, an unknown resize mode, a mode-2 resize whose output is larger than the scale gives.
    (The full list: tests/test_geom_bounds_cpu.py, where no GPU is needed; such a call is never launched to see what happens.)"""
    from stitch_amd._lib import check as rc_check
    from stitch_amd._lib import lib
    z = torch.zeros(1 << 16, device="cuda")
    Err, stream = ops.StitchErrorBase, ops._stream
    img = z[:2 * 3 * 8 * 8].view(2, 3, 8, 8)
    with pytest.raises(Err, match="ST_EINVAL"):
        ops.cost_lookup(z[:4 * 8].view(4, 8), z[:8].view(4, 2), z[1024:1024 + 4 * 84].view(4, 84), 4, 8, 1)
    with pytest.raises(Err, match="ST_EINVAL"):
        ops.cost_lookup(z[:4 * 8].view(4, 8), z[:8].view(4, 2), z[1024:1024 + 4 * 84].view(4, 84), 4, 1, 8)
    with pytest.raises(Err, match="ST_EINVAL"):
        ops.cost_lookup(z[:4 * 64].view(4, 64), z[:8].view(4, 2), z[1024:1024 + 4 * 80].view(4, 80), 4, 8, 8)         # ldo < 81
    with pytest.raises(Err, match="ST_EINVAL"):
        ops.resize_bilinear(img, 4, 4, 3)
    with pytest.raises(Err, match="ST_EINVAL"):
        ops.resize_bilinear(img, 12, 12, 2, div=(1.0, 1.0))                                  # scale 1 cannot give 12 rows of 8
    with pytest.raises(Err, match="ST_EINVAL"):
        ops.resize_bilinear(img, 0, 4, True)
    with pytest.raises(Err, match="ST_EINVAL"):
        ops.coords_grid(z[:64].view(32, 2), 2, 0, 4)
    with pytest.raises(Err, match="ST_EINVAL"):
        ops.flow_from_coords(z[:64].view(32, 2), z[1024:1024 + 32].view(32, 1), None, 2, 4, 4)                      # ld4 < 2
    with pytest.raises(Err, match="ST_EINVAL"):
        ops.convex_upsample(z[:64].view(32, 2), z[1024:1024 + 32 * 575].view(32, 575), z[32768:32768 + 2 * 2 * 32 * 32].view(2, 2, 32, 32), 2, 4, 4)
    with pytest.raises(Err, match="ST_EINVAL"):
        ops.convex_upsample(z[:64].view(32, 2), z[1024:1024 + 32 * 576].view(32, 576), z[32768:], 2, 0, 4)
    with pytest.raises(Err, match="ST_EINVAL"):                                                                 # ldo = 64 < Co = 128
        ops.flow_encode(z[:64].view(32, 2), z[1024:1024 + 98 * 128].view(98, 128), z[:128], z[32768:32768 + 32 * 64].view(32, 64), None, 2, 4, 4)
    # zero sizes with real, non-empty device buffers behind every pointer (an empty tensor's null pointer would be rejected for being null)
    p, q, s = (C.c_void_p(z[k << 12:].data_ptr()) for k in range(3))
    more = [C.c_void_p(z[k << 12:].data_ptr()) for k in range(3, 8)]
    for H, W in ((0, 8), (8, 0)):
        calls = dict(st_flow_warp=lambda: lib.st_flow_warp(p, q, None, s, 2, 3, H, W, stream()),
                     st_range_map=lambda: lib.st_range_map(p, q, s, 2, H, W, stream()),
                     st_morph_open=lambda: lib.st_morph_open(p, q, s, 2, H, W, 3, stream()),
                     st_mean_threshold=lambda: lib.st_mean_threshold(p, q, 2, 3, H, W, 0.5, stream()),
                     st_eval_finish=lambda: lib.st_eval_finish(p, q, s, 2, H, W, stream()),
                     st_blend=lambda: lib.st_blend(p, q, s, *more, H, W, stream()),
                     st_channel_mean=lambda: lib.st_channel_mean(p, 6 * 64, q, 2, 3, H, W, stream()),
                     st_coords_grid=lambda: lib.st_coords_grid(p, 2, H, W, stream()),
                     st_homo_flow_warp=lambda: lib.st_homo_flow_warp(p, q, s, more[0], more[1], None, 2, H, W, stream()))
        for name, call in calls.items():
            with pytest.raises(Err, match="ST_EINVAL"):
                rc_check(call(), name)
    with pytest.raises(Err, match="ST_EINVAL"):
        ops.load_rgb8(torch.zeros(1, 3, 3, 3, dtype=torch.uint8, device="cuda"))             # h w % 4 != 0
    torch.cuda.synchronize()
