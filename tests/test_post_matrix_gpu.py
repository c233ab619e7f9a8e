"""The kernels behind the flow network over the shapes and edges at which they can go wrong: the per-pixel stages and the arg-max of
csrc/tps_pipeline.hip on 64 x 4-pixel blocks and flat 256-thread grids (widths 63 / 64 / 65, heights 1 to 5, more than six planes, h w one
short of, equal to and one past 256), the fp64 Gauss-Jordan of csrc/tps_solve.h on both sides of its LDS / workspace switch (n = 134 / 135)
and of its second stride trip (n + 3 > 256), tps2_warp up to its 3800-point limit, and the Telea inpainter of csrc/inpaint.hip at ring
depths past 128, 256 and 1024.  References, generators and tables: tests/_post_bounds.py; tests/test_post_bounds_cpu.py shows on the CPU what
this file relies on.

Bars.  Per-pixel kernels, range_argmax, the Telea fields d and T, the ring counts: bit for bit (torch.equal / np.array_equal).  Solves and the
bounded warp modes: the control rule against the reference's own fp32 run on the same case (err <= 4 max(err32, 2^-24); rms 2 x), recorded
through _measure.check.  The quantised warp and the Telea fill: equality away from a rounding boundary, with a stated cap / the teacher-forced
method of tests/test_inpaint_gpu.py.  Every operand sits inside a NaN frame (+-inf where a NaN would be swallowed: the min / max filter, the
arg-max), every output frame must be untouched outside its view."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _post_bounds as pb  # noqa: E402
from _measure import check  # noqa: E402
from test_geom_matrix_gpu import MARGIN, _release_frames, cid, errs, frame, frame_intact, ops, put, st  # noqa: E402,F401

INF = float("inf")
FLOOR = pb.FLOOR
MIN_SAMPLES = 64


def put_in(t, fill):
    """an input framed with `fill` instead of NaN (a NaN would lose every fmaxf / `>` it meets and go unseen)"""
    buf, view = frame(tuple(t.shape), t.dtype, t)
    buf[:MARGIN] = fill
    buf[MARGIN + t.numel():] = fill
    return view


def opt(st, t):
    return st.p(put(t)) if t is not None else None


def done(*frames):
    """after the launch: no write outside any output view"""
    torch.cuda.synchronize()
    for buf, view in frames:
        assert frame_intact(buf, view), "a write outside the output view"


# ================================================================================================ 1. per-pixel kernels, bit for bit
@pytest.mark.parametrize("shape", pb.SHAPES, ids=cid)
def test_flow_boxavg_matrix(st, shape):
    H, W = shape
    for tag, (flow, valid), k, neg in pb.boxavg_cases(shape):
        B, Cc = flow.shape[:2]
        o = frame((B, Cc, H, W))
        st.check(st.lib.st_flow_boxavg(st.p(put(flow)), opt(st, valid), st.p(o[1]), B, Cc, H, W, k, int(neg), st.stream()), "st_flow_boxavg")
        done(o)
        assert torch.equal(o[1].cpu(), pb.boxavg_ref(flow, valid, k, neg)), tag


@pytest.mark.parametrize("shape", pb.SHAPES, ids=cid)
def test_sobel_magnitude_matrix(st, shape):
    H, W = shape
    for tag, img in pb.sobel_cases(shape):
        o = frame((H, W))
        st.check(st.lib.st_sobel_magnitude(st.p(put(img)), st.p(o[1]), img.shape[1], H, W, st.stream()), "st_sobel_magnitude")
        done(o)
        assert torch.equal(o[1].cpu(), pb.sobel_ref(img)), tag


@pytest.mark.parametrize("shape", pb.SHAPES, ids=cid)
def test_minmax_filter_matrix(st, shape):
    """the input framed with the value that would WIN the filter: +inf for the max, -inf for the min"""
    H, W = shape
    for tag, x in pb.minmax_cases(shape):
        planes, k, is_max, axis = tag
        o = frame((planes, H, W))
        st.check(st.lib.st_minmax_filter(st.p(put_in(x, INF if is_max else -INF)), st.p(o[1]), planes, H, W, k, is_max, axis, st.stream()), "st_minmax_filter")
        done(o)
        assert torch.equal(o[1].cpu(), pb.minmax_ref(x, k, bool(is_max), axis)), tag


@pytest.mark.parametrize("shape", pb.SHAPES, ids=cid)
def test_box_sum_cmp_matrix(st, shape):
    H, W = shape
    for tag, x, k, pad, Ho, Wo, cmp in pb.box_cases_of(shape):
        o = frame((Ho, Wo))
        st.check(st.lib.st_box_sum_cmp(st.p(put(x)), H, W, st.p(o[1]), Ho, Wo, k, pad, cmp, st.stream()), "st_box_sum_cmp")
        done(o)
        assert torch.equal(o[1].cpu(), pb.box_ref(x, k, pad, Ho, Wo, cmp)), tag


@pytest.mark.parametrize("shape", pb.FLAT_SHAPES, ids=cid)
def test_tps_mask_inv_and_mix_blend_matrix(st, shape):
    H, W = shape
    for tag, wm in pb.mask_inv_cases(shape):
        o = frame((1, 1, H, W))
        st.check(st.lib.st_tps_mask_inv(st.p(put(wm)), st.p(o[1]), wm.shape[1], H, W, st.stream()), "st_tps_mask_inv")
        done(o)
        assert torch.equal(o[1].cpu(), pb.mask_inv_ref(wm)), tag
    for s in (0, 1):
        tps, inv_clean, fw, o1, m1 = pb.mix_blend_inputs(H, W, pb.flat_seed(shape, 6000) + 8 * s)
        t = frame((1, 3, H, W), fill=tps)                                                    # in place: tps3 *= tmask
        tm, mix, mm, bl = frame((1, 1, H, W)), frame((1, 3, H, W)), frame((1, 1, H, W)), frame((1, 3, H, W), torch.uint8)
        st.check(st.lib.st_tps_mix_blend(st.p(t[1]), st.p(put(inv_clean)), st.p(put(fw)), st.p(put(o1)), st.p(put(m1)), st.p(tm[1]), st.p(mix[1]),
                                         st.p(mm[1]), st.p(bl[1]), H, W, st.stream()), "st_tps_mix_blend")
        done(t, tm, mix, mm, bl)
        want = pb.mix_blend_ref(tps, inv_clean, fw, o1, m1)
        for name, got, ref in zip(("tps", "tmask", "mix", "mixmask", "blend"), (t, tm, mix, mm, bl), want):
            assert torch.equal(got[1].cpu(), ref), (name, s)


@pytest.mark.parametrize("shape", pb.FLAT_SHAPES, ids=cid)
def test_mix_plane_op_matrix(st, shape):
    n = shape[0] * shape[1]
    for op in (0, 1, 2):
        a, b = pb.plane_op_inputs(n, op, pb.flat_seed(shape, 7000) + 2 * op)
        o0, o1 = frame((n,)), frame((n,))
        st.check(st.lib.st_mix_plane_op(st.p(put(a)), st.p(put(b)) if op < 2 else None, st.p(o0[1]), st.p(o1[1]) if op < 2 else None, n, op, pb.THR,
                                        st.stream()), "st_mix_plane_op")
        done(o0, o1)
        r0, r1 = pb.plane_op_ref(a, b, op, pb.THR)
        assert torch.equal(o0[1].cpu(), r0), op
        assert torch.equal(o1[1].cpu(), r1) if op < 2 else bool(torch.isnan(o1[1]).all()), op
    a, b = pb.plane_op_inputs(n, 1, pb.flat_seed(shape, 7000) + 9)                           # op 1 without its second output
    o0 = frame((n,))
    st.check(st.lib.st_mix_plane_op(st.p(put(a)), st.p(put(b)), st.p(o0[1]), None, n, 1, 0.0, st.stream()), "st_mix_plane_op")
    done(o0)
    assert torch.equal(o0[1].cpu(), pb.plane_op_ref(a, b, 1)[0])


@pytest.mark.parametrize("shape", pb.FLAT_SHAPES, ids=cid)
def test_mix_stages_matrix(st, shape):
    H, W = shape
    seed = pb.flat_seed(shape, 8000)
    fw, occ, m1, tps, tm, o1 = pb.stage_inputs(H, W, seed)
    for method in (0, 1):
        a, am, i0 = frame((1, 3, H, W)), frame((1, 3, H, W)), frame((1, 1, H, W))
        st.check(st.lib.st_mix_stage_a(st.p(put(fw)), st.p(put(occ)), st.p(put(m1)), st.p(put(tps)), st.p(put(tm)), st.p(a[1]), st.p(am[1]), st.p(i0[1]),
                                       H, W, method, st.stream()), "st_mix_stage_a")
        done(a, am, i0)
        for got, ref in zip((a, am, i0), pb.stage_a_ref(fw, occ, m1, tps, tm, method)):
            assert torch.equal(got[1].cpu(), ref), method
    iam = pb.pick(pb.NEAR_HALF, (1, 1, H, W), seed + 7)
    dil = pb.binary((1, 1, H, W), seed + 8, 0.6)
    only, other = frame((1, 3, H, W)), frame((1, 1, H, W))
    st.check(st.lib.st_mix_stage_b(st.p(put(iam)), st.p(put(dil)), st.p(put(m1)), st.p(put(fw)), st.p(put(o1)), st.p(only[1]), st.p(other[1]), H, W,
                                   st.stream()), "st_mix_stage_b")
    done(only, other)
    r_only, r_other = pb.stage_b_ref(iam, dil, m1, fw, o1)
    assert torch.equal(only[1].cpu(), r_only) and torch.equal(other[1].cpu(), r_other)
    for mask, invert, clip in ((tm, 0, 0), (tm, 1, 0), (tm, 0, 1), (tm, 1, 1), (iam, 1, 1), (None, 0, 1), (None, 0, 0), (None, 1, 0)):
        o = frame((1, 3, H, W))
        st.check(st.lib.st_mix_mul_mask(st.p(put(o1)), opt(st, mask), st.p(o[1]), H, W, invert, clip, st.stream()), "st_mix_mul_mask")
        done(o)
        assert torch.equal(o[1].cpu(), pb.mul_mask_ref(o1, mask, bool(invert), bool(clip))), (mask is None, invert, clip)
    for c2 in (1, 3):
        a1, b1, a2, b2 = pb.blend_pair_inputs(H, W, c2, seed + 10 + c2)
        bl = frame((1, 3, H, W), torch.uint8)
        st.check(st.lib.st_blend_pair(st.p(put(a1)), st.p(put(b1)), st.p(put(a2)), st.p(put(b2)), c2, st.p(bl[1]), H, W, st.stream()), "st_blend_pair")
        done(bl)
        assert torch.equal(bl[1].cpu(), pb.blend_pair_ref(a1, b1, a2, b2)[0]), c2


@pytest.mark.parametrize("shape", [(1, 1), (5, 65), (9, 130), (4, 64), (3, 2)], ids=cid)
def test_gather_points_matrix(st, shape):
    H, W = shape
    for P in pb.GATHER_P:
        for n in pb.GATHER_N:
            planes, pts = pb.gather_inputs(H, W, P, n, 9000 + 10 * P + n)
            o = frame((n, P))
            st.check(st.lib.st_gather_points(st.p(put(planes)), st.p(put(pts)), st.p(o[1]), n, P, H, W, st.stream()), "st_gather_points")
            done(o)
            assert torch.equal(o[1].cpu(), pb.gather_ref(planes, pts)), (P, n)


# ================================================================================================ 2. range_argmax
def run_argmax(st, grad, ranges):
    """grad framed with +inf: an element read outside the plane would win"""
    H, W = grad.shape
    r = torch.tensor(ranges, dtype=torch.int32)
    o = frame((len(ranges),), torch.int32)
    st.check(st.lib.st_range_argmax(st.p(put_in(grad, INF)), st.p(put(r)), st.p(o[1]), len(ranges), H, W, st.stream()), "st_range_argmax")
    done(o)
    return o[1].cpu().tolist()


@pytest.mark.parametrize("plane", pb.ARGMAX_PLANES, ids=cid)
def test_range_argmax_windows(st, plane):
    """every window of the table, 1 and 70 ranges per launch, on a plane of five levels (every window holds its maximum many times: the first
    in row-major order must win everywhere) and on a plane of distinct values"""
    H, W = plane
    for quantised in (True, False):
        grad = pb.argmax_plane(H, W, 11 + H, quantised)
        for count in pb.ARGMAX_LAUNCH:
            ranges = pb.argmax_ranges(plane, count)
            assert run_argmax(st, grad, ranges) == pb.argmax_ref(grad, ranges), (quantised, count)
        for name, rng in pb.ARGMAX_WINDOWS[plane].items():
            assert run_argmax(st, grad, [rng]) == pb.argmax_ref(grad, [rng]), (quantised, name)


@pytest.mark.parametrize("tie", pb.ARGMAX_TIES, ids=lambda t: cid((t[0], t[1], t[2])))
def test_range_argmax_planted_ties(st, tie):
    plane, name, elems = tie
    grad, rng, first = pb.argmax_planted(plane, name, elems, pb.ARGMAX_TIES.index(tie))
    want = pb.argmax_ref(grad, [rng])
    assert want == [first]
    assert run_argmax(st, grad, [rng]) == want
    assert run_argmax(st, grad, [rng] * 70) == want * 70


# ================================================================================================ 3. TPS solves
def run_solve(st, kind, sites, centers, values, n):
    """the entry on framed operands, the workspace exactly the (n + 3)(n + 6) doubles ops.tps2_solve allocates -> (w [n + 3, 2], status)"""
    work = frame(((n + 3) * (n + 6),), torch.float64)
    kw, aw, status = frame((n, 2)), frame((3, 2)), frame((1,), torch.int32)
    if kind == "other":
        rc = st.lib.st_tps_other_solve(st.p(put(sites)), st.p(put(values)), st.p(work[1]), st.p(kw[1]), st.p(aw[1]), n, st.p(status[1]), st.stream())
    else:
        rc = st.lib.st_tps2_solve(st.p(put(sites)), st.p(put(centers)), st.p(put(values)), st.p(work[1]), st.p(kw[1]), st.p(aw[1]), n, kind, st.p(status[1]),
                                  st.stream())
    st.check(rc, "st_tps_solve")
    done(work, kw, aw, status)
    return torch.cat([kw[1].cpu(), aw[1].cpu()], 0), int(status[1].cpu())


SOLVE_CASES = [(m, n) for m in pb.SOLVE_MODES for n in pb.SOLVE_N] + [("other", n) for n in pb.OTHER_N]


@pytest.mark.parametrize("kind,n", SOLVE_CASES, ids=[f"{k}_{n}" for k, n in SOLVE_CASES])
def test_tps_solve_matrix(st, kind, n):
    """err = max |w - w64| / max |w64| <= 4 max(the fp32 torch.linalg.solve's err on the same case, 2^-24), status 0, workspace / output
    frames intact.  w64: the fp64 solution of the system the kernel builds (tests/_post_bounds.solve_case).  n = 134 | 135 is the LDS |
    workspace switch, n >= 252 the second trip of the row swap, n >= 254 of every other stride loop"""
    c = pb.solve_case(kind, n)
    w, status = run_solve(st, kind, c["sites"], c["centers"], c["values"], n)
    assert status == 0
    assert bool(torch.isfinite(w).all())
    if kind == 1:           # recorded, not asserted: the distance to the spline of the fp64-evaluated U is the fp32 rounding of K (tests/_post_bounds.py)
        check(f"post_solve_1_n{n}_vs_fp64_U", pb.rel_err(w, c["w64_fp64_U"]), INF, note="K rounded to fp32 against K in fp64; recorded only")
    err = pb.rel_err(w, c["w64"])
    check(f"post_solve_{kind}_n{n}", err, pb.solve_bound(c), inclusive=True, note=f"4 x max(ctl, 2^-24); ctl = {c['ctl']:.4g}: torch.linalg.solve in fp32 on the same system")


@pytest.mark.parametrize("n,what", [(134, "dup"), (135, "dup"), (135, "line")])
def test_tps_solve_singular_across_the_switch(st, ops, n, what):
    src, tgt = pb.singular_sets(n, what)
    for mode in pb.SOLVE_MODES:
        a, b = (src, tgt) if mode == 0 else (src * pb.PIXELS, tgt * pb.PIXELS)
        centers = b if mode == 0 else a
        _, status = run_solve(st, mode, a, centers, b, n)
        assert status == 1, mode
        with pytest.raises(ops.SingularTPSError):
            ops.tps2_solve(a.cuda(), centers.cuda(), b.cuda(), mode=mode)


# ================================================================================================ 5. Telea inpainting at deep rings
import _telea_ref as R  # noqa: E402
from test_inpaint_gpu import _check_fields, _synthetic, _teacher_forced  # noqa: E402


def telea_inputs(name):
    """the texture of test_inpaint_gpu._synthetic (no hole of its own), zeroed on the case's hole"""
    H, W, radius, _, _ = pb.TELEA_CASES[name]
    img, _ = _synthetic(H, W, "texture", seed=21)
    fill = torch.from_numpy(pb.telea_fill(name)).cuda()
    img = img.clone()
    img[fill] = 0
    return img, fill.to(torch.uint8) * 255, radius


@pytest.fixture(scope="module")
def telea_run():
    """name -> (out, d, T) on the host, d and T already bit-equal to tests/_telea_ref.py and the known pixels untouched; one GPU run per case"""
    cache = {}

    def get(name):
        if name not in cache:
            img, mask, radius = telea_inputs(name)
            cache[name] = _check_fields(img, mask, radius)
        return cache[name]
    return get


def forced(out, d, T, radius, pixels):
    """test_inpaint_gpu._teacher_forced's check on the given pixels: the byte is round-half-up of the float64 restatement evaluated on the GPU's
    own output below the ring; within 1e-3 of a .5 boundary either neighbour passes (counted)"""
    offs = R.disc(radius)
    ambiguous = 0
    for y, x in pixels:
        ref = R.fill_value(out, d, T, y, x, radius, offs)
        got, exp = out[y, x].astype(np.int64), R.round_u8(ref).astype(np.int64)
        near = np.abs(ref - np.floor(ref) - 0.5) < 1e-3
        assert ((got == exp) | (near & (np.abs(got - exp) <= 1))).all(), (int(d[y, x]), y, x, ref, got)
        ambiguous += int((near & (got != exp)).sum())
    return ambiguous


@pytest.mark.parametrize("name", ["window_r88", "wrap_r64"])
def test_telea_deep_rings_two_pixels_per_ring(telea_run, name):
    """window_r88: a ring-k pixel reads 124 rings below it along the diagonal, the widest the signed 8-bit tag difference has to carry, across
    k = 128 and k = 256.  wrap_r64: vertical rings up to k = 396, the tag wrapping on rings 96 pixels long"""
    H, W, radius, _, _ = pb.TELEA_CASES[name]
    out, d, T = telea_run(name)
    assert int(d.max()) == {"window_r88": 312, "wrap_r64": 396}[name]
    checked, amb = _teacher_forced(out, d, T, radius, per_ring=2)
    assert checked == int(np.minimum(np.bincount(d.ravel())[1:], 2).sum())                # the last ring of window_r88 is one pixel
    print(f"[{name}] rings {d.max()}, {checked} pixels checked, {amb} channel values within 1e-3 of .5 rounded the other way")


RING_GROUPS = [(120, 125), (126, 131), (132, 136), (248, 256), (257, 264)]


@pytest.mark.parametrize("lo,hi", RING_GROUPS)
def test_telea_window_r88_whole_rings_around_128_and_256(telea_run, lo, hi):
    out, d, T = telea_run("window_r88")
    ys, xs = np.nonzero((d >= lo) & (d <= hi))
    amb = forced(out, d, T, 88, zip(ys, xs))
    print(f"[window_r88 rings {lo}..{hi}] {len(ys)} pixels checked, {amb} ambiguous")


@pytest.mark.parametrize("name", ["strip", "strip_t"])
def test_telea_strips_past_ring_1024(st, telea_run, name):
    """d = x + y up to 1301 from the single known pixel: H + W + 1 = 1304 buckets (more than one per thread of ring_scan_kernel), rings on both
    sides of the 1024-bin LDS histogram of ring_hist_kernel / ring_scatter_kernel.  The ring counts read back are np.bincount(d), every hole
    pixel is written and every one is checked teacher-forced.  strip_t: one thread per column in dt_cols_kernel, 1300 row threads"""
    H, W, radius, _, _ = pb.TELEA_CASES[name]
    img, mask, _ = telea_inputs(name)
    nbytes = C.c_int64()
    st.check(st.lib.st_inpaint_telea_workspace(H, W, radius, C.byref(nbytes)), "st_inpaint_telea_workspace")
    work = torch.empty((nbytes.value,), device="cuda", dtype=torch.uint8)
    counts = frame((H + W + 1,), torch.int32)
    st.check(st.lib.st_inpaint_telea_rings(st.p(img), st.p(mask), H, W, radius, st.p(work), nbytes.value, st.p(counts[1]), st.stream()), "st_inpaint_telea_rings")
    done(counts)
    d_ref = R.ring_distance(pb.telea_fill(name))
    assert int(d_ref.max()) == 1301 and H + W + 1 > 1024
    assert np.array_equal(counts[1].cpu().numpy(), np.bincount(d_ref.ravel(), minlength=H + W + 1))
    out, d, T = telea_run(name)
    fill = pb.telea_fill(name)
    assert bool((T[fill] > 0).all()) and (out[fill].sum(-1) > 0).mean() > 0.9          # every hole pixel got its arrival time and a colour
    checked, amb = _teacher_forced(out, d, T, radius, per_ring=3)
    assert checked == int(fill.sum())
    print(f"[{name}] rings {d.max()}, {checked} pixels checked, {amb} ambiguous")


# ================================================================================================ 4. tps2_warp on given weights
WARP_KEYS = ("img", "centers", "kw", "aw", "kscale", "ascale", "align", "mode")


def run_warp(st, k):
    img = k["img"]
    _, Cc, H, W = img.shape
    o = frame((1, Cc, H, W))
    st.check(st.lib.st_tps2_warp(st.p(put(img)), st.p(put(k["centers"])), st.p(put(k["kw"])), st.p(put(k["aw"])), st.p(o[1]), Cc, H, W, k["centers"].shape[0],
                                 k["kscale"], k["ascale"], k["align"], k["mode"], st.stream()), "st_tps2_warp")
    done(o)
    return o[1].cpu()


@pytest.mark.parametrize("mode", pb.WARP_MODES)
@pytest.mark.parametrize("case", pb.WARP_CASES, ids=cid)
def test_tps2_warp_matrix(st, case, mode):
    """modes 0 and 1: the control rule against the fp32 control of the same case (e_rms <= 2 max(ctl, 2^-24), e_max <= 4 max(ctl, 2^-24); asserted
    from 64 samples on, recorded always).  mode 3: equal to the fp64 restatement (taps truncated, half to even) wherever its value before the
    rounding is further than E from a .5 boundary; at most 1 % of the case is left out.  aw[0] = inf: all zeros, no NaN"""
    k = pb.warp_case(case, mode)
    args = {key: k[key] for key in WARP_KEYS}
    out = run_warp(st, k)
    ref, pre = pb.warp_eval(**args)
    ctl = pb.warp_control(**args)
    name = f"post_warp_m{mode}_{cid(case)}"
    failed = []
    if mode == 3:
        near, E = pb.quant_near(pre, ctl)
        todo = [(name + "_left_out", near.double().mean().item(), pb.CAP, f"share within E = {E:.3g} of a .5 boundary; the cap is stated, not measured")]
        assert torch.equal(out, out.round()) and out.min() >= 0 and out.max() <= 255
        assert torch.equal(out.double()[~near], ref[~near]), int((out.double()[~near] != ref[~near]).sum())
    else:
        asserted = out.numel() >= MIN_SAMPLES
        (hr, hm), (cr, cm) = errs(out, ref), errs(ctl, ref)
        note = f"asserted: {asserted}; fp32 control of the same case: " + ("oracle warp_image_tps" if mode == 0 else "the formula in torch fp32, in index order")
        todo = [(name + "_rms", hr, 2.0 * max(cr, FLOOR) if asserted else INF, note), (name + "_max", hm, 4.0 * max(cm, FLOOR) if asserted else INF, note)]
    for nm, val, bound, nt in todo:                                      # every figure is recorded before any is asserted
        try:
            check(nm, val, bound, inclusive=True, note=nt)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "; ".join(failed)
    bad = dict(k, aw=k["aw"].clone())
    bad["aw"][0] = INF
    ob = run_warp(st, bad)
    assert bool((ob == 0).all())
