"""The kernels of csrc/transref.hip and the wrapper steps of stitch_amd/transref.py over their shapes, the strided layouts the entry points
allow, their edges and the numerics the first-generation tests in test_transref_gpu.py never reach (a running maximum that rises tile after
tile, large logits, one dominant key, equal keys, ragged Nq and Nk at every head dimension, sample points on -1 and H and their float
neighbours, both GELU tails, 0 / 255 masks).  The references, bounds, tables and generators are those of tests/_transref_bounds.py;
tests/test_transref_bounds_cpu.py shows on the CPU that fp32 meets the bounds and that planted defects do not.

Three bars per case, none taken from a GPU measurement:

(a) elementwise: |out - ref| <= E, ref the fp64 statement of the operation, E the first-order worst-case bound of _transref_bounds.py;
    recorded as max err / E through _measure.check.  No exception.
(b) the control rule of tests/test_stage_fp64_gpu.py: with e_rms(X) = |X - ref|_2 / |ref|_2, e_max(X) = max|X - ref| / max|ref| and o32 =
    torch's CPU fp32 on the same inputs in the same run,  e_rms(HIP) <= 2 max(e_rms(o32), 2^-24)  and  e_max(HIP) <= 4 max(e_max(o32), 2^-24).
    Recorded for every case and asserted, except for the cases CONTROL_OFF names with their reason (at most one in ten of a kernel's table).
(c) bit identities: a query's output row does not depend on the other queries; every layout gives the bits of the contiguous one; a
    heads = h launch equals h single-head launches; zero and integer offsets make the deform sampler a pure gather; the interleave, the sum
    and the wrapper steps equal their torch-CPU fp32 statements bit for bit.

Every operand sits at an offset inside a NaN-filled buffer: an output buffer must be NaN outside the view afterwards, and a read outside an
input view would put a NaN into the result."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import _transref_bounds as tb  # noqa: E402
from _measure import check  # noqa: E402
from _nn_bounds import ratio  # noqa: E402
from test_split3_matrix_gpu import nan_wide, untouched  # noqa: E402

NAN = float("nan")
FLOOR = 2.0 ** -24
MARGIN = 8                                                        # floats of NaN in front of and behind every placed operand (keeps 32-byte alignment)

# where bar (b) is not asserted: case name -> reason.  The multiples stay 2 and 4 everywhere else.
CONTROL_OFF = {}


@pytest.fixture(scope="module")
def ops():
    import stitch_amd
    assert torch.cuda.is_available()
    return stitch_amd.ops


def errs(x, ref):
    x, ref = x.double().reshape(-1), ref.reshape(-1)
    if not bool(ref.any()):                                   # an exactly zero answer: only an exact zero is right
        e = 0.0 if not bool(x.any()) else float("inf")
        return e, e
    return ((x - ref).norm() / ref.norm()).item(), ((x - ref).abs().max() / ref.abs().max()).item()


def bars(name, out, ref, E, o32):
    """bar (a) and bar (b); every figure is recorded before any is asserted"""
    out, o32 = out.detach().cpu(), o32.detach().cpu()
    assert out.shape == ref.shape == E.shape == o32.shape, (out.shape, ref.shape, E.shape, o32.shape)
    control = name not in CONTROL_OFF
    todo = [(f"tr_{name}_err_over_E", ratio(out, ref, E), 1.0, "|out - ref| <= E elementwise, fp64 reference (tests/_transref_bounds.py)")]
    (hr, hm), (cr, cm) = errs(out, ref), errs(o32, ref)
    note = "torch CPU fp32 on the same inputs; multiples of tests/test_stage_fp64_gpu.py" + ("" if control else "; recorded, not asserted: " + CONTROL_OFF[name])
    todo += [(f"tr_{name}_rms_over_ctl", hr / max(cr, FLOOR), 2.0 if control else float("inf"), note),
             (f"tr_{name}_max_over_ctl", hm / max(cm, FLOOR), 4.0 if control else float("inf"), note)]
    failed = []
    for nm, val, bound, nt in todo:
        try:
            check(nm, val, bound, inclusive=True, note=nt)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "; ".join(failed)


def test_the_attention_table_covers_the_axes():
    """every pair (D, Nk) and every pair (D, Nq); heads, amplitudes, input kinds and layouts all occur (more in test_transref_bounds_cpu.py)"""
    cases = tb.ATT_CASES
    assert {(c[0], c[1]) for c in cases} == {(D, Nk) for D in tb.ATT_D for Nk in tb.ATT_NK}
    assert {(c[0], c[2]) for c in cases} == {(D, Nq) for D in tb.ATT_D for Nq in tb.ATT_NQ}
    for ax, vals in ((3, tb.ATT_HEADS), (4, tb.AMPS), (5, tb.ATT_KINDS), (6, tb.ATT_LAYOUTS)):
        assert {c[ax] for c in cases} == set(vals), ax


def test_control_exclusions_are_named_and_few():
    names = {"att_" + tb.att_id(c) for c in tb.ATT_CASES}
    off = [n for n in CONTROL_OFF if n.startswith("att_")]
    assert set(off) <= names and 10 * len(off) <= len(names)
    assert all(n.startswith(("att_", "deform_", "dwconv_", "prepare_")) and CONTROL_OFF[n] for n in CONTROL_OFF)
    for prefix, count in (("deform_", len(tb.DEFORM_HWC) * len(tb.DEFORM_FAMILIES)), ("dwconv_", len(tb.DW_HWC) * len(tb.DW_AMPS)), ("prepare_", len(tb.ORIGINS))):
        assert 10 * len([n for n in CONTROL_OFF if n.startswith(prefix)]) <= count


# ================================================================================================ placement
def placed(rows, C, off, ld, data=None, shared=None):
    """a [rows, C] view with row stride ld at float offset MARGIN + off of a NaN buffer (`shared`: an existing buffer) -> (buffer, view)"""
    n = MARGIN + off + (rows - 1) * ld + C + MARGIN
    flat = torch.full((n,), NAN, device="cuda") if shared is None else shared
    assert flat.numel() >= n
    view = flat.as_strided((rows, C), (ld, 1), MARGIN + off)
    if data is not None:
        view.copy_(data)
    return flat, view


def att_layout(lay, C):
    """operand -> (float offset, row stride); "kv": k and v share one buffer"""
    sp = dict(q=(0, C), k=(0, C), v=(0, C), o=(0, C))
    if lay == "slices":                                       # q and out as column slices of wider buffers, the offset a multiple of 4 floats
        sp.update(q=(8, C + 16), o=(4, C + 8))
    if lay == "kvhalf":                                       # k | v halves of one [Nk, 2C] buffer, as TransRefNet.block lays them out
        sp.update(k=(0, 2 * C), v=(C, 2 * C))
    if lay == "odd":                                          # v and out at an address that is only 4-byte aligned, with an odd ld
        sp.update(v=(1, C + 3), o=(3, C + 1))
    return sp


def run_attention(ops, lay, q, k, v, heads, D, scale=None):
    """-> out [Nq, C] (a clone); asserts the rest of the output buffer is still NaN"""
    C, Nq, Nk = heads * D, q.shape[0], k.shape[0]
    sp = att_layout(lay, C)
    _, qv = placed(Nq, C, *sp["q"], data=q)
    if lay == "kvhalf":
        kvbuf = torch.full((2 * MARGIN + Nk * 2 * C,), NAN, device="cuda")
        _, kv = placed(Nk, C, *sp["k"], data=k, shared=kvbuf)
        _, vv = placed(Nk, C, *sp["v"], data=v, shared=kvbuf)
    else:
        _, kv = placed(Nk, C, *sp["k"], data=k)
        _, vv = placed(Nk, C, *sp["v"], data=v)
    obuf, ov = placed(Nq, C, *sp["o"])
    if lay == "odd":
        assert vv.data_ptr() % 16 == 4 and ov.data_ptr() % 16 == 12 and vv.stride(0) % 2 == 1 and ov.stride(0) % 2 == 1
    assert qv.data_ptr() % 16 == 0 and kv.data_ptr() % 16 == 0
    ops.tr_attention(qv, kv, vv, ov, heads, D, D ** -0.5 if scale is None else scale)
    torch.cuda.synchronize()
    out = ov.clone()
    ov.fill_(NAN)
    assert bool(torch.isnan(obuf).all()), "a write outside the output view"
    return out


# ================================================================================================ st_tr_attention
@pytest.mark.parametrize("case", tb.ATT_CASES, ids=tb.att_id)
def test_attention_matrix(ops, case):
    D, Nk, Nq, heads, amp, kind, lay = case
    q, k, v = tb.att_inputs(heads, Nq, Nk, D, amp, kind, 1000 + tb.ATT_CASES.index(case))
    out = run_attention(ops, lay, q, k, v, heads, D)
    ref, E, smax = tb.att_bound(q, k, v, heads, D, D ** -0.5)
    if kind in ("randn", "equal"):
        assert abs(smax - amp) < 1e-3 * amp, (smax, amp)
    bars("att_" + tb.att_id(case), out, ref, E, tb.att32(q, k, v, heads, D, D ** -0.5))
    if kind == "dominant" and Nk > 1:                         # every other weight underflows to an exact zero and the sum is 1: that V row, bit for bit
        s = D ** -0.5 * (q.double().view(Nq, heads, D).transpose(0, 1) @ k.double().view(Nk, heads, D).permute(1, 2, 0))
        top = s.topk(2, -1)
        assert (top.values[..., 0] - top.values[..., 1]).min() > 100
        want = torch.cat([v[:, h * D:(h + 1) * D][top.indices[h, :, 0]] for h in range(heads)], 1)
        assert torch.equal(out.cpu(), want)
    if Nk == 1:
        assert torch.equal(out.cpu(), v.expand(Nq, -1))


@pytest.mark.parametrize("D", tb.ATT_D)
def test_attention_queries_are_independent(ops, D):
    """a prefix of Nq cut inside a wave (45, 1), inside a workgroup (100: its fourth wave has 4 queries) and one past a workgroup (129) gives
    the bits of the full run"""
    heads, Nq, Nk = 2, 300, 65
    q, k, v = tb.att_inputs(heads, Nq, Nk, D, 20.0, "randn", 2000 + D)
    full = run_attention(ops, "contig", q, k, v, heads, D)
    for n in (129, 100, 45, 1):
        part = run_attention(ops, "contig", q[:n].contiguous(), k, v, heads, D)
        assert torch.equal(part, full[:n]), (D, n, (part != full[:n]).sum().item())


@pytest.mark.parametrize("D", tb.ATT_D)
def test_attention_layouts_and_head_launches_same_bits(ops, D):
    """every layout gives the bits of the contiguous one, and a heads = 3 launch those of three single-head launches on column views"""
    heads, Nq, Nk = 3, 129, 65
    C = heads * D
    q, k, v = tb.att_inputs(heads, Nq, Nk, D, 20.0, "rise", 2100 + D)
    base = run_attention(ops, "contig", q, k, v, heads, D)
    for lay in tb.ATT_LAYOUTS[1:]:
        assert torch.equal(run_attention(ops, lay, q, k, v, heads, D), base), lay
    (_, qv), (_, kv), (_, vv) = (placed(t.shape[0], C, 0, C, data=t) for t in (q, k, v))
    obuf, ov = placed(Nq, C, 0, C)
    for h in range(heads):
        sl = slice(h * D, (h + 1) * D)
        ops.tr_attention(qv[:, sl], kv[:, sl], vv[:, sl], ov[:, sl], 1, D, D ** -0.5)
    torch.cuda.synchronize()
    assert torch.equal(ov, base)
    ov.fill_(NAN)
    assert bool(torch.isnan(obuf).all())


def test_attention_rejections_leave_the_output_untouched(ops):
    """what the kernel cannot take comes back as an error from the host and nothing is launched: the NaN output stays NaN"""
    heads, D, N = 2, 64, 40
    C = heads * D
    z = torch.zeros(1 << 16, device="cuda")
    obuf, ov = placed(N, C, 0, C)
    view = lambda off=0, ld=C, rows=N, cols=C: z.as_strided((rows, cols), (ld, 1), off)      # noqa: E731
    good = dict(q=view(), k=view(), v=view(), o=ov, heads=heads, D=D)
    bad = [dict(D=48, q=view(cols=96), k=view(cols=96), v=view(cols=96)),
           dict(q=view(off=1)), dict(k=view(off=1)), dict(q=view(off=3)), dict(k=view(off=2)),
           dict(q=view(ld=C + 2)), dict(k=view(ld=C + 1)), dict(q=view(ld=C + 3)),
           dict(q=view(ld=C - 4)), dict(k=view(ld=C - 4)), dict(v=view(ld=C - 1)), dict(o=z.as_strided((N, C), (C - 1, 1), 1 << 15)),
           dict(heads=0), dict(k=view(rows=0), v=view(rows=0))]
    for kw in bad:
        a = dict(good, **kw)
        with pytest.raises(ops.StitchErrorBase):
            ops.tr_attention(a["q"], a["k"], a["v"], a["o"], a["heads"], a["D"], 0.125)
    torch.cuda.synchronize()
    assert bool(torch.isnan(obuf).all()) and not bool(z.any())
    ops.tr_attention(good["q"], good["k"], good["v"], ov, heads, D, 0.125)                      # the unspoilt call is accepted
    torch.cuda.synchronize()
    assert bool((ov == 0).all())


# ================================================================================================ st_tr_deform_im2col
def run_deform(ops, x, off, H, W):
    n, C = x.shape
    _, xv = nan_wide(n, C, off=1, pad=3)
    _, offv = nan_wide(n, 18, off=2, pad=3)
    xv.copy_(x)
    offv.copy_(off)
    frame = torch.full((n + 2, 9 * C), NAN, device="cuda")
    ops.tr_deform_im2col(xv, offv, frame[1:-1], H, W)
    torch.cuda.synchronize()
    assert bool(torch.isnan(frame[0]).all() and torch.isnan(frame[-1]).all())
    return frame[1:-1].cpu()


@pytest.mark.parametrize("H,W,C", tb.DEFORM_HWC)
def test_deform_im2col_matrix(ops, H, W, C):
    i = tb.DEFORM_HWC.index((H, W, C))
    x = torch.randn(H * W, C, generator=tb.gen(300 + i)) + 0.5
    for fam in tb.DEFORM_FAMILIES:
        outs, refs, Es, ctls = [], [], [], []
        for shift in range(tb.EDGE_SHIFTS if fam.startswith("edge") else 1):
            off = tb.deform_offsets(H, W, fam, 310 + i, shift)
            out = run_deform(ops, x, off, H, W)
            ref, E = tb.deform_bound(x, off, H, W)
            if fam == "zero":                                 # the plain zero-padded im2col, bit for bit
                assert torch.equal(out, tb.im2col_zero_padded(x, H, W))
            if fam == "integer":                              # a pure gather
                assert torch.equal(out.double(), ref)
            if fam == "far":
                h, w = tb.deform_coords(off, H, W)
                gone = ((h.abs() > 1e5) | (w.abs() > 1e5))[..., None].expand(-1, -1, C).reshape(H * W, 9 * C)
                assert bool((out[gone] == 0).all())
            outs.append(out), refs.append(ref), Es.append(E), ctls.append(tb.deform_cols(x, off, H, W, torch.float32))
        bars(f"deform_{H}x{W}x{C}_{fam}", *(torch.cat(t) for t in (outs, refs, Es, ctls)))


# ================================================================================================ st_tr_phase_interleave, st_tr_add
@pytest.mark.parametrize("H,W,C", tb.PHASE_HWC)
def test_phase_interleave_bit_exact(ops, H, W, C):
    i = tb.PHASE_HWC.index((H, W, C))
    ph = torch.randn(4, H * W, C, generator=tb.gen(400 + i))
    res = torch.randn(4 * H * W, C, generator=tb.gen(450 + i))
    for with_res in (False, True):
        wide, out = nan_wide(4 * H * W, C, off=1, pad=3)
        rv = None
        if with_res:
            _, rv = nan_wide(4 * H * W, C, off=2, pad=5)
            rv.copy_(res)
        ops.tr_phase_interleave(ph.cuda(), out, H, W, res=rv)
        torch.cuda.synchronize()
        assert untouched(wide, 1, C)
        assert torch.equal(out.cpu(), tb.phase_interleave(ph, H, W, res if with_res else None)), with_res


@pytest.mark.parametrize("rows,C", [(1, 1), (7, 37), (300, 5), (3, 256)])
def test_add_bit_exact(ops, rows, C):
    """strided views, and the in-place form out = a that TransRefNet.forward uses; rows C = 1, 259, 1500 (no multiples of 256) and 768"""
    a, b = torch.randn(rows, C, generator=tb.gen(rows)), 1e3 * torch.randn(rows, C, generator=tb.gen(rows + 1))
    _, av = nan_wide(rows, C, off=1, pad=3)
    _, bv = nan_wide(rows, C, off=3, pad=4)
    wide, out = nan_wide(rows, C, off=2, pad=1)
    av.copy_(a), bv.copy_(b)
    ops.tr_add(av, bv, out)
    torch.cuda.synchronize()
    assert untouched(wide, 2, C) and torch.equal(out.cpu(), a + b)
    awide, av = nan_wide(rows, C, off=1, pad=3)
    av.copy_(a)
    ops.tr_add(av, bv, av)
    torch.cuda.synchronize()
    assert untouched(awide, 1, C) and torch.equal(av.cpu(), a + b)


# ================================================================================================ st_tr_dwconv3x3_gelu
@pytest.mark.parametrize("H,W,C", tb.DW_HWC)
@pytest.mark.parametrize("amp", tb.DW_AMPS)
def test_dwconv_gelu_matrix(ops, H, W, C, amp):
    x, w, b = tb.dw_inputs(H, W, C, amp, 500 + 10 * tb.DW_HWC.index((H, W, C)) + tb.DW_AMPS.index(amp))
    _, xv = nan_wide(H * W, C, off=1, pad=3)
    xv.copy_(x)
    wide, out = nan_wide(H * W, C, off=3, pad=2)
    ops.tr_dwconv3x3_gelu(xv, w.cuda(), b.cuda(), out, H, W)
    torch.cuda.synchronize()
    assert untouched(wide, 3, C)
    ref, E = tb.dw_bound(x, w, b, H, W)
    bars(f"dwconv_{H}x{W}x{C}_a{int(amp)}", out, ref, E, tb.dw_gelu(x, w, b, H, W, torch.float32))


# ================================================================================================ wrapper steps, bit for bit
def framed(rows, cols, dtype=torch.float32, fill=NAN):
    """a dense [rows, cols] slice between two guard rows -> (frame, view)"""
    frame = torch.full((rows + 2, cols), fill, device="cuda", dtype=dtype)
    return frame, frame[1:-1]


def guards_intact(frame, fill=NAN):
    g = torch.stack([frame[0], frame[-1]])
    return bool(torch.isnan(g).all()) if fill != fill else bool((g == fill).all())


@pytest.mark.parametrize("hw", [1, 770])
def test_prep_bit_exact(ops, hw):
    img, ctl = tb.prep_inputs(hw, 3)
    frame, out6 = framed(6, hw)
    ops.tr_prep(img.cuda(), ctl.cuda(), out6)
    torch.cuda.synchronize()
    assert guards_intact(frame)
    assert torch.equal(out6.cpu(), torch.cat([tb.prep_ref(img), tb.prep_ref(ctl)]))


@pytest.mark.parametrize("n", [30, 4099])
def test_pack_bit_exact(ops, n):
    """the three mask channels are the reference's 1 - mask.byte(): 1 / 0 for a 0 / 1 mask, -1 for 2.0, -254 for 255.0 and 255.9, 1 for 256.0"""
    rs6, mask = torch.randn(6, n, generator=tb.gen(n)), tb.pack_masks(n, n)
    (fx, x6), (fr, ref3), (fd, detail3) = framed(n, 6), framed(n, 3), framed(3, n)
    ops.tr_pack(rs6.cuda(), mask.cuda(), x6, ref3, detail3)
    torch.cuda.synchronize()
    assert guards_intact(fx) and guards_intact(fr) and guards_intact(fd)
    wx6, wref3, wdetail = tb.pack_ref(rs6, mask)
    assert torch.equal(ref3.cpu(), wref3) and torch.equal(detail3.cpu(), wdetail)
    assert torch.equal(x6.cpu()[:, :3], wx6[:, :3])
    assert torch.equal(x6.cpu()[:, 3:], wx6[:, 3:]), (x6.cpu()[:, 3][mask >= 2], wx6[:, 3][mask >= 2])
    assert {-254.0, -1.0, 0.0, 1.0} <= set(wx6[:, 3].tolist())


@pytest.mark.parametrize("n", [1, 1000])
@pytest.mark.parametrize("planes", [1, 3])
def test_blend_bit_exact(ops, n, planes):
    g = tb.gen(10 * n + planes)
    out3, detail3 = torch.randn(n, 3, generator=g), torch.randn(3, n, generator=g)
    mask = torch.cat([torch.rand(planes, n - n // 2, generator=g), 2.0 * torch.randn(planes, n // 2, generator=g)], 1)     # half inside [0, 1], half outside
    frame, fake = framed(3, n)
    ops.tr_blend(out3.cuda(), detail3.cuda(), mask.cuda(), fake)
    torch.cuda.synchronize()
    assert guards_intact(frame) and torch.equal(fake.cpu(), tb.blend_ref(out3, detail3, mask))


@pytest.mark.parametrize("planes", [2, 4])
def test_blend_rejects_other_plane_counts(ops, planes):
    n = 100
    frame, fake = framed(3, n)
    with pytest.raises(ops.StitchErrorBase):
        ops.tr_blend(torch.zeros(n, 3, device="cuda"), torch.zeros(3, n, device="cuda"), torch.zeros(planes, n, device="cuda"), fake)
    torch.cuda.synchronize()
    assert bool(torch.isnan(frame).all())


def test_to_u8_bit_exact(ops):
    x = tb.to_u8_inputs()
    frame, out = framed(1, x.numel(), dtype=torch.uint8, fill=77)
    ops.tr_to_u8(x.cuda()[None], out)
    torch.cuda.synchronize()
    assert guards_intact(frame, 77) and x.numel() % 256
    assert torch.equal(out.cpu()[0], tb.to_u8_ref(x))


# ================================================================================================ Inpainter.prepare / finish without the network
@pytest.fixture(scope="module")
def inp():
    from stitch_amd import transref as tr
    return tr.Inpainter(seed=0, device="cuda", graph=False)


@pytest.mark.parametrize("H,W", tb.ORIGINS)
def test_prepare_and_finish(inp, H, W):
    n = tb.SIZE * tb.SIZE
    init, mask, ctl = tb.wrapper_inputs(H, W, 60 + H)
    x6, ref3, detail3, mrs, hw = inp.prepare(init.cuda(), mask.cuda(), ctl.cuda())
    torch.cuda.synchronize()
    assert hw == (H, W) and x6.shape == (n, 6) and ref3.shape == (n, 3) and detail3.shape == (3, n) and mrs.shape == (3, tb.SIZE, tb.SIZE)
    planes6, _, hole, ref, E = tb.prepare_ref(init, mask, ctl)
    x6c, ref3c = x6.cpu(), ref3.cpu()
    # the hole set: where the mask channels are not 1 -- exactly the reference's byte; the channels themselves 1 - byte
    assert torch.equal((x6c[:, 3:] != 1).any(1).view(tb.SIZE, tb.SIZE), hole), int(((x6c[:, 3] != 1).view(tb.SIZE, tb.SIZE) != hole).sum())
    assert torch.equal(x6c[:, 3:], (1 - hole.float()).reshape(n, 1).expand(n, 3))
    hf = hole.reshape(n)
    for c in range(3):
        assert bool((x6c[hf, c] == torch.tensor(tb.FILL[c], dtype=torch.float32)).all())
    assert torch.equal(detail3.cpu(), x6c[:, :3].t())
    # the other channels: the resize of the prep planes, inside tests/_geom_bounds.resize_bound
    keep = ~hf
    got = torch.cat([x6c[:, :3][keep].t().reshape(-1), ref3c.t().reshape(-1)])
    pick = lambda t: torch.cat([t[:3].reshape(3, n)[:, keep].reshape(-1), t[3:].reshape(-1)])       # noqa: E731
    o32 = F.interpolate(planes6[None], size=[tb.SIZE, tb.SIZE], mode="bilinear")[0]
    bars(f"prepare_{H}x{W}", got, pick(ref), pick(E), pick(o32))
    if (H, W) == (tb.SIZE, tb.SIZE):                          # the identity resize, bit for bit
        assert torch.equal(got, pick(planes6)) and torch.equal(mrs.cpu(), mask[0])
    # finish on a seeded network output: bytes within 1 of torch-CPU fp32, every differing byte next to a .5 boundary in fp64
    g = tb.gen(70 + H)
    out3 = torch.rand(n, 3, generator=g) * 2.2 - 1.1
    u8 = inp.finish(out3.cuda(), detail3, mrs, hw)
    torch.cuda.synchronize()
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (1, 3, H, W)
    want, pre64, tol = tb.finish_ref(out3, detail3.cpu(), mrs.cpu(), hw)
    d = (u8[0].cpu().int() - want.int()).abs()
    diff = d != 0
    dist = (pre64 - torch.floor(pre64) - 0.5).abs()
    worst = (dist[diff] / tol[diff]).max().item() if bool(diff.any()) else 0.0
    check(f"tr_finish_{H}x{W}_differing_bytes", int(diff.sum()), float("inf"), inclusive=True, note=f"of {d.numel()} bytes; recorded")
    check(f"tr_finish_{H}x{W}_max_byte_difference", int(d.max()), 1, inclusive=True, note="against torch CPU fp32")
    check(f"tr_finish_{H}x{W}_half_distance_over_tol", worst, 1.0, inclusive=True,
          note="fp64 pre-round value of every differing byte within 127.5 E_resize of a .5 boundary")
    if (H, W) == (tb.SIZE, tb.SIZE):
        assert not bool(diff.any())
