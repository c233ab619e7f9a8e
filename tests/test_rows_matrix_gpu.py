"""The five persistent C = 128 row kernels (csrc/gemm_rows.hip, csrc/mlp_split3.h) and their three weight-image pack kernels over rounds, ring
residues, grid choices, operator forms, LayerNorm edge rows, non-finite rows, aliases and rejected arguments.  References, bounds and case lists:
tests/_rows_bounds.py; that the case lists reach every round / residue / grid situation is shown by the grid replay of
tests/test_rows_bounds_cpu.py.

Every output is a column slice (first column 4, row stride N + 8) of a NaN-filled buffer whose frame must still be NaN afterwards; inputs are column
slices of NaN-filled buffers wherever the entry takes a row stride.  The bars of a case:

(a) accuracy       |out - ref| <= E elementwise, ref and E in fp64 from the operator's definition (_rows_bounds.py), recorded as max(err / E) <= 1
(b) bit identity   to the unfused path where include/stitch_gfx950.h promises it: st_linear_chain128 == its layers as st_conv_gemm launches;
                   st_mlp128 with hidden <= 256 == fc1 and fc2 as st_conv_gemm launches; st_mlp128 with the projection == projection launch +
                   st_mlp128 without it
(c) block position rows [r0, M) of a multi-round launch == a launch over those rows alone, r0 in the second round and not a multiple of 32: the rows
                   move to the first round, another block and another lane.  No tolerance: a ring-phase or round-boundary fault cannot pass
(d) rerun          a second launch into the same buffers gives the same bits

ROUND is the number of rows the capped grid covers at once: 65 536 for st_linear_chain128, st_mlp128 and st_rowlin128_split3 (512 workgroups),
32 768 for st_mlp128_split3 and st_pe_tail_split3 (256).  Multi-round cases keep to hidden <= 192 and N <= 128.  The fp64 references run on the
GPU (torch fp64), tiling-free."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import _rows_bounds as rb  # noqa: E402
from _measure import check  # noqa: E402

NAN = float("nan")
RA, RB = rb.ROUND_A, rb.ROUND_B
EINVAL = 1001


@pytest.fixture(scope="module")
def ops():
    import stitch_amd
    assert torch.cuda.is_available()
    return stitch_amd.ops


@pytest.fixture(scope="module")
def lib():
    from stitch_amd import _lib
    return _lib


def dev(t):
    return None if t is None else t.cuda().contiguous()


def devd(d):
    return {k: dev(v) for k, v in d.items()}


def nan_wide(M, N, off=4, pad=4):
    wide = torch.full((M, N + off + pad), NAN, device="cuda")
    return wide, wide[:, off:off + N]


def in_wide(t, off=4, pad=4):
    """t as a column slice of a NaN-filled wider buffer"""
    wide, v = nan_wide(t.shape[0], t.shape[1], off, pad)
    v.copy_(t)
    return v


def untouched(wide, N, off=4):
    return bool(torch.isnan(wide[:, :off]).all()) and bool(torch.isnan(wide[:, off + N:]).all())


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def run(name, launch, M, N, ref=None, E=None):
    """launch(out) into a NaN-framed slice: frame, bar (a) if ref is given, bar (d) -> (out, err / E)"""
    wide, out = nan_wide(M, N)
    launch(out)
    torch.cuda.synchronize()
    assert untouched(wide, N), f"{name}: a write outside the [M, N] view"
    r = 0.0
    if ref is not None:
        r = rb.ratio(out, ref, E)
        assert r <= 1.0, f"{name}: max(err / E) = {r:.4g}"
    first = out.clone()
    launch(out)
    torch.cuda.synchronize()
    assert same(out, first) and untouched(wide, N), f"{name}: a second launch into the same buffers differs"
    return first, r


def r0_of(R, div=1):
    """first row of bar (c): in the second round, a multiple of div, not a multiple of 32"""
    r0 = -(-(R + 1) // div) * div
    while r0 % 32 == 0:
        r0 += div
    return r0


# ------------------------------------------------------------------------------------------------ st_linear_chain128
def chain_dev(layers):
    out = []
    for y in layers:
        y = dict(y)
        y["w"], y["bias"] = dev(y["w"]), dev(y.get("bias"))
        if y.get("res") is not None and not isinstance(y["res"], int):
            y["res"] = in_wide(dev(y["res"]))                       # ld_res = 136
        out.append(y)
    return out


def chain_rows(layers, r0):
    return [{**y, "res": y["res"][r0:]} if y.get("res") is not None and not isinstance(y["res"], int) else y for y in layers]


def pad_rows(t, M):
    """st_conv_gemm hands M <= 8 to skinny_gemm_kernel, which sums k in another order and is outside the promise: the unfused path of such a case runs
    on 16 rows (zero rows behind the M given ones) and its first M rows are compared"""
    return t if t is None or M > 8 else torch.cat([t, torch.zeros(16 - M, t.shape[1], device="cuda")])


def chain_unfused(ops, a, layers):
    """the layers one by one: st_conv_gemm (LayerNorm of its A rows, bias, activation), the residual added by torch (one IEEE fp32 add, as in the kernel)"""
    M = a.shape[0]
    if M <= 8:
        layers = [{**y, "res": pad_rows(y["res"], M)} if y.get("res") is not None and not isinstance(y["res"], int) else y for y in layers]
        return chain_unfused(ops, pad_rows(a, M), layers)[:M]
    x, inputs = a, []
    for y in layers:
        inputs.append(x)
        h = torch.empty(a.shape[0], 128, device="cuda")
        ops.conv_gemm(x, y["w"], h, bias=y.get("bias"), act=y.get("act", "none"), ln_eps=y.get("ln_eps"))
        r = y.get("res")
        if r is not None:
            h = h + (inputs[r] if isinstance(r, int) else r)
        x = h
    return x


def chain_case(ops, form, M, seed):
    layers = chain_dev(rb.chain_layers(form, M, seed))
    a = in_wide(dev(rb.rows(M, seed + 9)))
    ref, E = rb.chain_bound(a, layers)
    name = f"chain_{form}_{M}"
    out, r = run(name, lambda o: ops.linear_chain128(a, o, layers), M, 128, ref, E)
    assert same(out, chain_unfused(ops, a, layers)), f"{name}: differs from the unfused st_conv_gemm launches"
    if M > RA:
        r0 = r0_of(RA)
        part, _ = run(name + "_part", lambda o: ops.linear_chain128(a[r0:], o, chain_rows(layers, r0)), M - r0, 128)
        assert same(part, out[r0:]), f"{name}: rows {r0}.. depend on their block position"
    return r, a, layers, out


@pytest.mark.parametrize("form", rb.CHAIN_FORMS)
def test_chain_forms(ops, form):
    rs = [chain_case(ops, form, M, 1000)[0] for M in rb.CHAIN_ROWS + ((2 * RA + 1,) if form in rb.CHAIN_MODEL_FORMS else ())]
    check(f"rows_chain_{form}_err_over_E", max(rs), 1.0, inclusive=True, note="|out - ref| <= E elementwise (_rows_bounds.py)")


@pytest.mark.parametrize("M", rb.SMALL_ROWS + (RA,))
def test_chain_row_counts(ops, M):
    rs = [chain_case(ops, form, M, 1100)[0] for form in rb.CHAIN_MODEL_FORMS]
    check(f"rows_chain_model_{M}_err_over_E", max(rs), 1.0, inclusive=True)


@pytest.mark.parametrize("M", rb.CHAIN_ROWS)
def test_chain_aliases(ops, M):
    """in place (a == out: a wave reads its block's rows before it writes them) and res_ptr == a, against the out-of-place result"""
    for form in ("model_self", "ln012"):
        _, a, layers, out = chain_case(ops, form, M, 1200)
        wide, io = nan_wide(M, 128)
        io.copy_(a)
        ops.linear_chain128(io, io, layers)
        torch.cuda.synchronize()
        assert same(io, out) and untouched(wide, 128), (form, M)
    a = in_wide(dev(rb.rows(M, 1201)))
    layers = chain_dev(rb.chain_layers("n2", M, 1202))
    layers[1]["res"] = a                                            # the same rows as a tensor residual ...
    want, _ = run(f"chain_res_is_a_{M}", lambda o: ops.linear_chain128(a, o, layers), M, 128, *rb.chain_bound(a, layers))
    layers[1]["res"] = 0                                            # ... equal the saved input of layer 0
    got, _ = run(f"chain_res_l0_{M}", lambda o: ops.linear_chain128(a, o, layers), M, 128)
    assert same(got, want)
    layers[1]["res"] = a
    wide, io = nan_wide(M, 128)
    io.copy_(a)
    layers[1]["res"] = io                                           # in place AND the residual the rows being overwritten
    ops.linear_chain128(io, io, layers)
    torch.cuda.synchronize()
    assert same(io, want)


# ------------------------------------------------------------------------------------------------ st_mlp128 / st_mlp128_split3
class Mlp:
    """one weight set on the device, its split3 images packed once"""

    def __init__(self, ops, M, hidden, seed, edge=False):
        self.ops, self.M, self.hidden = ops, M, hidden
        self.d = devd(rb.mlp_inputs(M, hidden, seed, edge))
        d = self.d
        self.a, self.res, self.res0 = in_wide(d["a"]), in_wide(d["res"]), in_wide(d["res0"])
        self.img = {}

    def image(self, proj):
        d = self.d
        if proj not in self.img:
            self.img[proj] = self.ops.mlp128_split3_pack(d["w1"], d["b1"], d["w2"], proj=None if proj == "none" else (d["wp"], d["bp"] if proj == "full" else None))
        return self.img[proj]

    def proj(self, proj, rows=slice(None)):
        d = self.d
        return dict(none=None, full=(d["wp"], d["bp"], self.res0[rows]), bare=(d["wp"], None, None))[proj]

    def launch(self, out, split3, proj, ln, res, rows=slice(None), res_t=None):
        d = self.d
        res_t = res_t if res_t is not None else (self.res[rows] if res else None)
        self.ops.mlp128(self.a[rows], out, d["w1"], d["b1"], d["w2"], d["b2"], ln_eps=1e-5 if ln else None, res=res_t, proj=self.proj(proj, rows),
                        image=self.image(proj) if split3 else None)

    def bound(self, split3, proj, ln, res):
        d = self.d
        return rb.mlp_bound(self.a, d["w1"], d["b1"], d["w2"], d["b2"], ln_eps=1e-5 if ln else None, res=self.res if res else None, proj=self.proj(proj),
                            split3=split3)

    def unfused(self, proj, ln, res):
        """bar (b): with the projection, projection launch + st_mlp128; without it and hidden <= 256, fc1 and fc2 as st_conv_gemm launches"""
        d, ops, M0 = self.d, self.ops, self.M
        a, rs = pad_rows(self.a, M0), pad_rows(self.res, M0)
        M = a.shape[0]
        out = torch.empty(M, 128, device="cuda")
        if proj != "none":
            x = torch.empty(M, 128, device="cuda")
            wp, bp, res0 = self.proj(proj)
            ops.conv_gemm(a, wp, x, bias=bp, aux0=pad_rows(res0, M0))
            return ops.mlp128(x, out, d["w1"], d["b1"], d["w2"], d["b2"], ln_eps=1e-5 if ln else None, res=rs if res else None)[:M0]
        if self.hidden > 256:
            return None
        h = torch.empty(M, self.hidden, device="cuda")
        ops.conv_gemm(a, d["w1"], h, bias=d["b1"], act="gelu", ln_eps=1e-5 if ln else None)
        ops.conv_gemm(h, d["w2"], out, bias=d["b2"], aux0=a)
        return (out + rs if res else out)[:M0]

    def case(self, split3, proj, ln, res, part=False):
        name = f"mlp{'_s3' if split3 else ''}_{self.hidden}_{self.M}_{proj}_ln{int(ln)}_res{int(res)}"
        out, r = run(name, lambda o: self.launch(o, split3, proj, ln, res), self.M, 128, *self.bound(split3, proj, ln, res))
        if not split3:
            u = self.unfused(proj, ln, res)
            assert u is None or same(out, u), f"{name}: differs from the unfused launches"
        R = RB if split3 else RA
        if part and self.M > R:
            r0 = r0_of(R)
            p, _ = run(name + "_part", lambda o: self.launch(o, split3, proj, ln, res, slice(r0, None)), self.M - r0, 128)
            assert same(p, out[r0:]), f"{name}: rows {r0}.. depend on their block position"
        return r, out


FORMS4 = ((True, True), (True, False), (False, True), (False, False))


@pytest.mark.parametrize("hidden", rb.MLP_HIDDEN)
@pytest.mark.parametrize("split3", [False, True], ids=["fp32", "split3"])
def test_mlp_small(ops, hidden, split3):
    rs = []
    for M in ((129,) if hidden == 2048 else rb.SMALL_ROWS):
        m = Mlp(ops, M, hidden, 2000 + hidden + M)
        rs += [m.case(split3, proj, ln, res)[0] for proj in rb.MLP_PROJ for ln, res in FORMS4]
    check(f"rows_mlp_{'split3' if split3 else 'fp32'}_{hidden}_small_err_over_E", max(rs), 1.0, inclusive=True)


@pytest.mark.parametrize("hidden,with_proj", rb.MLP_MULTI)
@pytest.mark.parametrize("split3", [False, True], ids=["fp32", "split3"])
def test_mlp_multi_round(ops, hidden, with_proj, split3):
    rs = []
    for M in rb.multi_rows(RB if split3 else RA):
        m = Mlp(ops, M, hidden, 2100 + hidden)
        rs.append(m.case(split3, "full" if with_proj else "none", True, True, part=True)[0])
        del m
    check(f"rows_mlp_{'split3' if split3 else 'fp32'}_{hidden}_p{int(with_proj)}_multi_err_over_E", max(rs), 1.0, inclusive=True)


@pytest.mark.parametrize("split3,proj,M", [(False, "none", 129), (False, "none", RA + 33), (True, "none", 129), (True, "none", RB + 33), (True, "full", 129),
                                           (True, "full", RB + 33)])
def test_mlp_res_is_out(ops, split3, proj, M):
    """res == out: st_mlp128 allows it without the projection (a lane reads its residual values right before it writes the same addresses); the
    split3 kernel keeps x in registers, reads res in the epilogue of its own rows only, and allows it with the projection as well"""
    m = Mlp(ops, M, 128, 2200)
    _, want = m.case(split3, proj, True, True)
    wide, io = nan_wide(M, 128)
    io.copy_(m.res)
    m.launch(io, split3, proj, True, True, res_t=io)
    torch.cuda.synchronize()
    assert same(io, want) and untouched(wide, 128)


# ------------------------------------------------------------------------------------------------ st_rowlin128_split3
def aux_of(kind, M, N, seed):
    """-> (table view, row_div)"""
    if kind == "none":
        return None, 1
    div = dict(div1=1, div8=8, div7_ld=7)[kind]
    t = dev(rb.table(-(-M // div), seed, N))
    return (in_wide(t, 0, 4) if kind == "div7_ld" else t), div


def rowlin_case(ops, M, N, ln, bias, aux_kind, seed, edge=False, part=False):
    d = devd(rb.rowlin_inputs(M, N, seed, edge))
    a, b = in_wide(d["a"]), d["b"] if bias else None
    img = ops.rowlin128_split3_pack(d["w"], b)
    aux, div = aux_of(aux_kind, M, N, seed + 3)
    eps = 1e-5 if ln else None
    name = f"rowlin_{M}_{N}_ln{int(ln)}_b{int(bias)}_{aux_kind}"
    out, r = run(name, lambda o: ops.rowlin128_split3(a, o, img, ln_eps=eps, aux=aux, row_div=div), M, N, *rb.rowlin_bound(a, d["w"], b, eps, aux, div))
    if part and M > RA:
        r0 = r0_of(RA, div)
        p, _ = run(name + "_part", lambda o: ops.rowlin128_split3(a[r0:], o, img, ln_eps=eps, aux=None if aux is None else aux[r0 // div:], row_div=div), M - r0, N)
        assert same(p, out[r0:]), f"{name}: rows {r0}.. depend on their block position"
    return r, out


@pytest.mark.parametrize("N", rb.ROWLIN_N)
def test_rowlin_small(ops, N):
    rs = [rowlin_case(ops, M, N, ln, bias, aux, 3000 + N)[0] for M in ((129,) if N == 4096 else rb.SMALL_ROWS) for ln in (True, False)
          for bias in (True, False) for aux in rb.ROWLIN_AUX]
    check(f"rows_rowlin_{N}_small_err_over_E", max(rs), 1.0, inclusive=True)


@pytest.mark.parametrize("N", rb.ROWLIN_MULTI_N)
def test_rowlin_multi_round(ops, N):
    """with aux at ROUND + 33 the padding lanes of the one-row block read table row (M - 1) // row_div, the last one the table has"""
    rs = [rowlin_case(ops, M, N, True, True, aux, 3100 + N, part=True)[0]
          for M, aux in ((RA, "none"), (RA + 33, "div8"), (RA + 33, "div7_ld"), (RA + 33, "none"), (2 * RA + 1, "div8"))]
    check(f"rows_rowlin_{N}_multi_err_over_E", max(rs), 1.0, inclusive=True)


# ------------------------------------------------------------------------------------------------ st_pe_tail_split3
def pe_launch(ops, d, x, tab, img, out):
    ops.pe_tail_split3(x, tab, img, d["b2"], d["gamma"], d["beta"], out)


def pe_run(name, launch, R, ref=None, E=None):
    """the entry takes dense [R, 128] rows: the frame is a NaN row on either side"""
    buf = torch.full((R + 2, 128), NAN, device="cuda")
    out = buf[1:R + 1]
    r = 0.0
    for i in range(2):
        launch(out)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[R + 1]).all()), f"{name}: a write outside the [R, 128] rows"
        if i == 0:
            first = out.clone()
            if ref is not None:
                r = rb.ratio(out, ref, E)
                assert r <= 1.0, f"{name}: max(err / E) = {r:.4g}"
    assert same(out, first), f"{name}: a second launch into the same buffers differs"
    return first, r


def pe_case(ops, R, P, ld1, seed, edge=False):
    d = devd(rb.pe_inputs(R, P, seed, edge))
    w1 = d["w1"] if ld1 == 128 else d["w1"][:, :64].contiguous()
    img = ops.pe_tail_split3_pack(w1[:, :64] if ld1 == 128 else w1, d["w2"])
    name = f"pe_{R}_{P}_ld{ld1}"
    ref, E = rb.pe_tail_bound(d["x"], d["w1"][:, :64], d["tab"], d["w2"], d["b2"], d["gamma"], d["beta"])
    out, r = pe_run(name, lambda o: pe_launch(ops, d, d["x"], d["tab"], img, o), R, ref, E)
    nblk = -(-R // 32)
    G = min(-(-nblk // 4), 256)
    if nblk > 4 * G or (R, P) == (600, 3):
        # bar (c): rows of a wave's second block as a launch of their own, the table rotated so that its row 0 is row r0's
        r0 = 389 if R == 600 else RB + 5
        tab = torch.roll(d["tab"], -(r0 % P), 0).contiguous()
        part, _ = pe_run(name + "_part", lambda o: pe_launch(ops, d, d["x"][r0:].contiguous(), tab, img, o), R - r0)
        assert same(part, out[r0:]), f"{name}: rows {r0}.. depend on their block position"
    return r


@pytest.mark.parametrize("R,P", rb.PE_CASES)
def test_pe_tail(ops, R, P):
    rs = [pe_case(ops, R, P, ld1, 4000 + P) for ld1 in ((128, 64) if R <= 600 else (128,))]
    check(f"rows_pe_tail_{R}_{P}_err_over_E", max(rs), 1.0, inclusive=True)


# ------------------------------------------------------------------------------------------------ pack kernels
def test_pack_leaves_the_surplus_alone(ops, lib):
    """each image packed into a larger buffer: the bytes behind the image keep their pattern, the image equals the one packed to size"""
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())                                             # noqa: E731
    d = devd(rb.mlp_inputs(1, 96, 5000))
    w, b = dev(rb.weight(96, 128, 5001)), dev(rb.vec(96, 5002))
    w2o = torch.ones(128, 128, device="cuda")
    jobs = [
        (ops.mlp128_split3_pack(d["w1"], d["b1"], d["w2"]), lambda img, n: lib.lib.st_mlp128_split3_pack(p(d["w1"]), p(d["b1"]), p(d["w2"]), None, None, 96, img, n, st)),
        (ops.mlp128_split3_pack(d["w1"], d["b1"], d["w2"], proj=(d["wp"], d["bp"])),
         lambda img, n: lib.lib.st_mlp128_split3_pack(p(d["w1"]), p(d["b1"]), p(d["w2"]), p(d["wp"]), p(d["bp"]), 96, img, n, st)),
        (ops.rowlin128_split3_pack(w, b), lambda img, n: lib.lib.st_rowlin128_split3_pack(p(w), p(b), 96, img, n, st)),
        (ops.pe_tail_split3_pack(d["wp"], w2o), lambda img, n: lib.lib.st_pe_tail_split3_pack(p(d["wp"]), 128, p(w2o), img, n, st)),
    ]
    for exact, pack in jobs:
        n = exact.numel()
        big = torch.full((n + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
        assert pack(p(big), n + 4096) == 0
        torch.cuda.synchronize()
        assert torch.equal(big[:n], exact) and bool((big[n:] == 0xA5).all())


# ------------------------------------------------------------------------------------------------ LayerNorm edge rows, non-finite rows
def test_layernorm_edge_rows(ops):
    """constant rows (variance 0: rstd = eps^-1/2 amplifies the rounding of the mean), c + 1e-3 n for c = 1 and 100, zero rows, one-hot rows of 1e3 at rows
    0, 31, 32 and M - 1 and their neighbours: bar (a) with the same E, whose variance-zero term is what it rests on there"""
    M, rs = 129, {}
    for form in ("ln0", "ln012", "model_cross", "model_self", "res_self", "res_l0_from_l2"):
        layers = chain_dev(rb.chain_layers(form, M, 6000))
        a = in_wide(dev(rb.edge_rows(M, 6001)))
        out, r = run(f"edge_chain_{form}", lambda o: ops.linear_chain128(a, o, layers), M, 128, *rb.chain_bound(a, layers))
        assert same(out, chain_unfused(ops, a, layers))
        rs["chain"] = max(rs.get("chain", 0.0), r)
    for hidden in (128, 96):
        m = Mlp(ops, M, hidden, 6100, edge=True)
        for split3 in (False, True):
            k = "mlp_split3" if split3 else "mlp_fp32"
            rs[k] = max([rs.get(k, 0.0)] + [m.case(split3, proj, True, res)[0] for proj in rb.MLP_PROJ for res in (True, False)])
    rs["rowlin"] = max(rowlin_case(ops, M, N, True, True, aux, 6200, edge=True)[0] for N in (32, 128) for aux in ("none", "div8"))
    rs["pe_tail"] = pe_case(ops, M, 64, 128, 6300, edge=True)
    # a constant row into pe_tail's closing LayerNorm: w2 = 0 leaves b2 alone, and a constant b2 has variance 0
    d = devd(rb.pe_inputs(M, 5, 6301))
    d["w2"], d["b2"] = torch.zeros(128, 128, device="cuda"), torch.full((128,), 0.7, device="cuda")
    img = ops.pe_tail_split3_pack(d["w1"], d["w2"])
    ref, E = rb.pe_tail_bound(d["x"], d["w1"][:, :64], d["tab"], d["w2"], d["b2"], d["gamma"], d["beta"])
    rs["pe_tail_const"] = pe_run("edge_pe_const", lambda o: pe_launch(ops, d, d["x"], d["tab"], img, o), M, ref, E)[1]
    for k, v in rs.items():
        check(f"rows_edge_{k}_err_over_E", v, 1.0, inclusive=True)


def poison(x):
    x = x.clone()
    x[5] = NAN
    x[40, 7] = float("inf")
    x[x.shape[0] - 1] = NAN
    return x


BAD = (5, 40, 128)


def contained(name, clean, dirty, nonfinite=True):
    keep = torch.ones(clean.shape[0], dtype=torch.bool, device="cuda")
    keep[list(BAD)] = False
    assert same(dirty[keep], clean[keep]), f"{name}: a non-finite row reached another row"
    if nonfinite:
        assert not bool(torch.isfinite(dirty[~keep]).any()), f"{name}: a non-finite row came out finite"


def test_nonfinite_rows_stay_in_their_row(ops):
    """row 5 NaN, +inf in one column of row 40, row M - 1 (the clamp source of the padding lanes of the last block) NaN, M = 129: every other row keeps
    the bits of the clean run; the three rows come out non-finite (inf or NaN from the fp32 kernels, NaN from the split3 kernels).  pe_tail_split3_kernel
    is the exception the header states: its ReLU is v_max_f32, which returns 0 for a NaN, so the hidden layer of such a row is zero and the row leaves
    as LayerNorm(b2) -- finite, the same in all three rows, and still confined to its row."""
    M = 129
    for form in ("model_self", "model_cross", "n1"):
        layers = chain_dev(rb.chain_layers(form, M, 7000))
        a = dev(rb.rows(M, 7001))
        clean, _ = run("nf_chain", lambda o: ops.linear_chain128(a, o, layers), M, 128)
        b = poison(a)
        wide, out = nan_wide(M, 128)
        ops.linear_chain128(b, out, layers)
        contained(f"chain_{form}", clean, out)
    for split3 in (False, True):
        for proj, ln in (("none", True), ("full", True), ("none", False)):
            m = Mlp(ops, M, 128, 7100)
            _, clean = m.case(split3, proj, ln, True)
            m.a = in_wide(poison(m.a))
            wide, out = nan_wide(M, 128)
            m.launch(out, split3, proj, ln, True)
            contained(f"mlp_{split3}_{proj}_{ln}", clean, out)
    for ln in (True, False):
        d = devd(rb.rowlin_inputs(M, 64, 7200))
        img = ops.rowlin128_split3_pack(d["w"], d["b"])
        aux, div = aux_of("div8", M, 64, 7201)
        outs = []
        for a in (d["a"], poison(d["a"])):
            wide, out = nan_wide(M, 64)
            ops.rowlin128_split3(a, out, img, ln_eps=1e-5 if ln else None, aux=aux, row_div=div)
            outs.append(out)
        contained(f"rowlin_{ln}", *outs)
    d = devd(rb.pe_inputs(M, 5, 7300))
    img = ops.pe_tail_split3_pack(d["w1"], d["w2"])
    outs = []
    for x in (d["x"], poison(d["x"])):
        out = torch.full((M, 128), NAN, device="cuda")
        pe_launch(ops, d, x, d["tab"], img, out)
        outs.append(out)
    torch.cuda.synchronize()
    contained("pe_tail", *outs, nonfinite=False)
    rows = outs[1][list(BAD)]
    assert same(rows[0], rows[1]) and same(rows[0], rows[2])
    z = torch.zeros(1, 128, dtype=torch.float64, device="cuda")
    ref, E = rb.ln(d["b2"].double()[None], z, 1e-5, rb.LN_NS, rb.LN_NV_PE, d["gamma"], d["beta"])
    check("rows_pe_tail_relu_of_nan_row_err_over_E", rb.ratio(rows[:1], ref, E), 1.0, inclusive=True, note="ReLU(NaN) = 0: the row leaves as LayerNorm(b2)")


# ------------------------------------------------------------------------------------------------ rejections
def rejected(name, call, out):
    before = out.clone()
    rc = call()
    torch.cuda.synchronize()
    assert rc == EINVAL, f"{name}: returned {rc}"
    assert same(out, before), f"{name}: the output changed"


def test_chain_rejections(ops, lib):
    M = 64
    a, out, res = (torch.full((M, 136), 1.0, device="cuda") for _ in range(3))
    w, b = dev(rb.weight(128, 128, 8000)), dev(rb.vec(132, 8001))

    def desc(**kw):
        d = lib.ChainDesc()
        d.a, d.out, d.lda, d.ldo, d.M, d.nlayers = a.data_ptr(), out.data_ptr(), 136, 136, M, 3
        for l in range(3):
            d.layer[l].w, d.layer[l].bias = w.data_ptr(), b.data_ptr()
        for k, v in kw.items():
            if k[0] == "l" and k[1].isdigit():
                setattr(d.layer[int(k[1])], k[3:], v)
            else:
                setattr(d, k, v)
        return d

    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.lib.st_linear_chain128(C.byref(desc()), st) == 0
    torch.cuda.synchronize()
    out.fill_(1.0)
    cases = dict(
        a_null=dict(a=None), out_null=dict(out=None), m_zero=dict(M=0), no_layers=dict(nlayers=0), four_layers=dict(nlayers=4), lda_short=dict(lda=124),
        ldo_short=dict(ldo=124), lda_odd=dict(lda=138), ldo_odd=dict(ldo=138), a_misaligned=dict(a=a.data_ptr() + 4), out_misaligned=dict(out=out.data_ptr() + 8),
        w_null=dict(l1_w=None), w_misaligned=dict(l0_w=w.data_ptr() + 4), act_sigmoid=dict(l2_act=3), act_negative=dict(l0_act=-1), res_3=dict(l0_res=3),
        res_negative=dict(l1_res=-1), res_ptr_null=dict(l1_res=1), res_ld_short=dict(l1_res=1, l1_res_ptr=res.data_ptr(), l1_ld_res=64),
        res_ld_odd=dict(l1_res=1, l1_res_ptr=res.data_ptr(), l1_ld_res=130), res_misaligned=dict(l1_res=1, l1_res_ptr=res.data_ptr() + 4, l1_ld_res=136),
        res_layer_after=dict(l1_res=2, l1_res_layer=2), res_layer_negative=dict(l1_res=2, l1_res_layer=-1), bias_misaligned=dict(l2_bias=b.data_ptr() + 4),
        two_saved_layers=dict(l1_res=2, l1_res_layer=0, l2_res=2, l2_res_layer=1),
    )
    for name, kw in cases.items():
        rejected("chain_" + name, lambda: lib.lib.st_linear_chain128(C.byref(desc(**kw)), st), out)
    rejected("chain_desc_null", lambda: lib.lib.st_linear_chain128(None, st), out)


@pytest.mark.parametrize("split3", [False, True], ids=["fp32", "split3"])
def test_mlp_rejections(ops, lib, split3):
    M, hidden = 64, 64
    a, out, res, res0 = (torch.full((M, 136), 1.0, device="cuda") for _ in range(4))
    d0 = devd(rb.mlp_inputs(1, hidden, 8100))
    img, imgp = ops.mlp128_split3_pack(d0["w1"], d0["b1"], d0["w2"]), ops.mlp128_split3_pack(d0["w1"], d0["b1"], d0["w2"], proj=(d0["wp"], d0["bp"]))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(image=None, image_bytes=None, **kw):
        d = lib.MlpDesc()
        d.a, d.out, d.lda, d.ldo, d.M, d.hidden = a.data_ptr(), out.data_ptr(), 136, 136, M, hidden
        d.w1, d.b1, d.w2, d.b2 = (d0[k].data_ptr() for k in ("w1", "b1", "w2", "b2"))
        for k, v in kw.items():
            setattr(d, k, v)
        if not split3:
            return lib.lib.st_mlp128(C.byref(d), st)
        im = image if image is not None else (imgp if d.wp else img)
        return lib.lib.st_mlp128_split3(C.byref(d), C.c_void_p(im.data_ptr() if hasattr(im, "data_ptr") else im), im.numel() if image_bytes is None else image_bytes, st)

    assert call() == 0 and call(wp=d0["wp"].data_ptr(), bp=d0["bp"].data_ptr(), res0=res0.data_ptr(), ld_res0=136, res=res.data_ptr(), ld_res=136) == 0
    torch.cuda.synchronize()
    out.fill_(1.0)
    wp = d0["wp"].data_ptr()
    cases = dict(
        a_null=dict(a=None), out_null=dict(out=None), b2_null=dict(b2=None), m_zero=dict(M=0), hidden_16=dict(hidden=16), hidden_2080=dict(hidden=2080),
        hidden_48=dict(hidden=48), lda_short=dict(lda=124), ldo_short=dict(ldo=124), lda_odd=dict(lda=138), ldo_odd=dict(ldo=138), reserved=dict(reserved=1),
        a_misaligned=dict(a=a.data_ptr() + 4), out_misaligned=dict(out=out.data_ptr() + 8), b2_misaligned=dict(b2=d0["b2"].data_ptr() + 4),
        res_ld_short=dict(res=res.data_ptr(), ld_res=64), res_ld_odd=dict(res=res.data_ptr(), ld_res=130), res_misaligned=dict(res=res.data_ptr() + 4, ld_res=136),
        in_place=dict(a=out.data_ptr()), bp_without_wp=dict(bp=d0["bp"].data_ptr()), res0_without_wp=dict(res0=res0.data_ptr(), ld_res0=136),
        res0_ld_short=dict(wp=wp, res0=res0.data_ptr(), ld_res0=64), res0_ld_odd=dict(wp=wp, res0=res0.data_ptr(), ld_res0=130),
        res0_misaligned=dict(wp=wp, res0=res0.data_ptr() + 4, ld_res0=136), res0_is_out=dict(wp=wp, res0=out.data_ptr(), ld_res0=136),
    )
    if split3:
        cases.update(image_short=dict(image_bytes=img.numel() - 1), image_without_proj=dict(wp=wp, image=img), image_misaligned=dict(image=imgp[4:], image_bytes=img.numel()))
    else:
        cases.update(w1_null=dict(w1=None), b1_null=dict(b1=None), w2_null=dict(w2=None), w1_misaligned=dict(w1=d0["w1"].data_ptr() + 4),
                     b1_misaligned=dict(b1=d0["b1"].data_ptr() + 4), w2_misaligned=dict(w2=d0["w2"].data_ptr() + 4), wp_misaligned=dict(wp=wp + 4),
                     bp_misaligned=dict(wp=wp, bp=d0["bp"].data_ptr() + 4), res_is_out_with_proj=dict(wp=wp, res=out.data_ptr(), ld_res=136))
    for name, kw in cases.items():
        rejected(f"mlp_{split3}_{name}", lambda: call(**kw), out)
    fn = lib.lib.st_mlp128_split3 if split3 else lib.lib.st_mlp128
    rejected("mlp_desc_null", (lambda: fn(None, C.c_void_p(img.data_ptr()), img.numel(), st)) if split3 else (lambda: fn(None, st)), out)
    if split3:
        nb = C.c_int64(0)
        assert lib.lib.st_mlp128_split3_image_bytes(48, 0, C.byref(nb)) == EINVAL and lib.lib.st_mlp128_split3_image_bytes(64, 0, None) == EINVAL
        p = lambda t: C.c_void_p(t.data_ptr())                                        # noqa: E731
        for name, args in dict(w1_null=(None, p(d0["b1"]), p(d0["w2"]), None, None, hidden, p(img), img.numel()),
                               hidden_48=(p(d0["w1"]), p(d0["b1"]), p(d0["w2"]), None, None, 48, p(img), img.numel()),
                               bp_without_wp=(p(d0["w1"]), p(d0["b1"]), p(d0["w2"]), None, p(d0["bp"]), hidden, p(img), img.numel()),
                               image_short=(p(d0["w1"]), p(d0["b1"]), p(d0["w2"]), p(d0["wp"]), None, hidden, p(img), img.numel()),
                               image_misaligned=(p(d0["w1"]), p(d0["b1"]), p(d0["w2"]), None, None, hidden, p(imgp[4:]), img.numel())).items():
            rejected("mlp_pack_" + name, lambda: lib.lib.st_mlp128_split3_pack(*args, st), img)


def test_rowlin_rejections(ops, lib):
    M, N = 64, 64
    a, out = torch.full((M, 136), 1.0, device="cuda"), torch.full((M, N + 8), 1.0, device="cuda")
    aux = torch.full((M, N + 8), 1.0, device="cuda")
    w, b = dev(rb.weight(N, 128, 8200)), dev(rb.vec(N, 8201))
    img = ops.rowlin128_split3_pack(w, b)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    base = dict(a=a.data_ptr(), lda=136, out=out.data_ptr(), ldo=N + 8, M=M, N=N, ln=1, eps=1e-5, image=img.data_ptr(), image_bytes=img.numel(), aux=None, ld_aux=0,
                row_div=1)
    withaux = dict(aux=aux.data_ptr(), ld_aux=N + 8, row_div=8)

    def call(**kw):
        v = {**base, **kw}
        return lib.lib.st_rowlin128_split3(C.c_void_p(v["a"]), v["lda"], C.c_void_p(v["out"]), v["ldo"], v["M"], v["N"], v["ln"], v["eps"], C.c_void_p(v["image"]),
                                           v["image_bytes"], C.c_void_p(v["aux"]), v["ld_aux"], v["row_div"], st)

    assert call() == 0 and call(**withaux) == 0
    torch.cuda.synchronize()
    out.fill_(1.0)
    cases = dict(
        a_null=dict(a=None), out_null=dict(out=None), image_null=dict(image=None), m_zero=dict(M=0), n_16=dict(N=16), n_4128=dict(N=4128), n_48=dict(N=48),
        lda_short=dict(lda=124), ldo_short=dict(ldo=N - 4), lda_odd=dict(lda=138), ldo_odd=dict(ldo=N + 6), in_place=dict(out=a.data_ptr(), ldo=136),
        a_misaligned=dict(a=a.data_ptr() + 4), out_misaligned=dict(out=out.data_ptr() + 8), image_misaligned=dict(image=img.data_ptr() + 4),
        image_short=dict(image_bytes=img.numel() - 1),
        aux_ld_short=dict(withaux, ld_aux=N - 4), aux_ld_odd=dict(withaux, ld_aux=N + 6), aux_row_div_zero=dict(withaux, row_div=0),
        aux_misaligned=dict(withaux, aux=aux.data_ptr() + 4), aux_is_out=dict(withaux, aux=out.data_ptr()),
    )
    for name, kw in cases.items():
        rejected("rowlin_" + name, lambda: call(**kw), out)
    big = torch.full((M, 136), 1.0, device="cuda")
    rejected("rowlin_image_for_fewer_features", lambda: call(N=128, out=big.data_ptr(), ldo=136), big)
    nb = C.c_int64(0)
    assert lib.lib.st_rowlin128_split3_image_bytes(48, C.byref(nb)) == EINVAL and lib.lib.st_rowlin128_split3_image_bytes(64, None) == EINVAL
    p = lambda t: C.c_void_p(t.data_ptr())                                            # noqa: E731
    for name, args in dict(w_null=(None, p(b), N, p(img), img.numel()), n_48=(p(w), p(b), 48, p(img), img.numel()), image_null=(p(w), p(b), N, None, img.numel()),
                           image_misaligned=(p(w), p(b), N, p(img[4:]), img.numel()), image_short=(p(w), p(b), N, p(img), img.numel() - 1)).items():
        rejected("rowlin_pack_" + name, lambda: lib.lib.st_rowlin128_split3_pack(*args, st), img)


def test_pe_tail_rejections(ops, lib):
    R, P = 64, 5
    d = devd(rb.pe_inputs(R, P, 8300))
    img = ops.pe_tail_split3_pack(d["w1"], d["w2"])
    out = torch.full((R, 128), 1.0, device="cuda")
    xbig = torch.full((R, 128), 1.0, device="cuda")                 # (an x buffer large enough to stand in as `out` for the alias case)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    base = dict(x=d["x"].data_ptr(), tab=d["tab"].data_ptr(), P=P, image=img.data_ptr(), image_bytes=img.numel(), b2=d["b2"].data_ptr(), gamma=d["gamma"].data_ptr(),
                beta=d["beta"].data_ptr(), out=out.data_ptr(), R=R)

    def call(**kw):
        v = {**base, **kw}
        return lib.lib.st_pe_tail_split3(C.c_void_p(v["x"]), C.c_void_p(v["tab"]), v["P"], C.c_void_p(v["image"]), v["image_bytes"], C.c_void_p(v["b2"]),
                                         C.c_void_p(v["gamma"]), C.c_void_p(v["beta"]), 1e-5, C.c_void_p(v["out"]), v["R"], st)

    assert call() == 0
    torch.cuda.synchronize()
    out.fill_(1.0)
    cases = dict(x_null=dict(x=None), tab_null=dict(tab=None), image_null=dict(image=None), b2_null=dict(b2=None), gamma_null=dict(gamma=None), beta_null=dict(beta=None),
                 out_null=dict(out=None), r_zero=dict(R=0), p_zero=dict(P=0), image_short=dict(image_bytes=img.numel() - 1), x_misaligned=dict(x=d["x"].data_ptr() + 4),
                 tab_misaligned=dict(tab=d["tab"].data_ptr() + 4), image_misaligned=dict(image=img.data_ptr() + 4), out_misaligned=dict(out=out.data_ptr() + 8))
    for name, kw in cases.items():
        rejected("pe_" + name, lambda: call(**kw), out)
    rejected("pe_x_is_out", lambda: call(x=xbig.data_ptr(), out=xbig.data_ptr()), xbig)
    assert lib.lib.st_pe_tail_split3_image_bytes(None) == EINVAL
    p = lambda t: C.c_void_p(t.data_ptr())                                            # noqa: E731
    for name, args in dict(w1_null=(None, 128, p(d["w2"]), p(img), img.numel()), w2_null=(p(d["w1"]), 128, None, p(img), img.numel()),
                           ld1_short=(p(d["w1"]), 60, p(d["w2"]), p(img), img.numel()), image_null=(p(d["w1"]), 128, p(d["w2"]), None, img.numel()),
                           image_misaligned=(p(d["w1"]), 128, p(d["w2"]), p(img[4:]), img.numel()), image_short=(p(d["w1"]), 128, p(d["w2"]), p(img), img.numel() - 1)).items():
        rejected("pe_pack_" + name, lambda: lib.lib.st_pe_tail_split3_pack(*args, st), img)
