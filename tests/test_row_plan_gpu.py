"""What the C = 128 row launchers (csrc/gemm_rows.hip) report about themselves: the calling thread's plan (st_gemm_last_plan) after each of
st_linear_chain128, st_mlp128, st_mlp128_split3, st_rowlin128_split3 and st_pe_tail_split3, and the descriptor an installed profiling
observer (st_set_gemm_observer) receives for them -- bench.py's live roofline keys its byte formulas on exactly these values.

Pinned: kernel / tile ids 5/30, 6/31, 9/38, 10/40, 11/41, split 1, persistent 1; the observer sees ONE bracket per launch (phase 0, then
phase 1 with the plan already that of the launch), reported as a GEMM of the family M x N x 128 whose N carries the launch's FLOPs."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


def rnd(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def test_row_launchers_report_plan_and_observer_descriptor():
    import stitch_amd
    ops, lib, GemmDesc = stitch_amd.ops, stitch_amd._lib.lib, stitch_amd._lib.GemmDesc
    assert torch.cuda.is_available()
    M, hidden, N, P = 200, 256, 96, 64
    x, out = rnd((M, 128), 1), torch.empty(M, 128, device="cuda")
    w, b = rnd((128, 128), 2, 128 ** -0.5), rnd((128,), 3, 0.1)
    w1, b1, w2 = rnd((hidden, 128), 4, 128 ** -0.5), rnd((hidden,), 5, 0.1), rnd((128, hidden), 6, hidden ** -0.5)
    wn, bn, outn = rnd((N, 128), 7, 128 ** -0.5), rnd((N,), 8, 0.1), torch.empty(M, N, device="cuda")
    x64, tab = rnd((M, 64), 9), rnd((P, 128), 10, 0.5)
    img_mlp = ops.mlp128_split3_pack(w1, b1, w2)
    img_lin = ops.rowlin128_split3_pack(wn, bn)
    img_pe = ops.pe_tail_split3_pack(w, w)
    cases = [   # (name, call, plan, (M, N, ldx, ldc, split3) of the observer's descriptor)
        ("st_linear_chain128", lambda: ops.linear_chain128(x, out, [dict(w=w, bias=b, act="gelu"), dict(w=w, bias=b, res=0)]), [5, 30, 1, 1], (M, 256, 128, 128, 0)),
        ("st_mlp128", lambda: ops.mlp128(x, out, w1, b1, w2, b, ln_eps=1e-6), [6, 31, 1, 1], (M, 2 * hidden, 128, 128, 0)),
        ("st_mlp128_split3", lambda: ops.mlp128(x, out, w1, b1, w2, b, ln_eps=1e-6, image=img_mlp), [9, 38, 1, 1], (M, 2 * hidden, 128, 128, 1)),
        ("st_rowlin128_split3", lambda: ops.rowlin128_split3(x, outn, img_lin, ln_eps=1e-5), [10, 40, 1, 1], (M, N, 128, N, 1)),
        ("st_pe_tail_split3", lambda: ops.pe_tail_split3(x64, tab, img_pe, b, b, b, out), [11, 41, 1, 1], (M, 192, 64, 128, 1)),
    ]
    # (1) the plan, no observer installed; a tiled GEMM in between so that each launcher has to overwrite another family's plan
    for name, call, plan, _ in cases:
        ops.conv_gemm(x, w, out)
        assert ops.gemm_last_plan()[0] not in (5, 6, 9, 10, 11), name
        call()
        assert ops.gemm_last_plan() == plan, (name, ops.gemm_last_plan())
    # (2) the same launches under an observer
    seen = []
    p4 = (C.c_int32 * 4)()

    @C.CFUNCTYPE(None, C.POINTER(GemmDesc), C.c_void_p, C.c_int32, C.c_void_p)
    def observer(desc, stream, phase, user):
        d = desc.contents
        lib.st_gemm_last_plan(p4)
        seen.append((phase, list(p4), (d.M, d.N, d.ldx, d.ldc, d.split3), (d.K, d.Cin, d.ldw, d.H, d.W, d.Ho, d.Wo, d.kh, d.kw, d.sh, d.sw, d.batch, d.alpha)))

    for name, call, plan, desc in cases:
        ops.conv_gemm(x, w, out)
        before = ops.gemm_last_plan()
        del seen[:]
        lib.st_set_gemm_observer(C.cast(observer, C.c_void_p), None)
        try:
            call()
        finally:
            lib.st_set_gemm_observer(None, None)
        assert [s[0] for s in seen] == [0, 1], (name, seen)
        assert seen[0][1] == before and seen[1][1] == plan, (name, seen)            # phase 0 precedes the plan update, phase 1 follows it
        for s in seen:
            assert s[2] == desc, (name, s)
            assert s[3] == (128, 128, 128, 1, desc[0], 1, desc[0], 1, 1, 1, 1, 1, 1.0), (name, s)
        assert ops.gemm_last_plan() == plan, name
    torch.cuda.synchronize()
