"""The bounds of tests/_rows_bounds.py, shown on the CPU to be neither wrong nor vacuous, and the test matrix of tests/test_rows_matrix_gpu.py
shown to reach what it claims.

1. Sound.  A bound that fp32 itself breaks is wrong: a plain torch fp32 evaluation of each reference formula (for the split3 operators with
   every product taken as six fp32 products of the operands' hi / mid / lo bf16 parts, the three smallest dropped) lies within E elementwise on
   every generator, the LayerNorm edge rows included.
2. Sharp.  A bound that a real defect meets is vacuous: eight kernel-shaped faults, applied to the fp64 reference, must each exceed E somewhere
   by 10x or more.  The smallest ratio per fault is printed (pytest -s) and quoted in DESIGN.md.
3. Grid replay.  The grid each entry point picks (csrc/gemm_rows.hip: st_linear_chain128, st_mlp128, st_mlp128_split3, st_rowlin128_split3,
   st_pe_tail_split3) restated here from the launcher text, and the case lists of _rows_bounds.py held against it: rounds 1, 2 and 3, idle
   waves in an active workgroup, workgroups with fewer rounds than the first, every residue of steps per round against the ring depth, TABINV
   with and without a shrunken grid, a table walk of several blocks."""
import math

import pytest
import torch

import _rows_bounds as rb

M_CPU = 129


def f32_ln(x, eps):
    d = x - x.mean(-1, keepdim=True)
    return d * (1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps))


def f32_gelu(v):
    y = 0.5 * torch.special.erfc(v.abs() * (0.5 ** 0.5))
    return torch.where(v >= 0, v * (1.0 - y), v * y)


def mm32(x, w):
    return x @ w.t()


def parts(x):
    hi = x.bfloat16().float()
    mid = (x - hi).bfloat16().float()
    return hi, mid, ((x - hi) - mid).bfloat16().float()


def mm_s3(x, w):
    (xh, xm, xl), (wh, wm, wl) = parts(x), parts(w)
    return ((((mm32(xh, wl) + mm32(xl, wh)) + mm32(xm, wm)) + mm32(xh, wm)) + mm32(xm, wh)) + mm32(xh, wh)


def chain32(a, layers):
    x, inputs = a, []
    for y in layers:
        inputs.append(x)
        v = mm32(f32_ln(x, y["ln_eps"]) if y.get("ln_eps") is not None else x, y["w"])
        if y.get("bias") is not None:
            v = v + y["bias"]
        v = dict(none=lambda t: t, relu=torch.relu, gelu=f32_gelu)[y.get("act", "none")](v)
        r = y.get("res")
        if r is not None:
            v = v + (inputs[r] if isinstance(r, int) else r)
        x = v
    return x


def mlp32(a, w1, b1, w2, b2, ln_eps=None, res=None, proj=None, split3=False):
    mm = mm_s3 if split3 else mm32
    x = a
    if proj is not None:
        x = mm(a, proj[0])
        x = x + proj[1] if proj[1] is not None else x
        x = x + proj[2] if proj[2] is not None else x
    v = mm(f32_gelu(mm(f32_ln(x, ln_eps) if ln_eps is not None else x, w1) + b1), w2)
    v = (v + b2) + x
    return v + res if res is not None else v


def rowlin32(a, w, b=None, ln_eps=None, aux=None, row_div=1):
    v = mm_s3(f32_ln(a, ln_eps) if ln_eps is not None else a, w)
    v = v + b if b is not None else v
    return v + aux[torch.arange(a.shape[0]) // row_div] if aux is not None else v


def pe32(x, w1, tab, w2, b2, gamma, beta, eps=1e-5):
    h = torch.relu(mm_s3(x, w1) + tab[torch.arange(x.shape[0]) % tab.shape[0]])
    return f32_ln(mm_s3(h, w2) + b2, eps) * gamma + beta


def mlp_kw(d, proj, ln, res):
    return dict(ln_eps=1e-5 if ln else None, res=d["res"] if res else None,
                proj=dict(none=None, full=(d["wp"], d["bp"], d["res0"]), bare=(d["wp"], None, None))[proj])


def mlp_args(d):
    return d["a"], d["w1"], d["b1"], d["w2"], d["b2"]


def pe_args(d):
    return d["x"], d["w1"][:, :64].contiguous(), d["tab"], d["w2"], d["b2"], d["gamma"], d["beta"]


# ------------------------------------------------------------------------------------------------ 1. sound
@pytest.mark.parametrize("form", rb.CHAIN_FORMS)
@pytest.mark.parametrize("edge", [False, True])
def test_chain_fp32_within_bound(form, edge):
    layers = rb.chain_layers(form, M_CPU, 100)
    a = rb.edge_rows(M_CPU, 101) if edge else rb.rows(M_CPU, 101)
    ref, E = rb.chain_bound(a, layers)
    assert rb.ratio(chain32(a, layers), ref, E) <= 1.0


@pytest.mark.parametrize("hidden", rb.MLP_HIDDEN)
@pytest.mark.parametrize("split3", [False, True])
def test_mlp_fp32_within_bound(hidden, split3):
    for edge in (False, True):
        d = rb.mlp_inputs(M_CPU, hidden, 200 + hidden, edge)
        for proj in rb.MLP_PROJ:
            for ln, res in ((True, True), (True, False), (False, True), (False, False)):
                kw = mlp_kw(d, proj, ln, res)
                ref, E = rb.mlp_bound(*mlp_args(d), split3=split3, **kw)
                r = rb.ratio(mlp32(*mlp_args(d), split3=split3, **kw), ref, E)
                assert r <= 1.0, (hidden, split3, edge, proj, ln, res, r)


@pytest.mark.parametrize("N", rb.ROWLIN_N)
def test_rowlin_fp32_within_bound(N):
    for edge in (False, True):
        d = rb.rowlin_inputs(M_CPU, N, 300 + N, edge)
        for ln in (True, False):
            for div in (None, 1, 8, 7):
                aux = None if div is None else rb.table((M_CPU + div - 1) // div, 301, N)
                kw = dict(b=d["b"] if ln else None, ln_eps=1e-5 if ln else None, aux=aux, row_div=div or 1)
                ref, E = rb.rowlin_bound(d["a"], d["w"], **kw)
                assert rb.ratio(rowlin32(d["a"], d["w"], **kw), ref, E) <= 1.0, (N, edge, ln, div)


@pytest.mark.parametrize("P", [1, 3, 5, 7, 64, 257])
def test_pe_tail_fp32_within_bound(P):
    for edge in (False, True):
        d = rb.pe_inputs(M_CPU, P, 400 + P, edge)
        ref, E = rb.pe_tail_bound(*pe_args(d))
        assert rb.ratio(pe32(*pe_args(d)), ref, E) <= 1.0, (P, edge)
    # a constant row into the closing LayerNorm: w2 = 0 leaves b2 alone, and a constant b2 has variance 0
    d["w2"], d["b2"] = torch.zeros(128, 128), torch.full((128,), 0.7)
    ref, E = rb.pe_tail_bound(*pe_args(d))
    assert rb.ratio(pe32(*pe_args(d)), ref, E) <= 1.0


def test_gelu_bound_holds_for_the_polynomial_itself():
    """Abramowitz-Stegun 7.1.26 evaluated in fp32 the way st_gelu does (common.h), exp2 and the reciprocal through torch: inside the GELU step's bound
    on a dense grid of [-12, 12] -- the published 1.5e-7 and the evaluation's roundings are what the step adds up."""
    v = torch.linspace(-12, 12, 480001)
    s = v.abs() * torch.tensor(0.70710678118654752440)
    t = 1.0 / (torch.tensor(rb.AS_P) * s + 1.0)
    a = [torch.tensor(c) for c in rb.AS_A]
    y = a[4] * t + a[3]
    for c in (a[2], a[1], a[0]):
        y = y * t + c
    y = y * t * torch.exp2(s * s * torch.tensor(-rb.LOG2E)) * 0.5
    g = v * torch.where(v >= 0, 1.0 - y, y)
    ref, E = rb.gelu(v.double(), torch.zeros_like(v, dtype=torch.float64))
    assert rb.ratio(g, ref, E) <= 1.0


# ------------------------------------------------------------------------------------------------ 2. sharp
MIN_RATIO = {}


def faulty(name, out, ref, E):
    r = rb.ratio(out, ref, E)
    MIN_RATIO[name] = min(MIN_RATIO.get(name, float("inf")), r)
    assert r >= 10.0, f"{name}: the fault moves the result by only {r:.3g} E"


def swap_chunk(w, c, dim=0):
    """32-feature chunk c replaced by chunk c - 1 (the stale stage of a ring)"""
    w = w.clone()
    w.narrow(dim, 32 * c, 32).copy_(w.narrow(dim, 32 * (c - 1), 32).clone())
    return w


@pytest.mark.parametrize("hidden", rb.MLP_HIDDEN)
@pytest.mark.parametrize("split3", [False, True])
def test_mlp_faults_exceed_bound(hidden, split3):
    d = rb.mlp_inputs(M_CPU, hidden, 500 + hidden)
    # the faults of the hidden walk at the form without projection (a bound grows with every layer in front of the fault: each fault is planted
    # where the matrix is sharpest for it), those of the projection behind it
    kw = mlp_kw(d, "none", True, True)
    ref, E = rb.mlp_bound(*mlp_args(d), split3=split3, **kw)
    run = lambda **ch: rb.mlp_ref(*mlp_args({**d, **ch}), split3=split3, **{**kw, **{k: v for k, v in ch.items() if k in kw}})     # noqa: E731
    c = hidden // 32 - 1
    if c > 0:
        faulty("stale_w1_chunk", run(w1=swap_chunk(d["w1"], c)), ref, E)
        faulty("stale_w2_slice", run(w2=swap_chunk(d["w2"], c, 1)), ref, E)
        b1 = d["b1"].clone()
        b1[32 * (c - 1):32 * c] = d["b1"][32 * c:32 * c + 32]
        faulty("b1_of_next_chunk", run(b1=b1), ref, E)
    w2 = d["w2"].clone()
    w2[:, 32 * c:] = 0
    faulty("fc2_chunk_dropped", run(w2=w2), ref, E)
    w2 = d["w2"].clone()
    w2[:, 32 * c:] *= 2
    faulty("fc2_chunk_twice", run(w2=w2), ref, E)
    faulty("residual_row_plus_32", run(res=torch.roll(d["res"], -32, 0)), ref, E)
    kw = mlp_kw(d, "full", True, True)
    ref, E = rb.mlp_bound(*mlp_args(d), split3=split3, **kw)
    faulty("stale_wp_chunk", rb.mlp_ref(*mlp_args(d), split3=split3, **{**kw, "proj": (swap_chunk(d["wp"], 2), d["bp"], d["res0"])}), ref, E)
    faulty("residual_row_plus_32", rb.mlp_ref(*mlp_args(d), split3=split3, **{**kw, "proj": (d["wp"], d["bp"], torch.roll(d["res0"], -32, 0))}), ref, E)


@pytest.mark.parametrize("form", rb.CHAIN_FORMS)
def test_chain_faults_exceed_bound(form):
    layers = rb.chain_layers(form, M_CPU, 600)
    a = rb.rows(M_CPU, 601)
    ref, E = rb.chain_bound(a, layers)
    for l in range(len(layers)):
        bad = [dict(y) for y in layers]
        bad[l]["w"] = swap_chunk(layers[l]["w"], 1 + l)
        faulty("stale_chain_chunk", rb.chain_ref(a, bad), ref, E)
        r = layers[l].get("res")
        if r is not None and not isinstance(r, int):
            bad = [dict(y) for y in layers]
            bad[l]["res"] = torch.roll(r, -32, 0)
            faulty("residual_row_plus_32", rb.chain_ref(a, bad), ref, E)
        if isinstance(r, int) and layers[r].get("ln_eps") is not None:
            # the saved input of layer r taken behind its LayerNorm: x_r is recomputed as the chain up to layer r
            xr = rb.chain_ref(a, layers[:r]) if r else a.double()
            bad = [dict(y) for y in layers]
            bad[l]["res"] = rb.ln(xr, torch.zeros_like(xr), layers[r]["ln_eps"])[0]
            faulty("saved_input_after_ln", rb.chain_ref(a, bad), ref, E)


@pytest.mark.parametrize("N", rb.ROWLIN_N)
def test_rowlin_faults_exceed_bound(N):
    d = rb.rowlin_inputs(M_CPU, N, 700 + N)
    for div in (1, 8, 7):
        aux = rb.table((M_CPU + div - 1) // div + 1, 701, N)
        ref, E = rb.rowlin_bound(d["a"], d["w"], d["b"], 1e-5, aux, div)
        # the rows of block 1 (32..63) take the table row one further on
        idx = torch.arange(M_CPU) // div
        idx[32:64] += 1
        plain = rb.rowlin_ref(d["a"], d["w"], d["b"], 1e-5)
        faulty("aux_row_off_by_one", plain + aux.double()[idx], ref, E)
    if N > 32:
        faulty("stale_rowlin_chunk", rb.rowlin_ref(d["a"], swap_chunk(d["w"], N // 32 - 1), d["b"], 1e-5, aux, div), ref, E)


@pytest.mark.parametrize("P", [3, 5, 7, 64, 257])
def test_pe_tail_faults_exceed_bound(P):
    d = rb.pe_inputs(M_CPU, P, 800 + P)
    ref, E = rb.pe_tail_bound(*pe_args(d))
    faulty("table_row_plus_1", rb.pe_tail_ref(*pe_args({**d, "tab": torch.roll(d["tab"], -1, 0)})), ref, E)
    faulty("stale_pe_w1_chunk", rb.pe_tail_ref(*pe_args({**d, "w1": swap_chunk(d["w1"], 3)})), ref, E)
    w2 = d["w2"].clone()
    w2[:, 96:] = 0
    faulty("fc2_chunk_dropped", rb.pe_tail_ref(*pe_args({**d, "w2": w2})), ref, E)
    faulty("fc2_chunk_twice", rb.pe_tail_ref(*pe_args({**d, "w2": d["w2"] + (d["w2"] - w2)})), ref, E)


def test_every_fault_was_planted():
    """runs behind the fault tests of this file: each of the eight faults of the list met at least one case; prints the room each leaves"""
    want = {"stale_w1_chunk", "stale_w2_slice", "stale_wp_chunk", "stale_chain_chunk", "stale_rowlin_chunk", "stale_pe_w1_chunk", "fc2_chunk_dropped",
            "fc2_chunk_twice", "table_row_plus_1", "aux_row_off_by_one", "residual_row_plus_32", "saved_input_after_ln", "b1_of_next_chunk"}
    if not want <= set(MIN_RATIO):                              # run alone: one case of each fault test
        test_mlp_faults_exceed_bound(64, True)
        test_chain_faults_exceed_bound("res_l0_from_l2")
        test_chain_faults_exceed_bound("model_self")
        test_rowlin_faults_exceed_bound(64)
        test_pe_tail_faults_exceed_bound(5)
    assert want <= set(MIN_RATIO), want - set(MIN_RATIO)
    for k in sorted(MIN_RATIO):
        print(f"smallest max(err / E) of {k}: {MIN_RATIO[k]:.3g}")


# ------------------------------------------------------------------------------------------------ 3. grid replay
def ring_grid(M, cap, nw=4):
    """st_linear_chain128 / st_mlp128 / st_rowlin128_split3 (cap 512) and st_mlp128_split3 (cap 256): G = min(ceil(nblk / 4), cap); workgroup g's waves own
    blocks 4 g + wave + rd * 4 G -> (G, rounds of each workgroup, whether some active workgroup has an idle wave in its last round)"""
    nblk = (M + 31) // 32
    G = min((nblk + nw - 1) // nw, cap)
    rounds = [(nblk - nw * g + G * nw - 1) // (G * nw) if nw * g < nblk else 0 for g in range(G)]
    idle = any(r > 0 and any(nw * g + w + (r - 1) * G * nw >= nblk for w in range(nw)) for g, r in enumerate(rounds))
    return G, rounds, idle


def pe_grid(R, P):
    """st_pe_tail_split3: the capped grid, then the largest g in [G - G / 8 (1 below nine), G] with 128 g % P == 0 -> (G, tabinv, shrunk, blocks of wave 0)"""
    nblk = (R + 31) // 32
    G0 = min((nblk + 3) // 4, 256)
    G, tabinv = G0, False
    for g in range(G0, (G0 - G0 // 8 if G0 > 8 else 1) - 1, -1):
        if (g * 128) % P == 0:
            G, tabinv = g, True
            break
    return G, tabinv, G < G0, len(range(0, nblk, 4 * G))


@pytest.mark.parametrize("cap,R", [(512, rb.ROUND_A), (256, rb.ROUND_B)])
def test_row_counts_reach_the_rounds(cap, R):
    assert R == cap * 4 * 32
    for M in rb.SMALL_ROWS + (R,):
        G, rounds, _ = ring_grid(M, cap)
        assert max(rounds) == 1 and G == min(-(-M // 128), cap)
    assert ring_grid(R, cap) == (cap, [1] * cap, False)
    # R + 33: workgroup 0 alone has a second round, with one full block, one one-row block and two idle waves
    G, rounds, idle = ring_grid(R + 33, cap)
    assert (G, rounds[0], set(rounds[1:]), idle) == (cap, 2, {1}, True)
    assert (R + 33 + 31) // 32 - 4 * cap == 2
    # 2 R + 1: three rounds in workgroup 0 (three idle waves), two everywhere else
    G, rounds, idle = ring_grid(2 * R + 1, cap)
    assert (G, rounds[0], set(rounds[1:]), idle) == (cap, 3, {2}, True)
    # a small launch with idle waves in its only round, and the block-position launches of bar (c) in one round
    assert ring_grid(33, cap) == (1, [1], True)
    assert max(ring_grid(R - 4, cap)[1]) == 1


def test_steps_per_round_reach_every_ring_residue():
    # chain: 4 steps per layer through a 3-stage ring
    assert {4 * rb.CHAIN_NLAYERS[f] % 3 for f in rb.CHAIN_FORMS} == {0, 1, 2}
    assert {4 * rb.CHAIN_NLAYERS[f] % 3 for f in rb.CHAIN_MODEL_FORMS} == {0, 2}
    assert rb.CHAIN_ROWS[1] == rb.ROUND_A + 33
    # the MLPs: 4 projection steps + hidden / 32; 3 stages (split3), 2 stages (fp32); hidden 32 is the one-chunk pipeline
    spr = [(4 if p else 0) + h // 32 for h, p in rb.MLP_MULTI]
    assert {s % 3 for s in spr} == {0, 1, 2} and {s % 2 for s in spr} == {0, 1} and 1 in spr and (128, False) in rb.MLP_MULTI
    assert any(p for _, p in rb.MLP_MULTI) and all(h <= 192 for h, _ in rb.MLP_MULTI)
    # rowlin: N / 32 steps, 3 stages; one step per round included
    assert {n // 32 % 3 for n in rb.ROWLIN_MULTI_N} == {0, 1, 2} and 32 in rb.ROWLIN_MULTI_N and max(rb.ROWLIN_MULTI_N) <= 128


def test_pe_tail_cases_reach_every_grid_choice():
    got = {(R, P): pe_grid(R, P) for R, P in rb.PE_CASES}
    assert got[(600, 3)] == (3, True, True, 2)                                  # shrunk from 5: a wave walks two blocks where the cap alone gives one
    assert got[(2 * rb.ROUND_B + 1, 5)] == (255, True, True, 3)                 # shrunk from 256
    assert got[(600, 7)] == (5, False, False, 1)                                # no TABINV, one block per wave
    assert got[(rb.ROUND_B + 33, 257)] == (256, False, False, 2)                # no TABINV, a walk of two blocks
    assert got[(rb.ROUND_B + 33, 64)] == (256, True, False, 2) and got[(2 * rb.ROUND_B + 1, 64)] == (256, True, False, 3)      # TABINV at the capped grid
    assert got[(rb.ROUND_B, 64)] == (256, True, False, 1)
    assert got[(17, 257)][:2] == (1, False) and got[(33, 1)][:2] == (1, True)   # P > R; P == 1
    assert {P for _, P in rb.PE_CASES} >= {1, 3, 5, 7, 64, 257}
    assert any(t and s for _, t, s, _ in got.values()) and any(t and not s for _, t, s, _ in got.values())
    assert any(not t and n >= 2 for _, t, _, n in got.values())


def test_counts_follow_the_kernel_text():
    assert rb.n_f32(128) == 128 and rb.n_s3(128) == 50 and rb.n_s3(64) == 26 and rb.n_s3(2048) == 770
    assert rb.LN_NS == 2 + 16 + 1 and rb.LN_NV_PE == 64 + 1
    # the largest slope of GELU: Phi(x) + x phi(x) at x = sqrt 2
    x = math.sqrt(2.0)
    assert 0.5 * math.erfc(-1.0) + x * math.exp(-1.0) / math.sqrt(2 * math.pi) < rb.GELU_L
