"""The warm start on the GPU: the splat kernel against its CPU restatement (bit for bit), flow_init through FlowFormer against the
reference's own warm calls (tests/golden/warmstart.npz, tools/make_warmstart_golden.py), and SequenceStitcher against the reference's
three-frame chain -- teacher-forced (each frame's init is the golden's: the gate, under test_model_gpu.py's damped end-to-end
bounds) and free-running (a sensitivity figure, judged against the reference's own movement under an init perturbation)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _forward_interp_ref as R  # noqa: E402
from _measure import check  # noqa: E402

from oracle import inputs, spec  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T = torch.from_numpy


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "warmstart.npz"))


def _model(sd):
    import stitch_amd
    cfg, _ = stitch_amd.load_inference_config("all_img1_with_inpaint_g12_transRef")
    m = stitch_amd.build_model(cfg)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def model(seeded_sd):
    return _model(seeded_sd)


@pytest.fixture(scope="module")
def damped_model():
    return _model(spec.damped_state_dict(1234))


def _bits(t):
    return np.packbits((t.detach().cpu().numpy() >= 0.5).astype(np.uint8).reshape(-1))


def _same(x, y, key=""):
    """bit-for-bit equality of two output dicts / lists / tensors / plain values"""
    if isinstance(x, dict):
        assert set(x) == set(y), key
        for k in x:
            _same(x[k], y[k], f"{key}.{k}")
    elif isinstance(x, (list, tuple)):
        assert len(x) == len(y), key
        for i, (p, q) in enumerate(zip(x, y)):
            _same(p, q, f"{key}[{i}]")
    elif torch.is_tensor(x):
        assert x.shape == y.shape and torch.equal(x, y), key
    else:
        assert x == y, key


def _clone(o):
    if isinstance(o, dict):
        return {k: _clone(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_clone(v) for v in o]
    return o.clone() if torch.is_tensor(o) else o


def _grid(B, H, W):
    ii, jj = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    return np.broadcast_to(np.stack([jj, ii], -1).reshape(1, H * W, 2), (B, H * W, 2))


def _splat_both_layouts(flow):
    """flow [B,2,H,W] float32 numpy -> the kernel's result from the NCHW operand, and from coords1 rows = grid + flow (whose flow, as
    the kernel recovers it, is the fp32 (grid + flow) - grid: the restatement is given exactly that)"""
    from stitch_amd import ops
    B, _, H, W = flow.shape
    got = ops.forward_interpolate(T(flow).cuda()).cpu().numpy()
    assert np.array_equal(got.view(np.int32), R.forward_interpolate(flow).view(np.int32)), "NCHW layout"
    with np.errstate(invalid="ignore"):
        rows = (_grid(B, H, W) + flow.reshape(B, 2, H * W).transpose(0, 2, 1)).astype(np.float32)
        back = (rows - _grid(B, H, W)).astype(np.float32).transpose(0, 2, 1).reshape(B, 2, H, W)
    out = torch.full((B, 2, H, W), 7.0, device="cuda")
    ret = ops.forward_interpolate(T(np.ascontiguousarray(rows.reshape(B * H * W, 2))).cuda(), out=out, coords_rows=(B, H, W))
    assert ret is out
    assert np.array_equal(out.cpu().numpy().view(np.int32), R.forward_interpolate(back).view(np.int32)), "coords1 rows layout"
    return got


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
def test_splat_kernel_equals_the_reference_outputs_on_the_golden_fields(gold):
    for n in gold["a_names"]:
        got = _splat_both_layouts(gold[f"a_{n}_in"][None])
        assert np.array_equal(got[0].view(np.int32), gold[f"a_{n}_out"].view(np.int32)), n      # scipy's own output


def test_splat_kernel_batch_large_ties_invalid_nan(gold):
    from stitch_amd import ops
    names = [n for n in gold["a_names"] if gold[f"a_{n}_in"].shape[1:] == (64, 64)]
    _splat_both_layouts(np.stack([gold[f"a_{n}_in"] for n in names[:2]]))                         # B = 2
    _splat_both_layouts(R.generic_field(128, 128, 11.0, 21)[None])                                # N = 16384: eight LDS chunks
    _splat_both_layouts(R.generic_field(23, 37, 5.0, 22)[None])                                   # N not a multiple of anything
    seed, H, W = (int(v) for v in gold["a_tie_seed_hw"])
    ti = np.random.default_rng(seed).integers(-3, 4, (2, H, W)).astype(np.float32)
    _splat_both_layouts(np.stack([ti, ti[::-1].copy()]))                                          # exact ties: the lowest source index
    dead = np.full((2, 12, 16), 100.0, np.float32)
    live = R.generic_field(12, 16, 1.5, 3)
    got = _splat_both_layouts(np.stack([dead, live, dead]))                                       # no valid source: zeros, per element
    assert not got[0].any() and not got[2].any() and got[1].any()
    bad = live.copy()
    bad[0, 4, 5] = np.nan
    bad[1, 7, 2] = np.nan
    bad[:, 0, 0] = np.inf
    got = ops.forward_interpolate(T(bad[None]).cuda()).cpu().numpy()
    assert np.isfinite(got).all() and np.array_equal(got[0], R.forward_interpolate(bad))
    with pytest.raises(ValueError):
        ops.forward_interpolate(torch.zeros(1, 3, 8, 8, device="cuda"))
    with pytest.raises(Exception):
        ops.forward_interpolate(torch.zeros(1, 2, 256, 260, device="cuda"))                       # ST_EINVAL: N > 65536


# ---------------------------------------------------------------------------------------------------------------- 2. zero init
def test_zero_flow_init_is_the_cold_start(model):
    fb = model.flow_backbone
    a, b = (t.cuda() for t in inputs.structured_pair(96, 128, seed=3, shift=(2, -3)))
    up, c1, (B, H1, W1) = fb.flow_rows(a, b)
    upz, c1z, _ = fb.flow_rows(a, b, flow_init=torch.zeros(B, 2, H1, W1, device="cuda"))
    assert torch.equal(up, upz) and torch.equal(c1, c1z)
    up, c1, (B2, H1, W1) = fb.flow_rows_pair(a, b)
    upz, c1z, _ = fb.flow_rows_pair(a, b, flow_init=torch.zeros(B2, 2, H1, W1, device="cuda"))
    assert B2 == 2 and torch.equal(up, upz) and torch.equal(c1, c1z)
    # and the pair's second half starts from the second half of the init: a->b first, then b->a
    fi = 0.5 * torch.randn(2, 2, H1, W1, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    upp = fb.flow_rows_pair(a, b, flow_init=fi)[0]
    up_ab = fb.flow_rows(a, b, flow_init=fi[:1].contiguous())[0]
    up_ba = fb.flow_rows(b, a, flow_init=fi[1:].contiguous())[0]
    assert not torch.equal(upp, up)
    # (batched and single passes order their sums differently: close, not equal -- these weights amplify roundings)
    print(f"[pair vs single, warm] a->b {float((upp[:1] - up_ab).abs().max()):.3e} b->a {float((upp[1:] - up_ba).abs().max()):.3e} px")
    with pytest.raises(ValueError):
        fb.flow_rows(a, b, flow_init=torch.zeros(1, 2, H1 + 1, W1, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------- 3. flow network
def test_flowformer_warm_call_damped_512_vs_reference_golden(damped_model, gold):
    """the init bits are the golden's, so only the network's arithmetic differs, as in a cold call: the cold call's bounds on these
    weights (tests/test_model_gpu.py damped_e2e_flow_*)"""
    a, b = inputs.structured_pair(512, 512, seed=7, shift=(6, -10))
    up, low = damped_model.flow_backbone(a.cuda(), b.cuda(), flow_init=T(gold["b_damped_fi"]).cuda())
    assert up.shape == (1, 2, 512, 512) and low.shape == (1, 2, 64, 64)
    d = np.abs(up[..., ::4, ::4].cpu().numpy() - gold["b_damped_flow_up_sub"])
    dl = np.abs(low.cpu().numpy() - gold["b_damped_flow_lowres"]).max()
    print(f"[warm damped 512] flow_up max {d.max():.3e} p99 {np.percentile(d, 99):.3e} px, flow_lowres max {dl:.3e} low-res px "
          f"(reference 8 vs 1 thread: {float(gold['b_damped_floor_flow_up_max_px']):.3e} px; warm vs cold call: "
          f"{float(gold['b_damped_warm_vs_cold_flow_up_max_px']):.2f} px)")
    check("warm_damped_flow_max_px", d.max(), 7.5e-4, note="damped_e2e_flow_max_px's bound")
    check("warm_damped_flow_p99_px", np.percentile(d, 99), 3.6e-4, note="damped_e2e_flow_p99_px's bound")
    cs = np.array([float(up.double().sum()), float((up.double() ** 2).sum())])
    check("warm_damped_flow_checksum_rel", np.abs(cs / gold["b_damped_flow_up_cs"] - 1).max(), 7e-6, note="damped_e2e_flow_checksum_rel's bound")


def test_flowformer_warm_call_seeded_small_vs_reference_golden(model, gold):
    """seeded weights are chaotic: the bound is 3 x the distance of the reference's own fp32 warm call from its fp64 run of the same call
    (stored by the generator), the ratio ff_small_flow_px has to its own fp32-to-fp64 distance"""
    a, b = inputs.structured_pair(96, 128, seed=3, shift=(3, -4))
    up, low = model.flow_backbone(a.cuda(), b.cuda(), flow_init=T(gold["b_seeded_fi"]).cuda())
    d = np.abs(up.cpu().numpy() - gold["b_seeded_flow_up_sub"]).max()
    d64 = np.abs(up[..., ::2, ::2].cpu().numpy().astype(np.float64) - gold["b_seeded_flow_up_fp64_sub"]).max()
    ref = float(gold["b_seeded_fp32_to_fp64_max_px"])
    print(f"[warm seeded 96x128] flow_up vs reference fp32 {d:.3e} px, vs its fp64 run {d64:.3e} px (reference fp32 to fp64: {ref:.3e} px; "
          f"8 vs 1 thread {float(gold['b_seeded_floor_flow_up_max_px']):.3e} px; |flow| up to {float(gold['b_seeded_flow_absmax']):.1f} px)")
    check("warm_seeded_small_flow_px", d, 3 * ref, note="3 x the reference's fp32-to-fp64 distance on this warm call")


# ---------------------------------------------------------------------------------------------------------------- 4. sequence
def _frames(gold):
    return [tuple(t.cuda() for t in inputs.structured_pair(512, 512, seed=7, shift=tuple(int(v) for v in s))) for s in gold["c_shifts"]]


def _damped_e2e_checks(o, gold, k, floor_occ_flips):
    """tests/test_model_gpu.py::test_end_to_end_damped_eval_512_vs_reference_golden's bounds, unchanged, on frame k of the sequence golden
    (sub-sampled by 8 / 16 instead of 4 and with one of final_warp_output's three equal mask channels: the golden's size limit)"""
    p, n = f"c_f{k}_", f"warm_seq_f{k}_"
    H = o["H"].cpu().numpy()
    check(n + "H_rel", np.abs(H - gold[p + "H"]).max() / max(1.0, np.abs(gold[p + "H"]).max()), 3.6e-6)
    flow = o["flow_predictions"][0]
    dflow = np.abs(flow[..., ::8, ::8].cpu().numpy() - gold[p + "flow_sub"])
    occ_flip = np.unpackbits(_bits(o["origin_occlusion_mask"]) ^ gold[p + "occ_bits"]).sum()
    dH = np.abs(o["output_H"][:, 0:4, ::16, ::16].cpu().numpy() - gold[p + "output_H_sub"])
    fin = o["final_warp_output"]
    assert torch.equal(fin[:, 3], fin[:, 4]) and torch.equal(fin[:, 3], fin[:, 5])
    got, want = fin[:, 0:4, ::8, ::8].cpu().numpy(), gold[p + "final_sub"]
    dimg = np.abs(got[:, 0:3] - want[:, 0:3]) * (got[:, 3:4] == want[:, 3:4])
    fcs = np.array([float(flow.double().sum()), float((flow.double() ** 2).sum())])
    print(f"[sequence frame {k}, golden init] H {np.abs(H - gold[p + 'H']).max():.2e} flow max {dflow.max():.3e} p99 {np.percentile(dflow, 99):.3e} "
          f"occ flips {occ_flip} output_H max {dH.max():.3e} final max {dimg.max():.3e}")
    check(n + "flow_max_px", dflow.max(), 7.5e-4)
    check(n + "flow_p99_px", np.percentile(dflow, 99), 3.6e-4)
    check(n + "occ_flips", occ_flip, 3 * floor_occ_flips, inclusive=True)
    check(n + "overlap_flips", np.unpackbits(_bits(o["overlap"]) ^ gold[p + "overlap_bits"]).sum(), 2, inclusive=True)
    check(n + "output_H_max", dH.max(), 0.05)
    check(n + "final_max_where_masks_agree", dimg.max(), 0.04)
    check(n + "flow_checksum_rel", np.abs(fcs / gold[p + "flow_cs"] - 1).max(), 7e-6)


def test_sequence_first_call_is_the_model_and_teacher_forced_frames_meet_the_cold_bounds(damped_model, gold):
    import stitch_amd
    frames = _frames(gold)
    floor = int(np.load(os.path.join(GOLDEN, "e2e_eval_damped_512.npz"))["ref_floor_occ_flips"])
    seq = stitch_amd.SequenceStitcher(damped_model)
    assert seq.state() is None
    cold = damped_model(*frames[0], type="test_eval")
    seq.reset()
    _same(seq(*frames[0]), cold)
    st = seq.state()
    assert st.shape == (2, 2, 64, 64) and st.abs().max() > 0
    seq(*frames[1])
    seq.reset()
    assert not seq.state().any()
    _same(seq(*frames[0]), cold)                                    # after reset(): the cold result again
    # the state the first frame leaves: the splat of its own low-resolution flows, a->b then b->a
    low0 = gold["c_f0_flow_lowres"]
    d0 = np.abs(seq.state().cpu().numpy() - gold["c_f1_init"])
    print(f"[sequence] state after frame 0 vs the golden's frame-1 init: max {d0.max():.3e} low-res px, pixels with another source "
          f"{int((d0.max(1) > 1e-2).sum())} of {d0[:, 0].size} (low-res flow up to {np.abs(low0).max():.2f} px)")
    for k in (1, 2):
        seq.set_state(T(gold[f"c_f{k}_init"]).cuda())
        assert np.array_equal(seq.state().cpu().numpy(), gold[f"c_f{k}_init"])
        _damped_e2e_checks(seq(*frames[k]), gold, k, floor)


def test_sequence_free_running_against_the_references_own_sensitivity(damped_model, gold):
    """NOT the gate (that is the teacher-forced test above): the decoder is not contractive in its start point and the splat is
    discontinuous, so a free-running chain is judged against what the REFERENCE's own flow does when its init comes from a low-res
    flow perturbed by the GPU-vs-reference gap (golden part d): <= 3 x that movement."""
    import stitch_amd
    frames = _frames(gold)
    seq = stitch_amd.SequenceStitcher(damped_model)
    seq.reset()
    flows = [seq(a, b)["flow_predictions"][0][..., ::8, ::8].cpu().numpy() for a, b in frames]
    d = [np.abs(f - gold[f"c_f{k}_flow_sub"]) for k, f in enumerate(flows)]
    for k in range(3):
        print(f"[sequence free-running] frame {k}: flow vs golden max {d[k].max():.3e} p99 {np.percentile(d[k], 99):.3e} px"
              + (f"; the reference under an init perturbation of {float(gold['d_perturb_lowres_px']):.2e} low-res px: max "
                 f"{float(gold[f'd_f{k}_flow_moved_max_px']):.3e} p99 {float(gold[f'd_f{k}_flow_moved_p99_px']):.3e} px; its 8 vs 1 thread chain: "
                 f"{float(gold[f'c_f{k}_floor_flow_max_px']):.3e} px" if k else ""))
    for k in (1, 2):
        check(f"warm_seq_free_f{k}_flow_max_px", d[k].max(), 3 * float(gold[f"d_f{k}_flow_moved_max_px"]),
              note="a sensitivity figure, not the gate: 3 x the reference's own movement under a perturbed init")


# ---------------------------------------------------------------------------------------------------------------- 5. graph
def test_graphed_sequence_equals_eager_with_a_neighbour_and_a_reset(damped_model, gold):
    import stitch_amd
    frames = _frames(gold)
    eager = stitch_amd.SequenceStitcher(damped_model)
    want = [_clone(eager(a, b)) for a, b in frames]
    assert not torch.equal(want[1]["flow_predictions"][0], damped_model(*frames[1], type="test_eval")["flow_predictions"][0])
    g, other = stitch_amd.SequenceStitcher(damped_model, graphed=True), stitch_amd.SequenceStitcher(damped_model, graphed=True)
    s_other = torch.cuda.Stream()
    for rep in range(2):                                            # (rep 0 captures: the warm-up runs must not leak into the state)
        g.reset()
        for k, (a, b) in enumerate(frames):
            s_other.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s_other):
                other(*frames[2 - k])                               # another sequence, other frames, another stream, in flight
            _same(_clone(g(a, b)), want[k], f"rep {rep} frame {k}")
        torch.cuda.synchronize()
    g(*frames[1])
    g.reset()                                                       # mid-sequence: the cold result again
    _same(_clone(g(*frames[0])), want[0])
    _same(g.state(), eager_state_after(eager, frames[0]))
    assert stitch_amd.SequenceStitcher(damped_model, iters=6, graphed=True)(*frames[0])["flow_predictions"][0].shape == (1, 2, 512, 512)


def eager_state_after(seq, frame):
    seq.reset()
    seq(*frame)
    return seq.state()


# ---------------------------------------------------------------------------------------------------------------- 6. test_out
def test_sequence_test_out_first_frame_and_state(damped_model):
    import stitch_amd
    from stitch_amd import ops
    a, b = (t.cuda() for t in inputs.structured_pair(320, 480, seed=7))
    a2, b2 = (t.cuda() for t in inputs.structured_pair(320, 480, seed=7, shift=(6, -10)))
    seq = stitch_amd.SequenceStitcher(damped_model, type="test_out")
    cold = damped_model(a, b, type="test_out")
    o = seq(a, b)
    _same(o, cold)
    # the state the second frame starts from: the splat of the first frame's two 64x64 flows
    a512 = ops.resize_bilinear(a, 512, 512, False)
    _, coords1, (B2, H1, W1) = damped_model.flow_backbone.flow_rows_pair(a512, o["warp_input2_tensor_512"].contiguous())
    low = (coords1.cpu().numpy().reshape(B2, H1 * W1, 2) - _grid(B2, H1, W1)).astype(np.float32).transpose(0, 2, 1).reshape(B2, 2, H1, W1)
    assert np.array_equal(seq.state().cpu().numpy(), R.forward_interpolate(low))
    o2 = seq(a2, b2)
    assert not torch.equal(o2["residual_flow"], damped_model(a2, b2, type="test_out")["residual_flow"])      # it did start warm
    assert sorted(o2) == sorted(cold)
