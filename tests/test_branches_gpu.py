"""FlowHomoAdpater's homography-only (only_homo), H+flow (use_combine_h_flow) and no-mask test_out branches against the
reference's own outputs (tests/golden/branches_*.npz, tools/make_branch_goldens.py).  Bounds are constants; the reference's
8-vs-1-thread spread on the same case is quoted next to each."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _measure import check  # noqa: E402

from oracle import inputs, spec  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T = torch.from_numpy


def _bits(t):
    return np.packbits((t.detach().cpu().numpy() >= 0.5).astype(np.uint8).reshape(-1))


@contextlib.contextmanager
def flags(model, **kw):
    old = {k: getattr(model.cfg, k) for k in kw}
    for k, v in kw.items():
        setattr(model.cfg, k, v)
    try:
        yield model
    finally:
        for k, v in old.items():
            setattr(model.cfg, k, v)


@pytest.fixture(scope="module")
def homo_model(seeded_sd):
    import stitch_amd
    cfg, _ = stitch_amd.load_inference_config("all_img1_with_inpaint_g12_transRef", model_config_name="last_config_only_homo")
    m = stitch_amd.build_model(cfg)
    m.load_state_dict(seeded_sd, strict=True)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def damped_model():
    import stitch_amd
    cfg, _ = stitch_amd.load_inference_config("all_img1_with_inpaint_g12_transRef")
    m = stitch_amd.build_model(cfg)
    m.load_state_dict(spec.damped_state_dict(1234), strict=True)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def g_eval():
    return np.load(os.path.join(GOLDEN, "branches_eval_512.npz"))


class GemmCount:
    """st_conv_gemm calls enqueued while the context is open (the library's profiling observer)."""

    def __enter__(self):
        from stitch_amd._lib import lib
        self.lib, self.n = lib, 0

        def cb(desc, stream, phase, user):
            if phase == 0:
                self.n += 1
        self._cb = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p)(cb)
        lib.st_set_gemm_observer(C.cast(self._cb, C.c_void_p), None)
        return self

    def __exit__(self, *exc):
        self.lib.st_set_gemm_observer(None, None)


def test_only_homo_eval_vs_golden(homo_model, g_eval):
    a, b = inputs.structured_pair(512, 512, seed=7)
    a, b = a.cuda(), b.cuda()
    with GemmCount() as homo:
        homo_model.predict_homo(a, b)
    with GemmCount() as full:
        o = homo_model(a, b, type="test_eval")
    torch.cuda.synchronize()
    assert full.n == homo.n > 0                 # the homography network's GEMMs only: FlowFormer++ never ran
    assert sorted(o.keys()) == list(g_eval["oh_keys"])
    assert o["flow_predictions"] is None and o["overlap"] is None and o["final_warp_output"] is o["output_H"]
    assert "origin_occlusion_mask" not in o and tuple(o["output_H"].shape) == (1, 6, 512, 512)
    H = o["H"].cpu().numpy()
    check("only_homo_H_rel", np.abs(H - g_eval["oh_H"]).max() / max(1.0, np.abs(g_eval["oh_H"]).max()), 3.6e-6)   # reference 8 vs 1 threads: 2.0e-6
    dH = np.abs(o["output_H"][:, 0:4, ::4, ::4].cpu().numpy() - g_eval["oh_output_H_sub"])
    check("only_homo_output_H_max", dH.max(), 0.05)                                                    # reference 8 vs 1 threads: 0.067


def test_homo_flow_warp_kernel_vs_reference():
    """st_homo_flow_warp fed the reference's H, residual flow and uint8-valued image 2 (B=2, 96x128, a strong perspective:
    |final_flow| up to 1e6 px, 38 % of the pixels sampled outside): final_warp_output, overlap and the inverse H bit for bit."""
    import stitch_amd
    g = np.load(os.path.join(GOLDEN, "branches_kernel.npz"))
    img = T(g["k_image2"].astype(np.float32)).cuda()
    fin, overlap, Hi = stitch_amd.ops.homo_flow_warp(img, T(g["k_H"]).cuda(), T(g["k_flow"]).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(Hi.cpu().numpy().view(np.uint32), g["k_Hi"].view(np.uint32))
    f = fin.cpu().numpy()
    assert np.array_equal(f[:, 3], f[:, 4]) and np.array_equal(f[:, 3], f[:, 5])
    assert np.array_equal(f[:, 0:4].view(np.uint32), g["k_final4"].view(np.uint32))
    assert np.array_equal(overlap.cpu().numpy().astype(np.uint8), g["k_overlap"])


def test_column_major_inverse_vs_torch_inverse():
    """mat3_inv_cm (st_mat3_sandwich invert=2, between identities) against torch.inverse of 483 column-major 3x3s recorded on
    the CPU: bit for bit.  The row-major path (invert=1) is the other LAPACK path and differs on the same matrices."""
    import stitch_amd
    g = np.load(os.path.join(GOLDEN, "branches_kernel.npz"))
    X = T(g["k_cm_in"]).cuda()
    eye = torch.eye(3, device="cuda")
    out_cm, out_rm = torch.empty_like(X), torch.empty_like(X)
    stitch_amd.ops.mat3_sandwich(eye, X, eye, out_cm, invert=2)
    stitch_amd.ops.mat3_sandwich(eye, X, eye, out_rm, invert=1)
    got = out_cm.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), g["k_cm_inv"].view(np.uint32))
    assert not np.array_equal(out_rm.cpu().numpy(), g["k_cm_inv"])


def test_combine_h_flow_end_to_end_damped_512(damped_model, g_eval):
    a, b = inputs.structured_pair(512, 512, seed=7)
    with flags(damped_model, use_combine_h_flow=True, use_fb_consistency_mask=False):
        o = damped_model(a.cuda(), b.cuda(), type="test_eval")
    assert sorted(o.keys()) == list(g_eval["cb_keys"]) and len(o["flow_predictions"]) == 1
    H = o["H"].cpu().numpy()
    check("combine_H_rel", np.abs(H - g_eval["cb_H"]).max() / max(1.0, np.abs(g_eval["cb_H"]).max()), 3.6e-6)   # reference spread 1.8e-6
    dflow = np.abs(o["flow_predictions"][0][..., ::4, ::4].cpu().numpy() - g_eval["cb_flow_sub"])
    check("combine_flow_max_px", dflow.max(), 7.5e-4)                                                   # reference spread 4.5e-4
    got, want = o["final_warp_output"][:, 0:4, ::4, ::4].cpu().numpy(), g_eval["cb_final_sub"]
    same_mask = got[:, 3:4] == want[:, 3:4]
    # The branch's own arithmetic is bit-exact (test_homo_flow_warp_kernel_vs_reference); what remains is the homography
    # network's difference (corner offsets within 1.5e-5 px, test_model_gpu.py), which this branch amplifies: its 1/8-scale H is
    # applied to full-resolution coordinates.  The reference itself, its offsets moved by +-1.5e-5 px, moves by 0.041 .. 0.196
    # grey levels here (six draws, cb_sens_offsets_final_max, tools/make_branch_goldens.py) -- beyond the shipped branch's 0.04,
    # which this branch cannot meet (its 8-vs-1-thread spread is 0.016).  Measured 0.175 on one MI355X.
    check("combine_final_max_where_masks_agree", (np.abs(got[:, 0:3] - want[:, 0:3]) * same_mask).max(), 0.25)
    flips = np.unpackbits(_bits(o["overlap"]) ^ g_eval["cb_overlap_bits"]).sum()
    check("combine_overlap_flips", flips, 3 * max(1, int(g_eval["cb_floor_overlap_flips"])), inclusive=True)   # reference spread 0 (1 assumed)


@pytest.mark.parametrize("hw", [(512, 512), (320, 480)])
def test_test_out_no_mask_end_to_end_damped(damped_model, hw):
    g = np.load(os.path.join(GOLDEN, "branches_out.npz"))
    p = f"out{hw[0]}x{hw[1]}_"
    a, b = inputs.structured_pair(*hw, seed=7)
    with flags(damped_model, use_fb_consistency_mask=False):
        o = damped_model(a.cuda(), b.cuda(), type="test_out")
        assert damped_model._test_out_nets(a.cuda(), b.cuda())["back"] is None     # the backward flow is never computed
    assert sorted(o.keys()) == list(g[p + "keys"])
    assert "occlusion_mask" not in o and "origin_occlusion_mask" not in o
    assert [o["width_min"], o["height_min"], o["out_height"], o["out_width"]] == list(g[p + "ints"])
    check(f"out_plain_{p}H_rel", np.abs(o["H"].cpu().numpy() - g[p + "H"]).max() / max(1.0, np.abs(g[p + "H"]).max()), 7.5e-7)
    bl = o["blend_image"][..., ::2, ::2].cpu().numpy().astype(np.int32)
    d = np.abs(bl - g[p + "blend_sub"].astype(np.int32))
    check(f"out_plain_{p}blend_gt2_frac", (d > 2).mean(), 1.5e-3)        # reference spread 4.3e-4 / 4.6e-4 (full image)


def test_blend_plain_bitexact_vs_numpy():
    import stitch_amd
    gen = torch.Generator().manual_seed(5)
    h, w = 67, 131
    rnd = lambda *s: torch.rand(*s, generator=gen)          # noqa: E731
    homo1 = torch.cat([rnd(1, 3, h, w) * 255, (rnd(1, 3, h, w) > 0.3).float() * rnd(1, 3, h, w)], 1)
    homo2 = torch.cat([rnd(1, 3, h, w) * 255, rnd(1, 3, h, w)], 1)
    fin = torch.cat([rnd(1, 3, h, w) * 255, rnd(1, 3, h, w) * (rnd(1, 1, h, w) > 0.2).float()], 1)
    homo1[:, 3:, :5] = 0.0
    fin[:, 3:, :5] = 0.0
    homo2[:, 3:, :5] = 0.0                                   # 0/0 rows: NaN blend -> 0
    fin_d = fin.cuda()
    o2, m1, m2, bl = stitch_amd.ops.blend_plain(homo1.cuda(), homo2.cuda(), fin_d)
    f32 = np.float32
    H1, H2, Fn = homo1.numpy()[0], homo2.numpy()[0], fin.numpy()[0]
    mm2 = Fn[3:6]
    e_o2 = H2[0:3] * (f32(1) - mm2) + Fn[0:3] * mm2
    e_m2 = H2[3:6] * (f32(1) - mm2) + mm2 * mm2
    mm1 = H1[3:6]
    with np.errstate(invalid="ignore", divide="ignore"):
        e_bl = (H1[0:3] * mm1 + e_o2 * e_m2) / (mm1 + e_m2)
    e_bl = np.nan_to_num(np.clip(e_bl, 0, 255), nan=0.0).astype(np.uint8)
    e_a1 = np.clip(((mm1[0] + mm1[1]) + mm1[2]) / f32(3), 0, 1)
    e_a2 = np.clip(((e_m2[0] + e_m2[1]) + e_m2[2]) / f32(3), 0, 1)
    assert np.array_equal(o2.cpu().numpy()[0], e_o2)
    assert np.array_equal(bl.cpu().numpy()[0], e_bl)
    assert np.array_equal(m1.cpu().numpy()[0], np.broadcast_to(e_a1, (3, h, w)))
    assert np.array_equal(m2.cpu().numpy()[0], np.broadcast_to(e_a2, (3, h, w)))
    assert torch.equal(fin_d.cpu(), fin)                     # read only: no occlusion factor is written back


def test_graphed_equals_eager_and_recaptures_on_branch_switch(damped_model):
    a, b = inputs.structured_pair(512, 512, seed=7)
    a, b = a.cuda(), b.cuda()
    gf = damped_model.graphed("test_eval")
    for kw in (dict(only_homo=True), dict(use_combine_h_flow=True, use_fb_consistency_mask=False)):
        with flags(damped_model, **kw):
            eager = damped_model(a, b, type="test_eval")
            eager = {k: v.clone() for k, v in eager.items() if torch.is_tensor(v)}
            got = gf(a, b)
            for k, v in eager.items():
                assert torch.equal(got[k], v), (kw, k)
    assert len(gf._graphs) == 2                 # one capture per branch
    with flags(damped_model, use_fb_consistency_mask=False):          # the shipped branch without the mask: its own capture
        eager = damped_model(a, b, type="test_eval")
        eager = {k: v.clone() for k, v in eager.items() if torch.is_tensor(v)}
        got = gf(a, b)
        assert "origin_occlusion_mask" not in got and len(gf._graphs) == 3
        for k, v in eager.items():
            assert torch.equal(got[k], v), k
    assert "origin_occlusion_mask" in gf(a, b) and len(gf._graphs) == 4
    with flags(damped_model, only_homo=True):
        assert gf(a, b)["flow_predictions"] is None
    gt = damped_model.graphed_test_out()
    with flags(damped_model, use_fb_consistency_mask=False):
        eager = damped_model(a, b, type="test_out")
        got = gt(a, b)
        for k in ("blend_image", "H", "mask2", "output2", "final_warp"):
            assert torch.equal(got[k], eager[k]), k
        assert "occlusion_mask" not in got
    got = gt(a, b)                              # back to the shipped branch: a second capture, the mask keys return
    assert "occlusion_mask" in got and len(gt._graphs) == 2


def test_validate_with_model_only_homo_pipelined_equals_plain(damped_model):
    from stitch_amd import evaluate as sev

    class DS:
        def __init__(self):
            self.pairs = [inputs.structured_pair(512, 512, seed=s) for s in (1, 2)]

        def __len__(self):
            return len(self.pairs)

        def __getitem__(self, i):
            return self.pairs[i][0][0], self.pairs[i][1][0]

    with flags(damped_model, only_homo=True):
        _, t_pipe = sev.validate_with_model(damped_model, DS(), pipelined=True)
        _, t_plain = sev.validate_with_model(damped_model, DS(), pipelined=False)
    assert torch.equal(t_pipe, t_plain)


def test_dead_branches_raise_and_only_homo_precedence(damped_model):
    a, b = inputs.structured_pair(512, 512, seed=7)
    a, b = a.cuda(), b.cuda()
    for kw in (dict(use_combine_h_flow=True, use_fb_consistency_mask=True), dict(test_not_use_combine_h_flow=False),
               dict(use_whole_resolution=True)):
        with flags(damped_model, **kw), pytest.raises(NotImplementedError):
            damped_model(a, b, type="test_eval" if "use_combine_h_flow" in kw else "test_out")
    damped_model.use_forward = True
    try:
        with pytest.raises(NotImplementedError):
            damped_model(a, b, type="test_eval")
        with pytest.raises(NotImplementedError):
            damped_model(a, b, type="test_out")
        with flags(damped_model, only_homo=True, use_combine_h_flow=True):
            o = damped_model(a, b, type="test_eval")
        assert o["flow_predictions"] is None and o["final_warp_output"] is o["output_H"]
    finally:
        damped_model.use_forward = False
