"""dense_flow through the model: with configs/last_config_classical.py `test_eval` runs its whole shipped path -- homography from features, the
Lucas-Kanade residual in both directions, flow warp, range map, occlusion mask -- without launching a network GEMM, and every tensor it
returns equals the same chain of ops called by hand; `test_out` takes the consistency-mask branch with a non-zero residual,
`inference_one_data` writes the default config's files, the graph holders key their captures by the two sources, two graphs of one
`DenseFlow` replay side by side, and with both keys at "network" every output bit is what it is without them."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _dense_flow_ref as ref
from test_feature_align_gpu import GemmCount, _model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 192, 256


@pytest.fixture(scope="module")
def scene():
    a, b = ref.homography_residual_pair(H, W)
    return torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()


@pytest.fixture(scope="module")
def classical_model(seeded_sd):
    return _model(seeded_sd, "last_config_classical")


def test_eval_equals_the_chain_of_ops_and_launches_no_gemm(classical_model, scene):
    from stitch_amd import ops
    a, b = scene
    m = classical_model
    assert m.sources() == ("features", "dense_lk") and m.eval_branch() == "shipped"
    with GemmCount() as g:
        o = m(a, b, type="test_eval")
    torch.cuda.synchronize()
    assert g.n == 0
    assert sorted(o) == ["H", "final_warp_output", "flow_predictions", "origin_occlusion_mask", "output_H", "output_H_inv", "overlap"]
    output_H = o["output_H"]
    flow = ops.dense_flow(a, output_H[:, :3], mask2=output_H[:, 3:4])[0]
    assert len(o["flow_predictions"]) == 1 and torch.equal(o["flow_predictions"][0], flow) and flow.abs().max().item() > 1
    # the chain by hand
    motion = ops.feature_homography(a, b)[0]
    Hm = torch.empty((1, 3, 3), device="cuda")
    ops.dlt4(m._corners(a.device, W, H), motion.contiguous(), Hm, 1, 1.0, 1.0, 8.0)
    M, Minv = m._scale_pair(a.device, W / 8, H / 8)
    H_mat, H_inv_mat = torch.empty_like(Hm), torch.empty_like(Hm)
    ops.mat3_sandwich(Minv, Hm, M, H_mat)
    ops.mat3_sandwich(Minv, Hm, M, H_inv_mat, invert=True)
    want_H = ops.homo_warp(b, H_mat.view(1, 9), (H, W), n_ones=3)
    want_Hinv = ops.homo_warp(a, H_inv_mat.view(1, 9), (H, W), n_ones=3)
    warp2 = want_H[:, 0:3].contiguous()
    back = ops.dense_flow(warp2, a, mask1=want_H[:, 3:4])[0]
    final = ops.flow_warp(want_H, flow)
    occ = ops.occlusion_from_range(ops.range_map(back.contiguous()), True)
    overlap = ops.eval_finish(final, occ)
    for k, want in (("H", Hm), ("output_H", want_H), ("output_H_inv", want_Hinv), ("final_warp_output", final), ("overlap", overlap),
                    ("origin_occlusion_mask", occ.squeeze(1))):
        assert torch.equal(o[k], want), k
    assert 0 < occ.mean().item() < 1 or occ.min().item() == 1
    # the residual lands image 2 closer to image 1 than the homography alone, on the overlap
    ones = ((o["final_warp_output"][0, 3] > 0.999) & (output_H[0, 3] > 0.999)).cpu().numpy()
    g1 = a[0, 0].cpu().numpy().astype(np.float64)
    adj = lambda t: (t[0, 0].cpu().numpy().astype(np.float64) - 10.0) / 0.85                        # noqa: E731  (the known gain and bias of image 2)
    after, before = np.abs(adj(o["final_warp_output"]) - g1)[ones].mean(), np.abs(adj(output_H) - g1)[ones].mean()
    print(f"mean |difference| to image 1 on the overlap ({ones.mean():.2f} of the frame): homography {before:.3f}, homography + dense_lk {after:.3f}, "
          f"ratio {after / before:.3f}")
    assert ones.mean() > 0.5 and after < before


def test_eval_no_mask_and_combine_branches(classical_model, scene):
    from stitch_amd import ops
    a, b = scene
    m = classical_model
    shipped = m(a, b, type="test_eval")
    m.cfg.use_fb_consistency_mask = False
    try:
        assert m.eval_branch() == "shipped_no_mask"
        with GemmCount() as g:
            o = m(a, b, type="test_eval")
        assert g.n == 0 and "origin_occlusion_mask" not in o
        flow = shipped["flow_predictions"][0]
        final = ops.flow_warp(o["output_H"], flow)                                   # (eval_finish applies the occlusion factor to it in place: here all ones)
        overlap = ops.eval_finish(final, torch.ones((1, 1, H, W), device="cuda"))
        assert torch.equal(o["flow_predictions"][0], flow) and torch.equal(o["final_warp_output"], final) and torch.equal(o["overlap"], overlap)
        m.cfg.use_combine_h_flow = True
        assert m.eval_branch() == "combine"
        with GemmCount() as g:
            c = m(a, b, type="test_eval")
        assert g.n == 0 and torch.equal(c["flow_predictions"][0], shipped["flow_predictions"][0])
        assert torch.equal(c["final_warp_output"], ops.homo_flow_warp(b, shipped["H"], c["flow_predictions"][0])[0])
    finally:
        m.cfg.use_fb_consistency_mask = True
        m.cfg.use_combine_h_flow = False


def test_sequence_stitcher_forwards_to_the_model(classical_model, scene):
    import stitch_amd
    a, b = scene
    seq = stitch_amd.SequenceStitcher(classical_model, type="test_eval")
    want = classical_model(a, b, type="test_eval")
    for _ in range(2):                                                               # no state to carry: every call is the model's
        got = seq(a, b)
        assert torch.equal(got["final_warp_output"], want["final_warp_output"]) and torch.equal(got["flow_predictions"][0], want["flow_predictions"][0])
    assert seq.state() is None


def test_out_takes_the_consistency_mask_branch_with_a_residual(classical_model, scene, seeded_sd):
    from stitch_amd import ops
    a, b = scene
    with GemmCount() as g:
        o = classical_model(a, b, type="test_out")
    assert g.n == 0
    shipped = _model(seeded_sd)(a, b, type="test_out")
    assert sorted(o) == sorted(shipped) and "occlusion_mask" in o and "origin_occlusion_mask" in o
    assert tuple(o["residual_flow"].shape) == (1, 2, H, W) and o["residual_flow"].abs().max().item() > 0.5
    # the residual is the 512x512 flow resized exactly as FlowFormer's is (the thresholded warp mask sets the same bits as the ones-plane itself)
    a512 = ops.resize_bilinear(a, 512, 512, False)
    fwd = ops.dense_flow(a512, o["warp_input2_tensor_512"], mask2=o["warp_input2_mask"])[0]
    want = ops.resize_bilinear(fwd, H, W, True, div=(512 / float(W), 512 / float(H)))
    assert torch.equal(o["residual_flow"], want)
    got = classical_model.graphed_test_out()(a, b)
    for k in ("blend_image", "H", "mask2", "output2", "final_warp", "occlusion_mask"):
        assert torch.equal(got[k], o[k]), k


def test_graph_holders_recapture_on_a_source_flip(classical_model, scene):
    a, b = (torch.from_numpy(t).cuda() for t in ref.homography_residual_pair(512, 512))              # (the network's input size)
    m = classical_model
    gf = m.graphed("test_eval")
    eager = m(a, b, type="test_eval")
    got = gf(a, b)
    assert torch.equal(got["final_warp_output"], eager["final_warp_output"]) and torch.equal(got["flow_predictions"][0], eager["flow_predictions"][0])
    m.cfg.flow_source = "network"
    try:
        net = gf(a, b)
        assert len(gf._graphs) == 2 and not torch.equal(net["flow_predictions"][0], eager["flow_predictions"][0])
    finally:
        m.cfg.flow_source = "dense_lk"
    af, bf = a.flip(3).contiguous(), b.flip(3).contiguous()
    again = gf(af, bf)                                                               # a replay on other pixels
    assert len(gf._graphs) == 2 and torch.equal(again["final_warp_output"], m(af, bf, type="test_eval")["final_warp_output"])


def test_graphs_of_one_dense_flow_replay_side_by_side(scene):
    """two captures of one DenseFlow share no workspace: replayed together on two streams, each gives its own eager result"""
    from stitch_amd import DenseFlow
    a, b = scene
    pairs = [(a.clone(), b.clone()), (a.flip(3).contiguous(), b.flip(3).contiguous())]
    lk = DenseFlow()
    graphs, outs, spaces = [], [], []
    for x, y in pairs:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            spaces.append(lk.workspace(x.device, 1, H, W).data_ptr())
            outs.append(lk.flow_and_support(x, y))
        graphs.append(g)
    assert not lk._ws and spaces[0] != spaces[1]                    # nothing cached under the shared capture stream
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(5):
        for g, s in zip(graphs, streams):
            with torch.cuda.stream(s):
                g.replay()
    torch.cuda.synchronize()
    eager = [lk.flow_and_support(x, y) for x, y in pairs]
    assert len(lk._ws) == 1
    for got, exp in zip(outs, eager):
        for g, e in zip(got, exp):
            assert torch.equal(g, e)
    want = ref.dense_flow(a[0].cpu().numpy(), b[0].cpu().numpy())
    assert np.array_equal(outs[0][0][0].cpu().numpy(), want[0]) and not torch.equal(outs[0][0], outs[1][0])


def test_default_keys_change_no_bit(seeded_sd):
    from stitch_amd.data import structured_pair
    a, b = (t.cuda() for t in structured_pair(512, 512, seed=7))                      # (the network's input size)
    absent, named = _model(seeded_sd), _model(seeded_sd, flow_source="network")
    assert "flow_source" not in absent.cfg and absent.sources() == named.sources() == ("network", "network")
    with GemmCount() as g0:
        o0 = absent(a, b, type="test_eval")
    with GemmCount() as g1:
        o1 = named(a, b, type="test_eval")
    assert g0.n == g1.n > 0 and sorted(o0) == sorted(o1)
    for k, v in o0.items():
        if torch.is_tensor(v):
            assert torch.equal(v, o1[k]), k
    assert torch.equal(o0["flow_predictions"][0], o1["flow_predictions"][0])
    with pytest.raises(ValueError):
        _model(seeded_sd, flow_source="farneback").sources()


def test_out_py_writes_the_default_configs_files(tmp_path, seeded_sd, scene):
    from PIL import Image
    import stitch_amd
    spec_ = importlib.util.spec_from_file_location("stitch_out_harness_classical", os.path.join(ROOT, "out.py"))
    outmod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(outmod)
    root = tmp_path / "demo"
    (root / "p0").mkdir(parents=True)
    for name, t in (("input1.jpg", scene[0]), ("input2.jpg", scene[1])):
        Image.fromarray(t[0].permute(1, 2, 0).cpu().numpy().astype(np.uint8)).save(str(root / "p0" / name), quality=97)
    (root / "demo.txt").write_text("p0/\n")
    files = {}
    for tag, name in (("classical", "last_config_classical"), ("default", "last_config")):
        cfg = outmod.get_config(["--data_root_path", str(root) + "/", "--inf_cfg", "inpaint_all_area_g12_cv", "--model_config_name", name])
        model = stitch_amd.build_model(cfg)
        if tag == "default":
            model.load_state_dict(seeded_sd, strict=True)                           # (the classical run reads no network weight: random init)
        model = model.cuda().eval()
        todo = outmod.get_data_dict_list(cfg.data_root_path, cfg.txt_file)
        save = str(tmp_path / tag) + "/"
        print(f"[{tag}]")
        os.makedirs(save)
        with GemmCount() as g:
            outmod.inference_one_data(cfg, todo[0], save, model, None, outmod.load_inpainter("cv_inpainter"))
        assert (g.n == 0) == (tag == "classical")
        files[tag] = sorted(os.listdir(save + "p0"))
    assert files["classical"] == files["default"] and "ave_fusion.jpg" in files["classical"]
