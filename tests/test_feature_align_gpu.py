"""feature_align through the model: with configs/last_config_features.py `predict_homo` is `ops.feature_homography`'s motion, `test_eval`
launches no network GEMM, `test_out` takes the no-mask branch with a zero residual, `inference_one_data` writes the default config's
files, the graph holders key their captures by the two sources, and with both keys at "network" every output bit is what it is
without them."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import _features_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 192, 256


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


@pytest.fixture(scope="module")
def scene():
    a, b, Hgt = ref.pair(H, W, (32, 4, 0, 0, 0), 3)
    return torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), Hgt, ref.homography(a, b)


def _model(sd, model_config_name="last_config", **keys):
    import stitch_amd
    cfg, _ = stitch_amd.load_inference_config("all_img1_with_inpaint_g12_transRef", model_config_name=model_config_name)
    for k, v in keys.items():
        cfg[k] = v
    m = stitch_amd.build_model(cfg)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def feature_model(seeded_sd):
    return _model(seeded_sd, "last_config_features")


def test_predict_homo_is_the_aligners_motion(feature_model, scene):
    from stitch_amd import FeatureAligner, ops
    a, b, Hgt, want = scene
    assert feature_model.sources() == ("features", "zero") and feature_model.eval_branch() == "only_homo"
    with GemmCount() as g:
        motion = feature_model.predict_homo(a, b)
    assert g.n == 0 and tuple(motion.shape) == (1, 4, 2)
    direct = ops.feature_homography(a, b)
    assert torch.equal(motion, direct[0]) and np.array_equal(motion.cpu().numpy(), want["motion"])
    assert np.array_equal(feature_model.feature_aligner().last_info.cpu().numpy(), want["info"]) and want["info"][0, 0] == 1
    assert torch.equal(FeatureAligner(max_hyp=64, seed=5).motion(a, b), ops.feature_homography(a, b, max_hyp=64, seed=5)[0])
    Hd = torch.empty((1, 3, 3), device="cuda")                                     # dlt4 of the motion gives H back, to rounding
    ops.dlt4(feature_model._corners(a.device, float(W), float(H)), motion.contiguous(), Hd, 1, 1.0, 1.0, 1.0)
    assert np.abs(Hd.cpu().numpy() / Hd[0, 2, 2].item() - want["H"]).max() < 1e-4 * np.abs(want["H"]).max()


def test_eval_launches_no_network_gemm_and_lands_on_image_1(feature_model, scene, seeded_sd):
    a, b, Hgt, want = scene
    with GemmCount() as g:
        o = feature_model(a, b, type="test_eval")
    torch.cuda.synchronize()
    assert g.n == 0
    assert sorted(o) == ["H", "final_warp_output", "flow_predictions", "output_H", "output_H_inv", "overlap"]
    assert o["flow_predictions"] is None and o["overlap"] is None and o["final_warp_output"] is o["output_H"]
    # the direction, through st_dlt4 and st_homo_warp: image 2 warped by the motion lands on image 1
    warped, ones = o["output_H"][0, 0].cpu().numpy().astype(np.float64), o["output_H"][0, 3].cpu().numpy() > 0.999
    g1, g2 = a[0, 0].cpu().numpy().astype(np.float64), b[0, 0].cpu().numpy().astype(np.float64)
    adj = lambda g: (g - 10.0) / 0.85                                              # noqa: E731  (the known gain and bias of image 2)
    assert ones.mean() > 0.5 and np.abs(adj(warped) - g1)[ones].mean() < np.abs(adj(g2) - g1)[ones].mean() / 3
    old = feature_model.cfg.only_homo
    feature_model.cfg.only_homo = False
    try:
        with pytest.raises(ValueError):
            feature_model(a, b, type="test_eval")
    finally:
        feature_model.cfg.only_homo = old
    with pytest.raises(ValueError):
        _model(seeded_sd, homo_source="orb").sources()


def test_out_takes_the_no_mask_branch_with_a_zero_residual(feature_model, scene, seeded_sd):
    a, b, Hgt, want = scene
    with GemmCount() as g:
        o = feature_model(a, b, type="test_out")
    assert g.n == 0
    plain = _model(seeded_sd, use_fb_consistency_mask=False)(a, b, type="test_out")
    assert sorted(o) == sorted(plain) and "occlusion_mask" not in o
    assert tuple(o["residual_flow"].shape) == (1, 2, H, W) and not o["residual_flow"].any()
    m2 = o["mask2"] > 0
    # output2 is the plain homography warp where mask2 is set -- to the rounding of the path, not bit for bit: the flow warp keeps grid_sample's
    # normalise / unnormalise round trip, which returns a pixel's own coordinate to within 4 ulp (below 2e-4 px on a canvas under 512 px), so a
    # zero flow samples at most 2e-4 x 255 grey levels per axis beside the pixel, and o2 = a (1 - m) + a' m adds a few ulp of 255: 0.1 in all
    diff = (o["output2"] - o["H_warp"]).abs()[m2]
    print(f"output2 against H_warp where mask2 is set: max |difference| {diff.max().item():.3e} grey levels over {int(m2.sum())} values")
    assert m2.any() and max(o["out_width"], o["out_height"]) < 512 and diff.max().item() <= 0.1
    assert o["out_width"] >= W and o["out_height"] >= H
    got = feature_model.graphed_test_out()(a, b)
    for k in ("blend_image", "H", "mask2", "output2", "final_warp"):
        assert torch.equal(got[k], o[k]), k


def test_graph_holders_key_their_captures_by_the_sources(feature_model):
    a, b = (torch.from_numpy(t).cuda() for t in ref.pair(512, 512, ref.MOTIONS[0], 3)[:2])        # (the network's input size)
    gf = feature_model.graphed("test_eval")
    eager = feature_model(a, b, type="test_eval")
    got = gf(a, b)
    assert torch.equal(got["H"], eager["H"]) and torch.equal(got["output_H"], eager["output_H"])
    feature_model.cfg.homo_source = "network"
    try:
        net = gf(a, b)
        assert len(gf._graphs) == 2 and not torch.equal(net["H"], eager["H"])
    finally:
        feature_model.cfg.homo_source = "features"
    again = gf(a.flip(3).contiguous(), b.flip(3).contiguous())                     # a replay on other pixels
    assert len(gf._graphs) == 2 and torch.equal(again["H"], feature_model(a.flip(3).contiguous(), b.flip(3).contiguous(), type="test_eval")["H"])


def test_graphs_of_one_aligner_replay_side_by_side(scene):
    """two captures of one aligner share no workspace: replayed together on two streams, each gives its own eager result"""
    from stitch_amd import FeatureAligner
    a, b, _, want = scene
    pairs = [(a.clone(), b.clone()), (a.flip(3).contiguous(), b.flip(3).contiguous())]
    aligner = FeatureAligner()
    graphs, outs, spaces = [], [], []
    for x, y in pairs:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            spaces.append(aligner.workspace(x.device, 1, H, W).data_ptr())
            outs.append(aligner.homography(x, y))
        graphs.append(g)
    assert not aligner._ws and spaces[0] != spaces[1]               # nothing cached under the shared capture stream
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(5):
        for g, s in zip(graphs, streams):
            with torch.cuda.stream(s):
                g.replay()
    torch.cuda.synchronize()
    eager = [aligner.homography(x, y) for x, y in pairs]
    assert len(aligner._ws) == 1
    for got, exp in zip(outs, eager):
        for g, e in zip(got, exp):
            assert torch.equal(g, e)
    assert np.array_equal(outs[0][0].cpu().numpy(), want["motion"]) and not torch.equal(outs[0][0], outs[1][0])


def test_default_keys_change_no_bit(seeded_sd):
    from stitch_amd.data import structured_pair
    a, b = (t.cuda() for t in structured_pair(512, 512, seed=7))                      # (the network's input size)
    absent, named = _model(seeded_sd), _model(seeded_sd, homo_source="network", flow_source="network")
    assert "homo_source" not in absent.cfg and absent.sources() == named.sources() == ("network", "network")
    with GemmCount() as g0:
        o0 = absent(a, b, type="test_eval")
    with GemmCount() as g1:
        o1 = named(a, b, type="test_eval")
    assert g0.n == g1.n > 0 and sorted(o0) == sorted(o1)
    for k, v in o0.items():
        if torch.is_tensor(v):
            assert torch.equal(v, o1[k]), k
    assert torch.equal(o0["flow_predictions"][0], o1["flow_predictions"][0])


def test_out_py_writes_the_default_configs_files(tmp_path, seeded_sd, scene):
    from PIL import Image
    import stitch_amd
    spec_ = importlib.util.spec_from_file_location("stitch_out_harness_features", os.path.join(ROOT, "out.py"))
    outmod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(outmod)
    root = tmp_path / "demo"
    (root / "p0").mkdir(parents=True)
    for name, t in (("input1.jpg", scene[0]), ("input2.jpg", scene[1])):
        Image.fromarray(t[0].permute(1, 2, 0).cpu().numpy().astype(np.uint8)).save(str(root / "p0" / name), quality=97)
    (root / "demo.txt").write_text("p0/\n")
    files = {}
    for tag, name in (("features", "last_config_features"), ("default", "last_config")):
        cfg = outmod.get_config(["--data_root_path", str(root) + "/", "--inf_cfg", "inpaint_all_area_g12_cv", "--model_config_name", name])
        model = stitch_amd.build_model(cfg)
        if tag == "default":
            model.load_state_dict(seeded_sd, strict=True)                           # (the features run reads no network weight: random init)
        model = model.cuda().eval()
        todo = outmod.get_data_dict_list(cfg.data_root_path, cfg.txt_file)
        save = str(tmp_path / tag) + "/"
        os.makedirs(save)
        with GemmCount() as g:
            outmod.inference_one_data(cfg, todo[0], save, model, None, outmod.load_inpainter("cv_inpainter"))
        assert (g.n == 0) == (tag == "features")
        files[tag] = sorted(os.listdir(save + "p0"))
    assert files["features"] == files["default"] and "ave_fusion.jpg" in files["features"]
