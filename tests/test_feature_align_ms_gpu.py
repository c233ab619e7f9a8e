"""feature_align_ms through the model, on a pair whose second image is rolled by a quarter turn: with configs/last_config_classical_ms.py
`predict_homo` is `ops.feature_homography_ms`'s motion, `st_dlt4` gives its H back, `test_eval` launches no network GEMM and lands image 2 on
image 1 where configs/last_config_classical.py finds no model and stays unaligned; `FeatureAligner()` with default arguments is what it was;
two graphs of one multi-scale aligner replay side by side."""
import numpy as np
import pytest
import torch

import _features_ms_ref as ms
import _features_ref as ref
from test_feature_align_gpu import GemmCount, _model

pytestmark = pytest.mark.gpu

H, W = 192, 256


@pytest.fixture(scope="module")
def scene():
    a, b, Hgt = ref.pair(H, W, (10, 5, 90, 0, 0), 3)
    return torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), Hgt, ms.homography(a, b)


@pytest.fixture(scope="module")
def ms_model(seeded_sd):
    return _model(seeded_sd, "last_config_classical_ms")


def test_predict_homo_is_the_multiscale_motion(ms_model, scene):
    from stitch_amd import FeatureAligner, ops
    a, b, Hgt, want = scene
    assert ms_model.sources() == ("features", "dense_lk") and ms_model.eval_branch() == "shipped"
    aligner = ms_model.feature_aligner()
    assert aligner.multiscale and aligner.levels == 6 and aligner.oriented
    with GemmCount() as g:
        motion = ms_model.predict_homo(a, b)
    assert g.n == 0 and tuple(motion.shape) == (1, 4, 2)
    direct = ops.feature_homography_ms(a, b)
    assert torch.equal(motion, direct[0]) and np.array_equal(motion.cpu().numpy(), want["motion"])
    assert np.array_equal(aligner.last_info.cpu().numpy(), want["info"]) and want["info"][0, 0] == 1
    assert ref.corner_error(direct[1][0].cpu().numpy(), Hgt, H, W) < 3 * 0.486            # (tests/test_features_ms_cpu.py, MEASURED)
    got = FeatureAligner(max_hyp=64, seed=5, multiscale=True, levels=3, oriented=False).motion(a, b)
    assert torch.equal(got, ops.feature_homography_ms(a, b, max_hyp=64, seed=5, levels=3, oriented=False)[0])
    Hd = torch.empty((1, 3, 3), device="cuda")                                     # dlt4 of the motion gives H back, to rounding
    ops.dlt4(ms_model._corners(a.device, float(W), float(H)), motion.contiguous(), Hd, 1, 1.0, 1.0, 1.0)
    assert np.abs(Hd.cpu().numpy() / Hd[0, 2, 2].item() - want["H"]).max() < 1e-4 * np.abs(want["H"]).max()


def test_eval_launches_no_gemm_and_aligns_what_the_single_scale_config_cannot(ms_model, scene, seeded_sd):
    a, b, Hgt, want = scene
    with GemmCount() as g:
        o = ms_model(a, b, type="test_eval")
    torch.cuda.synchronize()
    assert g.n == 0
    classical = _model(seeded_sd, "last_config_classical")
    c = classical(a, b, type="test_eval")
    assert sorted(o) == sorted(c)
    info = classical.feature_aligner().last_info.cpu().numpy()
    assert info[0, 0] == 0 and not classical.feature_aligner().multiscale                # no model: the identity, image 2 as it is
    g1 = a[0, 0].cpu().numpy().astype(np.float64)
    adj = lambda t: (t[0, 0].cpu().numpy().astype(np.float64) - 10.0) / 0.85              # noqa: E731  (the known gain and bias of image 2)
    on = (o["final_warp_output"][0, 3] > 0.999).cpu().numpy()
    on_c = (c["output_H"][0, 3] > 0.999).cpu().numpy()
    after, before = np.abs(adj(o["final_warp_output"]) - g1)[on].mean(), np.abs(adj(c["output_H"]) - g1)[on_c].mean()
    print(f"mean |difference| to image 1 on the overlap: last_config_classical {before:.3f} ({on_c.mean():.2f} of the frame), "
          f"last_config_classical_ms {after:.3f} ({on.mean():.2f} of the frame)")
    assert on.mean() > 0.3 and after < before


def test_the_default_aligner_is_what_it_was(scene):
    from stitch_amd import FeatureAligner, ops
    a, b = (torch.from_numpy(t).cuda() for t in ref.pair(H, W, (32, 4, 0, 0, 0), 3)[:2])
    aligner = FeatureAligner()
    assert not aligner.multiscale
    got, want = aligner.homography(a, b), ops.feature_homography(a, b)
    assert all(torch.equal(g, w) for g, w in zip(got, want)) and want[2][0, 0].item() == 1
    assert aligner.workspace(a.device, 1, H, W).numel() == ops.feature_workspace_bytes(1, H, W)
    assert FeatureAligner(multiscale=True).workspace(a.device, 1, H, W).numel() == ops.feature_ms_workspace_bytes(1, H, W, 6, 2048)


def test_graphs_of_one_multiscale_aligner_replay_side_by_side(scene):
    """two captures of one aligner share no workspace: replayed together on two streams, each gives its own eager result"""
    from stitch_amd import FeatureAligner
    a, b, _, want = scene
    pairs = [(a.clone(), b.clone()), (a.flip(3).contiguous(), b.flip(3).contiguous())]
    aligner = FeatureAligner(multiscale=True)
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
