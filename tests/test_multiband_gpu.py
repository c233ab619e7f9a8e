"""csrc/multiband.hip on the GPU: `ops.edt_sq` and `ops.multiband_blend` equal the CPU restatement (tests/_multiband_ref.py) bit for bit,
whatever the stream, the workspace's history or a hipGraph replay, and `out.py` writes `multiband_fusion.jpg` as an eleventh file without
touching the other ten."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _multiband_ref as ref
from _multiband_cases import edt_cases, mask_cases, noise_pair, quads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _edt_both_modes(name, m):
    from stitch_amd import ops
    t = torch.from_numpy(m).cuda()
    for border in (True, False):
        want_d, want_i = ref.edt_sq(m, border, True)
        d, i = ops.edt_sq(t, border_is_site=border, return_index=True)
        assert d.dtype == torch.int32 and i.dtype == torch.int32
        assert np.array_equal(d.cpu().numpy(), want_d), (name, border)
        assert np.array_equal(i.cpu().numpy(), want_i), (name, border)
        assert np.array_equal(ops.edt_sq(t, border_is_site=border).cpu().numpy(), want_d), (name, border)


def test_edt_equals_the_restatement_on_the_cpu_cases():
    for name, m in edt_cases():
        _edt_both_modes(name, m)


def test_edt_at_the_workgroup_widths_and_the_longest_sides():
    """row pass: 256 threads stride over the row (63 / 64 / 65, 255 / 256 / 257 columns); column pass: 64 columns x 16 row segments per workgroup (heights below, at and above
    16 rows; 4096 rows: 256 per segment); 4096 is the longest side; 300 x 300 all ones is the deepest outward scan (150 steps with the ring, the whole row without it)"""
    rng = np.random.default_rng(7)
    for W in (63, 64, 65, 255, 256, 257):
        for H in (1, 2, 3):
            _edt_both_modes(f"{H}x{W}", rng.random((H, W)) < 0.9)
    _edt_both_modes("2x4096", rng.random((2, 4096)) < 0.97)
    _edt_both_modes("4096x2", rng.random((4096, 2)) < 0.97)
    _edt_both_modes("300x300 ones", np.ones((300, 300), bool))


def _blend(img1, img2, k1, k2, levels, **kw):
    from stitch_amd import ops
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()[None]          # noqa: E731
    out = ops.multiband_blend(c(img1), c(img2), c(k1), c(k2), levels=levels, **kw)
    assert out.dtype == torch.float32 and out.shape == (1,) + img1.shape
    return out[0].cpu().numpy()


LEVELS = (0, 1, 2, 3, 5, 16)


@pytest.mark.parametrize("size", [(1, 1), (1, 9), (9, 1), (2, 3), (17, 33), (64, 48), (95, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_blend_equals_the_restatement(size):
    """every mask arrangement at every level count (16 is capped by the size); the images hold fractions and values outside 0..255"""
    H, W = size
    img1, img2 = noise_pair(H, W, 11)
    if H * W >= 500:
        assert img1.min() < 0 and img1.max() > 255 and (img1 != np.trunc(img1)).any()
    for name, (k1, k2) in mask_cases(H, W).items():
        for L in LEVELS:
            got = _blend(img1, img2, k1, k2, L)
            assert np.array_equal(got, ref.blend(img1, img2, k1, k2, L)), (name, L)


def test_blend_reads_channel_0_of_three_channel_masks():
    H, W = 17, 33
    img1, img2 = noise_pair(H, W, 12)
    k1, k2 = quads(H, W)
    rng = np.random.default_rng(13)
    k1_3 = np.concatenate([k1, rng.random((2, H, W)).astype(np.float32)])
    k2_3 = np.concatenate([k2, rng.random((2, H, W)).astype(np.float32)])
    want = ref.blend(img1, img2, k1, k2, 3)
    assert np.array_equal(_blend(img1, img2, k1_3, k2_3, 3), want)
    assert np.array_equal(_blend(img1, img2, k1_3, k2, 3), want)
    # soft mask values: set where > 0.5
    soft = np.where(k1 > 0.5, 0.500001, 0.5).astype(np.float32)
    assert np.array_equal(_blend(img1, img2, soft, k2, 3), want)


@pytest.fixture(scope="module")
def two_cases():
    """a larger and a smaller canvas with their expected blends at L = 3"""
    big = noise_pair(95, 130, 21) + quads(95, 130)
    small = noise_pair(17, 33, 22) + quads(17, 33)
    return big, ref.blend(*big, 3), small, ref.blend(*small, 3)


def test_streams_and_workspace_history(two_cases):
    from stitch_amd import ops
    big, want_big, small, want_small = two_cases
    c = lambda arrs: [torch.from_numpy(a).cuda()[None] for a in arrs]               # noqa: E731
    tb, ts = c(big), c(small)
    ws1 = torch.full((ops.multiband_workspace_bytes(95, 130, 3),), 255, dtype=torch.uint8).cuda()
    ws2 = torch.full((ops.multiband_workspace_bytes(95, 130, 3),), 255, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):                                                     # a side stream; two blends in flight in separate workspaces
        r1 = ops.multiband_blend(*tb, levels=3, workspace=ws1)
    with torch.cuda.stream(s2):
        r2 = ops.multiband_blend(*ts, levels=3, workspace=ws2)
    with torch.cuda.stream(s1):                                                     # the workspace just held the larger canvas
        r3 = ops.multiband_blend(*ts, levels=3, workspace=ws1)
    s1.synchronize(), s2.synchronize()
    assert np.array_equal(r1[0].cpu().numpy(), want_big)
    assert np.array_equal(r2[0].cpu().numpy(), want_small)
    assert np.array_equal(r3[0].cpu().numpy(), want_small)
    with pytest.raises(ops.StitchErrorBase):
        ops.multiband_blend(*tb, levels=3, workspace=ws1[:4096])
    with pytest.raises(ValueError):
        ops.multiband_blend(*tb, levels=17)


def test_blend_captured_into_a_graph_replays_on_other_pixels(two_cases):
    from stitch_amd import ops
    big, want_big, _, _ = two_cases
    other = noise_pair(95, 130, 23) + tuple(k[:, ::-1].copy() for k in quads(95, 130))
    static = [torch.from_numpy(a).cuda()[None] for a in big]
    ws = torch.empty(ops.multiband_workspace_bytes(95, 130, 3), dtype=torch.uint8).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.multiband_blend(*static, levels=3, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.multiband_blend(*static, levels=3, workspace=ws)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), want_big)
    for t, a in zip(static, other):
        t.copy_(torch.from_numpy(a)[None])
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), ref.blend(*other, 3))


def test_out_py_writes_an_eleventh_file_and_leaves_the_ten(tmp_path, seeded_sd):
    """one synthetic pair at 96x128 through `inference_one_data`, with and without `multiband=5`, on both savers"""
    from PIL import Image
    import stitch_amd
    from stitch_amd.data import structured_pair
    spec_ = importlib.util.spec_from_file_location("stitch_out_harness_mb", os.path.join(ROOT, "out.py"))
    outmod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(outmod)
    root = tmp_path / "demo"
    (root / "p0").mkdir(parents=True)
    a, b = structured_pair(96, 128, seed=3, shift=(2, -3))
    for name, t in (("input1.jpg", a), ("input2.jpg", b)):
        Image.fromarray(t[0].permute(1, 2, 0).numpy().astype(np.uint8)).save(str(root / "p0" / name), quality=97)
    (root / "demo.txt").write_text("p0/\n")
    base = ["--data_root_path", str(root) + "/"]
    cfg = outmod.get_config(base)
    assert "multiband_fusion" not in dict(cfg) and "multiband_levels" not in dict(cfg) and outmod.multiband_of(cfg) is None       # config.txt stays what it was
    assert outmod.multiband_of(outmod.get_config(base + ["--multiband_fusion"])) == 5
    assert outmod.multiband_of(outmod.get_config(base + ["--multiband_fusion", "--multiband_levels", "3"])) == 3
    todo = outmod.get_data_dict_list(cfg.data_root_path, cfg.txt_file)
    model = stitch_amd.build_model(cfg)
    model.load_state_dict(seeded_sd, strict=True)
    model = model.cuda().eval()
    comp = stitch_amd.composition.Network().cuda().eval()
    inp = outmod.load_inpainter("passthrough_inpainter")
    dirs, outs = {}, {}
    for tag, kw in (("off", {}), ("pil", dict(multiband=5)), ("gpu", dict(multiband=5, gpu_jpeg=True))):
        dirs[tag] = str(tmp_path / tag) + "/"
        os.makedirs(dirs[tag])
        outs[tag], _ = outmod.inference_one_data(cfg, todo[0], dirs[tag], model, comp, inp, **kw)
    ten = sorted(os.listdir(dirs["off"] + "p0"))
    assert len(ten) == 10 and "multiband_fusion.jpg" not in ten and "multiband_image" not in outs["off"]
    for tag in ("pil", "gpu"):
        assert sorted(os.listdir(dirs[tag] + "p0")) == sorted(ten + ["multiband_fusion.jpg"])
        for f in ten:
            assert open(dirs[tag] + "p0/" + f, "rb").read() == open(dirs["off"] + "p0/" + f, "rb").read(), (tag, f)
        o = outs[tag]
        mb = stitch_amd.ops.multiband_blend(o["output1"].float().contiguous(), o["output2"].float().contiguous(), o["mask1"].float(),
                                            o["mask2"].float(), levels=5)
        assert torch.equal(mb, o["multiband_image"])
        saver = outmod._Saver(gpu_jpeg=tag == "gpu")
        saver.image(mb, dirs[tag] + "again.jpg")
        saver.wait()
        assert open(dirs[tag] + "again.jpg", "rb").read() == open(dirs[tag] + "p0/multiband_fusion.jpg", "rb").read(), tag
        want = ref.blend(o["output1"][0].cpu().numpy(), o["output2"][0].cpu().numpy(), o["mask1"][0].cpu().numpy(), o["mask2"][0].cpu().numpy(), 5)
        assert np.array_equal(mb[0].cpu().numpy(), want), tag
    assert open(dirs["pil"] + "p0/multiband_fusion.jpg", "rb").read() == open(dirs["gpu"] + "p0/multiband_fusion.jpg", "rb").read()
