"""csrc/seam.hip on the GPU: `ops.seam_cost` and `ops.seam_dp` equal the CPU restatement (tests/_seam_ref.py) bit for bit -- side, path and
info -- whatever the stream, the workspace's history or a hipGraph replay; `ops.multiband_blend(seam=...)` equals the restated blend along
that seam; `out.py --seam dp` changes `multiband_fusion.jpg` and nothing else."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _multiband_ref as mb
import _seam_ref as ref
from _multiband_cases import mask_cases, noise_pair, quads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(o, f) for o in ("auto", "vertical", "horizontal") for f in ("auto", 1, 2)]


def _dev(arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda()[None] for a in arrs]


def _check(img1, img2, k1, k2, modes=MODES, tag=""):
    """cost once, then side, path and info under every (orientation, first) of `modes`"""
    from stitch_amd import ops
    t = _dev((img1, img2, k1, k2))
    cost = ops.seam_cost(*t)
    assert cost.dtype == torch.int32 and np.array_equal(cost.cpu().numpy(), ref.cost(img1, img2, k1, k2)), tag
    for o, f in modes:
        want_side, want_info, want_path = ref.seam(img1, img2, k1, k2, o, f)
        side, info, path = ops.seam_dp(*t, orientation=o, first=f, return_path=True)
        assert side.dtype == torch.uint8 and info.dtype == torch.int32 and path.dtype == torch.int32
        assert info.cpu().numpy().tolist() == want_info.tolist(), (tag, o, f)
        assert np.array_equal(path.cpu().numpy(), want_path), (tag, o, f)
        assert np.array_equal(side.cpu().numpy(), want_side), (tag, o, f)
        side2, info2 = ops.seam_dp(*t, orientation=o, first=f)
        assert torch.equal(side2, side) and torch.equal(info2, info)


def _two_masks(H, W):
    ones = np.ones((1, H, W), np.float32)
    return {"ones": (ones, ones.copy()), "quads": quads(H, W)}


@pytest.mark.parametrize("size", [(1, 1), (1, 7), (7, 1), (2, 2), (5, 63), (5, 64), (5, 65), (5, 255), (5, 256), (5, 257), (5, 1023), (5, 1024), (5, 1025),
                                  (3, 4096), (4096, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes_at_the_wave_and_workgroup_widths(size):
    """a thread owns four positions, a wave 256: lines of 63 / 64 / 65 (one wave), 255 / 256 / 257 (the wave border), 1023 / 1024 / 1025 (four
    waves and one position into the fifth), 4096 (the longest line, 16 waves) -- as rows (vertical) and, with the orientation fixed the other
    way, as 5 positions over that many lines; 4096 lines is the longest walk"""
    H, W = size
    img1, img2 = noise_pair(H, W, 41)
    for name, (k1, k2) in _two_masks(H, W).items():
        _check(img1, img2, k1, k2, tag=name)


@pytest.mark.parametrize("lines", [63, 64, 65, 127, 128, 129])
def test_line_counts_round_the_backtrack_chunk(lines):
    """the backtrack walks chunks of 64 lines from the last line up; the DP prefetches four lines at a time (63 = 3 mod 4, 65 = 1 mod 4)"""
    for H, W in ((lines, 9), (9, lines)):
        img1, img2 = noise_pair(H, W, 42)
        for name, (k1, k2) in _two_masks(H, W).items():
            _check(img1, img2, k1, k2, modes=[("auto", "auto"), ("vertical", 1), ("horizontal", 2)], tag=name)


@pytest.mark.parametrize("kind", ["noise", "constant"])
def test_every_mask_arrangement(kind):
    """noise holds fractions and values outside 0..255; constant images are all ties inside the overlap"""
    H, W = 33, 47
    img1, img2 = noise_pair(H, W, 43)
    if kind == "constant":
        img1, img2 = np.full_like(img1, 90.5), np.full_like(img2, 17.25)
    else:
        assert img1.min() < 0 and img1.max() > 255 and (img1 != np.trunc(img1)).any()
    for name, (k1, k2) in mask_cases(H, W).items():
        _check(img1, img2, k1, k2, tag=name)
        _check(img1, img2, k2, k1, modes=[("auto", "auto")], tag=name + " swapped")
        _check(img1, img2, np.ascontiguousarray(k1[:, ::-1, ::-1]), np.ascontiguousarray(k2[:, ::-1, ::-1]), modes=[("auto", "auto")], tag=name + " mirrored")


def test_ghost_scene_and_the_corridor_across_chunk_borders():
    for framed in (False, True):
        _check(*ref.ghost_scene(framed=framed)[:4], modes=[("auto", "auto"), ("horizontal", 2)], tag=f"ghost {framed}")
    for orient in ("vertical", "horizontal"):                       # 300 lines: the window drifts 63 positions per chunk, and turns round
        img1, img2, k1, k2, c = ref.corridor_scene(300, 100, 3, orient)
        _check(img1, img2, k1, k2, modes=[(orient, 1), ("auto", 2)], tag=f"corridor {orient}")
        from stitch_amd import ops
        _, info, path = ops.seam_dp(*_dev((img1, img2, k1, k2)), orientation=orient, first=1, return_path=True)
        assert np.array_equal(path.cpu().numpy()[:300], c) and info.cpu().numpy()[3] == 300


def test_three_channel_and_soft_masks():
    from stitch_amd import ops
    H, W = 17, 33
    img1, img2 = noise_pair(H, W, 44)
    k1, k2 = quads(H, W)
    rng = np.random.default_rng(45)
    k1_3 = np.concatenate([k1, rng.random((2, H, W)).astype(np.float32)])
    soft = np.where(k2 > 0.5, 0.500001, 0.5).astype(np.float32)
    want_side, want_info, _ = ref.seam(img1, img2, k1, k2)
    for a, b in ((k1_3, k2), (k1_3, soft), (k1, soft)):
        side, info = ops.seam_dp(*_dev((img1, img2, a, b)))
        assert np.array_equal(side.cpu().numpy(), want_side) and info.cpu().numpy().tolist() == want_info.tolist()
        assert np.array_equal(ops.seam_cost(*_dev((img1, img2, a, b))).cpu().numpy(), ref.cost(img1, img2, k1, k2))
    t = _dev((img1, img2, k1, k2))
    with pytest.raises(ValueError):
        ops.seam_dp(*t, orientation="diagonal")
    with pytest.raises(ValueError):
        ops.seam_dp(*t, first=3)
    with pytest.raises(ValueError):
        ops.seam_dp(t[0], t[1], t[2], t[3][..., :-1])


@pytest.fixture(scope="module")
def two_cases():
    """a larger and a smaller canvas with their expected seams (auto)"""
    big = noise_pair(95, 130, 51) + quads(95, 130)
    small = noise_pair(17, 33, 52) + tuple(np.ascontiguousarray(k.transpose(0, 2, 1)) for k in quads(33, 17))
    return big, ref.seam(*big), small, ref.seam(*small)


def _same(got, want):
    return all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))


def test_streams_and_workspace_history(two_cases):
    from stitch_amd import ops
    big, want_big, small, want_small = two_cases
    assert want_big[1][1] == ref.VERTICAL and want_small[1][1] == ref.HORIZONTAL
    tb, ts = _dev(big), _dev(small)
    need = ops.seam_workspace_bytes(95, 130)
    ws1 = torch.full((need,), 255, dtype=torch.uint8).cuda()
    ws2 = torch.full((need,), 255, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):                                                     # a side stream; two calls in flight in separate workspaces
        r1 = ops.seam_dp(*tb, workspace=ws1, return_path=True)
    with torch.cuda.stream(s2):
        r2 = ops.seam_dp(*ts, workspace=ws2, return_path=True)
    with torch.cuda.stream(s1):                                                     # the workspace just held the larger canvas
        r3 = ops.seam_dp(*ts, workspace=ws1, return_path=True)
    s1.synchronize(), s2.synchronize()
    assert _same(r1, want_big) and _same(r2, want_small) and _same(r3, want_small)
    with pytest.raises(ops.StitchErrorBase):
        ops.seam_dp(*tb, workspace=ws1[:4096])


def test_seam_and_blend_captured_into_a_graph_replay_on_other_pixels(two_cases):
    from stitch_amd import ops
    big, want_big, _, _ = two_cases
    other = noise_pair(95, 130, 53) + tuple(np.ascontiguousarray(k[:, ::-1]) for k in quads(95, 130))
    static = _dev(big)
    ws = torch.empty(ops.seam_workspace_bytes(95, 130), dtype=torch.uint8).cuda()
    wsb = torch.empty(ops.multiband_workspace_bytes(95, 130, 3), dtype=torch.uint8).cuda()
    side_stream = torch.cuda.Stream()
    side_stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side_stream):
        ops.multiband_blend(*static, levels=3, workspace=wsb, seam=ops.seam_dp(*static, workspace=ws))
    torch.cuda.current_stream().wait_stream(side_stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = ops.seam_dp(*static, workspace=ws, return_path=True)
        out = ops.multiband_blend(*static, levels=3, workspace=wsb, seam=res[:2])
    graph.replay()
    torch.cuda.synchronize()
    assert _same(res, want_big)
    assert np.array_equal(out[0].cpu().numpy(), ref.blend(*big, 3, want_big[:2]))
    for t, a in zip(static, other):
        t.copy_(torch.from_numpy(a)[None])
    graph.replay()
    torch.cuda.synchronize()
    want = ref.seam(*other)
    assert _same(res, want)
    assert np.array_equal(out[0].cpu().numpy(), ref.blend(*other, 3, want[:2]))


@pytest.mark.parametrize("levels", [0, 2, 5])
def test_blend_along_the_seam_equals_the_restatement(levels):
    """every mask arrangement; where the seam is not valid (info[0] = 0, decided on the device) the blend is `multiband_blend` without one,
    bit for bit"""
    from stitch_amd import ops
    H, W = 64, 48
    img1, img2 = noise_pair(H, W, 54)
    seen = set()
    for name, (k1, k2) in mask_cases(H, W).items():
        for o, f in (("auto", "auto"), ("horizontal", 2)):
            t = _dev((img1, img2, k1, k2))
            seam = ops.seam_dp(*t, orientation=o, first=f)
            want_seam = ref.seam(img1, img2, k1, k2, o, f)
            got = ops.multiband_blend(*t, levels=levels, seam=seam)
            assert got.dtype == torch.float32 and got.shape == (1, 3, H, W)
            assert np.array_equal(got[0].cpu().numpy(), ref.blend(img1, img2, k1, k2, levels, want_seam[:2])), (name, o, f)
            plain = ops.multiband_blend(*t, levels=levels)
            assert np.array_equal(plain[0].cpu().numpy(), mb.blend(img1, img2, k1, k2, levels)), name      # the call without a seam keeps its bits
            valid = int(want_seam[1][0])
            seen.add(valid)
            if not valid:
                assert torch.equal(got, plain), (name, o, f)
    assert seen == {0, 1}
    t = _dev((img1, img2) + quads(H, W))
    side, info = ops.seam_dp(*t)
    with pytest.raises(ValueError):
        ops.multiband_blend(*t, levels=levels, seam=(side[:-1], info))
    with pytest.raises(ValueError):
        ops.multiband_blend(*t, levels=levels, seam=(side.float(), info))


def test_out_py_blends_along_the_seam_and_leaves_the_other_ten(tmp_path, seeded_sd):
    """one synthetic pair at 96x128 through `inference_one_data`: without the flag, with multiband=5, and with seam="dp" on top"""
    from PIL import Image
    import stitch_amd
    from stitch_amd.data import structured_pair
    spec_ = importlib.util.spec_from_file_location("stitch_out_harness_seam", os.path.join(ROOT, "out.py"))
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
    assert "seam" not in dict(cfg) and outmod.seam_of(cfg) is None                  # config.txt stays what it was
    assert "seam" not in dict(outmod.get_config(base + ["--multiband_fusion"]))
    assert outmod.seam_of(outmod.get_config(base + ["--multiband_fusion", "--seam", "dp"])) == "dp"
    with pytest.raises(SystemExit):
        outmod.get_config(base + ["--seam", "dp"])
    todo = outmod.get_data_dict_list(cfg.data_root_path, cfg.txt_file)
    model = stitch_amd.build_model(cfg)
    model.load_state_dict(seeded_sd, strict=True)
    model = model.cuda().eval()
    comp = stitch_amd.composition.Network().cuda().eval()
    inp = outmod.load_inpainter("passthrough_inpainter")
    with pytest.raises(ValueError):
        outmod.inference_one_data(cfg, todo[0], str(tmp_path / "bad") + "/", model, comp, inp, seam="dp")
    dirs, outs = {}, {}
    for tag, kw in (("off", {}), ("mb", dict(multiband=5)), ("dp", dict(multiband=5, seam="dp")), ("dp_gpu", dict(multiband=5, seam="dp", gpu_jpeg=True)),
                    ("dp_ec", dict(multiband=5, seam="dp", exposure=("gain", 32)))):
        dirs[tag] = str(tmp_path / tag) + "/"
        os.makedirs(dirs[tag])
        outs[tag], _ = outmod.inference_one_data(cfg, todo[0], dirs[tag], model, comp, inp, **kw)
    ten = sorted(os.listdir(dirs["off"] + "p0"))
    read = lambda tag, f: open(dirs[tag] + "p0/" + f, "rb").read()                 # noqa: E731
    assert len(ten) == 10 and "seam_side" not in outs["off"] and "seam_side" not in outs["mb"]
    ops = stitch_amd.ops
    for tag in ("mb", "dp", "dp_gpu", "dp_ec"):
        assert sorted(os.listdir(dirs[tag] + "p0")) == sorted(ten + ["multiband_fusion.jpg"])
        for f in ten:
            assert read(tag, f) == read("off", f), (tag, f)
    o = outs["mb"]
    plain = ops.multiband_blend(o["output1"].float().contiguous(), o["output2"].float().contiguous(), o["mask1"].float(), o["mask2"].float(), levels=5)
    assert torch.equal(plain, o["multiband_image"])                                 # without the flag: the blend it was
    for tag in ("dp", "dp_gpu", "dp_ec"):
        o = outs[tag]
        img1, img2 = (o["compensated1"], o["compensated2"]) if tag == "dp_ec" else (o["output1"].float().contiguous(), o["output2"].float().contiguous())
        k1, k2 = o["mask1"].float(), o["mask2"].float()
        n = [t[0].cpu().numpy() for t in (img1, img2, k1, k2)]
        want_side, want_info, _ = ref.seam(*n)
        assert np.array_equal(o["seam_side"].cpu().numpy(), want_side) and o["seam_info"].cpu().numpy().tolist() == want_info.tolist(), tag
        print(f"out.py pair, {tag}: seam info {want_info.tolist()}")
        if not want_info[0]:                                                        # (the seeded model's masks decide; both ways are asserted)
            assert torch.equal(o["multiband_image"], ops.multiband_blend(img1, img2, k1, k2, levels=5)), tag
        assert np.array_equal(o["multiband_image"][0].cpu().numpy(), ref.blend(*n, 5, (want_side, want_info))), tag
        saver = outmod._Saver(gpu_jpeg=tag == "dp_gpu")
        saver.image(o["multiband_image"], dirs[tag] + "again.jpg")
        saver.wait()
        assert open(dirs[tag] + "again.jpg", "rb").read() == read(tag, "multiband_fusion.jpg"), tag
    assert read("dp", "multiband_fusion.jpg") == read("dp_gpu", "multiband_fusion.jpg")
    saver = outmod._Saver()
    saver.image(plain, dirs["mb"] + "again.jpg")
    saver.wait()
    assert open(dirs["mb"] + "again.jpg", "rb").read() == read("mb", "multiband_fusion.jpg")
