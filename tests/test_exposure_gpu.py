"""csrc/exposure.hip on the GPU: `ops.exposure_stats`, `ops.exposure_compensate` and `ops.exposure_apply` equal the CPU restatement
(tests/_exposure_ref.py) bit for bit, whatever the stream, the workspace's history, in place or in a hipGraph replay, and `out.py` feeds
the compensated pair to the multiband blend without touching the ten reference files."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _exposure_ref as ref
from _multiband_cases import mask_cases, noise_pair, quads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()[None]


def single_pixel(H, W):
    """two full masks but for one shared pixel: the overlap is that pixel"""
    k1, k2 = np.zeros((1, H, W), f32), np.zeros((1, H, W), f32)
    k1[0, :, : W // 2 + 1] = 1
    k2[0, :, W // 2:] = 1
    k1[0, 1:] *= (np.arange(W) < W // 2)[None]
    return k1, k2


def stats_masks(H, W):
    m = mask_cases(H, W)
    out = {k: m[k] for k in ("quads", "disjoint", "nested", "both_empty")}
    full = np.ones((1, H, W), f32)
    out["full"] = (full, full.copy())
    out["single"] = single_pixel(H, W)
    return out


def gain_pair(H, W, seed, gain2=0.7):
    """fractional pixels, some outside 0..255; image 2 darker and with a gradient along W, so that tile gains differ"""
    rng = np.random.default_rng(seed)
    base = rng.random((3, H, W)) * 300 - 20
    ramp = 1 + 0.3 * np.linspace(-1, 1, W)[None, None, :]
    return base.astype(f32), (base * gain2 * ramp + rng.random((3, H, W)) * 4).astype(f32)


STAT_SIZES = [(1, 1, 32), (1, 9, 32), (9, 1, 32), (7, 7, 8), (31, 33, 32), (32, 32, 32), (33, 65, 32)] + [(20, W, b) for W in (63, 64, 65) for b in (8, 16, 32, 64)]


@pytest.mark.parametrize("case", STAT_SIZES, ids=lambda c: f"{c[0]}x{c[1]}b{c[2]}")
def test_stats_equal_the_restatement(case):
    """ragged tiles, tiles narrower than a wave, widths either side of a wave; the images hold fractions and values outside 0..255"""
    from stitch_amd import ops
    H, W, block = case
    img1, img2 = noise_pair(H, W, 31)
    for name, (k1, k2) in stats_masks(H, W).items():
        got = ops.exposure_stats(dev(img1), dev(img2), dev(k1), dev(k2), block=block)
        assert got.dtype == torch.int32 and got.shape == ref.grid(H, W, block) + (9,)
        want = ref.stats(img1, img2, k1, k2, block)
        assert np.array_equal(got.cpu().numpy(), want), name
        if name == "single":
            assert want[..., 0].sum() == 1
    for b in (8, 64):                                                       # a full tile of 255: the largest sum
        white = np.full((3, 64, 64), 300.0, f32)
        one = np.ones((1, 64, 64), f32)
        got = ops.exposure_stats(dev(white), dev(white), dev(one), dev(one), block=b).cpu().numpy()
        assert (got[..., 0] == b * b).all() and (got[..., 1:] == b * b * 255).all()


def _compensate(img1, img2, k1, k2, **kw):
    from stitch_amd import ops
    o1, o2, g = ops.exposure_compensate(dev(img1), dev(img2), dev(k1), dev(k2), return_gains=True, **kw)
    assert o1.dtype == torch.float32 and o1.shape == (1,) + img1.shape and o2.shape == o1.shape and g.dtype == torch.float32
    return o1[0].cpu().numpy(), o2[0].cpu().numpy(), g.cpu().numpy()


def _same(got, want, what):
    for name, g, w in zip(("out1", "out2", "gains"), got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, np.abs(g - w).max())


@pytest.mark.parametrize("size", [(1, 1, 8), (7, 9, 8), (33, 65, 8), (40, 64, 16), (70, 100, 32), (70, 101, 8)], ids=lambda s: f"{s[0]}x{s[1]}b{s[2]}")
def test_compensate_equals_the_restatement(size):
    """gains and both outputs, both modes, channels on and off, smooth 0 / 1 / 2, min_count 0 / default, every mask arrangement; W a multiple
    of 4 (16-byte path) and not"""
    H, W, block = size
    img1, img2 = gain_pair(H, W, 41)
    for name, (k1, k2) in stats_masks(H, W).items():
        for channels in (False, True):
            _same(_compensate(img1, img2, k1, k2, mode="gain", block=block, channels=channels),
                  ref.compensate(img1, img2, k1, k2, "gain", block, channels), (name, "gain", channels))
            for smooth, min_count in ((2, None), (0, None), (1, 0), (2, 0)):
                got = _compensate(img1, img2, k1, k2, mode="blocks", block=block, channels=channels, smooth=smooth, min_count=min_count)
                want = ref.compensate(img1, img2, k1, k2, "blocks", block, channels, min_count, smooth)
                _same(got, want, (name, "blocks", channels, smooth, min_count))
    k1, k2 = quads(H, W)
    if H * W > 1000:
        t = ref.gain_tables(img1, img2, k1, k2, "blocks", block, True)
        assert len(np.unique(t)) > 10 and (np.abs(t - 1) > 0.02).any()          # (the case does exercise the solve)
    _same(_compensate(img1, img2, k1, k2, mode="blocks", block=block, sigma_n=7.0, sigma_g=1.0),
          ref.compensate(img1, img2, k1, k2, "blocks", block, sigma_n=7.0, sigma_g=1.0), "sigmas")


def test_compensate_at_the_longest_sides():
    """4096 is the longest side: 512 tiles of block 8 in a row (the global sum strides over more records than it has threads at 20 x 4096),
    one ragged tile column of block 64"""
    for H, W, block in ((3, 4096, 8), (4096, 3, 64), (20, 4096, 8)):
        img1, img2 = gain_pair(H, W, 44)
        full = np.ones((1, H, W), f32)
        half = (np.arange(W)[None, None, :] * 7 % 11 < 6).astype(f32) * full
        for mode in ("gain", "blocks"):
            _same(_compensate(img1, img2, full, half, mode=mode, block=block, min_count=0), ref.compensate(img1, img2, full, half, mode, block, False, 0),
                  (H, W, mode))


def test_compensate_edge_images_and_three_channel_masks():
    H, W = 33, 68
    img1, img2 = gain_pair(H, W, 42)
    k1, k2 = quads(H, W)
    rng = np.random.default_rng(43)
    k1_3 = np.concatenate([k1, rng.random((2, H, W)).astype(f32)])
    k2_3 = np.concatenate([k2, rng.random((2, H, W)).astype(f32)])
    for mode in ("gain", "blocks"):
        want = ref.compensate(img1, img2, k1, k2, mode, 8)
        _same(_compensate(img1, img2, k1_3, k2_3, mode=mode, block=8), want, "3-channel masks")
        soft = np.where(k1 > 0.5, 0.500001, 0.5).astype(f32)                    # set where > 0.5
        _same(_compensate(img1, img2, soft, k2, mode=mode, block=8), want, "soft mask")
        # image 1 darker than image 2 in the overlap and 255 outside it: its gain is > 1 and those pixels stay at 255 (the clamp)
        O = (k1[0] > 0.5) & (k2[0] > 0.5)
        dark = np.where(O[None], 100 + img1 / 20, 255.0).astype(f32)
        light = np.full((3, H, W), 200.0, f32)
        got = _compensate(dark, light, k1, k2, mode=mode, block=8)
        _same(got, ref.compensate(dark, light, k1, k2, mode, 8), "clamp")
        g1 = ref.interpolate(got[2][0, 0], H, W, 8)
        assert g1.min() > 1 and (got[0][:, ~O] == 255).all() and (ref.apply(dark, light, got[2], 8, frozenset({"no_final_clamp"}))[0] > 255).any()
        white = np.full((3, H, W), 255.0, f32)                                  # an all-255 image: its gain is <= 1, the other's > 1
        got = _compensate(white, light, k1, k2, mode=mode, block=8, sigma_g=1.0)
        _same(got, ref.compensate(white, light, k1, k2, mode, 8, sigma_g=1.0), "white")
        assert got[2][0, 0].max() < 1 < got[2][0, 1].min()
        black = np.zeros((3, H, W), f32)                                        # S1 = 0: image 1 keeps the prior, image 2 is pulled toward 0
        got = _compensate(black, img2, k1, k2, mode=mode, block=8)
        _same(got, ref.compensate(black, img2, k1, k2, mode, 8), "black")
        assert (got[2][0, 0] == 1).all() and (got[2][0, 1] < 1).all() and not got[0].any()
        same = _compensate(img1, img1, k1, k2, mode=mode, block=8, channels=True)
        assert (same[2] == 1).all() and np.array_equal(same[0], ref.to_u8(img1).astype(f32)) and np.array_equal(same[1], same[0])


def test_apply_on_a_planted_checkerboard_table():
    from stitch_amd import ops
    for H, W, block, th, tw in ((21, 30, 8, 3, 4), (21, 32, 8, 3, 4), (40, 64, 16, 1, 1), (9, 12, 8, 5, 6), (64, 128, 64, 1, 2)):
        img1, img2 = noise_pair(H, W, 51)
        i, j = np.mgrid[:th, :tw]
        board = np.where((i + j) % 2 == 0, 0.5, 1.75).astype(f32)
        for channels in (False, True):
            t = np.stack([np.stack([board * f32(1 + 0.25 * s), (2.25 - board) * f32(1 + 0.125 * s)]) for s in range(3 if channels else 1)]).astype(f32)
            o1, o2 = ops.exposure_apply(dev(img1), dev(img2), torch.from_numpy(t).cuda(), block=block, channels=channels)
            w1, w2 = ref.apply(img1, img2, t, block)
            assert np.array_equal(o1[0].cpu().numpy(), w1) and np.array_equal(o2[0].cpu().numpy(), w2), (H, W, block, channels)
    white = np.full((3, 8, 12), 255.0, f32)                                         # an all-255 image under a gain > 1: the clamp
    o1, o2 = ops.exposure_apply(dev(white), dev(white), torch.full((1, 2, 1, 1), 1.5).cuda(), block=8)
    assert (o1 == 255).all() and (o2 == 255).all()
    with pytest.raises(ValueError):
        ops.exposure_apply(dev(img1), dev(img2), torch.ones(3, 2, 1, 1).cuda(), block=64, channels=False)


@pytest.fixture(scope="module")
def two_cases():
    """a larger and a smaller canvas with what `blocks` at block 8 makes of them"""
    big = gain_pair(70, 100, 61) + quads(70, 100)
    small = gain_pair(17, 33, 62) + quads(17, 33)
    return big, ref.compensate(*big, "blocks", 8), small, ref.compensate(*small, "blocks", 8)


def _np(ts):
    return tuple(t.cpu().numpy()[0] if t.dim() == 4 and t.shape[0] == 1 and t.shape[1] == 3 else t.cpu().numpy() for t in ts)


def test_in_place_streams_and_workspace_history(two_cases):
    from stitch_amd import ops
    big, want_big, small, want_small = two_cases
    tb, ts = [dev(a) for a in big], [dev(a) for a in small]
    kw = dict(mode="blocks", block=8, return_gains=True)
    need = ops.exposure_workspace_bytes(70, 100, 8)
    assert need >= ops.exposure_workspace_bytes(17, 33, 8) > 0 and ops.exposure_workspace_bytes(70, 100, 12) == 0
    ws1 = torch.full((need,), 255, dtype=torch.uint8).cuda()
    ws2 = torch.full((need,), 255, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):                                                     # a side stream; two calls in flight in separate workspaces
        r1 = ops.exposure_compensate(*tb, workspace=ws1, **kw)
    with torch.cuda.stream(s2):
        r2 = ops.exposure_compensate(*ts, workspace=ws2, **kw)
    with torch.cuda.stream(s1):                                                     # the workspace just held the larger canvas
        r3 = ops.exposure_compensate(*ts, workspace=ws1, **kw)
    s1.synchronize(), s2.synchronize()
    _same(_np(r1), want_big, "side stream")
    _same(_np(r2), want_small, "second stream")
    _same(_np(r3), want_small, "workspace reuse")
    a, b = tb[0].clone(), tb[1].clone()                                             # in place: each output is its own input
    r4 = ops.exposure_compensate(a, b, tb[2], tb[3], out=(a, b), **kw)
    torch.cuda.synchronize()
    assert r4[0].data_ptr() == a.data_ptr() and r4[1].data_ptr() == b.data_ptr()
    _same(_np(r4), want_big, "in place")
    a = tb[0].clone()                                                               # one side in place, gain mode
    r5 = ops.exposure_compensate(a, tb[1], tb[2], tb[3], mode="gain", block=8, out=(a, torch.empty_like(a)), return_gains=True)
    _same(_np(r5), ref.compensate(*big, "gain", 8), "in place, gain")
    both = torch.cat([tb[0].clone(), tb[1].clone()], 1)                             # a shifted view of the input is rejected before any launch
    with pytest.raises(ops.StitchErrorBase):
        ops.exposure_compensate(both[:, :3], tb[1], tb[2], tb[3], out=(both[:, 1:4], torch.empty_like(a)), **kw)
    with pytest.raises(ops.StitchErrorBase):
        ops.exposure_compensate(*tb, workspace=ws1[:256], **kw)
    for bad in (dict(block=12), dict(mode="tiles"), dict(smooth=9), dict(min_count=-1), dict(sigma_n=0.0), dict(sigma_g=float("inf"))):
        with pytest.raises(ValueError):
            ops.exposure_compensate(*tb, **bad)


def test_compensate_captured_into_a_graph_replays_on_other_pixels(two_cases):
    from stitch_amd import ops
    big, want_big, _, _ = two_cases
    other = gain_pair(70, 100, 63, gain2=1.3) + tuple(k[:, ::-1].copy() for k in quads(70, 100))
    static = [dev(a) for a in big]
    ws = torch.empty(ops.exposure_workspace_bytes(70, 100, 8), dtype=torch.uint8).cuda()
    kw = dict(mode="blocks", block=8, return_gains=True, workspace=ws)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.exposure_compensate(*static, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.exposure_compensate(*static, **kw)
    graph.replay()
    torch.cuda.synchronize()
    _same(_np(out), want_big, "replay")
    for t, a in zip(static, other):
        t.copy_(torch.from_numpy(a)[None])
    graph.replay()
    torch.cuda.synchronize()
    _same(_np(out), ref.compensate(*other, "blocks", 8), "replay on other pixels")
    _same(_np(ops.exposure_compensate(*static, **kw)), _np(out), "eager")


def test_out_py_blends_the_compensated_pair_and_leaves_the_ten(tmp_path, seeded_sd):
    """one synthetic pair at 96x128 through `inference_one_data`: without the multiband switch, with it, and with exposure compensation"""
    from PIL import Image
    import stitch_amd
    from stitch_amd import ops
    from stitch_amd.data import structured_pair
    spec_ = importlib.util.spec_from_file_location("stitch_out_harness_ec", os.path.join(ROOT, "out.py"))
    outmod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(outmod)
    root = tmp_path / "demo"
    (root / "p0").mkdir(parents=True)
    a, b = structured_pair(96, 128, seed=3, shift=(2, -3))
    for name, t in (("input1.jpg", a), ("input2.jpg", (b * 0.8))):
        Image.fromarray(t[0].permute(1, 2, 0).numpy().astype(np.uint8)).save(str(root / "p0" / name), quality=97)
    (root / "demo.txt").write_text("p0/\n")
    base = ["--data_root_path", str(root) + "/"]
    cfg = outmod.get_config(base + ["--multiband_fusion"])
    assert "exposure_compensation" not in dict(cfg) and "exposure_block" not in dict(cfg) and outmod.exposure_of(cfg) is None      # config.txt stays what it was
    assert outmod.exposure_of(outmod.get_config(base + ["--multiband_fusion", "--exposure_compensation", "gain"])) == ("gain", 32)
    assert outmod.exposure_of(outmod.get_config(base + ["--multiband_fusion", "--exposure_compensation", "blocks", "--exposure_block", "16"])) == ("blocks", 16)
    for bad in (["--exposure_compensation", "gain"], ["--multiband_fusion", "--exposure_block", "16"],
                ["--multiband_fusion", "--exposure_compensation", "blocks", "--exposure_block", "12"], ["--multiband_fusion", "--exposure_compensation", "tiles"]):
        with pytest.raises(SystemExit):
            outmod.get_config(base + bad)
    todo = outmod.get_data_dict_list(cfg.data_root_path, cfg.txt_file)
    model = stitch_amd.build_model(cfg)
    model.load_state_dict(seeded_sd, strict=True)
    model = model.cuda().eval()
    comp = stitch_amd.composition.Network().cuda().eval()
    inp = outmod.load_inpainter("passthrough_inpainter")
    dirs, outs = {}, {}
    for tag, kw in (("off", {}), ("mb", dict(multiband=5)), ("gain", dict(multiband=5, exposure=("gain", 32))), ("blocks", dict(multiband=5, exposure=("blocks", 16)))):
        dirs[tag] = str(tmp_path / tag) + "/"
        os.makedirs(dirs[tag])
        outs[tag], _ = outmod.inference_one_data(cfg, todo[0], dirs[tag], model, comp, inp, **kw)
    with pytest.raises(ValueError):
        outmod.inference_one_data(cfg, todo[0], dirs["off"], model, comp, inp, exposure=("gain", 32))
    ten = sorted(os.listdir(dirs["off"] + "p0"))
    assert len(ten) == 10 and "compensated1" not in outs["off"] and "compensated1" not in outs["mb"]
    o = outs["mb"]                                                                  # without the flag: the blend of the uncompensated pair, as before
    args = (o["output1"].float().contiguous(), o["output2"].float().contiguous(), o["mask1"].float(), o["mask2"].float())
    saver = outmod._Saver()
    saver.image(ops.multiband_blend(*args, levels=5), dirs["mb"] + "again.jpg")
    saver.wait()
    assert open(dirs["mb"] + "again.jpg", "rb").read() == open(dirs["mb"] + "p0/multiband_fusion.jpg", "rb").read()
    for tag, (mode, block) in (("gain", ("gain", 32)), ("blocks", ("blocks", 16))):
        assert sorted(os.listdir(dirs[tag] + "p0")) == sorted(ten + ["multiband_fusion.jpg"])
        for f in ten:
            assert open(dirs[tag] + "p0/" + f, "rb").read() == open(dirs["off"] + "p0/" + f, "rb").read(), (tag, f)
        o = outs[tag]
        c1, c2, gains = ops.exposure_compensate(*args, mode=mode, block=block, return_gains=True)
        assert torch.equal(c1, o["compensated1"]) and torch.equal(c2, o["compensated2"])
        assert (gains != 1).any()                                                   # (input 2 was written at 0.8 x: there is something to compensate)
        want = ref.compensate(*(t[0].cpu().numpy() for t in args), mode, block)
        assert np.array_equal(c1[0].cpu().numpy(), want[0]) and np.array_equal(c2[0].cpu().numpy(), want[1])
        mbi = ops.multiband_blend(c1, c2, args[2], args[3], levels=5)
        assert torch.equal(mbi, o["multiband_image"])
        saver = outmod._Saver()
        saver.image(mbi, dirs[tag] + "again.jpg")
        saver.wait()
        assert open(dirs[tag] + "again.jpg", "rb").read() == open(dirs[tag] + "p0/multiband_fusion.jpg", "rb").read(), tag
        assert open(dirs[tag] + "p0/multiband_fusion.jpg", "rb").read() != open(dirs["mb"] + "p0/multiband_fusion.jpg", "rb").read(), tag
