"""csrc/seam_gc.hip on the GPU: `ops.seam_gc` equals the CPU restatement (tests/_seam_gc_ref.py, scipy's maximum flow) bit for bit -- side and
info -- and converges, whatever the shape, the masks, the stream or the workspace's history; `ops.multiband_blend(seam=...)` equals the
restated blend along that cut; `out.py --seam gc` changes `multiband_fusion.jpg` and nothing else."""
import importlib.util
import os
import warnings

import numpy as np
import pytest
import torch

import _seam_gc_ref as ref
import _seam_ref as dpref
from _multiband_cases import mask_cases, noise_pair, quads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda()[None] for a in arrs]


def _check(img1, img2, k1, k2, tag="", want=None, **kw):
    """side and info equal the restatement; the call converged"""
    from stitch_amd import ops
    want_side, want_info = want or ref.seam(img1, img2, k1, k2)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="seam_gc")
        side, info, stats = ops.seam_gc(*_dev((img1, img2, k1, k2)), return_stats=True, **kw)
    assert side.dtype == torch.uint8 and info.dtype == torch.int32 and side.shape == img1.shape[1:] and info.shape == (4,)
    print(f"seam_gc {tag} {img1.shape[1]}x{img1.shape[2]}: info {want_info.tolist()}, {stats}")
    assert stats["converged"] and stats["rounds"] < ops.SEAM_GC_MAX_ROUNDS // 8, (tag, stats)
    assert info.cpu().numpy().tolist() == want_info.tolist(), tag
    assert np.array_equal(side.cpu().numpy(), want_side), tag
    return want_side, want_info, stats


def _tr(*arrs):
    return tuple(np.ascontiguousarray(a.transpose(0, 2, 1)) for a in arrs)


@pytest.mark.parametrize("size", [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiny_canvases(size):
    """all-overlap (no seed: not valid), bands where the canvas allows them, and `quads`"""
    H, W = size
    img1, img2 = noise_pair(H, W, 71)
    ones = np.ones((1, H, W), np.float32)
    _, info, _ = _check(img1, img2, ones, ones.copy(), "ones")
    assert info[0] == 0
    _check(img1, img2, *quads(H, W), "quads")
    if W == 7:                                                              # E1, five overlap pixels, E2 in a row
        _, info, _ = _check(img1, img2, *ref.bands(H, W, 0.2, 0.8), "bands")
        assert info[0] == 1
    if H == 7:
        _, info, _ = _check(img1, img2, *ref.bands(H, W, 0.2, 0.8, transposed=True), "bands T")
        assert info[0] == 1
    if H == W == 3:                                                         # one overlap pixel between E1 and E2: all source, not valid
        k1, k2 = np.ones((1, 3, 3), np.float32), np.ones((1, 3, 3), np.float32)
        k1[0, :, 2] = 0
        k2[0, :, 0] = 0
        _, info, _ = _check(img1, img2, k1, k2, "one column")
        assert info[0] == 0


@pytest.mark.parametrize("n", [31, 32, 33, 63, 64, 65])
def test_bands_across_tile_and_wave_edges(n):
    """a tile of the relabel is 32 x 32 pixels, a workgroup of the sweeps 32 x 8: the overlap starts and ends next to, on and beyond those
    edges, along rows and along columns"""
    img1, img2 = noise_pair(5, n, 72)
    for lo, hi in ((0.1, 0.9), (0.4, 0.6)):
        k1, k2 = ref.bands(5, n, lo, hi)
        _, info, _ = _check(img1, img2, k1, k2, f"band {lo}")
        assert info[0] == 1
        _check(*_tr(img1, img2, k1, k2), f"band {lo} T")
        _check(img1, img2, k2, k1, f"band {lo} swapped")


@pytest.mark.parametrize("size", [(33, 65), (40, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["noise", "constant"])
def test_every_mask_arrangement(size, kind):
    """noise holds fractions and values outside 0..255; constant images make every cut of equal length tie"""
    H, W = size
    img1, img2 = noise_pair(H, W, 73)
    if kind == "constant":
        img1, img2 = np.full_like(img1, 90.5), np.full_like(img2, 17.25)
    else:
        assert img1.min() < 0 and img1.max() > 255 and (img1 != np.trunc(img1)).any()
    seen = set()
    for name, (k1, k2) in mask_cases(H, W).items():
        seen.add(int(_check(img1, img2, k1, k2, name)[1][0]))
        _check(img1, img2, k2, k1, name + " swapped")
        _check(img1, img2, np.ascontiguousarray(k1[:, ::-1, ::-1]), np.ascontiguousarray(k2[:, ::-1, ::-1]), name + " mirrored")
    assert seen == {0, 1}


def test_ghost_serpentine_and_l_scenes():
    for framed in (False, True):
        _check(*dpref.ghost_scene(framed=framed)[:4], f"ghost framed={framed}")
    for orientation in ("vertical", "horizontal"):
        _check(*ref.serpentine_scene(orientation)[:4], f"serpentine {orientation}")
    side, info, _ = _check(*ref.l_hole_scene(), "L with hole")
    assert info[0] == 1 and (side == 0).any()


def test_equal_images():
    H, W = 40, 56
    img = noise_pair(H, W, 74)[0]
    for name, (k1, k2) in (("quads", quads(H, W)), ("bands", ref.bands(H, W))):
        side, info, _ = _check(img, img.copy(), k1, k2, "equal " + name)
        O, E1, E2 = ref.regions(k1, k2)
        T = ref.seeds(O, E1, E2)[1]
        assert info[0] == 1 and (side[T] == 0).all()
        if name == "bands":                                                 # every cut along the band ties: the seam sits against image 2's exclusive region
            assert np.array_equal(side == 0, T)


def test_noise_bands_128x129():
    _check(*noise_pair(128, 129, 75), *ref.bands(128, 129), "noise")
    _check(*noise_pair(128, 129, 76), *ref.bands(128, 129, 0.35, 0.65, transposed=True), "noise T")


def test_smooth_and_texture_bands_256x257():
    _check(*ref.smooth_texture_pair(256, 257, 77), *ref.bands(256, 257), "smooth + texture")


def test_three_channel_and_soft_masks_and_non_finite_pixels():
    from stitch_amd import ops
    H, W = 17, 33
    img1, img2 = noise_pair(H, W, 78)
    k1, k2 = quads(H, W)
    rng = np.random.default_rng(79)
    k1_3 = np.concatenate([k1, rng.random((2, H, W)).astype(np.float32)])
    soft = np.where(k2 > 0.5, 0.500001, 0.5).astype(np.float32)
    want = ref.seam(img1, img2, k1, k2)
    for a, b in ((k1_3, k2), (k1_3, soft), (k1, soft)):
        _check(img1, img2, a, b, "soft", want=want)
    O, _, _ = ref.regions(k1, k2)
    ys, xs = np.nonzero(O)
    bad = img1.copy()
    for i, v in enumerate((np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf)):
        bad[i % 3, ys[5 * i + 3], xs[5 * i + 3]] = v
    _check(bad, img2, k1, k2, "non-finite")
    t = _dev((img1, img2, k1, k2))
    with pytest.raises(ValueError):
        ops.seam_gc(*t, max_rounds=-1)
    with pytest.raises(ValueError):
        ops.seam_gc(t[0], t[1], t[2], t[3][..., :-1])
    with pytest.raises(ValueError):
        ops.seam_gc(t[0].double(), t[1], t[2], t[3])


def test_too_few_rounds_fall_back_to_the_distance_seam():
    from stitch_amd import ops
    img1, img2, k1, k2, _ = dpref.ghost_scene(framed=True)
    t = _dev((img1, img2, k1, k2))
    with pytest.warns(UserWarning, match="seam_gc"):
        side, info, stats = ops.seam_gc(*t, max_rounds=0, return_stats=True)
    assert not stats["converged"] and stats["rounds"] == 0 and stats["sweeps"] == 0
    assert info.cpu().numpy().tolist() == [0, 3, 0, 0] and bool((side == 1).all())
    assert torch.equal(ops.multiband_blend(*t, levels=3, seam=(side, info)), ops.multiband_blend(*t, levels=3))
    with pytest.warns(UserWarning, match="seam_gc"):
        side, info, stats = ops.seam_gc(*t, max_rounds=1, return_stats=True)
    assert not stats["converged"] and stats["rounds"] == 1 and info.cpu().numpy().tolist() == [0, 3, 0, 0] and bool((side == 1).all())


@pytest.fixture(scope="module")
def two_cases():
    """a larger and a smaller canvas with their expected cuts"""
    big = noise_pair(95, 130, 81) + quads(95, 130)
    small = noise_pair(17, 33, 82) + tuple(np.ascontiguousarray(k.transpose(0, 2, 1)) for k in quads(33, 17))
    return big, ref.seam(*big), small, ref.seam(*small)


def _same(got, want):
    return all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))


def test_workspace_frame_history_and_streams(two_cases):
    from stitch_amd import ops
    big, want_big, small, want_small = two_cases
    assert want_big[1][0] == 1 and want_small[1][0] == 1
    tb, ts = _dev(big), _dev(small)
    need = ops.seam_gc_workspace_bytes(95, 130)
    assert need % 16 == 0 and need > ops.seam_gc_workspace_bytes(17, 33) > 0
    framed = torch.full((need + 512,), 0xA5, dtype=torch.uint8).cuda()     # exactly `need` bytes inside a sentinel frame
    ws1 = framed[256:256 + need]
    ws2 = torch.full((need,), 255, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):                                                     # a side stream; two calls in flight in separate workspaces
        r1 = ops.seam_gc(*tb, workspace=ws1)
    with torch.cuda.stream(s2):
        r2 = ops.seam_gc(*ts, workspace=ws2)
    with torch.cuda.stream(s1):                                                     # the workspace just held the larger canvas
        r3 = ops.seam_gc(*ts, workspace=ws1)
    s1.synchronize(), s2.synchronize()
    assert _same(r1, want_big) and _same(r2, want_small) and _same(r3, want_small)
    assert bool((framed[:256] == 0xA5).all()) and bool((framed[256 + need:] == 0xA5).all())
    with pytest.raises(ops.StitchErrorBase):
        ops.seam_gc(*tb, workspace=ws1[:4096])
    with pytest.raises(ops.StitchErrorBase):
        ops.seam_gc(*tb, workspace=framed[8:])


@pytest.mark.parametrize("levels", [0, 2, 5])
def test_blend_along_the_cut_equals_the_restatement(levels):
    from stitch_amd import ops
    H, W = 64, 48
    img1, img2 = noise_pair(H, W, 83)
    for name in ("quads", "nested", "pinhole"):
        k1, k2 = mask_cases(H, W)[name]
        t = _dev((img1, img2, k1, k2))
        seam = ops.seam_gc(*t)
        want_seam = ref.seam(img1, img2, k1, k2)
        got = ops.multiband_blend(*t, levels=levels, seam=seam)
        assert np.array_equal(got[0].cpu().numpy(), dpref.blend(img1, img2, k1, k2, levels, want_seam)), name
        if not want_seam[1][0]:
            assert torch.equal(got, ops.multiband_blend(*t, levels=levels)), name
    img1, img2, k1, k2 = ref.l_hole_scene()
    t = _dev((img1, img2, k1, k2))
    got = ops.multiband_blend(*t, levels=levels, seam=ops.seam_gc(*t))
    assert np.array_equal(got[0].cpu().numpy(), dpref.blend(img1, img2, k1, k2, levels, ref.seam(img1, img2, k1, k2)))


def test_out_py_blends_along_the_cut_and_leaves_the_other_ten(tmp_path, seeded_sd):
    """one synthetic pair at 96x128 through `inference_one_data`: without the flag, with multiband=5, with seam="dp" and with seam="gc" on top"""
    import stitch_amd
    from PIL import Image
    from stitch_amd.data import structured_pair
    spec_ = importlib.util.spec_from_file_location("stitch_out_harness_seam_gc", os.path.join(ROOT, "out.py"))
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
    assert "seam" not in dict(cfg) and outmod.seam_of(cfg) is None
    assert outmod.seam_of(outmod.get_config(base + ["--multiband_fusion", "--seam", "gc"])) == "gc"
    assert outmod.seam_of(outmod.get_config(base + ["--multiband_fusion", "--seam", "dp"])) == "dp"
    with pytest.raises(SystemExit):
        outmod.get_config(base + ["--seam", "gc"])
    with pytest.raises(SystemExit):
        outmod.get_config(base + ["--multiband_fusion", "--seam", "cut"])
    todo = outmod.get_data_dict_list(cfg.data_root_path, cfg.txt_file)
    model = stitch_amd.build_model(cfg)
    model.load_state_dict(seeded_sd, strict=True)
    model = model.cuda().eval()
    comp = stitch_amd.composition.Network().cuda().eval()
    inp = outmod.load_inpainter("passthrough_inpainter")
    with pytest.raises(ValueError):
        outmod.inference_one_data(cfg, todo[0], str(tmp_path / "bad") + "/", model, comp, inp, seam="gc")
    with pytest.raises(ValueError, match='"gc"'):
        outmod.inference_one_data(cfg, todo[0], str(tmp_path / "bad") + "/", model, comp, inp, multiband=5, seam="cut")
    dirs, outs = {}, {}
    for tag, kw in (("off", {}), ("mb", dict(multiband=5)), ("dp", dict(multiband=5, seam="dp")), ("gc", dict(multiband=5, seam="gc")),
                    ("gc_gpu", dict(multiband=5, seam="gc", gpu_jpeg=True)), ("gc_ec", dict(multiband=5, seam="gc", exposure=("gain", 32)))):
        dirs[tag] = str(tmp_path / tag) + "/"
        os.makedirs(dirs[tag])
        outs[tag], _ = outmod.inference_one_data(cfg, todo[0], dirs[tag], model, comp, inp, **kw)
    ten = sorted(os.listdir(dirs["off"] + "p0"))
    read = lambda tag, f: open(dirs[tag] + "p0/" + f, "rb").read()                 # noqa: E731
    assert len(ten) == 10 and "seam_side" not in outs["off"] and "seam_side" not in outs["mb"]
    ops = stitch_amd.ops
    for tag in ("mb", "dp", "gc", "gc_gpu", "gc_ec"):
        assert sorted(os.listdir(dirs[tag] + "p0")) == sorted(ten + ["multiband_fusion.jpg"])
        for f in ten:
            assert read(tag, f) == read("off", f), (tag, f)
    # no flag and "dp": what they are without this seam
    o = outs["mb"]
    args = (o["output1"].float().contiguous(), o["output2"].float().contiguous(), o["mask1"].float(), o["mask2"].float())
    assert torch.equal(ops.multiband_blend(*args, levels=5), o["multiband_image"])
    o = outs["dp"]
    pair = ops.seam_dp(*args)
    assert torch.equal(o["seam_side"], pair[0]) and torch.equal(o["seam_info"], pair[1])
    assert torch.equal(o["multiband_image"], ops.multiband_blend(*args, levels=5, seam=pair))
    want_dp = dpref.seam(*[t[0].cpu().numpy() for t in args])
    assert np.array_equal(pair[0].cpu().numpy(), want_dp[0]) and pair[1].cpu().numpy().tolist() == want_dp[1].tolist()
    for tag in ("gc", "gc_gpu", "gc_ec"):
        o = outs[tag]
        img1, img2 = (o["compensated1"], o["compensated2"]) if tag == "gc_ec" else args[:2]
        k1, k2 = o["mask1"].float(), o["mask2"].float()
        n = [t[0].cpu().numpy() for t in (img1, img2, k1, k2)]
        want_side, want_info = ref.seam(*n)
        assert np.array_equal(o["seam_side"].cpu().numpy(), want_side) and o["seam_info"].cpu().numpy().tolist() == want_info.tolist(), tag
        print(f"out.py pair, {tag}: seam info {want_info.tolist()}")
        if not want_info[0]:                                                        # (the seeded model's masks decide; both ways are asserted)
            assert torch.equal(o["multiband_image"], ops.multiband_blend(img1, img2, k1, k2, levels=5)), tag
        assert np.array_equal(o["multiband_image"][0].cpu().numpy(), dpref.blend(*n, 5, (want_side, want_info))), tag
        saver = outmod._Saver(gpu_jpeg=tag == "gc_gpu")
        saver.image(o["multiband_image"], dirs[tag] + "again.jpg")
        saver.wait()
        assert open(dirs[tag] + "again.jpg", "rb").read() == read(tag, "multiband_fusion.jpg"), tag
    assert read("gc", "multiband_fusion.jpg") == read("gc_gpu", "multiband_fusion.jpg")
