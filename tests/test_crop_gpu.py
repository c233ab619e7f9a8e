"""csrc/crop.hip on the GPU: `ops.inner_rect` equals the CPU restatement (tests/_crop_ref.py) bit for bit -- info and the run plane -- at the
block, wave and segment borders, on structured rows, at full size against closed forms, whatever the stream, the workspace's history or a
hipGraph replay; `out.py --crop inner` adds the cropped files and changes nothing else."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import _crop_ref as ref
from _multiband_cases import mask_cases, quads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()[None]


def _want(k1, k2=None):
    u = ref.union(k1, k2)
    r = ref.runs(u)
    return ref.rect(u, r=r), r


def _check(k1, k2=None, tag=""):
    from stitch_amd import ops
    want_info, want_runs = _want(k1, k2)
    info, runs = ops.inner_rect(_dev(k1), _dev(k2), return_runs=True)
    assert info.dtype == torch.int32 and tuple(info.shape) == (6,) and runs.dtype == torch.int16 and tuple(runs.shape) == k1.shape[1:]
    assert np.array_equal(runs.cpu().numpy(), want_runs), tag
    assert info.cpu().numpy().tolist() == want_info, (tag, want_info)
    assert torch.equal(ops.inner_rect(_dev(k1), _dev(k2)), info), tag                  # without the plane: the same rectangle
    return want_info


def _of(u):
    return np.ascontiguousarray(u[None].astype(np.float32))


SIZES = ([(1, 1), (1, 7), (7, 1), (2, 2)] + [(5, w) for w in (63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4095, 4096)]
         + [(h, 9) for h in (15, 16, 17, 31, 32, 33, 255, 256, 257)] + [(4096, 3)])


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes_at_the_block_wave_and_segment_borders(size):
    """a block of the row search is 64 positions = one wave, a workgroup of it takes 256 per round (63 .. 129, 1023 .. 1025, the longest row);
    the run pass cuts a column into 16 segments (15 / 16 / 17 rows: segments of one row, with empty ones and with two rows; 255 .. 257; the
    longest column)"""
    H, W = size
    rng = np.random.default_rng(61)
    ones = np.ones((1, H, W), np.float32)
    cases = {"ones": (ones, ones.copy())}
    cases.update(mask_cases(H, W))
    for d in (0.5, 0.95):
        cases[f"noise {d}"] = (_of(rng.random((H, W)) < d), _of(rng.random((H, W)) < d * 0.5))
    seen = set()
    for name, (k1, k2) in cases.items():
        seen.add(_check(k1, k2, tag=name)[0])
    assert _check(ones)[1:] == [0, 0, H, W, H * W]
    assert seen == {0, 1}                                            # (both_empty is among the arrangements)


def test_structured_rows():
    H = 70
    y, x = np.mgrid[:H, :130]
    for name, u in (("ascending", y >= H - 1 - x // 2), ("descending", y >= H - 1 - (129 - x) // 2),
                    ("plateau 63|64", (y >= 60) | ((x >= 60) & (x < 68) & (y >= 20)) | ((x >= 120) & (y >= 40))),
                    ("set column between unset ones", (x == 64) | (x == 0) | (x == 129) | (y == 3))):
        info = _check(_of(u), tag=name)
        assert info[0] == 1, name
    for Hs in (32, 33, 48, 257):                                     # an unset pixel on the last row of a column segment, one on the first row of the next
        S = -(-Hs // 16)
        for yy in (S - 1, S, 7 * S - 1, 7 * S):
            u = np.ones((Hs, 66), bool)
            u[yy, 0] = u[yy, 65] = False
            _check(_of(u), tag=f"segment {Hs} {yy}")
            a, b = u.copy(), u.copy()
            a[yy:] = False                                           # the run crosses the masks as well: above the row from mask1, from it on from mask2
            b[:yy] = False
            _check(_of(a), _of(b), tag=f"segment {Hs} {yy} split")


def _info(mask1, mask2=None):
    from stitch_amd import ops
    return ops.inner_rect(mask1, mask2).cpu().numpy().tolist()


def test_closed_forms_at_full_size():
    for n in (2048, 4096):
        ones = torch.ones((1, 1, n, n), device="cuda")
        assert _info(ones) == [1, 0, 0, n, n, n * n]
    zero = torch.zeros_like(ones)
    assert _info(zero, ones) == [1, 0, 0, 4096, 4096, 1 << 24] and _info(zero, zero) == [0] * 6
    m = ones.clone()
    m[..., 1000, :] = 0
    m[..., :, 1500] = 0                                              # quadrants 1000 x 1500, 1000 x 2595, 3095 x 1500, 3095 x 2595
    assert _info(m) == [1, 1001, 1501, 3095, 2595, 3095 * 2595]
    assert _info(zero, m) == [1, 1001, 1501, 3095, 2595, 3095 * 2595]
    m = ones.clone()
    m[..., 1000, :] = 0
    m[..., :, 2047:2049] = 0                                         # two columns, so that the lower quadrants are both 3095 x 2047: the lowest left
    assert _info(m) == [1, 1001, 0, 3095, 2047, 3095 * 2047]
    m = ones.clone()
    m[..., 2047:2049, :] = 0
    m[..., :, 1000] = 0                                              # the right quadrants are both 2047 x 3095: the lowest top
    assert _info(m) == [1, 0, 1001, 2047, 3095, 2047 * 3095]
    m = ones.clone()
    m[..., 4095, 4095] = 0                                           # 4095 x 4096 at the top against 4096 x 4095 on the left, both at (0, 0): the smallest h
    assert _info(m) == [1, 0, 0, 4095, 4096, 4095 * 4096]


def test_empty_three_channel_soft_and_non_finite_masks():
    from stitch_amd import ops
    H, W = 33, 70
    k1, k2 = quads(H, W)
    rng = np.random.default_rng(62)
    empty = np.zeros_like(k1)
    assert _check(empty)[0] == 0 and _check(empty, empty)[0] == 0
    for a, b in ((k1, None), (k2, None), (empty, k2), (k1, empty)):
        assert _check(a, b)[0] == 1
    want = _check(k1, k2)
    k1_3 = np.concatenate([k1, rng.random((2, H, W)).astype(np.float32)])
    half = np.float32(0.5)
    soft = np.where(k2 > 0.5, np.nextafter(half, np.float32(1)), half).astype(np.float32)
    odd1 = np.where(k1 > 0.5, np.inf, np.where(rng.random(k1.shape) < 0.5, np.nan, -np.inf)).astype(np.float32)
    odd2 = np.where(k2 > 0.5, 1e30, np.where(rng.random(k2.shape) < 0.5, np.nan, -1e30)).astype(np.float32)
    for a, b in ((k1_3, k2), (k1_3, soft), (k1, soft), (odd1, odd2), (odd1, soft)):
        info, runs = ops.inner_rect(_dev(a), _dev(b), return_runs=True)
        assert info.cpu().numpy().tolist() == want and np.array_equal(runs.cpu().numpy(), _want(k1, k2)[1])
        assert _check(a, b) == want                                  # the restatement reads them the same way
    t = _dev(k1)
    with pytest.raises(ValueError):
        ops.inner_rect(t, t[..., :-1])
    with pytest.raises(ValueError):
        ops.inner_rect(t.double())
    with pytest.raises(ValueError):
        ops.inner_rect(torch.cat([t, t]))


@pytest.fixture(scope="module")
def two_cases():
    """a larger and a smaller canvas with their expected results"""
    big = quads(95, 130)
    rng = np.random.default_rng(63)
    small = (_of(rng.random((17, 33)) < 0.9), _of(rng.random((17, 33)) < 0.5))
    return big, _want(*big), small, _want(*small)


def _same(got, want):
    return got[0].cpu().numpy().tolist() == want[0] and np.array_equal(got[1].cpu().numpy(), want[1])


def test_streams_and_workspace_history(two_cases):
    from stitch_amd import ops
    big, want_big, small, want_small = two_cases
    tb, ts = [_dev(k) for k in big], [_dev(k) for k in small]
    need = ops.inner_rect_workspace_bytes(95, 130)
    assert need >= 2 * 95 * 130 + 8 * 95 > ops.inner_rect_workspace_bytes(17, 33) > 0
    ws1 = torch.full((need,), 255, dtype=torch.uint8).cuda()
    ws2 = torch.full((need,), 255, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):                                                     # a side stream; two calls in flight in separate workspaces
        r1 = ops.inner_rect(*tb, workspace=ws1, return_runs=True)
    with torch.cuda.stream(s2):
        r2 = ops.inner_rect(*ts, workspace=ws2, return_runs=True)
    with torch.cuda.stream(s1):                                                     # the workspace just held the larger canvas
        r3 = ops.inner_rect(*ts, workspace=ws1, return_runs=True)
        r4 = ops.inner_rect(*ts, workspace=ws1)                                     # and the run plane inside it
    s1.synchronize(), s2.synchronize()
    assert _same(r1, want_big) and _same(r2, want_small) and _same(r3, want_small) and r4.cpu().numpy().tolist() == want_small[0]
    with pytest.raises(ops.StitchErrorBase):
        ops.inner_rect(*tb, workspace=ws1[:4096])


def test_captured_into_a_graph_and_replayed_on_other_masks(two_cases):
    from stitch_amd import ops
    big, want_big, _, _ = two_cases
    other = tuple(np.ascontiguousarray(k[:, ::-1, ::-1]) for k in big)
    static = [_dev(k) for k in big]
    ws = torch.empty(ops.inner_rect_workspace_bytes(95, 130), dtype=torch.uint8).cuda()
    side_stream = torch.cuda.Stream()
    side_stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side_stream):
        ops.inner_rect(*static, workspace=ws)
    torch.cuda.current_stream().wait_stream(side_stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = ops.inner_rect(*static, workspace=ws, return_runs=True)
        bare = ops.inner_rect(*static, workspace=ws)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(res, want_big) and bare.cpu().numpy().tolist() == want_big[0]
    for t, a in zip(static, other):
        t.copy_(torch.from_numpy(a)[None])
    graph.replay()
    torch.cuda.synchronize()
    want = _want(*other)
    assert want[0] != want_big[0]
    assert _same(res, want) and bare.cpu().numpy().tolist() == want[0]


def test_every_operand_inside_a_frame_that_stays_intact():
    """the masks in NaN frames, info, the run plane and a workspace of exactly st_inner_rect_workspace_bytes in sentinel frames"""
    from stitch_amd import ops
    from stitch_amd._lib import lib
    H, W = 37, 53
    n, pad = H * W, 64
    k1, k2 = quads(H, W)
    want = _want(k1, k2)
    need = ops.inner_rect_workspace_bytes(H, W)

    def framed(count, dtype, fill, values=None):
        buf = torch.full((pad + count + pad,), fill, dtype=dtype, device="cuda")
        if values is not None:
            buf[pad:pad + count] = torch.from_numpy(values.reshape(-1)).cuda()
        return buf
    m1, m2 = framed(n, torch.float32, float("nan"), k1), framed(n, torch.float32, float("nan"), k2)
    info, runs, ws = framed(6, torch.int32, -77), framed(n, torch.int16, -77), framed(need, torch.uint8, 0xA5)
    assert (ws.data_ptr() + pad) % 16 == 0
    ptr = lambda t: C.c_void_p(t.data_ptr() + pad * t.element_size())                # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for runs_arg in (ptr(runs), None):
        info[pad:pad + 6] = -77
        assert lib.st_inner_rect(ptr(m1), ptr(m2), H, W, ptr(info), runs_arg, ptr(ws), need, stream) == 0
        torch.cuda.synchronize()
        assert info[pad:pad + 6].cpu().numpy().tolist() == want[0]
    assert np.array_equal(runs[pad:pad + n].cpu().numpy().reshape(H, W), want[1])
    for buf, count in ((m1, n), (m2, n)):
        assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + count:]).all()
    assert np.array_equal(m1[pad:pad + n].cpu().numpy(), k1.reshape(-1)) and np.array_equal(m2[pad:pad + n].cpu().numpy(), k2.reshape(-1))
    for buf, count, fill in ((info, 6, -77), (runs, n, -77), (ws, need, 0xA5)):
        assert (buf[:pad] == fill).all() and (buf[pad + count:] == fill).all()


def test_out_py_writes_the_cropped_files_and_leaves_the_others(tmp_path, seeded_sd):
    """one synthetic pair at 96x128 through `inference_one_data`: without the flag, with crop="inner" on both savers, and with multiband"""
    from PIL import Image
    import stitch_amd
    from stitch_amd.data import structured_pair
    spec_ = importlib.util.spec_from_file_location("stitch_out_harness_crop", os.path.join(ROOT, "out.py"))
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
    assert "crop" not in dict(cfg) and outmod.crop_of(cfg) is None                  # config.txt stays what it was
    assert outmod.crop_of(outmod.get_config(base + ["--crop", "inner"])) == "inner"                         # independent of --multiband_fusion
    assert outmod.crop_of(outmod.get_config(base + ["--multiband_fusion", "--crop", "inner"])) == "inner"
    with pytest.raises(SystemExit):
        outmod.get_config(base + ["--crop", "outer"])
    todo = outmod.get_data_dict_list(cfg.data_root_path, cfg.txt_file)
    model = stitch_amd.build_model(cfg)
    model.load_state_dict(seeded_sd, strict=True)
    model = model.cuda().eval()
    comp = stitch_amd.composition.Network().cuda().eval()
    inp = outmod.load_inpainter("passthrough_inpainter")
    with pytest.raises(ValueError):
        outmod.inference_one_data(cfg, todo[0], str(tmp_path / "bad") + "/", model, comp, inp, crop="outer")
    dirs, outs = {}, {}
    for tag, kw in (("off", {}), ("crop", dict(crop="inner")), ("crop_gpu", dict(crop="inner", gpu_jpeg=True)), ("mb", dict(multiband=5)),
                    ("mb_crop", dict(multiband=5, crop="inner")), ("mb_crop_gpu", dict(multiband=5, crop="inner", gpu_jpeg=True))):
        dirs[tag] = str(tmp_path / tag) + "/"
        os.makedirs(dirs[tag])
        outs[tag], _ = outmod.inference_one_data(cfg, todo[0], dirs[tag], model, comp, inp, **kw)
    ten = sorted(os.listdir(dirs["off"] + "p0"))
    read = lambda tag, f: open(dirs[tag] + "p0/" + f, "rb").read()                 # noqa: E731
    assert len(ten) == 10 and "crop_info" not in outs["off"] and "crop_rect" not in outs["mb"]
    assert sorted(os.listdir(dirs["mb"] + "p0")) == sorted(ten + ["multiband_fusion.jpg"])
    for tag in ("crop", "crop_gpu", "mb_crop", "mb_crop_gpu"):
        mb = tag.startswith("mb")
        extra = ["ave_fusion_crop.jpg"] + (["multiband_fusion.jpg", "multiband_fusion_crop.jpg"] if mb else [])
        assert sorted(os.listdir(dirs[tag] + "p0")) == sorted(ten + extra), tag
        for f in ten:
            assert read(tag, f) == read("off", f), (tag, f)
        if mb:
            assert read(tag, "multiband_fusion.jpg") == read("mb", "multiband_fusion.jpg"), tag
        o = outs[tag]
        want = ref.rect(ref.union(o["mask1"].float()[0].cpu().numpy(), o["mask2"].float()[0].cpu().numpy()))
        assert o["crop_info"].dtype == torch.int32 and o["crop_info"].cpu().numpy().tolist() == want, tag
        assert want[0] == 1 and o["crop_rect"] == tuple(want[1:5]), tag             # mask1 always holds image 1's rectangle
        top, left, h, w = o["crop_rect"]
        print(f"out.py pair, {tag}: canvas {tuple(o['mask1'].shape[2:])}, crop_rect {o['crop_rect']}")
        saver = outmod._Saver(gpu_jpeg=tag.endswith("gpu"))
        saver.image(o["new_blend_image"].float()[..., top:top + h, left:left + w], dirs[tag] + "again.jpg")
        if mb:
            saver.image(o["multiband_image"][..., top:top + h, left:left + w], dirs[tag] + "again_mb.jpg")
        saver.wait()
        assert open(dirs[tag] + "again.jpg", "rb").read() == read(tag, "ave_fusion_crop.jpg"), tag
        assert Image.open(dirs[tag] + "p0/ave_fusion_crop.jpg").size == (w, h)
        if mb:
            assert open(dirs[tag] + "again_mb.jpg", "rb").read() == read(tag, "multiband_fusion_crop.jpg"), tag
    assert read("crop", "ave_fusion_crop.jpg") == read("crop_gpu", "ave_fusion_crop.jpg") == read("mb_crop", "ave_fusion_crop.jpg")
    assert read("mb_crop", "multiband_fusion_crop.jpg") == read("mb_crop_gpu", "multiband_fusion_crop.jpg")
