"""csrc/patchmatch.hip on the GPU: `ops.inpaint_patchmatch` equals the CPU restatement (tests/_patchmatch_ref.py) bit for bit -- the image,
info and the level-0 NNF and SAD planes -- over the sizes, masks, level counts, sweep counts and seeds below; a constant 2048x2048 image
fills with the constant; the result does not depend on the stream, the workspace's history or a hipGraph replay and nothing is written
outside the operands; the plug-in and `out.py` with `inpaint_all_area_g12_pm`."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import _patchmatch_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(15, 15), (15, 16), (16, 130), (33, 47), (63, 65), (64, 64), (65, 63), (31, 257), (15, 4096), (4096, 15)]
MASKS = ("corner", "border", "frame", "noise", "thin_known", "all", "none")
LEVELS, ITERS, SEEDS = (1, 2, 3, None), (0, 1, 3), (1, 0x9E3779B9)


@functools.lru_cache(maxsize=None)
def _inputs(H, W, name):
    hole = ref.masks(H, W)[name]
    img = ref.scene("ramp", H, W).copy()
    img[hole] = 0
    return img, hole.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _want(H, W, name, levels, iters, seed):
    img, mask = _inputs(H, W, name)
    return ref.patchmatch(img, mask, levels, iters, seed)


def _run(img, mask, levels, iters, seed, **kw):
    from stitch_amd import ops
    return ops.inpaint_patchmatch(torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda(), levels=levels, iters=iters, seed=seed, return_fields=True, **kw)


def _same(got, want, tag=""):
    out, info, nnf, sad = got
    assert out.dtype == torch.uint8 and info.dtype == torch.int32 and nnf.dtype == torch.int32 and sad.dtype == torch.int32, tag
    assert info.cpu().numpy().tolist() == want[1], (tag, info.cpu().numpy().tolist(), want[1])
    assert np.array_equal(nnf.cpu().numpy(), want[2]), tag
    assert np.array_equal(sad.cpu().numpy(), want[3]), tag
    assert np.array_equal(out.cpu().numpy(), want[0]), tag
    return True


def _check(H, W, name, levels, iters, seed):
    from stitch_amd import ops
    img, mask = _inputs(H, W, name)
    want = _want(H, W, name, levels, iters, seed)
    tag = f"{H}x{W} {name} levels {levels} iters {iters} seed {seed}"
    _same(_run(img, mask, levels, iters, seed), want, tag)
    assert ops.patchmatch_levels(H, W, levels) == ref.level_count(H, W, levels), tag
    known = mask == 0
    assert np.array_equal(want[0][known], img[known]), tag
    return want[1]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_equals_the_restatement_bit_for_bit(size):
    """every mask of `ref.masks` at every size; the level count, the sweep count and the seed rotate so that every size meets every
    value of each (the two 4096-long strips, whose restatement is the slow part, run one sweep at the most)"""
    H, W = size
    strip = max(H, W) == 4096
    seen = set()
    for i, name in enumerate(MASKS):
        j = i + SIZES.index(size)
        levels, iters, seed = LEVELS[j % 4], (ITERS[j % 2] if strip else ITERS[j % 3]), SEEDS[j % 2]
        seen.add(_check(H, W, name, levels, iters, seed)[0])
    bare = _run(*_inputs(H, W, "corner"), None, 1, 1)[:2]
    from stitch_amd import ops
    img, mask = _inputs(H, W, "corner")
    out, info = ops.inpaint_patchmatch(torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda().bool(), iters=1)      # without the planes, a bool mask
    assert torch.equal(out, bare[0]) and torch.equal(info, bare[1])
    assert seen == {0, 1}                                            # ("all" and "none" have nothing to fill)


@pytest.mark.parametrize("levels", LEVELS, ids=lambda v: f"levels_{v}")
@pytest.mark.parametrize("iters", ITERS, ids=lambda v: f"iters_{v}")
def test_levels_sweeps_and_seeds_crossed(levels, iters):
    for H, W, name in ((33, 47, "corner"), (63, 65, "noise"), (64, 64, "thin_known")):
        infos = [_check(H, W, name, levels, iters, seed) for seed in SEEDS]
        assert infos[0][0] == 1
    if iters:                                                        # the seed reaches the result
        a, b = (_want(63, 65, "noise", levels, iters, seed) for seed in SEEDS)
        assert not np.array_equal(a[2], b[2])


def test_start_level_below_the_top_and_no_source_at_level_0():
    """a known strip 8 wide has sources at level 0 only: the levels above are skipped on the device; 6 wide has none anywhere"""
    info = _check(64, 64, "thin_known", 3, 3, 1)
    assert info[:2] == [1, 0] and info[2] == 2 * 58
    H, W = 40, 50
    img = ref.scene("ramp", H, W)
    mask = np.ones((H, W), np.uint8)
    mask[:, 20:26] = 0
    want = ref.patchmatch(img, mask, None, 2, 1)
    assert want[1] == [0, 0, 0, 34 * 44] and np.array_equal(want[0], img)
    _same(_run(img, mask, None, 2, 1), want)


def test_constant_2048_with_a_ragged_hole():
    from stitch_amd import ops
    n = 2048
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[:n, :n]
    edge = 600 + (200 * np.sin(xx / 37.0) + 100 * np.sin(yy / 11.0)).astype(np.int64) + rng.integers(0, 9, (n, n))
    hole = (yy > edge) | (rng.random((n, n)) < 0.001)
    img = np.full((n, n, 3), (31, 142, 253), np.uint8)
    dirty = img.copy()
    dirty[hole] = 0
    out, info = ops.inpaint_patchmatch(torch.from_numpy(dirty).cuda(), torch.from_numpy(hole).cuda(), iters=2)
    info = info.cpu().numpy().tolist()
    # (7 levels; the 0.1 % of single hole pixels leave the coarsest ones without a source patch, so the start level is read on the device)
    assert ops.patchmatch_levels(n, n) == 7 and info[0] == 1 and 0 <= info[1] < 6 and info[2] > 0 and info[3] > 0
    assert torch.equal(out, torch.from_numpy(img).cuda())


@pytest.fixture(scope="module")
def two_cases():
    big = _inputs(63, 65, "corner")
    small = _inputs(33, 47, "border")
    return big, _want(63, 65, "corner", None, 3, 1), small, _want(33, 47, "border", None, 3, 1)


def _dev(case):
    return [torch.from_numpy(a).cuda() for a in case]


def test_streams_and_workspace_history(two_cases):
    from stitch_amd import ops
    big, want_big, small, want_small = two_cases
    tb, ts = _dev(big), _dev(small)
    need = ops.patchmatch_workspace_bytes(63, 65)
    assert need > ops.patchmatch_workspace_bytes(33, 47) > 0 and need % 16 == 0
    ws1 = torch.full((need,), 255, dtype=torch.uint8).cuda()
    ws2 = torch.full((need,), 255, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    kw = dict(iters=3, seed=1, return_fields=True)
    with torch.cuda.stream(s1):                                                     # a side stream; two calls in flight in separate workspaces
        r1 = ops.inpaint_patchmatch(*tb, workspace=ws1, **kw)
    with torch.cuda.stream(s2):
        r2 = ops.inpaint_patchmatch(*ts, workspace=ws2, **kw)
    with torch.cuda.stream(s1):                                                     # the workspace just held the larger canvas
        r3 = ops.inpaint_patchmatch(*ts, workspace=ws1, **kw)
    s1.synchronize(), s2.synchronize()
    assert _same(r1, want_big) and _same(r2, want_small) and _same(r3, want_small)
    with pytest.raises(ops.StitchErrorBase):
        ops.inpaint_patchmatch(*tb, workspace=ws1[:4096])


def test_captured_into_a_graph_and_replayed_on_other_pixels(two_cases):
    from stitch_amd import ops
    big, want_big, _, _ = two_cases
    other = (np.ascontiguousarray(big[0][::-1, ::-1]), np.ascontiguousarray(big[1][::-1, ::-1]))
    static = _dev(big)
    ws = torch.empty(ops.patchmatch_workspace_bytes(63, 65), dtype=torch.uint8).cuda()
    kw = dict(iters=3, seed=1, return_fields=True, workspace=ws)
    side_stream = torch.cuda.Stream()
    side_stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side_stream):
        ops.inpaint_patchmatch(*static, **kw)
    torch.cuda.current_stream().wait_stream(side_stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = ops.inpaint_patchmatch(*static, **kw)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(res, want_big)
    for t, a in zip(static, other):
        t.copy_(torch.from_numpy(a))
    graph.replay()
    torch.cuda.synchronize()
    want = ref.patchmatch(other[0], other[1], None, 3, 1)
    assert not np.array_equal(want[0], want_big[0])
    assert _same(res, want)
    assert _same(ops.inpaint_patchmatch(*static, iters=3, seed=1, return_fields=True), want)       # eager on the same pixels


def test_every_operand_inside_a_frame_that_stays_intact():
    """the image and the mask in 0x5A frames; the outputs and a workspace of exactly st_patchmatch_workspace_bytes in sentinel frames"""
    from stitch_amd import ops
    from stitch_amd._lib import lib
    H, W = 33, 47
    n, pad = H * W, 64
    img, mask = _inputs(H, W, "corner")
    want = _want(H, W, "corner", None, 3, 1)
    need = ops.patchmatch_workspace_bytes(H, W)

    def framed(count, dtype, fill, values=None):
        buf = torch.full((pad + count + pad,), fill, dtype=dtype, device="cuda")
        if values is not None:
            buf[pad:pad + count] = torch.from_numpy(np.ascontiguousarray(values).reshape(-1)).cuda()
        return buf
    fi, fm = framed(3 * n, torch.uint8, 0x5A, img), framed(n, torch.uint8, 0x5A, mask)
    out, info, nnf, sad, ws = framed(3 * n, torch.uint8, 0xA5), framed(4, torch.int32, -77), framed(2 * n, torch.int32, -77), framed(n, torch.int32, -77), framed(need, torch.uint8, 0xA5)
    assert (ws.data_ptr() + pad) % 16 == 0
    ptr = lambda t: C.c_void_p(t.data_ptr() + pad * t.element_size())                # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for fields in ((ptr(nnf), ptr(sad)), (None, None)):
        out[pad:pad + 3 * n] = 0xA5
        assert lib.st_patchmatch_fill(ptr(fi), ptr(fm), H, W, 0, 3, 1, ptr(out), ptr(info), fields[0], fields[1], ptr(ws), need, stream) == 0
        torch.cuda.synchronize()
        assert np.array_equal(out[pad:pad + 3 * n].cpu().numpy().reshape(H, W, 3), want[0]) and info[pad:pad + 4].cpu().numpy().tolist() == want[1]
    assert np.array_equal(nnf[pad:pad + 2 * n].cpu().numpy().reshape(H, W, 2), want[2]) and np.array_equal(sad[pad:pad + n].cpu().numpy().reshape(H, W), want[3])
    assert np.array_equal(fi[pad:pad + 3 * n].cpu().numpy(), img.reshape(-1)) and np.array_equal(fm[pad:pad + n].cpu().numpy(), mask.reshape(-1))
    for buf, count, fill in ((fi, 3 * n, 0x5A), (fm, n, 0x5A), (out, 3 * n, 0xA5), (info, 4, -77), (nnf, 2 * n, -77), (sad, n, -77), (ws, need, 0xA5)):
        assert (buf[:pad] == fill).all() and (buf[pad + count:] == fill).all()


def test_plugin_protocol():
    from stitch_amd.mix_methods.utils import patchmatch_inpainter as mod
    inp = mod.inpainter
    assert inp.name == "patchmatch_inpainter" and isinstance(inp, mod.Inpainter)
    H, W = 63, 65
    img, mask = _inputs(H, W, "corner")
    want = _want(H, W, "corner", None, 4, 1)[0]
    t = torch.from_numpy(img.copy()).permute(2, 0, 1)[None].float() + 0.75          # (truncated by the preprocessing)
    m1 = torch.from_numpy(mask.copy())[None, None].float()
    for im, mk in ((t.cuda(), m1.cuda()), (t.cuda(), m1.repeat(1, 3, 1, 1).cuda() * 255), (t, m1)):
        got = inp.inpaint(im, mk, control_image_tensor=None, prompt="", resize_to_area_limit_before_inpaint=750 * 750)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 3, H, W) and got.device == im.device
        assert np.array_equal(got[0].permute(1, 2, 0).cpu().numpy(), want)
    with pytest.raises(ValueError):
        inp.inpaint(torch.cat([t, t]).cuda(), torch.cat([m1, m1]).cuda())
    with pytest.raises(ValueError):
        inp.inpaint(t.cuda(), m1[..., :-1].cuda())


def test_out_py_with_the_pm_config_fills_the_holes(tmp_path, seeded_sd):
    """one synthetic pair at 96x128 through `inference_one_data` under `inpaint_all_area_g12_pm` and `_cv`: the files are written, warp2.jpg's hole
    pixels are no longer all black, and what the mix method did not hand to the inpainter is the `_cv` run's"""
    from PIL import Image
    import stitch_amd
    from stitch_amd.data import structured_pair
    spec_ = importlib.util.spec_from_file_location("stitch_out_harness_pm", os.path.join(ROOT, "out.py"))
    outmod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(outmod)
    root = tmp_path / "demo"
    (root / "p0").mkdir(parents=True)
    a, b = structured_pair(96, 128, seed=3, shift=(2, -3))
    for name, t in (("input1.jpg", a), ("input2.jpg", b)):
        Image.fromarray(t[0].permute(1, 2, 0).numpy().astype(np.uint8)).save(str(root / "p0" / name), quality=97)
    (root / "demo.txt").write_text("p0/\n")
    base = ["--data_root_path", str(root) + "/"]
    outs, dirs, calls = {}, {}, {}
    model = comp = None
    for tag in ("pm", "cv"):
        cfg = outmod.get_config(base + ["--inf_cfg", f"inpaint_all_area_g12_{tag}"])
        name = {"pm": "patchmatch_inpainter", "cv": "cv_inpainter"}[tag]
        assert cfg.TPS_PIPELINE_CONFIG.inpainter == name and cfg.TPS_PIPELINE_CONFIG.mix_method == "inpaint_all_area"
        if model is None:
            model = stitch_amd.build_model(cfg)
            model.load_state_dict(seeded_sd, strict=True)
            model = model.cuda().eval()
            comp = stitch_amd.composition.Network().cuda().eval()
        inner = outmod.load_inpainter(name)
        assert inner.name == name
        calls[tag] = []

        class Spy:                                                   # records what the mix method hands to the inpainter
            name = inner.name

            def inpaint(self, init_image_tensor, mask_image_tensor, **kw):
                res = inner.inpaint(init_image_tensor, mask_image_tensor, **kw)
                calls[tag].append((mask_image_tensor.detach().clone(), res.clone()))
                return res
        todo = outmod.get_data_dict_list(cfg.data_root_path, cfg.txt_file)
        dirs[tag] = str(tmp_path / tag) + "/"
        os.makedirs(dirs[tag])
        outs[tag], _ = outmod.inference_one_data(cfg, todo[0], dirs[tag], model, comp, Spy())
    assert sorted(os.listdir(dirs["pm"] + "p0")) == sorted(os.listdir(dirs["cv"] + "p0")) and "warp2.jpg" in os.listdir(dirs["pm"] + "p0")
    assert len(calls["pm"]) == len(calls["cv"]) >= 1
    for (m_pm, r_pm), (m_cv, r_cv) in zip(calls["pm"], calls["cv"]):
        assert torch.equal(m_pm, m_cv)
        hole = (m_pm[0].float().amax(0) > 0).to(r_pm.device)
        assert hole.any() and not hole.all()
        assert torch.equal(r_pm[0][:, ~hole], r_cv[0][:, ~hole])                    # known pixels: both inpainters return them as they are
        assert (r_pm[0][:, hole] > 0).any()
    w_pm = np.asarray(Image.open(dirs["pm"] + "p0/warp2.jpg").convert("RGB")).astype(np.int64)
    w_cv = np.asarray(Image.open(dirs["cv"] + "p0/warp2.jpg").convert("RGB")).astype(np.int64)
    assert w_pm.shape == w_cv.shape
    hole = (calls["pm"][-1][0][0].float().amax(0) > 0).cpu().numpy()
    assert hole.shape == w_pm.shape[:2]
    assert w_pm[hole].max() > 16                                     # not all black (JPEG noise of a black area stays below)
    far = ~_dilate(hole, 16)                                         # (a JPEG block mixes a pixel with its neighbours: 16x16 with subsampled chroma)
    assert np.array_equal(w_pm[far], w_cv[far])
    print(f"out.py pair: canvas {w_pm.shape[:2]}, {int(hole.sum())} hole pixels, {len(calls['pm'])} inpainter call(s)")


def _dilate(m, r):
    out = m.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            out |= np.roll(np.roll(m, dy, 0), dx, 1)
    return out
