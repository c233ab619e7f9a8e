"""The restart kernels (jpegr_* in csrc/jpeg_dec.hip and csrc/jpeg.hip) on the GPU: `ops.jpeg_decode` gives Pillow's pixels bit for bit on every file of tests/golden/jpeg_rst_pil.npz, and on files
made here with Pillow -- one interval over three workgroups of subsequences, two long intervals, a row per interval, an MCU per interval, the
flat image whose stream never synchronises -- the pixels of the same image's file without restart markers, which go through the existing
path; whatever the row stride, stream or workspace history.  A damaged interval sets the status and leaves every other interval exact, a
cut file gives status 1; `evaluate` and `out.py` take DRI inputs with `gpu_decode` and compute what they compute without it."""
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

import _jpeg_dec_cases as cases
import _jpeg_ref as eref
import _jpeg_rst_ref as rst

pytestmark = pytest.mark.gpu

ROOT = cases.ROOT


@pytest.fixture(scope="module")
def golden():
    return rst.load_golden()


def _pillow_file(u8, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(u8).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def _decode(data, **kw):
    from stitch_amd import ops
    px, status = ops.jpeg_decode(data, **kw)
    assert px.is_cuda and px.dtype == torch.uint8 and status.is_cuda and status.dtype == torch.int32
    px = px.cpu().numpy()
    return (px[..., 0] if px.shape[2] == 1 else px), int(status.item())


def _diff(got, want):
    if got.shape != want.shape:
        return f"shapes {got.shape} / {want.shape}"
    bad = np.argwhere(got != want)
    return f"{len(bad)} samples differ, first at {tuple(bad[0]) if len(bad) else None}"


def test_every_golden_file_gives_pillows_pixels(golden):
    from stitch_amd import ops
    for name, (_, _, data, px) in golden.items():
        assert ops.jpeg_probe(data, restart=True).restart_interval > 0
        got, status = _decode(data)
        assert status == 0, name
        assert np.array_equal(got, px), (name, _diff(got, px))


NOISE = np.random.RandomState(5).randint(0, 256, (384, 384, 3)).astype(np.uint8)
SMOOTH = eref._smooth(96, 136, 3, 6)
GENERATED = {"one_interval_three_workgroups": (NOISE, dict(restart_marker_blocks=65535)),
             "two_long_intervals": (NOISE, dict(restart_marker_rows=12)),
             "a_row_per_interval": (NOISE, dict(restart_marker_rows=1)),
             "an_mcu_per_interval": (NOISE, dict(restart_marker_blocks=1)),
             "an_mcu_per_interval_smooth": (SMOOTH, dict(restart_marker_blocks=1)),
             "zeros_512_rows": (np.zeros((512, 512, 3), np.uint8), dict(restart_marker_rows=1))}


@pytest.fixture(scope="module")
def generated():
    """{name: (file with restart intervals, the decoder's pixels of the same image's file without them)}"""
    from stitch_amd import ops
    out, plain = {}, {}
    for name, (u8, kw) in GENERATED.items():
        data = _pillow_file(u8, quality=75, **kw)
        if id(u8) not in plain:
            base = _pillow_file(u8, quality=75)
            assert ops.jpeg_probe(base).restart_interval == 0
            want, status = _decode(base)
            assert status == 0 and np.array_equal(want, cases.pillow_pixels(base))
            plain[id(u8)] = want
        out[name] = (data, plain[id(u8)])
    info = ops.jpeg_probe(out["one_interval_three_workgroups"][0], restart=True)
    assert info.restart_interval == 65535 and info.scan_len * 8 > 2 * cases.SUB_BITS * cases.SYNC_THREADS       # the fixpoint crosses workgroups inside an interval
    longest = {name: max(n for _, n in rst.intervals(out[name][0], ops.jpeg_probe(out[name][0], restart=True)._asdict())) * 8 for name in out}
    assert cases.SUB_BITS < longest["an_mcu_per_interval"] < 2 * cases.SUB_BITS          # noise: an MCU of six blocks is one or two subsequences
    assert longest["an_mcu_per_interval_smooth"] < cases.SUB_BITS                        # every interval below one subsequence: nothing to repair
    return out


@pytest.mark.parametrize("name", list(GENERATED))
def test_generated_files_equal_the_file_without_restart_markers(generated, name):
    data, want = generated[name]
    got, status = _decode(data)
    assert status == 0 and np.array_equal(got, want), _diff(got, want)
    assert np.array_equal(want, cases.pillow_pixels(data))                    # and Pillow's pixels of the DRI file itself


def test_row_stride_streams_and_workspace_reuse(generated, golden):
    from stitch_amd import ops
    data, want = generated["a_row_per_interval"]
    plain = _pillow_file(np.zeros((512, 512, 3), np.uint8), quality=75)       # larger, no DRI
    small, want_s = golden[rst.case_name("rgb_64x48", subsampling=2, blocks=1)][2:]
    info, info_p, info_s = ops.jpeg_probe(data, restart=True), ops.jpeg_probe(plain), ops.jpeg_probe(small, restart=True)
    # a column slice of a wider canvas, untouched around it
    wide = torch.full((384, 500, 3), 9, dtype=torch.uint8).cuda()
    view = wide[:, 17:17 + 384]
    assert not view.is_contiguous()
    out, status = ops.jpeg_decode(data, out=view)
    assert out.data_ptr() == view.data_ptr() and int(status.item()) == 0
    w = wide.cpu().numpy()
    assert np.array_equal(w[:, 17:401], want) and (w[:, :17] == 9).all() and (w[:, 401:] == 9).all()
    # a side stream; two decodes in flight on two streams, one with and one without DRI
    dev, dev_p, dev_s = (torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in (data, plain, small))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        r1 = ops.jpeg_decode(dev, info=info)
    with torch.cuda.stream(s2):
        r2 = ops.jpeg_decode(dev_p, info=info_p)
    with torch.cuda.stream(s1):
        r3 = ops.jpeg_decode(dev_s, info=info_s)
    s1.synchronize(), s2.synchronize()
    want_p = cases.pillow_pixels(plain)
    assert np.array_equal(r1[0].cpu().numpy(), want) and np.array_equal(r2[0].cpu().numpy(), want_p) and np.array_equal(r3[0].cpu().numpy(), want_s)
    assert [int(r[1].item()) for r in (r1, r2, r3)] == [0, 0, 0]
    # one workspace that just held the larger no-DRI image, then a small DRI file, then the first again
    ws = torch.full((max(ops.jpeg_dec_workspace_bytes(i) for i in (info, info_p, info_s)),), 255, dtype=torch.uint8).cuda()
    for d, i, wnt in ((dev_p, info_p, want_p), (dev, info, want), (dev_s, info_s, want_s), (dev, info, want)):
        px, st = ops.jpeg_decode(d, info=i, workspace=ws)
        assert int(st.item()) == 0 and np.array_equal(px.cpu().numpy(), wnt)
    with pytest.raises(ops.StitchErrorBase):
        ops.jpeg_decode(dev, info=info, workspace=ws[:ops.jpeg_dec_workspace_bytes(info) - 16])


def test_a_damaged_interval_sets_the_status_and_spares_the_others():
    from stitch_amd import ops
    # 4:4:4, where no pixel leans on a neighbouring MCU (fancy upsampling does): 16 MCU rows of 16 MCUs of 8 x 8 pixels, a row per interval
    data = _pillow_file(NOISE[:128, :128], quality=75, subsampling=0, restart_marker_rows=1)
    want = cases.pillow_pixels(data)
    info = ops.jpeg_probe(data, restart=True)
    assert info.restart_interval == 16
    short = rst.damaged(data, info._asdict(), 7)
    i2 = info._replace(scan_len=info.scan_len - (len(data) - len(short)), nbytes=len(short))
    got, status = _decode(short, info=i2)
    assert status != 0
    rows = np.r_[0:7 * 8, 8 * 8:128]                                          # every MCU of the other intervals
    assert np.array_equal(got[rows], want[rows]), _diff(got[rows], want[rows])
    assert not np.array_equal(got[7 * 8:8 * 8], want[7 * 8:8 * 8])
    whole, status = _decode(data)
    assert status == 0 and np.array_equal(whole, want)


def test_a_cut_file_gives_status_1(generated):
    from stitch_amd import ops
    data, _ = generated["a_row_per_interval"]
    info = ops.jpeg_probe(data, restart=True)
    short = cases.cut(data, info, fraction=0.5)
    assert ops.jpeg_probe(short, restart=True) is None                        # its markers are missing: the harnesses keep Pillow for it
    px, status = _decode(short, info=info._replace(scan_len=info.scan_len // 2, nbytes=len(short)))
    assert status == 1 and px.shape == (384, 384, 3)


# ---- the harnesses --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(seeded_sd):
    import stitch_amd
    cfg, _ = stitch_amd.load_inference_config("all_img1_with_inpaint_g12_transRef")
    m = stitch_amd.build_model(cfg)
    m.load_state_dict(seeded_sd, strict=True)
    return m.cuda().eval()


def test_eval_harness_decodes_dri_inputs_on_the_device(tmp_path, model, capsys):
    """two 512x512 pairs whose four files carry restart intervals (a row, four MCUs, an MCU, the whole image per interval): no file keeps
    Pillow, and the table is the Pillow path's"""
    from PIL import Image
    from stitch_amd import evaluate as ev
    from stitch_amd.data import structured_pair
    for d in ("input1", "input2"):
        os.makedirs(tmp_path / "testing" / d)
    kws = iter((dict(restart_marker_rows=1), dict(restart_marker_blocks=4), dict(restart_marker_blocks=1), dict(restart_marker_blocks=65535)))
    for i in range(2):
        a, b = structured_pair(512, 512, seed=710 + i, shift=(i - 1, 2 - 3 * i))
        for d, t in (("input1", a), ("input2", b)):
            Image.fromarray(t[0].permute(1, 2, 0).numpy().astype(np.uint8)).save(str(tmp_path / "testing" / d / f"{i:06d}.jpg"), quality=90, **next(kws))
    ds = ev.UDISDataset(str(tmp_path) + "/", phase="testing")
    assert len(ds) == 2
    res0, tab0 = ev.validate_with_model(model, ds, batch_size=1)
    capsys.readouterr()
    res1, tab1 = ev.validate_with_model(model, ds, batch_size=1, gpu_decode=True)
    assert "gpu_decode:" not in capsys.readouterr().out                       # no pair fell back to Pillow
    assert torch.equal(torch.as_tensor(tab0), torch.as_tensor(tab1)) and repr(res0) == repr(res1) and torch.isfinite(torch.as_tensor(tab1)).all()


def test_out_harness_writes_the_same_files_from_dri_inputs(tmp_path, model, capsys):
    """one 96x128 pair whose inputs carry restart intervals (input2 grey) through `inference_one_data`, `gpu_decode` on and off"""
    from PIL import Image
    import stitch_amd
    from stitch_amd.data import structured_pair
    spec_ = importlib.util.spec_from_file_location("stitch_out_harness_jr", os.path.join(ROOT, "out.py"))
    outmod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(outmod)
    root = tmp_path / "demo"
    (root / "p0").mkdir(parents=True)
    a, b = structured_pair(96, 128, seed=3, shift=(2, -3))
    Image.fromarray(a[0].permute(1, 2, 0).numpy().astype(np.uint8)).save(str(root / "p0" / "input1.jpg"), quality=97, restart_marker_rows=1)
    Image.fromarray(b[0].permute(1, 2, 0).numpy().astype(np.uint8)).convert("L").save(str(root / "p0" / "input2.jpg"), quality=97, restart_marker_blocks=3)
    (root / "demo.txt").write_text("p0/\n")
    for f in ("input1.jpg", "input2.jpg"):
        data = open(str(root / "p0" / f), "rb").read()
        assert stitch_amd.ops.jpeg_probe(data) is None and stitch_amd.ops.jpeg_probe(data, restart=True).restart_interval in (8, 3)
    cfg = outmod.get_config(["--data_root_path", str(root) + "/"])
    todo = outmod.get_data_dict_list(cfg.data_root_path, cfg.txt_file)
    comp = stitch_amd.composition.Network().cuda().eval()
    inp = outmod.load_inpainter("passthrough_inpainter")
    dirs = {}
    capsys.readouterr()
    for tag, kw in (("pil", {}), ("gpu", dict(gpu_decode=True))):
        dirs[tag] = str(tmp_path / tag) + "/"
        os.makedirs(dirs[tag])
        outmod.inference_one_data(cfg, todo[0], dirs[tag], model, comp, inp, **kw)
    assert "gpu_decode:" not in capsys.readouterr().out
    files = sorted(os.listdir(dirs["pil"] + "p0"))
    assert len(files) == 10
    for f in files:
        assert open(dirs["gpu"] + "p0/" + f, "rb").read() == open(dirs["pil"] + "p0/" + f, "rb").read(), f


# ---- the encoder ----------------------------------------------------------------------------------------------------------------
def _encode(u8, **kw):
    from stitch_amd import ops
    buf, n = ops.jpeg_encode(torch.from_numpy(np.ascontiguousarray(u8)).cuda(), **kw)
    return ops.jpeg_bytes(buf, n)


def _first_diff(a, b):
    k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return f"lengths {len(a)} / {len(b)}, first difference at byte {k}"


def test_every_golden_input_encodes_to_pillows_bytes(golden):
    for name, (u8, kw, data, _) in golden.items():
        got = _encode(u8, **kw)
        assert got == data, (name, _first_diff(got, data))


def test_interval_zero_is_the_existing_entrys_file():
    for u8 in (eref._smooth(75, 130, 3, 21), eref._smooth(60, 47, 0, 22)):
        want = _encode(u8)
        assert want == _pillow_file(u8)
        assert _encode(u8, restart_marker_blocks=0) == want and _encode(u8, restart_marker_blocks=0, restart_marker_rows=0) == want
        assert _encode(u8, quality=75, restart_marker_blocks=None, restart_marker_rows=None) == want


@pytest.fixture(scope="module")
def canvas():
    """two 301x403 canvases (5 814 blocks at 4:4:4: more than one 4096-entry scan tile) and their optimised files with a row per interval, from
    the restatement that tests/test_jpeg_rst_cpu.py pins to Pillow"""
    kw = dict(quality=75, subsampling=0, optimize=True, restart_marker_rows=1)
    a, b = eref._smooth(301, 403, 3, 31), eref.pattern(301, 403, 3)
    return a, rst.encode(a, **kw), b, rst.encode(b, **kw), kw


def test_optimised_encode_row_stride_streams_and_workspace_reuse(canvas):
    from stitch_amd import ops
    a, want_a, b, want_b, kw = canvas
    assert want_a[want_a.index(b"\xff\xdd"):][:6] == b"\xff\xdd\x00\x04\x00\x33"                # 51 MCUs per row
    wide = torch.full((301, 500, 3), 9, dtype=torch.uint8)
    wide[:, 40:443] = torch.from_numpy(a)
    view = wide.cuda()[:, 40:443]
    assert not view.is_contiguous()
    buf, n = ops.jpeg_encode(view, **kw)
    got = ops.jpeg_bytes(buf, n)
    assert got == want_a, _first_diff(got, want_a)
    # side streams, two in flight with different intervals
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    kw2 = dict(quality=75, subsampling=0, restart_marker_blocks=7)
    want_b7 = _pillow_file(b, **kw2)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        r1 = ops.jpeg_encode(da, **kw)
    with torch.cuda.stream(s2):
        r2 = ops.jpeg_encode(db, **kw2)
    with torch.cuda.stream(s1):
        r3 = ops.jpeg_encode(db, **kw)
    s1.synchronize(), s2.synchronize()
    assert ops.jpeg_bytes(*r1) == want_a and ops.jpeg_bytes(*r2) == want_b7 and ops.jpeg_bytes(*r3) == want_b
    # one workspace, filled with 255, reused across images and intervals
    ws = torch.full((max(ops.jpeg_workspace_bytes(301, 403, 3, **k) for k in (kw, kw2)),), 255, dtype=torch.uint8).cuda()
    for d, k, want in ((da, kw, want_a), (db, kw2, want_b7), (db, kw, want_b), (da, kw, want_a)):
        got = ops.jpeg_bytes(*ops.jpeg_encode(d, workspace=ws, **k))
        assert got == want, _first_diff(got, want)
    with pytest.raises(ops.StitchErrorBase):
        ops.jpeg_encode(da, workspace=ws[:ops.jpeg_workspace_bytes(301, 403, 3, **kw) - 16], **kw)
    for bad in (dict(restart_marker_blocks=-1), dict(restart_marker_blocks=65536), dict(restart_marker_rows=-1)):
        with pytest.raises(ValueError):
            ops.jpeg_encode(da, **bad)


def test_captured_encode_replays_on_other_pixels(canvas):
    from stitch_amd import ops
    a, want_a, b, want_b, kw = canvas
    static = torch.from_numpy(a).cuda()
    ws = torch.empty((ops.jpeg_workspace_bytes(301, 403, 3, **kw),), dtype=torch.uint8).cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ops.jpeg_encode(static, workspace=ws, **kw)                 # (module load and allocator warm-up outside the capture)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        buf, n = ops.jpeg_encode(static, workspace=ws, **kw)
    for u8, want in ((a, want_a), (b, want_b), (a, want_a)):
        static.copy_(torch.from_numpy(u8).cuda())
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = ops.jpeg_bytes(buf, n)
        assert got == want, _first_diff(got, want)


def test_round_trip_with_the_decoder():
    from stitch_amd import ops
    for u8 in (eref._smooth(75, 130, 3, 21), eref._smooth(60, 47, 0, 22)):
        buf, n = ops.jpeg_encode(torch.from_numpy(u8).cuda(), restart_marker_rows=1)
        data = ops.jpeg_bytes(buf, n)
        assert data == _pillow_file(u8, restart_marker_rows=1)
        info = ops.jpeg_probe(data, restart=True)
        assert info.restart_interval == -(-u8.shape[1] // (16 if u8.ndim == 3 else 8))
        got, status = ops.jpeg_decode(buf[:len(data)], info=info)              # the encoder's device buffer, never on the host
        got = got.cpu().numpy()
        assert int(status.item()) == 0 and np.array_equal(got[..., 0] if u8.ndim == 2 else got, cases.pillow_pixels(data))


def test_saver_writes_the_same_files_with_restart_rows_on_both_paths(tmp_path, model):
    """one 96x128 pair through `inference_one_data` with jpeg_params={"restart_marker_rows": 1} on the Pillow and the GPU saver, and today's
    files without"""
    from PIL import Image
    import stitch_amd
    from stitch_amd.data import structured_pair
    spec_ = importlib.util.spec_from_file_location("stitch_out_harness_je", os.path.join(ROOT, "out.py"))
    outmod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(outmod)
    root = tmp_path / "demo"
    (root / "p0").mkdir(parents=True)
    a, b = structured_pair(96, 128, seed=3, shift=(2, -3))
    for name, t in (("input1.jpg", a), ("input2.jpg", b)):
        Image.fromarray(t[0].permute(1, 2, 0).numpy().astype(np.uint8)).save(str(root / "p0" / name), quality=97)
    (root / "demo.txt").write_text("p0/\n")
    cfg = outmod.get_config(["--data_root_path", str(root) + "/"])
    assert "jpeg_restart_rows" not in dict(cfg) and outmod.jpeg_params_of(cfg) is None
    cfg2 = outmod.get_config(["--data_root_path", str(root) + "/", "--jpeg_restart_rows", "1", "--jpeg_restart_blocks", "3"])
    assert outmod.jpeg_params_of(cfg2) == {"restart_marker_rows": 1, "restart_marker_blocks": 3}
    todo = outmod.get_data_dict_list(cfg.data_root_path, cfg.txt_file)
    comp = stitch_amd.composition.Network().cuda().eval()
    inp = outmod.load_inpainter("passthrough_inpainter")

    def run(tag, **kw):
        d = str(tmp_path / tag) + "/"
        os.makedirs(d)
        outmod.inference_one_data(cfg, todo[0], d, model, comp, inp, **kw)
        return {f: open(d + "p0/" + f, "rb").read() for f in sorted(os.listdir(d + "p0"))}
    prm = {"restart_marker_rows": 1}
    pil, gpu = run("pil", jpeg_params=prm), run("gpu", gpu_jpeg=True, jpeg_params=prm)
    assert len(pil) == 10 and sorted(gpu) == sorted(pil)
    for f in pil:
        assert gpu[f] == pil[f], (f, _first_diff(gpu[f], pil[f]))
        assert pil[f].count(b"\xff\xdd\x00\x04") == 1
    pil0, gpu0 = run("pil0"), run("gpu0", gpu_jpeg=True)
    assert gpu0 == pil0 and all(b"\xff\xdd" not in d[:700] for d in pil0.values())
