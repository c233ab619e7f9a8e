"""csrc/jpeg_dec.hip on the GPU: `ops.jpeg_decode` gives Pillow's pixels bit for bit on every golden file (tests/golden/jpeg_dec_pil.npz and
the encoder's 18 files), the restatement's on the product's shape, on a stream that spans three workgroups of subsequences, on the flat image
whose stream never synchronises and on a 1x1 file -- whatever the row stride, stream or workspace history -- and decodes what
`ops.jpeg_encode` writes; a cut file sets the status word; `evaluate` and `out.py` compute the same results with `gpu_decode` as without."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _jpeg_dec_cases as cases
import _jpeg_dec_ref as ref
import _jpeg_ref as eref

pytestmark = pytest.mark.gpu

ROOT = cases.ROOT


@pytest.fixture(scope="module")
def golden():
    return cases.load_golden()


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
    for name, (data, px, sha) in golden.items():
        got, status = _decode(data)
        assert status == 0, name
        assert cases.same_pixels(got, px, sha), (name, _diff(got, px) if px is not None else "digest")


@pytest.fixture(scope="module")
def generated():
    """{name: (file, the restatement's pixels)}; checked against live Pillow too where there is one"""
    files = {"product_512": eref.encode(eref._smooth(512, 512, 3, 5)),
             "three_workgroups": eref.encode(np.random.RandomState(5).randint(0, 256, (384, 384, 3)).astype(np.uint8)),
             "zeros_512": cases.zeros_file(),
             "one_pixel": eref.encode(np.full((1, 1, 3), 77, np.uint8))}
    out = {}
    for name, data in files.items():
        want = ref.decode(data)
        if cases.pillow_turbo():
            assert np.array_equal(want, cases.pillow_pixels(data)), name
        out[name] = (data, want)
    info = ref.probe(files["three_workgroups"])
    assert info["scan_len"] * 8 > 2 * cases.SUB_BITS * cases.SYNC_THREADS                      # at least three workgroups of subsequences
    assert ref.probe(files["one_pixel"])["scan_len"] * 8 < cases.SUB_BITS
    return out


@pytest.mark.parametrize("name", ["product_512", "three_workgroups", "zeros_512", "one_pixel"])
def test_generated_files_equal_the_restatement(generated, name):
    data, want = generated[name]
    got, status = _decode(data)
    assert status == 0 and np.array_equal(got, want), _diff(got, want)


def test_row_stride_streams_and_workspace_reuse(generated, golden):
    from stitch_amd import ops
    data, want = generated["product_512"]
    small, want_s, _ = golden["420_64x48_q95"]
    grey, want_g, _ = golden["l_33x15_q75"]
    info, info_s, info_g = ops.jpeg_probe(data), ops.jpeg_probe(small), ops.jpeg_probe(grey)
    # a column slice of a wider canvas, untouched around it
    wide = torch.full((512, 640, 3), 9, dtype=torch.uint8).cuda()
    view = wide[:, 17:17 + 512]
    assert not view.is_contiguous()
    out, status = ops.jpeg_decode(data, out=view)
    assert out.data_ptr() == view.data_ptr() and int(status.item()) == 0
    w = wide.cpu().numpy()
    assert np.array_equal(w[:, 17:529], want) and (w[:, :17] == 9).all() and (w[:, 529:] == 9).all()
    wide_g = torch.full((33, 40, 1), 9, dtype=torch.uint8).cuda()
    ops.jpeg_decode(grey, out=wide_g[:, 5:20])
    assert np.array_equal(wide_g.cpu().numpy()[:, 5:20, 0], want_g) and (wide_g.cpu().numpy()[:, :5] == 9).all()
    # device bytes with the host's probe; a side stream; two decodes in flight on two streams
    dev, dev_s = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda(), torch.frombuffer(bytearray(small), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        r1 = ops.jpeg_decode(dev, info=info)
    with torch.cuda.stream(s2):
        r2 = ops.jpeg_decode(dev_s, info=info_s)
    with torch.cuda.stream(s1):
        r3 = ops.jpeg_decode(dev_s, info=info_s)
    s1.synchronize(), s2.synchronize()
    assert np.array_equal(r1[0].cpu().numpy(), want) and np.array_equal(r2[0].cpu().numpy(), want_s) and np.array_equal(r3[0].cpu().numpy(), want_s)
    assert [int(r[1].item()) for r in (r1, r2, r3)] == [0, 0, 0]
    # one workspace reused: it still holds the larger image's stream, states and coefficients
    ws = torch.full((ops.jpeg_dec_workspace_bytes(info),), 255, dtype=torch.uint8).cuda()
    for d, i, wnt in ((dev, info, want), (dev_s, info_s, want_s), (grey, info_g, want_g[..., None]), (dev, info, want)):
        px, st = ops.jpeg_decode(d, info=i, workspace=ws)
        assert int(st.item()) == 0 and np.array_equal(px.cpu().numpy(), wnt)
    with pytest.raises(ops.StitchErrorBase):
        ops.jpeg_decode(dev, info=info, workspace=ws[:1024])
    with pytest.raises(ops.StitchErrorBase):
        ops.jpeg_decode(b"\xff\xd8 not a jpeg")


def test_round_trip_with_the_encoder():
    from stitch_amd import ops
    for u8 in (eref._smooth(75, 130, 3, 21), eref._smooth(60, 47, 0, 22)):
        buf, n = ops.jpeg_encode(torch.from_numpy(u8).cuda())
        data = ops.jpeg_bytes(buf, n)
        assert data == eref.encode(u8)
        info = ops.jpeg_probe(data)
        got, status = ops.jpeg_decode(buf[:len(data)], info=info)              # the encoder's device buffer, never on the host
        want = ref.decode(data)
        if cases.pillow_turbo():
            assert np.array_equal(want, cases.pillow_pixels(data))
        got = got.cpu().numpy()
        assert int(status.item()) == 0 and np.array_equal(got[..., 0] if u8.ndim == 2 else got, want)


def test_guards_return_before_a_launch_and_a_cut_file_sets_the_status(golden):
    from stitch_amd import ops
    data = golden["420_64x48_q75"][0]
    info = ops.jpeg_probe(data)
    need = ops.jpeg_dec_workspace_bytes(info)
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    out = torch.full((64, 48, 3), 7, dtype=torch.uint8).cuda()
    status = torch.full((1,), -5, dtype=torch.int32).cuda()
    ws = torch.zeros((need + 16,), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    call = cases.entry_call(info, dev.data_ptr(), out.data_ptr(), status.data_ptr(), ws.data_ptr(), need)
    cases.guard_cases(call, len(data), need, info.W, info.ncomp)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7).all() and int(status.item()) == -5 and not ws.cpu().numpy().any()       # nothing ran
    short = cases.cut(data, info, fraction=0.5)
    i2 = ops.jpeg_probe(short)
    assert i2 is not None and i2.scan_len == info.scan_len // 2
    px, st = ops.jpeg_decode(short, info=i2)
    torch.cuda.synchronize()
    assert int(st.item()) == 1 and tuple(px.shape) == (64, 48, 3)
    assert call() == 0 and int(status.item()) == 0 and np.array_equal(out.cpu().numpy(), golden["420_64x48_q75"][1])


# ---- the harnesses --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(seeded_sd):
    import stitch_amd
    cfg, _ = stitch_amd.load_inference_config("all_img1_with_inpaint_g12_transRef")
    m = stitch_amd.build_model(cfg)
    m.load_state_dict(seeded_sd, strict=True)
    return m.cuda().eval()


def test_eval_harness_returns_the_same_table_with_gpu_decode(tmp_path, model, capsys):
    """four 512x512 pairs (the one shape `test_eval` takes: its homography head expects the 4096 features of a 512x512 input), one file
    of them progressive: that pair keeps Pillow (one printed line), the others are decoded on the device"""
    from PIL import Image
    from stitch_amd import evaluate as ev
    from stitch_amd.data import structured_pair
    for d in ("input1", "input2"):
        os.makedirs(tmp_path / "testing" / d)
    for i in range(4):
        a, b = structured_pair(512, 512, seed=700 + i, shift=(i - 2, 3 - 2 * i))
        for d, t in (("input1", a), ("input2", b)):
            Image.fromarray(t[0].permute(1, 2, 0).numpy().astype(np.uint8)).save(str(tmp_path / "testing" / d / f"{i:06d}.jpg"), quality=90,
                                                                                  progressive=(i == 2 and d == "input2"))
    ds = ev.UDISDataset(str(tmp_path) + "/", phase="testing")
    assert len(ds) == 4
    res0, tab0 = ev.validate_with_model(model, ds, batch_size=1)
    capsys.readouterr()
    res1, tab1 = ev.validate_with_model(model, ds, batch_size=1, gpu_decode=True)
    printed = capsys.readouterr().out
    assert printed.count("gpu_decode:") == 1 and "000002.jpg" in printed
    assert torch.equal(torch.as_tensor(tab0), torch.as_tensor(tab1)) and repr(res0) == repr(res1) and torch.isfinite(torch.as_tensor(tab1)).all()
    res2, tab2 = ev.validate_with_model(model, ds, batch_size=2, gpu_decode=True)          # a batch with the Pillow pair in it, a batch without
    res3, tab3 = ev.validate_with_model(model, ds, batch_size=2)
    assert torch.equal(torch.as_tensor(tab2), torch.as_tensor(tab3))
    with pytest.raises(ValueError):
        ev.validate_with_model(model, ds, pipelined=False, gpu_decode=True)
    # a cut file: the status word is read back with the table, the error names the file
    path = ds.image_list[1][0]
    data = open(path, "rb").read()
    from stitch_amd import ops
    open(path, "wb").write(cases.cut(data, ops.jpeg_probe(data), fraction=0.5))
    with pytest.raises(RuntimeError, match="000001.jpg"):
        ev.validate_with_model(model, ds, batch_size=1, gpu_decode=True)


def test_out_harness_writes_the_same_files_with_gpu_decode(tmp_path, model):
    """one 96x128 pair (input2 grey: tiled to three channels) through `inference_one_data` and `run_pairs`, `gpu_decode` on and off"""
    from PIL import Image
    import stitch_amd
    from stitch_amd.data import structured_pair
    spec_ = importlib.util.spec_from_file_location("stitch_out_harness_jd", os.path.join(ROOT, "out.py"))
    outmod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(outmod)
    root = tmp_path / "demo"
    (root / "p0").mkdir(parents=True)
    a, b = structured_pair(96, 128, seed=3, shift=(2, -3))
    Image.fromarray(a[0].permute(1, 2, 0).numpy().astype(np.uint8)).save(str(root / "p0" / "input1.jpg"), quality=97)
    Image.fromarray(b[0].permute(1, 2, 0).numpy().astype(np.uint8)).convert("L").save(str(root / "p0" / "input2.jpg"), quality=97)
    (root / "demo.txt").write_text("p0/\n")
    cfg = outmod.get_config(["--data_root_path", str(root) + "/"])
    assert "gpu_decode" not in dict(cfg) and outmod.get_config(["--data_root_path", str(root) + "/", "--gpu_decode"]).gpu_decode is True
    todo = outmod.get_data_dict_list(cfg.data_root_path, cfg.txt_file)
    comp = stitch_amd.composition.Network().cuda().eval()
    inp = outmod.load_inpainter("passthrough_inpainter")
    dirs = {}
    for tag, kw in (("pil", {}), ("gpu", dict(gpu_decode=True))):
        dirs[tag] = str(tmp_path / tag) + "/"
        os.makedirs(dirs[tag])
        outmod.inference_one_data(cfg, todo[0], dirs[tag], model, comp, inp, **kw)
    dirs["loop"] = str(tmp_path / "loop") + "/"
    os.makedirs(dirs["loop"])
    outmod.run_pairs(cfg, todo, dirs["loop"], model, comp, inp, gpu_decode=True)
    files = sorted(os.listdir(dirs["pil"] + "p0"))
    assert len(files) == 10
    for tag in ("gpu", "loop"):
        assert sorted(os.listdir(dirs[tag] + "p0")) == files
        for f in files:
            assert open(dirs[tag] + "p0/" + f, "rb").read() == open(dirs["pil"] + "p0/" + f, "rb").read(), (tag, f)
