"""csrc/jpeg.hip on the GPU: `ops.jpeg_encode` writes Pillow's file byte for byte on every golden case (tests/golden/jpeg_pil.npz), on a
result-canvas-sized image against the CPU restatement, whatever the row stride, stream or workspace history, and `out.py`'s saver
writes the same ten files with it as with Pillow."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _jpeg_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz"))
    return {k[3:]: (z[k], z["jpg_" + k[3:]].tobytes()) for k in z.files if k.startswith("in_")}


def _first_diff(a, b):
    n = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    return f"lengths {len(a)} / {len(b)}, first difference at byte {n}"


def _encode(u8, **kw):
    from stitch_amd import ops
    buf, n = ops.jpeg_encode(torch.from_numpy(np.ascontiguousarray(u8)).cuda(), **kw)
    assert buf.is_cuda and n.is_cuda and n.dtype == torch.int32
    return ops.jpeg_bytes(buf, n)


def test_every_golden_case_is_pillows_file(golden):
    """incl. 130x1030 RGB (more blocks than one 4096-entry scan tile, several MCU rows) and 24x2056 L (one long row of blocks)"""
    assert "big_rgb_130x1030" in golden and "big_l_24x2056" in golden
    for name, (u8, want) in golden.items():
        got = _encode(u8)
        assert got == want, (name, _first_diff(got, want))


@pytest.fixture(scope="module")
def canvas():
    u8 = ref._smooth(548, 588, 3, 5)
    return u8, ref.encode(u8)


def test_result_canvas_equals_the_restatement(canvas):
    u8, want = canvas
    got = _encode(u8)
    assert got == want, _first_diff(got, want)


def test_row_stride_streams_and_workspace_reuse(canvas, golden):
    from stitch_amd import ops
    u8, want = canvas
    # a column slice of a wider canvas: rows 640 * 3 bytes apart
    wide = torch.zeros((548, 640, 3), dtype=torch.uint8).cuda()
    wide[:, 17:17 + 588] = torch.from_numpy(u8).cuda()
    view = wide[:, 17:17 + 588]
    assert not view.is_contiguous()
    assert ops.jpeg_bytes(*ops.jpeg_encode(view)) == want
    grey, want_l = golden["l_33x41"]
    wide_l = torch.full((33, 64), 9, dtype=torch.uint8).cuda()
    wide_l[:, 5:46] = torch.from_numpy(grey).cuda()
    assert ops.jpeg_bytes(*ops.jpeg_encode(wide_l[:, 5:46])) == want_l
    # a side stream; two encodes in flight on two streams
    noise, want_n = golden["noise_64x48"]
    a, b = torch.from_numpy(u8).cuda(), torch.from_numpy(noise).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        r1 = ops.jpeg_encode(a)
    with torch.cuda.stream(s2):
        r2 = ops.jpeg_encode(b)
    with torch.cuda.stream(s1):
        r3 = ops.jpeg_encode(b)
    s1.synchronize(), s2.synchronize()
    assert ops.jpeg_bytes(*r1) == want and ops.jpeg_bytes(*r2) == want_n and ops.jpeg_bytes(*r3) == want_n
    # one workspace reused: it still holds the bits of the larger, busier stream before it; zeroing is part of the call
    ws = torch.full((ops.jpeg_workspace_bytes(548, 588, 3),), 255, dtype=torch.uint8).cuda()
    assert ops.jpeg_bytes(*ops.jpeg_encode(a, workspace=ws)) == want
    assert ops.jpeg_bytes(*ops.jpeg_encode(b, workspace=ws)) == want_n
    zeros, want_z = golden["zeros_24x24"]
    assert ops.jpeg_bytes(*ops.jpeg_encode(torch.from_numpy(zeros).cuda(), workspace=ws)) == want_z
    assert ops.jpeg_bytes(*ops.jpeg_encode(a, workspace=ws)) == want
    with pytest.raises(ops.StitchErrorBase):
        ops.jpeg_encode(a, workspace=ws[:1024])


def test_saver_writes_the_same_files_with_gpu_jpeg(tmp_path, seeded_sd):
    """one synthetic pair at 96x128 through `inference_one_data`: `_Saver(gpu_jpeg=True)` and `_Saver()` write identical files"""
    from PIL import Image
    import stitch_amd
    from stitch_amd.data import structured_pair
    spec_ = importlib.util.spec_from_file_location("stitch_out_harness_j", os.path.join(ROOT, "out.py"))
    outmod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(outmod)
    root = tmp_path / "demo"
    (root / "p0").mkdir(parents=True)
    a, b = structured_pair(96, 128, seed=3, shift=(2, -3))
    for name, t in (("input1.jpg", a), ("input2.jpg", b)):
        Image.fromarray(t[0].permute(1, 2, 0).numpy().astype(np.uint8)).save(str(root / "p0" / name), quality=97)
    (root / "demo.txt").write_text("p0/\n")
    cfg = outmod.get_config(["--data_root_path", str(root) + "/"])
    assert not getattr(cfg, "gpu_jpeg", False) and outmod.get_config(["--data_root_path", str(root) + "/", "--gpu_jpeg"]).gpu_jpeg is True
    todo = outmod.get_data_dict_list(cfg.data_root_path, cfg.txt_file)
    model = stitch_amd.build_model(cfg)
    model.load_state_dict(seeded_sd, strict=True)
    model = model.cuda().eval()
    comp = stitch_amd.composition.Network().cuda().eval()
    inp = outmod.load_inpainter("passthrough_inpainter")
    dirs = {}
    for tag, kw in (("pil", dict(saver=outmod._Saver())), ("gpu", dict(saver=outmod._Saver(gpu_jpeg=True))), ("kw", dict(gpu_jpeg=True))):
        dirs[tag] = str(tmp_path / tag) + "/"
        os.makedirs(dirs[tag])
        outmod.inference_one_data(cfg, todo[0], dirs[tag], model, comp, inp, **kw)
        kw.get("saver", outmod._Saver()).wait()
    files = sorted(os.listdir(dirs["pil"] + "p0"))
    assert len(files) == 10
    for tag in ("gpu", "kw"):
        assert sorted(os.listdir(dirs[tag] + "p0")) == files
        for f in files:
            assert open(dirs[tag] + "p0/" + f, "rb").read() == open(dirs["pil"] + "p0/" + f, "rb").read(), (tag, f)
