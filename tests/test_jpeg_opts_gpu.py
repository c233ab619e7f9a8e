"""The options of csrc/jpeg.hip on the GPU: `ops.jpeg_encode(quality=, subsampling=, optimize=)` writes Pillow's file byte for byte on every golden case
(tests/golden/jpeg_opts_pil.npz) and on the code-length-limit case, whatever the row stride, stream, workspace history or hipGraph replay;
`jpeg_decode` reads the files back as Pillow does; and `out.py`'s saver writes the same ten files with the options on either path."""
import hashlib
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

import _jpeg_opts_ref as opts
import _jpeg_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_opts_pil.npz"))
    inputs = {k[3:]: z[k] for k in z.files if k.startswith("in_")}
    files = {k[4:]: z[k].tobytes() for k in z.files if k.startswith("jpg_")}
    return inputs, files, (int(z["limit_len"][0]), z["limit_sha256"].tobytes())


def _first_diff(a, b):
    n = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    return f"lengths {len(a)} / {len(b)}, first difference at byte {n}"


def _encode(u8, **kw):
    from stitch_amd import ops
    buf, n = ops.jpeg_encode(torch.from_numpy(np.ascontiguousarray(u8)).cuda(), **kw)
    assert buf.is_cuda and n.is_cuda and n.dtype == torch.int32
    return ops.jpeg_bytes(buf, n)


def test_every_golden_case_is_pillows_file(golden):
    inputs, files, _ = golden
    assert len(files) >= 113
    for name, want in files.items():
        inp, kw = opts.parse_case(name)
        got = _encode(inputs[inp], **kw)
        assert got == want, (name, _first_diff(got, want))


def test_code_length_limit_case_is_pillows_file(golden):
    """840x840 L, quality 50, optimize: the unlimited AC code is 19 bits deep, Pillow's table has one code of 15 and five of 16 bits"""
    _, _, (limit_len, limit_sha) = golden
    got = _encode(opts.limit_case(), quality=50, optimize=True)
    assert (len(got), hashlib.sha256(got).digest()) == (limit_len, limit_sha)


@pytest.fixture(scope="module")
def canvas():
    """an image of 5 814 blocks at 4:4:4 (more than one 4096-entry scan tile) and its optimised file, and a second one with other tables"""
    a, b = ref._smooth(301, 403, 3, 5), ref.pattern(301, 403, 3)
    kw = dict(quality=95, subsampling=0, optimize=True)
    return a, opts.encode(a, **kw), b, opts.encode(b, **kw), kw


def test_defaults_through_the_new_entry_are_the_old_entrys_bytes(canvas):
    a = canvas[0]
    grey = ref._smooth(137, 203, 0, 9)
    assert _encode(a, quality=75, subsampling=2) == _encode(a) == ref.encode(a)
    assert _encode(a, quality=75) == _encode(a)
    assert _encode(grey, quality=75) == _encode(grey) == ref.encode(grey)


def test_optimised_encode_row_stride_streams_and_workspace_reuse(canvas, golden):
    from stitch_amd import ops
    a, want_a, b, want_b, kw = canvas
    assert want_a != want_b and want_a[:700] != want_b[:700]         # other tables
    wide = torch.zeros((301, 448, 3), dtype=torch.uint8).cuda()
    wide[:, 17:17 + 403] = torch.from_numpy(a).cuda()
    view = wide[:, 17:17 + 403]
    assert not view.is_contiguous()
    got = ops.jpeg_bytes(*ops.jpeg_encode(view, **kw))
    assert got == want_a, _first_diff(got, want_a)
    inputs, files, _ = golden
    grey, want_l = inputs["l_15x17"], files[opts.case_name("l_15x17", 75, None, True)]
    wide_l = torch.full((15, 64), 9, dtype=torch.uint8).cuda()
    wide_l[:, 5:22] = torch.from_numpy(grey).cuda()
    assert ops.jpeg_bytes(*ops.jpeg_encode(wide_l[:, 5:22], quality=75, optimize=True)) == want_l
    # a side stream; two encodes in flight on two streams with different tables
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        r1 = ops.jpeg_encode(ta, **kw)
    with torch.cuda.stream(s2):
        r2 = ops.jpeg_encode(tb, **kw)
    with torch.cuda.stream(s1):
        r3 = ops.jpeg_encode(tb, **kw)
    s1.synchronize(), s2.synchronize()
    assert ops.jpeg_bytes(*r1) == want_a and ops.jpeg_bytes(*r2) == want_b and ops.jpeg_bytes(*r3) == want_b
    # one workspace reused: it still holds the histograms, code tables and stream bits of the larger image before it
    ws = torch.full((ops.jpeg_workspace_bytes(301, 403, 3, **kw),), 255, dtype=torch.uint8).cuda()
    assert ops.jpeg_bytes(*ops.jpeg_encode(ta, workspace=ws, **kw)) == want_a
    assert ops.jpeg_bytes(*ops.jpeg_encode(tb, workspace=ws, **kw)) == want_b
    small, want_s = inputs["noise_17x33"], files[opts.case_name("noise_17x33", 95, 0, True)]
    assert ops.jpeg_bytes(*ops.jpeg_encode(torch.from_numpy(small).cuda(), workspace=ws, **kw)) == want_s
    flat = np.full((24, 24, 3), 77, np.uint8)                       # one-symbol tables behind full ones
    assert ops.jpeg_bytes(*ops.jpeg_encode(torch.from_numpy(flat).cuda(), workspace=ws, **kw)) == opts.encode(flat, **kw)
    assert ops.jpeg_bytes(*ops.jpeg_encode(ta, workspace=ws, **kw)) == want_a
    with pytest.raises(ops.StitchErrorBase):
        ops.jpeg_encode(ta, workspace=ws[:1024], **kw)


def test_plain_encodes_ignore_the_tables_an_optimised_encode_left_in_the_workspace():
    """One workspace of the optimised size, filled with 255: an optimised encode leaves its histograms and code tables where the plain layout
    has its stream; the encodes of Pillow's defaults through either entry must read none of it."""
    from stitch_amd import ops
    H, W = 37, 53
    rng = np.random.RandomState(11)
    noise, other = rng.randint(0, 256, (H, W, 3)).astype(np.uint8), ref._smooth(H, W, 3, 13)
    kw = dict(quality=95, subsampling=0, optimize=True)
    ws = torch.full((ops.jpeg_workspace_bytes(H, W, 3, **kw),), 255, dtype=torch.uint8).cuda()
    assert ws.numel() > ops.jpeg_workspace_bytes(H, W, 3)
    got = ops.jpeg_bytes(*ops.jpeg_encode(torch.from_numpy(noise).cuda(), workspace=ws, **kw))
    assert got == opts.encode(noise, **kw), _first_diff(got, opts.encode(noise, **kw))
    want = ref.encode(other)
    got = ops.jpeg_bytes(*ops.jpeg_encode(torch.from_numpy(other).cuda(), workspace=ws))                               # st_jpeg_encode_u8
    assert got == want, _first_diff(got, want)
    got = ops.jpeg_bytes(*ops.jpeg_encode(torch.from_numpy(noise).cuda(), workspace=ws, quality=75, subsampling=2))    # _ex at {75, 2, 2, 0}
    assert got == opts.encode(noise, quality=75, subsampling=2), _first_diff(got, opts.encode(noise, quality=75, subsampling=2))


def test_captured_optimised_encode_replays_on_other_pixels(canvas):
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


@pytest.mark.parametrize("sub", [0, 1, 2, None])
def test_decoder_reads_the_files_as_pillow_does(sub):
    """jpeg_decode(jpeg_encode(x, quality=95, subsampling=s, optimize=True)): custom DHT tables and every sampling the decoder takes"""
    from PIL import Image, features
    from stitch_amd import ops
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    u8 = ref._smooth(61, 83, 3 if sub is not None else 0, 21)
    kw = dict(quality=95, optimize=True) if sub is None else dict(quality=95, subsampling=sub, optimize=True)
    buf = io.BytesIO()
    Image.fromarray(u8).save(buf, format="JPEG", **kw)
    data = _encode(u8, **kw)
    assert data == buf.getvalue()
    want = np.array(Image.open(io.BytesIO(buf.getvalue())))
    px, status = ops.jpeg_decode(data)
    got = px.cpu().numpy()
    assert int(status.item()) == 0 and np.array_equal(got.reshape(want.shape), want)


@pytest.fixture(scope="module")
def pair_runner(tmp_path_factory, seeded_sd):
    """one synthetic pair at 96x128 through `inference_one_data`: run(tag, **kw) -> {file name: bytes} of the ten result files"""
    from PIL import Image
    import stitch_amd
    from stitch_amd.data import structured_pair
    tmp_path = tmp_path_factory.mktemp("jpeg_opts_pair")
    spec_ = importlib.util.spec_from_file_location("stitch_out_harness_jo", os.path.join(ROOT, "out.py"))
    outmod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(outmod)
    root = tmp_path / "demo"
    (root / "p0").mkdir(parents=True)
    a, b = structured_pair(96, 128, seed=3, shift=(2, -3))
    for name, t in (("input1.jpg", a), ("input2.jpg", b)):
        Image.fromarray(t[0].permute(1, 2, 0).numpy().astype(np.uint8)).save(str(root / "p0" / name), quality=97)
    (root / "demo.txt").write_text("p0/\n")
    cfg = outmod.get_config(["--data_root_path", str(root) + "/"])
    todo = outmod.get_data_dict_list(cfg.data_root_path, cfg.txt_file)
    model = stitch_amd.build_model(cfg)
    model.load_state_dict(seeded_sd, strict=True)
    model = model.cuda().eval()
    comp = stitch_amd.composition.Network().cuda().eval()
    inp = outmod.load_inpainter("passthrough_inpainter")

    def run(tag, **kw):
        d = str(tmp_path / tag) + "/"
        os.makedirs(d)
        outmod.inference_one_data(cfg, todo[0], d, model, comp, inp, **kw)
        if "saver" in kw:
            kw["saver"].wait()
        return {f: open(d + "p0/" + f, "rb").read() for f in sorted(os.listdir(d + "p0"))}
    return outmod, run


def test_saver_writes_the_same_files_with_the_options_on_both_paths(pair_runner):
    outmod, run = pair_runner
    prm = dict(quality=95, subsampling=0, optimize=True)
    pil = run("pil", jpeg_params=prm)
    gpu = run("gpu", gpu_jpeg=True, jpeg_params=prm)
    own = run("own", saver=outmod._Saver(gpu_jpeg=True, jpeg_params=prm))
    assert len(pil) == 10 and sorted(gpu) == sorted(pil) == sorted(own)
    for f in pil:
        assert gpu[f] == pil[f] and own[f] == pil[f], (f, _first_diff(gpu[f], pil[f]))
    sof = {f: d[d.index(b"\xff\xc0") + 9:d.index(b"\xff\xc0") + 12] for f, d in pil.items()}
    assert sof["mask1.jpg"] == b"\x01\x01\x11" and sof["warp1.jpg"] == b"\x03\x01\x11"          # L: one component; RGB: 4:4:4
    assert all(d.index(b"\xff\xda") + (10 if sof[f][0] == 1 else 14) < (328 if sof[f][0] == 1 else 623) for f, d in pil.items())   # optimised tables


def test_without_jpeg_params_the_pair_writes_todays_files(pair_runner):
    outmod, run = pair_runner
    pil = run("pil0")
    gpu = run("gpu0", gpu_jpeg=True)
    none = run("gpu_none", gpu_jpeg=True, jpeg_params=None)
    assert len(pil) == 10 and gpu == pil and none == pil
    for f, d in pil.items():                                        # Pillow's defaults: the Annex K header
        ncomp = d[d.index(b"\xff\xc0") + 9]
        H, W = int.from_bytes(d[d.index(b"\xff\xc0") + 5:][:2], "big"), int.from_bytes(d[d.index(b"\xff\xc0") + 7:][:2], "big")
        assert d[:ref.HEADER_BYTES[ncomp]] == ref.header(H, W, ncomp), f
