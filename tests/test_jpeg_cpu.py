"""The JPEG contract, decided on the CPU: tests/_jpeg_ref.py (what csrc/jpeg.hip implements) equals Pillow's files byte for byte, the golden
cases exercise every rule of the contract (a planted defect changes a file), the C entry rejects bad arguments before any launch, the size
queries of both entries return the documented formulas, and the kernels use no scratch and the LDS the README states."""
import ctypes as C
import importlib.util
import io
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _jpeg_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = ["rgb_1x1", "rgb_8x8", "rgb_16x16", "rgb_17x23", "rgb_18x16", "rgb_16x24", "rgb_9x40", "rgb_40x9", "rgb_25x17", "l_33x41", "mask_37x53",
            "zeros_24x24", "ones_24x40", "noise_64x48", "zrl_8x8", "big_rgb_130x1030", "big_l_24x2056"]


@pytest.fixture(scope="module")
def golden():
    path = os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz")
    assert os.path.getsize(path) < 200 * 1024
    z = np.load(path)
    cases = {k[3:]: (z[k], z["jpg_" + k[3:]].tobytes()) for k in z.files if k.startswith("in_")}
    assert set(REQUIRED) <= set(cases)
    return cases


def test_restatement_equals_the_golden_files(golden):
    built = ref.golden_cases()
    assert set(built) == set(golden)
    for name, (u8, want) in golden.items():
        assert np.array_equal(built[name], u8), name                 # the stored inputs are the ones the builders make
        assert u8.dtype == np.uint8
        got = ref.encode(u8)
        assert got == want, (name, len(got), len(want))
        hdr = ref.HEADER_BYTES[3 if u8.ndim == 3 else 1]
        assert want[:2] == b"\xff\xd8" and want[-2:] == b"\xff\xd9" and want[:hdr] == ref.header(u8.shape[0], u8.shape[1], 3 if u8.ndim == 3 else 1)


def test_golden_scans_hold_stuffed_bytes_and_zrl_codes(golden):
    n_ff00 = sum(want[ref.HEADER_BYTES[3 if u8.ndim == 3 else 1]:-2].count(b"\xff\x00") for u8, want in golden.values())
    stats = {}
    ref.encode(golden["zrl_8x8"][0], stats=stats)
    assert n_ff00 >= 1 and stats["zrl"] >= 1
    # all-0 and all-255 images: every block after the first is a zero DC difference and an EOB
    for name in ("zeros_24x24", "ones_24x40"):
        coefs, _ = ref.scan_blocks(golden[name][0])
        assert not coefs[:, 1:].any()


def test_restatement_equals_live_pillow(golden):
    from PIL import Image, features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo: the contract restates libjpeg-turbo's arithmetic (the golden comparison still runs)")
    for name, (u8, _) in golden.items():
        buf = io.BytesIO()
        Image.fromarray(u8).save(buf, format="JPEG")
        assert ref.encode(u8) == buf.getvalue(), name


@pytest.mark.parametrize("defect", ref.DEFECTS)
def test_a_planted_defect_changes_a_golden_file(golden, defect):
    changed = [name for name, (u8, want) in golden.items() if not name.startswith("big_") and ref.encode(u8, defect=defect) != want]
    assert changed, defect


def test_entry_rejects_bad_arguments_without_touching_the_gpu():
    from stitch_amd._lib import lib
    enc, ws_bytes, max_bytes = lib.st_jpeg_encode_u8, lib.st_jpeg_workspace_bytes, lib.st_jpeg_max_bytes
    base = 0x7f0000000000                                           # never dereferenced on the host
    src, out, nb, ws = base, base + (1 << 30), base + (2 << 30), base + (3 << 30)
    H, W = 37, 53
    cap, need = max_bytes(H, W, 3), ws_bytes(H, W, 3)
    nblocks = 6 * 3 * 4
    assert cap == 623 + 2 * ((nblocks * (20 + 63 * 26) + 7) // 8) + 2 and need > nblocks * 128
    assert max_bytes(33, 41, 1) == 328 + 2 * ((5 * 6 * (20 + 63 * 26) + 7) // 8) + 2

    def call(src=src, H=H, W=W, ch=3, stride=None, out=out, cap=cap, nb=nb, ws=ws, need=need):
        return enc(src, H, W, ch, W * ch if stride is None else stride, out, cap, nb, ws, need, None)
    assert call(src=None) == 1001 and call(out=None) == 1001 and call(nb=None) == 1001 and call(ws=None) == 1001
    assert call(ch=2) == 1001 and call(ch=0) == 1001 and call(ch=4) == 1001
    assert call(H=0) == 1001 and call(W=0) == 1001 and call(W=65536, cap=1 << 40, need=1 << 40) == 1001 and call(H=65536, cap=1 << 40, need=1 << 40) == 1001
    assert call(H=4096, W=4097, cap=1 << 40, need=1 << 40) == 1001                    # H * W above 2^24
    assert max_bytes(4096, 4096, 3) > 0 and max_bytes(4096, 4097, 3) == 0 and ws_bytes(65535, 256, 1) > 0 and ws_bytes(65535, 257, 1) == 0
    assert call(cap=cap - 1) == 1001                                                   # capacity one byte short of the worst case
    assert call(need=need - 1) == 1001 and call(ws=ws + 4) == 1001 and call(stride=W * 3 - 1) == 1001


SIZE_SHAPES = [(1, 1, 1), (1, 1, 3), (37, 53, 3), (33, 41, 1), (548, 588, 3), (4096, 4096, 3), (65535, 256, 1)]


def test_size_queries_return_the_documented_formulas():
    """No GPU is touched.  Both entries at Pillow's defaults: the layout without a table area; `optimize` adds the table area, a constant."""
    from stitch_amd._lib import JpegEncParams, lib

    def a16(v):
        return (v + 15) & ~15
    extra = set()
    for H, W, ch in SIZE_SHAPES:
        nb = 6 * -(-W // 16) * -(-H // 16) if ch == 3 else -(-W // 8) * -(-H // 8)
        bits = nb * 1658
        words, nbytes = -(-bits // 32) + 4, -(-bits // 8)
        chunks = -(-nbytes // 2048)
        ws = a16(128 * nb) + a16(4 * nb) + a16(4 * chunks) + 16 + a16(4 * words)
        out = (623 if ch == 3 else 328) + 2 * nbytes + 2
        assert (lib.st_jpeg_workspace_bytes(H, W, ch), lib.st_jpeg_max_bytes(H, W, ch)) == (ws, out), (H, W, ch)
        s = 2 if ch == 3 else 1
        plain, opt = JpegEncParams(75, s, s, 0), JpegEncParams(75, s, s, 1)
        assert (lib.st_jpeg_workspace_bytes_ex(H, W, ch, C.byref(plain)), lib.st_jpeg_max_bytes_ex(H, W, ch, C.byref(plain))) == (ws, out), (H, W, ch)
        assert lib.st_jpeg_max_bytes_ex(H, W, ch, C.byref(opt)) == out
        extra.add(lib.st_jpeg_workspace_bytes_ex(H, W, ch, C.byref(opt)) - ws)
    (table_area,) = extra                                           # the same for every shape: four code tables, DHT payloads and histograms
    assert table_area >= 9312 and table_area % 16 == 0


def _resource_report():
    spec = importlib.util.spec_from_file_location("_stitch_build", os.path.join(ROOT, "seamless-through-breaking-rethinking-image-stitching-for-optimal-alignment_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "jpeg.s")
        subprocess.check_call(build.compile_cmd("jpeg.hip", out, ["-S", "--cuda-device-only"]), stderr=subprocess.DEVNULL)
        text = open(out).read()
    rep = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+)\n.*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)",
                         text, re.S):
        if "jpegr_" not in m.group(2):                              # (the restart kernels' rows: tests/test_jpeg_rst_cpu.py)
            rep[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    return rep, text


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_kernels_use_no_scratch_and_the_stated_lds():
    rep, text = _resource_report()
    lds = {"jpeg_blocks_kernelILi1ELi1ELi1E": 8704, "jpeg_blocks_kernelILi3ELi1ELi1E": 6528, "jpeg_blocks_kernelILi3ELi2ELi1E": 10752,
           "jpeg_blocks_kernelILi3ELi2ELi2E": 17152, "jpeg_hist_kernel": 4112, "jpeg_table_kernel": 1808, "jpeg_bits_kernel": 2176, "jpeg_scan_kernel": 68,
           "jpeg_zero_kernel": 0, "jpeg_pack_kernel": 2176, "jpeg_count_kernel": 16, "jpeg_stuff_kernel": 16}
    assert len(rep) == len(lds), sorted(rep)
    readme = open(os.path.join(ROOT, "README.md")).read()
    readme = readme[readme.index("## gpu_jpeg"):readme.index("## gpu_decode")]             # (the decoder's table lists the scan kernel too)
    for key, want in lds.items():
        (name, r), = [(n, r) for n, r in rep.items() if key in n]
        assert r["scratch"] == 0 and r["spill"] == 0 and r["lds"] == want and r["vgpr"] <= 64, (name, r)
        row, = [l for l in readme.splitlines() if l.startswith("| `" + re.sub(r"ILi(\d)ELi(\d)ELi(\d)E", r"<\1, \2, \3>", key) + "`")]
        assert row.rstrip().endswith(f"| {want} |"), row                                    # the README's kernel table states the same LDS
    assert not re.search(r"^\s*scratch_(load|store)", text, re.M)                           # no stack traffic at all
