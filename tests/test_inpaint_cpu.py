"""cv_inpainter without a GPU: the mask preprocessing restatement against PIL itself, the CPU restatement of the Telea contract
(tests/_telea_ref.py) on hand-made cases, the C-ABI's argument checks and an ISA guard on the built inpaint kernels."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import _telea_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "seamless-through-breaking-rethinking-image-stitching-for-optimal-alignment_amd")
LLVM = "/opt/rocm/llvm/bin"


def _pil_mask(mask):
    """the reference's own steps (cv_inpainter.inpaint_cv) with torch + PIL"""
    import torch
    from PIL import Image
    m = torch.from_numpy(mask)[None]
    if m.shape[1] == 1:
        m = m.repeat(1, 3, 1, 1)
    if m.max() <= 1.1:
        m = (m * 255).clamp(0, 255)
    return np.array(Image.fromarray(m[0].permute(1, 2, 0).to(torch.uint8).numpy()).convert("L"))


@pytest.mark.parametrize("kind", ["binary1", "binary3", "soft3", "u8range3", "soft1"])
def test_mask_preprocessing_matches_pil(kind):
    rng = np.random.default_rng(5)
    shape = (1 if kind.endswith("1") else 3, 37, 53)
    m = {"binary1": rng.integers(0, 2, shape).astype(np.float32), "binary3": rng.integers(0, 2, shape).astype(np.float32),
         "soft3": rng.random(shape, np.float32) * np.float32(0.012), "soft1": rng.random(shape, np.float32),
         "u8range3": rng.random(shape, np.float32) * np.float32(255)}[kind]
    got, ref = R.prep_mask(m), _pil_mask(m)
    assert got.dtype == np.uint8 and np.array_equal(got, ref)
    if kind == "soft3":
        assert 0 < (got != 0).mean() < 1


def test_image_truncation():
    v = np.array([[[-3.0, 0.2, 0.99, 1.0, 254.7, 255.0, 300.0]]] * 3, np.float32)
    assert R.prep_image(v)[0, :, 0].tolist() == [0, 0, 0, 1, 254, 255, 255]


def test_ring_distance_is_the_l1_distance():
    rng = np.random.default_rng(1)
    fill = rng.random((19, 23)) < 0.8
    d = R.ring_distance(fill)
    ky, kx = np.nonzero(~fill)
    yy, xx = np.mgrid[0:19, 0:23]
    brute = np.min(np.abs(yy[..., None] - ky) + np.abs(xx[..., None] - kx), -1)
    assert np.array_equal(d, brute)


def test_arrival_time_first_rings():
    fill = np.zeros((9, 9), bool)
    fill[2:7, 2:7] = True
    T = R.arrival_time(R.ring_distance(fill))
    assert T[2, 4] == np.float32(1) and T[2, 2] == np.float32(np.sqrt(np.float32(2)) * np.float32(0.5))
    assert T.dtype == np.float32 and (T[~fill] == 0).all()


def test_straight_edge_fills_with_the_constant_colour():
    img = np.zeros((20, 24, 3), np.uint8)
    img[:] = (10, 200, 30)
    fill = np.zeros((20, 24), bool)
    fill[:, 14:] = True
    img[fill] = 0
    out, d, _ = R.telea(img, fill, 5)
    assert d.max() == 10 and (out == np.array([10, 200, 30], np.uint8)).all()


@pytest.mark.parametrize("radius", [3, 5])
def test_linear_ramp_is_reproduced_by_the_gradient_term(radius):
    yy, xx = np.mgrid[0:24, 0:28]
    ramp = np.stack([2 * xx + 3 * yy + 10, 5 * xx + 20, 200 - 4 * yy], -1).astype(np.uint8)
    fill = np.zeros((24, 28), bool)
    fill[6:17, 7:20] = True
    img = ramp.copy()
    img[fill] = 0
    out, d, _ = R.telea(img, fill, radius)
    assert d.max() == 6 and np.array_equal(out, ramp)


def test_empty_and_all_masked():
    img = np.random.default_rng(2).integers(0, 256, (8, 9, 3)).astype(np.uint8)
    out, d, _ = R.telea(img, np.zeros((8, 9), bool), 5)
    assert np.array_equal(out, img) and (d == 0).all()
    out, d, _ = R.telea(img, np.ones((8, 9), bool), 5)
    assert np.array_equal(out, img) and (d == R.FAR).all()


def test_capi_rejects_bad_arguments_without_a_gpu():
    from stitch_amd import _lib
    lib = _lib.lib
    nb = C.c_int64()
    dp = C.c_void_p(256)            # never dereferenced: every call below is rejected on the host
    assert lib.st_inpaint_telea_workspace(64, 64, 64, C.byref(nb)) == 0 and nb.value > 64 * 64 * 16
    assert lib.st_inpaint_telea_workspace(64, 64, 0, C.byref(nb)) == 1001
    assert lib.st_inpaint_telea_workspace(64, 64, 89, C.byref(nb)) == 1001
    assert lib.st_inpaint_telea_workspace(0, 64, 5, C.byref(nb)) == 1001
    assert lib.st_inpaint_telea_workspace(64, 64, 5, None) == 1001
    assert lib.st_inpaint_prep(dp, dp, 2, dp, dp, dp, 8, 8, None) == 1001
    assert lib.st_inpaint_prep(None, dp, 3, dp, dp, dp, 8, 8, None) == 1001
    assert lib.st_inpaint_prep(dp, dp, 1, dp, dp, dp, -1, 8, None) == 1001
    assert lib.st_inpaint_telea_rings(dp, dp, 8, 8, 5, dp, 16, dp, None) == 1001          # workspace too small
    assert lib.st_inpaint_telea_rings(dp, None, 8, 8, 5, dp, 1 << 20, dp, None) == 1001
    counts = (C.c_int32 * 3)(10, 4, 0)
    assert lib.st_inpaint_telea_fill(counts, 2, 8, 8, 5, dp, 1 << 20, dp, None, None, None) == 1001   # empty ring 2
    counts = (C.c_int32 * 3)(10, 40, 40)
    assert lib.st_inpaint_telea_fill(counts, 2, 8, 8, 5, dp, 1 << 20, dp, None, None, None) == 1001   # more than h*w
    assert lib.st_inpaint_telea_fill(None, 2, 8, 8, 5, dp, 1 << 20, dp, None, None, None) == 1001
    assert lib.st_inpaint_telea_fill(counts, 17, 8, 8, 5, dp, 1 << 20, dp, None, None, None) == 1001
    assert lib.st_inpaint_telea_fill(counts, 1, 8, 8, 5, dp, 1 << 20, None, None, None, None) == 1001


def _inpaint_code_object(tmp_path):
    """the gfx950 code object of csrc/inpaint.hip out of the library's offload bundles"""
    lib = os.path.join(PKG, "libstitch_gfx950.so")
    fb = str(tmp_path / "fatbin")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fb}", lib, str(tmp_path / "lib_copy.so")])
    data = open(fb, "rb").read()
    for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data):
        s = m.start()
        (n,) = struct.unpack_from("<Q", data, s + 24)
        p = s + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            co = data[s + off:s + off + size]
            if triple.endswith("gfx950") and b"telea_ring_kernel" in co:
                path = tmp_path / "inpaint.co"
                path.write_bytes(co)
                return str(path)
    raise AssertionError("no gfx950 code object with the inpaint kernels in the library")


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-objdump"), reason="needs the ROCm LLVM tools")
def test_inpaint_kernels_isa_no_packed_fp32_no_scratch(tmp_path):
    co = _inpaint_code_object(tmp_path)
    asm = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", co], capture_output=True, text=True, check=True).stdout
    bodies = dict((m.group(1), m.group(2)) for m in re.finditer(r"^[0-9a-f]+ <(\S+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", asm, re.S | re.M))
    names = [k for k in bodies if "inpaint" in k or any(s in k for s in ("telea_ring", "dt_rows", "dt_cols", "ring_", "disc_", "prep_kernel", "unpack_kernel", "mask_max"))]
    assert any("telea_ring_kernel" in k for k in names) and any("dt_cols_kernel" in k for k in names), sorted(bodies)
    for k in names:
        assert not re.search(r"v_pk_(mul|add|fma)_f32", bodies[k]), k
        assert "scratch_" not in bodies[k], k
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", notes, re.S):
        body = m.group(2)
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", body), m.group(1)
        spill = re.search(r"\.vgpr_spill_count:\s+(\d+)", body)
        assert spill is None or int(spill.group(1)) == 0, m.group(1)
