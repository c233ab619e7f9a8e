"""The contract of the JPEG encoder's options, decided on the CPU: tests/_jpeg_opts_ref.py (what csrc/jpeg.hip implements behind
`st_jpeg_encode_u8_ex`) equals Pillow's files byte for byte at every quality, sampling and with optimised tables; the golden cases exercise
every rule (a planted defect changes a file); the C entry rejects bad arguments before any launch; and the table builder the kernel runs
(csrc/jpeg_huff_core.h) gives the restatement's tables on 1 000 histograms under the host compiler's sanitizers."""
import ctypes as C
import hashlib
import importlib.util
import io
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import _jpeg_opts_ref as opts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "seamless-through-breaking-rethinking-image-stitching-for-optimal-alignment_amd")


@pytest.fixture(scope="module")
def golden():
    path = os.path.join(ROOT, "tests", "golden", "jpeg_opts_pil.npz")
    assert os.path.getsize(path) < 200 * 1024
    z = np.load(path)
    inputs = {k[3:]: z[k] for k in z.files if k.startswith("in_")}
    files = {k[4:]: z[k].tobytes() for k in z.files if k.startswith("jpg_")}
    return inputs, files, (int(z["limit_len"][0]), z["limit_sha256"].tobytes())


@pytest.fixture(scope="module")
def limit_image():
    return opts.limit_case()


def test_restatement_equals_the_golden_files(golden, limit_image):
    inputs, files, (limit_len, limit_sha) = golden
    built = opts.golden_inputs()
    assert set(built) == set(inputs) and sorted(files) == sorted(opts.golden_cases())
    for name, u8 in inputs.items():
        assert np.array_equal(built[name], u8) and u8.dtype == np.uint8, name
    for h, w in opts.SIZES:                                         # the cases the contract names
        for s in (0, 1, 2):
            assert opts.case_name(f"rgb_{h}x{w}", 75, s, True) in files and opts.case_name(f"rgb_{h}x{w}", 75, s, False) in files
    for name, want in files.items():
        inp, kw = opts.parse_case(name)
        got = opts.encode(inputs[inp], **kw)
        assert got == want, (name, len(got), len(want))
    got = opts.encode(limit_image, quality=50, optimize=True)
    assert (len(got), hashlib.sha256(got).digest()) == (limit_len, limit_sha)


def test_goldens_reach_the_corners(golden, limit_image):
    inputs, files, _ = golden
    # one-symbol tables: a 1-bit code each (DHT: 16 counts with a single 1 at length 1, one symbol)
    flat = files[opts.case_name("flat_l_8x8", 75, None, True)]
    assert flat.count(b"\xff\xc4\x00\x14") == 2 and len(flat) < 328
    stats = {}
    opts.encode(inputs["wave_l_64x64"], quality=100, optimize=True, stats=stats)
    assert stats["max_dc"] == 11 and stats["max_ac"] == 10
    n_ff00 = sum(f[f.index(b"\xff\xda") + 2:-2].count(b"\xff\x00") for n, f in files.items() if n.endswith("__o1"))
    zrl = 0
    for q in opts.QUALITIES:
        st = {}
        opts.encode(inputs["noise_17x33"], quality=q, subsampling=2, optimize=True, stats=st)
        zrl += st["zrl"]
    assert n_ff00 >= 1 and zrl >= 1
    # quality 1: quantisers of 255; quality 100: all ones
    for q, want in ((1, 255), (100, 1)):
        f = files[opts.case_name("noise_17x33", q, 0, False)]
        at = f.index(b"\xff\xdb")
        assert set(f[at + 5:at + 69]) == {want} and set(f[at + 74:at + 138]) == {want}
    # header length varies with the tables
    a, b = files[opts.case_name("noise_17x33", 75, 2, False)], files[opts.case_name("noise_17x33", 75, 2, True)]
    assert a.index(b"\xff\xda") + 14 == 623 and b.index(b"\xff\xda") + 14 < 623
    st = {}
    opts.encode(limit_image, quality=50, optimize=True, stats=st)
    assert st["depth"][1] > 16 and list(st["tabs"][1][0][13:16]) == [0, 1, 5]


def test_restatement_equals_live_pillow(golden, limit_image):
    from PIL import Image, features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo: the contract restates libjpeg-turbo's arithmetic (the golden comparison still runs)")

    def pil(u8, **kw):
        buf = io.BytesIO()
        Image.fromarray(u8).save(buf, format="JPEG", **kw)
        return buf.getvalue()
    inputs, files, (limit_len, limit_sha) = golden
    for name, want in files.items():
        inp, kw = opts.parse_case(name)
        assert pil(inputs[inp], **kw) == want, name
    data = pil(limit_image, quality=50, optimize=True)
    assert (len(data), hashlib.sha256(data).digest()) == (limit_len, limit_sha)
    rng = np.random.RandomState(5)                                   # beyond the goldens: every quality once, random sizes
    for q in range(1, 101):
        h, w = rng.randint(1, 40, 2)
        u8 = rng.randint(0, 256, (h, w, 3)).astype(np.uint8) if q % 4 else opts.ref._smooth(h, w, 0, q)
        kw = dict(quality=q, optimize=bool(q & 1))
        if u8.ndim == 3 and q % 3:
            kw["subsampling"] = (q // 4) % 3
        assert opts.encode(u8, **kw) == pil(u8, **kw), (q, h, w, kw)


@pytest.mark.parametrize("defect", opts.DEFECTS)
def test_a_planted_defect_changes_a_golden_file(golden, limit_image, defect):
    inputs, files, (limit_len, limit_sha) = golden
    for name, want in files.items():
        inp, kw = opts.parse_case(name)
        if opts.encode(inputs[inp], defect=defect, **kw) != want:
            return
    got = opts.encode(limit_image, quality=50, optimize=True, defect=defect)      # the only case with codes longer than 16 bits
    assert (len(got), hashlib.sha256(got).digest()) != (limit_len, limit_sha), defect


def test_entry_rejects_bad_arguments_without_touching_the_gpu():
    from stitch_amd._lib import JpegEncParams, lib
    enc, ws_bytes, max_bytes = lib.st_jpeg_encode_u8_ex, lib.st_jpeg_workspace_bytes_ex, lib.st_jpeg_max_bytes_ex
    assert lib.st_abi_jpeg_enc_params_size() == C.sizeof(JpegEncParams) == 32
    base = 0x7f0000000000                                           # never dereferenced on the host
    src, out, nb, ws = base, base + (1 << 30), base + (2 << 30), base + (3 << 30)
    H, W = 37, 53

    def P(quality=95, hs=1, vs=1, optimize=1, reserved=(0, 0, 0, 0)):
        return JpegEncParams(quality, hs, vs, optimize, (C.c_int32 * 4)(*reserved))
    p = P()
    cap, need = max_bytes(H, W, 3, C.byref(p)), ws_bytes(H, W, 3, C.byref(p))
    nblocks = 3 * 5 * 7
    assert cap == 623 + 2 * ((nblocks * (20 + 63 * 26) + 7) // 8) + 2 and need > nblocks * 128 + 4 * 257 * 4
    p420, pl = P(75, 2, 2, 0), P(75, 1, 1, 0)
    assert max_bytes(H, W, 3, C.byref(p420)) == lib.st_jpeg_max_bytes(H, W, 3) and max_bytes(33, 41, 1, C.byref(pl)) == lib.st_jpeg_max_bytes(33, 41, 1)
    assert max_bytes(H, W, 3, C.byref(P(95, 2, 1))) == 623 + 2 * ((4 * 4 * 5 * (20 + 63 * 26) + 7) // 8) + 2

    def call(src=src, H=H, W=W, ch=3, stride=None, prm=p, out=out, cap=cap, nb=nb, ws=ws, need=need):
        return enc(src, H, W, ch, W * ch if stride is None else stride, C.byref(prm) if prm is not None else None, out, cap, nb, ws, need, None)
    big = dict(cap=1 << 40, need=1 << 40)
    # what the old entry rejects
    assert call(src=None) == 1001 and call(out=None) == 1001 and call(nb=None) == 1001 and call(ws=None) == 1001
    assert call(ch=2) == 1001 and call(ch=0) == 1001 and call(ch=4) == 1001
    assert call(H=0) == 1001 and call(W=0) == 1001 and call(W=65536, **big) == 1001 and call(H=65536, **big) == 1001
    assert call(H=4096, W=4097, **big) == 1001                                         # H * W above 2^24
    assert max_bytes(4096, 4097, 3, C.byref(p)) == 0 and ws_bytes(65535, 257, 1, C.byref(pl)) == 0 and ws_bytes(65535, 256, 1, C.byref(pl)) > 0
    assert call(cap=cap - 1) == 1001 and call(need=need - 1) == 1001 and call(ws=ws + 4) == 1001 and call(stride=W * 3 - 1) == 1001
    # what the options add
    assert call(prm=None) == 1001 and max_bytes(H, W, 3, None) == 0 and ws_bytes(H, W, 3, None) == 0
    for bad in (P(quality=0), P(quality=101), P(quality=-5), P(hs=1, vs=2), P(hs=2, vs=3), P(hs=4, vs=1), P(hs=0, vs=0), P(hs=3, vs=1), P(optimize=2),
                P(optimize=-1), P(reserved=(0, 0, 1, 0))):
        assert call(prm=bad, **big) == 1001 and max_bytes(H, W, 3, C.byref(bad)) == 0 and ws_bytes(H, W, 3, C.byref(bad)) == 0
    for bad in (P(hs=2, vs=1), P(hs=2, vs=2)):                                         # one channel: 1 x 1 only
        assert call(ch=1, prm=bad, **big) == 1001 and max_bytes(H, W, 1, C.byref(bad)) == 0
        assert max_bytes(H, W, 3, C.byref(bad)) > 0


def test_python_entry_rejects_what_pillow_would_not_write_the_same():
    from stitch_amd import ops
    import torch
    grey, rgb = torch.zeros((8, 8), dtype=torch.uint8), torch.zeros((8, 8, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.jpeg_encode(grey, subsampling=0)                        # Pillow writes 0x21 / 0x22 into an L file's SOF0 there: out of scope
    for kw in (dict(quality=0), dict(quality=101), dict(quality=75.0), dict(subsampling=3), dict(subsampling="4:2:0")):
        with pytest.raises(ValueError):
            ops.jpeg_encode(rgb, **kw)
    assert ops.jpeg_workspace_bytes(37, 53, 3, quality=95, subsampling=0, optimize=True) > ops.jpeg_workspace_bytes(37, 53, 3)


def test_saver_never_passes_subsampling_for_an_l_array():
    spec_ = importlib.util.spec_from_file_location("stitch_out_harness_jo", os.path.join(ROOT, "out.py"))
    outmod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(outmod)
    s = outmod._Saver(jpeg_params=dict(quality=95, subsampling=0, optimize=True))
    assert s._keywords(2) == dict(quality=95, optimize=True) and s._keywords(3) == dict(quality=95, subsampling=0, optimize=True)
    assert outmod._Saver()._keywords(3) == {}
    with pytest.raises(ValueError):
        outmod._Saver(jpeg_params=dict(qtables="web_low"))
    with tempfile.TemporaryDirectory() as td:
        u8 = opts.golden_inputs()
        s.array(u8["l_15x17"], os.path.join(td, "l.jpg"))
        s.array(u8["rgb_15x17"], os.path.join(td, "rgb.jpg"))
        s.wait()
        assert open(os.path.join(td, "l.jpg"), "rb").read() == opts.encode(u8["l_15x17"], quality=95, optimize=True)
        assert open(os.path.join(td, "rgb.jpg"), "rb").read() == opts.encode(u8["rgb_15x17"], quality=95, subsampling=0, optimize=True)


def test_unset_flags_leave_the_config_as_it_was():
    spec_ = importlib.util.spec_from_file_location("stitch_out_harness_jc", os.path.join(ROOT, "out.py"))
    outmod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(outmod)
    cfg = outmod.get_config([])
    assert not any(hasattr(cfg, k) or k in cfg for k in ("jpeg_quality", "jpeg_subsampling", "jpeg_optimize")) and outmod.jpeg_params_of(cfg) is None
    cfg = outmod.get_config(["--jpeg_quality", "95", "--jpeg_subsampling", "0", "--jpeg_optimize"])
    assert outmod.jpeg_params_of(cfg) == dict(quality=95, subsampling=0, optimize=True)
    assert outmod.jpeg_params_of(outmod.get_config(["--jpeg_subsampling", "1"])) == dict(subsampling=1)


def _histograms():
    """1 000 seeded histograms: one symbol, all equal, Fibonacci (deeper than 16 bits), sparse, dense, and counts with many ties"""
    rng = np.random.RandomState(2024)
    hs = []
    for k in range(1000):
        h = np.zeros(256, np.int64)
        kind = k % 8
        if kind == 0:
            h[rng.randint(256)] = rng.randint(1, 1 << 20)
        elif kind == 1:
            h[rng.choice(256, rng.randint(2, 257), replace=False)] = rng.randint(1, 1000)
        elif kind == 2:
            n = rng.randint(18, 31)
            fib = [1, 2]
            while len(fib) < n:
                fib.append(fib[-1] + fib[-2])
            h[rng.choice(256, n, replace=False)] = rng.permutation(fib)
        elif kind == 3:
            n = rng.randint(2, 30)
            h[rng.choice(256, n, replace=False)] = rng.randint(1, 100000, n)
        elif kind == 4:
            h[:] = rng.randint(0, 4, 256)                           # ties everywhere
        elif kind == 5:
            h[:] = (rng.pareto(0.7, 256) * 10).astype(np.int64) % (1 << 22)
        elif kind == 6:
            h[:] = rng.randint(1, 1 << 22, 256)
        else:
            n = rng.randint(100, 257)
            h[rng.choice(256, n, replace=False)] = np.maximum(1, (2.0 ** rng.uniform(0, 21, n)).astype(np.int64))
        if not h.any():
            h[0] = 1
        hs.append(h)
    return hs


@pytest.mark.skipif(shutil.which("c++") is None and shutil.which("g++") is None and shutil.which("clang++") is None, reason="needs a host C++ compiler")
def test_table_builder_under_sanitizers_equals_the_restatement(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    exe = str(tmp_path / "jpeg_huff_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tools", "jpeg_huff_host_check.cpp"), "-o", exe])
    hs = _histograms()
    cases, outp = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(cases, "wb") as f:
        f.write(struct.pack("<I", len(hs)))
        for h in hs:
            f.write(h.astype("<u4").tobytes())
    r = subprocess.run([exe, cases, outp], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(outp, "rb").read()
    rec = 16 + 4 + 256 + 1024
    assert len(raw) == rec * len(hs)
    deep = 0
    for k, h in enumerate(hs):
        bits, vals, depth = opts.gen_optimal_table(h)
        deep += depth > 16
        at = k * rec
        got_bits = list(raw[at:at + 16])
        nsym, = struct.unpack_from("<I", raw, at + 16)
        got_vals = list(raw[at + 20:at + 20 + nsym])
        assert not any(bits[16:]) and got_bits == list(bits[:16]) and got_vals == vals, k
        assert sum(n << (16 - l - 1) for l, n in enumerate(got_bits)) < 65536           # Kraft: the all-ones code stays free
        codes = np.frombuffer(raw, "<u4", 256, at + 276)
        want = opts.huff_codes(bits[:16], vals)
        assert {s: (int(c) & 0xffff, int(c) >> 16) for s, c in enumerate(codes) if c} == want, k
    assert deep >= 50                                               # the length limit was at work
