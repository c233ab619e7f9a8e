"""The restart-interval contract, decided on the CPU: tests/_jpeg_rst_ref.py writes Pillow's files byte for byte and decodes them to Pillow's
pixels (tests/golden/jpeg_rst_pil.npz and live Pillow), the goldens exercise every rule (a planted defect changes one), `jpeg_probe` takes a
DRI file only with `restart=True` and only with all its markers in order, the entry and the size query reject bad arguments before any
launch, the restart kernels (jpegr_* in csrc/jpeg.hip and csrc/jpeg_dec.hip) use no scratch and the LDS the README states, and their interval logic (csrc/jpeg_rst_core.h) runs
clean under the host compiler's address and undefined-behaviour sanitizers on golden, cut, damaged and random streams."""
import importlib.util
import io
import os
import re
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import _jpeg_dec_cases as cases
import _jpeg_dec_ref as dref
import _jpeg_ref as eref
import _jpeg_rst_ref as rst

ROOT = cases.ROOT
PKG = os.path.join(ROOT, "seamless-through-breaking-rethinking-image-stitching-for-optimal-alignment_amd")


@pytest.fixture(scope="module")
def golden():
    return rst.load_golden()


def _pillow_file(u8, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(u8).save(buf, format="JPEG", **kw)
    return buf.getvalue()


# ---- parity -----------------------------------------------------------------------------------------------------------------------
def test_goldens_cover_the_stated_cases(golden):
    for h, w in rst.SIZES:
        for kind, sub in rst.KINDS:
            name = rst.case_name(f"{'l' if kind == 'l' else 'rgb'}_{h}x{w}", subsampling=sub, blocks=1)
            info = rst.probe(golden[name][2])
            assert (info["H"], info["W"], info["restart_interval"]) == (h, w, 1)
            assert (info["ncomp"], info["hs"], info["vs"]) == dict(l=(1, 1, 1), **{"444": (3, 1, 1), "422": (3, 2, 1), "420": (3, 2, 2)})[kind]
    one = golden[rst.case_name("rgb_1x1", subsampling=2, blocks=1)][2]
    assert one.count(b"\xff\xdd\x00\x04\x00\x01") == 1 and not any(bytes([0xFF, 0xD0 + k]) in one for k in range(8))      # one MCU: a DRI segment, no marker
    markers = {name: len(rst.intervals(d, rst.probe(d))) - 1 for name, (_, _, d, _) in golden.items()}
    assert max(markers.values()) >= 10                                        # the marker number wraps past D7
    for name, (u8, kw, data, _) in golden.items():
        info = rst.probe(data)
        mr, mc, _, _ = dref.geometry(info)
        assert info["restart_interval"] == rst.restart_interval(info["H"], info["W"], info["hs"], info["vs"], kw.get("restart_marker_blocks"), kw.get("restart_marker_rows"))
        assert markers[name] == -(-(mr * mc) // info["restart_interval"]) - 1, name
        sos = info["scan_off"] - (8 + 2 * info["ncomp"])                      # the DRI segment sits directly in front of SOS
        assert data[sos:sos + 2] == b"\xff\xda" and data[sos - 6:sos] == b"\xff\xdd\x00\x04" + info["restart_interval"].to_bytes(2, "big"), name
    std = golden[rst.case_name("rgb_40x52", subsampling=2, rows=1)][2]
    assert std.index(b"\xff\xdd") == 609 and std.index(b"\xff\xda") == 615        # a default RGB file: DRI behind the DHTs, directly in front of SOS
    assert rst.probe(golden[rst.CLAMP_CASE][2])["restart_interval"] == 65535 and markers[rst.CLAMP_CASE] == 0
    assert markers[rst.case_name("rgb_17x23", subsampling=2, blocks=1000)] == 0 and markers[rst.case_name("rgb_17x23", subsampling=2, blocks=4)] == 0
    assert rst.probe(golden[rst.case_name("rgb_40x52", subsampling=2, blocks=3, rows=1)][2])["restart_interval"] == 4          # rows win over blocks
    assert any(b"\xff\x00\xff\xd0" in d or b"\xff\x00\xff\xd1" in d for _, _, d, _ in golden.values())
    assert sum(kw["optimize"] for _, kw, _, _ in golden.values()) >= 3 and {30, 95} <= {kw["quality"] for _, kw, _, _ in golden.values()}


def test_restatement_writes_the_golden_files(golden):
    for name, (u8, kw, data, _) in golden.items():
        assert rst.encode(u8, **kw) == data, name


def test_restatement_decodes_the_golden_pixels(golden):
    for name, (u8, kw, data, px) in golden.items():
        if name == rst.CLAMP_CASE:
            continue                                                          # (8188 blocks: decoded by the host program below and on the GPU)
        got = rst.decode(data)
        assert got.dtype == np.uint8 and got.shape == px.shape and np.array_equal(got, px), name
        coef, status, pads = rst.coefficients(data)
        assert status == 0 and all(0 <= p < 8 for p in pads), name


def test_restatement_equals_live_pillow():
    if not cases.pillow_turbo():
        pytest.skip("this Pillow is not built on libjpeg-turbo: the contract restates libjpeg-turbo's arithmetic (the golden comparison still runs)")
    rng = np.random.RandomState(77)
    for k in range(12):
        h, w = int(rng.randint(1, 60)), int(rng.randint(1, 60))
        u8 = eref._smooth(h, w, 3 if k % 3 else 0, 1000 + k) if k % 2 else rng.randint(0, 256, (h, w, 3) if k % 3 else (h, w)).astype(np.uint8)
        kw = dict(quality=int(rng.choice([30, 75, 95])), optimize=bool(k % 4 == 0))
        if u8.ndim == 3:
            kw["subsampling"] = int(rng.randint(0, 3))
        if k % 3 == 2:
            kw["restart_marker_rows"] = int(rng.randint(1, 3))
        else:
            kw["restart_marker_blocks"] = int(rng.randint(1, 12))
        data = _pillow_file(u8, **kw)
        assert rst.encode(u8, **kw) == data, (k, kw)
        assert np.array_equal(rst.decode(data), cases.pillow_pixels(data)), (k, kw)


@pytest.mark.parametrize("defect", rst.DEFECTS)
def test_a_planted_defect_changes_a_golden(golden, defect):
    def differs(u8, kw, data):
        try:
            return rst.encode(u8, defect=defect, **kw) != data
        except KeyError:                                                      # hist_no_reset: the scan needs a symbol the wrong histogram never counted
            return True
    changed = [name for name, (u8, kw, data, _) in golden.items() if differs(u8, kw, data)]
    assert changed, defect


# ---- probe ------------------------------------------------------------------------------------------------------------------------
def test_probe_takes_restart_files_only_when_asked(golden):
    from stitch_amd import ops
    for name, (_, _, data, _) in golden.items():
        assert ops.jpeg_probe(data) is None, name
        info = ops.jpeg_probe(data, restart=True)
        assert info is not None and info.restart_interval == rst.probe(data)["restart_interval"] > 0 and info[-1] == info.restart_interval, name
        assert data[info.scan_off + info.scan_len:] == b"\xff\xd9"
    plain = cases.load_golden()["420_17x23_q75"]
    assert ops.jpeg_probe(plain[0], restart=True) == ops.jpeg_probe(plain[0]) and ops.jpeg_probe(plain[0]).restart_interval == 0
    at = plain[0].index(b"\xff\xc0")
    dri4 = plain[0][:at] + b"\xff\xdd\x00\x04\x00\x04" + plain[0][at:]          # four MCUs, Ri = 4: a valid one-interval file
    assert ops.jpeg_probe(dri4) is None
    info = ops.jpeg_probe(dri4, restart=True)
    assert info.restart_interval == 4 and np.array_equal(rst.decode(dri4), plain[1])


def test_probe_refuses_wrong_markers(golden):
    from stitch_amd import ops
    data = golden[rst.case_name("rgb_40x52", subsampling=2, blocks=1)][2]      # 3 x 4 MCUs: 11 markers, D0 .. D7, D0, D1, D2
    info = rst.probe(data)
    parts = rst.intervals(data, info)
    assert len(parts) == 12
    m3, m9 = parts[3][0] - 2, parts[9][0] - 2
    assert data[m3:m3 + 2] == b"\xff\xd2" and data[m9:m9 + 2] == b"\xff\xd0"
    dri = data.index(b"\xff\xdd")
    refused = {"missing": data[:m3] + data[m3 + 2:],
               "one_too_many": data[:-2] + b"\xff\xd3" + data[-2:],
               "out_of_order": data[:m3 + 1] + b"\xd3" + data[m3 + 2:],
               "not_wrapped": data[:m9 + 1] + b"\xd7" + data[m9 + 2:],
               "without_dri": data[:dri] + data[dri + 6:],
               "other_marker": data[:m3 + 1] + b"\xc4" + data[m3 + 2:]}
    for name, d in refused.items():
        assert ops.jpeg_probe(d, restart=True) is None and ops.jpeg_probe(d) is None, name
    assert ops.jpeg_probe(data, restart=True) is not None


# ---- guards -----------------------------------------------------------------------------------------------------------------------
def test_entry_and_size_query_reject_bad_arguments_without_touching_the_gpu(golden):
    import ctypes as C
    from stitch_amd import ops
    from stitch_amd._lib import JpegDecParams, JpegEncParams, lib
    assert lib.st_abi_jpeg_dec_params_size() == C.sizeof(JpegDecParams) == 24 * 4 and C.sizeof(JpegEncParams) == lib.st_abi_jpeg_enc_params_size() == 32
    data = golden[rst.case_name("rgb_64x48", subsampling=2, blocks=1)][2]
    info = ops.jpeg_probe(data, restart=True)
    need = ops.jpeg_dec_workspace_bytes(info)
    plain = lib.st_jpeg_dec_workspace_bytes(info.H, info.W, info.ncomp, info.hs, info.vs, info.scan_len)
    assert need % 16 == 0 and need > plain > 0
    base = 0x7f0000000000                                                     # never dereferenced on the host

    def params(**kw):
        prm = ops._jpeg_dec_params(info)
        for k, v in kw.items():
            setattr(prm, k, v)
        return prm

    def entry(need_=need, **kw):
        """only ever called with arguments the entry must reject: with valid ones it would launch on these pointers"""
        return lib.st_jpeg_decode_u8(base, len(data), C.byref(params(**kw)), base + (1 << 30), info.W * 3, base + (2 << 30), base + (3 << 30), need_, None)

    def size(**kw):
        return lib.st_jpeg_dec_workspace_bytes_ex(C.byref(params(**kw)))
    for kw in (dict(restart_interval=-1), dict(restart_interval=65536), dict(reserved=1), dict(reserved=-1), dict(H=0), dict(ncomp=2), dict(hs=1, vs=2), dict(scan_len=0)):
        assert (entry(**kw), size(**kw)) == (1001, 0), kw
    assert entry(need_=need - 1) == 1001 and entry(need_=plain) == 1001         # the plain size is too small for a restart file
    assert size() == need and size(restart_interval=0) == plain and size(restart_interval=65535) > plain
    assert lib.st_jpeg_dec_workspace_bytes_ex(None) == 0
    # the 13 positional values of the callers before the two new fields: no restart interval
    old = JpegDecParams(info.H, info.W, info.ncomp, info.hs, info.vs, (C.c_int32 * 3)(*info.tq), (C.c_int32 * 3)(*info.td), (C.c_int32 * 3)(*info.ta),
                        (C.c_int32 * 2)(*info.q_off), (C.c_int32 * 2)(*info.dc_off), (C.c_int32 * 2)(*info.ac_off), info.scan_off, info.scan_len)
    assert (old.restart_interval, old.reserved) == (0, 0) and lib.st_jpeg_dec_workspace_bytes_ex(C.byref(old)) == plain


def test_encoder_guards_and_sizes_without_a_gpu():
    import ctypes as C
    from stitch_amd import ops
    from stitch_amd._lib import JpegEncParams, lib
    assert C.sizeof(JpegEncParams) == lib.st_abi_jpeg_enc_params_size() == 32 and len(JpegEncParams._fields_) == 5
    base = 0x7f0000000000                                                     # never dereferenced on the host

    def prm(ri=0, r1=0, r2=0, r3=0):
        return JpegEncParams(75, 2, 2, 0, (C.c_int32 * 4)(ri, r1, r2, r3))

    def entry(p, cap, need):
        """only ever called with arguments the entry must reject"""
        return lib.st_jpeg_encode_u8_ex(base, 64, 48, 3, 48 * 3, C.byref(p), base + (1 << 30), cap, base + (2 << 30), base + (3 << 30), need, None)
    size = lambda p: (lib.st_jpeg_max_bytes_ex(64, 48, 3, C.byref(p)), lib.st_jpeg_workspace_bytes_ex(64, 48, 3, C.byref(p)))
    cap0, need0 = size(prm())
    assert (cap0, need0) == (lib.st_jpeg_max_bytes(64, 48, 3), lib.st_jpeg_workspace_bytes(64, 48, 3))
    for bad in (prm(-1), prm(65536), prm(4, 1), prm(4, 0, 1), prm(0, 0, 0, 1)):
        assert size(bad) == (0, 0) and entry(bad, cap0 + 4096, need0 + 4096) == 1001
    # 12 MCUs: the DRI segment, and per interval the marker and one padded byte doubled for stuffing
    for ri, nint in ((1, 12), (5, 3), (12, 1), (65535, 1)):
        cap, need = size(prm(ri))
        assert cap == cap0 + 6 + 4 * nint and need >= need0 + 2 * 4 * (nint + 1) and need % 16 == 0, (ri, cap, need)
        assert entry(prm(ri), cap - 1, need) == 1001 and entry(prm(ri), cap, need - 1) == 1001 and entry(prm(ri), cap0, need) == 1001
    assert ops.jpeg_workspace_bytes(48, 64, 3, restart_marker_rows=1) == lib.st_jpeg_workspace_bytes_ex(48, 64, 3, C.byref(prm(4)))
    assert ops.jpeg_workspace_bytes(48, 64, 3, restart_marker_rows=2, restart_marker_blocks=3) == lib.st_jpeg_workspace_bytes_ex(48, 64, 3, C.byref(prm(8)))
    assert ops.jpeg_workspace_bytes(48, 64, 3, restart_marker_blocks=0) == lib.st_jpeg_workspace_bytes(48, 64, 3)
    assert ops._jpeg_enc_params(1, None, None, False, 65500, None, 9).reserved[0] == 65535          # the clamp
    for bad in (dict(restart_marker_blocks=-1), dict(restart_marker_blocks=65536), dict(restart_marker_rows=-2), dict(restart_marker_rows=True)):
        with pytest.raises(ValueError):
            ops.jpeg_workspace_bytes(48, 64, 3, **bad)


# ---- compiler metadata ------------------------------------------------------------------------------------------------------------
LDS_TABLES = 4 * (17 * 4 + 17 * 4 + 256) + 4 * 272     # JdTables: four tables of lim[17], valoff[17], vals[256]; the four raw DHT payloads
LDS_STREAM = (256 * 1024 // 32 + 4) * 4                # a workgroup's part of the unstuffed stream
ENC_TABLES = (2 * 16 + 2 * 256) * 4                    # HuffLds: code | length << 16 of the DC categories and the AC symbols of both tables
WGRED = 256                                            # the device library's scratch for __syncthreads_or


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_kernels_use_no_scratch_and_the_stated_lds():
    spec = importlib.util.spec_from_file_location("_stitch_build_jr", os.path.join(PKG, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    text = ""
    with tempfile.TemporaryDirectory() as td:
        for src in ("jpeg.hip", "jpeg_dec.hip"):                              # the encoder's and the decoder's restart kernels
            out = os.path.join(td, src.replace(".hip", ".s"))
            subprocess.check_call(build.compile_cmd(src, out, ["-S", "--cuda-device-only"]), stderr=subprocess.DEVNULL)
            text += open(out).read()
    rep = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+)\n.*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)",
                         text, re.S):
        if "jpegr_" in m.group(2):                                            # (the plain kernels' rows: tests/test_jpeg_cpu.py, tests/test_jpeg_dec_cpu.py)
            rep[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    lds = {"jpegr_count_kernel": 32, "jpegr_unstuff_kernel": 32, "jpegr_cut_kernel": 0, "jpegr_enc_hist_kernel": 4 * 257 * 4, "jpegr_enc_bits_kernel": ENC_TABLES,
           "jpegr_enc_pad_kernel": 0, "jpegr_enc_offsets_kernel": 0, "jpegr_enc_pack_kernel": ENC_TABLES, "jpegr_enc_stuff_kernel": 16, "jpegr_sync_kernel": LDS_TABLES + LDS_STREAM + 2048 + 8 + WGRED,       # (+ the base word, padded to 8)
           "jpegr_write_kernel": LDS_TABLES + LDS_STREAM + 4, "jpegr_dc_kernel": 132}
    vgpr = {"jpegr_count_kernel": 12, "jpegr_unstuff_kernel": 24, "jpegr_cut_kernel": 6, "jpegr_sync_kernel": 42, "jpegr_write_kernel": 28, "jpegr_dc_kernel": 36,
            "jpegr_enc_hist_kernel": 16, "jpegr_enc_bits_kernel": 18, "jpegr_enc_pad_kernel": 9, "jpegr_enc_offsets_kernel": 9, "jpegr_enc_pack_kernel": 28,
            "jpegr_enc_stuff_kernel": 31}                                                     # the README's column
    assert len(rep) == len(lds) == len(vgpr), sorted(rep)
    for key, want in lds.items():
        (name, r), = [(n, r) for n, r in rep.items() if key in n]
        assert r["scratch"] == 0 and r["spill"] == 0 and r["lds"] == want and r["vgpr"] == vgpr[key], (name, r)
    assert not re.search(r"^\s*scratch_(load|store)", text, re.M)                           # no stack traffic at all


# ---- the interval logic under the host sanitizers ---------------------------------------------------------------------------------
def _case(data, info, nblocks=None, ri=None):
    _, _, nb, n = dref.geometry(info)
    head = struct.pack("<I16i", len(data), nblocks or n, nb, nb - 2 if info["ncomp"] == 3 else 1, *info["td"], *info["ta"], *info["dc_off"], *info["ac_off"],
                       info["scan_off"], info["scan_len"], ri or info["restart_interval"])
    return head + data


@pytest.mark.skipif(shutil.which("c++") is None and shutil.which("g++") is None and shutil.which("clang++") is None, reason="needs a host C++ compiler")
def test_interval_logic_is_clean_under_host_sanitizers(golden, tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    exe = str(tmp_path / "jpeg_rst_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tools", "jpeg_rst_host_check.cpp"), "-o", exe])
    blobs, expect = [], []
    for name, (_, _, data, _) in golden.items():                              # whole files, then files with one interval's bytes halved
        info = rst.probe(data)
        blobs.append(_case(data, info))
        expect.append((name, data, info))
    for name, (_, _, data, _) in golden.items():
        info = rst.probe(data)
        nint = len(rst.intervals(data, info))
        if nint >= 3:
            short = rst.damaged(data, info, nint // 2)
            i2 = dict(info, scan_len=info["scan_len"] - (len(data) - len(short)))
            blobs.append(_case(short, i2))
            expect.append((name + " damaged", short, i2))
            off, n = rst.intervals(data, info)[1]                             # an interval's bytes removed, its markers stay: FF Dn FF Dn+1
            gone = data[:off] + data[off + n:]
            i3 = dict(info, scan_len=info["scan_len"] - n)
            blobs.append(_case(gone, i3))
            expect.append((name + " removed", gone, i3))
    n_checked = len(blobs)
    for name, (_, _, data, _) in golden.items():                              # cut files: the stream ends inside an interval, a block, a symbol
        info = rst.probe(data)
        for kw in (dict(fraction=0.25), dict(fraction=0.5), dict(drop=1)):
            short = cases.cut(data, info, **kw)
            i2 = dict(info, scan_len=len(short) - info["scan_off"])
            if i2["scan_len"] >= 1:
                blobs.append(_case(short, i2))
    base = golden[rst.case_name("rgb_64x48", subsampling=2, blocks=1)][2]
    binfo = rst.probe(base)
    rng = np.random.RandomState(12)
    for k in range(200):                                                     # random bytes, a third of them rich in FF, 00 and marker bytes
        n = int(rng.randint(1, 700))
        noise = rng.randint(0, 256, n).astype(np.uint8).tobytes()
        if k % 3 == 0:
            noise = bytes(rng.choice([0xFF, 0x00, 0xD0, 0xD3, 0xD7, 0x7F], n).astype(np.uint8))
        ri = int(rng.choice([1, 2, 5, 12, 65535]))
        if k % 2 == 0:
            blobs.append(_case(base[:binfo["scan_off"]] + noise, dict(binfo, scan_len=n), 72, ri))
        else:
            offs = [int(v) for v in rng.randint(0, n, 5)]
            info = dict(ncomp=3, hs=2, vs=2, H=16, W=16, td=[0, 1, 1], ta=[0, 1, 1], dc_off=offs[0:2], ac_off=offs[2:4], scan_off=offs[4], scan_len=n - offs[4])
            blobs.append(_case(noise, info, 30, ri))
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(blobs)) + b"".join(blobs))
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    out = open(dst, "rb").read()
    at = 0
    for name, data, info in expect[:n_checked]:
        nblocks = dref.geometry(info)[3]
        got_status, = struct.unpack_from("<I", out, at)
        got = np.frombuffer(out, np.int16, nblocks * 64, at + 4).reshape(nblocks, 64)
        at += 4 + 2 * nblocks * 64
        if name == rst.CLAMP_CASE:
            assert got_status == 0 and got[0, 0] == 0 and not got[:, 1:].any() and not got[:, 0].any()            # flat 128: every coefficient 0
            continue
        coef, status, _ = rst.coefficients(data, info)
        assert got_status == status and np.array_equal(got, coef), name
        assert (status != 0) == (" " in name), name
