"""The JPEG decode contract, decided on the CPU: tests/_jpeg_dec_ref.py (what csrc/jpeg_dec.hip implements) equals Pillow's pixels bit for
bit, the golden files exercise every rule of the contract (a planted defect changes a golden's pixels), `probe` refuses what the decoder
does not take, the parallel entropy-decode scheme reaches the sequential decoder's states, the entry rejects bad arguments before any
launch, the kernels use no scratch and the LDS the README states, and the kernels' symbol decoder (csrc/jpeg_dec_core.h) runs clean under
the host compiler's address and undefined-behaviour sanitizers on golden, cut and random streams."""
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
import _jpeg_dec_ref as ref
import _jpeg_ref as eref

ROOT = cases.ROOT
PKG = os.path.join(ROOT, "seamless-through-breaking-rethinking-image-stitching-for-optimal-alignment_amd")


@pytest.fixture(scope="module")
def golden():
    return cases.load_golden()


def test_goldens_cover_the_stated_files(golden):
    for h, w in [(1, 1), (2, 3), (4, 5), (5, 4), (8, 8), (16, 16), (17, 23), (33, 15), (40, 9), (9, 40), (64, 48)]:
        for kind in ("l", "444", "422", "420"):
            data, px, _ = golden[f"{kind}_{h}x{w}_q75"]
            info = ref.probe(data)
            assert (info["H"], info["W"]) == (h, w) and px.shape == ((h, w) if kind == "l" else (h, w, 3))
            assert (info["ncomp"], info["hs"], info["vs"]) == dict(l=(1, 1, 1), **{"444": (3, 1, 1), "422": (3, 2, 1), "420": (3, 2, 2)})[kind]
    assert sum(k.startswith("420_") and k.endswith("_q30") for k in golden) >= 3 and sum(k.startswith("420_") and k.endswith("_q95") for k in golden) >= 3
    assert sum(k.startswith("enc_") for k in golden) == 18
    std = eref.header(40, 56, 3)
    opt = golden["optimize_40x56"][0]
    assert opt.count(b"\xff\xc4") >= 1 and opt[:ref.probe(opt)["scan_off"]].count(bytes(eref.AC_LUMA[1][:32])) == 0 and std.count(bytes(eref.AC_LUMA[1][:32])) == 1
    seg = golden["com_app1_24x40"][0]
    assert b"\xff\xfe" in seg[:200] and b"\xff\xe1" in seg[:200]
    assert any(d[ref.probe(d)["scan_off"]:].count(b"\xff\x00") for d, _, _ in golden.values())           # byte stuffing is exercised


def test_restatement_equals_the_golden_pixels(golden):
    for name, (data, px, sha) in golden.items():
        got = ref.decode(data)
        assert got.dtype == np.uint8 and cases.same_pixels(got, px, sha), name
        if sha is not None:                                                   # the stored crop of a digested case
            crop = np.load(cases.GOLDEN)["px_enc_" + name[4:]]
            assert np.array_equal(got[:, -crop.shape[1]:], crop), name


def test_restatement_equals_live_pillow(golden):
    if not cases.pillow_turbo():
        pytest.skip("this Pillow is not built on libjpeg-turbo: the contract restates libjpeg-turbo's arithmetic (the golden comparison still runs)")
    for name, (data, _, _) in golden.items():
        assert np.array_equal(ref.decode(data), cases.pillow_pixels(data)), name
    from PIL import Image
    for k, (u8, kw) in enumerate([(eref._smooth(37, 53, 3, 900), dict(quality=85, subsampling=1)), (eref.pattern(48, 70, 3), dict(quality=60, optimize=True)),
                                  (eref._smooth(21, 3, 3, 901), dict(quality=90)), (eref._smooth(3, 4, 3, 902), dict(subsampling=1))]):
        buf = io.BytesIO()
        Image.fromarray(u8).save(buf, format="JPEG", **kw)
        assert np.array_equal(ref.decode(buf.getvalue()), cases.pillow_pixels(buf.getvalue())), k


@pytest.mark.parametrize("defect", ref.DEFECTS)
def test_a_planted_defect_changes_a_golden(golden, defect):
    small = {k: v for k, v in golden.items() if v[2] is None}
    changed = [name for name, (data, px, _) in small.items() if not np.array_equal(ref.decode(data, defect=defect), px)]
    assert changed, defect


def _patched(data, marker, payload):
    """`data` with one more segment in front of its SOF0"""
    at = data.index(b"\xff\xc0")
    return data[:at] + bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload + data[at:]


def test_probe_refuses_what_the_decoder_does_not_take(golden):
    from stitch_amd import ops
    base = golden["420_17x23_q75"][0]
    sof = base.index(b"\xff\xc0")
    refused = {"dri": _patched(base, 0xDD, b"\x00\x04"),
               "precision12": base[:sof + 4] + b"\x0c" + base[sof + 5:],
               "440": base[:sof + 11] + b"\x12" + base[sof + 12:],
               "rst_in_scan": base[:-2] + b"\xff\xd0" + base[-2:],
               "adobe_rgb": _patched(base.replace(b"JFIF\x00", b"JFXX\x00"), 0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x00"),
               "no_soi": base[2:], "empty": b""}
    eoi = len(base) - 2
    sos = base.index(b"\xff\xda")
    refused["two_scans"] = base[:eoi] + base[sos:]                           # a second SOS behind the first scan
    nc4 = bytearray(base[:sof] + b"\xff\xc0" + struct.pack(">H", 8 + 12) + base[sof + 4:sof + 9] + b"\x04" + base[sof + 10:sof + 19] + b"\x04\x11\x01" + base[sof + 19:])
    refused["four_components"] = bytes(nc4)
    try:
        from PIL import Image
        buf = io.BytesIO()
        Image.fromarray(eref._smooth(24, 24, 3, 1)).save(buf, format="JPEG", progressive=True)
        refused["progressive"] = buf.getvalue()
    except ImportError:
        refused["progressive"] = base[:sof] + b"\xff\xc2" + base[sof + 2:]
    assert ops.jpeg_probe(_patched(base, 0xDD, b"\x00\x00")) is not None          # DRI 0 is no restart interval
    for name, data in refused.items():
        assert ops.jpeg_probe(data) is None, name
    assert ref.probe(refused["progressive"]) is None                          # the restatement uses the same parser


def test_probe_fields_of_every_golden(golden):
    from stitch_amd import ops
    for name, (data, px, _) in golden.items():
        b = ops.jpeg_probe(data)
        assert b is not None, name
        a = b._asdict()                                                       # (there is one parser: checked against the file's bytes)
        assert b.nbytes == len(data) and data[a["scan_off"] + a["scan_len"]:] == b"\xff\xd9"
        assert b"\xff" not in data[a["scan_off"]:a["scan_off"] + a["scan_len"]].replace(b"\xff\x00", b"")
        sof = data.index(b"\xff\xc0")
        assert (a["H"], a["W"], a["ncomp"]) == (int.from_bytes(data[sof + 5:sof + 7], "big"), int.from_bytes(data[sof + 7:sof + 9], "big"), data[sof + 9])
        assert (a["hs"], a["vs"]) == (data[sof + 11] >> 4, data[sof + 11] & 15)
        assert data[a["scan_off"] - 3:a["scan_off"]] == b"\x00\x3f\x00"
        if px is not None:
            assert (a["H"], a["W"]) == px.shape[:2] and a["ncomp"] == (3 if px.ndim == 3 else 1)
        for c in range(a["ncomp"]):
            assert data[a["q_off"][a["tq"][c]] - 5:a["q_off"][a["tq"][c]] - 3] == b"\xff\xdb"
            assert sum(data[a["dc_off"][a["td"][c]]:a["dc_off"][a["td"][c]] + 16]) <= 12
            for off, cls in ((a["dc_off"][a["td"][c]], 0), (a["ac_off"][a["ta"][c]], 1)):
                assert data[off - 1] == (cls << 4 | (a["ta"][c] if cls else a["td"][c]))                 # the Tc | Th byte in front of the counts
            assert data[a["q_off"][a["tq"][c]] - 1] == a["tq"][c]


def test_fixpoint_model_reaches_the_sequential_states(golden):
    for name, (data, _, _) in golden.items():
        if name.startswith("enc_big_"):
            continue
        for S in (64, 1024):
            m = ref.sync_model(data, S)
            states, _, _ = ref.sequential_states(m["stream"], S)
            assert m["states"] == states, (name, S)
            assert m["rounds"] <= max(0, len(states) - 1)
    for name in ("enc_big_rgb_130x1030", "enc_big_l_24x2056"):
        m = ref.sync_model(golden[name][0], cases.SUB_BITS)
        assert m["states"] == ref.sequential_states(m["stream"], cases.SUB_BITS)[0] and len(m["states"]) > 16, name


def test_flat_image_never_synchronises():
    """the property the GPU test's zeros file is chosen for: at the kernel's S fewer than a tenth of the subsequences reach the right state
    from their guessed start, so the fixpoint walks them one by one"""
    data = cases.zeros_file()
    m = ref.sync_model(data, cases.SUB_BITS)
    n = len(m["states"])
    assert m["states"] == ref.sequential_states(m["stream"], cases.SUB_BITS)[0]
    assert n >= 30 and sum(m["synced"]) * 10 < n, (sum(m["synced"]), n)
    assert m["rounds"] >= n * 9 // 10 - 1


def test_entry_rejects_bad_arguments_without_touching_the_gpu(golden):
    from stitch_amd import ops
    from stitch_amd._lib import lib
    data = golden["420_64x48_q75"][0]
    info = ops.jpeg_probe(data)
    need = ops.jpeg_dec_workspace_bytes(info)
    assert need > 0 and need % 16 == 0 and need > 64 * 48 * 3
    base = 0x7f0000000000                                                     # never dereferenced on the host
    call = cases.entry_call(info, base, base + (1 << 30), base + (2 << 30), base + (3 << 30), need)
    cases.guard_cases(call, len(data), need, info.W, info.ncomp)
    ws = lib.st_jpeg_dec_workspace_bytes
    assert ws(4096, 4096, 3, 2, 2, 1000) > 0 and ws(4096, 4097, 3, 2, 2, 1000) == 0 and ws(64, 48, 1, 2, 2, 100) == 0 and ws(64, 48, 3, 2, 2, 0) == 0


def _resource_report():
    spec = importlib.util.spec_from_file_location("_stitch_build_jd", os.path.join(PKG, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "jpeg_dec.s")
        subprocess.check_call(build.compile_cmd("jpeg_dec.hip", out, ["-S", "--cuda-device-only"]), stderr=subprocess.DEVNULL)
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
    lds = {"jpegd_count_kernel": 16, "jpegd_unstuff_kernel": 16, "jpegd_sync_kernel": LDS_TABLES + LDS_STREAM + 2048 + WGRED, "jpegd_zero_kernel": 0, "jpegd_write_kernel": LDS_TABLES + LDS_STREAM, "jpegd_dc_kernel": 68,
           "jpegd_idct_kernel": 768 + 4 * 8 * 72 * 4, "jpegd_pixels_kernel": 0}
    assert len(rep) == len(lds), sorted(rep)
    for key, want in lds.items():
        (name, r), = [(n, r) for n, r in rep.items() if key in n]
        assert r["scratch"] == 0 and r["spill"] == 0 and r["lds"] == want and r["vgpr"] <= 64, (name, r)
    assert not re.search(r"^\s*scratch_(load|store)", text, re.M)                           # no stack traffic at all


LDS_TABLES = 4 * (17 * 4 + 17 * 4 + 256) + 4 * 272     # JdTables: four tables of lim[17], valoff[17], vals[256]; the four raw DHT payloads
LDS_STREAM = (256 * 1024 // 32 + 4) * 4                # a workgroup's part of the unstuffed stream
WGRED = 256                                            # the device library's scratch for __syncthreads_or


# ---- the kernels' symbol decoder under the host sanitizers ------------------------------------------------------------------------
def _case(data, info, nblocks=None):
    _, _, nb, n = ref.geometry(info)
    head = struct.pack("<I15i", len(data), nblocks or n, nb, nb - 2 if info["ncomp"] == 3 else 1, *info["td"], *info["ta"], *info["dc_off"], *info["ac_off"],
                       info["scan_off"], info["scan_len"])
    return head + data


@pytest.mark.skipif(shutil.which("c++") is None and shutil.which("g++") is None and shutil.which("clang++") is None, reason="needs a host C++ compiler")
def test_symbol_decoder_is_clean_under_host_sanitizers(golden, tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    exe = str(tmp_path / "jpeg_dec_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tools", "jpeg_dec_host_check.cpp"), "-o", exe])
    names = [n for n in golden if not n.startswith("enc_big_rgb")]
    blobs, expect = [], []
    for name in names:
        data = golden[name][0]
        info = ref.probe(data)
        blobs.append(_case(data, info))
        expect.append(ref.coefficients(data, info))
    n_checked = len(blobs)
    rng = np.random.RandomState(11)
    for name in names:                                                       # cut files: the stream ends inside a block, or inside a symbol
        data = golden[name][0]
        info = ref.probe(data)
        nblocks = ref.geometry(info)[3]
        for kw in (dict(fraction=0.25), dict(fraction=0.5), dict(drop=1)):
            short = cases.cut(data, info, **kw)
            i2 = dict(info, scan_len=len(short) - info["scan_off"])
            if i2["scan_len"] >= 1:
                blobs.append(_case(short, i2, nblocks))
    base = golden["420_64x48_q75"][0]
    binfo = ref.probe(base)
    for k in range(200):                                                     # random bytes: as the scan behind real tables, and as the whole file
        n = int(rng.randint(1, 700))
        noise = rng.randint(0, 256, n).astype(np.uint8).tobytes()
        if k % 5 == 0:
            noise = bytes(rng.choice([0xFF, 0x00, 0x7F], n).astype(np.uint8))
        if k % 2 == 0:
            data = base[:binfo["scan_off"]] + noise
            blobs.append(_case(data, dict(binfo, scan_len=n), 72))
        else:
            offs = [int(v) for v in rng.randint(0, n, 5)]
            info = dict(ncomp=3, hs=2, vs=2, H=16, W=16, td=[0, 1, 1], ta=[0, 1, 1], dc_off=offs[0:2], ac_off=offs[2:4], scan_off=offs[4], scan_len=n - offs[4])
            blobs.append(_case(noise, info, 30))
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(blobs)) + b"".join(blobs))
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    out = open(dst, "rb").read()
    at = 0
    for name, (coef, total) in zip(names[:n_checked], expect):
        got_total, = struct.unpack_from("<I", out, at)
        got = np.frombuffer(out, np.int16, coef.size, at + 4).reshape(coef.shape)
        at += 4 + 2 * coef.size
        assert got_total == total == coef.shape[0] and np.array_equal(got, coef), name
