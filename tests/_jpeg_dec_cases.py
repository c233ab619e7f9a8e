"""What tests/test_jpeg_dec_cpu.py and tests/test_jpeg_dec_gpu.py share: the golden files, files built at test time, the argument guards."""
import hashlib
import io
import os

import numpy as np

import _jpeg_dec_ref as dref
import _jpeg_ref as eref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_dec_pil.npz")
SUB_BITS, SYNC_THREADS = 1024, 256                 # csrc/jpeg_dec.hip: kSubBits, kSyncThreads


def load_golden():
    """{name: (file bytes, Pillow's pixels or None, SHA-256 of Pillow's pixels or None)}: the decoder's own files, then the encoder's 18 (`enc_`)"""
    assert os.path.getsize(GOLDEN) < 200 * 1024
    z = np.load(GOLDEN)
    enc = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz"))
    out = {}
    for k in z.files:
        if k.startswith("jpg_"):
            out[k[4:]] = (z[k].tobytes(), z["px_" + k[4:]], None)
    for k in enc.files:
        if k.startswith("jpg_"):
            name = k[4:]
            sha = bytes(z["sha_enc_" + name]) if "sha_enc_" + name in z.files else None
            out["enc_" + name] = (enc[k].tobytes(), None if sha else z["px_enc_" + name], sha)
    return out


def same_pixels(got, px, sha):
    got = np.ascontiguousarray(got)
    if sha is not None:
        return hashlib.sha256(got.tobytes()).digest() == sha
    return got.shape == px.shape and np.array_equal(got, px)


def pillow_turbo():
    try:
        from PIL import features
    except ImportError:
        return False
    return bool(features.check_feature("libjpeg_turbo"))


def pillow_pixels(data):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)))


def zeros_file():
    """512x512 zeros RGB: a periodic stream on which a wrong start never synchronises"""
    return eref.encode(np.zeros((512, 512, 3), np.uint8))


def cut(data, info, fraction=None, drop=None):
    """the file with its scan cut (no EOI): to `fraction` of its length, or by `drop` bytes"""
    n = info["scan_len"] if isinstance(info, dict) else info.scan_len
    off = info["scan_off"] if isinstance(info, dict) else info.scan_off
    keep = max(1, int(n * fraction)) if fraction is not None else n - drop
    return data[:off + keep]


def guard_cases(call, nbytes, need, W, ch):
    """`call(**overrides)` invokes st_jpeg_decode_u8 with valid arguments except the overrides; every case must give ST_EINVAL (1001)"""
    bad = [dict(file=None), dict(prm=None), dict(out=None), dict(status=None), dict(ws=None),
           dict(H=0), dict(W=0), dict(H=65536), dict(W=65536), dict(H=4096, W=4097, stride=1 << 20),
           dict(ncomp=2), dict(ncomp=4), dict(hs=1, vs=2), dict(hs=2, vs=3), dict(hs=4, vs=1), dict(hs=0),
           dict(tq=(2, 0, 0)), dict(td=(0, 2, 0)), dict(ta=(0, 0, -1)),
           dict(q_off=(nbytes - 63, nbytes - 63)), dict(q_off=(-1, -1)), dict(dc_off=(nbytes - 15, nbytes - 15)), dict(ac_off=(-1, 5)),
           dict(scan_off=-1), dict(scan_len=0), dict(scan_off=nbytes - 3, scan_len=4), dict(nbytes=0), dict(nbytes=(1 << 28) + 1),
           dict(stride=W * ch - 1), dict(need=need - 1), dict(ws_shift=4)]
    for kw in bad:
        assert call(**kw) == 1001, kw


def entry_call(info, file_ptr, out_ptr, status_ptr, ws_ptr, need):
    """the `call` of `guard_cases` over a probed file; the pointers are only dereferenced when every guard passes"""
    import ctypes as C
    from stitch_amd._lib import JpegDecParams, lib

    def call(**kw):
        f = dict(info._asdict())
        f.update({k: v for k, v in kw.items() if k in f})
        prm = JpegDecParams(f["H"], f["W"], f["ncomp"], f["hs"], f["vs"], (C.c_int32 * 3)(*f["tq"]), (C.c_int32 * 3)(*f["td"]), (C.c_int32 * 3)(*f["ta"]),
                            (C.c_int32 * 2)(*f["q_off"]), (C.c_int32 * 2)(*f["dc_off"]), (C.c_int32 * 2)(*f["ac_off"]), f["scan_off"], f["scan_len"])
        ws = kw.get("ws", ws_ptr)
        if ws is not None:
            ws += kw.get("ws_shift", 0)
        return lib.st_jpeg_decode_u8(kw.get("file", file_ptr), f["nbytes"], None if "prm" in kw else C.byref(prm), kw.get("out", out_ptr),
                                     kw.get("stride", info.W * info.ncomp), kw.get("status", status_ptr), ws, kw.get("need", need), None)
    return call
