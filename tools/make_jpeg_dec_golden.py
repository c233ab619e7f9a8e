"""Writes tests/golden/jpeg_dec_pil.npz: JPEG files written by Pillow (tests/_jpeg_dec_ref.py `golden_sources()`: L, 4:4:4, 4:2:2 and 4:2:0 at
several sizes and qualities, an optimize=True file, a file with COM and APP1 segments) with the pixels `np.array(Image.open(...))` returns
for them (`jpg_<name>` / `px_<name>`), and Pillow's pixels for the 18 files of tests/golden/jpeg_pil.npz (`px_enc_<name>`; the files stay
where they are).  The pixels of the two large files (130x1030, 24x2056) would not fit the size limit: a SHA-256 (`sha_enc_<name>`) pins all of them, the last 48
columns (`px_enc_<name>`, the partial MCU column included) are stored to be looked at.  Data only; needs a Pillow built on libjpeg-turbo.

    python tools/make_jpeg_dec_golden.py
"""
import hashlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _jpeg_dec_ref as ref  # noqa: E402


CROP_ABOVE, CROP_COLS = 40000, 48


def pillow_pixels(data):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)))


def main():
    from PIL import Image, features
    assert features.check_feature("libjpeg_turbo"), "the contract is libjpeg-turbo's arithmetic"
    out = {}
    for name, (u8, kw) in ref.golden_sources().items():
        buf = io.BytesIO()
        Image.fromarray(u8).save(buf, format="JPEG", **kw)
        data = buf.getvalue()
        px = pillow_pixels(data)
        assert px.shape == u8.shape and np.array_equal(ref.decode(data), px), name
        out["jpg_" + name] = np.frombuffer(data, np.uint8)
        out["px_" + name] = px
    enc = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz"))
    for k in enc.files:
        if k.startswith("jpg_"):
            data = enc[k].tobytes()
            px = pillow_pixels(data)
            assert np.array_equal(ref.decode(data), px), k
            if px.size > CROP_ABOVE:
                out["sha_enc_" + k[4:]] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(px).tobytes()).digest(), np.uint8)
                px = px[:, -CROP_COLS:]
            out["px_enc_" + k[4:]] = px
    path = os.path.join(ROOT, "tests", "golden", "jpeg_dec_pil.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 200 * 1024, size
    print(f"{path}: {sum(k.startswith('jpg_') for k in out)} files + {sum(k.startswith('px_enc_') for k in out)} of jpeg_pil.npz, {size} bytes")


if __name__ == "__main__":
    main()
