"""Writes tests/golden/jpeg_pil.npz: the inputs of tests/_jpeg_ref.py's `golden_cases()` and the files Pillow's `Image.save` (defaults:
quality 75, 4:2:0, standard Huffman tables) writes for them.  Data only; needs a Pillow built on libjpeg-turbo.

    python tools/make_jpeg_golden.py
"""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _jpeg_ref as ref  # noqa: E402


def pillow_file(u8):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(u8).save(buf, format="JPEG")
    return buf.getvalue()


def main():
    from PIL import features
    assert features.check_feature("libjpeg_turbo"), "the contract is libjpeg-turbo's arithmetic"
    out, n_ff00, n_zrl = {}, 0, 0
    for name, u8 in ref.golden_cases().items():
        data = pillow_file(u8)
        hdr = ref.HEADER_BYTES[3 if u8.ndim == 3 else 1]
        stats = {}
        assert ref.encode(u8, stats=stats) == data, name
        n_ff00 += data[hdr:-2].count(b"\xff\x00")
        n_zrl += stats["zrl"]
        out["in_" + name] = u8
        out["jpg_" + name] = np.frombuffer(data, np.uint8)
    # the cases exercise byte stuffing and the 16-zero run code
    assert n_ff00 >= 1 and n_zrl >= 1, (n_ff00, n_zrl)
    path = os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 200 * 1024, size
    print(f"{path}: {len(out) // 2} cases, {size} bytes, {n_ff00} stuffed bytes, {n_zrl} ZRL codes")


if __name__ == "__main__":
    main()
