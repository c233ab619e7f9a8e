"""Writes tests/golden/jpeg_rst_pil.npz: the inputs of tests/_jpeg_rst_ref.py's `golden_inputs()`, the files Pillow's
`Image.save(..., restart_marker_blocks=, restart_marker_rows=)` writes for `golden_cases()`, and the pixels Pillow decodes from them.  The seed
of the two noise inputs is searched until the set holds an interval that ends exactly on a byte boundary, a padded last byte that is 0xFF and
therefore stuffed (FF 00 FF Dn), a ZRL code inside an interval and a DC difference at an interval's start that differs from the unreset one.
Data only; needs a Pillow built on libjpeg-turbo.

    python tools/make_jpeg_rst_golden.py
"""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _jpeg_rst_ref as rst  # noqa: E402


def pillow_file(u8, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(u8).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def pillow_pixels(data):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)))


def build(seed):
    inputs = rst.golden_inputs(seed)
    out = {"in_" + k: v for k, v in inputs.items()}
    seen = dict(aligned=0, padded_ff=0, zrl=0, dc_differs=0, wraps=0)
    for name in rst.golden_cases():
        inp, kw = rst.parse_case(name)
        data = pillow_file(inputs[inp], **kw)
        stats = {}
        assert rst.encode(inputs[inp], stats=stats, **kw) == data, name
        plain = {k: v for k, v in kw.items() if not k.startswith("restart_")}
        px = pillow_pixels(data)
        assert np.array_equal(px, pillow_pixels(pillow_file(inputs[inp], **plain))), name      # the pixels of the file without the keywords
        n = len(stats["pad_bits"])
        seen["aligned"] += sum(p == 0 for p in stats["pad_bits"][:-1])                           # in front of a marker
        seen["padded_ff"] += sum(stats["padded_ff"][:-1])
        seen["zrl"] += stats["zrl"] if n > 1 else 0
        seen["dc_differs"] += bool(stats["dc_differs"])
        seen["wraps"] += n >= 10
        out["jpg_" + name] = np.frombuffer(data, np.uint8)
        out["px_" + name] = px
    clamp = out["jpg_" + rst.CLAMP_CASE].tobytes()
    assert clamp[clamp.index(b"\xff\xdd"):][:6] == b"\xff\xdd\x00\x04\xff\xff"                # 9 rows of 8188 MCUs: clamped to 65535
    return out, seen


def main():
    from PIL import features
    assert features.check_feature("libjpeg_turbo"), "the contract is libjpeg-turbo's arithmetic"
    for seed in range(64):
        out, seen = build(seed)
        if all(seen.values()):
            break
        print(f"seed {seed}: {seen}")
    assert all(seen.values()), seen
    out["seed"] = np.array([seed], np.int64)
    path = os.path.join(ROOT, "tests", "golden", "jpeg_rst_pil.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 400 * 1024, size
    print(f"{path}: {len(rst.golden_cases())} cases, seed {seed}, {size} bytes, {seen}")


if __name__ == "__main__":
    main()
