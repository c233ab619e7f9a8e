"""Writes tests/golden/jpeg_opts_pil.npz: the inputs of tests/_jpeg_opts_ref.py's `golden_inputs()` and the files Pillow's
`Image.save(quality=, subsampling=, optimize=)` writes for `golden_cases()`; for the code-length-limit case (made by recipe, 840x840) only the
length and SHA-256 of Pillow's file.  Data only; needs a Pillow built on libjpeg-turbo.

    python tools/make_jpeg_opts_golden.py
"""
import hashlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _jpeg_opts_ref as opts  # noqa: E402


def pillow_file(u8, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(u8).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def main():
    from PIL import features
    assert features.check_feature("libjpeg_turbo"), "the contract is libjpeg-turbo's arithmetic"
    inputs = opts.golden_inputs()
    out = {"in_" + k: v for k, v in inputs.items()}
    n_ff00 = n_zrl = max_dc = max_ac = 0
    for name in opts.golden_cases():
        inp, kw = opts.parse_case(name)
        data = pillow_file(inputs[inp], **kw)
        stats = {}
        assert opts.encode(inputs[inp], stats=stats, **kw) == data, name
        if kw["optimize"]:
            n_ff00 += data[data.index(b"\xff\xda") + 2:-2].count(b"\xff\x00")
            n_zrl += stats["zrl"]
        if inp.startswith("wave_"):
            max_dc, max_ac = max(max_dc, stats["max_dc"]), max(max_ac, stats["max_ac"])
        out["jpg_" + name] = np.frombuffer(data, np.uint8)
    # the goldens reach what they claim: the largest DC and AC categories, stuffed bytes and ZRL codes in optimised scans
    assert max_dc == 11 and max_ac == 10, (max_dc, max_ac)
    assert n_ff00 >= 1 and n_zrl >= 1, (n_ff00, n_zrl)
    flat = out["jpg_" + opts.case_name("flat_l_8x8", 75, None, True)].tobytes()
    assert flat.count(b"\xff\xc4\x00\x14") == 2                      # two one-symbol tables: 2 + 1 + 16 + 1 bytes each
    u8 = opts.limit_case()
    data = pillow_file(u8, quality=50, optimize=True)
    stats = {}
    assert opts.encode(u8, quality=50, optimize=True, stats=stats) == data
    assert stats["depth"][1] > 16, stats["depth"]                    # the AC code is deeper than 16 bits before the Annex K.2 adjustment
    assert max(l + 1 for l, n in enumerate(stats["tabs"][1][0]) if n) == 16
    out["limit_len"] = np.array([len(data)], np.int64)
    out["limit_sha256"] = np.frombuffer(hashlib.sha256(data).digest(), np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "jpeg_opts_pil.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 200 * 1024, size
    print(f"{path}: {len(opts.golden_cases())} cases, {size} bytes, {n_ff00} stuffed bytes and {n_zrl} ZRL codes in optimised scans, "
          f"DC / AC categories up to {max_dc} / {max_ac}, limit case {len(data)} bytes, unlimited depth {stats['depth'][1]}, AC counts per length "
          f"{stats['tabs'][1][0][:16]}")


if __name__ == "__main__":
    main()
