"""CPU restatement of JPEG restart intervals, on top of tests/_jpeg_ref.py, tests/_jpeg_opts_ref.py (encoder) and tests/_jpeg_dec_ref.py
(decoder), which stay as they are.  The jpegr_* kernels of csrc/jpeg_dec.hip implement the decoder side on the GPU; tests/test_jpeg_rst_cpu.py pins this file to
Pillow on libjpeg-turbo (tests/golden/jpeg_rst_pil.npz, written by tools/make_jpeg_rst_golden.py).

Encoder (libjpeg's jcmaster.c / jchuff.c as Pillow's `save(..., restart_marker_blocks=b, restart_marker_rows=r)` drives them):
  interval     Ri in MCUs: with r > 0 min(r * MCUs per row, 65535), rows win over blocks; otherwise b (0..65535); 0: the file without the keywords
  DRI          FF DD 00 04 Ri directly in front of SOS, behind the DHTs
  in front of MCU k * Ri (k >= 1): the pending bits padded with 1-bits to a byte (a padded 0xFF is stuffed like any data byte), the marker
               FF D0 + ((k - 1) & 7) unstuffed, every component's DC prediction back to 0; no marker behind the last interval
  optimize     the histograms count the DC differences after those resets; markers and padding are no symbols

Decoder (jdhuff.c): `probe(data, restart=True)` takes today's files plus one DRI > 0 with exactly ceil(MCUs / Ri) - 1 markers D0, D1, ... D7,
D0, ... in order; an interval decodes like today's scan from DC predictions 0, the padding bits behind its last MCU are ignored, its
coefficient writes stay inside its own blocks.  The pixels are `np.array(PIL.Image.open(...))`.

`defect` plants one deliberate deviation in the encoder (tests only: each must change at least one golden file): see DEFECTS."""
from unittest import mock

import numpy as np

import _jpeg_dec_ref as dref
import _jpeg_opts_ref as oref
import _jpeg_ref as eref

DEFECTS = ("dc_no_reset", "marker_no_wrap", "pad0", "marker_behind_last", "rows_as_blocks", "no_clamp", "hist_no_reset")


# ---- encoder --------------------------------------------------------------------------------------------------------------------
def restart_interval(H, W, hs, vs, restart_marker_blocks=0, restart_marker_rows=0, defect=None):
    """Ri in MCUs of Pillow's two keywords (None counts as 0)"""
    b, r = int(restart_marker_blocks or 0), int(restart_marker_rows or 0)
    assert 0 <= b <= 65535 and r >= 0
    if r > 0:
        ri = r if defect == "rows_as_blocks" else r * -(-W // (8 * hs))
        return ri if defect == "no_clamp" else min(ri, 65535)
    return b


def encode(u8, quality=None, subsampling=None, optimize=False, restart_marker_blocks=0, restart_marker_rows=0, defect=None, stats=None):
    """uint8 [H,W,3] (RGB) or [H,W] (L) -> the file `Image.fromarray(u8).save(path, quality=, subsampling=, optimize=, restart_marker_blocks=,
    restart_marker_rows=)` writes.  stats (a dict) receives per interval the padding bits and whether its last byte is a padded 0xFF."""
    u8 = np.asarray(u8)
    assert defect is None or defect in DEFECTS, defect
    quality = 75 if quality is None else int(quality)
    hs, vs = oref.SAMPLING[subsampling] if u8.ndim == 3 else (1, 1)
    H, W = u8.shape[:2]
    channels = 1 if u8.ndim == 2 else 3
    ri = restart_interval(H, W, hs, vs, restart_marker_blocks, restart_marker_rows, defect)
    if ri == 0:
        return oref.encode(u8, quality=quality, subsampling=subsampling, optimize=optimize)
    coefs, comp = oref.scan_blocks(u8, quality, hs, vs)
    nb = hs * vs + 2 if channels == 3 else 1
    nmcu = len(coefs) // nb
    cuts = list(range(0, nmcu, ri))
    if defect == "dc_no_reset":                                              # one prediction chain, cut into the intervals' symbols afterwards
        syms_all = oref.symbols(coefs, comp)
        ends = np.flatnonzero([not t & 1 for t, _, _, _ in syms_all])        # a DC symbol starts every block
        at = [int(ends[m * nb]) for m in cuts] + [len(syms_all)]
        syms = [syms_all[at[i]:at[i + 1]] for i in range(len(cuts))]
    else:
        syms = [oref.symbols(coefs[m * nb:(m + ri) * nb], comp[m * nb:(m + ri) * nb]) for m in cuts]
    ntab = 2 if channels == 1 else 4
    if optimize:
        counted = oref.symbols(coefs, comp) if defect == "hist_no_reset" else [s for part in syms for s in part]
        tabs = oref.optimal_tables(oref.histograms(counted), ntab)
    else:
        tabs = [(list(b), list(v)) for b, v in oref.STD_TABLES[:ntab]]
    scan = b""
    for k, part in enumerate(syms):
        if k:
            scan += bytes([0xFF, 0xD0 + ((k - 1) if defect == "marker_no_wrap" else (k - 1) & 7)])
        body = oref.entropy_code(part, tabs)
        total = sum(oref.huff_codes(*tabs[t])[s][1] + n for t, s, _, n in part)
        if defect == "pad0" and total % 8:
            raw = bytearray(dref.unstuff(body).tobytes())
            raw[-1] &= 0xFF ^ ((1 << (8 - total % 8)) - 1)
            data = np.frombuffer(bytes(raw), np.uint8)
            body = np.insert(data, np.flatnonzero(data == 0xFF) + 1, 0).tobytes()
        if stats is not None:
            stats.setdefault("pad_bits", []).append(-total % 8)
            stats.setdefault("padded_ff", []).append(bool(total % 8) and body.endswith(b"\xff\x00"))
        scan += body
    if defect == "marker_behind_last":
        scan += bytes([0xFF, 0xD0 + ((len(syms) - 1) & 7)])
    if stats is not None:
        stats["zrl"] = sum(1 for part in syms for _, s, _, _ in part if s == 0xF0)
        chain = oref.symbols(coefs, comp)                                       # one prediction chain: the DC symbol of every block
        dc = [s for s in chain if not s[0] & 1]
        stats["dc_differs"] = any(part[0][2] != dc[m * nb][2] for part, m in zip(syms, cuts))
    head = oref.header(H, W, channels, quality, hs, vs, tabs)
    sos = len(head) - (2 + 6 + 2 * channels)
    assert head[sos:sos + 2] == b"\xff\xda"
    return head[:sos] + b"\xff\xdd\x00\x04" + (ri & 0xFFFF).to_bytes(2, "big") + head[sos:] + scan + b"\xff\xd9"


# ---- decoder --------------------------------------------------------------------------------------------------------------------
def probe(data, restart=True):
    """`_jpeg_dec_ref.probe` with the package parser's `restart` switch: the dict has `restart_interval` too"""
    info = dref._probe(data, restart=restart)
    if info is None:
        return None
    d = {k: (list(v) if isinstance(v, tuple) else v) for k, v in info._asdict().items()}
    del d["nbytes"]
    return d


def intervals(data, info):
    """[(offset in the file, length)] of the entropy-coded bytes between the restart markers (any FF D0..D7), in order"""
    d = bytes(data)
    at, end = info["scan_off"], info["scan_off"] + info["scan_len"]
    out, q = [], at
    while True:
        q = d.find(b"\xff", q, end)
        if q < 0 or q + 1 >= end:
            break
        if 0xD0 <= d[q + 1] <= 0xD7:
            out.append((at, q - at))
            at = q + 2
        q += 2 if d[q + 1] != 0xFF else 1                            # (in a damaged file the next byte may start the marker)
    return out + [(at, end - at)]


def coefficients(data, info=None):
    """int64 [nblocks, 64] in zigzag order with the DC DIFFERENCES of the file (against 0 at an interval's start), the status the decoder
    reports (0; bit 0: an interval's bytes held fewer blocks than it has, bit 1: more), and per interval its padding bits"""
    info = info or probe(data)
    ri = info["restart_interval"]
    mr, mc, nb, nblocks = dref.geometry(info)
    nint = -(-(mr * mc) // ri)
    d = bytes(data)
    parts = [d[off:off + n] for off, n in intervals(d, info)]
    parts = parts[:nint - 1] + [b"".join(parts[nint - 1:])]                    # a marker too many is dropped: its bytes stay in the last interval
    parts += [b""] * (nint - len(parts))                                        # a missing one leaves empty intervals at the end
    coef = np.zeros((nblocks, 64), np.int64)
    status, pads = 0, []
    for i, body in enumerate(parts):
        lo, hi = i * ri * nb, min((i + 1) * ri * nb, nblocks)
        s = dref.Stream(d[:info["scan_off"]] + body, dict(info, scan_len=len(body)))

        def sink(b, k, v):
            if lo + b < hi:
                coef[lo + b, k] = v
        (pos, _, _), got = s.run((0, 0, 0), s.nbits, sink)
        pads.append(s.nbits - pos)
        if got != hi - lo:
            status |= 1 if got < hi - lo else 2
    return coef, status, pads


def decode(data, info=None):
    """file bytes -> uint8 [H,W,3] or [H,W]: `np.array(PIL.Image.open(io.BytesIO(data)))` for a file with or without restart intervals"""
    info = info or probe(data)
    assert info is not None, "unsupported file"
    if not info["restart_interval"]:
        return dref.decode(data, info)
    coef, _, _ = coefficients(data, info)
    ri = info["restart_interval"]
    mr, mc, nb, nblocks = dref.geometry(info)
    comp = np.tile(np.array([0] * (nb - 2) + [1, 2]) if info["ncomp"] == 3 else np.array([0]), mr * mc)
    mcu = np.repeat(np.arange(mr * mc), nb)
    for c in range(info["ncomp"]):                                            # absolute DC per interval, then as differences along the whole scan:
        m = comp == c                                                         # what `_jpeg_dec_ref.planes` expects of `coefficients`
        v, seg = coef[m, 0], mcu[m] // ri
        tot = np.cumsum(v)
        first = np.flatnonzero(np.diff(seg, prepend=-1))
        absolute = tot - np.repeat(tot[first] - v[first], np.diff(np.append(first, len(v))))
        coef[m, 0] = np.diff(absolute, prepend=0)
    with mock.patch.object(dref, "coefficients", lambda *a, **k: (coef, nblocks)):
        return dref.decode(data, info)


# ---- the cases of tests/golden/jpeg_rst_pil.npz (inputs are stored there; these build them) -------------------------------------------
SIZES = ((1, 1), (17, 23), (40, 52), (64, 48))
KINDS = (("l", None), ("444", 0), ("422", 1), ("420", 2))
CLAMP_CASE = "flat_l_8x65500__q75__sn__o0__b0__r9"


def case_name(inp, quality=75, subsampling=None, optimize=False, blocks=0, rows=0):
    return f"{inp}__q{quality}__s{'n' if subsampling is None else subsampling}__o{int(optimize)}__b{blocks}__r{rows}"


def parse_case(name):
    """-> (input name, dict of `save` / `encode` keywords)"""
    inp, q, s, o, b, r = name.split("__")
    kw = dict(quality=int(q[1:]), optimize=bool(int(o[1:])))
    if s[1:] != "n":
        kw["subsampling"] = int(s[1:])
    if int(b[1:]):
        kw["restart_marker_blocks"] = int(b[1:])
    if int(r[1:]):
        kw["restart_marker_rows"] = int(r[1:])
    return inp, kw


def golden_inputs(seed=0):
    """`seed` moves the two noise images: tools/make_jpeg_rst_golden.py searches it until the set holds every situation it asserts"""
    inputs = {}
    for k, (h, w) in enumerate(SIZES):
        inputs[f"rgb_{h}x{w}"] = eref._smooth(h, w, 3, 600 + k)
        inputs[f"l_{h}x{w}"] = eref._smooth(h, w, 0, 700 + k)
    inputs["l_9x70"] = eref._smooth(9, 70, 0, 710)
    inputs["noise_l_64x48"] = np.random.RandomState(800 + seed).randint(0, 256, (64, 48)).astype(np.uint8)
    inputs["noise_rgb_40x52"] = np.random.RandomState(900 + seed).randint(0, 256, (40, 52, 3)).astype(np.uint8)
    inputs["flat_l_8x65500"] = np.full((8, 65500), 128, np.uint8)      # libjpeg's largest side: 8188 MCUs per row
    return inputs


def golden_cases():
    names = []
    for h, w in SIZES:
        for kind, sub in KINDS:
            inp = f"{'l' if kind == 'l' else 'rgb'}_{h}x{w}"
            names.append(case_name(inp, subsampling=sub, blocks=1))                     # 1x1: one MCU, a DRI segment and no marker
            if (h, w) == (40, 52):
                names += [case_name(inp, subsampling=sub, blocks=b) for b in (2, 3, 7)]     # 3 and 7 do not divide an MCU row
                names += [case_name(inp, subsampling=sub, rows=1), case_name(inp, subsampling=sub, rows=2), case_name(inp, subsampling=sub, blocks=3, rows=1)]
            if (h, w) == (17, 23):
                hs, vs = (1, 1) if kind == "l" else oref.SAMPLING[sub]
                names += [case_name(inp, subsampling=sub, blocks=-(-h // (8 * vs)) * -(-w // (8 * hs))), case_name(inp, subsampling=sub, blocks=1000)]
    names += [case_name("l_9x70", blocks=1), case_name("l_9x70", blocks=4), case_name("l_9x70", rows=1)]
    names += [case_name("rgb_64x48", 95, 0, True, blocks=9), case_name("l_64x48", 95, None, True, blocks=9), case_name("rgb_40x52", 95, 2, True, blocks=9)]
    names += [case_name("rgb_40x52", q, 2, blocks=3) for q in (30, 95)] + [case_name("l_40x52", q, None, blocks=3) for q in (30, 95)]
    names += [case_name("noise_l_64x48", 95, None, blocks=1), case_name("noise_l_64x48", 95, None, True, blocks=1), case_name("noise_rgb_40x52", 30, 0, rows=1),
              case_name("noise_rgb_40x52", 95, 2, True, blocks=2)]
    return names + [CLAMP_CASE]


def load_golden():
    """{case: (input, `save` keywords, Pillow's file, Pillow's pixels of it)} of tests/golden/jpeg_rst_pil.npz"""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_rst_pil.npz")
    assert os.path.getsize(path) < 400 * 1024
    z = np.load(path)
    out = {}
    for name in golden_cases():
        inp, kw = parse_case(name)
        out[name] = (z["in_" + inp], kw, z["jpg_" + name].tobytes(), z["px_" + name])
    return out


def damaged(data, info, which):
    """the file with the bytes of interval `which` halved (its marker stays): that interval holds too few blocks, no other one changes"""
    off, n = intervals(data, info)[which]
    return data[:off + n // 2] + data[off + n:]
