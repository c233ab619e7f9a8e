"""CPU restatement of the JPEG encoder's options, on top of tests/_jpeg_ref.py (its DCT, colour conversion, h2v2 downsampling and, for the
Annex K tables, its entropy coder): the file `Image.fromarray(u8).save(path, quality=q, subsampling=s, optimize=o)` writes on
libjpeg-turbo, in integer numpy.  csrc/jpeg.hip implements the same contract on the GPU (`st_jpeg_encode_u8_ex`);
tests/test_jpeg_opts_cpu.py pins this file to Pillow (tests/golden/jpeg_opts_pil.npz, written by tools/make_jpeg_opts_golden.py).

  quality      1..100: libjpeg's scaling (5000 / q below 50, 200 - 2 q from 50 up), (base * scale + 50) / 100 clamped to 1..255
  subsampling  None / 2: 4:2:0 (16x16 MCU), 1: 4:2:2 (16x8 MCU: Y Y Cb Cr, h2v1 with the alternating 0 / 1 bias), 0: 4:4:4 (8x8 MCU)
  optimize     libjpeg's two passes: four histograms (DC / AC x table 0 / 1) of exactly the symbols the scan emits, `gen_optimal_table`
               (jpeg_gen_optimal_table) on each, DHT segments that list only those symbols

`defect` plants one deliberate deviation (tests only: each must change at least one golden file)."""
import numpy as np

import _jpeg_ref as ref

DEFECTS = ("h2v1_bias_const", "h2v1_right_downsampled", "scale_no_round", "no_clamp_255", "no_pseudo_symbol", "tie_reversed", "no_length_limit",
           "huffval_unsorted", "dht_unused_symbols")
SAMPLING = {None: (2, 2), 2: (2, 2), 1: (2, 1), 0: (1, 1)}
STD_TABLES = (ref.DC_LUMA, ref.AC_LUMA, ref.DC_CHROMA, ref.AC_CHROMA)               # DHT order: DC0, AC0, DC1, AC1


def quant_table(base, quality, defect=None):
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    q = (base * scale + (0 if defect == "scale_no_round" else 50)) // 100
    return np.clip(q, 1, 1 << 20 if defect == "no_clamp_255" else 255).astype(np.int64)


# ---- sample planes -> quantised blocks in scan order ------------------------------------------------------------------------------------
def _downsample_h2v1(c, H, W, mcu_rows, mcu_cols, defect):
    """right edge from the padded INPUT columns; bias 0 in even, 1 in odd output columns"""
    c = ref._pad_to(c, H, 16 * mcu_cols)
    bias = 1 if defect == "h2v1_bias_const" else np.tile(np.array([0, 1]), 4 * mcu_cols)[None, :]
    d = (c[:, 0::2] + c[:, 1::2] + bias) >> 1
    if defect == "h2v1_right_downsampled":
        d = ref._pad_to(d[:, :(W + 1) // 2], d.shape[0], d.shape[1])
    return ref._pad_to(d, 8 * mcu_rows, 8 * mcu_cols)


def scan_blocks(u8, quality=75, hs=2, vs=2, defect=None):
    """(coefficients [n, 64] zigzag, component index [n]) in scan order"""
    ql, qc = quant_table(ref.Q_LUMA, quality, defect), quant_table(ref.Q_CHROMA, quality, defect)
    H, W = u8.shape[:2]
    hb, wb = -(-H // 8), -(-W // 8)
    if u8.ndim == 2:
        c = ref._blocks(ref._pad_to(u8.astype(np.int64), 8 * hb, 8 * wb), ql, None)
        return c.reshape(-1, 64), np.zeros(hb * wb, np.int64)
    mr, mc = -(-H // (8 * vs)), -(-W // (8 * hs))
    y, cb, cr = ref._ycc(u8)
    yq = np.zeros((vs * mr, hs * mc, 64), np.int64)
    yq[:hb, :wb] = ref._blocks(ref._pad_to(y, 8 * hb, 8 * wb), ql, None)
    if wb < hs * mc:                                             # dummy block right of a real one: AC zero, DC of the block before it
        yq[:hb, wb, 0] = yq[:hb, wb - 1, 0]
    if hb < vs * mr:                                             # dummy bottom row (4:2:0 only): DC of the last block of the row above, per MCU
        yq[hb, :, 0] = np.repeat(yq[hb - 1, 1::2, 0], 2)
    if (hs, vs) == (2, 2):
        planes = [ref._downsample(c, H, W, mr, mc, None) for c in (cb, cr)]
    elif (hs, vs) == (2, 1):
        planes = [_downsample_h2v1(c, H, W, mr, mc, defect) for c in (cb, cr)]
    else:
        planes = [ref._pad_to(c, 8 * mr, 8 * mc) for c in (cb, cr)]
    cq = [ref._blocks(p, qc, None) for p in planes]
    mcu = np.stack([yq[i::vs, j::hs] for i in range(vs) for j in range(hs)] + cq, axis=2)
    return mcu.reshape(-1, 64), np.tile(np.array([0] * (hs * vs) + [1, 2]), mr * mc)


# ---- symbols, optimal tables ------------------------------------------------------------------------------------------------------------
def symbols(coefs, comp):
    """what the scan emits, in order: (table 0..3 in DHT order, symbol, value, magnitude bits)"""
    out, pred = [], [0, 0, 0]
    for blk, ci in zip(coefs, comp):
        t = 0 if ci == 0 else 2
        diff = int(blk[0]) - pred[ci]
        pred[ci] = int(blk[0])
        n = ref._nbits(diff)
        out.append((t, n, diff, n))
        last = 0
        for k in np.flatnonzero(blk[1:]) + 1:
            run = int(k) - last - 1
            while run > 15:
                out.append((t + 1, 0xF0, 0, 0))
                run -= 16
            v = int(blk[k])
            n = ref._nbits(v)
            out.append((t + 1, (run << 4) | n, v, n))
            last = int(k)
        if last < 63:
            out.append((t + 1, 0x00, 0, 0))
    return out


def histograms(syms):
    h = np.zeros((4, 257), np.int64)
    for t, s, _, _ in syms:
        h[t, s] += 1
    return h


def gen_optimal_table(freq, defect=None):
    """jpeg_gen_optimal_table (jchuff.c): freq [256] or [257] -> (bits of lengths 1.., huffval, the longest code before the limit)"""
    freq = [int(v) for v in freq[:256]] + [0 if defect == "no_pseudo_symbol" else 1]      # the pseudo-symbol keeps the all-ones code free
    codesize, others = [0] * 257, [-1] * 257
    if sum(1 for v in freq if v) == 1:                           # (only without the pseudo-symbol: a lone symbol still needs a code)
        codesize[[i for i in range(257) if freq[i]][0]] = 1
    while True:
        # the two least frequent entries; among equals the LARGER symbol
        order = sorted((i for i in range(257) if freq[i]), key=(lambda i: (freq[i], i)) if defect == "tie_reversed" else (lambda i: (freq[i], -i)))
        if len(order) < 2:
            break
        c1, c2 = order[0], order[1]
        freq[c1] += freq[c2]
        freq[c2] = 0
        for c, link in ((c1, c2), (c2, None)):                  # every member of both trees gets one bit longer; c2's chain is hung behind c1's
            codesize[c] += 1
            while others[c] >= 0:
                c = others[c]
                codesize[c] += 1
            if link is not None:
                others[c] = link
    bits = [0] * 40
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    depth = max((i for i in range(40) if bits[i]), default=0)
    if defect != "no_length_limit":
        for i in range(32, 16, -1):                              # Annex K.2: move pairs of the longest codes up
            while bits[i] > 0:
                j = i - 2
                while bits[j] == 0:
                    j -= 1
                bits[i] -= 2
                bits[i - 1] += 1
                bits[j + 1] += 2
                bits[j] -= 1
    if defect != "no_pseudo_symbol":
        i = max(k for k in range(40) if bits[k])
        bits[i] -= 1                                             # the pseudo-symbol had one of the longest codes
    huffval = []
    for length in range(1, 40):
        at = [j for j in range(256) if codesize[j] == length]
        huffval += at[::-1] if defect == "huffval_unsorted" else at
    return bits[1:], huffval, depth


def huff_codes(bits, huffval):
    """{symbol: (code, length)} (Annex C), lengths past 16 included (a planted defect may leave them)"""
    out, code, k = {}, 0, 0
    for length in range(1, len(bits) + 1):
        for _ in range(bits[length - 1]):
            out[huffval[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def optimal_tables(hist, ntab, defect=None):
    """the (bits, huffval) of the DHT segments, in their order"""
    tabs = []
    for t in range(ntab):
        freq = hist[t].copy()
        if defect == "dht_unused_symbols":
            freq[STD_TABLES[t][1]] = np.maximum(freq[STD_TABLES[t][1]], 1)
        bits, vals, _ = gen_optimal_table(freq, defect)
        tabs.append((bits, vals))
    return tabs


def entropy_code(syms, tabs):
    """the symbols with the given tables -> the stuffed scan bytes (the bit packing of _jpeg_ref.entropy_code)"""
    codes = [huff_codes(*t) for t in tabs]
    vals, lens = [], []
    for t, s, v, n in syms:
        code, length = codes[t][s]
        if v < 0:
            v -= 1
        vals.append((code << n) | (v & ((1 << n) - 1)))
        lens.append(length + n)
    vals, lens = np.array(vals, np.int64), np.array(lens, np.int64)      # (at most 16 + 16 bits: a planted defect's long codes have no magnitude bits)
    off = np.cumsum(lens) - lens
    total = int(lens.sum())
    bits = np.ones((total + 7) // 8 * 8, np.uint8)
    bits[:total] = 0
    for k in range(int(lens.max())):
        m = lens > k
        bits[off[m] + k] = (vals[m] >> (lens[m] - 1 - k)) & 1
    data = np.packbits(bits)
    return np.insert(data, np.flatnonzero(data == 0xFF) + 1, 0).tobytes()


def header(H, W, channels, quality, hs, vs, tabs, defect=None):
    """SOI .. SOS: APP0, DQT x n, SOF0, DHT x n (DC0, AC0, DC1, AC1), SOS"""
    def seg(marker, payload):
        return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)
    qs = [quant_table(ref.Q_LUMA, quality, defect)] + ([quant_table(ref.Q_CHROMA, quality, defect)] if channels == 3 else [])
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, q in enumerate(qs):
        out += seg(0xDB, bytes([i]) + bytes(int(v) & 255 for v in q[ref.ZIGZAG]))
    comps = [(1, hs << 4 | vs, 0), (2, 0x11, 1), (3, 0x11, 1)] if channels == 3 else [(1, 0x11, 0)]
    out += seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([len(comps)]) + bytes(b for c in comps for b in c))
    for tc_th, (bits, vals) in zip((0x00, 0x10, 0x01, 0x11), tabs):
        out += seg(0xC4, bytes([tc_th]) + bytes(list(bits[:16])) + bytes(vals))
    sel = [(1, 0x00), (2, 0x11), (3, 0x11)] if channels == 3 else [(1, 0x00)]
    return out + seg(0xDA, bytes([len(sel)]) + bytes(b for s in sel for b in s) + bytes([0, 63, 0]))


def encode(u8, quality=None, subsampling=None, optimize=False, defect=None, stats=None):
    """uint8 [H,W,3] (RGB) or [H,W] (L) -> the file `Image.fromarray(u8).save(path, quality=, subsampling=, optimize=)` writes"""
    u8 = np.asarray(u8)
    assert u8.dtype == np.uint8 and (u8.ndim == 2 or (u8.ndim == 3 and u8.shape[2] == 3)), (u8.dtype, u8.shape)
    assert defect is None or defect in DEFECTS, defect
    quality = 75 if quality is None else int(quality)
    assert 1 <= quality <= 100 and subsampling in SAMPLING and (u8.ndim == 3 or subsampling is None)
    hs, vs = SAMPLING[subsampling] if u8.ndim == 3 else (1, 1)
    H, W = u8.shape[:2]
    channels = 1 if u8.ndim == 2 else 3
    coefs, comp = scan_blocks(u8, quality, hs, vs, defect)
    ntab = 2 if channels == 1 else 4
    if optimize:
        syms = symbols(coefs, comp)
        hist = histograms(syms)
        tabs = optimal_tables(hist, ntab, defect)
        scan = entropy_code(syms, tabs)
        if stats is not None:
            stats.update(hist=hist, tabs=tabs, zrl=int(hist[1, 0xF0] + hist[3, 0xF0]), depth=[gen_optimal_table(hist[t])[2] for t in range(ntab)],
                         max_dc=int(max(np.flatnonzero(hist[0, :256]).max(), np.flatnonzero(hist[2, :256]).max() if ntab == 4 else 0)),
                         max_ac=int(max((s & 15) for t, s, _, _ in syms if t & 1)))
    else:
        tabs = [(list(b), list(v)) for b, v in STD_TABLES[:ntab]]
        scan = ref.entropy_code(coefs, comp, None, stats)
        if stats is not None:
            syms = symbols(coefs, comp)
            stats.update(max_dc=max(s for t, s, _, _ in syms if not t & 1), max_ac=max((s & 15) for t, s, _, _ in syms if t & 1))
    return header(H, W, channels, quality, hs, vs, tabs, defect) + scan + b"\xff\xd9"


# ---- the cases of tests/golden/jpeg_opts_pil.npz (inputs are stored there; these build them) -------------------------------------------
SIZES = ((1, 1), (8, 8), (7, 9), (16, 16), (15, 17), (17, 15), (9, 33), (40, 24))          # where an MCU edge can go wrong
QUALITIES = (1, 25, 50, 75, 90, 95, 100)
LIMIT_CASE = "limit_840x840"


def square_wave():
    """64x64 L: rows of alternating all-0 / all-255 blocks (DC differences of 11 bits at quality 100), then blocks holding a 128 +- 127 square
    wave of period 8, horizontal, vertical and both (AC coefficients of 10 bits)"""
    u8 = np.zeros((64, 64), np.uint8)
    by, bx = np.mgrid[0:8, 0:8]
    u8[:32] = np.kron((((by[:4] + bx[:4]) & 1) * 255), np.ones((8, 8), np.int64)).astype(np.uint8)
    i, j = np.mgrid[0:32, 0:64]
    kind = ((i >> 3) + (j >> 3)) % 3
    wave = np.where(kind == 0, (j & 7) < 4, np.where(kind == 1, (i & 7) < 4, ((j & 7) < 4) ^ ((i & 7) < 4)))
    u8[32:] = np.where(wave, 255, 1).astype(np.uint8)
    return u8


def limit_case():
    """The code-length-limit case: an L image of 105 x 105 blocks for quality 50, optimize.  Block type k of 18 holds one AC coefficient at
    zigzag index 1 + run -- value 1 q for runs 0..9, then 3 q for runs 0..7 -- made as rint(128 + IDCT), and occurs 1, 2, 3, 5, 8, ...
    (Fibonacci) times, in this order along the block rows; the remaining 81 blocks are flat 128.  The AC histogram is Fibonacci-like, so the
    unlimited Huffman code is deeper than 16 bits."""
    q = quant_table(ref.Q_LUMA, 50)
    x = np.arange(8)
    basis = np.cos((2 * x[:, None] + 1) * x[None, :] * np.pi / 16) * np.where(x == 0, np.sqrt(0.5), 1.0)[None, :] / 2       # [sample, frequency]
    kinds = [(run, 1) for run in range(10)] + [(run, 3) for run in range(8)]
    counts, a, b = [], 1, 2
    for _ in kinds:
        counts.append(a)
        a, b = b, a + b
    assert sum(counts) == 10944
    blocks = []
    for (run, mult), n in zip(kinds, counts):
        nat = int(ref.ZIGZAG[1 + run])
        F = np.zeros((8, 8))
        F[nat >> 3, nat & 7] = mult * int(q[nat])
        blk = np.rint(128 + basis @ F @ basis.T).astype(np.uint8)
        blocks += [blk] * n
    blocks += [np.full((8, 8), 128, np.uint8)] * (105 * 105 - len(blocks))
    return np.stack(blocks).reshape(105, 105, 8, 8).transpose(0, 2, 1, 3).reshape(840, 840)


def case_name(inp, quality, subsampling, optimize):
    return f"{inp}__q{quality}__s{'n' if subsampling is None else subsampling}__o{int(optimize)}"


def parse_case(name):
    """-> (input name, dict of `save` / `encode` keywords)"""
    inp, q, s, o = name.split("__")
    kw = dict(quality=int(q[1:]), optimize=bool(int(o[1:])))
    if s[1:] != "n":
        kw["subsampling"] = int(s[1:])
    return inp, kw


def golden_inputs():
    inputs = {}
    for k, (h, w) in enumerate(SIZES):
        inputs[f"rgb_{h}x{w}"] = ref._smooth(h, w, 3, 300 + k)
        inputs[f"l_{h}x{w}"] = ref._smooth(h, w, 0, 400 + k)
    inputs["noise_17x33"] = np.random.RandomState(11).randint(0, 256, (17, 33, 3)).astype(np.uint8)
    inputs["flat_l_8x8"] = np.full((8, 8), 128, np.uint8)
    inputs["wave_l_64x64"] = square_wave()
    inputs["wave_rgb_64x64"] = np.repeat(square_wave()[:, :, None], 3, axis=2)
    return inputs


def golden_cases():
    """the case names (the limit case apart: it is made by recipe and pinned by length and SHA-256)"""
    names = []
    for h, w in SIZES:
        names += [case_name(f"rgb_{h}x{w}", 75, s, o) for s in (0, 1, 2) for o in (False, True)]
        names += [case_name(f"l_{h}x{w}", 75, None, o) for o in (False, True)]
    names += [case_name("noise_17x33", q, s, o) for q in QUALITIES for s in (0, 1, 2) for o in (False, True)]
    names.append(case_name("flat_l_8x8", 75, None, True))
    names += [case_name("wave_l_64x64", 100, None, o) for o in (False, True)]
    names += [case_name("wave_rgb_64x64", 100, s, o) for s in (0, 2) for o in (False, True)]
    return names
