"""CPU restatement of the baseline JPEG encoder the result files are written with: Pillow's `Image.save(path)` defaults on top of
libjpeg-turbo (quality 75, 4:2:0 for RGB, one component for L, the Annex K Huffman tables, JFIF header, integer "islow" DCT), in
integer numpy.  `encode(u8)` returns the whole file, SOI to EOI; csrc/jpeg.hip implements the same contract on the GPU and
tests/test_jpeg_cpu.py pins this file to Pillow (tests/golden/jpeg_pil.npz, written by tools/make_jpeg_golden.py).

`defect` plants one deliberate deviation (tests only: each must change at least one golden file, so the cases are known to exercise
the rule): "bias2", "chroma_right", "dummy_dc0", "quant_trunc", "no_stuffing", "pad0"."""
import numpy as np

DEFECTS = ("bias2", "chroma_right", "dummy_dc0", "quant_trunc", "no_stuffing", "pad0")

# ---- tables (ITU-T T.81 Annex K) ---------------------------------------------------------------------------------------------
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                    + [99] * 32)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
            0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
            0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
            0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
            0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
            0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
            0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
              0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
              0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
              0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
              0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
              0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
              0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
HEADER_BYTES = {3: 623, 1: 328}


def quant_table(base, quality=75):
    """jpeg_quality_scaling + jpeg_add_quant_table (natural order)."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base * scale + 50) // 100, 1, 255).astype(np.int64)


def huff_codes(spec):
    """{symbol: (code, length)} of a (bits, values) table (Annex C)."""
    bits, vals = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def header(H, W, channels):
    """SOI .. SOS exactly as Pillow writes them; only the four size bytes depend on the image."""
    def seg(marker, payload):
        return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)
    qs = [quant_table(Q_LUMA)] + ([quant_table(Q_CHROMA)] if channels == 3 else [])
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, q in enumerate(qs):
        out += seg(0xDB, bytes([i]) + bytes(int(v) for v in q[ZIGZAG]))
    comps = [(1, 0x22, 0), (2, 0x11, 1), (3, 0x11, 1)] if channels == 3 else [(1, 0x11, 0)]
    out += seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([len(comps)]) + bytes(b for c in comps for b in c))
    tabs = [(0x00, DC_LUMA), (0x10, AC_LUMA)] + ([(0x01, DC_CHROMA), (0x11, AC_CHROMA)] if channels == 3 else [])
    for tc_th, (bits, vals) in tabs:
        out += seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    sel = [(1, 0x00), (2, 0x11), (3, 0x11)] if channels == 3 else [(1, 0x00)]
    out += seg(0xDA, bytes([len(sel)]) + bytes(b for s in sel for b in s) + bytes([0, 63, 0]))
    assert len(out) == HEADER_BYTES[channels]
    return out


# ---- sample planes --------------------------------------------------------------------------------------------------------------
def _ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad_to(p, h, w):
    return np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge")


def _downsample(c, H, W, mcu_rows, mcu_cols, defect):
    """h2v2: right edge from the padded INPUT columns, bottom edge by replicating the last DOWNSAMPLED row."""
    c = _pad_to(c, H + (H & 1), 16 * mcu_cols)
    bias = np.tile(np.array([1, 2]), 4 * mcu_cols)[None, :]
    if defect == "bias2":
        bias = 2
    d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
    if defect == "chroma_right":
        d = _pad_to(d[:, :(W + 1) // 2], d.shape[0], d.shape[1])
    return _pad_to(d, 8 * mcu_rows, 8 * mcu_cols)


# ---- DCT + quantisation ---------------------------------------------------------------------------------------------------------
def _fdct_1d(d, first):
    """jfdctint.c along the last axis; first pass scales up by 2^PASS1_BITS, second removes it (outputs scaled by 8)."""
    CB, P1 = 13, 2
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    sh = CB - P1 if first else CB + P1

    def ds(x, n):
        return (x + (1 << (n - 1))) >> n
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << P1, (t10 - t11) << P1
    else:
        o[0], o[4] = ds(t10 + t11, P1), ds(t10 - t11, P1)
    z1 = (t12 + t13) * 4433
    o[2], o[6] = ds(z1 + t13 * 6270, sh), ds(z1 - t12 * 15137, sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = ds(t4 + z1 + z3, sh), ds(t5 + z2 + z4, sh), ds(t6 + z2 + z3, sh), ds(t7 + z1 + z4, sh)
    return np.stack(o, axis=-1)


def _blocks(plane, q, defect):
    """plane [8 bh, 8 bw] samples -> quantised coefficients [bh, bw, 64] in zigzag order."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128
    b = _fdct_1d(b, True)                                        # rows
    b = _fdct_1d(b.swapaxes(-1, -2), False).swapaxes(-1, -2)     # columns
    q8 = (q << 3).reshape(8, 8)
    r = (np.abs(b) + (0 if defect == "quant_trunc" else q8 >> 1)) // q8
    return (np.sign(b) * r).reshape(bh, bw, 64)[..., ZIGZAG]


def scan_blocks(u8, defect=None):
    """The quantised blocks in scan order: (coefficients [n, 64] zigzag, component index [n])."""
    H, W = u8.shape[:2]
    if u8.ndim == 2:
        hb, wb = -(-H // 8), -(-W // 8)
        c = _blocks(_pad_to(u8.astype(np.int64), 8 * hb, 8 * wb), quant_table(Q_LUMA), defect)
        return c.reshape(-1, 64), np.zeros(hb * wb, np.int64)
    mr, mc = -(-H // 16), -(-W // 16)
    hb, wb = -(-H // 8), -(-W // 8)
    y, cb, cr = _ycc(u8)
    yq = np.zeros((2 * mr, 2 * mc, 64), np.int64)
    yq[:hb, :wb] = _blocks(_pad_to(y, 8 * hb, 8 * wb), quant_table(Q_LUMA), defect)
    dummy = 0 if defect == "dummy_dc0" else 1
    if wb < 2 * mc:                                              # dummy block right of a real one: DC of the block before it
        yq[:hb, wb, 0] = yq[:hb, wb - 1, 0] * dummy
    if hb < 2 * mr:                                              # dummy bottom row: DC of the last block of the row above, per MCU
        yq[hb, :, 0] = np.repeat(yq[hb - 1, 1::2, 0], 2) * dummy
    cq = [_blocks(_downsample(c, H, W, mr, mc, defect), quant_table(Q_CHROMA), defect) for c in (cb, cr)]
    mcu = np.stack([yq[0::2, 0::2], yq[0::2, 1::2], yq[1::2, 0::2], yq[1::2, 1::2], cq[0], cq[1]], axis=2)      # [mr, mc, 6, 64]
    return mcu.reshape(-1, 64), np.tile(np.array([0, 0, 0, 0, 1, 2]), mr * mc)


# ---- entropy coding -------------------------------------------------------------------------------------------------------------
def _nbits(v):
    return int(abs(int(v))).bit_length()


def entropy_code(coefs, comp, defect=None, stats=None):
    """Huffman-code the blocks (interleaved scan, no restarts) -> the stuffed scan bytes."""
    dc = [huff_codes(DC_LUMA), huff_codes(DC_CHROMA)]
    ac = [huff_codes(AC_LUMA), huff_codes(AC_CHROMA)]
    vals, lens = [], []

    def put(code_len, v, n):
        code, length = code_len
        if v < 0:
            v = v - 1
        vals.append((code << n) | (v & ((1 << n) - 1)))
        lens.append(length + n)
    pred = [0, 0, 0]
    zrl = 0
    for blk, ci in zip(coefs, comp):
        t = 0 if ci == 0 else 1
        diff = int(blk[0]) - pred[ci]
        pred[ci] = int(blk[0])
        n = _nbits(diff)
        put(dc[t][n], diff, n)
        last = 0
        for k in np.flatnonzero(blk[1:]) + 1:
            run = int(k) - last - 1
            while run > 15:
                put(ac[t][0xF0], 0, 0)
                run -= 16
                zrl += 1
            v = int(blk[k])
            n = _nbits(v)
            put(ac[t][(run << 4) | n], v, n)
            last = int(k)
        if last < 63:
            put(ac[t][0x00], 0, 0)
    if stats is not None:
        stats["zrl"] = zrl
    vals, lens = np.array(vals, np.int64), np.array(lens, np.int64)
    off = np.cumsum(lens) - lens
    total = int(lens.sum())
    bits = np.full((total + 7) // 8 * 8, 0 if defect == "pad0" else 1, np.uint8)
    bits[:total] = 0
    for k in range(int(lens.max())):
        m = lens > k
        bits[off[m] + k] = (vals[m] >> (lens[m] - 1 - k)) & 1
    data = np.packbits(bits)
    if defect != "no_stuffing":
        ff = np.flatnonzero(data == 0xFF)
        data = np.insert(data, ff + 1, 0)
    return data.tobytes()


def encode(u8, defect=None, stats=None):
    """uint8 [H,W,3] (RGB) or [H,W] (L) -> the JPEG file Pillow's `Image.fromarray(u8).save(path)` writes."""
    u8 = np.asarray(u8)
    assert u8.dtype == np.uint8 and (u8.ndim == 2 or (u8.ndim == 3 and u8.shape[2] == 3)), (u8.dtype, u8.shape)
    assert defect is None or defect in DEFECTS, defect
    H, W = u8.shape[:2]
    coefs, comp = scan_blocks(u8, defect)
    return header(H, W, 1 if u8.ndim == 2 else 3) + entropy_code(coefs, comp, defect, stats) + b"\xff\xd9"


# ---- the cases of tests/golden/jpeg_pil.npz (inputs are stored there; these build them) -----------------------------------------
def _smooth(h, w, c, seed):
    """noise smoothed by a 5x5 box, stretched to 0..255: photographic statistics from integers only."""
    rng = np.random.RandomState(seed)
    x = rng.randint(0, 256, (h + 4, w + 4) + ((c,) if c else ())).astype(np.int64)
    s = sum(x[i:i + h, j:j + w] for i in range(5) for j in range(5))
    s = (s - s.min()) * 255 // max(1, int(s.max() - s.min()))
    return s.astype(np.uint8)


def pattern(h, w, c):
    """a seedless integer pattern for the large shapes: ramps with wrap-around edges"""
    i, j = np.mgrid[0:h, 0:w]
    p = [(3 * i + 2 * j + 40 * k + ((i * j) >> 6) + 17 * ((i >> 4) ^ (j >> 5))) & 255 for k in range(max(c, 1))]
    return (np.stack(p, -1) if c else p[0]).astype(np.uint8)


def zrl_block():
    """one 8x8 L block whose only AC energy is the highest frequency: zigzag index 63 after 62 zeros (three ZRL codes)"""
    i = np.arange(8)
    c = np.cos((2 * i + 1) * 7 * np.pi / 16)
    return np.clip(np.rint(128 + 120 * np.outer(c, c)), 0, 255).astype(np.uint8)


def golden_cases():
    cases = {}
    for k, (h, w) in enumerate([(1, 1), (8, 8), (16, 16), (17, 23), (18, 16), (16, 24), (9, 40), (40, 9), (25, 17)]):
        cases[f"rgb_{h}x{w}"] = _smooth(h, w, 3, 100 + k)
    cases["l_33x41"] = _smooth(33, 41, 0, 200)
    cases["mask_37x53"] = ((_smooth(37, 53, 0, 201) > 127) * 255).astype(np.uint8)
    cases["zeros_24x24"] = np.zeros((24, 24, 3), np.uint8)
    cases["ones_24x40"] = np.full((24, 40, 3), 255, np.uint8)
    cases["zeros_l_16x24"] = np.zeros((16, 24), np.uint8)
    cases["noise_64x48"] = np.random.RandomState(7).randint(0, 256, (64, 48, 3)).astype(np.uint8)
    cases["zrl_8x8"] = zrl_block()
    cases["big_rgb_130x1030"] = pattern(130, 1030, 3)
    cases["big_l_24x2056"] = pattern(24, 2056, 0)
    return cases
