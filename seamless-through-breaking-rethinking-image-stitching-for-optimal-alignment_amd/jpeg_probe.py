"""Host-side marker parse of a JPEG file for the GPU decoder (csrc/jpeg_dec.hip; contract: README.md, tests/_jpeg_dec_ref.py `probe`).

Taken: one SOF0 frame at 8 bits; one component, or three (YCbCr: JFIF, or no Adobe marker saying otherwise) with luma sampling 1x1, 2x1 or
2x2 and chroma 1x1; one interleaved scan over all 63 AC coefficients; 8-bit DQT entries; any DHT tables 0..1; no restart interval; H * W <=
2^24; APPn / COM segments are skipped.  Everything else -- progressive, arithmetic, 12-bit, DRI, 4:4:0 and other factors, four components,
Adobe transform 0, several scans, a marker other than FF00 inside the scan -- is unsupported: `probe` returns None and nothing touches the
device.

`probe(data, restart=True)` also takes a file with one restart interval Ri > 0 (the last DRI in front of SOS) whose scan holds exactly
ceil(MCUs / Ri) - 1 restart markers, RST0, RST1, ... RST7, RST0, ... in that order (csrc/jpeg_dec.hip; contract: README.md "Restart
intervals", tests/_jpeg_rst_ref.py).  A marker without DRI, a missing one, one too many or one out of order: None."""
from typing import NamedTuple, Tuple

SAMPLINGS = ((1, 1), (2, 1), (2, 2))
MAX_PIXELS = 1 << 24
MAX_FILE_BYTES = 1 << 28


class JpegInfo(NamedTuple):
    """Offsets point into the file: q_off at the 64 zigzag-ordered entries of DQT table i, dc_off / ac_off at the 16 code counts of DHT table i
    (its values follow), -1: not defined; scan_off at the first entropy-coded byte, scan_len up to the EOI marker (or the end of a cut file)."""
    H: int
    W: int
    ncomp: int
    hs: int
    vs: int
    tq: Tuple[int, ...]
    td: Tuple[int, ...]
    ta: Tuple[int, ...]
    q_off: Tuple[int, ...]
    dc_off: Tuple[int, ...]
    ac_off: Tuple[int, ...]
    scan_off: int
    scan_len: int
    nbytes: int
    restart_interval: int = 0        # MCUs per restart interval, 0: none


def probe(data, restart=False):
    """JpegInfo of a file the decoder takes, or None: the file keeps the Pillow path.  `data`: bytes-like.  restart: also take a file with a
    restart interval and the restart markers that belong to it."""
    d = bytes(data)
    n = len(d)
    if n < 4 or n > MAX_FILE_BYTES or d[0:2] != b"\xff\xd8":
        return None
    q_off, dc_off, ac_off = [-1, -1], [-1, -1], [-1, -1]
    frame, jfif, adobe, ri = None, False, None, 0
    p = 2
    while True:
        if p + 4 > n or d[p] != 0xFF:
            return None
        m = d[p + 1]
        if m == 0xFF:                                                # fill byte
            p += 1
            continue
        L = (d[p + 2] << 8) | d[p + 3]
        if L < 2 or p + 2 + L > n:
            return None
        body, end = p + 4, p + 2 + L
        if m == 0xDB:
            q = body
            while q < end:
                if d[q] >> 4 != 0 or (d[q] & 15) > 1 or q + 65 > end:                     # 8-bit entries, tables 0 / 1
                    return None
                q_off[d[q] & 15] = q + 1
                q += 65
        elif m == 0xC4:
            q = body
            while q < end:
                if q + 17 > end or (d[q] >> 4) > 1 or (d[q] & 15) > 1:
                    return None
                cnt = sum(d[q + 1:q + 17])
                if cnt > 256 or q + 17 + cnt > end:
                    return None
                (ac_off if d[q] >> 4 else dc_off)[d[q] & 15] = q + 1
                q += 17 + cnt
        elif m == 0xC0:
            if frame is not None or L < 8:
                return None
            prec, H, W, nc = d[body], (d[body + 1] << 8) | d[body + 2], (d[body + 3] << 8) | d[body + 4], d[body + 5]
            if prec != 8 or nc not in (1, 3) or L != 8 + 3 * nc or H < 1 or W < 1 or H * W > MAX_PIXELS:
                return None
            comps = [(d[body + 6 + 3 * i], d[body + 7 + 3 * i] >> 4, d[body + 7 + 3 * i] & 15, d[body + 8 + 3 * i]) for i in range(nc)]
            frame = (H, W, comps)
        elif m == 0xDD:
            if L != 4:
                return None
            ri = (d[body] << 8) | d[body + 1]
            if ri and not restart:
                return None
        elif m == 0xE0:
            jfif = jfif or d[body:body + 5] == b"JFIF\x00"
        elif m == 0xEE:
            if d[body:body + 5] == b"Adobe" and L >= 14:
                adobe = d[body + 11]
        elif 0xE1 <= m <= 0xEF or m == 0xFE:
            pass
        elif m == 0xDA:
            break
        else:                                                        # SOF1.., DAC, DNL, RSTn, a second SOI, ...
            return None
        p = end
    if frame is None:
        return None
    H, W, comps = frame
    nc = len(comps)
    if L != 6 + 2 * nc or d[body] != nc or tuple(d[body + 1 + 2 * nc:body + 4 + 2 * nc]) != (0, 63, 0):
        return None
    td, ta, tq = [0] * 3, [0] * 3, [0] * 3
    for i, (cid, h, v, q) in enumerate(comps):
        if d[body + 1 + 2 * i] != cid:
            return None
        t = d[body + 2 + 2 * i]
        td[i], ta[i], tq[i] = t >> 4, t & 15, q
        if td[i] > 1 or ta[i] > 1 or q > 1 or dc_off[td[i]] < 0 or ac_off[ta[i]] < 0 or q_off[q] < 0:
            return None
    if nc == 1:
        if (comps[0][1], comps[0][2]) != (1, 1):
            return None
        hs, vs = 1, 1
    else:
        hs, vs = comps[0][1], comps[0][2]
        if (hs, vs) not in SAMPLINGS or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            return None
        if not jfif and (adobe is not None and adobe != 1):
            return None
        if not jfif and adobe is None and tuple(c[0] for c in comps) == (82, 71, 66):       # 'R' 'G' 'B': libjpeg takes these as RGB
            return None
    scan_off = end
    q = scan_off
    nrst = 0                                                         # restart markers met so far: the next one is RST(nrst & 7)
    want_rst = -(-(-(-H // (8 * vs)) * -(-W // (8 * hs))) // ri) - 1 if ri else 0
    while True:                                                      # the scan runs to EOI, or to the end of a cut file
        q = d.find(b"\xff", q)
        if q < 0 or q + 1 >= n:
            scan_len = n - scan_off
            break
        if d[q + 1] == 0:
            q += 2
            continue
        if d[q + 1] == 0xD0 + (nrst & 7) and nrst < want_rst:        # the restart marker that is due
            nrst += 1
            q += 2
            continue
        if d[q + 1] != 0xD9:                                         # an RSTn that is not due, a further scan, fill bytes
            return None
        scan_len = q - scan_off
        break
    if scan_len < 1 or nrst != want_rst:
        return None
    return JpegInfo(H, W, nc, hs, vs, tuple(tq), tuple(td), tuple(ta), tuple(q_off), tuple(dc_off), tuple(ac_off), scan_off, scan_len, n, ri)
