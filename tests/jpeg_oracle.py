"""Pure-numpy restatement of what the thumbnail path must reproduce (a helper, not a test; imports neither the product
nor Pillow):

  * libjpeg's baseline encoder as Pillow drives it (``Image.save(buf, "JPEG", quality=q)``: 4:2:0, Annex K Huffman tables,
    "islow" integer DCT, no restart markers): colour conversion, the two padding rules, chroma averaging, DCT,
    quantisation, dummy blocks, entropy coding, markers;
  * Pillow's antialiased bicubic ``Image.resize`` in its 8-bit integer form;
  * ``Image.thumbnail``'s size rule.

Everything is integer arithmetic except the resize tap tables, which are float64 as in Pillow's ``precompute_coeffs``.
"""
from __future__ import annotations

import math

import numpy as np

# ---- tables -------------------------------------------------------------------------------------------------------
STD_LUMA_Q = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
    103, 99], np.int64)
STD_CHROMA_Q = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
    + [99] * 32, np.int64)


def _zigzag():
    order = []
    for s in range(15):
        cells = [(y, s - y) for y in range(8) if 0 <= s - y < 8]
        order += cells if s % 2 else cells[::-1]
    return np.array([y * 8 + x for y, x in order], np.int64)


ZIGZAG = _zigzag()  # zigzag position -> natural (row-major) index

DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18,
    0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
    0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5,
    0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25,
    0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA,
    0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4,
    0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])


def huff_codes(bits, vals):
    """symbol -> (code, length) by the JPEG C.2 procedure."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


def quant_tables(quality: int):
    """libjpeg ``jpeg_set_quality(q, force_baseline=TRUE)`` -> (luma, chroma) int64[64] in natural order."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * scale + 50) // 100, 1, 255) for base in (STD_LUMA_Q, STD_CHROMA_Q))


# ---- encoder stages ----------------------------------------------------------------------------------------------
def ycbcr_planes(rgb: np.ndarray):
    """(h,w,3) uint8 RGB -> Y (padded to whole 8x8 blocks of its own size, then to the MCU rows) and the downsampled,
    padded Cb / Cr planes, int64, not yet level shifted."""
    h, w, _ = rgb.shape
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    mcu_rows = -(-h // 16)
    yw = -(-w // 8) * 8
    cw = -(-(-(-w // 2)) // 8) * 8

    def pad(p, rows, cols):
        return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")

    y = pad(y, mcu_rows * 16, yw)
    out = [y]
    for c in (cb, cr):
        c = pad(c, h + (h & 1), 2 * cw)  # rows only to an even count, columns to twice the padded chroma width
        bias = 1 + (np.arange(cw) & 1)
        d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias[None, :]) >> 2
        out.append(pad(d, mcu_rows * 8, cw))  # the downsampled rows are what gets replicated
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_pass(d, first: bool):
    """jfdctint.c, one pass over the last axis of d (..., 8)."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    sh = 13 - 2 if first else 13 + 2
    out = np.empty_like(d)
    if first:
        out[..., 0] = (t10 + t11) << 2
        out[..., 4] = (t10 - t11) << 2
    else:
        out[..., 0] = _descale(t10 + t11, 2)
        out[..., 4] = _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[..., 2] = _descale(z1 + t13 * 6270, sh)
    out[..., 6] = _descale(z1 - t12 * 15137, sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[..., 7] = _descale(t4 + z1 + z3, sh)
    out[..., 5] = _descale(t5 + z2 + z4, sh)
    out[..., 3] = _descale(t6 + z2 + z3, sh)
    out[..., 1] = _descale(t7 + z1 + z4, sh)
    return out


def fdct_quant(blocks: np.ndarray, q: np.ndarray) -> np.ndarray:
    """(..., 8, 8) samples (not level shifted) -> (..., 64) quantised coefficients in zigzag order."""
    d = blocks.astype(np.int64) - 128
    d = _dct_pass(d, True)                                   # rows
    d = _dct_pass(d.swapaxes(-1, -2), False).swapaxes(-1, -2)  # columns
    d = d.reshape(*d.shape[:-2], 64)
    qv = q.astype(np.int64) * 8
    mag = (np.abs(d) + (qv >> 1)) // qv
    return (np.sign(d) * mag)[..., ZIGZAG]


def coefficients(rgb: np.ndarray, quality: int) -> np.ndarray:
    """(h,w,3) uint8 RGB -> int16 (mcus, 6, 64): per 16x16 MCU in scan order the blocks Y00 Y01 Y10 Y11 Cb Cr, zigzag."""
    h, w, _ = rgb.shape
    ql, qc = quant_tables(quality)
    y, cb, cr = ycbcr_planes(rgb)
    my, mx = -(-h // 16), -(-w // 16)
    bw, bh = -(-w // 8), -(-h // 8)
    out = np.zeros((my, mx, 6, 64), np.int64)
    yb = np.pad(y, ((0, 0), (0, mx * 16 - y.shape[1])))  # columns past Y's own padding belong to dummy blocks only
    yb = fdct_quant(yb.reshape(my * 2, 8, mx * 2, 8).swapaxes(1, 2), ql)
    for s in range(4):
        out[:, :, s] = yb[s >> 1::2, s & 1::2]
    out[:, :, 4] = fdct_quant(cb.reshape(my, 8, mx, 8).swapaxes(1, 2), qc)
    out[:, :, 5] = fdct_quant(cr.reshape(my, 8, mx, 8).swapaxes(1, 2), qc)
    for j in range(my):
        for i in range(mx):
            for s in range(1, 4):
                if 2 * i + (s & 1) >= bw or 2 * j + (s >> 1) >= bh:  # dummy: DC of the block before it, no AC
                    out[j, i, s] = 0
                    out[j, i, s, 0] = out[j, i, s - 1, 0]
    return out.reshape(my * mx, 6, 64).astype(np.int16)


def _nbits(v: int) -> int:
    return int(abs(v)).bit_length()


def entropy_symbols(coef: np.ndarray):
    """The (bits, length) pairs of the scan, in order, plus whether a ZRL (run of 16 zeros) was emitted."""
    dc_t = (huff_codes(*DC_LUMA), huff_codes(*DC_CHROMA))
    ac_t = (huff_codes(*AC_LUMA), huff_codes(*AC_CHROMA))
    out, zrl = [], False
    last = [0, 0, 0]
    for mcu in coef.astype(np.int64):
        for s in range(6):
            comp = 0 if s < 4 else s - 3
            t = 0 if comp == 0 else 1
            blk = mcu[s]
            diff = int(blk[0]) - last[comp]
            last[comp] = int(blk[0])
            n = _nbits(diff)
            out.append(dc_t[t][n])
            if n:
                out.append(((diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n))
            run = 0
            for k in range(1, 64):
                v = int(blk[k])
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    out.append(ac_t[t][0xF0])
                    zrl = True
                    run -= 16
                n = _nbits(v)
                out.append(ac_t[t][(run << 4) + n])
                out.append(((v if v >= 0 else v - 1) & ((1 << n) - 1), n))
                run = 0
            if run:
                out.append(ac_t[t][0x00])
    return out, zrl


def bitstream_slow(coef: np.ndarray):
    """The literal restatement: -> (bytes of the unstuffed stream, the last byte zero padded; bit count; saw a ZRL)."""
    syms, zrl = entropy_symbols(coef)
    acc, n = 0, 0
    for bits, length in syms:
        acc = (acc << length) | bits
        n += length
    pad = -n % 8
    return (acc << pad).to_bytes((n + pad) // 8, "big"), n, zrl


def _table_arrays(spec):
    code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
    for sym, (c, n) in huff_codes(*spec).items():
        code[sym], length[sym] = c, n
    return code, length


def _bit_length(a):
    return np.frexp(a.astype(np.float64))[1].astype(np.int64)  # exact for the 12-bit magnitudes of a baseline scan


def bitstream(coef: np.ndarray):
    """``bitstream_slow`` with numpy doing the per-coefficient work (the two are compared in tests/test_thumbs_host.py):
    every code and every value field becomes a (bits, length) token keyed by (block, zigzag position, order within the
    position); the tokens are sorted and their bits packed."""
    blocks = coef.astype(np.int64).reshape(-1, 64)
    nb = len(blocks)
    slot = np.arange(nb) % 6
    chroma = (slot >= 4).astype(np.int64)
    dc_code = np.stack([_table_arrays(DC_LUMA)[0], _table_arrays(DC_CHROMA)[0]])
    dc_len = np.stack([_table_arrays(DC_LUMA)[1], _table_arrays(DC_CHROMA)[1]])
    ac_code = np.stack([_table_arrays(AC_LUMA)[0], _table_arrays(AC_CHROMA)[0]])
    ac_len = np.stack([_table_arrays(AC_LUMA)[1], _table_arrays(AC_CHROMA)[1]])
    diff = np.zeros(nb, np.int64)
    for sel in (slot < 4, slot == 4, slot == 5):  # the predictor is the previous block of the same component
        diff[sel] = np.diff(blocks[sel, 0], prepend=0)

    def value_bits(v, n):
        return np.where(v < 0, v - 1, v) & ((1 << n) - 1)

    toks = []  # (block, position, order, bits, length)
    n = _bit_length(np.abs(diff))
    b = np.arange(nb)
    toks.append((b, np.zeros(nb, np.int64), np.zeros(nb, np.int64), dc_code[chroma, n], dc_len[chroma, n]))
    has = n > 0
    toks.append((b[has], np.zeros(has.sum(), np.int64), np.ones(has.sum(), np.int64), value_bits(diff[has], n[has]), n[has]))
    bb, kk = np.nonzero(blocks[:, 1:])
    kk = kk + 1
    first = np.ones(len(bb), bool)
    first[1:] = bb[1:] != bb[:-1]
    prev = np.where(first, 0, np.concatenate([[0], kk[:-1]]))
    run = kk - prev - 1
    v = blocks[bb, kk]
    n = _bit_length(np.abs(v))
    zr = run // 16
    rep = np.repeat(np.arange(len(bb)), zr)
    toks.append((bb[rep], kk[rep], np.zeros(len(rep), np.int64), ac_code[chroma[bb[rep]], 0xF0], ac_len[chroma[bb[rep]], 0xF0]))
    sym = ((run % 16) << 4) + n
    toks.append((bb, kk, np.ones(len(bb), np.int64), ac_code[chroma[bb], sym], ac_len[chroma[bb], sym]))
    toks.append((bb, kk, np.full(len(bb), 2, np.int64), value_bits(v, n), n))
    eob = blocks[:, 63] == 0
    toks.append((b[eob], np.full(eob.sum(), 64, np.int64), np.zeros(eob.sum(), np.int64), ac_code[chroma[eob], 0], ac_len[chroma[eob], 0]))
    tb, tk, to, bits, length = (np.concatenate([t[i] for t in toks]) for i in range(5))
    order = np.lexsort((to, tk, tb))
    bits, length = bits[order], length[order]
    total = int(length.sum())
    start = np.cumsum(length) - length
    idx = np.repeat(np.arange(len(bits)), length)
    within = np.arange(total) - start[idx]
    stream = np.packbits(((bits[idx] >> (length[idx] - 1 - within)) & 1).astype(np.uint8)).tobytes()
    return stream, total, bool((zr > 0).any())


def _dht(cls_id: int, spec) -> bytes:
    bits, vals = spec
    return b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([cls_id]) + bytes(bits) + bytes(vals)


def jpeg_file(stream: bytes, nbits: int, w: int, h: int, quality: int) -> bytes:
    """Pad the last byte with 1-bits, stuff FF -> FF 00, and wrap in the markers Pillow writes (no dpi)."""
    data = bytearray(stream[: (nbits + 7) // 8])
    if nbits % 8:
        data[-1] |= (1 << (8 - nbits % 8)) - 1
    data = bytes(data).replace(b"\xff", b"\xff\x00")
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    for i, q in enumerate((ql, qc)):
        out += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(int(v) for v in q[ZIGZAG])
    out += b"\xff\xc0\x00\x11\x08" + h.to_bytes(2, "big") + w.to_bytes(2, "big") + b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01"
    out += _dht(0x00, DC_LUMA) + _dht(0x10, AC_LUMA) + _dht(0x01, DC_CHROMA) + _dht(0x11, AC_CHROMA)
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    return out + data + b"\xff\xd9"


def encode(rgb: np.ndarray, quality: int):
    """(h,w,3) uint8 RGB -> dict(coef, stream, nbits, zrl, file)."""
    rgb = np.asarray(rgb)
    coef = coefficients(rgb, quality)
    stream, nbits, zrl = bitstream(coef)
    return {"coef": coef, "stream": stream, "nbits": nbits, "zrl": zrl,
            "file": jpeg_file(stream, nbits, rgb.shape[1], rgb.shape[0], quality)}


# ---- Pillow's bicubic resize ------------------------------------------------------------------------------------
PRECISION_BITS = 22


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def bicubic_tables(in_size: int, out_size: int):
    """``precompute_coeffs`` + ``normalize_coeffs_8bpc``: (bounds int32 (out,2) = first input index | taps, k int32
    (out,ksize), ksize)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [float(_bicubic((x + xmin - center + 0.5) * ss)) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return bounds, kk, ksize


def _resample_axis1(img: np.ndarray, out_size: int) -> np.ndarray:
    """(rows, in, c) uint8 -> (rows, out, c) uint8 along axis 1."""
    bounds, kk, _ = bicubic_tables(img.shape[1], out_size)
    out = np.empty((img.shape[0], out_size, img.shape[2]), np.uint8)
    src = img.astype(np.int64)
    for xx in range(out_size):
        lo, n = (int(v) for v in bounds[xx])
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(src[:, lo:lo + n], kk[xx, :n].astype(np.int64), axes=([1], [0]))
        out[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_bicubic(rgb: np.ndarray, size) -> np.ndarray:
    """``Image.resize(size, BICUBIC)`` of an (h,w,3) uint8 image; size = (width, height).  Horizontal pass, 8-bit
    intermediate, vertical pass."""
    tw, th = size
    tmp = _resample_axis1(np.asarray(rgb), tw)
    return np.ascontiguousarray(_resample_axis1(tmp.swapaxes(0, 1), th).swapaxes(0, 1))


def thumbnail_size(w: int, h: int, box=(320, 180)):
    """The size ``Image.thumbnail(box)`` gives a w x h image (unchanged when it already fits)."""
    x, y = (math.floor(v) for v in box)
    if x >= w and y >= h:
        return w, h
    aspect = w / h

    def round_aspect(number, key):
        return max(min(math.floor(number), math.ceil(number), key=key), 1)

    if x / y >= aspect:
        x = round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    return x, y
