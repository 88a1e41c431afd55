"""Pure-numpy restatement of libjpeg's default baseline decode, which the Motion-JPEG path (K28) must reproduce bit for bit
(a helper, not a test; imports neither the product nor Pillow):

  * marker parsing, Huffman decoding (one symbol at a time, as ``csrc/jpeg_entropy.h`` defines the step) and DC prediction;
  * dequantisation and the ``jidctint.c`` "islow" IDCT (CONST_BITS 13, PASS1_BITS 2, descale by 11 then 18, +128, clamp);
  * ``jdsample.c`` fancy upsampling (h2v1 / h2v2; plain replication when the chroma plane is at most 2 samples wide, which
    is libjpeg's own choice) and ``jdcolor.c`` YCbCr -> RGB with SCALEBITS 16;
  * the fixed-point iteration that synchronises decoders started at arbitrary bits, so round counts can be compared.

Everything is integer arithmetic.
"""
from __future__ import annotations

import functools

import numpy as np

from jpeg_oracle import AC_CHROMA, AC_LUMA, DC_CHROMA, DC_LUMA, ZIGZAG

STD_DHT = {(0, 0): DC_LUMA, (0, 1): DC_CHROMA, (1, 0): AC_LUMA, (1, 1): AC_CHROMA}  # (class, id) -> (counts, symbols)


# ---- markers -------------------------------------------------------------------------------------------------------
def parse(data: bytes) -> dict:
    """One baseline JPEG file -> its tables, geometry and unstuffed restart segments."""
    assert data[:2] == b"\xff\xd8", "no SOI"
    pos, qt, dht, ri, sof, sos = 2, {}, {}, 0, None, None
    while True:
        assert data[pos] == 0xFF, f"no marker at byte {pos}"
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        n = int.from_bytes(data[pos + 2:pos + 4], "big")
        body = data[pos + 4:pos + 2 + n]
        if m == 0xDB:
            while body:
                assert body[0] >> 4 == 0, "16-bit DQT"
                q = np.zeros(64, np.int64)
                q[ZIGZAG] = np.frombuffer(body[1:65], np.uint8)
                qt[body[0] & 15] = q
                body = body[65:]
        elif m == 0xC4:
            while body:
                counts = list(body[1:17])
                k = sum(counts)
                dht[(body[0] >> 4, body[0] & 15)] = (counts, list(body[17:17 + k]))
                body = body[17 + k:]
        elif m == 0xC0:
            sof = body
        elif m == 0xDD:
            ri = int.from_bytes(body[:2], "big")
        elif m == 0xDA:
            sos = body
            pos += 2 + n
            break
        else:
            assert m not in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF), f"frame type {m:#x}"
        pos += 2 + n
    assert sof[0] == 8
    h, w, nc = int.from_bytes(sof[1:3], "big"), int.from_bytes(sof[3:5], "big"), sof[5]
    comps = [(sof[6 + 3 * i], sof[7 + 3 * i] >> 4, sof[7 + 3 * i] & 15, sof[8 + 3 * i]) for i in range(nc)]
    assert sos[0] == nc
    sel = {sos[1 + 2 * i]: (sos[2 + 2 * i] >> 4, sos[2 + 2 * i] & 15) for i in range(nc)}
    end = pos
    while True:  # the scan ends at the first marker that is neither a stuffed FF nor a restart
        end = data.index(b"\xff", end)
        if data[end + 1] == 0 or 0xD0 <= data[end + 1] <= 0xD7:
            end += 2
            continue
        break
    raw, pieces, start, i = data[pos:end], [], 0, 0
    while True:
        i = raw.find(b"\xff", i)
        if i < 0:
            break
        if 0xD0 <= raw[i + 1] <= 0xD7:
            pieces.append(raw[start:i])
            start = i + 2
        i += 2
    pieces.append(raw[start:])
    hs, vs = comps[0][1], comps[0][2]
    for key, spec in STD_DHT.items():
        dht.setdefault(key, spec)
    return {"h": h, "w": w, "ncomp": nc, "hs": hs, "vs": vs, "qt": qt, "dht": dht, "ri": ri,
            "comps": [(tq, *sel[cid]) for cid, _, _, tq in comps],  # per component: quant, DC, AC table ids
            "segments": [p.replace(b"\xff\x00", b"\xff") for p in pieces]}


def geometry(p: dict) -> dict:
    hs, vs = p["hs"], p["vs"]
    mcux, mcuy = -(-p["w"] // (8 * hs)), -(-p["h"] // (8 * vs))
    bpm = 1 if p["ncomp"] == 1 else hs * vs + 2
    return {"mcux": mcux, "mcuy": mcuy, "bpm": bpm, "blocks": mcux * mcuy * bpm,
            "comp_of": [0] * (hs * vs) + ([1, 2] if p["ncomp"] == 3 else [])}


def segment_mcus(p: dict):
    """[(first MCU, MCU count)] of the restart segments."""
    g = geometry(p)
    total = g["mcux"] * g["mcuy"]
    ri = p["ri"] or total
    out = [(a, min(ri, total - a)) for a in range(0, total, ri)]
    assert len(out) == len(p["segments"]), f"{len(p['segments'])} segments for {len(out)} restart intervals"
    return out


# ---- entropy -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def _lut(counts: tuple, symbols: tuple):
    """16-bit prefix -> length << 8 | symbol (0: no code)."""
    lut = np.zeros(1 << 16, np.int64)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            lut[code << (16 - length):(code + 1) << (16 - length)] = length << 8 | symbols[k]
            code += 1
            k += 1
        code <<= 1
    return lut.tolist()


def _windows(seg: bytes):
    """The 32 bits at every bit position of a segment (zeros past its end), as a list."""
    b = np.concatenate([np.frombuffer(seg, np.uint8), np.zeros(8, np.uint8)]).astype(np.uint64)
    five = (b[:-4] << np.uint64(32)) | (b[1:-3] << np.uint64(24)) | (b[2:-2] << np.uint64(16)) | (b[3:-1] << np.uint64(8)) | b[4:]
    p = np.arange(8 * len(seg) + 1)
    return ((five[p >> 3] >> (8 - (p & 7)).astype(np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.int64).tolist()


def _extend(v: int, n: int) -> int:
    return 0 if n == 0 else (v - (1 << n) + 1 if v < (1 << (n - 1)) else v)


class _Tables:
    def __init__(self, p: dict):
        g = geometry(p)
        self.bpm = g["bpm"]
        self.dc = [_lut(tuple(p["dht"][(0, p["comps"][c][1])][0]), tuple(p["dht"][(0, p["comps"][c][1])][1])) for c in g["comp_of"]]
        self.ac = [_lut(tuple(p["dht"][(1, p["comps"][c][2])][0]), tuple(p["dht"][(1, p["comps"][c][2])][1])) for c in g["comp_of"]]


def run(t: _Tables, win: list, nbits: int, stop: int, state, sink=None):
    """``jpeg_entropy::run``: from ``state = (p, b, z)`` to the first symbol boundary at or past ``stop``; returns the new
    state and the number of blocks closed.  ``sink(kind, z, value)`` hears "dc" / "ac" / "close"."""
    p, b, z = state
    stop = min(stop, nbits)
    closed = 0
    while p < stop:
        bits = win[p]
        e = (t.dc[b] if z == 0 else t.ac[b])[bits >> 16]
        used = 1
        if e:
            length, sym = e >> 8, e & 255
            n, r = sym & 15, (0 if z == 0 else sym >> 4)
            v = ((bits << length) & 0xFFFFFFFF) >> (32 - n) if n else 0
            used = length + n
            close = False
            if z == 0:
                if sink:
                    sink("dc", 0, _extend(v, n))
                z = 1
            elif n == 0:
                if r == 15:
                    z += 16
                else:
                    close = True
            else:
                z += r
                if z < 64 and sink:
                    sink("ac", z, _extend(v, n))
                z += 1
            if close or z >= 64:
                if sink:
                    sink("close", 0, 0)
                closed += 1
                z = 0
                b = 0 if b + 1 >= t.bpm else b + 1
        p = nbits if nbits - p <= used else p + used
    return (p, b, z), closed


def coefficients(data: bytes) -> tuple[np.ndarray, int]:
    """-> (int16 (blocks, 64) in natural order, DC predicted; blocks in scan order), status (1: a segment ran short)."""
    p = parse(data)
    g, t = geometry(p), _Tables(p)
    out = np.zeros((g["blocks"], 64), np.int64)
    status = 0
    for seg, (first, count) in zip(p["segments"], segment_mcus(p)):
        owned, base = count * g["bpm"], first * g["bpm"]
        ord_ = [0]

        def sink(kind, z, v):
            if kind == "close":
                ord_[0] += 1
            elif ord_[0] < owned:
                out[base + ord_[0], ZIGZAG[z]] = v

        _, closed = run(t, _windows(seg), 8 * len(seg), 8 * len(seg), (0, 0, 0), sink)
        status |= closed < owned
        for c in range(p["ncomp"]):  # the predictor is 0 at every restart
            idx = [base + m * g["bpm"] + k for m in range(count) for k, cc in enumerate(g["comp_of"]) if cc == c]
            out[idx, 0] = np.cumsum(out[idx, 0])
    return out.astype(np.int16), int(status)


def sync_rounds(files, S: int) -> int:
    """The number of rounds, over all segments of all files at once, in which the fixed-point iteration of K28 decodes a
    subsequence: round 1 decodes every subsequence (subsequence i > 0 of a segment from the guess (i S, 0, 0)); each later
    round decodes those whose entry state -- the left neighbour's exit state of the round before -- changed."""
    segs = []
    for data in files:
        p = parse(data)
        t = _Tables(p)
        segs += [(t, _windows(s), 8 * len(s)) for s in p["segments"]]
    state = []
    for t, win, nbits in segs:
        n = max(1, -(-nbits // S))
        entry = [(i * S, 0, 0) for i in range(n)]
        state.append([entry, [None] * n, [None] * n])  # entry, the entry last decoded from, exit
    rounds = 0
    while True:
        decoded = False
        for (t, win, nbits), (entry, last, exit_) in zip(segs, state):
            for i, e in enumerate(entry):
                if last[i] != e:
                    exit_[i], last[i] = run(t, win, nbits, (i + 1) * S, e)[0], e
                    decoded = True
        if not decoded:
            return rounds
        rounds += 1
        for entry, _, exit_ in state:
            entry[1:] = exit_[:-1]


# ---- pixels --------------------------------------------------------------------------------------------------------
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_pass(d, shift):
    """jidctint.c, one pass over the last axis of d (..., 8)."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    z1 = (d2 + d6) * 4433
    e2, e3 = z1 + d6 * -15137, z1 + d2 * 6270
    e0, e1 = (d0 + d4) << 13, (d0 - d4) << 13
    t10, t13, t11, t12 = e0 + e3, e0 - e3, e1 + e2, e1 - e2
    t0, t1, t2, t3 = d7, d5, d3, d1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    return np.stack([_descale(t10 + t3, shift), _descale(t11 + t2, shift), _descale(t12 + t1, shift), _descale(t13 + t0, shift),
                     _descale(t13 - t0, shift), _descale(t12 - t1, shift), _descale(t11 - t2, shift), _descale(t10 - t3, shift)], -1)


def idct(coef: np.ndarray, q: np.ndarray) -> np.ndarray:
    """(n, 64) coefficients and a (64,) table, natural order -> (n, 8, 8) samples."""
    d = (coef.astype(np.int64) * q.astype(np.int64)).reshape(-1, 8, 8)
    d = _idct_pass(d.swapaxes(-1, -2), 11).swapaxes(-1, -2)  # columns
    return np.clip(_idct_pass(d, 18) + 128, 0, 255)


def planes(data: bytes, coef: np.ndarray | None = None):
    """-> the component planes at their real sizes (Y: h x w; chroma: the downsampled size, rounded up)."""
    p = parse(data)
    g = geometry(p)
    if coef is None:
        coef = coefficients(data)[0]
    hs, vs, mcux, mcuy, bpm = p["hs"], p["vs"], g["mcux"], g["mcuy"], g["bpm"]
    blocks = coef.reshape(mcuy, mcux, bpm, 64)
    out = []
    for c in range(p["ncomp"]):
        q = p["qt"][p["comps"][c][0]]
        ch, cv = (hs, vs) if c == 0 else (1, 1)
        first = 0 if c == 0 else hs * vs + c - 1
        s = idct(blocks[:, :, first:first + ch * cv].reshape(-1, 64), q).reshape(mcuy, mcux, cv, ch, 8, 8)
        plane = s.transpose(0, 2, 4, 1, 3, 5).reshape(mcuy * cv * 8, mcux * ch * 8)
        ph, pw = -(-p["h"] * cv // vs), -(-p["w"] * ch // hs)
        out.append(plane[:ph, :pw])
    return p, out


def _upsample(c: np.ndarray, hs: int, vs: int, h: int, w: int) -> np.ndarray:
    if hs == 1:
        return c
    dh, dw = c.shape
    if dw <= 2:  # libjpeg: do_fancy_upsampling wants downsampled_width > 2, else plain replication
        return np.repeat(np.repeat(c, vs, 0), 2, 1)[:h, :w]
    left, right = np.maximum(np.arange(dw) - 1, 0), np.minimum(np.arange(dw) + 1, dw - 1)
    if vs == 1:
        out = np.empty((dh, 2 * dw), np.int64)
        out[:, 0::2] = (3 * c + c[:, left] + 1) >> 2
        out[:, 1::2] = (3 * c + c[:, right] + 2) >> 2
        return out[:h, :w]
    out = np.empty((2 * dh, 2 * dw), np.int64)
    for par, far in ((0, c[np.maximum(np.arange(dh) - 1, 0)]), (1, c[np.minimum(np.arange(dh) + 1, dh - 1)])):
        s = 3 * c + far
        out[par::2, 0::2] = (3 * s + s[:, left] + 8) >> 4
        out[par::2, 1::2] = (3 * s + s[:, right] + 7) >> 4
    return out[:h, :w]


def decode(data: bytes, fmt: str = "rgb", coef: np.ndarray | None = None) -> np.ndarray:
    """-> uint8 (h, w, 3) for "rgb" / "bgr" (a one-component file repeats Y), (h, w) for "luma"."""
    p, pl = planes(data, coef)
    y = pl[0]
    if fmt == "luma":
        return y.astype(np.uint8)
    if p["ncomp"] == 1:
        return np.repeat(y[..., None], 3, -1).astype(np.uint8)
    cb, cr = (_upsample(c, p["hs"], p["vs"], p["h"], p["w"]) - 128 for c in pl[1:])
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    rgb = np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
    return rgb if fmt == "rgb" else np.ascontiguousarray(rgb[..., ::-1])
