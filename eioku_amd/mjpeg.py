"""Motion-JPEG on the HIP kernels of ``csrc/mjpeg.hip`` (K28): AVI / raw MJPEG / JPEG stills from file bytes to BGR in HBM.

The host does what is sequential and small: it walks the RIFF tree of an AVI file chunk by chunk (``idx1`` is not
trusted; OpenDML ``AVIX`` parts, ``LIST rec`` groups, pad bytes, ``JUNK`` and other streams' chunks are stepped over),
reads each sampled frame's JPEG markers (SOF0, DQT, DHT, DRI, SOS), cuts the entropy-coded data at the restart markers
and removes the byte stuffing -- all of it through ``bytes`` / ``re`` calls, never per byte or per coefficient in Python.
The device does the rest: Huffman decoding with one thread per S-bit subsequence and a fixed-point synchronisation of the
decoder states, DC prediction, dequantisation, the "islow" IDCT, fancy upsampling and colour conversion.  The pixels are
bit for bit what libjpeg-turbo, and therefore Pillow, decodes (``cv2``'s FFmpeg backend uses ffmpeg's own IDCT and
swscale and can differ by a few code values).  No decoded pixel crosses PCIe unless the caller asks
for a host array, and a frame that is skipped (``grab``) is never read from the file.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import json
import re
import struct
from pathlib import Path

import numpy as np

from . import _lib
from ._buffers import ptr
from ._handle import Handle
from .frames import FrameSource
from .thumbs import _AC_CHROMA, _AC_LUMA, _DC_CHROMA, _DC_LUMA, _ZIGZAG

MAX_SIDE = 8192
DEFAULT_SUBSEQ_BITS = 512  # kDefaultSubseqBits of csrc/mjpeg.hip: the fastest measured size (profiles/mjpeg.json)
FORMATS = {"bgr": 0, "rgb": 1, "luma": 2}
EXTENSIONS = (".avi", ".mjpeg", ".mjpg", ".jpg", ".jpeg")

_HUFF_BYTES = 16 + 256
_SOF_NAMES = {0xC1: "SOF1 (extended sequential)", 0xC2: "SOF2 (progressive)", 0xC3: "SOF3 (lossless)", 0xC5: "SOF5", 0xC6: "SOF6",
              0xC7: "SOF7", 0xC9: "SOF9 (arithmetic coding)", 0xCA: "SOF10 (arithmetic coding)", 0xCB: "SOF11 (arithmetic coding)",
              0xCD: "SOF13 (arithmetic coding)", 0xCE: "SOF14 (arithmetic coding)", 0xCF: "SOF15 (arithmetic coding)"}
_SCAN_END = re.compile(rb"\xff[^\x00\xd0-\xd7\xff]")  # the first marker that is neither stuffing nor a restart
_RESTART = re.compile(rb"\xff[\xd0-\xd7]")  # a literal first byte keeps the search at memchr speed


class UnsupportedJpeg(RuntimeError):
    """The file is a JPEG, but not one K28 decodes; the message names the rule."""


def _std_huff() -> np.ndarray:
    t = np.zeros((4, _HUFF_BYTES), np.uint8)
    for i, payload in enumerate((_DC_LUMA, _DC_CHROMA, _AC_LUMA, _AC_CHROMA)):
        t[i, :len(payload)] = np.frombuffer(payload, np.uint8)
    return t


_STD_HUFF = _std_huff()  # Annex K: what a frame without DHT segments (AVI writers leave them out) is coded with


class ParsedFrame:
    """One baseline JPEG, ready for the device: geometry, tables and unstuffed restart segments."""

    __slots__ = ("h", "w", "ncomp", "hs", "vs", "qtab", "huff", "comp", "pieces", "mcus_per_piece")

    @property
    def geometry(self):
        return (self.h, self.w, self.ncomp, self.hs, self.vs)


def parse_jpeg(data, what: str = "JPEG") -> ParsedFrame:
    """Read the markers of one baseline JPEG (``bytes``-like).  ``UnsupportedJpeg`` says which rule a file breaks."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise UnsupportedJpeg(f"{what}: no SOI marker (not a JPEG)")
    qtab = np.ones((4, 64), np.uint16)
    have_q = set()
    huff = _STD_HUFF.copy()
    ri, sof, adobe_transform, pos, n_data = 0, None, None, 2, len(data)
    while True:
        if pos + 4 > n_data:
            raise UnsupportedJpeg(f"{what}: the markers end before SOS")
        if data[pos] != 0xFF:
            raise UnsupportedJpeg(f"{what}: no marker at byte {pos}")
        m = data[pos + 1]
        if m == 0xFF:  # fill byte
            pos += 1
            continue
        if m in _SOF_NAMES:
            kind = "arithmetic coding is not supported" if "arithmetic" in _SOF_NAMES[m] else "only baseline SOF0 is decoded"
            raise UnsupportedJpeg(f"{what}: frame type {_SOF_NAMES[m]}: {kind}")
        if m == 0xCC:
            raise UnsupportedJpeg(f"{what}: DAC marker: arithmetic coding is not supported")
        n = int.from_bytes(data[pos + 2:pos + 4], "big")
        body = data[pos + 4:pos + 2 + n]
        if n < 2 or len(body) != n - 2:
            raise UnsupportedJpeg(f"{what}: marker {m:#04x} at byte {pos} runs past the end")
        if m == 0xDB:
            while body:
                if body[0] >> 4:
                    raise UnsupportedJpeg(f"{what}: 16-bit DQT table {body[0] & 15}: only 8-bit tables are decoded")
                if (body[0] & 15) > 3 or len(body) < 65:
                    raise UnsupportedJpeg(f"{what}: bad DQT segment")
                qtab[body[0] & 15, _ZIGZAG] = np.frombuffer(body[1:65], np.uint8)
                have_q.add(body[0] & 15)
                body = body[65:]
        elif m == 0xC4:
            while body:
                cls, tid = body[0] >> 4, body[0] & 15
                k = sum(body[1:17])
                if cls > 1 or tid > 1 or k > 256 or len(body) < 17 + k:
                    raise UnsupportedJpeg(f"{what}: DHT class {cls} id {tid}: baseline has tables 0 and 1 of each class")
                row = huff[cls * 2 + tid]
                row[:] = 0
                row[:17 + k - 1] = np.frombuffer(body[1:17 + k], np.uint8)
                body = body[17 + k:]
        elif m == 0xC0:
            sof = body
        elif m == 0xDD:
            ri = int.from_bytes(body[:2], "big")
        elif m == 0xE0 and body[:4] == b"AVI1" and len(body) > 4 and body[4] != 0:
            raise UnsupportedJpeg(f"{what}: AVI1 field polarity {body[4]}: interlaced Motion-JPEG is not supported")
        elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe_transform = body[11]
        elif m == 0xDA:
            sos = body
            pos += 2 + n
            break
        pos += 2 + n
    if sof is None:
        raise UnsupportedJpeg(f"{what}: SOS before SOF0")
    if sof[0] != 8:
        raise UnsupportedJpeg(f"{what}: {sof[0]}-bit samples: only 8-bit is decoded")
    f = ParsedFrame()
    f.h, f.w, f.ncomp = int.from_bytes(sof[1:3], "big"), int.from_bytes(sof[3:5], "big"), sof[5]
    if not (1 <= f.h <= MAX_SIDE and 1 <= f.w <= MAX_SIDE):
        raise UnsupportedJpeg(f"{what}: {f.w} x {f.h}: width and height must be in [1, {MAX_SIDE}]")
    if f.ncomp not in (1, 3):
        raise UnsupportedJpeg(f"{what}: {f.ncomp} components: 1 or 3 are decoded")
    comps = [(sof[6 + 3 * i], sof[7 + 3 * i] >> 4, sof[7 + 3 * i] & 15, sof[8 + 3 * i]) for i in range(f.ncomp)]
    sampling = [(c[1], c[2]) for c in comps]
    if f.ncomp == 1:
        sampling = [(1, 1)]  # a single component is not interleaved: its sampling factors do not matter
    if sampling[0] not in ((1, 1), (2, 1), (2, 2)) or any(s != (1, 1) for s in sampling[1:]):
        raise UnsupportedJpeg(f"{what}: sampling {'/'.join(f'{a}x{b}' for a, b in sampling)}: luma 1x1, 2x1 or 2x2 with 1x1 chroma")
    if f.ncomp == 3 and adobe_transform is not None and adobe_transform != 1:
        raise UnsupportedJpeg(f"{what}: Adobe APP14 transform {adobe_transform}: only YCbCr (transform 1) is decoded")
    f.hs, f.vs = sampling[0]
    if sos[0] != f.ncomp:
        raise UnsupportedJpeg(f"{what}: a scan of {sos[0]} of {f.ncomp} components: multiple scans are not supported")
    if bytes(sos[1 + 2 * f.ncomp:4 + 2 * f.ncomp]) != b"\x00\x3f\x00":
        raise UnsupportedJpeg(f"{what}: spectral selection / successive approximation in SOS: not a baseline scan")
    f.comp = np.zeros((3, 3), np.uint8)
    for i, (cid, _, _, tq) in enumerate(comps):
        if sos[1 + 2 * i] != cid:
            raise UnsupportedJpeg(f"{what}: scan component {sos[1 + 2 * i]} where the frame has {cid}")
        td, ta = sos[2 + 2 * i] >> 4, sos[2 + 2 * i] & 15
        if tq > 3 or tq not in have_q or td > 1 or ta > 1:
            raise UnsupportedJpeg(f"{what}: component {cid} uses tables DQT {tq}, DC {td}, AC {ta} (missing, or not baseline)")
        f.comp[i] = (tq, td, ta)
    f.qtab, f.huff = qtab, huff
    end = _SCAN_END.search(data, pos)
    if end is not None and data[end.start() + 1] != 0xD9:
        raise UnsupportedJpeg(f"{what}: marker {data[end.start() + 1]:#04x} after the scan: multiple scans are not supported")
    raw = data[pos:end.start() if end else n_data]  # a frame without EOI (a cut recording) ends with its bytes
    mcus = -(-f.w // (8 * f.hs)) * -(-f.h // (8 * f.vs))
    per = ri or mcus
    f.pieces = [p.replace(b"\xff\x00", b"\xff") for p in (_RESTART.split(raw) if ri else [raw])]
    if len(f.pieces) != -(-mcus // per):
        raise UnsupportedJpeg(f"{what}: {len(f.pieces)} restart segments for {-(-mcus // per)} restart intervals")
    f.mcus_per_piece = per
    return f


def pack(frames: list) -> tuple:
    """``ParsedFrame`` list -> the call's buffers: entropy bytes (every segment on a 4-byte boundary), segment table
    uint32 ``(nseg, 5)`` = frame, first MCU, MCU count, byte offset, bit length; quant / Huffman / selector tables."""
    chunks, rows, off = [], [], 0
    for i, f in enumerate(frames):
        mcus = -(-f.w // (8 * f.hs)) * -(-f.h // (8 * f.vs))
        for k, piece in enumerate(f.pieces):
            first = k * f.mcus_per_piece
            rows.append((i, first, min(f.mcus_per_piece, mcus - first), off, 8 * len(piece)))
            pad = -len(piece) % 4
            chunks.append(piece)
            if pad:
                chunks.append(bytes(pad))
            off += len(piece) + pad
    n = len(frames)
    entropy = np.frombuffer(b"".join(chunks) or bytes(4), np.uint8)
    if entropy.size == 0:
        entropy = np.zeros(4, np.uint8)
    seg = np.array(rows, np.uint32).reshape(-1, 5)
    qtab = np.ascontiguousarray(np.stack([f.qtab for f in frames])) if n else np.zeros((0, 4, 64), np.uint16)
    huff = np.ascontiguousarray(np.stack([f.huff for f in frames])) if n else np.zeros((0, 4, _HUFF_BYTES), np.uint8)
    comp = np.ascontiguousarray(np.stack([f.comp for f in frames])) if n else np.zeros((0, 3, 3), np.uint8)
    return entropy, seg, qtab, huff, comp


class MjpegDecoder:
    """Batches of baseline JPEG frames of one geometry -> device tensors.  The geometry (h, w, components, sampling) is
    fixed by the first frame; a later frame that departs from it fails the call."""

    def __init__(self, subseq_bits: int | None = None):
        self._h = Handle("mjpeg")
        self.geometry = None
        if subseq_bits is not None:
            self.set_subseq_bits(subseq_bits)

    def set_subseq_bits(self, bits: int) -> None:
        """The size S of the subsequences one thread decodes: a multiple of 32 in [32, 4096].  Results do not depend on it."""
        _lib.check(self._h.eioku_mjpeg_set_subseq_bits(int(bits)), "eioku_mjpeg_set_subseq_bits")

    def set_batch_frames(self, frames: int) -> None:
        """Frames per internal sub-batch (0: as many as the coefficient budget holds).  Results do not depend on it."""
        _lib.check(self._h.eioku_mjpeg_set_batch_frames(int(frames)), "eioku_mjpeg_set_batch_frames")

    def _prepare(self, frames):
        parsed = [f if isinstance(f, ParsedFrame) else parse_jpeg(f, f"frame {i}") for i, f in enumerate(frames)]
        for i, f in enumerate(parsed):
            if self.geometry is None:
                self.geometry = f.geometry
            if f.geometry != self.geometry:
                raise RuntimeError(f"frame {i}: geometry (h, w, components, sampling) {f.geometry} departs from the source's "
                                   f"{self.geometry}")
        return parsed, pack(parsed)

    @staticmethod
    def _check_status(status):
        bad = np.flatnonzero(status)
        if bad.size:
            raise RuntimeError(f"frame {int(bad[0])}: the entropy-coded data ends before the frame's last block "
                               f"({bad.size} damaged frame(s) in the call)")

    def decode(self, frames, fmt: str = "bgr", device=None):
        """``frames``: JPEG files (``bytes``) or ``ParsedFrame``s -> CUDA uint8 tensor ``(n, h, w, 3)`` for ``"bgr"`` /
        ``"rgb"``, ``(n, h, w)`` for ``"luma"`` (the decoded Y plane)."""
        import torch

        if fmt not in FORMATS:
            raise ValueError(f"unknown format {fmt!r}")
        parsed, (entropy, seg, qtab, huff, comp) = self._prepare(frames)
        n = len(parsed)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if n == 0:
            return torch.empty((0,), dtype=torch.uint8, device=dev)
        h, w, ncomp, hs, vs = self.geometry
        out = torch.empty((n, h, w) if fmt == "luma" else (n, h, w, 3), dtype=torch.uint8, device=dev)
        status = np.zeros(n, np.int32)
        _lib.check(self._h.eioku_mjpeg_decode(ptr(entropy), entropy.size, ptr(seg), len(seg), ptr(qtab), ptr(huff), ptr(comp), n, h, w,
                                              ncomp, hs, vs, FORMATS[fmt], ptr(out), ptr(status),
                                              torch.cuda.current_stream(dev).cuda_stream), "eioku_mjpeg_decode")
        self._check_status(status)
        return out

    def coefficients(self, frames) -> np.ndarray:
        """The entropy stage alone: int16 ``(n, blocks, 64)`` in natural order, DC predicted, blocks in scan order."""
        parsed, (entropy, seg, qtab, huff, comp) = self._prepare(frames)
        n = len(parsed)
        h, w, ncomp, hs, vs = self.geometry
        blocks = -(-w // (8 * hs)) * -(-h // (8 * vs)) * (1 if ncomp == 1 else hs * vs + 2)
        coef = np.zeros((n, blocks, 64), np.int16)
        status = np.zeros(max(n, 1), np.int32)
        _lib.check(self._h.eioku_mjpeg_coefficients(ptr(entropy), entropy.size, ptr(seg), len(seg), ptr(qtab), ptr(huff), ptr(comp), n, h,
                                                    w, ncomp, hs, vs, ptr(coef), ptr(status), None), "eioku_mjpeg_coefficients")
        self._check_status(status[:n])
        return coef

    def last(self) -> dict:
        """Device milliseconds per stage and the synchronisation rounds of the last call."""
        ms = np.zeros(5, np.float64)
        rounds = C.c_int(0)
        _lib.check(self._h.eioku_mjpeg_last(ptr(ms), C.byref(rounds)), "eioku_mjpeg_last")
        return dict(zip(("upload", "sync", "write", "idct", "colour"), (float(v) for v in ms)), rounds=rounds.value)

    def close(self):
        self._h.close()


# ---- containers ----------------------------------------------------------------------------------------------------
_MJPEG_FOURCCS = (b"MJPG", b"JPEG")


class NotMjpeg(RuntimeError):
    """An AVI file whose video stream is not Motion-JPEG (``open_video`` hands it to the next decoder)."""


def parse_avi(f, size: int) -> dict:
    """Walk the RIFF tree of an AVI file object chunk by chunk -> ``{"scale", "rate", "width", "height", "frames":
    [(offset, size)]}`` of the first video stream, which must be Motion-JPEG.  Only chunk headers and the three header
    chunks' bodies are read; ``idx1`` is ignored.  A zero-length video chunk repeats the frame before it."""
    info = {"stream": None, "frames": [], "n_strl": 0, "fourcc": None}

    def walk(pos, end, in_movi):
        while pos + 8 <= end:
            f.seek(pos)
            head = f.read(8)
            if len(head) < 8:
                return
            cc, n = head[:4], struct.unpack("<I", head[4:])[0]
            body_end = min(pos + 8 + n, end)
            if cc in (b"RIFF", b"LIST"):
                kind = f.read(4)
                if kind in (b"AVI ", b"AVIX", b"hdrl", b"strl", b"movi", b"rec "):
                    if kind == b"strl":
                        info["cur"] = info["n_strl"]
                        info["n_strl"] += 1
                    walk(pos + 12, body_end, in_movi or kind == b"movi")
            elif cc == b"strh" and "cur" in info:
                b = f.read(56)
                if len(b) >= 32 and b[0:4] == b"vids" and info["stream"] is None and "pending" not in info:
                    info["pending"] = (info["cur"], b[4:8], struct.unpack("<II", b[20:28]))
            elif cc == b"strf" and info.get("pending", (None,))[0] == info.get("cur"):
                b = f.read(40)
                cur, handler, (scale, rate) = info.pop("pending")
                comp = b[16:20] if len(b) >= 20 else b""
                info["fourcc"] = comp if comp.strip(b"\0 ") else handler
                if handler.upper() in _MJPEG_FOURCCS or comp.upper() in _MJPEG_FOURCCS:
                    w, h = struct.unpack("<ii", b[4:12])
                    info.update(stream=cur, scale=scale, rate=rate, width=abs(w), height=abs(h))
                else:
                    info["stream"] = -1  # the first video stream is something else
            elif in_movi and info["stream"] is not None and info["stream"] >= 0 and cc[2:] in (b"dc", b"db") \
                    and cc[:2] == b"%02d" % info["stream"]:
                if n == 0:  # AVI's dropped-frame rule
                    if not info["frames"]:
                        raise RuntimeError("the AVI stream begins with a zero-length (dropped) frame")
                    info["frames"].append(info["frames"][-1])
                else:
                    info["frames"].append((pos + 8, body_end - pos - 8))
            pos += 8 + n + (n & 1)

    pos = 0
    while pos + 12 <= size:  # RIFF 'AVI ', then any RIFF 'AVIX'
        f.seek(pos)
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] not in (b"AVI ", b"AVIX"):
            if pos == 0:
                raise NotMjpeg("not a RIFF AVI file")
            break
        n = struct.unpack("<I", head[4:8])[0]
        walk(pos + 12, min(pos + 8 + n, size), False)
        pos += 8 + n + (n & 1)
    if info["stream"] is None or info["stream"] < 0:
        cc = info["fourcc"]
        raise NotMjpeg("no video stream" if cc is None else f"video stream codec {cc.decode('latin-1')!r} is not Motion-JPEG")
    if not info["rate"] or not info["scale"]:
        raise RuntimeError("the AVI stream header has a zero rate or scale")
    return info


def _jpeg_spans(buf) -> list:
    """(offset, size) of the concatenated JPEG files in a raw MJPEG stream: from each SOI, marker by marker to SOS, then to
    the EOI that ends the scan data."""
    spans, pos, n = [], 0, len(buf)
    while True:
        pos = buf.find(b"\xff\xd8", pos)
        if pos < 0:
            return spans
        q = pos + 2
        while q + 4 <= n and buf[q] == 0xFF:
            m = buf[q + 1]
            if m == 0xFF:
                q += 1
                continue
            q += 2 + int.from_bytes(buf[q + 2:q + 4], "big")
            if m == 0xDA:
                break
        end = buf.find(b"\xff\xd9", q)
        end = n if end < 0 else end + 2
        spans.append((pos, end - pos))
        pos = end


class MjpegSource(FrameSource):
    """Motion-JPEG in AVI (``.avi``), raw concatenated JPEGs (``.mjpeg`` / ``.mjpg``; fps from a ``<file>.json`` sidecar as
    for ``.npy`` clips, else 25) or one still (``.jpg`` / ``.jpeg``) behind the ``cv2.VideoCapture`` look-alike.

    ``grab()`` advances without touching a frame's bytes.  ``read()`` decodes one frame on the device and returns a host
    BGR array, so every frame loop works unchanged; ``read_encoded()`` returns the frame's bytes instead, for loops that
    collect a batch and call ``decoder.decode(batch)`` once, keeping the pixels in HBM.  ``luma_planes`` is the decoded Y
    plane (what ffmpeg's ``select`` filter scores for a ``yuvj420p`` stream)."""

    def __init__(self, path, file=None):
        self.path = str(path)
        self._f = file if file is not None else open(self.path, "rb")
        self._f.seek(0, 2)
        size = self._f.tell()
        if self.path.lower().endswith(".avi"):
            try:
                info = parse_avi(self._f, size)
            except BaseException:
                if file is None:
                    self._f.close()
                raise
            self._frames = info["frames"]
            self.time_base = (int(info["scale"]), int(info["rate"]))
            self.fps = info["rate"] / info["scale"]
        else:
            self._f.seek(0)
            buf = self._f.read()
            self._frames = _jpeg_spans(buf)
            if not self._frames:
                raise RuntimeError(f"{self.path!r}: no JPEG frame found")
            meta = {}
            side = Path(self.path + ".json")
            if side.exists():
                meta = json.loads(side.read_text())
            self.fps = float(meta.get("fps", 25.0))
            from .frames import _fps_to_time_base

            self.time_base = tuple(meta.get("time_base", _fps_to_time_base(self.fps)))
        self.total_frames = len(self._frames)
        self.duration_s = self.total_frames * self.time_base[0] / self.time_base[1]
        self.pos = 0
        self._decoder = None

    @property
    def decoder(self) -> MjpegDecoder:
        if self._decoder is None:
            self._decoder = MjpegDecoder()
        return self._decoder

    def frame_bytes(self, index: int) -> bytes:
        off, n = self._frames[index]
        self._f.seek(off)
        return self._f.read(n)

    def grab(self):
        if self.pos >= self.total_frames:
            return False
        self.pos += 1
        return True

    def read_encoded(self):
        """``(ok, JPEG bytes of the next frame)``; the position advances as with ``read``."""
        if self.pos >= self.total_frames:
            return False, None
        data = self.frame_bytes(self.pos)
        self.pos += 1
        return True, data

    def decode(self, encoded: list, fmt: str = "bgr"):
        """One device decode call for a batch of ``read_encoded`` frames -> CUDA uint8 ``(n, h, w, 3)`` (or ``(n, h, w)``)."""
        return self.decoder.decode(encoded, fmt)

    def read(self):
        ok, data = self.read_encoded()
        if not ok:
            return False, None
        return True, self.decoder.decode([data], "bgr")[0].cpu().numpy()

    def luma_planes_device(self, start, count):
        """``luma_planes`` as a CUDA tensor: one decode call, and the planes stay in HBM."""
        from .frames import EndOfStream

        stop = min(start + count, self.total_frames)
        if stop <= start:
            raise EndOfStream(f"{self.path!r}: no frame at index {start}")
        return self.decoder.decode([self.frame_bytes(i) for i in range(start, stop)], "luma")

    def luma_planes(self, start, count):
        return self.luma_planes_device(start, count).cpu().numpy()

    def release(self):
        if self._decoder is not None:
            self._decoder.close()
            self._decoder = None
        if self._f is not None:
            self._f.close()
            self._f = None


def open_mjpeg(path):
    """``MjpegSource`` for a path with one of ``EXTENSIONS``; ``None`` for an ``.avi`` whose video is not Motion-JPEG, and for
    a path that is no readable local file (``cv2`` also takes URLs and device names): the caller goes on as before."""
    try:
        return MjpegSource(path)
    except OSError:
        return None
    except NotMjpeg:
        if str(path).lower().endswith(".avi"):
            return None
        raise
