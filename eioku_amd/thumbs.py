"""Scene thumbnails on the HIP kernels of ``csrc/thumbs.hip`` (K18): the ``thumbnail_generation`` stage.

The reference's design schedules a thumbnail worker behind scene detection and shows one thumbnail per matching scene
(``.kiro/specs/semantic-video-search/design.md:276-297, 931``); the CPU way is ``Image.thumbnail`` + ``Image.save(...,
"JPEG")`` on a frame pulled back over PCIe.  Here the frame stays in HBM: Pillow's antialiased bicubic resize (8-bit
integer form) and libjpeg's baseline 4:2:0 encoder (colour conversion, padding, chroma averaging, "islow" DCT,
quantisation, Huffman coding) run on the device and only the coded bits come back.  The host builds the tap and
quantisation tables, pads and byte-stuffs the stream and writes the markers.  Every stage is integer arithmetic: the
files are the bytes ``Image.resize((tw, th), BICUBIC).save(buf, "JPEG", quality=q)`` writes.  One stated deviation from
``Image.thumbnail``: its ``reducing_gap`` / JPEG-draft pre-reduction is not applied (that is ``reducing_gap=None``).
No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._buffers import current_stream, on_device, ptr
from ._handle import Handle

PRECISION_BITS = 22  # Pillow Resample.c: 32 - 8 - 2 for 8-bit pixels
MAX_SIDE = 1024      # per thumbnail side (eioku_thumbs_*)
MAX_BATCH = 64       # images per call


# ---- size rule and resize tables ---------------------------------------------------------------------------------
def thumbnail_size(w: int, h: int, box=(320, 180)) -> tuple[int, int]:
    """The ``(width, height)`` ``Image.thumbnail(box)`` gives a ``w x h`` image (its ``preserve_aspect_ratio`` rule);
    an image that already fits keeps its size."""
    x, y = (math.floor(v) for v in box)
    if x >= w and y >= h:
        return int(w), int(h)
    aspect = w / h

    def round_aspect(number, key):
        return max(min(math.floor(number), math.ceil(number), key=key), 1)

    if x / y >= aspect:
        x = round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    return x, y


def _triangle(x):
    return np.where(x < 1.0, 1.0 - x, 0.0)


def _bicubic(x, a=-0.5):
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1,
                    np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


_FILTERS = {"bilinear": (_triangle, 1.0), "bicubic": (_bicubic, 2.0)}


def resample_tables(in_size: int, out_size: int, filter: str = "bicubic"):
    """Pillow ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` (float64, as Pillow computes them) for one axis
    ``in_size`` -> ``out_size``: ``(bounds int32 (out,2) = first input index | taps, k int32 (out,ksize) taps x 2**22,
    ksize)``.  The sibling of ``places.resize_tables`` for any of Pillow's filters with negative lobes: a tap rounds as
    ``(int)(-0.5 + v)`` below zero and ``(int)(0.5 + v)`` otherwise."""
    fn, fsupport = _FILTERS[filter]
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = fsupport * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    xx = np.arange(out_size, dtype=np.float64)
    center = (xx + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)  # C (int) cast: truncation toward zero
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.float64)[None, :]
    w = fn(np.abs((x + xmin[:, None] - center[:, None] + 0.5) * (1.0 / filterscale)))
    outside = x >= xmax[:, None]
    w[outside] = 0.0
    ww = np.zeros(out_size, np.float64)
    for t in range(ksize):  # Pillow sums the taps in index order
        ww = ww + w[:, t]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    v = w * (1 << PRECISION_BITS)
    k = np.where(w < 0, -0.5 + v, 0.5 + v).astype(np.int64)
    k[outside] = 0
    bounds = np.stack([xmin, xmax], 1).astype(np.int32)
    return np.ascontiguousarray(bounds), np.ascontiguousarray(k.astype(np.int32)), ksize


def bicubic_tables(in_size: int, out_size: int):
    """``resample_tables`` for ``Resampling.BICUBIC`` (what ``Image.thumbnail`` resizes with)."""
    return resample_tables(in_size, out_size, "bicubic")


# ---- JPEG tables and file assembly -------------------------------------------------------------------------------
_STD_LUMA_Q = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
               80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
               95, 98, 112, 100, 103, 99)
_STD_CHROMA_Q = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
                 99, 99) + (99,) * 32


def _zigzag_order():
    order = []
    for s in range(15):
        cells = [(y, s - y) for y in range(8) if 0 <= s - y < 8]
        order += cells if s % 2 else cells[::-1]
    return np.array([y * 8 + x for y, x in order], np.int64)


_ZIGZAG = _zigzag_order()  # zigzag position -> natural index

# Annex K (ITU-T T.81 K.3) Huffman tables as DHT payloads: 16 code-length counts, then the symbols
_DC_LUMA = bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]) + bytes(range(12))
_DC_CHROMA = bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]) + bytes(range(12))
_AC_LUMA = bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]) + bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA = bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]) + bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")


def jpeg_tables(quality: int = 75):
    """libjpeg ``jpeg_quality_scaling`` + ``jpeg_add_quant_table(..., force_baseline=TRUE)``: the (luma, chroma)
    quantisation tables of ``quality`` as one uint16 ``(2, 64)`` array in natural (row-major) order, each 1..255."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    base = np.array([_STD_LUMA_Q, _STD_CHROMA_Q], np.int64)
    return np.ascontiguousarray(np.clip((base * scale + 50) // 100, 1, 255).astype(np.uint16))


def jpeg_file(bitstream, nbits: int, tw: int, th: int, quality: int = 75) -> bytes:
    """The entropy-coded bits of one ``tw x th`` 4:2:0 baseline scan -> the file Pillow writes: the last byte padded with
    1-bits, ``FF`` stuffed to ``FF 00``, between SOI, APP0 JFIF (no dpi: unit 0, density 1 x 1), two DQT, SOF0, four DHT
    (DC0, AC0, DC1, AC1), SOS and EOI."""
    data = bytearray(bytes(bitstream)[: (nbits + 7) // 8])
    if len(data) != (nbits + 7) // 8:
        raise ValueError(f"bitstream of {len(data)} bytes for {nbits} bits")
    if nbits % 8:
        data[-1] |= (1 << (8 - nbits % 8)) - 1
    body = bytes(data).replace(b"\xff", b"\xff\x00")
    tab = jpeg_tables(quality)
    out = [b"\xff\xd8", b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"]
    for i in range(2):
        out.append(b"\xff\xdb\x00\x43" + bytes([i]) + bytes(tab[i][_ZIGZAG].astype(np.uint8)))
    out.append(b"\xff\xc0\x00\x11\x08" + int(th).to_bytes(2, "big") + int(tw).to_bytes(2, "big")
               + b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01")
    for cls_id, payload in ((0x00, _DC_LUMA), (0x10, _AC_LUMA), (0x01, _DC_CHROMA), (0x11, _AC_CHROMA)):
        out.append(b"\xff\xc4" + (3 + len(payload)).to_bytes(2, "big") + bytes([cls_id]) + payload)
    out.append(b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00")
    out.append(body)
    out.append(b"\xff\xd9")
    return b"".join(out)


# ---- the encoder ---------------------------------------------------------------------------------------------------
class ThumbnailEncoder:
    """``im.thumbnail(size, reducing_gap=None); im.save(buf, "JPEG", quality=quality)`` for batches of BGR frames, on the
    device.  ``size`` is the bounding box ``(width, height)``; a frame that fits inside it keeps its size."""

    def __init__(self, size=(320, 180), quality: int = 75):
        self.size = (int(size[0]), int(size[1]))
        self.quality = int(quality)
        self._tables = {}
        self._h = Handle("thumbs")

    def _device(self, x):
        import torch

        if on_device(x):
            return x.contiguous()
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint8)).to(torch.device("cuda", torch.cuda.current_device()))

    def _tab(self, h: int, w: int, th: int, tw: int):
        key = (h, w, th, tw)
        if key not in self._tables:
            self._tables[key] = (*bicubic_tables(w, tw), *bicubic_tables(h, th))
        return self._tables[key]

    def resize(self, frames_bgr, size):
        """BGR uint8 ``(n,h,w,3)`` (numpy or CUDA tensor) -> RGB uint8 ``(n,th,tw,3)`` CUDA tensor:
        ``Image.resize(size, BICUBIC)`` with ``size = (tw, th)``."""
        import torch

        n, h, w, c = (int(s) for s in frames_bgr.shape)
        if c != 3:
            raise ValueError("expected (n,h,w,3) BGR frames")
        tw, th = int(size[0]), int(size[1])
        src = self._device(frames_bgr)
        out = torch.empty((n, max(th, 0), max(tw, 0), 3), dtype=torch.uint8, device=src.device)
        if 1 <= tw <= MAX_SIDE and 1 <= th <= MAX_SIDE:
            xb, xk, kx, yb, yk, ky = self._tab(h, w, th, tw)
        else:  # the library refuses the size before it reads a table
            xb = xk = yb = yk = np.zeros((1, 2), np.int32)
            kx = ky = 1
        _lib.check(self._h.eioku_thumbs_resize(ptr(src), n, h, w, th, tw, ptr(xb), ptr(xk), kx, ptr(yb), ptr(yk), ky,
                                               ptr(out), current_stream(src)), "eioku_thumbs_resize")
        return out

    def jpeg(self, rgb, quality: int | None = None, with_coef: bool = False):
        """RGB uint8 ``(n,th,tw,3)`` (numpy or CUDA tensor) -> ``(streams, nbits[, coef])``: per image the entropy-coded
        bytes (unpadded, unstuffed; unused trailing bits 0) and their bit count; ``coef`` int16 ``(n, mcus, 6, 64)``."""
        n, th, tw, c = (int(s) for s in rgb.shape)
        if c != 3:
            raise ValueError("expected (n,th,tw,3) RGB images")
        src = self._device(rgb)
        qtab = jpeg_tables(self.quality if quality is None else quality)
        nbits = np.zeros(max(n, 1), np.uint32)
        total = C.c_uint64(0)
        coef = np.empty((n, -(-th // 16) * -(-tw // 16), 6, 64), np.int16) if with_coef else None
        _lib.check(self._h.eioku_thumbs_jpeg(ptr(src), n, th, tw, ptr(qtab), ptr(coef), ptr(nbits), C.byref(total),
                                             current_stream(src)), "eioku_thumbs_jpeg")
        packed = np.empty(max(total.value, 1), np.uint8)
        _lib.check(self._h.eioku_thumbs_read(ptr(packed), total.value, current_stream(src)), "eioku_thumbs_read")
        streams, pos = [], 0
        for i in range(n):
            nb = int(nbits[i])
            streams.append(packed[pos:pos + (nb + 7) // 8].tobytes())
            pos += (nb + 31) // 32 * 4
        nbits = [int(v) for v in nbits[:n]]
        return (streams, nbits, coef) if with_coef else (streams, nbits)

    def encode(self, frames_bgr) -> list[bytes]:
        """BGR uint8 ``(n,h,w,3)`` (numpy array or CUDA tensor) -> one JPEG file per frame."""
        n, h, w, _ = (int(s) for s in frames_bgr.shape)
        tw, th = thumbnail_size(w, h, self.size)
        files = []
        for lo in range(0, n, MAX_BATCH):
            rgb = self.resize(frames_bgr[lo:lo + MAX_BATCH], (tw, th))
            streams, nbits = self.jpeg(rgb)
            files += [jpeg_file(s, b, tw, th, self.quality) for s, b in zip(streams, nbits)]
        return files

    def last_ms(self) -> dict:
        """Device milliseconds of the last resize, block stage, entropy stage and bitstream read."""
        ms = np.zeros(4, np.float64)
        _lib.check(self._h.eioku_thumbs_last_ms(ptr(ms)), "eioku_thumbs_last_ms")
        return dict(zip(("resize", "blocks", "entropy", "d2h"), (float(v) for v in ms)))

    def close(self):
        self._h.close()


# ---- which frame, which segment -----------------------------------------------------------------------------------
def _timestamp_ms(frame_idx: int, fps) -> int:
    return int((frame_idx / fps) * 1000)  # the frame loops' timestamp (model_manager._timestamp_ms)


def scene_frame_index(scene: dict, fps, total_frames: int, position: str = "start") -> int:
    """The frame a scene's thumbnail is taken from: the first frame whose timestamp (``int(idx / fps * 1000)``, as every
    frame loop stamps it) is at least ``start_ms`` (``"start"``) or ``(start_ms + end_ms) // 2`` (``"middle"``), clamped
    to the last frame."""
    if position not in ("start", "middle"):
        raise ValueError(f"unknown position {position!r}")
    target = int(scene["start_ms"]) if position == "start" else (int(scene["start_ms"]) + int(scene["end_ms"])) // 2
    idx = max(0, int(target * fps / 1000.0))
    while idx > 0 and _timestamp_ms(idx - 1, fps) >= target:
        idx -= 1
    while _timestamp_ms(idx, fps) < target:
        idx += 1
    return max(0, min(idx, int(total_frames) - 1))


def _segment_start_ms(seg: dict) -> int:
    return int(seg["start_ms"]) if "start_ms" in seg else int(float(seg.get("start", 0.0)) * 1000)


def assign_thumbnails(segments: list[dict], thumbnails: list[dict]) -> list[dict]:
    """Transcript segments with ``thumbnail_path`` set to the thumbnail of the scene whose span ``[start_ms, end_ms)``
    contains the segment's start; if none does, the nearest scene that starts earlier, else the first.  New dicts are
    returned; ``embed_segments`` / ``index_transcript`` carry the path into the store's metadata and the search results."""
    rows = sorted(thumbnails, key=lambda r: (int(r["start_ms"]), int(r["end_ms"])))
    out = []
    for seg in segments:
        seg = dict(seg)
        if rows:
            t = _segment_start_ms(seg)
            inside = [r for r in rows if int(r["start_ms"]) <= t < int(r["end_ms"])]
            earlier = [r for r in rows if int(r["start_ms"]) <= t]
            seg["thumbnail_path"] = (inside[0] if inside else earlier[-1] if earlier else rows[0])["thumbnail_path"]
        out.append(seg)
    return out
