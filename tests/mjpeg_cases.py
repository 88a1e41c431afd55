"""The baseline JPEG files the Motion-JPEG tests decode (a helper, not a test).

256 cases: 8 sizes x 2 contents x 4 samplings x 4 encoder variants, plus the same files with their DHT segments removed
(AVI writers leave them out; the decoder falls back to the Annex K tables) and files with a restart marker after every MCU
row.  ``tests/golden/make_mjpeg_fixture.py`` encodes them with Pillow into ``tests/golden/mjpeg_pillow.npz``; the tests read
the bytes from there, so they need no Pillow.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "mjpeg_pillow.npz"

SIZES = [(1, 1), (8, 8), (16, 16), (17, 9), (15, 31), (33, 47), (40, 56), (94, 95)]  # (width, height)
CONTENTS = ["noise", "smooth"]
SAMPLINGS = ["444", "422", "420", "grey"]
VARIANTS = {  # Image.save(..., "JPEG", **options)
    "q75": {"quality": 75},
    "q100": {"quality": 100},
    "q20opt": {"quality": 20, "optimize": True},        # custom Huffman tables
    "q90rst": {"quality": 90, "restart_marker_blocks": 1},
    "q75rows": {"quality": 75, "restart_marker_rows": 1},
}
_SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def name_of(size, content, sampling, variant, stripped=False) -> str:
    return f"{size[0]}x{size[1]}-{content}-{sampling}-{variant}" + ("-nodht" if stripped else "")


def _all():
    encoded, stripped = [], []
    for size in SIZES:
        for content in CONTENTS:
            for sampling in SAMPLINGS:
                for variant in ("q75", "q100", "q20opt", "q90rst"):
                    encoded.append((size, content, sampling, variant))
    for size in ((33, 47), (94, 95)):
        for sampling in SAMPLINGS:
            encoded.append((size, "noise", sampling, "q75rows"))
    for size in SIZES:  # the standard tables are what a file without DHT means
        for sampling in SAMPLINGS:
            stripped.append((size, "noise", sampling, "q75"))
    return encoded, stripped


ENCODED, STRIPPED = _all()
NAMES = [name_of(*c) for c in ENCODED] + [name_of(*c, stripped=True) for c in STRIPPED]
# the cases whose Pillow pixels are committed: every sampling and every variant, at two sizes that are no multiple of an MCU
WITH_PIXELS = [name_of(*c) for c in ENCODED if c[0] in ((17, 9), (33, 47)) and c[1] == "noise"]


def image(size, content, sampling) -> np.ndarray:
    """The uint8 source image of a case: (h, w, 3) RGB, or (h, w) for ``grey``."""
    w, h = size
    rng = np.random.default_rng(1000 * w + h)
    if content == "noise":
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 255) // max(w + h - 2, 1)], -1).astype(np.uint8)
    return img[..., 1].copy() if sampling == "grey" else img


def save_options(sampling, variant) -> dict:
    opts = dict(VARIANTS[variant])
    if sampling != "grey":
        opts["subsampling"] = _SUBSAMPLING[sampling]
    return opts


def strip_dht(data: bytes) -> bytes:
    """The file without its DHT segments (only the marker segments before SOS are walked)."""
    out, pos = [data[:2]], 2
    while True:
        m = data[pos + 1]
        n = int.from_bytes(data[pos + 2:pos + 4], "big")
        if m != 0xC4:
            out.append(data[pos:pos + 2 + n])
        pos += 2 + n
        if m == 0xDA:
            return b"".join(out) + data[pos:]


def _chunk(cc: bytes, body: bytes) -> bytes:
    return cc + len(body).to_bytes(4, "little") + body + (b"\0" if len(body) & 1 else b"")


def _list(kind: bytes, body: bytes, cc: bytes = b"LIST") -> bytes:
    return cc + (4 + len(body)).to_bytes(4, "little") + kind + body


def avi_bytes(frames, rate=30000, scale=1001, width=0, height=0, fourcc=b"MJPG", awkward=False) -> bytes:
    """A small AVI writer.  ``frames``: JPEG files; ``None`` writes a zero-length video chunk (a dropped frame).  No ``idx1``.
    ``awkward`` adds what real files have: a second (audio) stream with interleaved odd-sized ``01wb`` chunks, a ``JUNK``
    chunk, a ``LIST 'rec '`` group around the second frame, and the last two frames in a second ``RIFF 'AVIX'``."""
    import struct

    n = len(frames)
    avih = struct.pack("<14I", scale * 1000000 // rate, 0, 0, 0x10, n, 0, 2 if awkward else 1, 0, width, height, 0, 0, 0, 0)
    strh = b"vids" + fourcc + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, scale, rate, 0, n, 0, 0xFFFFFFFF, 0, 0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, fourcc, width * height * 3, 0, 0, 0, 0)
    hdrl = _chunk(b"avih", avih) + _list(b"strl", _chunk(b"strh", strh) + _chunk(b"strf", strf))
    if awkward:
        auds = b"auds" + b"\0\0\0\0" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, 1, 8000, 0, 0, 0, 0, 1, 0, 0, 0, 0)
        hdrl += _list(b"strl", _chunk(b"strh", auds) + _chunk(b"strf", struct.pack("<HHIIHH", 1, 1, 8000, 8000, 1, 8)))
        hdrl += _chunk(b"JUNK", b"\x55" * 5)
    video = [_chunk(b"00dc", f or b"") for f in frames]
    if not awkward:
        return _list(b"AVI ", _list(b"hdrl", hdrl) + _list(b"movi", b"".join(video)), b"RIFF")
    audio = _chunk(b"01wb", b"\x80\x81\x82")
    head, tail = video[:-2], video[-2:]
    body = b"".join(v + audio if i != 1 else _list(b"rec ", v + audio) for i, v in enumerate(head))
    first = _list(b"AVI ", _list(b"hdrl", hdrl) + _chunk(b"JUNK", b"\0" * 7) + _list(b"movi", body), b"RIFF")
    return first + _list(b"AVIX", _list(b"movi", b"".join(tail)), b"RIFF")


_files = None


def files() -> dict:
    """name -> JPEG bytes, for every name in ``NAMES``."""
    global _files
    if _files is None:
        with np.load(GOLDEN) as z:
            _files = {n: z["jpeg/" + n].tobytes() for n in NAMES if "jpeg/" + n in z.files}
        for c in STRIPPED:
            _files[name_of(*c, stripped=True)] = strip_dht(_files[name_of(*c)])
    return _files


def pillow_pixels() -> dict:
    """name -> the pixels Pillow decoded when the fixture was made (RGB, or L for ``grey``)."""
    with np.load(GOLDEN) as z:
        return {n: z["pixels/" + n] for n in WITH_PIXELS}


_oracle = {}


def oracle(name: str) -> dict:
    """The oracle's coefficients and RGB / luma pixels of a case, computed once per process."""
    if name not in _oracle:
        import jpeg_decode_oracle as jd

        data = files()[name]
        coef, status = jd.coefficients(data)
        _oracle[name] = {"coef": coef, "status": status, "rgb": jd.decode(data, "rgb", coef), "luma": jd.decode(data, "luma", coef)}
    return _oracle[name]
