"""Audio front end on the HIP path (K23): PCM of any sample rate, width and channel count -> 16 kHz mono float32.

The reference hands the file to faster-whisper, which decodes and resamples to 16 kHz mono itself; this module is that step
for PCM audio: :func:`read_pcm` (a RIFF parser that also reads float and ``WAVE_FORMAT_EXTENSIBLE`` files),
:func:`filter_bank` (the taps, designed here in float64) and :class:`AudioFrontEnd` (decode, downmix and the polyphase
resampler in ``csrc/audio.hip``).

The resampler is ``scipy.signal.resample_poly(x, 16000, rate)`` with its default window (Kaiser, beta 5), restated here so
that scipy is no dependency.  faster-whisper resamples with libswresample through PyAV; the difference is listed in
INTEGRATION.md §3.  Compressed audio and container demuxing stay outside this path.
"""
from __future__ import annotations

import ctypes as C
import math
import struct
from pathlib import Path

import numpy as np

from ._handle import Handle

SAMPLE_RATE = 16000
MAX_TAPS = 14336             # 56 KiB of fp32: bank and a tile's input share 64 KiB of LDS
MAX_CHANNELS = 8
DEFAULT_SLAB_OUT = 1 << 22   # output samples per device slab (4.4 minutes; 16 MB out, 50 MB of 48 kHz stereo s16 in)
FORMATS = {"u8": (0, 1), "s16": (1, 2), "s24": (2, 3), "s32": (3, 4), "f32": (4, 4)}   # name -> (library code, bytes)
PLAN_KEYS = ("out_start", "n_out", "first_frame", "frames", "lead", "trail", "phase")


# ---- the filter -------------------------------------------------------------------------------------------------------------
def resample_ratio(rate) -> tuple[int, int]:
    """``(up, down)`` with ``up / down = 16000 / rate`` in lowest terms; ``ValueError`` for a rate that is not a positive
    integer or whose filter has more than :data:`MAX_TAPS` taps."""
    if isinstance(rate, bool) or not isinstance(rate, (int, np.integer)) or rate <= 0:
        raise ValueError(f"sample rate must be a positive integer, got {rate!r}")
    rate = int(rate)
    g = math.gcd(rate, SAMPLE_RATE)
    up, down = SAMPLE_RATE // g, rate // g
    taps = 20 * max(up, down) + 1
    if up != down and taps > MAX_TAPS:
        raise ValueError(f"audio is {rate} Hz: resampling to {SAMPLE_RATE} Hz takes {taps} taps, more than {MAX_TAPS}")
    if up != down and kernel_tile(up, down) == 0:
        raise ValueError(f"audio is {rate} Hz: the bank of {taps} taps and the input of one tile do not fit 64 KiB of LDS")
    return up, down


def kernel_tile(up: int, down: int) -> int:
    """Outputs per workgroup tile, as ``eioku_audio_create`` picks it: the largest of 256, 128, 64, 32 whose input span fits
    the LDS next to the bank; 0 when none does (rates above 2.5 MHz)."""
    T = -(-(20 * max(up, down) + 1) // up)
    for tile in (256, 128, 64, 32):
        if up * T + (up - 1 + (tile - 1) * down) // up + T <= 16384:
            return tile
    return 0


def _geometry(rate) -> tuple[int, int, int, int]:
    """``(up, down, half, T)``; the passthrough is ``(1, 1, 0, 1)``."""
    up, down = resample_ratio(rate)
    if up == down:
        return 1, 1, 0, 1
    half = 10 * max(up, down)
    return up, down, half, -(-(2 * half + 1) // up)


def filter_taps(rate) -> np.ndarray:
    """The ``2 * half + 1`` taps in float64: a windowed sinc with cutoff ``1 / max(up, down)`` under a Kaiser window of beta 5,
    normalised to sum 1 and scaled by ``up`` (``scipy.signal.firwin(L, 1 / m, window=("kaiser", 5.0)) * up``)."""
    up, down = resample_ratio(rate)
    m = max(up, down)
    half = 10 * m
    k = np.arange(2 * half + 1, dtype=np.float64) - half
    h = (1.0 / m) * np.sinc(k / m) * np.i0(5.0 * np.sqrt(1.0 - (k / half) ** 2)) / np.i0(5.0)
    return h / h.sum() * up


def filter_bank(rate) -> np.ndarray:
    """``B[p][q] = float32(h[p + q * up])``, zero from the last tap on: float32 ``[up][ceil(L / up)]``."""
    up, down = resample_ratio(rate)
    h = filter_taps(rate)
    T = -(-h.size // up)
    padded = np.zeros(up * T, dtype=np.float64)
    padded[:h.size] = h
    return np.ascontiguousarray(padded.reshape(T, up).T.astype(np.float32))


def output_length(n_frames: int, rate) -> int:
    up, down = resample_ratio(rate)
    return -(-int(n_frames) * up // down)


def plan_slabs(n_frames: int, rate, slab_out: int = DEFAULT_SLAB_OUT) -> list[dict]:
    """The slabs in which a file of ``n_frames`` is resampled, as ``eioku_audio_resample`` walks them.  Per slab:
    ``out_start`` / ``n_out`` (its outputs), ``first_frame`` / ``frames`` (the input it reads), ``lead`` / ``trail`` (zero
    frames in front of and behind that input: the filter reaches past both ends of the file) and ``phase`` (``t mod up`` of
    its first output, ``t = n * down + half``).  Absolute positions are Python integers; ``slab_out`` is clamped so that
    every slab-relative position (``phase + n * down`` and the frames the filter reaches) stays below 2^31."""
    up, down, half, T = _geometry(rate)
    n_frames, slab_out = int(n_frames), int(slab_out)
    if n_frames < 0 or slab_out < 1:
        raise ValueError(f"n_frames {n_frames} / slab_out {slab_out} out of range")
    total = -(-n_frames * up // down)
    eff = min(slab_out, (2 ** 31 - 1 - up - T * up) // down)
    slabs = []
    for n0 in range(0, total, eff):
        cnt = min(eff, total - n0)
        t0, t1 = n0 * down + half, (n0 + cnt - 1) * down + half
        lo, hi = t0 // up - (T - 1), t1 // up + 1
        first = min(max(lo, 0), n_frames)
        frames = max(min(hi, n_frames) - first, 0)
        slabs.append({"out_start": n0, "n_out": cnt, "first_frame": first, "frames": frames, "lead": first - lo,
                      "trail": (hi - lo) - (first - lo) - frames, "phase": t0 % up})
    return slabs


# ---- RIFF / WAVE ------------------------------------------------------------------------------------------------------------
def _pcm_format(tag: int, bits: int, path) -> str:
    if tag == 1 and bits in (8, 16, 24, 32):
        return {8: "u8", 16: "s16", 24: "s24", 32: "s32"}[bits]
    if tag == 3 and bits == 32:
        return "f32"
    raise ValueError(f"{path}: format tag 0x{tag:04X} with {bits} bits per sample is not read "
                     "(PCM of 8, 16, 24 or 32 bits and 32-bit float are)")


def read_pcm(path: str | Path) -> tuple[np.ndarray, str, int, int, int]:
    """A WAVE file's samples, undecoded: ``(raw bytes as uint8, format, channels, rate, frames)`` with ``format`` one of
    :data:`FORMATS`.  Reads format tags 1 (PCM), 3 (float) and 0xFFFE (extensible: the tag is the start of the sub-format);
    skips other chunks, with the pad byte after an odd size; takes a ``data`` size of 0 or 0xFFFFFFFF (a piped encoder that
    could not seek back) or one past the end of the file as "to the end of the file"; drops a truncated last frame."""
    path = Path(path)
    size = path.stat().st_size
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError(f"{path}: not a RIFF/WAVE file")
        fmt = None
        pos = 12
        while True:
            f.seek(pos)
            chunk = f.read(8)
            if len(chunk) < 8:
                raise ValueError(f"{path}: no data chunk")
            cid, csize = chunk[:4], struct.unpack("<I", chunk[4:])[0]
            pos += 8
            if cid == b"fmt ":
                body = f.read(min(csize, 40))
                if len(body) < 16:
                    raise ValueError(f"{path}: fmt chunk of {len(body)} bytes")
                tag, channels, rate, _, _, bits = struct.unpack("<HHIIHH", body[:16])
                if tag == 0xFFFE:
                    if len(body) < 26:
                        raise ValueError(f"{path}: extensible fmt chunk of {len(body)} bytes")
                    tag = struct.unpack("<H", body[24:26])[0]
                fmt = (tag, channels, rate, bits)
            elif cid == b"data":
                break
            pos += csize + (csize & 1)
        if fmt is None:
            raise ValueError(f"{path}: data chunk before the fmt chunk")
        tag, channels, rate, bits = fmt
        name = _pcm_format(tag, bits, path)
        if not 1 <= channels <= MAX_CHANNELS:
            raise ValueError(f"{path}: {channels} channels, outside 1..{MAX_CHANNELS}")
        if rate <= 0:
            raise ValueError(f"{path}: sample rate {rate}")
        left = size - pos
        nbytes = left if csize in (0, 0xFFFFFFFF) or csize > left else csize
        frame = FORMATS[name][1] * channels
        frames = nbytes // frame
        f.seek(pos)
        raw = np.fromfile(f, dtype=np.uint8, count=frames * frame)
    return raw, name, channels, rate, frames


# ---- the device stage -------------------------------------------------------------------------------------------------------
def check_pcm(fmt, channels, rate) -> tuple[int, int, int, int]:
    """``(library code, bytes per frame, up, down)`` or ``ValueError``, before any device work."""
    up, down = resample_ratio(rate)
    if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)) or not 1 <= channels <= MAX_CHANNELS:
        raise ValueError(f"channels must be an integer in 1..{MAX_CHANNELS}, got {channels!r}")
    if fmt not in FORMATS:
        raise ValueError(f"unknown PCM format {fmt!r}; known: {tuple(FORMATS)}")
    code, width = FORMATS[fmt]
    return code, width * int(channels), up, down


class AudioFrontEnd:
    """Decode, downmix and resample to 16 kHz on the device.  One library handle per ``(up, down)``, built on first use and
    kept until :meth:`close`.  ``slab_out`` bounds device memory; the result does not depend on it."""

    def __init__(self, *, slab_out: int = DEFAULT_SLAB_OUT):
        self.slab_out = int(slab_out)
        if not 1 <= self.slab_out <= 1 << 26:
            raise ValueError(f"slab_out must be in 1..2^26, got {slab_out!r}")
        self._handles: dict[tuple[int, int], Handle] = {}
        self._last = None
        self.lib = None  # the library is loaded with the first handle, not before

    def _handle(self, rate, up: int, down: int) -> Handle:
        h = self._handles.get((up, down))
        if h is None:
            if up == down:
                h = Handle("audio", 1, 1, 0, None, self.slab_out)
            else:
                bank = filter_bank(rate)
                h = Handle("audio", up, down, bank.shape[1], bank.ctypes.data, self.slab_out)
            self._handles[(up, down)], self.lib = h, h.lib
        return h

    def resample(self, raw, fmt: str, channels: int, rate: int) -> np.ndarray:
        """Interleaved PCM bytes (any array, read as bytes) -> float32 ``[ceil(frames * 16000 / rate)]``."""
        code, frame, up, down = check_pcm(fmt, channels, rate)
        raw = np.ascontiguousarray(raw).reshape(-1).view(np.uint8)
        frames = raw.size // frame
        out = np.empty(-(-frames * up // down), dtype=np.float32)
        if not frames:
            return out
        h = self._handle(rate, up, down)
        n = C.c_longlong(0)
        h.check(h.eioku_audio_resample(raw.ctypes.data, code, int(channels), frames, out.ctypes.data, out.size, C.byref(n)),
                "eioku_audio_resample")
        assert n.value == out.size
        self._last = h
        return out

    def resample_float(self, samples, rate: int) -> np.ndarray:
        """Mono float32 samples of an injected ``audio_source`` at ``rate`` -> 16 kHz."""
        return self.resample(np.ascontiguousarray(samples, dtype=np.float32).reshape(-1), "f32", 1, rate)

    def load(self, path: str | Path) -> tuple[np.ndarray, int]:
        """``(16 kHz mono samples, 16000)`` for ``path`` itself when it is a ``.wav``, otherwise for its sibling
        ``<stem>.wav``.  A ``.npy`` file, or a path without that sibling, goes through
        :func:`eioku_amd.transcribe.default_audio_source`, unchanged."""
        from .transcribe import default_audio_source

        p = Path(path)
        if p.suffix.lower() == ".npy":
            return default_audio_source(path)
        if p.suffix.lower() != ".wav":
            p = p.with_suffix(".wav")
        if not p.exists():
            return default_audio_source(path)
        raw, fmt, channels, rate, _ = read_pcm(p)
        return self.resample(raw, fmt, channels, rate), SAMPLE_RATE

    def tile(self, rate: int) -> int:
        """Outputs per workgroup tile of the handle for ``rate`` (tests pick their lengths by it)."""
        up, down = resample_ratio(rate)
        t = C.c_int(0)
        h = self._handle(rate, up, down)
        h.check(h.eioku_audio_tile(C.byref(t)), "eioku_audio_tile")
        return t.value

    def last_ms(self) -> float:
        """Kernel milliseconds of the last :meth:`resample`, summed over its slabs."""
        return 0.0 if self._last is None else self._last.doubles("last_ms")[0]

    def close(self) -> None:
        for h in self._handles.values():
            h.close()
        self._handles = {}
        self._last = None
