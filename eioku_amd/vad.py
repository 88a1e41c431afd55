"""Voice activity on the HIP path (K22): Silero VAD speech gating in front of the Whisper decode.

The reference passes ``vad_filter=config.get("vad_filter", True)`` to faster-whisper
(``ml-service/src/services/model_manager.py:432-443``), which runs Silero VAD over the file, transcribes the concatenation
of the speech chunks and maps the times back.  This module is that path: :class:`SileroVad` (the network, in
``csrc/vad.hip``), :func:`speech_timestamps` (Silero's ``get_speech_timestamps`` as faster-whisper carries it),
:func:`collect_chunks`, :class:`SpeechTimestampsMap` and :func:`restore_speech_timestamps`.

[PUBLIC-LIB] The network, the chunking rule and the timestamp logic are restated from the published model and from
faster-whisper's public sources; neither package nor the checkpoint is a dependency.  Times stay integer milliseconds.
"""
from __future__ import annotations

import bisect
import ctypes as C
import math
from dataclasses import dataclass, fields
from pathlib import Path

import numpy as np

from ._handle import Handle

SAMPLE_RATE = 16000
WINDOW = 512                 # new samples per chunk (32 ms)
CONTEXT = 64                 # samples carried over from the previous chunk
SAMPLES_PER_MS = SAMPLE_RATE // 1000
DEFAULT_SLAB_CHUNKS = 16384  # chunks per device slab (about 8.7 minutes; 34 MB of gate pre-activations)
TENSORS = (("stft.forward_basis_buffer", 258, 256),
           ("encoder.0.weight", 128, 387), ("encoder.0.bias", 128, 1), ("encoder.1.weight", 64, 384), ("encoder.1.bias", 64, 1),
           ("encoder.2.weight", 64, 192), ("encoder.2.bias", 64, 1), ("encoder.3.weight", 128, 192), ("encoder.3.bias", 128, 1),
           ("decoder.rnn.weight_ih", 512, 128), ("decoder.rnn.weight_hh", 512, 128), ("decoder.rnn.bias_ih", 512, 1),
           ("decoder.rnn.bias_hh", 512, 1), ("decoder.out.weight", 1, 128), ("decoder.out.bias", 1, 1))


# ---- options ----------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class VadOptions:
    """faster-whisper's ``VadOptions`` defaults.  ``neg_threshold`` None = ``max(threshold - 0.15, 0.01)``."""
    threshold: float = 0.5
    neg_threshold: float | None = None
    min_speech_duration_ms: int = 0
    max_speech_duration_s: float = math.inf
    min_silence_duration_ms: int = 2000
    speech_pad_ms: int = 400


VAD_KEYS = tuple(f.name for f in fields(VadOptions))


def _is_real(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and not math.isnan(v)


def check_vad_options(threshold=0.5, neg_threshold=None, min_speech_duration_ms=0, max_speech_duration_s=math.inf,
                      min_silence_duration_ms=2000, speech_pad_ms=400) -> VadOptions:
    """The six options, normalised, or ``ValueError``: thresholds in (0, 1), ``_ms`` durations integers >= 0,
    ``max_speech_duration_s`` a positive number (``inf`` = no limit)."""
    for name, v in (("threshold", threshold), ("neg_threshold", neg_threshold)):
        if name == "neg_threshold" and v is None:
            continue
        if not _is_real(v) or not 0.0 < v < 1.0:
            raise ValueError(f"{name} must be a number in (0, 1), got {v!r}")
    for name, v in (("min_speech_duration_ms", min_speech_duration_ms), ("min_silence_duration_ms", min_silence_duration_ms),
                    ("speech_pad_ms", speech_pad_ms)):
        if not _is_real(v) or math.isinf(v) or int(v) != v or v < 0:
            raise ValueError(f"{name} must be an integer >= 0, got {v!r}")
    if not _is_real(max_speech_duration_s) or max_speech_duration_s <= 0:
        raise ValueError(f"max_speech_duration_s must be a positive number, got {max_speech_duration_s!r}")
    return VadOptions(float(threshold), None if neg_threshold is None else float(neg_threshold), int(min_speech_duration_ms),
                      float(max_speech_duration_s), int(min_silence_duration_ms), int(speech_pad_ms))


def vad_options_from(parameters) -> VadOptions:
    """``vad_parameters`` of a task's config (None, a dict of the six options, or a :class:`VadOptions`), validated."""
    if parameters is None:
        return VadOptions()
    if isinstance(parameters, VadOptions):
        parameters = {k: getattr(parameters, k) for k in VAD_KEYS}
    if not isinstance(parameters, dict):
        raise ValueError(f"vad_parameters must be a dict of {VAD_KEYS}, got {parameters!r}")
    unknown = sorted(set(parameters) - set(VAD_KEYS))
    if unknown:
        raise ValueError(f"vad_parameters has unknown keys {unknown}; known: {VAD_KEYS}")
    return check_vad_options(**parameters)


# ---- probabilities -> speech chunks --------------------------------------------------------------------------------------------
def num_chunks(n_samples: int) -> int:
    """faster-whisper pads the tail by ``512 - n % 512`` zeros: a whole zero chunk when ``n`` is a multiple of 512."""
    return int(n_samples) // WINDOW + 1


def speech_timestamps(probs, n_samples: int, options: VadOptions | None = None) -> list[dict]:
    """Silero's ``get_speech_timestamps`` over per-chunk probabilities: ``[{"start", "end"}]`` in samples."""
    o = options or VadOptions()
    W = WINDOW
    threshold = o.threshold
    neg_threshold = max(threshold - 0.15, 0.01) if o.neg_threshold is None else o.neg_threshold
    min_speech = SAMPLES_PER_MS * o.min_speech_duration_ms
    pad = SAMPLES_PER_MS * o.speech_pad_ms
    max_speech = SAMPLE_RATE * o.max_speech_duration_s - W - 2 * pad
    min_silence = SAMPLES_PER_MS * o.min_silence_duration_ms
    min_silence_at_max = SAMPLES_PER_MS * 98
    n_samples = int(n_samples)

    speeches: list[dict] = []
    triggered = False
    cur: dict = {}
    temp_end = prev_end = next_start = 0
    for i, p in enumerate(np.asarray(probs, dtype=np.float64).reshape(-1)):
        at = W * i
        if p >= threshold and temp_end:
            temp_end = 0
            if next_start < prev_end:
                next_start = at
        if p >= threshold and not triggered:
            triggered = True
            cur["start"] = at
            continue
        if triggered and at - cur["start"] > max_speech:
            if prev_end:
                cur["end"] = prev_end
                speeches.append(cur)
                cur = {}
                if next_start < prev_end:
                    triggered = False
                else:
                    cur["start"] = next_start
                prev_end = next_start = temp_end = 0
            else:
                cur["end"] = at
                speeches.append(cur)
                cur = {}
                prev_end = next_start = temp_end = 0
                triggered = False
                continue
        if p < neg_threshold and triggered:
            if not temp_end:
                temp_end = at
            if at - temp_end > min_silence_at_max:
                prev_end = temp_end
            if at - temp_end < min_silence:
                continue
            cur["end"] = temp_end
            if cur["end"] - cur["start"] > min_speech:
                speeches.append(cur)
            cur = {}
            prev_end = next_start = temp_end = 0
            triggered = False
            continue
    if cur and n_samples - cur["start"] > min_speech:
        cur["end"] = n_samples
        speeches.append(cur)

    for k, s in enumerate(speeches):
        if k == 0:
            s["start"] = int(max(0, s["start"] - pad))
        if k != len(speeches) - 1:
            nxt = speeches[k + 1]
            silence = nxt["start"] - s["end"]
            if silence < 2 * pad:
                s["end"] += int(silence // 2)
                nxt["start"] = int(max(0, nxt["start"] - silence // 2))
            else:
                s["end"] = int(min(n_samples, s["end"] + pad))
                nxt["start"] = int(max(0, nxt["start"] - pad))
        else:
            s["end"] = int(min(n_samples, s["end"] + pad))
    return [{"start": int(s["start"]), "end": int(s["end"])} for s in speeches]


def collect_chunks(samples: np.ndarray, chunks: list[dict]) -> np.ndarray:
    """The chunks' samples, concatenated."""
    samples = np.asarray(samples, dtype=np.float32).reshape(-1)
    if not chunks:
        return np.zeros(0, dtype=np.float32)
    return np.concatenate([samples[c["start"]:c["end"]] for c in chunks])


class SpeechTimestampsMap:
    """Times in the concatenated speech audio -> times in the file, in integer milliseconds."""

    def __init__(self, chunks: list[dict]):
        self.chunk_end: list[int] = []
        self.silence_before: list[int] = []
        previous_end = silent = 0
        for c in chunks:
            silent += int(c["start"]) - previous_end
            previous_end = int(c["end"])
            if silent % SAMPLES_PER_MS:
                raise ValueError(f"speech chunks {chunks!r} are not on whole milliseconds")
            self.silence_before.append(silent)
            self.chunk_end.append(int(c["end"]) - silent)

    def _index(self, sample: int, is_end: bool = False) -> int:
        if is_end and sample in self.chunk_end:
            return self.chunk_end.index(sample)
        return min(bisect.bisect_right(self.chunk_end, sample), len(self.chunk_end) - 1)

    def chunk_index(self, t_ms: int, is_end: bool = False) -> int:
        return self._index(SAMPLES_PER_MS * int(t_ms), is_end)

    def original_ms(self, t_ms: int, k: int | None = None, is_end: bool = False) -> int:
        if k is None:
            k = self.chunk_index(t_ms, is_end)
        return int(t_ms) + self.silence_before[k] // SAMPLES_PER_MS


def restore_speech_timestamps(segments: list[dict], chunks: list[dict]) -> list[dict]:
    """faster-whisper's ``restore_speech_timestamps`` on raw segments (``start_ms``, ``end_ms``, ``words`` with
    ``start_ms`` / ``end_ms`` and the reference schema's ``start`` / ``end`` seconds): new dicts, other keys untouched.
    A word moves with the chunk of its midpoint; a segment with words spans its first word's start to its last word's end."""
    ts_map = SpeechTimestampsMap(chunks)
    out = []
    for seg in segments:
        seg = dict(seg)
        if seg.get("words"):
            words = []
            for w in seg["words"]:
                w = dict(w)
                k = ts_map._index((SAMPLES_PER_MS // 2) * (int(w["start_ms"]) + int(w["end_ms"])))
                w["start_ms"] = ts_map.original_ms(w["start_ms"], k)
                w["end_ms"] = ts_map.original_ms(w["end_ms"], k)
                w["start"], w["end"] = w["start_ms"] / 1000, w["end_ms"] / 1000
                words.append(w)
            seg["words"] = words
            seg["start_ms"], seg["end_ms"] = words[0]["start_ms"], words[-1]["end_ms"]
        else:
            seg["start_ms"] = ts_map.original_ms(seg["start_ms"])
            seg["end_ms"] = ts_map.original_ms(seg["end_ms"], is_end=True)
        out.append(seg)
    return out


# ---- the device model -------------------------------------------------------------------------------------------------------
def stft_basis() -> np.ndarray:
    """A basis in the layout of the checkpoint's ``forward_basis_buffer``, for seeded weights: the 256-point DFT (129 cosine
    rows, 129 negated sine rows) under a periodic Hann window."""
    n = np.arange(256, dtype=np.float64)
    k = np.arange(129, dtype=np.float64)[:, None]
    window = 0.5 - 0.5 * np.cos(2 * np.pi * n / 256)
    ang = 2 * np.pi * k * n / 256
    return (np.concatenate([np.cos(ang), -np.sin(ang)]) * window).astype(np.float32)


def seeded_weights(seed: int):
    """Random weights for benchmarks and tests (never a substitute for the checkpoint): ``(name, rows, cols) -> fp32``."""
    rng = np.random.default_rng(seed)

    def make(name: str, rows: int, cols: int) -> np.ndarray:
        if name == "stft.forward_basis_buffer":
            return stft_basis().reshape(-1)
        if name.endswith("bias") or name.startswith("decoder.rnn.bias"):
            return (rng.standard_normal(rows * cols) * 0.1).astype(np.float32)
        std = math.sqrt(2.0 / cols) if name.startswith("encoder") else 1.0 / math.sqrt(cols)
        if name == "decoder.out.weight":
            std = 0.5
        return (rng.standard_normal(rows * cols) * std).astype(np.float32)

    return make


class SileroVad:
    """Silero VAD (16 kHz) on the device: ``speech_probs(samples) -> float32[n_chunks]``.

    ``weights``: ``{tensor name: array}`` or a callable ``(name, rows, cols) -> array``.  ``slab_chunks`` bounds device
    memory: longer files run slab by slab with the context samples and the LSTM state carried on the device."""

    def __init__(self, weights, *, slab_chunks: int = DEFAULT_SLAB_CHUNKS):
        self.slab_chunks = int(slab_chunks)
        self._h = Handle("vad", self.slab_chunks)
        self._h.or_close(self._h.set_tensors, weights)

    @classmethod
    def from_cache(cls, cache_dir: str | Path, seed: int | None = None, **kw):
        """``<cache>/silero_vad/model.safetensors`` under the names of :data:`TENSORS` (INTEGRATION.md §3 maps them to the
        published model's).  ``seed``: random weights, for benchmarks only."""
        if seed is not None:
            return cls(seeded_weights(seed), **kw)
        path = Path(cache_dir) / "silero_vad" / "model.safetensors"
        if not path.exists():
            raise FileNotFoundError(f"Silero VAD checkpoint {path} is missing (safetensors; ONNX and TorchScript files are not read)")
        from .transcribe import read_safetensors

        return cls(read_safetensors(path), **kw)

    def close(self) -> None:
        self._h.close()

    def speech_probs(self, samples: np.ndarray) -> np.ndarray:
        samples = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
        out = np.empty(num_chunks(samples.size), dtype=np.float32)
        n = C.c_longlong(0)
        self._h.check(self._h.eioku_vad_probs(samples.ctypes.data, samples.size, out.ctypes.data, out.size,
                                              C.byref(n)), "eioku_vad_probs")
        assert n.value == out.size
        return out

    def last_ms(self) -> tuple[float, float]:
        """Kernel milliseconds of the last ``speech_probs``: (batched stages, recurrence)."""
        return self._h.doubles("last_ms", 2)
