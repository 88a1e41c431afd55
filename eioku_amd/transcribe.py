"""Transcription on the HIP path: Whisper log-mel (K19), greedy decode with timestamp rules (K20), beam search (K20b),
sampling at a temperature and the one-pass prompt prefill (K20c), word timestamps from cross-attention DTW (K21).

The reference calls ``faster_whisper.WhisperModel.transcribe`` (``model_manager.py:406-467``), which has no ROCm backend.
This module keeps its result dict and replaces the arithmetic: the audio goes up once, ``csrc/whisper.hip`` computes the
log-mel windows, the encoder, and the decoder steps with token selection on the device; the host only cuts the token
lists into segments (Whisper's seek rule) and turns ids into text (byte-level BPE from ``vocab.json``).

Deviations from the reference's call are listed in INTEGRATION.md §3: greedy by default (``beam_size: 5`` restores the
reference's beam search), temperature fallback and conditioning on previous text are opt-in config keys
(:func:`check_fallback`), ``vad_filter`` accepted but not applied, integer millisecond times.  There is no CPU fallback: without the library or a
gfx950 device every compute call raises.
"""

from __future__ import annotations

import ctypes as C
import json
import logging
import math
import string
import struct
import wave
import zlib
from itertools import takewhile
from pathlib import Path

import numpy as np

from ._handle import Handle

logger = logging.getLogger(__name__)

SAMPLE_RATE = 16000
HOP = 160                 # samples per mel frame (10 ms)
N_BINS = 201
MS_PER_FRAME = 10
MS_PER_TIMESTAMP = 20     # one timestamp id = two mel frames
NO_SPEECH_THRESHOLD = 0.6
LOGPROB_THRESHOLD = -1.0
MAX_BEAM = 8              # beam slots per window on the device
MAX_LANES = 64            # windows x beam decoded in lockstep
MAX_FINISH = 16           # finished hypotheses a window can keep (round(beam x patience))


MAX_BEST_OF = 8           # sampled rows per window at a temperature > 0
REFERENCE_TEMPERATURES = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)     # faster-whisper's default schedule
_M64 = (1 << 64) - 1


def _is_number(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v)


def check_fallback(temperature=0.0, best_of=5, compression_ratio_threshold=2.4, log_prob_threshold=-1.0,
                   condition_on_previous_text=False, prompt_reset_on_temperature=0.5, seed=0) -> dict:
    """The temperature-fallback and conditioning keys, normalised, or ``ValueError``.  ``temperature``: a number or a
    non-empty list of numbers >= 0, tried in turn; ``best_of`` 1..8 rows sampled per window at a temperature > 0;
    the two thresholds are numbers (the compression ratio's positive) or None = off; ``condition_on_previous_text`` a bool;
    ``prompt_reset_on_temperature`` a number >= 0; ``seed`` an integer in 0 .. 2^64 - 1."""
    temps = list(temperature) if isinstance(temperature, (list, tuple)) else [temperature]
    if not temps or not all(_is_number(t) and t >= 0 for t in temps):
        raise ValueError(f"temperature must be a number >= 0 or a non-empty list of them, got {temperature!r}")
    if not _is_number(best_of) or int(best_of) != best_of or not 1 <= int(best_of) <= MAX_BEST_OF:
        raise ValueError(f"best_of must be an integer in 1..{MAX_BEST_OF}, got {best_of!r}")
    if compression_ratio_threshold is not None and not (_is_number(compression_ratio_threshold) and compression_ratio_threshold > 0):
        raise ValueError(f"compression_ratio_threshold must be a positive number or None, got {compression_ratio_threshold!r}")
    if log_prob_threshold is not None and not _is_number(log_prob_threshold):
        raise ValueError(f"log_prob_threshold must be a number or None, got {log_prob_threshold!r}")
    if not isinstance(condition_on_previous_text, (bool, np.bool_)):
        raise ValueError(f"condition_on_previous_text must be a bool, got {condition_on_previous_text!r}")
    if not _is_number(prompt_reset_on_temperature) or prompt_reset_on_temperature < 0:
        raise ValueError(f"prompt_reset_on_temperature must be a number >= 0, got {prompt_reset_on_temperature!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) <= _M64:
        raise ValueError(f"seed must be an integer in 0..2^64-1, got {seed!r}")
    return {"temperature": tuple(float(t) for t in temps), "best_of": int(best_of),
            "compression_ratio_threshold": None if compression_ratio_threshold is None else float(compression_ratio_threshold),
            "log_prob_threshold": None if log_prob_threshold is None else float(log_prob_threshold),
            "condition_on_previous_text": bool(condition_on_previous_text),
            "prompt_reset_on_temperature": float(prompt_reset_on_temperature), "seed": int(seed)}


FALLBACK_KEYS = tuple(check_fallback())


def compression_ratio(text: str) -> float:
    """Whisper's loop detector: utf-8 bytes of the text over their zlib-compressed length."""
    raw = text.encode("utf-8")
    return len(raw) / len(zlib.compress(raw))


def _mix64(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def lane_seed(seed: int, start_frame: int, temperature_index: int, row: int) -> int:
    """The noise stream of one sampled row: a function of the run's seed, the window's first mel frame, the position of the
    temperature in the schedule and the row among ``best_of`` - and of nothing else, so a window samples the same tokens
    whatever batch it is decoded in."""
    z = int(seed) & _M64
    for v in (start_frame, temperature_index, row):
        z = _mix64((z + (int(v) + 1) * 0x9E3779B97F4A7C15) & _M64)
    return z


def needs_fallback(avg_logprob: float, ratio: float, no_speech_prob: float, compression_ratio_threshold, log_prob_threshold) -> bool:
    """Whether a window has to be decoded again at the next temperature: its text loops (compression ratio above the
    threshold) or its average log-probability is below the threshold - unless it is silence (``no_speech_prob > 0.6`` with
    the average below the threshold), which no temperature improves."""
    needs = compression_ratio_threshold is not None and ratio > compression_ratio_threshold
    low = log_prob_threshold is not None and avg_logprob < log_prob_threshold
    if no_speech_prob > NO_SPEECH_THRESHOLD and low:
        return False
    return bool(needs or low)


def pick_fallback(tried: list[dict], compression_ratio_threshold) -> dict:
    """Every temperature failed: the try with the highest average log-probability, among those within the compression
    threshold when there are any (faster-whisper's rule; OpenAI's ``transcribe`` keeps the last try instead)."""
    ok = [r for r in tried if compression_ratio_threshold is None or r["compression_ratio"] <= compression_ratio_threshold]
    pool = ok or tried
    best = pool[0]
    for r in pool[1:]:
        if r["avg_logprob"] > best["avg_logprob"]:
            best = r
    return best


def emitted_tokens(tokens, eot: int, timestamp_begin: int) -> list[int]:
    """The sampled ids that :func:`cut_window` turns into segments, timestamps included, EOT excluded: everything up to the
    last consecutive timestamp pair when the window is cut there, otherwise everything before EOT."""
    toks = []
    for t in tokens:
        if int(t) == eot:
            break
        toks.append(int(t))
    is_ts = [t >= timestamp_begin for t in toks]
    single_ending = len(toks) >= 2 and is_ts[-1] and not is_ts[-2]
    cuts = [i + 1 for i in range(len(toks) - 1) if is_ts[i] and is_ts[i + 1]]
    return toks[:cuts[-1]] if cuts and not single_ending else toks


def finish_count(beam_size: int, patience: float) -> int:
    """Whisper's ``max_candidates``: the number of finished hypotheses that ends a window's beam search."""
    return max(1, round(beam_size * patience))


def check_beam(beam_size, patience) -> tuple[int, float]:
    """-> (beam_size, patience) or ``ValueError``: the beam is 1..8, patience positive with at most 16 finished hypotheses."""
    if isinstance(beam_size, bool) or not isinstance(beam_size, (int, float, np.integer, np.floating)) \
            or not math.isfinite(beam_size) or int(beam_size) != beam_size or not 1 <= int(beam_size) <= MAX_BEAM:
        raise ValueError(f"beam_size must be an integer in 1..{MAX_BEAM}, got {beam_size!r}")
    if isinstance(patience, bool) or not isinstance(patience, (int, float, np.integer, np.floating)) \
            or not math.isfinite(patience) or not patience > 0:
        raise ValueError(f"patience must be a positive number, got {patience!r}")
    patience = float(patience)
    if finish_count(int(beam_size), patience) > MAX_FINISH:
        raise ValueError(f"beam_size {beam_size} x patience {patience} keeps more than {MAX_FINISH} finished hypotheses")
    return int(beam_size), patience


# ---- audio input ----------------------------------------------------------------------------------------------------------
def read_wav(path: str | Path) -> tuple[np.ndarray, int]:
    """PCM16 WAV -> (float32 mono samples in [-1, 1], sample rate); stereo is downmixed by mean."""
    with wave.open(str(path), "rb") as w:
        if w.getsampwidth() != 2 or w.getcomptype() != "NONE":
            raise ValueError(f"{path}: only 16-bit PCM WAV is read (sample width {w.getsampwidth()}, {w.getcomptype()})")
        channels, rate = w.getnchannels(), w.getframerate()
        data = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    samples = data.astype(np.float32) / 32768.0
    if channels > 1:
        samples = samples.reshape(-1, channels).mean(axis=1, dtype=np.float32)
    return np.ascontiguousarray(samples, dtype=np.float32), rate


def default_audio_source(path: str | Path) -> tuple[np.ndarray, int]:
    """``path`` itself when it is a ``.wav`` / ``.npy`` (16 kHz samples), otherwise the sibling ``<stem>.wav``.  Audio
    decoding (ffmpeg) is outside this path, as video decoding is."""
    p = Path(path)
    if p.suffix.lower() not in (".wav", ".npy"):
        p = p.with_suffix(".wav")
    if not p.exists():
        raise FileNotFoundError(f"no audio for {path}: {p} does not exist (audio decoding is not part of the HIP path)")
    if p.suffix.lower() == ".npy":
        samples = np.load(p)
        if samples.ndim == 2:
            samples = samples.mean(axis=1 if samples.shape[1] <= 8 else 0)
        return np.ascontiguousarray(samples, dtype=np.float32), SAMPLE_RATE
    return read_wav(p)


def check_rate(rate: int) -> None:
    if int(rate) != SAMPLE_RATE:
        raise ValueError(f"audio is {rate} Hz: Whisper needs {SAMPLE_RATE} Hz and resampling is not built")


# ---- mel filterbank (host, float64) ---------------------------------------------------------------------------------------
def mel_filter_bank(n_mels: int, sr: int = SAMPLE_RATE) -> np.ndarray:
    """Slaney-scale, Slaney-normalised triangular filters [n_mels][201] in float64 (``WhisperFeatureExtractor``'s
    ``mel_filter_bank(norm="slaney", mel_scale="slaney")``, whisper's ``mel_filters.npz``)."""
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    mel_max = min_log_mel + math.log((sr / 2.0) / min_log_hz) / logstep if sr / 2.0 >= min_log_hz else (sr / 2.0) / f_sp
    mels = np.linspace(0.0, mel_max, n_mels + 2)
    hz = np.where(mels >= min_log_mel, min_log_hz * np.exp(logstep * (mels - min_log_mel)), f_sp * mels)
    freqs = np.linspace(0.0, sr / 2.0, N_BINS)
    ramps = hz[:, None] - freqs[None, :]
    fdiff = np.diff(hz)
    w = np.maximum(0.0, np.minimum(-ramps[:-2] / fdiff[:-1, None], ramps[2:] / fdiff[1:, None]))
    return np.ascontiguousarray(w * (2.0 / (hz[2:] - hz[:-2]))[:, None], dtype=np.float64)


# ---- token -> text ----------------------------------------------------------------------------------------------------------
def _gpt2_byte_table() -> dict[str, int]:
    """GPT-2's printable stand-ins for the 256 byte values, inverted (character -> byte)."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    chars, n = keep[:], 0
    for b in range(256):
        if b not in keep:
            keep.append(b)
            chars.append(256 + n)
            n += 1
    return {chr(c): b for b, c in zip(keep, chars)}


class ByteDecoder:
    """Byte-level BPE decode: ids -> vocabulary strings -> bytes (GPT-2 table) -> utf-8 with ``errors="replace"``."""

    def __init__(self, vocab: dict[str, int]):
        self._tokens = {int(i): s for s, i in vocab.items()}
        self._bytes = _gpt2_byte_table()

    def decode(self, ids) -> str:
        raw = bytearray()
        for i in ids:
            s = self._tokens.get(int(i))
            if s is None:
                continue  # special tokens are not in vocab.json
            for ch in s:
                b = self._bytes.get(ch)
                if b is None:
                    raw.extend(ch.encode("utf-8"))
                else:
                    raw.append(b)
        return raw.decode("utf-8", errors="replace")


# ---- words (K21) ------------------------------------------------------------------------------------------------------------
NO_SPACE_LANGUAGES = ("zh", "ja", "th", "lo", "my", "yue")
PREPEND_PUNCTUATIONS = "\"'“¿([{-"
APPEND_PUNCTUATIONS = "\"'.。,，!！?？:：”)]}、"


def check_word_timestamps(value) -> bool:
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"word_timestamps must be a bool, got {value!r}")
    return bool(value)


def _split_on_unicode(ids, decoder) -> tuple[list[str], list[list[int]]]:
    """Whisper's ``split_tokens_on_unicode``: grow a group of tokens until its decoded text holds no U+FFFD (or holds one
    that the text itself has at that place)."""
    full = decoder.decode(ids)
    words, groups, current, offset = [], [], [], 0
    for t in ids:
        current.append(int(t))
        decoded = decoder.decode(current)
        at = decoded.find("\ufffd")
        if at < 0 or offset + at >= len(full) or full[offset + at] == "\ufffd":
            words.append(decoded)
            groups.append(current)
            current = []
            offset += len(decoded)
    return words, groups


def split_to_word_tokens(ids, decoder, language: str | None, eot: int) -> tuple[list[str], list[list[int]]]:
    """Whisper's ``split_to_word_tokens``: (words, the token ids of each).  Always the unicode split; for every language
    but :data:`NO_SPACE_LANGUAGES` a subword then opens a new word when it starts with a space, is punctuation
    (``subword.strip() in string.punctuation``) or is a special id (``>= eot``), and joins the previous word otherwise."""
    subwords, groups = _split_on_unicode(ids, decoder)
    if language is not None and language.strip("<|>").lower() in NO_SPACE_LANGUAGES:
        return subwords, groups
    words, tokens = [], []
    for sub, grp in zip(subwords, groups):
        if grp[0] >= eot or sub.startswith(" ") or sub.strip() in string.punctuation or not words:
            words.append(sub)
            tokens.append(list(grp))
        else:
            words[-1] += sub
            tokens[-1].extend(grp)
    return words, tokens


def merge_punctuations(words: list[dict], prepend: str = PREPEND_PUNCTUATIONS, append: str = APPEND_PUNCTUATIONS) -> list[dict]:
    """Whisper's ``merge_punctuations`` on ``[{"word", "tokens"}]``: a word that is a space and one of ``prepend`` goes in
    front of the next word, a word that is one of ``append`` goes behind the previous one (unless that ends on a space);
    the emptied entries are dropped.  -> the merged list (new dicts)."""
    ws = [{"word": w["word"], "tokens": list(w["tokens"])} for w in words]
    i, j = len(ws) - 2, len(ws) - 1
    while i >= 0:
        if ws[i]["word"].startswith(" ") and ws[i]["word"].strip() in prepend:
            ws[j]["word"] = ws[i]["word"] + ws[j]["word"]
            ws[j]["tokens"] = ws[i]["tokens"] + ws[j]["tokens"]
            ws[i]["word"], ws[i]["tokens"] = "", []
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(ws):
        if not ws[i]["word"].endswith(" ") and ws[j]["word"] in append:
            ws[i]["word"] += ws[j]["word"]
            ws[i]["tokens"] += ws[j]["tokens"]
            ws[j]["word"], ws[j]["tokens"] = "", []
        else:
            i = j
        j += 1
    return [w for w in ws if w["tokens"]]


def window_words(pieces: list[list[int]], jump, prob, window_start_ms: int, decoder, language: str | None, eot: int) -> list[list[dict]]:
    """The words of one aligned window, per segment.  ``pieces``: the text ids of the window's segments in order;
    ``jump[i]`` the frame index (20 ms) at which token row ``i`` of ``text + [eot]`` starts, ``prob[i]`` the probability of
    text token ``i``.  A word over token rows ``[a, b)`` starts at row ``a``, ends at row ``b`` (the EOT row ends the last
    word) and has confidence ``mean(prob[a:b])`` clipped to [0, 1].  Words go to the segments by token count, Whisper's
    loop: a segment takes words until its text-token count is used up."""
    text = [int(t) for piece in pieces for t in piece]
    names, groups = split_to_word_tokens(text, decoder, language, eot)
    merged = merge_punctuations([{"word": w, "tokens": g} for w, g in zip(names, groups)])
    words, a = [], 0
    for w in merged:
        b = a + len(w["tokens"])
        start_ms = int(window_start_ms) + MS_PER_TIMESTAMP * int(jump[a])
        end_ms = int(window_start_ms) + MS_PER_TIMESTAMP * int(jump[b])
        conf = float(np.clip(np.mean(np.asarray(prob[a:b], dtype=np.float64)), 0.0, 1.0))
        words.append({"word": w["word"], "start": start_ms / 1000, "end": end_ms / 1000, "confidence": conf,
                      "start_ms": start_ms, "end_ms": end_ms, "tokens": w["tokens"]})
        a = b
    out, k = [], 0
    for piece in pieces:
        mine, used = [], 0
        while k < len(words) and used < len(piece):
            if words[k]["word"]:
                mine.append(words[k])
            used += len(words[k]["tokens"])
            k += 1
        out.append(mine)
    return out


# ---- segment cutting and the seek rule ------------------------------------------------------------------------------------
def cut_window(tokens, eot: int, timestamp_begin: int, window_start_ms: int, window_frames: int):
    """Whisper's segment and seek rule for one window.  ``tokens``: the sampled ids (anything from the first EOT on is
    dropped).  Returns (``[(start_ms, end_ms, text_ids)]``, frames to advance).

    Segments are cut at consecutive timestamp pairs.  When the window ends on a single unpaired timestamp, everything up
    to it is one more segment and seek advances by the whole window; otherwise seek advances to the last pair's timestamp.
    With no pair at all there is one segment up to the last timestamp, or up to the window's end."""
    toks = []
    for t in tokens:
        if int(t) == eot:
            break
        toks.append(int(t))
    is_ts = [t >= timestamp_begin for t in toks]
    single_ending = len(toks) >= 2 and is_ts[-1] and not is_ts[-2]  # Whisper's test: the last two flags are [False, True]
    cuts = [i + 1 for i in range(len(toks) - 1) if is_ts[i] and is_ts[i + 1]]
    segments = []

    def ms(tok):
        return window_start_ms + MS_PER_TIMESTAMP * (tok - timestamp_begin)

    if cuts:
        if single_ending:
            cuts.append(len(toks))
        last = 0
        for cut in cuts:
            piece = toks[last:cut]
            segments.append((ms(piece[0]), ms(piece[-1]), [t for t in piece if t < eot]))
            last = cut
        if single_ending:
            advance = window_frames
        else:
            advance = 2 * (toks[last - 1] - timestamp_begin)
    else:
        end_ms = window_start_ms + MS_PER_FRAME * window_frames
        stamps = [t for t in toks if t >= timestamp_begin]
        if stamps and stamps[-1] != timestamp_begin:
            end_ms = ms(stamps[-1])
        segments.append((window_start_ms, end_ms, [t for t in toks if t < eot]))
        advance = window_frames
    return segments, advance


def skip_window(no_speech_prob: float, sum_logprob: float, n_text_tokens: int) -> bool:
    """The no-speech rule: skip when ``no_speech_prob > 0.6`` and the average log-probability is ``< -1.0`` (the average
    runs over the sampled tokens and the closing EOT, as in Whisper)."""
    return no_speech_prob > NO_SPEECH_THRESHOLD and sum_logprob / (n_text_tokens + 1) < LOGPROB_THRESHOLD


# ---- checkpoint files -----------------------------------------------------------------------------------------------------
_ST_DTYPES = {"F32": np.float32, "F16": np.float16, "F64": np.float64}


def read_safetensors(path: str | Path) -> dict[str, np.ndarray]:
    """Minimal safetensors reader (8-byte header length, JSON header, raw little-endian data); fp32 arrays out."""
    buf = Path(path).read_bytes()
    (hlen,) = struct.unpack("<Q", buf[:8])
    header = json.loads(buf[8:8 + hlen])
    out = {}
    for name, meta in header.items():
        if name == "__metadata__":
            continue
        a, b = meta["data_offsets"]
        raw = buf[8 + hlen + a:8 + hlen + b]
        if meta["dtype"] == "BF16":
            arr = (np.frombuffer(raw, dtype="<u2").astype(np.uint32) << 16).view(np.float32)
        elif meta["dtype"] in _ST_DTYPES:
            arr = np.frombuffer(raw, dtype=_ST_DTYPES[meta["dtype"]]).astype(np.float32)
        else:
            raise ValueError(f"{path}: tensor {name} has unsupported dtype {meta['dtype']}")
        out[name] = arr.reshape(meta["shape"])
    return out


def whisper_dims(config: dict, generation_config: dict) -> dict:
    """The dimensions and special ids the library needs, from ``config.json`` and ``generation_config.json``."""
    gen = generation_config
    d, heads = int(config["d_model"]), int(config["encoder_attention_heads"])
    if int(config.get("decoder_attention_heads", heads)) != heads:
        raise ValueError("encoder and decoder head counts differ")
    lang_to_id = gen.get("lang_to_id") or {}
    langs = sorted(lang_to_id.items(), key=lambda kv: kv[1])
    no_ts = int(gen["no_timestamps_token_id"])
    task_to_id = gen.get("task_to_id") or {}
    return {
        "n_mels": int(config.get("num_mel_bins", 80)), "d_model": d, "heads": heads,
        "enc_layers": int(config["encoder_layers"]), "dec_layers": int(config["decoder_layers"]),
        "enc_ffn": int(config["encoder_ffn_dim"]), "dec_ffn": int(config["decoder_ffn_dim"]),
        "vocab": int(config["vocab_size"]), "max_source_positions": int(config["max_source_positions"]),
        "max_target_positions": int(config["max_target_positions"]),
        "sot": int(gen.get("decoder_start_token_id", config.get("decoder_start_token_id"))),
        "eot": int(gen.get("eos_token_id", config.get("eos_token_id"))),
        "transcribe": int(task_to_id["transcribe"]) if "transcribe" in task_to_id else None,
        "no_timestamps": no_ts, "timestamp_begin": no_ts + 1,
        # <|nospeech|> sits right before <|notimestamps|> in every Whisper vocabulary
        "no_speech": int(gen.get("no_speech_token_id", no_ts - 1)),
        # <|startofprev|> sits right before <|nospeech|>
        "sot_prev": int(gen.get("prev_sot_token_id", int(gen.get("no_speech_token_id", no_ts - 1)) - 1)),
        "max_initial_timestamp_index": int(gen.get("max_initial_timestamp_index", 50)),
        "suppress": [int(t) for t in gen.get("suppress_tokens") or []],
        "begin_suppress": [int(t) for t in gen.get("begin_suppress_tokens") or []],
        "lang_ids": [int(i) for _, i in langs],
        "lang_codes": [k.strip("<|>") for k, _ in langs],
        # [[layer, head], ...] or None = every head of the upper half of the decoder layers (Whisper's default)
        "alignment_heads": [[int(l), int(h)] for l, h in gen["alignment_heads"]] if gen.get("alignment_heads") else None,
    }


def seeded_weights(dims: dict, seed: int):
    """Random weights for the benchmark (never a substitute for a checkpoint): name, shape -> fp32 array."""
    rng = np.random.default_rng(seed)

    def make(name: str, rows: int, cols: int) -> np.ndarray:
        if name.endswith("layer_norm.weight"):
            return np.ones(rows * cols, dtype=np.float32)
        if name.endswith(".bias"):
            return np.zeros(rows * cols, dtype=np.float32)
        std = 0.1 if "embed" in name else math.sqrt(2.0 / cols)
        return (rng.standard_normal(rows * cols, dtype=np.float32) * np.float32(std)).astype(np.float32)

    return make


# ---- the device model -----------------------------------------------------------------------------------------------------
class WhisperTranscriber:
    """One Whisper checkpoint on the device: log-mel, encoder, greedy decoder, and the host loop around them.

    ``dims``: the dict of :func:`whisper_dims`.  ``weights``: ``{HF tensor name: array}`` or a callable
    ``(name, rows, cols) -> array``.  ``vocab``: ``vocab.json`` as a dict (may be empty: ids then decode to "")."""

    def __init__(self, dims: dict, weights, vocab: dict | None = None, *, sync_every: int = 8):
        from . import _lib

        self._lib_mod = _lib
        self.dims = dict(dims)
        self.sync_every = int(sync_every)
        self.decoder = ByteDecoder(vocab or {})
        d = self.dims
        self._keep = [np.asarray(d["suppress"], dtype=np.int32), np.asarray(d["begin_suppress"], dtype=np.int32),
                      np.asarray(d["lang_ids"], dtype=np.int32), mel_filter_bank(d["n_mels"])]
        cfg = _lib.WhisperCfg()
        for k in ("n_mels", "d_model", "heads", "enc_layers", "dec_layers", "enc_ffn", "dec_ffn", "vocab",
                  "max_source_positions", "max_target_positions", "eot", "no_timestamps", "timestamp_begin", "no_speech"):
            setattr(cfg, k, int(d[k]))
        mi = d.get("max_initial_timestamp_index")
        cfg.max_initial_timestamp_index = -1 if mi is None else int(mi)
        cfg.n_suppress, cfg.n_begin_suppress, cfg.n_langs = (len(a) for a in self._keep[:3])
        cfg.suppress, cfg.begin_suppress, cfg.lang_ids, cfg.mel_filters = (a.ctypes.data for a in self._keep)
        self._h = Handle("whisper", C.byref(cfg))
        self.window_frames = 2 * d["max_source_positions"]
        self._h.or_close(self._load, weights)

    def _load(self, weights) -> None:
        if self.dims.get("alignment_heads"):
            self.set_alignment_heads(self.dims["alignment_heads"])
        self._h.set_tensors(weights)

    @classmethod
    def from_cache(cls, cache_dir: str | Path, model_name: str = "base", seed: int | None = None, **kw):
        """``<cache>/whisper/<model_name>/{config.json, generation_config.json, model.safetensors, vocab.json}`` (the
        Hugging Face ``openai/whisper-*`` files; ctranslate2 ``model.bin`` is not read).  ``seed``: random weights, for
        the benchmark only - the three JSON files are still required."""
        root = Path(cache_dir) / "whisper" / model_name
        need = ["config.json", "generation_config.json", "vocab.json"] + ([] if seed is not None else ["model.safetensors"])
        missing = [f for f in need if not (root / f).exists()]
        if missing:
            raise FileNotFoundError(f"Whisper checkpoint {root} is missing {missing} (Hugging Face format; a ctranslate2 "
                                    "model.bin is not read)")
        dims = whisper_dims(json.loads((root / "config.json").read_text()),
                            json.loads((root / "generation_config.json").read_text()))
        vocab = json.loads((root / "vocab.json").read_text())
        if seed is not None:
            weights = seeded_weights(dims, seed)
        else:
            weights = read_safetensors(root / "model.safetensors")
            if "proj_out.weight" in weights and "model.decoder.embed_tokens.weight" not in weights:
                weights["model.decoder.embed_tokens.weight"] = weights["proj_out.weight"]
        return cls(dims, weights, vocab, **kw)

    def close(self) -> None:
        if getattr(self, "_h", None):  # subclasses that script the device calls never create one
            self._h.close()

    # -- device calls
    def set_audio(self, samples: np.ndarray) -> None:
        self._samples = np.ascontiguousarray(samples, dtype=np.float32)
        self._lib_mod.check(self._h.eioku_whisper_set_audio(self._samples.ctypes.data, self._samples.size),
                            "eioku_whisper_set_audio")

    def logmel(self, offsets, fetch: bool = True):
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        out = np.empty((len(off), self.dims["n_mels"], self.window_frames), dtype=np.float32) if fetch else None
        self._lib_mod.check(self._h.eioku_whisper_logmel(off.ctypes.data, len(off), out.ctypes.data if fetch else None),
                            "eioku_whisper_logmel")
        return out

    def encode(self, n_windows: int, mel: np.ndarray | None = None) -> None:
        if mel is not None:
            mel = np.ascontiguousarray(mel, dtype=np.float32)
            if mel.shape != (n_windows, self.dims["n_mels"], self.window_frames):
                raise ValueError(f"mel must be {(n_windows, self.dims['n_mels'], self.window_frames)}, got {mel.shape}")
        self._lib_mod.check(self._h.eioku_whisper_encode(mel.ctypes.data if mel is not None else None, n_windows),
                            "eioku_whisper_encode")

    def encoder_output(self, n_windows: int) -> np.ndarray:
        out = np.empty((n_windows, self.dims["max_source_positions"], self.dims["d_model"]), dtype=np.float16)
        self._lib_mod.check(self._h.eioku_whisper_encoder_output(out.ctypes.data, out.size), "eioku_whisper_encoder_output")
        return out

    def decode(self, prompt, n_windows: int, max_new_tokens: int, sync_every: int | None = None) -> dict:
        p = np.ascontiguousarray(prompt, dtype=np.int32)
        B, n = int(n_windows), int(max_new_tokens)
        tokens = np.zeros((B, max(n, 1)), dtype=np.int32)
        n_out = np.zeros(B, dtype=np.int32)
        lang = np.zeros(B, dtype=np.int32)
        total = np.zeros(B, dtype=np.float32)
        nsp = np.zeros(B, dtype=np.float32)
        self._lib_mod.check(self._h.eioku_whisper_decode(
            p.ctypes.data, len(p), B, n, int(sync_every or self.sync_every), tokens.ctypes.data, n_out.ctypes.data,
            total.ctypes.data, nsp.ctypes.data, lang.ctypes.data), "eioku_whisper_decode")
        return {"tokens": tokens[:, :n], "n": n_out, "sum_logprob": total, "no_speech_prob": nsp, "lang": lang}

    def decode_beam(self, prompt, n_windows: int, max_new_tokens: int, beam_size: int, patience: float = 1.0,
                    sync_every: int | None = None, trace: bool = False) -> dict:
        """Beam search over the last encode.  Per window ``H = max(beam_size, C)`` hypothesis rows (``C`` =
        :func:`finish_count`): the finished hypotheses in the order they finished, then live beams in slot order while
        there are fewer than ``beam_size``; ``n_hyp`` rows are in use.  ``tokens`` [B][H][max_new] EOT-filled, ``n`` tokens
        sampled up to and including EOT, ``ended`` whether the row ended on EOT, ``sum_logprob``, ``best`` the row with the
        largest ``sum_logprob / max(1, tokens before EOT)``.  ``trace=True`` (tests) adds ``trace_src`` / ``trace_tok``
        [max_new][B][W]: per sampled step the source slot and token of every next slot (-1: none)."""
        W, patience = check_beam(beam_size, patience)
        p = np.ascontiguousarray(prompt, dtype=np.int32)
        B, n, Cn = int(n_windows), int(max_new_tokens), finish_count(W, patience)
        out, tr, tr_ptrs = self._beam_outputs(B, W, Cn, n, trace)
        lang = np.zeros(B, dtype=np.int32)
        self._lib_mod.check(self._h.eioku_whisper_decode_beam(
            p.ctypes.data, len(p), B, W, Cn, n, int(sync_every or self.sync_every), *(a.ctypes.data for a in out.values()),
            lang.ctypes.data, *tr_ptrs), "eioku_whisper_decode_beam")
        return {**out, "lang": lang, **tr}

    @staticmethod
    def _beam_outputs(B: int, W: int, Cn: int, n: int, trace: bool) -> tuple[dict, dict, tuple]:
        """The output arrays of a beam decode, in the order the library takes them: the hypothesis rows, then (with
        ``trace``) the trace arrays, and what the library is handed for the trace (NULL without one)."""
        H = max(W, Cn)
        out = {"tokens": np.zeros((B, H, max(n, 1)), dtype=np.int32), "n": np.zeros((B, H), dtype=np.int32),
               "ended": np.zeros((B, H), dtype=np.int32), "sum_logprob": np.zeros((B, H), dtype=np.float32),
               "n_hyp": np.zeros(B, dtype=np.int32), "best": np.zeros(B, dtype=np.int32),
               "no_speech_prob": np.zeros(B, dtype=np.float32)}
        tr = {k: np.full((max(n, 1), B, W), -1, dtype=np.int32) for k in ("trace_src", "trace_tok")} if trace else {}
        return out, tr, tuple(a.ctypes.data for a in tr.values()) if trace else (None, None)

    @staticmethod
    def _pad_prefixes(prefixes, rows: int) -> tuple[np.ndarray, int, np.ndarray]:
        """Per-lane prefixes as the debug entries take them: [rows][cap] zero-padded, cap, and the lengths."""
        cap = max(1, max(len(p) for p in prefixes))
        pre = np.zeros((rows, cap), dtype=np.int32)
        for i, p in enumerate(prefixes):
            pre[i, :len(p)] = p
        return pre, cap, np.asarray([len(p) for p in prefixes], dtype=np.int32)

    def beam_select(self, logits, prefixes, sums, fin_count, beam_size: int, patience: float = 1.0) -> list[dict]:
        """Debug: one beam step on supplied logits [B * W][vocab].  ``prefixes`` / ``sums`` per lane (window-major; a sum of
        -inf is a dead slot), ``fin_count`` per window.  Per window: ``live`` [(src, token, sum)], ``finished`` [(src,
        sum)] in walk order, ``fin_count`` afterwards, ``complete``."""
        W, patience = check_beam(beam_size, patience)
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        L = logits.shape[0]
        B = L // W
        if B * W != L or len(prefixes) != L or len(sums) != L or len(fin_count) != B:
            raise ValueError("logits, prefixes and sums are per lane (windows x beam), fin_count per window")
        pre, cap, plen = self._pad_prefixes(prefixes, L)
        sums = np.ascontiguousarray(sums, dtype=np.float32)
        fc = np.ascontiguousarray(fin_count, dtype=np.int32)
        src, tok, fsrc = (np.zeros(L, dtype=np.int32) for _ in range(3))
        osum, fsum = np.zeros(L, dtype=np.float32), np.zeros(L, dtype=np.float32)
        n_live, n_fin, fc_out, complete = (np.zeros(B, dtype=np.int32) for _ in range(4))
        self._lib_mod.check(self._h.eioku_whisper_beam_select(
            logits.ctypes.data, B, W, finish_count(W, patience), pre.ctypes.data, cap, plen.ctypes.data, sums.ctypes.data,
            fc.ctypes.data, src.ctypes.data, tok.ctypes.data, osum.ctypes.data, n_live.ctypes.data, fsrc.ctypes.data,
            fsum.ctypes.data, n_fin.ctypes.data, fc_out.ctypes.data, complete.ctypes.data), "eioku_whisper_beam_select")
        out = []
        for b in range(B):
            o = b * W
            out.append({"live": [(int(src[o + i]), int(tok[o + i]), float(osum[o + i])) for i in range(n_live[b])],
                        "finished": [(int(fsrc[o + i]), float(fsum[o + i])) for i in range(n_fin[b])],
                        "fin_count": int(fc_out[b]), "complete": bool(complete[b])})
        return out

    def decode_prompted(self, prompts, sot_index: int, max_new_tokens: int, *, windows=None, group: int = 1,
                        temperature: float = 0.0, seeds=None, sync_every: int | None = None) -> dict:
        """K20c: rows with prompts ``[B][P]`` (one common length) prefilled in one pass, then ``group`` lanes per row decoded in
        lockstep.  ``windows[b]``: the encoded window row ``b`` reads (None: identity).  ``temperature == 0`` is the greedy
        rule (``group`` 1, no seeds); above 0 every lane samples with its own ``seeds[b][g]``.  ``tokens`` [B][G][max_new],
        ``n`` / ``sum_logprob`` [B][G], ``best`` [B], ``no_speech_prob`` [B] (at prompt position ``sot_index``)."""
        p = np.ascontiguousarray(prompts, dtype=np.int32)
        if p.ndim != 2:
            raise ValueError("prompts must be [rows][P]: one common prompt length")
        B, P, G, n = p.shape[0], p.shape[1], int(group), int(max_new_tokens)
        win = None if windows is None else np.ascontiguousarray(windows, dtype=np.int32)
        if win is not None and win.shape != (B,):
            raise ValueError("windows names one encoded window per row")
        sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        if sd is not None and sd.size != B * G:
            raise ValueError("seeds must hold one value per lane (rows x group)")
        tokens = np.zeros((B, G, max(n, 1)), dtype=np.int32)
        n_out, total = np.zeros((B, G), dtype=np.int32), np.zeros((B, G), dtype=np.float32)
        best, nsp = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.float32)
        self._lib_mod.check(self._h.eioku_whisper_decode_prompted(
            p.ctypes.data, P, int(sot_index), win.ctypes.data if win is not None else None, B, G, float(temperature),
            sd.ctypes.data if sd is not None else None, n, int(sync_every or self.sync_every), tokens.ctypes.data,
            n_out.ctypes.data, total.ctypes.data, best.ctypes.data, nsp.ctypes.data), "eioku_whisper_decode_prompted")
        return {"tokens": tokens, "n": n_out, "sum_logprob": total, "best": best, "no_speech_prob": nsp}

    def decode_beam_prompted(self, prompts, sot_index: int, max_new_tokens: int, beam_size: int, patience: float = 1.0, *,
                             windows=None, sync_every: int | None = None, trace: bool = False) -> dict:
        """:meth:`decode_beam` with per-window prompts ``[B][P]`` prefilled once per window, the no-speech probability at
        ``sot_index`` and the row -> window map of :meth:`decode_prompted`.  The same outputs, without ``lang``."""
        W, patience = check_beam(beam_size, patience)
        p = np.ascontiguousarray(prompts, dtype=np.int32)
        if p.ndim != 2:
            raise ValueError("prompts must be [windows][P]: one common prompt length")
        B, P, n, Cn = p.shape[0], p.shape[1], int(max_new_tokens), finish_count(W, patience)
        win = None if windows is None else np.ascontiguousarray(windows, dtype=np.int32)
        if win is not None and win.shape != (B,):
            raise ValueError("windows names one encoded window per row")
        out, tr, tr_ptrs = self._beam_outputs(B, W, Cn, n, trace)
        self._lib_mod.check(self._h.eioku_whisper_decode_beam_prompted(
            p.ctypes.data, P, int(sot_index), win.ctypes.data if win is not None else None, B, W, Cn, n,
            int(sync_every or self.sync_every), *(a.ctypes.data for a in out.values()), *tr_ptrs), "eioku_whisper_decode_beam_prompted")
        return {**out, **tr}

    def sample(self, logits, prefixes, temperature: float, seeds, idx) -> tuple[np.ndarray, np.ndarray]:
        """Debug: rules + Gumbel-max sampling on supplied logits [B][vocab]; per lane a prefix, a seed and a sample index."""
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        B = logits.shape[0]
        pre, cap, plen = self._pad_prefixes(prefixes, B)
        sd, ix = np.ascontiguousarray(seeds, dtype=np.uint64), np.ascontiguousarray(idx, dtype=np.int32)
        if len(prefixes) != B or sd.shape != (B,) or ix.shape != (B,):
            raise ValueError("prefixes, seeds and idx are per lane")
        tok, lp = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.float32)
        self._lib_mod.check(self._h.eioku_whisper_sample(logits.ctypes.data, B, pre.ctypes.data, cap, plen.ctypes.data,
                                                         float(temperature), sd.ctypes.data, ix.ctypes.data, tok.ctypes.data,
                                                         lp.ctypes.data), "eioku_whisper_sample")
        return tok, lp

    def prefill_logits(self, ids, n_prefill: int | None = None) -> np.ndarray:
        """Debug: rule-free logits [B][T][vocab] of ids [B][T]; the first ``n_prefill`` (default: all) positions in one
        prefill pass, the others position by position on the keys and values it left."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        out = np.empty(ids.shape + (self.dims["vocab"],), dtype=np.float32)
        self._lib_mod.check(self._h.eioku_whisper_prefill_logits(
            ids.ctypes.data, ids.shape[1], ids.shape[0], int(ids.shape[1] if n_prefill is None else n_prefill),
            out.ctypes.data), "eioku_whisper_prefill_logits")
        return out

    def forced_logits(self, ids) -> np.ndarray:
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        out = np.empty(ids.shape + (self.dims["vocab"],), dtype=np.float32)
        self._lib_mod.check(self._h.eioku_whisper_forced_logits(ids.ctypes.data, ids.shape[1], ids.shape[0], out.ctypes.data),
                            "eioku_whisper_forced_logits")
        return out

    def select(self, logits, prefixes) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Debug: rules + argmax on supplied logits [B][vocab]; ``prefixes``: per lane the tokens sampled so far."""
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        B = logits.shape[0]
        pre, cap, plen = self._pad_prefixes(prefixes, B)
        tok, lp, masked = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.float32), np.empty_like(logits)
        self._lib_mod.check(self._h.eioku_whisper_select(logits.ctypes.data, B, pre.ctypes.data, cap, plen.ctypes.data,
                                                         tok.ctypes.data, lp.ctypes.data, masked.ctypes.data), "eioku_whisper_select")
        return tok, lp, masked

    def set_alignment_heads(self, pairs) -> None:
        """K21: the (layer, head) pairs whose cross-attention is aligned; empty or None = the default (upper half)."""
        p = np.ascontiguousarray(pairs if pairs is not None else [], dtype=np.int32).reshape(-1, 2)
        self._lib_mod.check(self._h.eioku_whisper_set_alignment_heads(p.ctypes.data if len(p) else None, len(p)),
                            "eioku_whisper_set_alignment_heads")

    def align(self, seqs, n_tok, sot_len: int, n_frames, windows=None, cost: bool = False) -> dict:
        """K21: one teacher-forced pass over ``seqs`` [R][T] (sot sequence, ``<|notimestamps|>``, text, EOT, EOT padding;
        true lengths ``n_tok``) against the last encode, then cost, DTW and token probabilities on the device.  ``jump``
        [R][T - sot_len - 1] (-1 past a row's text + EOT), ``prob`` of the same shape (0 past a row's text), and with
        ``cost=True`` (tests) ``cost`` [R][T - sot_len - 1][max(n_frames) // 2]."""
        s = np.ascontiguousarray(seqs, dtype=np.int32)
        if s.ndim != 2:
            raise ValueError("seqs must be [rows][T]: pad the rows with EOT to one length")
        R, T = s.shape
        nt, nf = np.ascontiguousarray(n_tok, dtype=np.int32), np.ascontiguousarray(n_frames, dtype=np.int32)
        win = None if windows is None else np.ascontiguousarray(windows, dtype=np.int32)
        if nt.shape != (R,) or nf.shape != (R,) or (win is not None and win.shape != (R,)):
            raise ValueError("n_tok, n_frames and windows hold one value per row")
        N = max(T - int(sot_len) - 1, 1)
        jump, prob = np.full((R, N), -1, dtype=np.int32), np.zeros((R, N), dtype=np.float32)
        cst = np.zeros((R, N, max(int(nf.max()) // 2, 1)), dtype=np.float32) if cost else None
        self._lib_mod.check(self._h.eioku_whisper_align(
            s.ctypes.data, T, nt.ctypes.data, int(sot_len), win.ctypes.data if win is not None else None, nf.ctypes.data, R,
            jump.ctypes.data, prob.ctypes.data, cst.ctypes.data if cost else None), "eioku_whisper_align")
        out = {"jump": jump, "prob": prob}
        if cost:
            out["cost"] = cst
        return out

    def align_cost(self, weights, sot_len: int) -> np.ndarray:
        """Debug: normalise + median filter + head mean on supplied weights [H][T][F] -> cost [T - sot_len - 1][F]."""
        a = np.ascontiguousarray(weights, dtype=np.float32)
        H, T, F = a.shape
        out = np.zeros((max(T - int(sot_len) - 1, 1), F), dtype=np.float32)
        self._lib_mod.check(self._h.eioku_whisper_align_cost(a.ctypes.data, H, T, F, int(sot_len), out.ctypes.data),
                            "eioku_whisper_align_cost")
        return out

    def dtw(self, cost) -> dict:
        """Debug: the warping on a supplied cost [N][F]: ``jump`` [N], and the path as ``text_idx`` / ``time_idx``."""
        c = np.ascontiguousarray(cost, dtype=np.float32)
        N, F = c.shape
        jump, ti, fi = np.zeros(N, dtype=np.int32), np.zeros(N + F, dtype=np.int32), np.zeros(N + F, dtype=np.int32)
        n = C.c_int(0)
        self._lib_mod.check(self._h.eioku_whisper_dtw(c.ctypes.data, N, F, jump.ctypes.data, ti.ctypes.data, fi.ctypes.data,
                                                      C.byref(n)), "eioku_whisper_dtw")
        return {"jump": jump, "text_idx": ti[:n.value].copy(), "time_idx": fi[:n.value].copy()}

    def last_align_ms(self) -> tuple[float, float, float]:
        """Device milliseconds of the last :meth:`align`: the pass with the probabilities, the cost kernels, the DTW."""
        return self._h.doubles("last_align_ms", 3)

    def last_launches(self) -> tuple[int, int]:
        a, b = C.c_int(0), C.c_int(0)
        self._lib_mod.check(self._h.eioku_whisper_last_launches(C.byref(a), C.byref(b)), "eioku_whisper_last_launches")
        return a.value, b.value

    def last_flops(self) -> float:
        return self._h.doubles("last_flops")[0]

    # -- the host loop
    def _language_token(self, language: str | None):
        d = self.dims
        if language is None:
            return None
        code = language.strip("<|>").lower()
        if code not in d["lang_codes"]:
            raise ValueError(f"language {language!r} is not in the checkpoint's generation_config ({len(d['lang_codes'])} codes)")
        return d["lang_ids"][d["lang_codes"].index(code)]

    def _prompt(self, lang_id: int | None) -> list[int]:
        d = self.dims
        prompt = [d["sot"]]
        if lang_id is not None:
            prompt.append(lang_id)
        if d.get("transcribe") is not None:
            prompt.append(d["transcribe"])
        return prompt

    def _window_words(self, items: list[tuple[int, int, int, list[list[int]]]], lang_id, code) -> list[list[list[dict]]]:
        """K21: one :meth:`align` call for the accepted windows of the current encode.  ``items``: per window (encoded window
        index, first mel frame, content frames, the text ids of its segments).  -> per window, per segment, the words."""
        d = self.dims
        sot_seq = self._prompt(lang_id)
        out: list[list[list[dict]]] = [[[] for _ in pieces] for _, _, _, pieces in items]
        rows = [k for k, (_, _, size, pieces) in enumerate(items) if size >= 2 and any(pieces)]
        if not rows:
            return out
        seqs = [sot_seq + [d["no_timestamps"]] + [t for piece in items[k][3] for t in piece] + [d["eot"]] for k in rows]
        T = max(len(q) for q in seqs)
        if T > d["max_target_positions"]:
            raise ValueError(f"a window of {T - len(sot_seq) - 2} text tokens does not fit the decoder's "
                             f"{d['max_target_positions']} positions for the word alignment")
        res = self.align([q + [d["eot"]] * (T - len(q)) for q in seqs], [len(q) for q in seqs], len(sot_seq),
                         [items[k][2] for k in rows], windows=[items[k][0] for k in rows])
        for row, k in enumerate(rows):
            _, seek, _, pieces = items[k]
            out[k] = window_words(pieces, res["jump"][row], res["prob"][row], seek * MS_PER_FRAME, self.decoder, code, d["eot"])
        return out

    def transcribe(self, samples: np.ndarray, language: str | None = None, *, window_mode: str = "seek",
                   batch_windows: int = 8, max_new_tokens: int | None = None, beam_size: int = 1,
                   patience: float = 1.0, word_timestamps: bool = False, **fallback) -> dict:
        """-> ``{"segments": [{start_ms, end_ms, text, language, confidence: None, words: None}], "language": code}``.

        ``window_mode="seek"``: one window at a time, the next one starts where Whisper's seek rule says.
        ``window_mode="fixed"``: independent back-to-back windows, up to ``batch_windows`` decoded in lockstep; a segment
        cannot span a window edge.

        ``beam_size=1`` decodes greedily.  ``beam_size > 1`` runs beam search with Whisper's ``patience`` and keeps each
        window's best hypothesis by length-normalised log-probability (``faster_whisper``'s call: 5 and 1.0); in ``fixed``
        mode a batch is split so that windows x beam stays within the device's 64 lanes.

        ``**fallback``: the keys of :func:`check_fallback`.  With a temperature schedule, a window whose text loops or whose
        average log-probability is poor is decoded again at the next temperature (``best_of`` sampled rows, the best kept;
        ``beam_size`` applies at temperature 0 only); when every temperature fails the try with the highest average
        log-probability is kept, among those within the compression threshold when there are any (faster-whisper's rule).
        ``condition_on_previous_text`` (``seek`` mode only) puts up to ``max_target_positions // 2 - 1`` previous tokens
        behind ``<|startofprev|>`` in front of the prompt; a window accepted above ``prompt_reset_on_temperature`` resets
        them.  Raw segments then also carry ``temperature``, ``avg_logprob`` and ``compression_ratio``, and the raw result a
        ``windows`` list with the same figures per decoded window.  With none of these keys the device calls are the ones
        above.

        ``word_timestamps=True`` (K21) aligns every accepted window's text tokens to its audio on the device (one
        :meth:`align` call per window in ``seek`` mode, one per batch in ``fixed`` mode) and fills each segment's ``words``
        with ``{"word", "start", "end", "confidence"}`` (seconds; raw segments also ``start_ms`` / ``end_ms`` / ``tokens``
        per word).  Segments, text and the seek position are what they are without it."""
        word_timestamps = check_word_timestamps(word_timestamps)
        if window_mode not in ("seek", "fixed"):
            raise ValueError(f"window_mode must be 'seek' or 'fixed', got {window_mode!r}")
        beam_size, patience = check_beam(beam_size, patience)
        unknown = sorted(set(fallback) - set(FALLBACK_KEYS))
        if unknown:
            raise TypeError(f"transcribe() got unexpected keyword arguments {unknown}")
        fb = check_fallback(**fallback) if fallback else None
        if fb and fb["condition_on_previous_text"] and window_mode != "seek":
            raise ValueError("condition_on_previous_text needs window_mode='seek': fixed windows decode in lockstep")
        d = self.dims
        Tm, eot, tb = d["max_target_positions"], d["eot"], d["timestamp_begin"]
        samples = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
        content_frames = len(samples) // HOP
        lang_id = self._language_token(language)
        if content_frames == 0:
            return {"segments": [], "language": language}
        self.set_audio(samples)
        segments: list[dict] = []
        # the no-speech rule skips a window on no_speech_prob > 0.6 with the average log-probability below this (None: on the
        # probability alone)
        threshold = fb["log_prob_threshold"] if fb else LOGPROB_THRESHOLD
        # fallback only: the figures of every decoded window, the tokens emitted so far and where the previous text starts
        windows_log: list[dict] = []
        all_tokens: list[int] = []
        reset = 0

        def record(tokens, total, nsp, **extra) -> dict:
            """One window's accepted decode; the average runs over the sampled tokens and the closing EOT, as in Whisper."""
            toks = [int(t) for t in tokens]
            n_text = toks.index(eot) if eot in toks else len(toks)
            return {"tokens": toks, "sum_logprob": float(total), "no_speech_prob": float(nsp),
                    "avg_logprob": float(total) / (n_text + 1), **extra}

        def decode_plain(seeks: list[int]) -> list[dict]:
            """The windows of the last encode, decoded once: greedy, or the best hypothesis of a beam search."""
            max_new = min(int(max_new_tokens) if max_new_tokens is not None else Tm // 2, Tm - 3)
            if beam_size == 1:
                res = self.decode(self._prompt(lang_id), len(seeks), max_new)
                rows, sums = res["tokens"], res["sum_logprob"]
            else:
                res = self.decode_beam(self._prompt(lang_id), len(seeks), max_new, beam_size, patience)
                pick = np.arange(len(seeks)), np.asarray(res["best"])
                rows, sums = np.asarray(res["tokens"])[pick], np.asarray(res["sum_logprob"])[pick]
            return [record(rows[k], sums[k], res["no_speech_prob"][k]) for k in range(len(seeks))]

        def decode_fallback(seeks: list[int]) -> list[dict]:
            """The temperature schedule over the windows of the last encode that still need another try."""
            temps, best_of = fb["temperature"], fb["best_of"]
            crt, lpt = fb["compression_ratio_threshold"], fb["log_prob_threshold"]
            sot_prev = d.get("sot_prev")
            if sot_prev is None:
                sot_prev = d["no_speech"] - 1   # <|startofprev|> sits right before <|nospeech|> in every Whisper vocabulary
            prompt, sot_index = self._prompt(lang_id), 0
            prev = all_tokens[reset:][-(Tm // 2 - 1):] if fb["condition_on_previous_text"] else []
            if prev:
                prompt, sot_index = [sot_prev] + prev + prompt, 1 + len(prev)
            max_new = min(Tm // 2, Tm - len(prompt))
            if max_new_tokens is not None:
                max_new = min(max_new, int(max_new_tokens))
            tried: list[list[dict]] = [[] for _ in seeks]
            accepted: list[dict | None] = [None] * len(seeks)
            pending = list(range(len(seeks)))
            for ti, temp in enumerate(temps):
                if not pending:
                    break
                rows = 1 if temp > 0 else beam_size
                per_call = max(1, MAX_LANES // (best_of if temp > 0 else rows))
                for i in range(0, len(pending), per_call):
                    part = pending[i:i + per_call]
                    windows = None if part == list(range(len(seeks))) else part
                    prompts = [prompt] * len(part)
                    if temp > 0:
                        seeds = [[lane_seed(fb["seed"], seeks[w], ti, g) for g in range(best_of)] for w in part]
                        res = self.decode_prompted(prompts, sot_index, max_new, windows=windows, group=best_of, temperature=temp,
                                                   seeds=seeds)
                    elif beam_size == 1:
                        res = self.decode_prompted(prompts, sot_index, max_new, windows=windows)
                    else:
                        res = self.decode_beam_prompted(prompts, sot_index, max_new, beam_size, patience, windows=windows)
                    for k, w in enumerate(part):
                        row = int(res["best"][k])
                        r = record(res["tokens"][k][row], res["sum_logprob"][k][row], res["no_speech_prob"][k], temperature=float(temp))
                        text = self.decoder.decode([t for t in takewhile(lambda t: t != eot, r["tokens"]) if t < eot])
                        tried[w].append({**r, "compression_ratio": compression_ratio(text)})
                still = []
                for w in pending:
                    r = tried[w][-1]
                    if needs_fallback(r["avg_logprob"], r["compression_ratio"], r["no_speech_prob"], crt, lpt):
                        still.append(w)
                    else:
                        accepted[w] = r
                pending = still
            for w in pending:
                accepted[w] = pick_fallback(tried[w], crt)
            return accepted

        def emit_all(accepted: list[dict], seeks: list[int]) -> int:
            """The segments of the windows of one encode; -> the frames the last of them advances by."""
            nonlocal reset
            code = d["lang_codes"][d["lang_ids"].index(lang_id)] if lang_id in d["lang_ids"] else language
            cut = []
            for w, (r, seek) in enumerate(zip(accepted, seeks)):
                size = min(self.window_frames, content_frames - seek)
                if r["no_speech_prob"] > NO_SPEECH_THRESHOLD and (threshold is None or r["avg_logprob"] < threshold):
                    cut.append((w, seek, size, None, size))
                    continue
                pieces, advance = cut_window(r["tokens"], eot, tb, seek * MS_PER_FRAME, size)
                cut.append((w, seek, size, pieces, advance))
            kept = [c for c in cut if c[3] is not None]
            words = None
            if word_timestamps and kept:
                words = dict(zip((c[0] for c in kept), self._window_words(
                    [(w, seek, size, [ids for _, _, ids in pieces]) for w, seek, size, pieces, _ in kept], lang_id, code)))
            for w, seek, size, pieces, advance in cut:
                r = accepted[w]
                figures = {k: r[k] for k in ("temperature", "avg_logprob", "compression_ratio")} if fb else {}
                if fb:
                    windows_log.append({"start_frame": seek, **figures, "no_speech_prob": r["no_speech_prob"]})
                if pieces is None:
                    continue
                for n, (start_ms, end_ms, ids) in enumerate(pieces):
                    text = self.decoder.decode(ids)
                    if start_ms == end_ms or (self.decoder._tokens and text.strip() == "") or not ids:
                        continue  # faster-whisper drops empty and zero-length segments
                    segments.append({"start_ms": int(start_ms), "end_ms": int(end_ms), "text": text, "language": code,
                                     "confidence": None, "words": words[w][n] if words is not None else None, "tokens": ids, **figures})
                if fb and fb["condition_on_previous_text"]:
                    all_tokens.extend(emitted_tokens(r["tokens"], eot, tb))
                    if r["temperature"] > fb["prompt_reset_on_temperature"]:
                        reset = len(all_tokens)
            _, _, size, _, advance = cut[-1]
            return max(1, min(advance, size)) if window_mode == "seek" else size

        def run(seeks: list[int]) -> int:
            nonlocal lang_id
            self.logmel([s * HOP for s in seeks], fetch=False)
            self.encode(len(seeks))
            if lang_id is None and d["lang_ids"]:  # language of the first window: argmax over the language ids after SOT
                lang_id = int(self.decode([d["sot"]], len(seeks), 0)["lang"][0])
            return emit_all((decode_fallback if fb else decode_plain)(seeks), seeks)

        if window_mode == "seek":
            seek = 0
            while seek < content_frames:
                seek += run([seek])
        else:
            starts = list(range(0, content_frames, self.window_frames))
            per_batch = max(1, int(batch_windows))
            if beam_size > 1:
                per_batch = min(per_batch, MAX_LANES // beam_size)
            for i in range(0, len(starts), per_batch):
                run(starts[i:i + per_batch])
        code = d["lang_codes"][d["lang_ids"].index(lang_id)] if lang_id in d["lang_ids"] else language
        return {"segments": segments, "language": code, **({"windows": windows_log} if fb else {})}


# the config under which transcribe_video decodes as the reference's WhisperModel.transcribe(path, language=..., vad_filter=...)
# does with faster-whisper's defaults
REFERENCE_CALL = {"beam_size": 5, "patience": 1.0, "temperature": list(REFERENCE_TEMPERATURES), "best_of": 5,
                  "compression_ratio_threshold": 2.4, "log_prob_threshold": -1.0, "condition_on_previous_text": True,
                  "prompt_reset_on_temperature": 0.5}


def transcribe_result(raw: dict) -> dict:
    """The reference's result dict (``model_manager.py:449-463``): exactly its six keys per segment."""
    keys = ("start_ms", "end_ms", "text", "language", "confidence")
    word_keys = ("word", "start", "end", "confidence")       # the reference's ``Word`` schema
    return {"segments": [{**{k: s[k] for k in keys},
                          "words": None if s["words"] is None else [{k: w[k] for k in word_keys} for w in s["words"]]}
                         for s in raw["segments"]]}


def transcribe_video(path: str, config: dict, *, transcriber, audio_source=None, vad=None, audio_frontend=None,
                     speakers=None) -> dict:
    """``ModelManager.transcribe_video`` body.  Config keys consumed: ``languages`` (string or list: the first entry; None =
    detect), ``vad_filter`` (applied when a ``vad`` object is given, see below), ``window_mode``, ``batch_windows``, ``beam_size`` (1..8, default 1 =
    greedy; 5 is the reference's call) and ``patience`` (positive, default 1.0); ``model_name`` picks the checkpoint in the
    caller.  ``beam_size`` / ``patience`` are passed to the transcriber only when the config sets them, and so are the
    temperature-fallback and conditioning keys of :func:`check_fallback` (``temperature``, ``best_of``,
    ``compression_ratio_threshold``, ``log_prob_threshold``, ``condition_on_previous_text``,
    ``prompt_reset_on_temperature``, ``seed``); the reference's call is :data:`REFERENCE_CALL`.  ``word_timestamps`` (a bool;
    anything else is a ``ValueError``) fills every segment's ``words`` with ``{"word", "start", "end", "confidence"}`` from the
    device's cross-attention alignment; it too is passed on only when the config sets it.

    ``vad``: an object with ``speech_probs(samples) -> probability per 512-sample chunk`` (:class:`eioku_amd.vad.SileroVad`).
    With it and ``config.get("vad_filter", True)`` (the reference's default), the transcriber sees the concatenation of the
    speech chunks of :func:`eioku_amd.vad.speech_timestamps` (``vad_parameters``: a dict of its six options) and the times
    are mapped back to the file; no speech returns no segments without a transcriber call.  Without ``vad`` the filter is
    logged and not applied.

    ``audio_frontend``: an object with ``load(path) -> (16 kHz samples, 16000)`` and ``resample_float(samples, rate)``
    (:class:`eioku_amd.audio.AudioFrontEnd`).  With it and no ``audio_source`` the audio comes from ``load``: PCM WAV of any
    rate, width and channel count; with both, a source whose rate is not 16000 goes through ``resample_float``.  Everything
    after it sees 16 kHz samples.  Without it any other rate raises, as before.

    ``speakers``: an object with ``label(samples, segments, eps=, min_samples=, assign_max=) -> one label or None per
    segment`` (:class:`eioku_amd.speakers.SpeakerLabeller`).  With it and ``config["speaker_labels"]`` true (a bool; anything
    else is a ``ValueError``) every segment gains a ``"speaker"`` key (``speaker_001`` ... by first appearance, ``None`` for a
    segment too short to embed or one no cluster claims); ``speaker_eps`` in (0, 2), ``speaker_min_samples`` >= 1 and
    ``speaker_assign_max`` in [0, 2] tune the clustering.  The labeller sees the file's own 16 kHz samples and file-time
    segments, also under VAD.  Without either the result is the reference's six keys and no speaker code runs."""
    config = config or {}
    use_speakers = False
    if "speaker_labels" in config:
        if not isinstance(config["speaker_labels"], bool):
            raise ValueError(f"speaker_labels must be a bool, got {config['speaker_labels']!r}")
        use_speakers = config["speaker_labels"] and speakers is not None
    if use_speakers:
        from .speakers import SPEAKER_KEYS, check_speaker_options

        speaker_options = check_speaker_options(**{k: config[k] for k in SPEAKER_KEYS if k in config})
    languages = config.get("languages")
    if isinstance(languages, (list, tuple)):
        languages = languages[0] if languages else None
    use_vad = vad is not None and bool(config.get("vad_filter", True))
    if use_vad:
        from . import vad as vad_mod

        vad_options = vad_mod.vad_options_from(config.get("vad_parameters"))
    elif config.get("vad_filter"):
        logger.info("vad_filter is accepted but not applied: Silero VAD is not built; the no-speech rule skips silence")
    beam = {}
    if "beam_size" in config or "patience" in config:
        b, pt = check_beam(config.get("beam_size", 1), config.get("patience", 1.0))
        if "beam_size" in config:
            beam["beam_size"] = b
        if "patience" in config:
            beam["patience"] = pt
    given = {k: config[k] for k in FALLBACK_KEYS if k in config}
    if given:
        fb = check_fallback(**given)
        if fb["condition_on_previous_text"] and config.get("window_mode", "seek") != "seek":
            raise ValueError("condition_on_previous_text needs window_mode 'seek': fixed windows decode in lockstep")
        given = {k: (list(fb[k]) if k == "temperature" else fb[k]) for k in given}
    if "word_timestamps" in config:
        given["word_timestamps"] = check_word_timestamps(config["word_timestamps"])
    if audio_frontend is not None and audio_source is None:
        samples, rate = audio_frontend.load(path)
    else:
        samples, rate = (audio_source or default_audio_source)(path)
        if audio_frontend is not None and int(rate) != SAMPLE_RATE:
            samples, rate = audio_frontend.resample_float(samples, rate), SAMPLE_RATE
    check_rate(rate)
    samples = np.asarray(samples, dtype=np.float32)
    file_samples = samples
    chunks = None
    if use_vad:
        samples = samples.reshape(-1)
        chunks = vad_mod.speech_timestamps(vad.speech_probs(samples), samples.size, vad_options)
        logger.info(f"VAD kept {sum(c['end'] - c['start'] for c in chunks) / SAMPLE_RATE:.2f} s of "
                    f"{samples.size / SAMPLE_RATE:.2f} s in {len(chunks)} chunks")
        if not chunks:
            return {"segments": []}
        samples = vad_mod.collect_chunks(samples, chunks)
    raw = transcriber.transcribe(samples, languages,
                                 window_mode=config.get("window_mode", "seek"),
                                 batch_windows=int(config.get("batch_windows", 8)), **beam, **given)
    if chunks is not None:
        raw = {**raw, "segments": vad_mod.restore_speech_timestamps(raw["segments"], chunks)}
    result = transcribe_result(raw)
    if use_speakers:
        labels = speakers.label(file_samples.reshape(-1), raw["segments"], **speaker_options)
        if len(labels) != len(result["segments"]):
            raise ValueError(f"{len(labels)} speaker labels for {len(result['segments'])} segments")
        for seg, label in zip(result["segments"], labels):
            seg["speaker"] = label
    return result
