"""K21 host side (no GPU): the oracle's median filter and DTW and the product's word rules against
tests/golden/whisper_align_hf.json (written by tests/golden/make_whisper_align_fixture.py from the installed
``transformers``), the hand-out of words to segments, the ``word_timestamps`` key and ``alignment_heads``."""
import asyncio
import json

import numpy as np
import pytest

import whisper_align_oracle as wa
from conftest import GOLDEN
from eioku_amd import transcribe
from eioku_amd.model_manager import ModelManager

FIX = json.loads((GOLDEN / "whisper_align_hf.json").read_text())


def _decoder():
    inv = {b: ch for ch, b in transcribe._gpt2_byte_table().items()}
    return transcribe.ByteDecoder({"".join(inv[b] for b in bytes.fromhex(h)): int(i) for i, h in FIX["vocab"].items()})


# ---- the oracle against transformers ---------------------------------------------------------------------------------------------
def test_the_fixture_covers_the_edge_shapes():
    shapes = {(c["name"], c["N"], c["F"]) for c in FIX["dtw"]}
    assert {("zeros", 5, 7), ("levels", 8, 11), ("random", 1, 6), ("random", 6, 1), ("random", 4, 3), ("random", 1, 1)} <= shapes
    assert {c["shape"][-1] for c in FIX["median"]} >= {1, 3, 4, 7}


@pytest.mark.parametrize("case", FIX["median"], ids=lambda c: "x".join(map(str, c["shape"])))
def test_oracle_median_filter_equals_transformers(case):
    x = np.asarray(case["x"], dtype=np.float32).reshape(case["shape"])
    want = np.asarray(case["y"], dtype=np.float32).reshape(case["shape"])
    assert np.array_equal(wa.median_filter(x, FIX["filter_width"]), want)
    if case["shape"][-1] <= 3:
        assert np.array_equal(want, x)                              # the filter is skipped


@pytest.mark.parametrize("case", FIX["dtw"], ids=lambda c: f"{c['name']}-{c['N']}x{c['F']}")
def test_oracle_dtw_equals_transformers(case):
    cost = np.asarray(case["cost"], dtype=np.float32).reshape(case["N"], case["F"])
    ti, fi = wa.dtw(cost)
    assert ti.tolist() == case["text_idx"] and fi.tolist() == case["time_idx"]
    jump = wa.jumps(ti, fi, case["N"])
    # Whisper's own reading of the path: the frames at which the token index changes
    change = np.pad(np.diff(np.asarray(case["text_idx"])), (1, 0), constant_values=1).astype(bool)
    assert jump.tolist() == np.asarray(case["time_idx"])[change].tolist()


def test_oracle_cost_is_the_negated_head_mean_of_the_filtered_z_scores():
    a = np.random.default_rng(3).random((2, 6, 9))
    z = (a - a.mean(axis=1, keepdims=True)) / a.std(axis=1, keepdims=True)
    want = -np.stack([wa.median_filter(z[h]) for h in range(2)]).mean(axis=0)[2:-1]
    assert np.array_equal(wa.cost_from_weights(a, 2), want) and want.shape == (3, 9)


# ---- the product's word rules against transformers ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FIX["split"], ids=lambda c: f"{c['language']}-{len(c['ids'])}")
def test_word_split_and_punctuation_merge_equal_transformers(case):
    dec = _decoder()
    words, tokens = transcribe._split_on_unicode(case["ids"], dec)
    assert words == case["unicode"]["words"] and tokens == case["unicode"]["tokens"]
    words, tokens = transcribe.split_to_word_tokens(case["ids"], dec, case["language"], FIX["eot"])
    assert words == case["split"]["words"] and tokens == case["split"]["tokens"]
    if "merged" in case:
        merged = transcribe.merge_punctuations([{"word": w, "tokens": t} for w, t in zip(words, tokens)])
        assert [w["word"] for w in merged] == case["merged"]["words"]
        assert [w["tokens"] for w in merged] == case["merged"]["tokens"]
        assert sum(len(w["tokens"]) for w in merged) == len(case["ids"])


def test_the_fixture_exercises_every_rule():
    by_lang = {c["language"]: c for c in reversed(FIX["split"]) if "merged" in c}      # the first case of each language
    en = by_lang["en"]
    assert " café" in en["split"]["words"]                          # é arrives as two tokens
    assert " (aside)" in en["merged"]["words"] and " Hello," in en["merged"]["words"]     # leading and trailing punctuation
    assert by_lang["ja"]["split"]["words"][:2] == ["中", "文"]        # no-space language: the unicode split alone
    assert transcribe.PREPEND_PUNCTUATIONS == FIX["prepend"] and transcribe.APPEND_PUNCTUATIONS == FIX["append"]


# ---- words to segments -----------------------------------------------------------------------------------------------------------
def test_words_go_to_the_segments_by_token_count():
    dec = _decoder()
    pieces = [[0, 1, 2, 3], [8, 9, 10, 16, 22, 21]]                 # " Hello, world!" | " café. it's"
    jump = [5, 9, 12, 20, 30, 34, 34, 35, 40, 44, 50]               # 10 text rows + the EOT row
    prob = [0.5, 1.0, 0.25, 0.75, 0.9, 0.8, 0.7, 1.0, 1.2, 1.0]
    per_seg = transcribe.window_words(pieces, jump, prob, 3000, dec, "en", FIX["eot"])
    assert [[w["word"] for w in seg] for seg in per_seg] == [[" Hello,", " world!"], [" café.", " it's"]]
    assert [[len(w["tokens"]) for w in seg] for seg in per_seg] == [[2, 2], [4, 2]]
    flat = [w for seg in per_seg for w in seg]
    want = wa.word_times([2, 2, 4, 2], jump, prob, 3000)
    for w, (start_ms, end_ms, conf) in zip(flat, want):
        assert (w["start_ms"], w["end_ms"]) == (start_ms, end_ms) and w["start"] == start_ms / 1000 and w["end"] == end_ms / 1000
        assert w["confidence"] == pytest.approx(min(1.0, conf))
    assert flat[0]["start_ms"] == 3100 and flat[-1]["end_ms"] == 4000          # the EOT row ends the last word
    assert flat[2]["confidence"] == pytest.approx(0.85) and flat[3]["confidence"] == 1.0     # mean 1.1, clipped
    assert all(0.0 <= w["confidence"] <= 1.0 for w in flat)
    # a word that straddles the segments' token counts stays with the segment that started it
    per_seg = transcribe.window_words([[0, 1, 2], [3, 8]], [0, 1, 2, 3, 4, 5], [0.5] * 5, 0, dec, "en", FIX["eot"])
    assert [[w["word"] for w in seg] for seg in per_seg] == [[" Hello,", " world!"], [" caf"]]


def test_transcribe_result_keeps_six_keys_and_the_word_schema():
    word = {"word": " a", "start": 1.0, "end": 1.5, "confidence": 0.5, "start_ms": 1000, "end_ms": 1500, "tokens": [5]}
    raw = {"segments": [{"start_ms": 0, "end_ms": 2000, "text": " a", "language": "en", "confidence": None, "words": [word],
                         "tokens": [5]},
                        {"start_ms": 2000, "end_ms": 3000, "text": " b", "language": "en", "confidence": None, "words": None,
                         "tokens": [6]}]}
    out = transcribe.transcribe_result(raw)["segments"]
    assert [list(s) for s in out] == [["start_ms", "end_ms", "text", "language", "confidence", "words"]] * 2
    assert out[0]["words"] == [{"word": " a", "start": 1.0, "end": 1.5, "confidence": 0.5}] and out[1]["words"] is None


# ---- the key ---------------------------------------------------------------------------------------------------------------------
class _Scripted(transcribe.WhisperTranscriber):
    """Three 30 s windows, each decoding to <0.00> " a" " b" <2.00><2.00> " b" <4.00>; ``align`` is scripted too."""

    def __init__(self):
        self.dims = {"max_source_positions": 1500, "max_target_positions": 448, "sot": 901, "eot": 900, "transcribe": 950,
                     "timestamp_begin": 1000, "lang_ids": [910], "lang_codes": ["en"], "no_speech": 960, "no_timestamps": 999}
        self.decoder, self.window_frames, self.sync_every, self.calls = transcribe.ByteDecoder({"Ġa": 5, "Ġb": 6}), 3000, 8, []

    def set_audio(self, samples):
        pass

    def logmel(self, offsets, fetch=True):
        pass

    def encode(self, n, mel=None):
        self.calls.append(("encode", n))

    def decode(self, prompt, n_windows, max_new_tokens, sync_every=None):
        toks = np.full((n_windows, max_new_tokens), 900, dtype=np.int32)
        toks[:, :7] = [1000, 5, 6, 1100, 1100, 6, 1200]
        return {"tokens": toks, "sum_logprob": np.full(n_windows, -1.0, dtype=np.float32),
                "no_speech_prob": np.zeros(n_windows, dtype=np.float32)}

    def align(self, seqs, n_tok, sot_len, n_frames, windows=None, cost=False):
        self.calls.append(("align", [list(map(int, s)) for s in seqs], list(n_tok), sot_len, list(n_frames), list(windows)))
        R, N = len(seqs), len(seqs[0]) - sot_len - 1
        return {"jump": np.tile(np.arange(N, dtype=np.int32) * 10, (R, 1)), "prob": np.full((R, N), 0.5, dtype=np.float32)}


def test_transcribe_aligns_once_per_window_in_seek_mode_and_once_per_batch_in_fixed_mode():
    audio = np.zeros(16000 * 75, dtype=np.float32)                  # 7500 frames: fixed windows 3000 + 3000 + 1500
    plain = _Scripted()
    base = plain.transcribe(audio, "en", window_mode="fixed", batch_windows=2)
    assert not [c for c in plain.calls if c[0] == "align"] and all(s["words"] is None for s in base["segments"])
    t = _Scripted()
    out = t.transcribe(audio, "en", window_mode="fixed", batch_windows=2, word_timestamps=True)
    aligns = [c for c in t.calls if c[0] == "align"]
    seq = [901, 910, 950, 999, 5, 6, 6, 900]
    assert aligns == [("align", [seq, seq], [8, 8], 3, [3000, 3000], [0, 1]), ("align", [seq], [8], 3, [1500], [0])]
    strip = lambda segs: [{k: v for k, v in s.items() if k != "words"} for s in segs]       # noqa: E731
    assert strip(out["segments"]) == strip(base["segments"]) and len(out["segments"]) == 6
    first, second = out["segments"][0]["words"], out["segments"][1]["words"]
    assert [w["word"] for w in first] == [" a", " b"] and [w["word"] for w in second] == [" b"]
    assert [(w["start_ms"], w["end_ms"]) for w in first + second] == [(0, 200), (200, 400), (400, 600)]
    assert out["segments"][2]["words"][0]["start_ms"] == 30000      # the second window's words start at its first frame
    s = _Scripted()
    seek_out = s.transcribe(audio, "en", word_timestamps=True)      # seek mode: every window advances to <4.00> = 400 frames
    aligns = [c for c in s.calls if c[0] == "align"]
    assert len(aligns) == len([c for c in s.calls if c[0] == "encode"]) and all(len(c[1]) == 1 and c[5] == [0] for c in aligns)
    assert all(isinstance(seg["words"], list) for seg in seek_out["segments"])
    plain_seek = _Scripted().transcribe(audio, "en")
    assert strip(seek_out["segments"]) == strip(plain_seek["segments"])


@pytest.mark.parametrize("bad", [1, 0, "true", None, 1.0, [True]])
def test_word_timestamps_must_be_a_bool(bad):
    with pytest.raises(ValueError, match="word_timestamps"):
        _Scripted().transcribe(np.zeros(16000, dtype=np.float32), "en", word_timestamps=bad)
    with pytest.raises(ValueError, match="word_timestamps"):
        _video({"word_timestamps": bad}, _Stub())


class _Stub:
    def __init__(self):
        self.kw, self.aligned = None, 0

    def align(self, *a, **kw):
        self.aligned += 1
        raise AssertionError("a config without word_timestamps must not align")

    def transcribe(self, samples, language, **kw):
        self.kw = kw
        words = [{"word": " a", "start": 0.1, "end": 0.3, "confidence": 0.5, "start_ms": 100, "end_ms": 300, "tokens": [5]}]
        return {"language": "en", "segments": [{"start_ms": 0, "end_ms": 1000, "text": " a", "language": "en", "confidence": None,
                                                "words": words if kw.get("word_timestamps") else None, "tokens": [5]}]}


def _video(config, stub):
    mm = ModelManager(cache_dir="/tmp", gpu_transcription=True, transcriber_factory=lambda cache, name: stub,
                      audio_source=lambda path: (np.zeros(1600, dtype=np.float32), 16000))
    return asyncio.run(mm.transcribe_video("v.mp4", config))


def test_transcribe_video_passes_the_key_only_when_the_config_sets_it():
    stub = _Stub()
    out = _video({}, stub)
    assert stub.kw == {"window_mode": "seek", "batch_windows": 8} and stub.aligned == 0
    assert out["segments"][0]["words"] is None
    out = _video({"word_timestamps": True}, stub)
    assert stub.kw == {"window_mode": "seek", "batch_windows": 8, "word_timestamps": True}
    assert out["segments"][0]["words"] == [{"word": " a", "start": 0.1, "end": 0.3, "confidence": 0.5}]
    _video({"word_timestamps": False}, stub)
    assert stub.kw["word_timestamps"] is False


def test_a_transcriber_without_the_key_never_aligns():
    class NoAlign(_Scripted):
        def align(self, *a, **kw):
            raise AssertionError("align called without word_timestamps")

    mm = ModelManager(cache_dir="/tmp", gpu_transcription=True, transcriber_factory=lambda cache, name: NoAlign(),
                      audio_source=lambda path: (np.zeros(16000 * 5, dtype=np.float32), 16000))
    out = asyncio.run(mm.transcribe_video("v.mp4", {"languages": ["en"]}))
    assert out["segments"] and all(s["words"] is None for s in out["segments"])


# ---- alignment heads ---------------------------------------------------------------------------------------------------------------
def test_whisper_dims_reads_alignment_heads():
    config = {"d_model": 128, "encoder_attention_heads": 2, "encoder_layers": 2, "decoder_layers": 2, "encoder_ffn_dim": 512,
              "decoder_ffn_dim": 512, "vocab_size": 1003, "max_source_positions": 100, "max_target_positions": 64,
              "decoder_start_token_id": 891, "eos_token_id": 890}
    gen = {"no_timestamps_token_id": 901}
    assert transcribe.whisper_dims(config, gen)["alignment_heads"] is None
    dims = transcribe.whisper_dims(config, dict(gen, alignment_heads=[[1, 0], [0, 1]]))
    assert dims["alignment_heads"] == [[1, 0], [0, 1]]
