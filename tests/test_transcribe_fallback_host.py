"""Temperature fallback and previous-text prompts, host side (no GPU): the loop of ``WhisperTranscriber.transcribe`` over a
scripted transcriber that records every device call and answers from a table keyed by (window start frame, temperature)."""
import asyncio

import numpy as np
import pytest

from eioku_amd import transcribe
from eioku_amd.model_manager import ModelManager

EOT, SOT, LANG, TASK, TB, SOT_PREV = 900, 901, 910, 950, 1000, 959
BASE = [SOT, LANG, TASK]
WINDOW = 3000                      # frames of one window
PLAIN = [TB, 5, 6, TB + 1500]      # " a b", one unpaired closing timestamp: one segment, seek advances by the whole window
LOOP = [TB] + [5] * 60 + [TB + 1500]


def _audio(windows: float) -> np.ndarray:
    return np.zeros(int(windows * WINDOW * transcribe.HOP), dtype=np.float32)


class Scripted(transcribe.WhisperTranscriber):
    """``script(seek, temperature) -> (tokens, sum_logprob, no_speech_prob)``; every sampled row of a window is the same."""

    def __init__(self, script, target_positions=448):
        self.dims = {"max_source_positions": WINDOW // 2, "max_target_positions": target_positions, "sot": SOT, "eot": EOT,
                     "transcribe": TASK, "timestamp_begin": TB, "lang_ids": [LANG], "lang_codes": ["en"], "no_speech": 960}
        self.decoder, self.window_frames, self.sync_every = transcribe.ByteDecoder({"Ġa": 5, "Ġb": 6}), WINDOW, 8
        self.script, self.calls, self.seeks = script, [], []

    def set_audio(self, samples):
        pass

    def logmel(self, offsets, fetch=True):
        self.seeks = [int(o) // transcribe.HOP for o in offsets]
        self.calls.append(("logmel", list(self.seeks)))

    def encode(self, n, mel=None):
        self.calls.append(("encode", n))

    def _rows(self, seeks, temperature, rows, max_new):
        toks = np.full((len(seeks), rows, max_new), EOT, dtype=np.int32)
        total, nsp = np.zeros((len(seeks), rows), dtype=np.float32), np.zeros(len(seeks), dtype=np.float32)
        for k, s in enumerate(seeks):
            t, lp, p = self.script(s, temperature)
            t = list(t)[:max_new]
            toks[k, :, :len(t)] = t
            total[k], nsp[k] = lp, p
        return toks, total, nsp

    def decode(self, prompt, n_windows, max_new_tokens, sync_every=None):
        self.calls.append(("decode", list(prompt), n_windows, max_new_tokens))
        toks, total, nsp = self._rows(self.seeks, 0.0, 1, max(max_new_tokens, 1))
        return {"tokens": toks[:, 0], "sum_logprob": total[:, 0], "no_speech_prob": nsp, "lang": np.full(n_windows, LANG)}

    def decode_beam(self, *a, **kw):
        raise AssertionError("not scripted")

    def decode_prompted(self, prompts, sot_index, max_new_tokens, *, windows=None, group=1, temperature=0.0, seeds=None,
                        sync_every=None):
        self.calls.append(("prompted", [list(p) for p in prompts], sot_index, max_new_tokens,
                           None if windows is None else list(windows), group, temperature,
                           None if seeds is None else [list(r) for r in seeds]))
        seeks = self.seeks if windows is None else [self.seeks[w] for w in windows]
        assert len(prompts) == len(seeks) and len({len(p) for p in prompts}) == 1
        toks, total, nsp = self._rows(seeks, temperature, group, max_new_tokens)
        return {"tokens": toks, "sum_logprob": total, "best": np.zeros(len(seeks), dtype=np.int32), "no_speech_prob": nsp}

    def decode_beam_prompted(self, prompts, sot_index, max_new_tokens, beam_size, patience=1.0, *, windows=None, sync_every=None,
                             trace=False):
        self.calls.append(("beam_prompted", [list(p) for p in prompts], sot_index, max_new_tokens,
                           None if windows is None else list(windows), beam_size, patience))
        seeks = self.seeks if windows is None else [self.seeks[w] for w in windows]
        toks, total, nsp = self._rows(seeks, 0.0, beam_size, max_new_tokens)
        return {"tokens": toks, "sum_logprob": total, "best": np.zeros(len(seeks), dtype=np.int32), "no_speech_prob": nsp}

    def prompted(self):
        return [c for c in self.calls if c[0] in ("prompted", "beam_prompted")]


def test_compression_ratio_of_a_looped_and_a_plain_string():
    looped = "thank you " * 40
    plain = "The committee met on Tuesday to review seven proposals, of which two were funded."
    assert transcribe.compression_ratio(looped) > 2.4 > transcribe.compression_ratio(plain) > 0.5
    import zlib
    assert transcribe.compression_ratio(looped) == len(looped) / len(zlib.compress(looped.encode()))


def test_a_looping_window_is_retried_at_the_next_temperature_and_the_retry_is_emitted():
    t = Scripted(lambda seek, temp: (LOOP, -3.0, 0.0) if temp == 0 else (PLAIN, -0.4, 0.0))
    out = t.transcribe(_audio(1), "en", temperature=[0.0, 0.2, 0.4])
    calls = t.prompted()
    assert [(c[0], c[5], c[6]) for c in calls] == [("prompted", 1, 0.0), ("prompted", 5, 0.2)]    # beam 1 at T 0, best_of 5 after
    assert calls[0][7] is None and len(calls[1][7][0]) == 5
    assert sum(c[0] == "encode" for c in t.calls) == 1                                            # a retry does not encode again
    (seg,) = out["segments"]
    assert seg["text"] == " a b" and seg["temperature"] == 0.2 and seg["tokens"] == [5, 6]
    assert seg["avg_logprob"] == pytest.approx(-0.4 / 5) and seg["compression_ratio"] == transcribe.compression_ratio(" a b")
    assert (seg["start_ms"], seg["end_ms"]) == (0, 30000)


def test_beam_size_applies_at_temperature_zero_only():
    t = Scripted(lambda seek, temp: (PLAIN, -9.0, 0.0) if temp == 0 else (PLAIN, -0.4, 0.0))
    t.transcribe(_audio(1), "en", temperature=[0.0, 0.2], beam_size=5, best_of=3)
    a, b = t.prompted()
    assert (a[0], a[5], a[6]) == ("beam_prompted", 5, 1.0) and (b[0], b[5], b[6]) == ("prompted", 3, 0.2)


def test_the_silence_case_does_not_retry():
    t = Scripted(lambda seek, temp: (PLAIN, -20.0, 0.9))          # average -4 < -1, but no_speech_prob > 0.6
    out = t.transcribe(_audio(1), "en", temperature=[0.0, 0.2, 0.4])
    assert len(t.prompted()) == 1 and out["segments"] == []       # one try, and the no-speech rule then skips the window
    t = Scripted(lambda seek, temp: (PLAIN, -20.0, 0.5))          # the same average without the no-speech mass: every temperature
    t.transcribe(_audio(1), "en", temperature=[0.0, 0.2, 0.4])
    assert len(t.prompted()) == 3


def test_when_every_temperature_fails_the_best_average_within_the_compression_threshold_is_kept():
    table = {0.0: (PLAIN, -10.0, 0.0), 0.2: (PLAIN, -7.0, 0.0), 0.4: (PLAIN, -15.0, 0.0)}
    t = Scripted(lambda seek, temp: table[temp])
    (seg,) = t.transcribe(_audio(1), "en", temperature=[0.0, 0.2, 0.4])["segments"]
    assert seg["temperature"] == 0.2 and seg["avg_logprob"] == pytest.approx(-7.0 / 5)
    # the loop has the best average (-62 / 63) but is beyond the compression threshold: the plain try wins
    table = {0.0: (LOOP, -62.5, 0.0), 0.2: (PLAIN, -7.0, 0.0), 0.4: (PLAIN, -6.0, 0.0)}
    t = Scripted(lambda seek, temp: table[temp])
    (seg,) = t.transcribe(_audio(1), "en", temperature=[0.0, 0.2, 0.4], log_prob_threshold=-0.5)["segments"]
    assert seg["temperature"] == 0.4
    # and with no try within it, the best average of all
    table = {0.0: (LOOP, -70.0, 0.0), 0.2: (LOOP, -65.0, 0.0)}
    t = Scripted(lambda seek, temp: table[temp])
    (seg,) = t.transcribe(_audio(1), "en", temperature=[0.0, 0.2])["segments"]
    assert seg["temperature"] == 0.2
    assert transcribe.pick_fallback([{"avg_logprob": -1.0, "compression_ratio": 1.0, "k": 0},
                                     {"avg_logprob": -1.0, "compression_ratio": 1.0, "k": 1}], 2.4)["k"] == 0


def test_prompt_construction_sot_prev_truncation_sot_index_and_the_max_new_clamp():
    long = [TB] + [5, 6] * 111 + [TB + 1500]                       # 224 sampled ids, none of them EOT
    t = Scripted(lambda seek, temp: (PLAIN, -0.4, 0.0) if seek == 0 else (long, -2.0, 0.0))
    t.transcribe(_audio(3), "en", condition_on_previous_text=True, compression_ratio_threshold=None)
    w1, w2, w3 = t.prompted()
    assert (w1[1], w1[2], w1[3]) == ([BASE], 0, 224)                                       # nothing before the first window
    assert (w2[1], w2[2], w2[3]) == ([[SOT_PREV] + PLAIN + BASE], 5, 224)                  # timestamps included, EOT not
    prev = (PLAIN + long)[-223:]
    assert len(prev) == 223 and w3[1] == [[SOT_PREV] + prev + BASE]
    assert len(w3[1][0]) == 227 and w3[2] == 224 and w3[3] == 448 - 227                    # max_new = min(224, 448 - P)
    assert [c[1] for c in t.calls if c[0] == "logmel"] == [[0], [WINDOW], [2 * WINDOW]]
    assert not [c for c in t.calls if c[0] == "decode"]                                    # the language was given
    # sot_prev from the generation config when it names one; test model A's layout gives no_speech - 1 = 899
    gen = {"no_timestamps_token_id": 901, "lang_to_id": {}, "task_to_id": {}, "decoder_start_token_id": 891, "eos_token_id": 890}
    cfg = {"d_model": 128, "encoder_attention_heads": 2, "encoder_layers": 1, "decoder_layers": 1, "encoder_ffn_dim": 64,
           "decoder_ffn_dim": 64, "vocab_size": 1003, "max_source_positions": 100, "max_target_positions": 64}
    assert transcribe.whisper_dims(cfg, gen)["sot_prev"] == 899
    assert transcribe.whisper_dims(cfg, dict(gen, prev_sot_token_id=50361))["sot_prev"] == 50361
    # a small decoder: 64 positions keep 31 previous tokens, P = 35, max_new = min(32, 29)
    t = Scripted(lambda seek, temp: ([TB] + [5, 6] * 15 + [TB + 1500], -2.0, 0.0), target_positions=64)
    t.transcribe(_audio(2), "en", condition_on_previous_text=True, compression_ratio_threshold=None)
    w1, w2 = t.prompted()
    assert w1[3] == 32 and len(w2[1][0]) == 35 and w2[2] == 32 and w2[3] == 29


def test_language_detection_keeps_its_own_sot_call():
    t = Scripted(lambda seek, temp: (PLAIN, -0.4, 0.0))
    t.transcribe(_audio(1), None, temperature=[0.0, 0.2])
    assert [c for c in t.calls if c[0] == "decode"] == [("decode", [SOT], 1, 0)]


def test_the_prompt_is_reset_after_a_window_accepted_above_the_reset_temperature():
    def script(seek, temp):
        return (PLAIN, -9.0, 0.0) if (seek == 0 and temp == 0) else (PLAIN, -0.4, 0.0)

    t = Scripted(script)
    t.transcribe(_audio(2), "en", condition_on_previous_text=True, temperature=[0.0, 0.6])
    assert t.prompted()[-1][1] == [BASE]                           # window 1 was accepted at 0.6 > 0.5: nothing is carried
    t = Scripted(script)
    t.transcribe(_audio(2), "en", condition_on_previous_text=True, temperature=[0.0, 0.4])
    assert t.prompted()[-1][1] == [[SOT_PREV] + PLAIN + BASE]      # accepted at 0.4: carried
    t = Scripted(script)
    t.transcribe(_audio(2), "en", condition_on_previous_text=True, temperature=[0.0, 0.4], prompt_reset_on_temperature=0.3)
    assert t.prompted()[-1][1] == [BASE]


def test_fixed_mode_with_conditioning_raises():
    t = Scripted(lambda seek, temp: (PLAIN, -0.4, 0.0))
    with pytest.raises(ValueError):
        t.transcribe(_audio(1), "en", window_mode="fixed", condition_on_previous_text=True)
    with pytest.raises(ValueError):
        _video({"window_mode": "fixed", "condition_on_previous_text": True}, _Fake())
    t.transcribe(_audio(1), "en", window_mode="fixed", condition_on_previous_text=False)


class _Fake:
    def __init__(self):
        self.kw = None

    def transcribe(self, samples, language, **kw):
        self.kw = kw
        return {"language": "en", "segments": []}


def _video(config, fake):
    mm = ModelManager(cache_dir="/tmp", gpu_transcription=True, transcriber_factory=lambda cache, name: fake,
                      audio_source=lambda path: (np.zeros(1600, dtype=np.float32), 16000))
    return asyncio.run(mm.transcribe_video("v.mp4", config))


BAD = {"temperature": [-0.1, "0.2", None, [], [0.0, -1.0], [0.0, "x"], float("nan"), True],
       "best_of": [0, 9, 2.5, "5", None, True],
       "compression_ratio_threshold": [0, -1.0, "2.4", float("inf"), True],
       "log_prob_threshold": ["-1", float("nan"), False],
       "condition_on_previous_text": [1, "yes", None],
       "prompt_reset_on_temperature": [-0.5, None, "0.5"],
       "seed": [-1, 1.5, "0", None, 1 << 64, True]}


@pytest.mark.parametrize("key", sorted(BAD))
def test_every_new_key_rejects_bad_values(key):
    fake = _Fake()
    for bad in BAD[key]:
        with pytest.raises(ValueError):
            _video({key: bad}, fake)
        with pytest.raises(ValueError):
            Scripted(lambda seek, temp: (PLAIN, -0.4, 0.0)).transcribe(_audio(1), "en", **{key: bad})
    assert fake.kw is None


def test_good_values_reach_the_transcriber_only_when_the_config_sets_them():
    fake = _Fake()
    _video({"temperature": 0.2, "seed": 7, "log_prob_threshold": None}, fake)
    assert fake.kw == {"window_mode": "seek", "batch_windows": 8, "temperature": [0.2], "seed": 7, "log_prob_threshold": None}
    _video(dict(transcribe.REFERENCE_CALL), fake)
    assert fake.kw == {"window_mode": "seek", "batch_windows": 8, "beam_size": 5, "patience": 1.0,
                       "temperature": [0.0, 0.2, 0.4, 0.6, 0.8, 1.0], "best_of": 5, "compression_ratio_threshold": 2.4,
                       "log_prob_threshold": -1.0, "condition_on_previous_text": True, "prompt_reset_on_temperature": 0.5}
    with pytest.raises(TypeError):
        Scripted(lambda seek, temp: (PLAIN, -0.4, 0.0)).transcribe(_audio(1), "en", temperatures=[0.0])


def test_with_no_new_key_the_device_calls_are_todays():
    t = Scripted(lambda seek, temp: (LOOP, -300.0, 0.0))           # a loop with a poor average: still one greedy call per window
    out = t.transcribe(_audio(2), "en")
    assert t.calls == [("logmel", [0]), ("encode", 1), ("decode", BASE, 1, 224),
                       ("logmel", [WINDOW]), ("encode", 1), ("decode", BASE, 1, 224)]
    assert len(out["segments"]) == 2
    assert set(out["segments"][0]) == {"start_ms", "end_ms", "text", "language", "confidence", "words", "tokens"}
    fake = _Fake()
    _video({}, fake)
    assert fake.kw == {"window_mode": "seek", "batch_windows": 8}


def test_the_seed_derivation_is_independent_of_batching():
    def script(seek, temp):
        return (PLAIN, -9.0, 0.0) if temp == 0 else (PLAIN, -0.4, 0.0)

    def seeds_by_window(mode, batch):
        t = Scripted(script)
        out = t.transcribe(_audio(3), "en", window_mode=mode, batch_windows=batch, temperature=[0.0, 0.2], best_of=3, seed=11)
        got, seeks = {}, []
        for c in t.calls:
            if c[0] == "logmel":
                seeks = c[1]
            if c[0] == "prompted" and c[6] > 0:
                rows = seeks if c[4] is None else [seeks[w] for w in c[4]]
                got.update({s: tuple(r) for s, r in zip(rows, c[7])})
        return got, out

    a, out_a = seeds_by_window("seek", 8)
    b, out_b = seeds_by_window("fixed", 2)
    c, out_c = seeds_by_window("fixed", 8)
    assert sorted(a) == [0, WINDOW, 2 * WINDOW] and a == b == c and out_a == out_b == out_c
    flat = [s for rows in a.values() for s in rows]
    assert len(set(flat)) == 9 and all(0 <= s < 1 << 64 for s in flat)
    assert a[WINDOW] == tuple(transcribe.lane_seed(11, WINDOW, 1, g) for g in range(3))
    assert transcribe.lane_seed(11, WINDOW, 1, 0) != transcribe.lane_seed(12, WINDOW, 1, 0)
    assert transcribe.lane_seed(11, WINDOW, 1, 0) != transcribe.lane_seed(11, WINDOW, 2, 0)


def test_a_fixed_batch_retries_only_the_windows_that_failed():
    t = Scripted(lambda seek, temp: (PLAIN, -9.0, 0.0) if (temp == 0 and seek in (0, 2 * WINDOW)) else (PLAIN, -0.4, 0.0))
    out = t.transcribe(_audio(3), "en", window_mode="fixed", batch_windows=4, temperature=[0.0, 0.2])
    first, retry = t.prompted()
    assert first[4] is None and len(first[1]) == 3 and retry[4] == [0, 2] and len(retry[1]) == 2
    assert [s["temperature"] for s in out["segments"]] == [0.2, 0.0, 0.2]
    # 20 windows x best_of 5 do not fit the 64 lanes: the sampled retry is split into calls of at most 12 windows
    t = Scripted(lambda seek, temp: (PLAIN, -9.0, 0.0) if temp == 0 else (PLAIN, -0.4, 0.0))
    t.transcribe(_audio(20), "en", window_mode="fixed", batch_windows=20, temperature=[0.0, 0.2])
    assert [len(c[1]) for c in t.prompted()] == [20, 12, 8]
