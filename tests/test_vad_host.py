"""K22 host side (no GPU): speech_timestamps on hand-worked cases, the timestamp map, option checks, and the wiring of
``vad`` through ``transcribe_video``, ``ModelManager`` and ``process_ml_task`` with fakes."""
import asyncio
import logging
import math

import numpy as np
import pytest

from eioku_amd import task_handler, transcribe, vad
from eioku_amd.model_manager import ModelManager

N200 = 200 * 512


def _probs(n, *runs):
    p = np.full(n, 0.1)
    for a, b in runs:
        p[a:b + 1] = 0.9
    return p


def _spans(chunks):
    return [(c["start"], c["end"]) for c in chunks]


# ---- speech_timestamps ----------------------------------------------------------------------------------------------------
def test_two_bursts_far_apart_are_padded_by_400_ms():
    # (5120, 10240) and (51200, 56320) before padding; the silence between them exceeds 2 x 6400 samples
    assert _spans(vad.speech_timestamps(_probs(200, (10, 19), (100, 109)), N200)) == [(0, 16640), (44800, 62720)]


def test_a_gap_shorter_than_min_silence_is_bridged():
    # chunks 20..39 are 640 ms of silence < 2000 ms: one speech (5120, 25600), padded to (0, 32000)
    assert _spans(vad.speech_timestamps(_probs(200, (10, 19), (40, 49)), N200)) == [(0, 32000)]


def test_a_short_gap_between_two_speeches_is_shared_in_halves():
    o = vad.VadOptions(min_silence_duration_ms=100)
    # (5120, 10240) and (15360, 20480): 5120 samples of silence < 2 x 6400 -> 2560 to each side
    assert _spans(vad.speech_timestamps(_probs(200, (10, 19), (30, 39)), N200, o)) == [(0, 12800), (12800, 26880)]


def test_nothing_above_the_threshold_gives_no_chunks():
    assert vad.speech_timestamps(np.full(200, 0.49), N200) == []


def test_speech_running_to_the_last_chunk_ends_at_n_samples():
    out = vad.speech_timestamps(_probs(200, (150, 199)), N200 - 37)
    assert _spans(out) == [(150 * 512 - 6400, N200 - 37)]


def test_neg_threshold_default_and_override():
    p = np.full(200, 0.1)
    p[10:20] = 0.9
    p[20:] = 0.4            # between 0.35 and 0.5: never ends the speech under the default neg_threshold
    assert _spans(vad.speech_timestamps(p, N200)) == [(0, N200)]
    o = vad.VadOptions(neg_threshold=0.45)
    assert _spans(vad.speech_timestamps(p, N200, o)) == [(0, 16640)]


def test_min_speech_duration_drops_short_speeches():
    o = vad.VadOptions(min_speech_duration_ms=400)          # 6400 samples
    assert _spans(vad.speech_timestamps(_probs(200, (10, 19), (100, 119)), N200, o)) == [(44800, 67840)]


@pytest.mark.parametrize("seed", range(8))
def test_chunks_are_ordered_disjoint_in_range_and_bounded(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(50, 400))
    # runs of speech and silence of random lengths, with noise across both thresholds
    p = np.repeat(rng.random(n // 5 + 1), 5)[:n] * 0.6 + rng.random(n) * 0.4
    n_samples = n * 512 - int(rng.integers(0, 512))
    max_s = float(rng.choice([1.0, 1.5, 3.0]))
    o = vad.VadOptions(max_speech_duration_s=max_s, min_silence_duration_ms=int(rng.choice([0, 64, 500])),
                       speech_pad_ms=int(rng.choice([0, 30, 100])))
    chunks = vad.speech_timestamps(p, n_samples, o)
    assert chunks, "the sequence should contain speech"
    previous_end = 0
    for c in chunks:
        assert 0 <= c["start"] < c["end"] <= n_samples
        assert c["start"] >= previous_end
        assert c["end"] - c["start"] <= 16000 * max_s
        previous_end = c["end"]


# ---- options --------------------------------------------------------------------------------------------------------------
def test_options_defaults_are_faster_whispers():
    o = vad.check_vad_options()
    assert (o.threshold, o.neg_threshold, o.min_speech_duration_ms, o.max_speech_duration_s, o.min_silence_duration_ms,
            o.speech_pad_ms) == (0.5, None, 0, math.inf, 2000, 400)
    assert vad.vad_options_from(None) == o and vad.vad_options_from({"speech_pad_ms": 30}).speech_pad_ms == 30


@pytest.mark.parametrize("bad", [{"threshold": 0.0}, {"threshold": 1.0}, {"threshold": "0.5"}, {"threshold": True},
                                 {"neg_threshold": 1.5}, {"min_speech_duration_ms": -1}, {"min_speech_duration_ms": 2.5},
                                 {"min_silence_duration_ms": None}, {"speech_pad_ms": float("inf")},
                                 {"max_speech_duration_s": 0}, {"max_speech_duration_s": float("nan")}, {"window_size": 512}])
def test_bad_options_raise(bad):
    with pytest.raises(ValueError):
        vad.vad_options_from(bad)
    with pytest.raises(ValueError):
        vad.vad_options_from([0.5])


# ---- the map back to file time --------------------------------------------------------------------------------------------
CASE1 = [{"start": 0, "end": 16640}, {"start": 44800, "end": 62720}]


def test_map_round_trip_on_the_first_worked_case():
    m = vad.SpeechTimestampsMap(CASE1)
    assert m.silence_before == [0, 28160] and m.chunk_end == [16640, 34560]
    assert m.original_ms(0) == 0
    assert m.original_ms(1040, is_end=True) == 1040       # the end of the first chunk stays in the first chunk
    assert m.original_ms(1040) == 2800                    # as a start it is the start of the second
    assert m.original_ms(2160, is_end=True) == 3920
    assert m.original_ms(5000) == 5000 + 1760             # past the end: the last chunk


def test_map_refuses_chunks_off_the_millisecond_grid():
    with pytest.raises(ValueError):
        vad.SpeechTimestampsMap([{"start": 5, "end": 100}])


def test_collect_chunks_concatenates():
    x = np.arange(70000, dtype=np.float32)
    got = vad.collect_chunks(x, CASE1)
    assert got.dtype == np.float32 and np.array_equal(got, np.concatenate([x[0:16640], x[44800:62720]]))
    assert vad.collect_chunks(x, []).size == 0


def _seg(start_ms, end_ms, words=None):
    return {"start_ms": start_ms, "end_ms": end_ms, "text": " x", "language": "en", "confidence": None, "tokens": [1],
            "words": None if words is None else [{"word": f" w{i}", "start": a / 1000, "end": b / 1000, "confidence": 0.5,
                                                  "start_ms": a, "end_ms": b, "tokens": [i]} for i, (a, b) in enumerate(words)]}


def test_restore_without_words_maps_start_and_end_separately():
    segs = [_seg(0, 1040), _seg(1040, 2160)]
    out = vad.restore_speech_timestamps(segs, CASE1)
    assert [(s["start_ms"], s["end_ms"]) for s in out] == [(0, 1040), (2800, 3920)]
    assert segs[1]["start_ms"] == 1040 and out[0]["text"] == " x" and out[0]["words"] is None


def test_restore_moves_a_word_with_the_chunk_of_its_midpoint():
    # the first word straddles the boundary at 1040 ms with its midpoint (1030) in chunk 0: both ends stay;
    # the second has its midpoint (1050) in chunk 1: both ends move by 1760 ms, also the one at 1000 ms
    segs = [_seg(900, 1200, [(960, 1100), (1000, 1100), (1100, 1200)])]
    out = vad.restore_speech_timestamps(segs, CASE1)
    w = out[0]["words"]
    assert [(x["start_ms"], x["end_ms"]) for x in w] == [(960, 1100), (2760, 2860), (2860, 2960)]
    assert [(x["start"], x["end"]) for x in w] == [(0.96, 1.1), (2.76, 2.86), (2.86, 2.96)]
    assert (out[0]["start_ms"], out[0]["end_ms"]) == (960, 2960)      # first word's start, last word's end
    assert segs[0]["words"][1]["start_ms"] == 1000                    # the input is not modified


# ---- transcribe_video -----------------------------------------------------------------------------------------------------
class _FakeVad:
    def __init__(self, probs):
        self.probs, self.calls, self.closed = np.asarray(probs, dtype=np.float32), [], False

    def speech_probs(self, samples):
        self.calls.append(np.array(samples))
        return self.probs

    def close(self):
        self.closed = True


class _FakeTranscriber:
    def __init__(self, segments=None):
        self.calls, self.closed = [], False
        self.segments = segments if segments is not None else [_seg(0, 1040), _seg(1040, 2160, [(1040, 1500), (1500, 2160)])]

    def transcribe(self, samples, language, **kw):
        self.calls.append((np.array(samples), language, kw))
        return {"language": "en", "segments": self.segments}

    def close(self):
        self.closed = True


AUDIO = (np.arange(N200, dtype=np.float32) % 1000) / 1000


def _run(config, fake_t, fake_v):
    return transcribe.transcribe_video("v.mp4", config, transcriber=fake_t, audio_source=lambda path: (AUDIO, 16000), vad=fake_v)


def test_transcriber_gets_the_speech_chunks_and_times_come_back_restored():
    t, v = _FakeTranscriber(), _FakeVad(_probs(200, (10, 19), (100, 109)))
    out = _run({"languages": ["en"], "beam_size": 5, "word_timestamps": True, "batch_windows": 4}, t, v)
    assert len(v.calls) == 1 and np.array_equal(v.calls[0], AUDIO)
    samples, language, kw = t.calls[0]
    assert np.array_equal(samples, np.concatenate([AUDIO[0:16640], AUDIO[44800:62720]])) and samples.dtype == np.float32
    assert language == "en" and kw == {"window_mode": "seek", "batch_windows": 4, "beam_size": 5, "word_timestamps": True}
    s0, s1 = out["segments"]
    assert (s0["start_ms"], s0["end_ms"], s0["words"]) == (0, 1040, None)
    assert (s1["start_ms"], s1["end_ms"]) == (2800, 3920)
    assert s1["words"] == [{"word": " w0", "start": 2.8, "end": 3.26, "confidence": 0.5},
                           {"word": " w1", "start": 3.26, "end": 3.92, "confidence": 0.5}]
    assert set(s0) == {"start_ms", "end_ms", "text", "language", "confidence", "words"}


def test_vad_filter_defaults_to_on_and_keywords_are_todays():
    t, v = _FakeTranscriber(), _FakeVad(_probs(200, (10, 19)))
    _run({}, t, v)
    assert len(v.calls) == 1 and t.calls[0][0].size == 16640 and t.calls[0][1] is None
    assert t.calls[0][2] == {"window_mode": "seek", "batch_windows": 8}


def test_vad_parameters_are_used():
    t, v = _FakeTranscriber(), _FakeVad(_probs(200, (10, 19), (30, 39)))
    _run({"vad_parameters": {"min_silence_duration_ms": 100, "speech_pad_ms": 0}}, t, v)
    assert t.calls[0][0].size == 2 * 5120


def test_no_speech_returns_no_segments_and_never_calls_the_transcriber():
    t, v = _FakeTranscriber(), _FakeVad(np.full(200, 0.1))
    assert _run({"vad_filter": True}, t, v) == {"segments": []}
    assert t.calls == [] and len(v.calls) == 1


def test_vad_filter_false_never_touches_the_vad():
    t, v = _FakeTranscriber(), _FakeVad(np.full(200, 0.1))
    out = _run({"vad_filter": False, "vad_parameters": {"threshold": 7}}, t, v)
    assert v.calls == [] and t.calls[0][0].size == N200
    assert [(s["start_ms"], s["end_ms"]) for s in out["segments"]] == [(0, 1040), (1040, 2160)]


def test_without_a_vad_everything_is_as_before(caplog):
    t = _FakeTranscriber()
    with caplog.at_level(logging.INFO, logger=transcribe.logger.name):
        out = _run({"vad_filter": True}, t, None)
    assert "vad_filter is accepted but not applied" in caplog.text
    assert t.calls[0][0].size == N200 and t.calls[0][2] == {"window_mode": "seek", "batch_windows": 8}
    assert [(s["start_ms"], s["end_ms"]) for s in out["segments"]] == [(0, 1040), (1040, 2160)]
    with pytest.raises(ValueError):            # not 16 kHz: still refused
        transcribe.transcribe_video("v.mp4", {}, transcriber=t, audio_source=lambda path: (AUDIO, 8000), vad=_FakeVad([0.9]))


@pytest.mark.parametrize("bad", [{"threshold": 2}, {"speech_pad_ms": -5}, {"nonsense": 1}, "fast"])
def test_bad_vad_parameters_raise_before_any_work(bad):
    t, v = _FakeTranscriber(), _FakeVad(np.full(200, 0.9))
    with pytest.raises(ValueError):
        _run({"vad_parameters": bad}, t, v)
    assert t.calls == [] and v.calls == []


# ---- ModelManager and process_ml_task ---------------------------------------------------------------------------------------
def _manager(tmp_path, fake_t, fake_v, made, **kw):
    def vad_factory(cache_dir):
        made.append(cache_dir)
        return fake_v

    return ModelManager(cache_dir=str(tmp_path), gpu_transcription=True, transcriber_factory=lambda cache, name: fake_t,
                        audio_source=lambda path: (AUDIO, 16000), vad_factory=vad_factory, **kw)


def test_model_manager_routes_through_the_vad_and_closes_it(tmp_path):
    t, v, made = _FakeTranscriber(), _FakeVad(_probs(200, (10, 19), (100, 109))), []
    out = asyncio.run(_manager(tmp_path, t, v, made, gpu_vad=True).transcribe_video("v.mp4", {"languages": "en"}))
    assert len(made) == 1 and str(made[0]) == str(tmp_path)
    assert t.calls[0][0].size == 16640 + 17920 and v.closed and t.closed
    assert [(s["start_ms"], s["end_ms"]) for s in out["segments"]] == [(0, 1040), (2800, 3920)]


def test_model_manager_builds_no_vad_when_the_task_turns_the_filter_off(tmp_path):
    t, v, made = _FakeTranscriber(), _FakeVad(np.full(200, 0.1)), []
    asyncio.run(_manager(tmp_path, t, v, made, gpu_vad=True).transcribe_video("v.mp4", {"vad_filter": False}))
    assert made == [] and t.calls[0][0].size == N200


def test_model_manager_without_gpu_vad_passes_everything(tmp_path):
    t, v, made = _FakeTranscriber(), _FakeVad(np.full(200, 0.1)), []
    asyncio.run(_manager(tmp_path, t, v, made).transcribe_video("v.mp4", {"vad_filter": True}))
    assert made == [] and v.calls == [] and t.calls[0][0].size == N200


def test_model_manager_missing_checkpoint_is_an_error(tmp_path):
    mm = ModelManager(cache_dir=str(tmp_path), gpu_transcription=True, transcriber_factory=lambda cache, name: _FakeTranscriber(),
                      audio_source=lambda path: (AUDIO, 16000), gpu_vad=True)
    with pytest.raises(FileNotFoundError, match="silero_vad"):
        asyncio.run(mm.transcribe_video("v.mp4", {}))


def test_process_ml_task_honours_gpu_vad(tmp_path, monkeypatch):
    monkeypatch.setenv("MODEL_CACHE_DIR", str(tmp_path))
    t, v, made, kwargs, got = _FakeTranscriber(), _FakeVad(_probs(200, (10, 19), (100, 109))), [], [], []

    def factory(cache_dir, **kw):
        kwargs.append(kw)
        return _manager(tmp_path, t, v, made, gpu_vad=kw.get("gpu_vad", False))

    ctx = {"gpu_transcription": True, "gpu_vad": True, "model_manager_factory": factory, "artifact_sink": got.extend}
    res = asyncio.run(task_handler.process_ml_task(ctx, "t1", "transcription", "vid", "v.mp4", {"languages": "en"}))
    assert kwargs == [{"gpu_transcription": True, "gpu_vad": True}]
    assert res == {"task_id": "t1", "status": "completed", "artifact_count": 2}
    assert [(e.span_start_ms, e.span_end_ms) for e in got] == [(0, 1040), (2800, 3920)]
    ctx = {"gpu_transcription": True, "model_manager_factory": factory, "artifact_sink": got.extend}
    asyncio.run(task_handler.process_ml_task(ctx, "t2", "transcription", "vid", "v.mp4", {"languages": "en"}))
    assert kwargs[1] == {"gpu_transcription": True} and len(v.calls) == 1
