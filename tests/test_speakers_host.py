"""Host side of K24 (speaker labels): the window plan, the state-dict folding, the oracle's own properties and the plumbing
through transcribe_video, ModelManager and process_ml_task.  No GPU."""
import asyncio
import json

import numpy as np
import pytest

import speaker_oracle as so
from eioku_amd import speakers, transcribe


# ---- plan_windows: hand-computed ----------------------------------------------------------------------------------------
def _ms_for_samples(n):  # a segment of exactly n samples needs n % 16 == 0; otherwise cut it with n_samples
    return -(-n // 16)


@pytest.mark.parametrize("length, want", [
    (399, []), (400, []),                                      # 0 and 1 frames
    (400 + 160 * 38, []),                                      # nf = 39
    (400 + 160 * 39, [(0, 40)]),                               # nf = 40
    (400 + 160 * 199, [(0, 200)]),                             # nf = 200
    (400 + 160 * 200, [(0, 200), (160, 200)]),                 # nf = 201: span 1, k = 2, frames 0 and 1
    (400 + 160 * 299, [(0, 200), (160 * 100, 200)]),           # nf = 300: span 100, k = 2
])
def test_plan_windows_hand_cases(length, want):
    # the audio ends at `length`: end_ms is past it (rounded up), so the plan is cut by n_samples
    assert speakers.plan_windows(0, _ms_for_samples(length) + 5, length) == want


def test_plan_windows_long_segment_is_capped():
    n = 400 + 160 * 1999                                       # nf = 2000: span 1800, 1 + 18 windows capped at 8
    plan = speakers.plan_windows(0, n // 16 + 1, n)
    assert len(plan) == 8 and all(v == 200 for _, v in plan)
    frames = [s // 160 for s, _ in plan]
    assert frames == [(j * 1800) // 7 for j in range(8)] and frames[0] == 0 and frames[-1] + 200 == 2000
    assert plan[-1][0] + 400 + 160 * 199 == n                  # the last window ends on the last frame


def test_plan_windows_offset_end_past_audio_and_small_windows():
    # start at 1 s; 3 s of audio in all: L = 32000 -> nf = 198
    assert speakers.plan_windows(1000, 9000, 48000) == [(16000, 198)]
    assert speakers.plan_windows(3000, 9000, 48000) == [] and speakers.plan_windows(5000, 9000, 48000) == []
    # win_frames = 40: nf = 198 -> span 158, hop 20, k = min(8, 1 + 8) = 8
    plan = speakers.plan_windows(1000, 9000, 48000, 40)
    assert [(s - 16000) // 160 for s, _ in plan] == [(j * 158) // 7 for j in range(8)] and {v for _, v in plan} == {40}
    for s, v in plan:
        assert 16000 <= s and s + 400 + 160 * (v - 1) <= 48000


# ---- fold_state ---------------------------------------------------------------------------------------------------------
def test_fold_state_equals_conv_then_bn_in_float64():
    sd = speakers.random_state_dict(5, (1, 1, 1, 1))
    st = speakers.fold_state(sd)
    rng = np.random.default_rng(0)
    for conv, bn, k in (("conv1", "bn1", 3), ("layer2.0.conv1", "layer2.0.bn1", 3), ("layer3.0.conv2", "layer3.0.bn2", 3),
                        ("layer2.0.shortcut.0", "layer2.0.shortcut.1", 1)):
        w = sd[conv + ".weight"].astype(np.float64)
        x = rng.standard_normal((w.shape[1], k, k))            # one receptive field
        y = np.einsum("oikl,ikl->o", w, x)
        g, b, mu, var = (sd[f"{bn}.{f}"].astype(np.float64) for f in ("weight", "bias", "running_mean", "running_var"))
        want = (y - mu) / np.sqrt(var + 1e-5) * g + b
        fw, fb = st["convs"][conv]
        got = np.einsum("oikl,ikl->o", fw.astype(np.float64), x) + fb
        assert np.allclose(got, want, rtol=0, atol=1e-5 * max(1.0, np.abs(want).max()))
    assert st["depths"] == (1, 1, 1, 1) and "layer1.0.shortcut.0" not in st["convs"]


def test_seg1_columns_round_trip_and_order():
    w = np.arange(3 * speakers.N_STAT, dtype=np.float32).reshape(3, -1)
    d = speakers.torch_to_device_columns(w)
    assert np.array_equal(speakers.device_to_torch_columns(d), w)
    c, f = 37, 6                                               # torch column c * 10 + f (mean) sits at device f * 256 + c
    assert d[1, f * 256 + c] == w[1, c * 10 + f] and d[2, 2560 + f * 256 + c] == w[2, 2560 + c * 10 + f]
    sd = speakers.random_state_dict(2, (1, 1, 1, 1))
    assert np.array_equal(speakers.device_to_torch_columns(speakers.fold_state(sd)["head"][0]), sd["seg_1.weight"])


def test_fold_state_rejects_missing_and_misshapen_and_strips_prefixes():
    sd = speakers.random_state_dict(2, (1, 1, 1, 1))
    missing = {k: v for k, v in sd.items() if k != "layer3.0.bn2.running_var"}
    with pytest.raises(KeyError):
        speakers.fold_state(missing)
    with pytest.raises(KeyError):
        speakers.fold_state({k: v for k, v in sd.items() if k != "seg_1.weight"})
    bad = dict(sd)
    bad["layer2.0.conv1.weight"] = bad["layer2.0.conv1.weight"][:, :, :2]
    with pytest.raises(ValueError):
        speakers.fold_state(bad)
    want = speakers.fold_state(sd)
    for prefix in ("resnet.", "module.", "module.resnet."):
        got = speakers.fold_state({"state_dict": {prefix + k: v for k, v in sd.items()}})
        assert all(np.array_equal(got["convs"][k][0], want["convs"][k][0]) for k in want["convs"])
        assert np.array_equal(got["head"][0], want["head"][0])


def test_depths_are_read_for_r18_and_r34():
    for name in ("r18", "r34"):
        sd = speakers.random_state_dict(1, speakers.DEPTHS[name])
        assert speakers.depths_from_state(sd) == speakers.DEPTHS[name]
        assert speakers.depths_from_state({"resnet." + k: v for k, v in sd.items()}) == speakers.DEPTHS[name]
    with pytest.raises(KeyError):
        speakers.depths_from_state({"conv1.weight": np.zeros((32, 1, 3, 3), np.float32)})


def test_from_cache_needs_a_checkpoint_or_a_seed(tmp_path):
    with pytest.raises(FileNotFoundError):
        speakers.SpeakerLabeller.from_cache(tmp_path)


# ---- tables and oracle self-checks -------------------------------------------------------------------------------------------
def test_tables_equal_the_oracles_restatement():
    assert np.allclose(speakers.kaldi_mel_banks(), so.mel_banks(), rtol=0, atol=1e-12)
    assert np.allclose(speakers.povey_window(), so.povey(), rtol=0, atol=1e-15)


def test_kaldi_mel_filters_are_triangles_that_tile():
    banks = so.mel_banks()
    assert banks.shape == (80, 256) and banks.min() >= 0 and banks.max() <= 1
    mel = so.mel_scale(np.arange(256) * 31.25)
    lo, hi = so.mel_scale(20.0), so.mel_scale(8000.0)
    delta = (hi - lo) / 81
    for j in (0, 17, 79):
        nz = np.nonzero(banks[j])[0]
        assert np.array_equal(nz, np.arange(nz[0], nz[-1] + 1))            # one run of bins
        peak = np.argmax(banks[j])
        assert np.all(np.diff(banks[j][nz[0]:peak + 1]) > 0) and np.all(np.diff(banks[j][peak:nz[-1] + 1]) < 0)
    # neighbouring triangles cross at complementary heights: between the first and the last centre every bin sums to 1
    interior = (mel >= lo + delta) & (mel <= hi - delta)
    assert interior.sum() > 200 and np.allclose(banks.sum(axis=0)[interior], 1.0, rtol=0, atol=1e-12)
    assert banks[:, 0].sum() == 0                                          # bin 0 (0 Hz) lies below 20 Hz


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_silence_and_dc_give_exactly_zero_features(dtype):
    n = 400 + 160 * 49
    for x in (np.zeros(n, np.float32), np.full(n, 0.25, np.float32)):
        f = so.fbank_cmn(x, 0, 50, dtype)
        assert f.shape == (80, 50) and not f.any()
    f = so.features(np.zeros(n, np.float32), [(0, 50), (160, 17)], 56)
    assert f.shape == (2, 80, 56) and not f.any()


def test_voices_have_distinct_features():
    a, b = (so.voice(i, *so.VOICES[i], 400 + 160 * 39) for i in (0, 1))
    fa, fb = so.fbank_cmn(a, 0, 40), so.fbank_cmn(b, 0, 40)
    assert np.abs(fa).max() > 1 and np.abs(fa - fb).mean() > 0.1
    assert np.allclose(fa.mean(axis=1), 0, atol=1e-9)                      # CMN


# ---- labels ---------------------------------------------------------------------------------------------------------------
def test_labels_are_renumbered_by_first_appearance():
    assert speakers.speaker_ids([2, -1, 0, 2, None, 1]) == ["speaker_001", None, "speaker_002", "speaker_001", None, "speaker_003"]
    assert speakers.speaker_ids([0, 1, 0], starts_ms=[500, 100, 900]) == ["speaker_002", "speaker_001", "speaker_002"]
    assert speakers.speaker_ids([]) == [] and speakers.speaker_ids([-1, -1]) == [None, None]


def test_more_segments_than_k14_clusters_is_an_error():
    class Planned:                                             # the plan and the limit come before any device work
        win = speakers.WIN

    segments = [{"start_ms": 0, "end_ms": 1000}] * (speakers.MAX_SEGMENTS + 1)
    with pytest.raises(ValueError, match="65537 segments"):
        speakers.SpeakerLabeller.embed_segments(Planned(), np.zeros(16000, np.float32), segments)


# ---- transcribe_video ---------------------------------------------------------------------------------------------------------
SEGMENTS = [{"start_ms": 0, "end_ms": 900, "text": " a", "language": "en", "confidence": None, "words": None},
            {"start_ms": 900, "end_ms": 2000, "text": " b", "language": "en", "confidence": None, "words": None}]


class StubTranscriber:
    def __init__(self):
        self.calls = []

    def transcribe(self, samples, language, **kw):
        self.calls.append((np.array(samples), kw))
        return {"segments": [dict(s) for s in SEGMENTS], "language": "en"}


class StubSpeakers:
    def __init__(self, labels=("speaker_001", None)):
        self.calls, self.labels, self.closed = [], list(labels), False

    def label(self, samples, segments, **kw):
        self.calls.append((np.array(samples), [dict(s) for s in segments], kw))
        return list(self.labels)

    def close(self):
        self.closed = True


def _audio(n=48000, seed=0):
    return (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _run(config, spk, **kw):
    audio = _audio()
    return transcribe.transcribe_video("clip.wav", config, transcriber=StubTranscriber(), audio_source=lambda p: (audio, 16000),
                                       speakers=spk, **kw), audio


def test_speaker_key_appears_only_when_asked():
    plain, _ = _run({}, None)
    assert plain == {"segments": SEGMENTS} and all(set(s) == {"start_ms", "end_ms", "text", "language", "confidence", "words"}
                                                   for s in plain["segments"])
    for config in ({}, {"speaker_labels": False}, {"speaker_eps": 7.0}):       # options are not even looked at
        spk = StubSpeakers()
        got, _ = _run(config, spk)
        assert got == plain and spk.calls == []
    assert _run({"speaker_labels": True}, None)[0] == plain                    # no labeller: the plain result
    spk = StubSpeakers()
    got, audio = _run({"speaker_labels": True, "speaker_eps": 0.4, "speaker_min_samples": 3, "speaker_assign_max": 0}, spk)
    assert [s["speaker"] for s in got["segments"]] == ["speaker_001", None]
    assert [{k: v for k, v in s.items() if k != "speaker"} for s in got["segments"]] == SEGMENTS
    (samples, segments, kw), = spk.calls
    assert np.array_equal(samples, audio) and kw == {"eps": 0.4, "min_samples": 3, "assign_max": 0.0}
    assert [(s["start_ms"], s["end_ms"]) for s in segments] == [(0, 900), (900, 2000)]
    spk = StubSpeakers()
    _run({"speaker_labels": True}, spk)
    assert spk.calls[0][2] == {"eps": speakers.DEFAULT_EPS, "min_samples": 2, "assign_max": speakers.DEFAULT_ASSIGN_MAX}


@pytest.mark.parametrize("config", [
    {"speaker_labels": 1}, {"speaker_labels": "yes"}, {"speaker_labels": None},
    {"speaker_labels": True, "speaker_eps": 0}, {"speaker_labels": True, "speaker_eps": 2}, {"speaker_labels": True, "speaker_eps": "0.3"},
    {"speaker_labels": True, "speaker_eps": float("nan")}, {"speaker_labels": True, "speaker_eps": True},
    {"speaker_labels": True, "speaker_min_samples": 0}, {"speaker_labels": True, "speaker_min_samples": 1.5},
    {"speaker_labels": True, "speaker_assign_max": -0.1}, {"speaker_labels": True, "speaker_assign_max": 2.5}])
def test_bad_speaker_options_raise(config):
    spk = StubSpeakers()
    with pytest.raises(ValueError):
        _run(config, spk)
    assert spk.calls == []


def test_with_vad_the_labeller_sees_file_time_and_the_original_samples():
    class StubVad:
        def speech_probs(self, samples):
            p = np.zeros(len(samples) // 512 + 1, np.float32)
            p[40:80] = 1.0                                                      # speech from sample 20480
            return p

    spk = StubSpeakers()
    tr = StubTranscriber()
    audio = _audio(64000, 1)
    got = transcribe.transcribe_video("clip.wav", {"speaker_labels": True, "vad_parameters": {"speech_pad_ms": 0, "min_silence_duration_ms": 100}},
                                      transcriber=tr, audio_source=lambda p: (audio, 16000), vad=StubVad(), speakers=spk)
    (samples, segments, _), = spk.calls
    assert np.array_equal(samples, audio) and len(tr.calls[0][0]) < len(audio)  # the transcriber saw the speech only
    assert segments[0]["start_ms"] == 20480 // 16 and [s["start_ms"] for s in got["segments"]] == [s["start_ms"] for s in segments]
    assert [s["speaker"] for s in got["segments"]] == ["speaker_001", None]


def test_a_labeller_with_the_wrong_count_is_an_error():
    with pytest.raises(ValueError):
        _run({"speaker_labels": True}, StubSpeakers(labels=("speaker_001",)))


# ---- ModelManager / process_ml_task ------------------------------------------------------------------------------------------
def _manager(tmp_path, built, **kw):
    from eioku_amd.model_manager import ModelManager

    def speaker_factory(cache_dir, model_name):
        built.append(model_name)
        return built_stub

    built_stub = StubSpeakers()
    audio = _audio()
    mm = ModelManager(cache_dir=str(tmp_path), gpu_transcription=True, audio_source=lambda p: (audio, 16000),
                      transcriber_factory=lambda c, m: StubTranscriber(), speaker_factory=speaker_factory, **kw)
    return mm, built_stub


def test_model_manager_builds_the_labeller_only_when_asked(tmp_path):
    built = []
    mm, stub = _manager(tmp_path, built, gpu_speakers=True)
    plain = asyncio.run(mm.transcribe_video("clip.wav", {"vad_filter": False}))
    assert built == [] and plain == {"segments": SEGMENTS}
    got = asyncio.run(mm.transcribe_video("clip.wav", {"vad_filter": False, "speaker_labels": True, "speaker_model": "r34_custom"}))
    assert built == ["r34_custom"] and stub.closed and [s["speaker"] for s in got["segments"]] == ["speaker_001", None]
    built.clear()
    mm, stub = _manager(tmp_path, built)                                       # gpu_speakers off: never built
    assert asyncio.run(mm.transcribe_video("clip.wav", {"vad_filter": False, "speaker_labels": True})) == plain and built == []


def test_process_ml_task_passes_gpu_speakers_and_the_payload_carries_the_key(tmp_path, monkeypatch):
    from eioku_amd import task_handler

    made, sunk = [], []

    def factory(cache_dir, **kw):
        made.append(kw)
        mm, _ = _manager(tmp_path, [], **{k: v for k, v in kw.items() if k != "gpu_transcription"})
        return mm

    monkeypatch.setenv("MODEL_CACHE_DIR", str(tmp_path))
    for ctx_extra, config, want in (({"gpu_speakers": True}, {"vad_filter": False, "speaker_labels": True}, ["speaker_001", None]),
                                    ({}, {"vad_filter": False, "speaker_labels": True}, None)):
        made.clear()
        sunk.clear()
        ctx = {"gpu_transcription": True, "model_manager_factory": factory, "artifact_sink": sunk.extend, **ctx_extra}
        asyncio.run(task_handler.process_ml_task(ctx, "t1", "transcription", "v1", "clip.wav", config=config))
        assert made == [{"gpu_transcription": True, **ctx_extra}]
        assert {e.artifact_type for e in sunk} == {"transcript.segment"}
        payloads = [json.loads(e.payload_json) for e in sunk]
        assert len(payloads) == 2
        if want is None:
            assert all("speaker" not in p for p in payloads)
        else:
            assert [p["speaker"] for p in payloads] == want
