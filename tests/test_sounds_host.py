"""K29 on the host: the oracle against ``transformers`` (feature extractor and model), the tables, the window plan, the task
settings, the two checkpoint layouts, event merging and the task plumbing.  No GPU."""
import asyncio
import json

import numpy as np
import pytest
import torch

import sounds_oracle as so
from eioku_amd import sounds, task_handler
from eioku_amd.model_manager import ModelManager

PAD = np.float32((0.0 - so.MEAN) / (2 * so.STD))
SILENCE = np.float32((np.log(so.MEL_FLOOR) - so.MEAN) / (2 * so.STD))


# ---- the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,max_length,mel", [("full", 400 + 160 * 47, 48, 32), ("partial", 5000, 48, 32), ("one-frame", 400, 48, 32),
                                                   ("2s-of-1024", 32000, 1024, 128)])
def test_float64_fbank_equals_the_feature_extractor(name, n, max_length, mel):
    """The extractor computes in float64 and rounds to float32 (its log, then its normalisation), the oracle rounds once: the
    two may differ by one float32 ulp of the values, which stay below 2 (ulp 2^-23 = 1.19e-7).  Measured here: 6.0e-8 at
    the three small cases (all |values| < 1.3), 1.19e-7 at 2 s of 1024 x 128."""
    tr = pytest.importorskip("transformers")
    x = so.audio(n, 3)
    if name == "partial":
        x[1000:2200] = 0.0  # frames 7 .. 11 see silence only
    fe = tr.ASTFeatureExtractor(num_mel_bins=mel, max_length=max_length)
    want = fe(x, sampling_rate=16000, return_tensors="np")["input_values"][0]
    valid = min(max_length, 1 + (n - 400) // 160)
    got = so.fbank(x, 0, valid, max_length, mel)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (max_length, mel)
    diff = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{name}: oracle vs ASTFeatureExtractor {diff:.3e} (max |.| {np.abs(want).max():.3f}, {valid} valid frames)")
    assert np.abs(want).max() < 2 and diff <= float(np.spacing(np.float32(1.0)))
    assert PAD == np.float32(0.46703237) and SILENCE == np.float32(-1.2775939)
    assert (got[valid:] == PAD).all() and (want[valid:] == PAD).all()
    if name == "partial":
        assert (got[7:12] == SILENCE).all() and (want[7:12] == SILENCE).all() and (got[:7] != SILENCE).all()


def test_fp32_oracle_equals_transformers():
    """Measured here: hidden 1.5e-6 / logits 6.9e-6 on values up to 6.4 (hidden) and 10.8 (logits).  The bar is that of
    tests/test_actions_host.py, 5e-5: a few fp32 roundings, nothing a wrong token order, patch order or epsilon could meet."""
    tr = pytest.importorskip("transformers")
    cfg = so.config_s()
    w = so.random_weights(cfg, 3)
    model = tr.ASTForAudioClassification(tr.ASTConfig(**so.hf_config(cfg))).eval()
    assert list(model.state_dict()) == list(w)
    model.load_state_dict(w, strict=True)
    spec = np.random.default_rng(1).standard_normal((2, cfg["max_length"], cfg["mel"])).astype(np.float32)
    with torch.no_grad():
        logits = model(input_values=torch.from_numpy(spec)).logits
        emb = hidden = model.audio_spectrogram_transformer.embeddings(torch.from_numpy(spec))
        for layer in model.audio_spectrogram_transformer.layers:
            hidden = layer(hidden, None)
    o = so.Oracle(cfg, w, fp16=False)
    rows = so.patch_rows(spec, cfg)
    h, lg = o.forward(rows)
    e = o.embed(rows)
    dh, dl, de = (hidden - h).abs().max().item(), (logits - lg).abs().max().item(), (emb - e).abs().max().item()
    print(f"S: oracle vs transformers: embedding {de:.3e}, hidden {dh:.3e} (max |.| {hidden.abs().max():.2f}), logits {dl:.3e} "
          f"(max |.| {logits.abs().max():.2f})")
    assert so.grid(cfg) == (2, 4) and hidden.shape == h.shape == (2, 10, cfg["hidden"])  # 2 x 4 patches + CLS + distillation
    assert de <= 5e-5 and dh <= 5e-5 and dl <= 5e-5
    # token order: CLS, the distillation token, then the patches, frequency-major
    pre = so.PREFIX + "embeddings."
    pos = w[pre + "position_embeddings"][0]
    assert torch.equal(e[0, 0], w[pre + "cls_token"][0, 0] + pos[0]) and torch.equal(e[1, 1], w[pre + "distillation_token"][0, 0] + pos[1])


def test_patch_rows_are_frequency_major_with_unequal_strides():
    cfg = so.config_r()
    f, t = so.grid(cfg)
    assert (f, t) == (4, 5)
    spec = np.random.default_rng(0).standard_normal((2, cfg["max_length"], cfg["mel"])).astype(np.float32)
    rows = so.patch_rows(spec, cfg)
    assert rows.shape == (2, 20, 256)
    # patch fi = 3, ti = 2; element df = 5, dt = 9: time 12 * 2 + 9, mel 8 * 3 + 5
    assert rows[1, 3 * t + 2, 16 * 5 + 9] == spec[1, 24 + 9, 24 + 5]
    assert cfg["max_length"] - (12 * (t - 1) + 16) == 6  # six frames lie in no patch


def test_ast_tables_equal_audio_utils():
    au = pytest.importorskip("transformers.audio_utils")
    for bins in (128, 40, 32):
        window, mel = sounds.ast_tables(bins)
        ref = au.mel_filter_bank(num_frequency_bins=257, num_mel_filters=bins, min_frequency=20, max_frequency=8000, sampling_rate=16000,
                                 norm=None, mel_scale="kaldi", triangularize_in_mel_space=True)
        assert window.dtype == mel.dtype == np.float64 and mel.shape == ref.shape == (257, bins) and window.shape == (400,)
        assert np.abs(window - au.window_function(400, "hann", periodic=False)).max() <= 1e-15
        assert np.abs(mel - ref).max() <= 1e-15
        assert np.abs(mel - so.mel_matrix(bins)).max() <= 1e-13 and np.abs(window - so.hann()).max() <= 1e-15


# ---- the window plan -------------------------------------------------------------------------------------------------------
def test_plan_windows():
    span = sounds.window_samples(48)
    assert span == 400 + 160 * 47 == 7920 and sounds.window_samples(1024) == 164080
    plan = sounds.plan_windows
    # a full file: three windows end to end
    assert plan(3 * span, 48, span) == [(0, 48), (span, 48), (2 * span, 48)]
    # overlapping windows; the tail [2 * 4000, n) is already inside window 1, so there is no window 2
    assert plan(4000 + span, 48, 4000) == [(0, 48), (4000, 48)]
    assert plan(4000 + span + 1, 48, 4000) == [(0, 48), (4000, 48), (8000, 1 + (span + 1 - 4000 - 400) // 160)]
    # 399 new samples make no frame, 400 make one
    assert plan(span + 399, 48, span) == [(0, 48)]
    assert plan(span + 400, 48, span) == [(0, 48), (span, 1)]
    assert plan(span + 400 + 159, 48, span)[-1] == (span, 1) and plan(span + 400 + 160, 48, span)[-1] == (span, 2)
    # a stride longer than the window leaves gaps
    assert plan(3 * span, 48, 2 * span) == [(0, 48), (2 * span, 48)]
    # short files
    assert plan(399, 48, span) == [] and plan(0, 48, span) == [] and plan(400, 48, span) == [(0, 1)]
    assert plan(5000, 48, span) == [(0, 29)]
    with pytest.raises(ValueError, match="stride_samples"):
        plan(1000, 48, 0)


@pytest.mark.parametrize("config,match", [
    ({"model_name": "../x"}, "sound_detection: model_name"), ({"model_name": 3}, "sound_detection: model_name"),
    ({"model_name": ""}, "sound_detection: model_name"), ({"window_stride": 0.001}, "sound_detection: window_stride"),
    ({"window_stride": "10"}, "sound_detection: window_stride"), ({"window_stride": True}, "sound_detection: window_stride"),
    ({"top_k": 0}, "sound_detection: top_k"), ({"top_k": 8}, "sound_detection: top_k"), ({"top_k": 2.5}, "sound_detection: top_k"),
    ({"top_k": True}, "sound_detection: top_k"), ({"min_score": -0.1}, "sound_detection: min_score"),
    ({"min_score": 1.5}, "sound_detection: min_score"), ({"min_score": "0"}, "sound_detection: min_score"),
    ({"batch_windows": 0}, "sound_detection: batch_windows"), ({"batch_windows": 65}, "sound_detection: batch_windows"),
    ({"batch_windows": 1.0}, "sound_detection: batch_windows"),
])
def test_sound_settings_refuse_bad_values(config, match):
    with pytest.raises(ValueError, match=match):
        sounds.sound_settings(config, 7)


def test_sound_settings_defaults():
    assert sounds.sound_settings({}, 527) == {"model_name": "ast-finetuned-audioset-10-10-0.4593", "window_stride": 10.0, "top_k": 5,
                                              "min_score": 0.0, "batch_windows": 32}
    assert sounds.sound_settings({}, 3)["top_k"] == 3 and sounds.sound_settings({})["top_k"] == 5
    got = sounds.sound_settings({"window_stride": 1, "top_k": 7, "min_score": 1, "batch_windows": 64, "model_name": "tiny"}, 7)
    assert got == {"model_name": "tiny", "window_stride": 1.0, "top_k": 7, "min_score": 1.0, "batch_windows": 64}


# ---- configuration and loading -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change,match", [
    ({"num_attention_heads": 4}, "head dimension must be 64"), ({"patch_size": 8}, "patch_size must be 16"),
    ({"num_mel_bins": 8}, r"num_mel_bins must be in \[16, 128\]"), ({"num_mel_bins": 160}, r"num_mel_bins must be in \[16, 128\]"),
    ({"frequency_stride": 0}, "stride"), ({"time_stride": 17}, "stride"), ({"max_length": 15}, "max_length must be at least 16"),
    ({"max_length": 100000, "num_mel_bins": 128}, "at most 4094 tokens"), ({"intermediate_size": 100}, "multiple of 32"),
    ({"hidden_act": "relu"}, "is not built"),
])
def test_config_validation(change, match):
    with pytest.raises(ValueError, match=match):
        sounds.ast_dims({**so.hf_config(so.config_s()), **change})


def test_config_defaults_labels_and_preprocessor_agreement():
    d = sounds.ast_dims({})
    assert (d["mel"], d["max_length"], d["f"], d["t"], d["patches"], d["tokens"]) == (128, 1024, 12, 101, 1212, 1214)
    assert (d["hidden"], d["layers"], d["heads"], d["ffn"], d["labels"], d["ln_eps"]) == (768, 12, 12, 3072, 527, 1e-12)
    assert sounds.config_labels({"id2label": {"0": "Speech", "2": "Bark"}}, 3) == ["Speech", "sound_1", "Bark"]
    assert sounds.preprocessing({}) == {"mean": -4.2677393, "std": 4.5689974}
    assert sounds.preprocessing({}, {"mean": -5.0, "std": 4.0, "max_length": 1024, "num_mel_bins": 128}) == {"mean": -5.0, "std": 4.0}
    with pytest.raises(ValueError, match="max_length"):
        sounds.preprocessing({}, {"max_length": 512})
    with pytest.raises(ValueError, match="num_mel_bins"):
        sounds.preprocessing({"num_mel_bins": 64}, {"num_mel_bins": 128})
    with pytest.raises(ValueError, match="sampling_rate"):
        sounds.preprocessing({}, {"sampling_rate": 44100})


def test_both_checkpoint_layouts_give_the_same_tensors_in_the_table_order():
    cfg = so.config_s()
    dims = sounds.ast_dims(so.hf_config(cfg))
    order = [name for name, _ in sounds.tensor_shapes(dims)]
    new = {k: v.numpy() for k, v in so.random_weights(cfg, 3).items()}
    old = so.old_layout(new)
    assert list(new) == order and sorted(old) != sorted(new)
    assert f"{so.PREFIX}encoder.layer.1.attention.attention.query.weight" in old and f"{so.PREFIX}encoder.layer.0.output.dense.bias" in old
    a, b = sounds.canonical_state(new), sounds.canonical_state(old)
    assert sorted(a) == sorted(b) == sorted(order)
    assert all(a[k] is new[k] and b[k] is new[k] for k in order)
    assert all(tuple(new[k].shape) == shape for k, shape in sounds.tensor_shapes(dims))


def test_random_state_has_the_state_dict_shapes_and_from_cache_needs_a_directory(tmp_path):
    cfg = so.hf_config(so.config_s())
    sd = sounds.random_state(cfg, 5)
    ref = so.random_weights(so.config_s(), 0)
    assert list(sd) == list(ref)
    assert all(sd[k].shape == tuple(ref[k].shape) and sd[k].dtype == np.float32 for k in sd)
    again = sounds.random_state(cfg, 5)
    assert all(np.array_equal(sd[k], again[k]) for k in sd)
    assert not np.array_equal(sd["classifier.dense.weight"], sounds.random_state(cfg, 6)["classifier.dense.weight"])
    with pytest.raises(FileNotFoundError, match="config.json"):
        sounds.SoundTagger.from_cache(tmp_path, sounds.DEFAULT_MODEL)


# ---- events --------------------------------------------------------------------------------------------------------------------
def test_sound_events_merge_consecutive_windows():
    def item(i, labels, scores):
        return {"start_ms": 1000 * i, "end_ms": 1000 * i + 3000, "timestamp_ms": 1000 * i, "labels": labels, "scores": scores}

    items = [item(0, ["Music", "Speech"], [0.9, 0.2]), item(1, ["Music", "Applause"], [0.7, 0.6]), item(2, ["Applause", "Music"], [0.8, 0.4]),
             item(3, ["Music"], [0.95]), item(4, [], [])]
    assert sounds.sound_events(items, 0.5) == [
        {"label": "Music", "start_ms": 0, "end_ms": 4000, "score": 0.9},          # windows 0 and 1; window 2 is below the threshold
        {"label": "Applause", "start_ms": 1000, "end_ms": 5000, "score": 0.8},
        {"label": "Music", "start_ms": 3000, "end_ms": 6000, "score": 0.95}]
    assert sounds.sound_events(items, 0.99) == [] and sounds.sound_events([], 0.5) == []
    assert [e["label"] for e in sounds.sound_events(items, 0.2)] == ["Music", "Speech", "Applause"]
    assert sounds.sound_events(items, 0.2)[0] == {"label": "Music", "start_ms": 0, "end_ms": 6000, "score": 0.95}


# ---- detect_sounds on a stub tagger ----------------------------------------------------------------------------------------------
class _Tagger:
    """Records its calls; the labels of window w are (w, w + 1, ..) mod labels with scores 0.5, 0.25, .."""
    labels, max_length, window_samples = [f"s{i}" for i in range(6)], 48, 7920

    def __init__(self):
        self.calls, self.closed = [], False

    def classify(self, samples, plan, top_k, batch_windows=32):
        assert isinstance(samples, np.ndarray) and samples.dtype == np.float32 and samples.ndim == 1
        self.calls.append((samples.size, list(plan), top_k, batch_windows))
        ids = np.stack([(w + np.arange(top_k)) % 6 for w in range(len(plan))]).astype(np.int32)
        scores = np.tile(np.float32(0.5) ** np.arange(1, top_k + 1, dtype=np.float32), (len(plan), 1))
        return scores, ids

    def close(self):
        self.closed = True


def _detect(n, config, rate=16000):
    tagger = _Tagger()
    mm = ModelManager(cache_dir="/tmp/eioku-test-cache", audio_source=lambda p: (np.zeros(n, np.float32), rate),
                      sound_tagger_factory=lambda cache, name: tagger)
    out = asyncio.run(mm.detect_sounds("video.mp4", config))
    assert tagger.closed and sorted(out) == ["sounds"]
    return out["sounds"], tagger


def test_detect_sounds_windows_fields_and_filtering():
    n = 20000  # windows of 7920 samples every 0.25 s = 4000 samples: 0, 4000, 8000, 12000, 16000 (a tail of 4000: 23 frames)
    items, tagger = _detect(n, {"window_stride": 0.25, "top_k": 3, "batch_windows": 2})
    plan = sounds.plan_windows(n, 48, 4000)
    assert tagger.calls == [(n, plan, 3, 2)] and [p[0] for p in plan] == [0, 4000, 8000, 12000, 16000] and plan[-1][1] == 23
    assert [(s["start_ms"], s["end_ms"], s["timestamp_ms"]) for s in items] == [(0, 495, 0), (250, 745, 250), (500, 995, 500),
                                                                               (750, 1245, 750), (1000, 1250, 1000)]
    assert items[1]["labels"] == ["s1", "s2", "s3"] and items[1]["scores"] == [0.5, 0.25, 0.125]
    assert all(sorted(s) == ["end_ms", "labels", "scores", "start_ms", "timestamp_ms"] for s in items)
    assert all(type(s[k]) is int for s in items for k in ("start_ms", "end_ms", "timestamp_ms"))
    assert all(type(v) is float for s in items for v in s["scores"]) and all(type(v) is str for s in items for v in s["labels"])
    items, _ = _detect(n, {"window_stride": 0.25, "top_k": 3, "min_score": 0.2})
    assert all(s["labels"] == [f"s{w % 6}", f"s{(w + 1) % 6}"] and s["scores"] == [0.5, 0.25] for w, s in enumerate(items))
    assert len(_detect(n, {})[0]) == 1  # the default stride of 10 s


def test_detect_sounds_short_files_and_bad_input():
    items, tagger = _detect(399, {})
    assert items == [] and tagger.calls == []
    assert len(_detect(400, {})[0]) == 1
    with pytest.raises(ValueError, match="44100 Hz"):
        _detect(20000, {}, rate=44100)
    with pytest.raises(ValueError, match="sound_detection: top_k"):
        _detect(20000, {"top_k": 7})


def test_detect_sounds_resolves_audio_as_transcription_does():
    """``gpu_audio``: the front end loads the file (and is closed); with an injected source it only resamples other rates."""
    class FrontEnd:
        def __init__(self):
            self.loaded, self.resampled, self.closed = [], [], False

        def load(self, path):
            self.loaded.append(path)
            return np.zeros(9000, np.float32), 16000

        def resample_float(self, samples, rate):
            self.resampled.append((len(samples), rate))
            return np.zeros(len(samples) * 16000 // rate, np.float32)

        def close(self):
            self.closed = True

    fe, tagger = FrontEnd(), _Tagger()
    mm = ModelManager(cache_dir="/tmp/eioku-test-cache", gpu_audio=True, audio_frontend_factory=lambda: fe,
                      sound_tagger_factory=lambda cache, name: tagger)
    out = asyncio.run(mm.detect_sounds("video.mp4", {}))
    assert fe.loaded == ["video.mp4"] and fe.resampled == [] and fe.closed and tagger.closed
    assert tagger.calls == [(9000, [(0, 48)], 5, 32)] and len(out["sounds"]) == 1
    fe, tagger = FrontEnd(), _Tagger()
    mm = ModelManager(cache_dir="/tmp/eioku-test-cache", gpu_audio=True, audio_frontend_factory=lambda: fe,
                      audio_source=lambda p: (np.zeros(4000, np.float32), 8000), sound_tagger_factory=lambda cache, name: tagger)
    asyncio.run(mm.detect_sounds("video.mp4", {}))
    assert fe.loaded == [] and fe.resampled == [(4000, 8000)] and tagger.calls[0][0] == 8000


# ---- task plumbing -----------------------------------------------------------------------------------------------------------
def test_task_tables_name_the_new_type():
    assert task_handler.TASK_TO_ARTIFACT_TYPE["sound_detection"] == "sound.detection"
    assert task_handler.TASK_TO_RESULT_KEY["sound_detection"] == "sounds"
    assert "sound_detection" in task_handler.KNOWN_TASK_TYPES
    # added, nothing reordered
    assert task_handler.KNOWN_TASK_TYPES[:12] == ("object_detection", "face_detection", "transcription", "ocr", "place_detection",
                                                  "scene_detection", "metadata_extraction", "segment_embedding", "topic_extraction",
                                                  "thumbnail_generation", "action_detection", "frame_embedding")


def test_process_ml_task_emits_sound_envelopes():
    class Stub:
        def __init__(self, cache_dir):
            pass

        async def detect_sounds(self, video_path, config):
            assert config == {"top_k": 2}
            return {"sounds": [{"start_ms": 0, "end_ms": 10255, "timestamp_ms": 0, "labels": ["Music", "Speech"], "scores": [0.75, 0.125]},
                               {"start_ms": 10000, "end_ms": 12000, "timestamp_ms": 10000, "labels": ["Applause"], "scores": [0.5]}]}

    got = []
    res = asyncio.run(task_handler.process_ml_task({"model_manager_factory": Stub, "artifact_sink": got.extend}, "t1",
                                                   "sound_detection", "vid", "/x.mp4", {"top_k": 2}))
    assert res == {"task_id": "t1", "status": "completed", "artifact_count": 2}
    assert [e.artifact_type for e in got] == ["sound.detection"] * 2
    assert [(e.span_start_ms, e.span_end_ms) for e in got] == [(0, 10255), (10000, 12000)]
    assert json.loads(got[1].payload_json)["labels"] == ["Applause"] and got[0].asset_id == "vid"
