"""K29 on the device against tests/sounds_oracle.py (the CPU oracle; transformers is not needed here).

Configurations, the smallest at which each kernel can still go wrong:
  S   32 mel bins, max_length 48, strides 10 / 10: 2 x 4 patches + 2 = 10 tokens (below one MFMA tile), hidden 128 (2 heads),
      ffn 256, 2 layers, 7 labels, 3 windows
  R   40 mel bins, max_length 70, strides 8 (frequency) / 12 (time): 4 x 5 + 2 = 22 tokens, 6 frames in no patch, 1 layer:
      a swapped stride or axis shows here
  W   the base width: 128 mel bins, max_length 176: 12 x 17 + 2 = 206 tokens (two LDS stages of the attention, a multiple
      of neither 16 nor 64), hidden 768, 12 heads, ffn 3072, 2 layers, 527 labels, 1 window
  L   the real token count: 128 mel bins, max_length 1024: 1214 tokens (ten LDS stages, the full position table), hidden
      128, 1 layer, 7 labels, 2 windows
"""
import asyncio
import json
import wave

import numpy as np
import pytest
import torch

import sounds_oracle as so

pytestmark = pytest.mark.gpu

PAD = np.float32((0.0 - so.MEAN) / (2 * so.STD))


def _span(cfg):
    return 400 + 160 * (cfg["max_length"] - 1)


def _plan(cfg):
    """three windows: every frame valid, about two thirds of them, one"""
    T = cfg["max_length"]
    return [(0, T), (3000, max(2, 2 * T // 3)), (5000, 1)]


class Model:
    """One test model: the device tagger, both oracles, the device's features of the three plan windows, and the three
    results on the first ``n_windows`` of them."""

    def __init__(self, cfg, n_windows, seed):
        from eioku_amd.sounds import SoundTagger

        self.cfg, self.n, self.weights = cfg, n_windows, so.random_weights(cfg, seed)
        self.dev = SoundTagger({k: v.numpy() for k, v in self.weights.items()}, so.hf_config(cfg))
        self.o32, self.o16 = so.Oracle(cfg, self.weights, False), so.Oracle(cfg, self.weights, True)
        self.audio, self.plan = so.audio(3000 + _span(cfg), seed + 1), _plan(cfg)
        spec, rows = self.dev.features(self.audio, self.plan)
        self.spec, self.rows = spec.cpu().numpy(), rows.cpu().numpy()
        f32 = self.rows[:n_windows].astype(np.float32)
        self.h32, self.l32 = (t.numpy() for t in self.o32.forward(f32))
        self.h16, self.l16 = (t.numpy() for t in self.o16.forward(f32))
        self.logits, self.hidden = self.run(self.rows[:n_windows])

    def run(self, rows):
        logits, hidden = self.dev.forward_raw(torch.from_numpy(rows).cuda(), with_hidden=True)
        return logits.cpu().numpy(), hidden.cpu().numpy()


def _model(cfg, n_windows, seed):
    m = Model(cfg, n_windows, seed)
    yield m
    m.dev.close()


@pytest.fixture(scope="module")
def model_s(gpu):
    yield from _model(so.config_s(), 3, 11)


@pytest.fixture(scope="module")
def model_r(gpu):
    yield from _model(so.config_r(), 3, 13)


@pytest.fixture(scope="module")
def model_w(gpu):
    yield from _model(so.config_w(), 1, 17)


@pytest.fixture(scope="module")
def model_l(gpu):
    yield from _model(so.config_l(), 2, 19)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint16)


# ---- 1. features ---------------------------------------------------------------------------------------------------------------
def _check_features(name, m):
    """The project's K22 / K24 rule: the device may differ from the float64 oracle by at most four times what the oracle's
    own float32 mode does on the same windows."""
    cfg = m.cfg
    T, mel = cfg["max_length"], cfg["mel"]
    want = so.fbank_plan(m.audio, m.plan, T, mel)
    w32 = so.fbank_plan(m.audio, m.plan, T, mel, np.float32)
    bar = 4 * float(np.abs(w32.astype(np.float64) - want).max())
    diff = float(np.abs(m.spec.astype(np.float64) - want).max())
    print(f"{name} features: device vs float64 oracle {diff:.3e}; bar (4 x the oracle's float32 mode) {bar:.3e}")
    assert m.spec.shape == want.shape == (3, T, mel) and np.isfinite(m.spec).all()
    assert diff <= bar
    for (_, valid), spec in zip(m.plan, m.spec):
        assert np.array_equal(_bits(spec[valid:]), _bits(np.full((T - valid, mel), PAD))) and (spec[:valid] != PAD).any()
    # the patch rows: the gather of the device's own spectrogram, rounded to fp16
    assert np.array_equal(_bits(m.rows), _bits(so.patch_rows(m.spec, cfg).astype(np.float16)))


def test_features_s(model_s):
    _check_features("S", model_s)


def test_features_r(model_r):
    _check_features("R", model_r)


def test_features_w(model_w):
    _check_features("W", model_w)


# ---- 2. drift ------------------------------------------------------------------------------------------------------------------
def _drift(got, ref):
    """(mean, max) of |got - ref| as fractions of the reference RMS"""
    rms = float(np.sqrt(np.mean(np.square(ref, dtype=np.float64))))
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    return float(d.mean()) / rms, float(d.max()) / rms


def _check_drift(name, got, ref32, ref16):
    """The rule of tests/test_actions_gpu.py: the device may drift from the fp32 oracle by at most twice what the oracle's own
    fp16 mode does on the same input."""
    assert got.shape == ref32.shape and np.isfinite(got).all()
    bar_mean, bar_max = (2 * v for v in _drift(ref16, ref32))
    mean, mx = _drift(got, ref32)
    print(f"{name}: device drift mean {mean:.3e} max {mx:.3e} of the rms; bar (2 x CPU fp16 drift) mean {bar_mean:.3e} max {bar_max:.3e}")
    assert mean <= bar_mean and mx <= bar_max


def _check_model_drift(name, m):
    """Measured values: DESIGN.md "K29 sound events"."""
    _check_drift(f"{name} hidden", m.hidden, m.h32, m.h16)
    _check_drift(f"{name} logits", m.logits, m.l32, m.l16)


def test_hidden_and_logits_drift_s(model_s):
    assert model_s.hidden.shape == (3, 10, 128)
    _check_model_drift("S", model_s)


def test_hidden_and_logits_drift_r(model_r):
    assert model_r.hidden.shape == (3, 22, 128)
    _check_model_drift("R", model_r)


def test_hidden_and_logits_drift_w(model_w):
    assert model_w.hidden.shape == (1, 206, 768)
    _check_model_drift("W", model_w)


def test_hidden_and_logits_drift_l(model_l):
    assert model_l.hidden.shape == (2, 1214, 128)
    _check_model_drift("L", model_l)


def test_embedding_alone_w(gpu, model_w):
    """A zero-layer handle with W's embedding weights: hidden_out is the embedding, so an error in the token order or the
    position rows shows here on its own (it would move rows by whole position embeddings: 0.2 rms against a bar near 1e-3)."""
    from eioku_amd.sounds import SoundTagger

    cfg = so.config_w(layers=0)
    weights = {k: v for k, v in model_w.weights.items() if ".layers." not in k}
    dev = SoundTagger({k: v.numpy() for k, v in weights.items()}, so.hf_config(cfg))
    try:
        logits, hidden = dev.forward_raw(torch.from_numpy(model_w.rows[:2]).cuda(), with_hidden=True)
        f32 = model_w.rows[:2].astype(np.float32)
        h32, l32 = (t.numpy() for t in so.Oracle(cfg, weights, False).forward(f32))
        h16, l16 = (t.numpy() for t in so.Oracle(cfg, weights, True).forward(f32))
        _check_drift("W embedding", hidden.cpu().numpy(), h32, h16)
        _check_drift("W embedding logits", logits.cpu().numpy(), l32, l16)
    finally:
        dev.close()


# ---- 3. independence -------------------------------------------------------------------------------------------------------------
def test_a_window_does_not_depend_on_its_batch(model_s):
    for i in range(3):
        logits, hidden = model_s.run(model_s.rows[i:i + 1])
        assert np.array_equal(_bits(logits[0]), _bits(model_s.logits[i]))
        assert np.array_equal(_bits(hidden[0]), _bits(model_s.hidden[i]))


def test_classify_does_not_depend_on_batching_or_on_where_the_audio_is(model_s):
    m = model_s
    ref = m.dev.classify(m.audio, m.plan, 7, batch_windows=32, with_logits=True, with_hidden=True)
    # the whole path gives what its stages give
    assert np.array_equal(_bits(ref[2]), _bits(m.logits)) and np.array_equal(_bits(ref[3]), _bits(m.hidden))
    one = m.dev.classify(m.audio, m.plan, 7, batch_windows=1, with_logits=True, with_hidden=True)
    dev = m.dev.classify(torch.from_numpy(m.audio).cuda(), m.plan, 7, batch_windows=32, with_logits=True, with_hidden=True)
    for got in (one, dev):
        assert np.array_equal(got[1], ref[1])
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip((got[0], got[2], got[3]), (ref[0], ref[2], ref[3])))
    ms = m.dev.last_ms()
    assert ms["features"] > 0 and ms["encoder"] > 0 and ms["head"] > 0 and m.dev.last_flops() > 0


def test_more_windows_than_one_pass(model_s):
    """65 windows, 40 samples apart: two device calls at 64 windows per call, 65 at one."""
    m = model_s
    plan = [(40 * i, 48 if i % 3 else 20) for i in range(65)]
    a = m.dev.classify(m.audio, plan, 3, batch_windows=64, with_logits=True)
    b = m.dev.classify(None, plan, 3, batch_windows=1, with_logits=True)
    assert a[0].shape == (65, 3) and np.array_equal(a[1], b[1])
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[2]), _bits(b[2]))
    assert len({l.tobytes() for l in a[2]}) == 65  # 65 different windows


def test_samples_past_the_valid_frames_are_not_read(model_s):
    m = model_s
    first, valid = m.plan[1]
    end = first + 400 + 160 * (valid - 1)
    other = m.audio.copy()
    other[end:] = np.random.default_rng(5).uniform(-0.5, 0.5, other.size - end).astype(np.float32)
    a = m.dev.classify(m.audio, [(first, valid)], 7, with_logits=True, with_hidden=True)
    b = m.dev.classify(other, [(first, valid)], 7, with_logits=True, with_hidden=True)
    assert np.array_equal(_bits(a[2]), _bits(b[2])) and np.array_equal(_bits(a[3]), _bits(b[3]))
    other[end - 1] += 0.25  # the last sample of the last valid frame is read
    c = m.dev.classify(other, [(first, valid)], 7, with_logits=True)
    assert not np.array_equal(_bits(a[2]), _bits(c[2]))


# ---- 4. the head -----------------------------------------------------------------------------------------------------------------
def _check_topk(dev, logits, top_k):
    scores, ids = (t.cpu().numpy() for t in dev.topk(torch.from_numpy(logits).cuda(), top_k))
    want_s, want_i = so.sigmoid_topk(logits, top_k)
    assert np.array_equal(ids, want_i) and ids.dtype == np.int32 and scores.dtype == np.float32
    ulps = np.abs(scores.astype(np.float64) - want_s) / np.spacing(want_s)
    print(f"top-{top_k} of {logits.shape}: max sigmoid difference {ulps.max():.2f} ulp")
    assert (ulps <= 2).all()


def test_head_selection_on_the_device_logits(model_s, model_w):
    for k in (1, 5, 7):
        _check_topk(model_s.dev, model_s.logits, k)
    for k in (1, 5, 527):
        _check_topk(model_w.dev, model_w.logits, k)
    scores, ids = model_w.dev.classify(model_w.audio, model_w.plan[:1], 5)
    assert np.array_equal(ids, so.sigmoid_topk(model_w.logits, 5)[1])


def test_head_ties_go_to_the_smaller_index(model_w):
    logits = np.zeros((2, 527), np.float32)
    logits[0, [526, 7, 260, 3]] = 2.0           # four equal maxima, then 523 equal values
    logits[1] = np.float32(-1.5)                # all equal
    scores, ids = (t.cpu().numpy() for t in model_w.dev.topk(torch.from_numpy(logits).cuda(), 6))
    assert ids[0].tolist() == [3, 7, 260, 526, 0, 1] and ids[1].tolist() == [0, 1, 2, 3, 4, 5]
    _check_topk(model_w.dev, logits, 6)
    _check_topk(model_w.dev, logits, 527)


def test_head_picks_logits_at_the_floor_in_index_order(model_s):
    """-inf is the selection's floor: such logits are picked after every finite one, in index order, with a score of 0, and a
    pick that was taken (NaN) never comes back."""
    logits = np.array([[-np.inf, 0.5, -np.inf, 0.5, -1.0, -np.inf, -np.inf]], np.float32)
    assert so.sigmoid_topk(logits, 7)[1].tolist() == [[1, 3, 4, 0, 2, 5, 6]]
    scores, ids = (t.cpu().numpy() for t in model_s.dev.topk(torch.from_numpy(logits).cuda(), 7))
    assert ids.tolist() == [[1, 3, 4, 0, 2, 5, 6]]
    assert (scores[0, 3:] == 0.0).all()
    _check_topk(model_s.dev, logits, 7)


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------
E2E_SEED, E2E_AUDIO_SEED = 48, 41


def _write_wav(path, samples):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.clip(np.round(samples * 32768.0), -32768, 32767).astype("<i2").tobytes())


def test_detect_sounds_end_to_end_w(gpu, tmp_path):
    """A 25 s WAV -> windows -> labels, against the fp32 oracle on the oracle's own features.  The comparison is only
    meaningful while the oracle's six best logits of every window are further apart than the device may drift, so that
    condition is asserted, not assumed.  25 windows of 527 labels have 125 such gaps, and independent ones are never all wide:
    the signal repeats every second under a slowly rising gain (``sounds_oracle.steady_audio``), so the windows' logits differ
    by about 0.03 and their gaps move together; the weight seed was then chosen on the CPU (gap 0.11 against an fp16-mode
    drift of the oracle of 0.005).  The last window is partial (98 valid frames) and has other labels than the full ones."""
    from eioku_amd import task_handler
    from eioku_amd.model_manager import ModelManager
    from eioku_amd.sounds import SoundTagger, plan_windows, random_state
    from eioku_amd.transcribe import read_wav

    cfg = so.config_w()
    hf = so.hf_config(cfg)
    root = tmp_path / "cache" / "ast" / "tiny-w"
    root.mkdir(parents=True)
    (root / "config.json").write_text(json.dumps(hf))
    _write_wav(tmp_path / "clip.wav", so.steady_audio(25, E2E_AUDIO_SEED))
    samples, rate = read_wav(tmp_path / "clip.wav")
    n, span = samples.size, _span(cfg)
    plan = plan_windows(n, cfg["max_length"], 16000)
    assert rate == 16000 and [p[0] for p in plan] == [16000 * i for i in range(25)] and plan[-1][1] == 1 + (16000 - 400) // 160

    state = random_state(hf, E2E_SEED)
    rows = so.patch_rows(so.fbank_plan(samples, plan, cfg["max_length"], cfg["mel"]), cfg).astype(np.float16).astype(np.float32)
    l32 = so.Oracle(cfg, state, False).forward(rows)[1].numpy()
    dev = SoundTagger.from_cache(tmp_path / "cache", "tiny-w", seed=E2E_SEED)
    try:
        logits = dev.classify(samples, plan, 5, with_logits=True)[2]
    finally:
        dev.close()
    drift = float(np.abs(logits - l32).max())
    top6 = -np.sort(-l32, axis=1)[:, :6]
    gap = float(np.min(top6[:, :-1] - top6[:, 1:]))
    print(f"W end to end: max logit drift {drift:.3e}, smallest gap among the oracle's six best logits of a window {gap:.3e}")
    assert gap > 4 * drift
    want_s, want_i = so.sigmoid_topk(l32, 5)
    assert len({tuple(r) for r in want_i}) >= 2

    mm = ModelManager(cache_dir=str(tmp_path / "cache"), random_init_seed=E2E_SEED)
    config = {"model_name": "tiny-w", "window_stride": 1.0}
    out = asyncio.run(mm.detect_sounds(str(tmp_path / "clip.wav"), config))
    assert sorted(out) == ["sounds"] and len(out["sounds"]) == len(plan) == 25
    for item, (first, _), ids in zip(out["sounds"], plan, want_i):
        assert sorted(item) == ["end_ms", "labels", "scores", "start_ms", "timestamp_ms"]
        assert item["start_ms"] == item["timestamp_ms"] == first * 1000 // 16000
        assert item["end_ms"] == min(n, first + span) * 1000 // 16000
        assert item["labels"] == [f"LABEL_{i}" for i in ids]
        assert all(type(item[k]) is int for k in ("start_ms", "end_ms", "timestamp_ms"))
        assert all(type(v) is str for v in item["labels"]) and all(type(v) is float for v in item["scores"])
        assert item["scores"] == sorted(item["scores"], reverse=True) and len(item["scores"]) == 5
    assert out["sounds"][-1]["end_ms"] == 25000 and out["sounds"][0]["end_ms"] == span * 1000 // 16000
    # min_score: a prefix of every window's list
    bar = float(np.median([s for item in out["sounds"] for s in item["scores"]]))
    kept = asyncio.run(mm.detect_sounds(str(tmp_path / "clip.wav"), {**config, "min_score": bar}))["sounds"]
    assert 0 < sum(len(k["scores"]) for k in kept) < 125 and len(kept) == 25
    for k, item in zip(kept, out["sounds"]):
        m = sum(s >= bar for s in item["scores"])
        assert k["scores"] == item["scores"][:m] and k["labels"] == item["labels"][:m] and k["start_ms"] == item["start_ms"]
    # the task: one envelope per window
    got = []
    ctx = {"model_manager_factory": lambda cache_dir: mm, "artifact_sink": got.extend}
    res = asyncio.run(task_handler.process_ml_task(ctx, "t1", "sound_detection", "vid", str(tmp_path / "clip.wav"), config))
    assert res == {"task_id": "t1", "status": "completed", "artifact_count": 25}
    assert [json.loads(e.payload_json) for e in got] == out["sounds"] and {e.artifact_type for e in got} == {"sound.detection"}
    assert [(e.span_start_ms, e.span_end_ms) for e in got] == [(s["start_ms"], s["end_ms"]) for s in out["sounds"]]
    # under one frame of audio: no windows
    _write_wav(tmp_path / "short.wav", so.audio(399, 1))
    assert asyncio.run(mm.detect_sounds(str(tmp_path / "short.wav"), config)) == {"sounds": []}


# ---- 6. limits -------------------------------------------------------------------------------------------------------------------
def test_limits_and_handle_lifecycle(gpu, model_s):
    from eioku_amd._buffers import ptr
    from eioku_amd._handle import Handle
    from eioku_amd._lib import EiokuHipError
    from eioku_amd.sounds import ast_tables

    def create(mel=32, length=48, fs=10, ts=10, hidden=128, layers=1, heads=2, ffn=256, labels=7, eps=1e-12):
        window, m = ast_tables(min(max(mel, 1), 128))
        return Handle("ast", mel, length, fs, ts, hidden, layers, heads, ffn, labels, eps, ptr(window), ptr(m), so.MEAN, so.STD)

    for kw, match in [({"heads": 4}, "head_dim must be 64"), ({"mel": 15}, r"num_mel_bins must be in \[16, 128\]"),
                      ({"mel": 129}, r"num_mel_bins must be in \[16, 128\]"), ({"length": 15}, "max_length must be at least 16"),
                      ({"mel": 128, "length": 3426}, "at most 4094 tokens"),  # 12 x 341 + 2 = 4094 tokens fit, 12 x 342 + 2 do not
                      ({"fs": 0}, r"frequency_stride must be in \[1, 16\]"), ({"fs": 17}, r"frequency_stride must be in \[1, 16\]"),
                      ({"ts": 0}, r"time_stride must be in \[1, 16\]"), ({"ts": 17}, r"time_stride must be in \[1, 16\]"),
                      ({"labels": 0}, "num_labels must be at least 1"), ({"ffn": 100}, "bad config")]:
        with pytest.raises(EiokuHipError, match=match):
            create(**kw)
    h = create()
    names = [n for n, _, _ in h.tensors()]
    assert names[0] == "audio_spectrogram_transformer.embeddings.cls_token" and names[-1] == "classifier.dense.bias"
    assert len(names) == 5 + 16 + 6
    assert names == list(so.random_weights({**so.config_s(), "layers": 1}, 0))  # the state_dict() order
    shapes = dict((n, (r, c)) for n, r, c in h.tensors())
    assert shapes["audio_spectrogram_transformer.embeddings.patch_embeddings.projection.weight"] == (128, 256)
    assert shapes["audio_spectrogram_transformer.embeddings.position_embeddings"] == (10, 128)
    rows = torch.zeros((1, 8, 256), dtype=torch.float16, device="cuda")
    logits = torch.empty((1, 7), dtype=torch.float32, device="cuda")
    rc = h.eioku_ast_forward(rows.data_ptr(), 1, logits.data_ptr(), None, None)
    assert rc != 0 and b"has no weights" in h.lib.eioku_last_error()
    h.close()
    h.close()  # idempotent
    with pytest.raises(EiokuHipError, match="closed"):
        h.eioku_ast_num_tensors()
    # the pass limit, a plan outside the audio, and the published file's older tensor names
    m = model_s
    with pytest.raises(EiokuHipError, match="at most 64 windows"):
        m.dev.features(m.audio, [(0, 1)] * 65)
    with pytest.raises(EiokuHipError, match="outside the audio"):
        m.dev.features(m.audio, [(m.audio.size - 399, 1)])
    with pytest.raises(EiokuHipError, match=r"valid frames outside \[1, 48\]"):
        m.dev.features(m.audio, [(0, 49)])
    from eioku_amd.sounds import SoundTagger

    old = SoundTagger(so.old_layout({k: v.numpy() for k, v in m.weights.items()}), so.hf_config(m.cfg))
    try:
        logits = old.forward_raw(torch.from_numpy(m.rows).cuda()).cpu().numpy()
        assert np.array_equal(_bits(logits), _bits(m.logits))
        old.close()
        old.close()
        with pytest.raises(EiokuHipError, match="closed"):
            old.classify(m.audio, m.plan, 1)
    finally:
        old.close()
