"""K25 on the host: the oracle against ``transformers``, the preprocessing restatement against the Pillow fixture, the
loaders, the config checks, the window rule of ``detect_actions`` and the task plumbing.  No GPU."""
import asyncio
import json
import struct

import numpy as np
import pytest
import torch

import actions_oracle as ao
from eioku_amd import actions, task_handler
from eioku_amd.frames import FrameSource
from eioku_amd.model_manager import ModelManager

SOURCES = [(54, 96), (96, 54), (30, 40), (48, 48), (49, 97)]


# ---- the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S", "S1"])
def test_fp32_oracle_equals_transformers(name):
    """Measured here: hidden 7.9e-6 / logits 1.1e-5 at S, 6.2e-6 / 1.3e-5 at S1, on values up to 9 (hidden) and 27 (logits):
    a few fp32 roundings (6e-8 relative) of sums of that size.  The bar is 5e-5: that order, nothing a wrong token order,
    CLS rule or epsilon could meet (each moves the output by 1e-2 or more)."""
    tr = pytest.importorskip("transformers")
    cfg = ao.config_s() if name == "S" else ao.config_s1()
    w = ao.random_weights(cfg, 3)
    model = tr.TimesformerForVideoClassification(tr.TimesformerConfig(**ao.hf_config(cfg))).eval()
    model.load_state_dict(w, strict=True)
    rows = np.random.default_rng(1).standard_normal((2, 9, cfg["frames"], 768)).astype(np.float32)
    pix = torch.from_numpy(ao.pixel_values(rows, cfg["image"]))
    with torch.no_grad():
        logits = model(pixel_values=pix).logits
        hidden = model.timesformer.encoder(model.timesformer.embeddings(pix))[0]
    h, lg = ao.Oracle(cfg, w, fp16=False).forward(rows)
    dh, dl = (hidden - h).abs().max().item(), (logits - lg).abs().max().item()
    print(f"{name}: oracle vs transformers: hidden {dh:.3e} (max |.| {hidden.abs().max():.2f}), logits {dl:.3e} "
          f"(max |.| {logits.abs().max():.2f})")
    assert hidden.shape == h.shape == (2, 1 + 9 * cfg["frames"], cfg["hidden"])
    assert dh <= 5e-5 and dl <= 5e-5


def test_patch_row_relayout_round_trips():
    x = np.random.default_rng(0).standard_normal((2, 3, 48, 48, 3)).astype(np.float32)
    rows = ao.patch_rows(x)
    assert rows.shape == (2, 9, 3, 768)
    # patch 4 (row 1, column 1), frame 2, channel 1, ky 5, kx 7
    assert rows[1, 4, 2, 256 + 5 * 16 + 7] == x[1, 2, 16 + 5, 16 + 7, 1]
    assert np.array_equal(ao.pixel_values(rows, 48), x.transpose(0, 1, 4, 2, 3))


# ---- preprocessing ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    from pathlib import Path

    return np.load(Path(__file__).resolve().parent / "golden" / "actions_preproc.npz")


@pytest.mark.parametrize("h,w", SOURCES)
def test_preprocessing_restatement_equals_pillow_and_the_image_processor(golden, h, w):
    u8, norm = ao.preprocess(golden[f"bgr_{h}x{w}"], 48, 48)
    assert np.array_equal(u8, golden[f"u8_{h}x{w}"])
    assert np.abs(norm - golden[f"norm_{h}x{w}"]).max() <= 1e-6


@pytest.mark.parametrize("h,w", SOURCES)
def test_clip_tables_are_the_cropped_rows_of_the_full_tables(h, w):
    """The product's tables compute only the crop: applying them gives the oracle's resize-then-crop image."""
    from oracle.places import _pass

    rng = np.random.default_rng(h * 100 + w)
    bgr = rng.integers(0, 256, (1, h, w, 3), dtype=np.uint8)
    xb, xk, kx, yb, yk, ky = actions.clip_tables(h, w, 48, 48)
    assert xb.shape == yb.shape == (48, 2) and xk.shape == (48, kx) and yk.shape == (48, ky)
    assert (xb[:, 0] >= 0).all() and (xb.sum(1) <= w).all() and (yb[:, 0] >= 0).all() and (yb.sum(1) <= h).all()
    img = _pass(_pass(np.ascontiguousarray(bgr[0][..., ::-1]), xb, xk, axis=1), yb, yk, axis=0)
    assert np.array_equal(img, ao.preprocess(bgr, 48, 48)[0][0])


def test_clip_tables_refuse_a_frame_smaller_than_the_crop_after_resize():
    assert actions.clip_tables(10, 10, 48, 48)[0].shape == (48, 2)  # upscaling is fine
    with pytest.raises(ValueError, match="smaller than the 48 crop"):
        actions.clip_tables(100, 100, 32, 48)


# ---- loading ---------------------------------------------------------------------------------------------------------------
def _write_safetensors(path, tensors):
    header, blobs, off = {}, [], 0
    for k, v in tensors.items():
        raw = np.ascontiguousarray(v, dtype=np.float32).tobytes()
        header[k] = {"dtype": "F32", "shape": list(v.shape), "data_offsets": [off, off + len(raw)]}
        blobs.append(raw)
        off += len(raw)
    hj = json.dumps(header).encode()
    path.write_bytes(struct.pack("<Q", len(hj)) + hj + b"".join(blobs))


def test_state_dict_round_trips_through_safetensors(tmp_path):
    cfg = ao.config_s()
    root = tmp_path / "timesformer" / "tiny"
    root.mkdir(parents=True)
    tr = pytest.importorskip("transformers")
    model = tr.TimesformerForVideoClassification(tr.TimesformerConfig(**ao.hf_config(cfg)))
    sd = model.state_dict()
    st = pytest.importorskip("safetensors.torch")
    st.save_file({k: v.contiguous() for k, v in sd.items()}, str(root / "model.safetensors"))
    got = actions.read_state(root)
    assert sorted(got) == sorted(sd)
    for k, v in sd.items():
        assert np.array_equal(got[k], v.numpy()), k
    # every tensor the library asks for is there, in the shape it expects
    shapes = dict(actions.tensor_shapes(actions.timesformer_dims(ao.hf_config(cfg))))
    assert sorted(shapes) == sorted(sd)
    assert all(tuple(sd[k].shape) == shapes[k] for k in shapes)


def test_read_state_reads_the_minimal_writer_and_refuses_an_empty_directory(tmp_path):
    w = {"classifier.bias": np.arange(7, dtype=np.float32), "classifier.weight": np.ones((7, 128), np.float32)}
    _write_safetensors(tmp_path / "model.safetensors", w)
    got = actions.read_state(tmp_path)
    assert np.array_equal(got["classifier.bias"], w["classifier.bias"]) and got["classifier.weight"].shape == (7, 128)
    (tmp_path / "empty").mkdir()
    with pytest.raises(FileNotFoundError):
        actions.read_state(tmp_path / "empty")


def test_random_state_has_the_state_dict_shapes():
    cfg = ao.hf_config(ao.config_s())
    sd = actions.random_state(cfg, 5)
    ref = ao.random_weights(ao.config_s(), 0)
    assert sorted(sd) == sorted(ref)
    assert all(sd[k].shape == tuple(ref[k].shape) and sd[k].dtype == np.float32 for k in sd)
    again = actions.random_state(cfg, 5)
    assert all(np.array_equal(sd[k], again[k]) for k in sd)
    assert not np.array_equal(sd["classifier.weight"], actions.random_state(cfg, 6)["classifier.weight"])


def test_from_cache_without_a_directory_raises(tmp_path):
    with pytest.raises(FileNotFoundError, match="config.json"):
        actions.ActionRecognizer.from_cache(tmp_path, "timesformer-base-finetuned-k400")


@pytest.mark.parametrize("change,match", [
    ({"num_attention_heads": 4}, "head dimension must be 64"),
    ({"patch_size": 8}, "patch_size must be 16"),
    ({"image_size": 40}, "image_size must be a multiple of 16"),
    ({"image_size": 464}, "at most 448"),
    ({"num_frames": 97}, r"num_frames must be in \[1, 96\]"),
    ({"num_frames": 0}, r"num_frames must be in \[1, 96\]"),
    ({"attention_type": "space_only"}, "attention_type 'space_only' is not built"),
    ({"attention_type": "joint_space_time"}, "is not built"),
    ({"intermediate_size": 100}, "multiple of 32"),
])
def test_config_validation(change, match):
    with pytest.raises(ValueError, match=match):
        actions.timesformer_dims({**ao.hf_config(ao.config_s()), **change})


def test_config_defaults_and_labels():
    d = actions.timesformer_dims({})
    assert (d["image"], d["frames"], d["hidden"], d["layers"], d["heads"], d["ffn"], d["labels"]) == (224, 8, 768, 12, 12, 3072, 400)
    assert d["ln_eps"] == 1e-6
    assert actions.config_labels({"id2label": {"0": "abseiling", "2": "archery"}}, 3) == ["abseiling", "action_1", "archery"]
    pre = actions.preprocessing({})
    assert pre == {"shortest_edge": 224, "crop": 224, "mean": (0.45,) * 3, "std": (0.225,) * 3}
    pre = actions.preprocessing({}, {"size": {"shortest_edge": 256}, "image_mean": [0.5, 0.4, 0.3], "image_std": [0.2, 0.2, 0.2]})
    assert pre["shortest_edge"] == 256 and pre["mean"] == (0.5, 0.4, 0.3)
    with pytest.raises(ValueError, match="crop_size"):
        actions.preprocessing({}, {"crop_size": {"height": 256, "width": 256}})


@pytest.mark.parametrize("config,match", [
    ({"top_k": 0}, "action_detection: top_k"), ({"top_k": 2.5}, "action_detection: top_k"), ({"top_k": True}, "action_detection: top_k"),
    ({"clip_stride": 0}, "action_detection: clip_stride"), ({"clip_stride": "8"}, "action_detection: clip_stride"),
    ({"frame_interval": -1}, "action_detection: frame_interval"), ({"model_name": "../x"}, "action_detection: model_name"),
    ({"model_name": 3}, "action_detection: model_name"),
])
def test_task_settings_refuse_bad_values(config, match):
    with pytest.raises(ValueError, match=match):
        actions.action_settings(config, 8, 400)


def test_task_settings_defaults_and_clamp():
    s = actions.action_settings({}, 8, 400)
    assert s == {"model_name": "timesformer-base-finetuned-k400", "frame_interval": 1, "top_k": 5, "clip_stride": 8}
    assert actions.action_settings({"top_k": 9}, 3, 7)["top_k"] == 7
    assert actions.action_settings({"clip_stride": 2}, 3, 7)["clip_stride"] == 2


# ---- the window rule ---------------------------------------------------------------------------------------------------------
class _Frames(FrameSource):
    """n frames of 4 x 6; every pixel of frame i is i."""

    def __init__(self, n, fps=10.0):
        self.n, self.fps, self.total_frames, self.pos, self.released = n, fps, n, 0, False

    def read(self):
        if self.pos >= self.n:
            return False, None
        self.pos += 1
        return True, np.full((4, 6, 3), self.pos - 1, np.uint8)

    def grab(self):
        if self.pos >= self.n:
            return False
        self.pos += 1
        return True

    def release(self):
        self.released = True


class _Recognizer:
    """Records the clips it is given; class = first frame's value mod labels."""
    frames, labels = 4, [f"a{i}" for i in range(6)]

    def __init__(self):
        self.clips, self.calls, self.closed = [], 0, False

    def classify(self, clips, top_k):
        assert isinstance(clips, np.ndarray) and clips.shape[1:] == (self.frames, 4, 6, 3) and clips.dtype == np.uint8
        self.calls += 1
        self.clips.extend(c[:, 0, 0, 0].tolist() for c in clips)
        ids = np.stack([(int(c[0, 0, 0, 0]) + np.arange(top_k)) % len(self.labels) for c in clips]).astype(np.int32)
        probs = np.tile(np.float32(0.5) ** np.arange(1, top_k + 1, dtype=np.float32), (len(clips), 1))
        return probs, ids

    def close(self):
        self.closed = True


def _run(n_frames, config, batch_size=64, fps=10.0):
    rec, src = _Recognizer(), _Frames(n_frames, fps)
    mm = ModelManager(cache_dir="/tmp/eioku-test-cache", frame_source=lambda p: src, batch_size=batch_size,
                      action_recognizer_factory=lambda cache, name: rec)
    out = asyncio.run(mm.detect_actions("video.mp4", config))
    assert rec.closed and src.released
    return out["actions"], rec


@pytest.mark.parametrize("batch_size", [64, 3, 1])
def test_windows_exact_and_remainder_dropped(batch_size):
    # fps 10, frame_interval 0.2 s: every 2nd frame is sampled; 19 frames -> 10 sampled (0, 2, .., 18) -> 2 clips of 4, 2 left over
    acts, rec = _run(19, {"frame_interval": 0.2, "top_k": 2}, batch_size)
    assert rec.clips == [[0, 2, 4, 6], [8, 10, 12, 14]]
    assert [(a["frame_index"], a["timestamp_ms"], a["start_ms"], a["end_ms"]) for a in acts] == [(0, 0, 0, 600), (8, 800, 800, 1400)]
    assert acts[1]["labels"] == ["a2", "a3"] and acts[1]["scores"] == [0.5, 0.25]
    assert all(type(s) is float for a in acts for s in a["scores"]) and all(type(a["frame_index"]) is int for a in acts)
    # 8 sampled frames: exactly two windows, nothing dropped
    assert _run(8, {"frame_interval": 0.1}, batch_size)[1].clips == [[0, 1, 2, 3], [4, 5, 6, 7]]
    windows = actions.clip_windows(10, 4, 4)
    assert windows == [(0, 3), (4, 7)] and actions.clip_windows(8, 4, 4) == [(0, 3), (4, 7)]


@pytest.mark.parametrize("batch_size", [64, 2])
def test_short_video_is_padded_with_its_last_frame(batch_size):
    acts, rec = _run(3, {"frame_interval": 0.1}, batch_size)
    assert rec.clips == [[0, 1, 2, 2]]
    assert [(a["frame_index"], a["start_ms"], a["end_ms"]) for a in acts] == [(0, 0, 200)]
    assert len(acts[0]["labels"]) == 5  # top_k default
    assert actions.clip_windows(3, 4, 4) == [(0, 2)] and actions.clip_windows(0, 4, 4) == []
    assert _run(0, {})[0] == []


@pytest.mark.parametrize("batch_size", [64, 3, 1])
def test_overlapping_and_sparse_strides(batch_size):
    acts, rec = _run(9, {"frame_interval": 0.1, "clip_stride": 2}, batch_size)
    assert rec.clips == [[0, 1, 2, 3], [2, 3, 4, 5], [4, 5, 6, 7]]  # the window at 6 would need frame 9
    assert [w[0] for w in actions.clip_windows(9, 4, 2)] == [0, 2, 4]
    assert [a["end_ms"] for a in acts] == [300, 500, 700]
    acts, rec = _run(14, {"frame_interval": 0.1, "clip_stride": 6}, batch_size)
    assert rec.clips == [[0, 1, 2, 3], [6, 7, 8, 9]] and actions.clip_windows(14, 4, 6) == [(0, 3), (6, 9)]


def test_top_k_is_clamped_to_the_label_count_and_bad_values_raise():
    acts, _ = _run(4, {"frame_interval": 0.1, "top_k": 50})
    assert len(acts[0]["labels"]) == 6 == len(acts[0]["scores"])
    with pytest.raises(ValueError, match="action_detection: top_k"):
        _run(4, {"top_k": 0})


# ---- task plumbing -----------------------------------------------------------------------------------------------------------
def test_task_tables_name_the_new_type():
    assert task_handler.TASK_TO_ARTIFACT_TYPE["action_detection"] == "action.detection"
    assert task_handler.TASK_TO_RESULT_KEY["action_detection"] == "actions"
    assert "action_detection" in task_handler.KNOWN_TASK_TYPES


def test_process_ml_task_emits_action_envelopes():
    class Stub:
        def __init__(self, cache_dir):
            pass

        async def detect_actions(self, video_path, config):
            assert config == {"top_k": 2}
            return {"actions": [{"frame_index": 0, "timestamp_ms": 0, "start_ms": 0, "end_ms": 700, "labels": ["a", "b"],
                                 "scores": [0.75, 0.125]},
                                {"frame_index": 240, "timestamp_ms": 8000, "start_ms": 8000, "end_ms": 8700, "labels": ["c", "a"],
                                 "scores": [0.5, 0.25]}]}

    got = []
    res = asyncio.run(task_handler.process_ml_task({"model_manager_factory": Stub, "artifact_sink": got.extend}, "t1",
                                                   "action_detection", "vid", "/x.mp4", {"top_k": 2}))
    assert res == {"task_id": "t1", "status": "completed", "artifact_count": 2}
    assert [e.artifact_type for e in got] == ["action.detection"] * 2
    assert [(e.span_start_ms, e.span_end_ms) for e in got] == [(0, 700), (8000, 8700)]
    assert json.loads(got[1].payload_json)["labels"] == ["c", "a"] and got[0].asset_id == "vid"
