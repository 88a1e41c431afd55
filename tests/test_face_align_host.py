"""Host side of face alignment (no GPU): the Umeyama matrices, the Pose rows of the weight table and loader, the
``landmarks`` payload key and the clusterer's embedder seam."""
import asyncio
import sys

import numpy as np
import pytest
import torch

import align_oracle as ao
import test_faces_host as tfh
import test_loaders as tl
from eioku_amd import faces, weights as W

DST = faces.ARCFACE_DST


def _similar(rng, pts, max_deg=60.0, smin=0.3, smax=8.0, jitter=2.0):
    """``pts`` under a random rotation, scale, translation and per-point jitter."""
    a = np.deg2rad(rng.uniform(-max_deg, max_deg))
    s = rng.uniform(smin, smax)
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return s * pts @ R.T + rng.uniform(-500, 1500, 2) + rng.uniform(-jitter, jitter, pts.shape)


def _landmark_sets():
    rng = np.random.default_rng(17)
    sets = [_similar(rng, DST) for _ in range(200)]
    mirrored = _similar(rng, DST * np.array([-1.0, 1.0]))            # det(A) < 0: the reflection branch
    t = np.linspace(-2, 2, 5)[:, None]
    collinear = np.array([300.0, 200.0]) + t * np.array([30.0, 12.0])  # rank 1
    return np.stack(sets + [mirrored, collinear])


def test_align_matrices_equal_the_umeyama_port():
    lm = _landmark_sets()
    M, fallback = faces.align_matrices(lm)
    want = ao.estimate(lm)
    assert M.shape == (202, 2, 3) and M.dtype == np.float64 and not fallback.any()
    assert np.linalg.matrix_rank(np.cov((lm[201] - lm[201].mean(0)).T)) == 1  # the collinear set is what it says
    A = (DST - DST.mean(0)).T @ (lm[200] - lm[200].mean(0))
    assert np.linalg.det(A) < 0                                                # ... and so is the mirrored one
    for i in range(len(lm)):
        assert np.abs(M[i] - want[i]).max() <= 1e-12 * np.abs(want[i]).max(), i
    # a proper similarity everywhere but the mirrored set, where Umeyama refuses the reflection
    lin = M[:, :, :2]
    assert np.all(np.linalg.det(lin[:200]) > 0) and np.linalg.det(lin[200]) >= 0


def test_coincident_landmarks_set_the_mask_without_raising():
    lm = _landmark_sets()[:3].copy()
    lm[1] = np.array([123.0, 45.0])
    M, fallback = faces.align_matrices(lm)
    assert fallback.tolist() == [False, True, False]
    assert np.isfinite(M[[0, 2]]).all()
    M0, f0 = faces.align_matrices(np.zeros((0, 5, 2)))
    assert M0.shape == (0, 2, 3) and f0.shape == (0,)


@pytest.mark.parametrize("s,t", [(1.0, (0.0, 0.0)), (2.5, (100.0, -40.0)), (0.4, (-3.25, 700.5))])
def test_scaled_and_shifted_template_gives_the_inverse_scale_and_shift(s, t):
    M, fallback = faces.align_matrices((DST * s + np.array(t))[None])
    want = np.array([[1 / s, 0, -t[0] / s], [0, 1 / s, -t[1] / s]])
    assert not fallback[0] and np.abs(M[0] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_umeyama_port_equals_skimage():
    tf = pytest.importorskip("skimage.transform")
    for lm in _landmark_sets():
        t = tf.SimilarityTransform()
        t.estimate(lm, DST)
        assert np.allclose(t.params, ao.umeyama(lm, DST), rtol=0, atol=1e-12 * np.abs(t.params).max())


WARP_MATRICES = {  # the GPU test's twelve (tests/test_face_align_gpu.py builds the last one from align_matrices)
    "near identity": [1.0001, 0.0002, 0.3, -0.0002, 0.9999, -0.2],
    "rot 30": [0.8660254037844387, -0.5, 40.0, 0.5, 0.8660254037844387, -20.0],
    "rot -75": [0.2588190451025207, 0.9659258262890683, -30.0, -0.9659258262890683, 0.2588190451025207, 140.0],
    "scale 0.2": [0.2, 0.0, 10.0, 0.0, 0.2, 20.0],
    "scale 5": [5.0, 0.0, -200.0, 0.0, 5.0, -150.0],
    "fractional shift": [1.0, 0.0, -17.37, 0.0, 1.0, -3.61],
    "partly outside": [1.0, 0.0, 60.0, 0.0, 1.0, 55.0],
    "wholly outside": [1.0, 0.0, 4000.0, 0.0, 1.0, 4000.0],
    "negative source": [0.5, 0.0, 100.0, 0.0, 0.5, 90.0],
    "mirrored": [-1.0, 0.0, 130.0, 0.0, 1.0, -4.0],
    "D = 0": [0.0, 0.0, 12.0, 0.0, 0.0, 34.0],
}


def test_warp_oracle_equals_cv2():
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (120, 160, 3), dtype=np.uint8)
    for name, m in WARP_MATRICES.items():
        M = np.array(m, np.float64).reshape(2, 3)
        want = cv2.warpAffine(img, M, (112, 112), flags=cv2.INTER_LINEAR, borderValue=0)
        assert np.array_equal(ao.warp_one(img, M), want), name


def test_warp_oracle_is_exact_where_the_answer_is_known():
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (120, 160, 3), dtype=np.uint8)
    assert np.array_equal(ao.warp_one(img, [1, 0, 0, 0, 1, 0]), img[:112, :112])            # identity
    assert np.array_equal(ao.warp_one(img, [1, 0, -20, 0, 1, -5]), img[5:117, 20:132])      # whole-pixel shift
    assert not ao.warp_one(img, WARP_MATRICES["wholly outside"]).any()                      # borderValue 0
    half = ao.warp_one(img, [1, 0, -0.5, 0, 1, 0]).astype(int)                              # half a pixel: the mean, rounded
    assert np.array_equal(half, (img[:112, :112].astype(int) + img[:112, 1:113] + 1) >> 1)
    assert np.array_equal(ao.warp_one(img, WARP_MATRICES["D = 0"]), np.broadcast_to(img[0, 0], (112, 112, 3)))


# ---- weights ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,c4", [("n", 16), ("s", 32)])
def test_conv_table_appends_the_keypoint_branch(variant, c4):
    base, pose = W.conv_table(variant, 1), W.conv_table(variant, 1, 15)
    assert pose[:len(base)] == base and len(pose) == len(base) + 9
    c3, c4_, c5 = W.YOLO_VARIANTS[variant][0][2:]
    assert pose[len(base):] == [row for l, cx in enumerate((c3, c4_, c5)) for row in (
        (f"model.22.cv4.{l}.0.conv", c4, cx, 3, 1), (f"model.22.cv4.{l}.1.conv", c4, c4, 3, 1), (f"model.22.cv4.{l}.2", 15, c4, 1, 1))]
    assert W.conv_table(variant, 1, 0) == base
    a, b = W.random_state(variant, 1, 3), W.random_state(variant, 1, 3, nk=15)
    assert set(b) - set(a) == {r[0] for r in pose[len(base):]} and W.nk_of_state(a) == 0 and W.nk_of_state(b) == 15
    assert all(np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1]) for k in a)
    for bad in (16, 54, -3):
        with pytest.raises(ValueError):
            W.conv_table(variant, 1, bad)


def _save_pt(tmp_path, nk, monkeypatch):
    """``tests/test_loaders.py``'s fake Ultralytics checkpoint, with a Pose head when ``nk > 0``."""
    mods, K = tl._fake_ultralytics()
    for k, v in mods.items():
        monkeypatch.setitem(sys.modules, k, v)
    monkeypatch.setattr(W, "conv_table", lambda variant, nc, _nk=0, _orig=W.conv_table: _orig(variant, nc, nk))
    model = tl._build_model("n", 1, seed=9, K=K)
    monkeypatch.undo()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    for k, v in mods.items():
        monkeypatch.setitem(sys.modules, k, v)
    path = tmp_path / f"yolov8n-face-{nk}.pt"
    torch.save({"epoch": -1, "model": model.half(), "ema": None, "train_args": {"imgsz": 640}}, path)
    monkeypatch.undo()
    assert "ultralytics" not in sys.modules
    return path, sd


def test_pose_checkpoint_round_trips_and_detect_checkpoint_is_unchanged(tmp_path, monkeypatch):
    path, sd = _save_pt(tmp_path, 15, monkeypatch)
    state, names = W.load_checkpoint(path, "n", 1)
    assert W.nk_of_state(state) == 15 and list(state) == [r[0] for r in W.conv_table("n", 1, 15)] and names == {0: "thing0"}
    for name in ("model.22.cv4.0.0.conv", "model.22.cv4.1.1.conv", "model.22.cv4.2.2", "model.22.cv2.0.2", "model.0.conv"):
        w, b = tl._hand_fold({k: v.half().float() for k, v in sd.items()}, name)  # (the checkpoint stores fp16)
        assert np.allclose(state[name][0], w, rtol=1e-6, atol=1e-7) and np.allclose(state[name][1], b, rtol=1e-6, atol=1e-6), name
    assert state["model.22.cv4.0.2"][0].shape == (15, 16, 1, 1) and state["model.22.cv4.1.0.conv"][0].shape == (16, 128, 3, 3)
    dpath, _ = _save_pt(tmp_path, 0, monkeypatch)
    dstate = W.load_state(dpath, "n", 1)
    assert W.nk_of_state(dstate) == 0 and list(dstate) == [r[0] for r in W.conv_table("n", 1)]
    assert all(np.array_equal(dstate[k][0], state[k][0]) for k in dstate)  # same seed: the shared layers are the same tensors


@pytest.mark.parametrize("nk", [16, 54])
def test_checkpoint_with_a_bad_keypoint_count_is_refused(tmp_path, nk):
    t = {f"{n}.weight": np.zeros((co, ci, k, k), np.float32) for n, co, ci, k, _ in W.conv_table("n", 1)}
    t[W.KPT_KEY] = np.zeros((nk, 16, 1, 1), np.float32)
    np.savez(tmp_path / "bad.npz", **t)
    with pytest.raises(ValueError, match="keypoint"):
        W.load_state(tmp_path / "bad.npz", "n", 1)


# ---- FaceClusterer and the payload ------------------------------------------------------------------------------------------
def test_clusterer_with_an_embed_only_fake_takes_landmarks_or_none():
    log = []
    frames = tfh._frames()
    for lm in (None, np.zeros((2, 5, 2))):
        c = faces.FaceClusterer(tfh._Embedder(log), 0.2, 1)
        dets = [{"cluster_id": None}, {"cluster_id": None}]
        c.add(frames, [(0, 1, 2, 3, 4), (1, 1, 2, 3, 4)], dets, landmarks=lm) if lm is not None else c.add(
            frames, [(0, 1, 2, 3, 4), (1, 1, 2, 3, 4)], dets)
        c.finish()
        assert [d["cluster_id"] for d in dets] == ["face_cluster_001", "face_cluster_002"]
    assert [e[0] for e in log] == ["embed", "cluster"] * 2


def test_clusterer_hands_landmarks_to_embed_aligned():
    calls = []

    class E(tfh._Embedder):
        def embed_aligned(self, frames, boxes, landmarks):
            calls.append((np.asarray(boxes).copy(), np.asarray(landmarks).copy()))
            return self.embed(frames, boxes)

    log = []
    c = faces.FaceClusterer(E(log), 0.2, 1)
    lm = np.arange(20, dtype=np.float64).reshape(2, 5, 2)
    c.add(tfh._frames(), [(0, 1, 2, 3, 4), (1, 1, 2, 3, 4)], [{}, {}], landmarks=lm)
    c.add(tfh._frames(), [(2, 1, 2, 3, 4)], [{}])
    assert len(calls) == 1 and np.array_equal(calls[0][1], lm) and calls[0][0].shape == (2, 5)
    assert [e[0] for e in log] == ["embed", "embed"]  # (the aligned call goes through the fake's embed, the plain one directly)


class _PoseDetector(tfh._Detector):
    """``_Detector`` with five keypoints per face: keypoint k of face i of a frame at (10 k + i, 20 k + i), confidence 0.5."""
    nk = 15

    def detect(self, frames, conf=0.25, with_kpts=False):
        out, counts = super().detect(frames, conf)
        if not with_kpts:
            return out, counts
        kpts = np.zeros((len(frames), 3, 5, 3), np.float32)
        for i in range(2):
            for k in range(5):
                kpts[:, i, k] = (10 * k + i, 20 * k + i, 0.5)
        return out, counts, kpts


def _manager(tmp_path, detector, log):
    from eioku_amd.model_manager import ModelManager

    return ModelManager(cache_dir=str(tmp_path), frame_source=lambda p: tfh._Src(tfh._frames()), detector_factory=lambda m, c: detector,
                        batch_size=2, face_embedder_factory=lambda c, m: tfh._Embedder(log))


def test_landmarks_key_exists_only_with_keypoints(tmp_path):
    plain = asyncio.run(_manager(tmp_path, tfh._Detector(), []).detect_faces("/v.mp4", {"frame_interval": 1}))["detections"]
    pose = asyncio.run(_manager(tmp_path, _PoseDetector(), []).detect_faces("/v.mp4", {"frame_interval": 1}))["detections"]
    assert all("landmarks" not in d for d in plain)
    assert [{k: v for k, v in d.items() if k != "landmarks"} for d in pose] == plain
    for d in pose:  # only the face above the threshold (index 0 of its frame) is emitted
        assert d["landmarks"] == [{"x": 10.0 * k, "y": 20.0 * k, "confidence": 0.5} for k in range(5)]
        assert all(type(v) is float for p in d["landmarks"] for v in p.values())


def test_face_alignment_config(tmp_path):
    log = []
    cfg = {"frame_interval": 1, "cluster_faces": True, "cluster_eps": 0.2}
    with pytest.raises(ValueError, match="5 keypoints"):
        asyncio.run(_manager(tmp_path, tfh._Detector(), log).detect_faces("/v.mp4", dict(cfg, face_alignment=True)))
    assert not [e for e in log if e[0] == "embed"]  # refused before any embedding
    with pytest.raises(ValueError, match="face_alignment"):
        asyncio.run(_manager(tmp_path, _PoseDetector(), log).detect_faces("/v.mp4", dict(cfg, face_alignment="yes")))
    # an embed-only fake embedder: "auto" and False give the same clustering through embed()
    a = asyncio.run(_manager(tmp_path, _PoseDetector(), []).detect_faces("/v.mp4", cfg))["detections"]
    b = asyncio.run(_manager(tmp_path, _PoseDetector(), []).detect_faces("/v.mp4", dict(cfg, face_alignment=False)))["detections"]
    assert a == b and a[0]["cluster_id"] == "face_cluster_001" and "landmarks" in b[0]
