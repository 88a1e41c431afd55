"""Face clustering on the host (no GPU): the arcface_torch state-dict loader and its BatchNorm / fc folding, the crop taps,
the numpy DBSCAN restatement against scikit-learn, and the ModelManager / task-handler wiring with fake detector and
embedder factories."""
import asyncio

import numpy as np
import pytest

import face_oracle as fo
from eioku_amd import faces


@pytest.mark.parametrize("arch", ["r18", "r50"])
def test_loader_infers_depths_and_maps_every_key(arch):
    sd = faces.random_state_dict(1, faces.DEPTHS[arch])
    st = faces.fold_state(sd)
    assert st["depths"] == faces.DEPTHS[arch]
    nb = sum(st["depths"])
    assert len(st["prelu"]) == nb + 1 and len(st["bn"]) == nb
    assert len(st["convs"]) == 1 + 2 * nb + 4
    assert st["head"][0].shape == (512, 25088) and st["head"][1].shape == (512,)
    net = fo.iresnet(sd)  # strict load: the synthetic dict is exactly arcface_torch's key set
    assert set(net.state_dict()) == set(sd)
    # module. prefixes and a "state_dict" wrapper are accepted
    st2 = faces.fold_state({"state_dict": {"module." + k: v for k, v in sd.items()}})
    assert np.array_equal(st2["head"][0], st["head"][0])


def test_loader_rejects_missing_or_misshapen_tensors():
    sd = faces.random_state_dict(1)
    bad = dict(sd)
    del bad["layer2.1.prelu.weight"]
    with pytest.raises(KeyError):
        faces.fold_state(bad)
    bad = dict(sd)
    bad["layer3.0.conv2.weight"] = bad["layer3.0.conv2.weight"][:, :128]
    with pytest.raises(ValueError):
        faces.fold_state(bad)
    bad = dict(sd)
    bad["features.running_var"] = bad["features.running_var"][:10]
    with pytest.raises(ValueError):
        faces.fold_state(bad)
    with pytest.raises(KeyError):
        faces.fold_state({k: v for k, v in sd.items() if not k.startswith("layer4")})


def _conv(x, w, b, stride):
    """float64 NHWC 3x3 (pad 1) or 1x1 (pad 0) convolution."""
    k = w.shape[2]
    p = k // 2
    n, h, wd, c = x.shape
    xp = np.pad(x, ((0, 0), (p, p), (p, p), (0, 0)))
    ho, wo = (h + 2 * p - k) // stride + 1, (wd + 2 * p - k) // stride + 1
    out = np.zeros((n, ho, wo, w.shape[0])) + b
    for dy in range(k):
        for dx in range(k):
            patch = xp[:, dy:dy + stride * ho:stride, dx:dx + stride * wo:stride]
            out += patch @ w[:, :, dy, dx].T.astype(np.float64)
    return out


def test_folding_and_nhwc_fc_permutation_equal_the_unfolded_module():
    """A numpy float64 forward of the FOLDED parameters (NHWC activations, as the device holds them: bn1 and PReLU as
    separate passes, every other BatchNorm inside its conv, the head as one fc over the NHWC flatten) against the torch
    module in float64 on its state dict."""
    import torch
    import torch.nn.functional as F

    sd = faces.random_state_dict(2, (1, 1, 1, 1))
    st = faces.fold_state(sd)
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, (2, 112, 112, 3))

    def prelu(v, a):
        return np.where(v > 0, v, v * a.astype(np.float64))

    cv = st["convs"]
    h = prelu(_conv(x, *cv["conv1"], 1), st["prelu"][0])
    for bi, li in enumerate(range(1, 5)):
        p = f"layer{li}.0"
        s, t = st["bn"][bi]
        u = prelu(_conv(h * s + t, *cv[p + ".conv1"], 1), st["prelu"][bi + 1])
        h = _conv(u, *cv[p + ".conv2"], 2) + _conv(h, *cv[p + ".downsample.0"], 2)
    z = h.reshape(2, -1) @ st["head"][0].T.astype(np.float64) + st["head"][1]
    net = fo.iresnet(sd).double()
    with torch.no_grad():
        want = net(torch.from_numpy(x).permute(0, 3, 1, 2)).numpy()
    rel = np.abs(z - want).max() / np.abs(want).max()
    assert rel < 1e-5, rel  # float32-rounded folded parameters
    assert np.allclose(F.normalize(torch.from_numpy(z), dim=1).numpy(), F.normalize(torch.from_numpy(want), dim=1).numpy(),
                       atol=1e-5)


def test_nchw_to_nhwc_columns():
    w = np.arange(2 * 25088, dtype=np.float64).reshape(2, 25088)
    p = faces.nchw_to_nhwc_columns(w)
    c, y, x = 300, 4, 5
    assert p[1, (y * 7 + x) * 512 + c] == w[1, c * 49 + y * 7 + x]


@pytest.mark.parametrize("box", [(10.0, 20.0, 60.0, 90.0), (-30.0, -10.0, 40.0, 50.0), (150.0, 100.0, 400.0, 300.0),
                                 (33.3, 44.4, 33.7, 44.5), (0.0, 0.0, 160.0, 120.0), (500.0, 500.0, 600.0, 560.0)])
def test_crop_taps_match_float64_bilinear_within_one_code(box):
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (2, 120, 160, 3), dtype=np.uint8)
    got = fo.crop_u8(frames, [(1, *box)])[0].astype(np.float64)
    want = np.round(fo.crop_float64(frames[1], box))
    assert np.abs(got - want).max() <= 1, np.abs(got - want).max()


def test_crop_rule_square_centred_on_the_box():
    x0, wx1, y0, wy1 = faces.crop_taps((10.0, 20.0, 38.0, 76.0), 200, 200)  # w 28, h 56 -> side 56, centre (24, 48)
    src = 24 - 28 + (np.arange(112) + 0.5) * 0.5 - 0.5
    assert np.array_equal(x0, np.clip(np.floor(src).astype(np.int64), -2, 200))  # left of -2: both taps outside
    assert np.array_equal(wx1, np.floor((src - np.floor(src)) * 2048 + 0.5).astype(np.int64))
    x0, _, _, _ = faces.crop_taps((1e5, 0.0, 1e5 + 10, 10.0), 50, 50)
    assert x0.min() == 50  # clamped: both taps stay outside the frame


def _sk_labels(e, eps, ms):
    sk = pytest.importorskip("sklearn.cluster")
    return sk.DBSCAN(eps=eps, min_samples=ms, metric="cosine").fit(e).labels_


def test_numpy_dbscan_equals_sklearn_on_the_golden_cases():
    g = np.load(fo_golden())
    names = sorted({k.split("__")[0] for k in g.files})
    assert len(names) >= 6
    for name in names:
        e, eps, ms, labels = (g[f"{name}__{f}"] for f in ("emb", "eps", "min_samples", "labels"))
        assert np.array_equal(fo.dbscan(e, float(eps), int(ms)), labels), name
        assert np.array_equal(_sk_labels(e, float(eps), int(ms)), labels), name


@pytest.mark.parametrize("seed,ms,noise", [(1, 1, 0), (2, 3, 20), (3, 5, 60), (4, 10, 5)])
def test_numpy_dbscan_equals_sklearn_on_generated_sets(seed, ms, noise):
    e = fo.clustered_set(seed, 400, 64, 8, 0.12, noise)
    assert np.array_equal(fo.dbscan(e, 0.3, ms), _sk_labels(e, 0.3, ms))


def test_shared_border_point_takes_the_smallest_label():
    g = np.load(fo_golden())
    lab = g["shared_border__labels"]
    assert lab[0] == 0 and set(lab[1:]) == {0, 1}  # index 0 is the border point between the two clusters


def fo_golden():
    from pathlib import Path

    return Path(__file__).resolve().parent / "golden" / "face_dbscan.npz"


def test_cluster_ids_format():
    assert faces.cluster_ids([0, -1, 11, 2]) == ["face_cluster_001", None, "face_cluster_012", "face_cluster_003"]


# ---- ModelManager wiring with fakes ------------------------------------------------------------------------------------
DET = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("conf", "<f4"), ("cls", "<i4"),
                ("pad", "V8")])


class _Src:
    def __init__(self, frames, fps=1.0):
        self.frames, self.fps, self.total_frames, self.pos = frames, fps, len(frames), 0

    def read(self):
        if self.pos >= len(self.frames):
            return False, None
        self.pos += 1
        return True, self.frames[self.pos - 1]

    def grab(self):
        if self.pos >= len(self.frames):
            return False
        self.pos += 1
        return True

    def release(self):
        pass


class _Detector:
    """Two faces per frame: one above the threshold, one below; boxes vary with the frame's first pixel."""
    names = {0: "face"}

    def detect(self, frames, conf=0.25):
        out = np.zeros((len(frames), 3), DET)
        counts = np.zeros(len(frames), np.int32)
        for i, f in enumerate(frames):
            k = float(f[0, 0, 0])
            out[i][0] = (k, 2.0, k + 10.0, 14.0, 0.9, 0, b"")
            out[i][1] = (1.0, 1.0, 5.0, 5.0, 0.5, 0, b"")
            counts[i] = 2
        return out, counts


class _Embedder:
    def __init__(self, log):
        self.log = log

    def embed(self, frames, boxes):
        self.log.append(("embed", np.asarray(boxes).copy(), int(len(frames))))
        return np.stack([np.eye(32, dtype=np.float32)[int(frames[int(b[0])][0, 0, 0]) % 3] for b in boxes])

    def cluster(self, emb, eps, min_samples):
        self.log.append(("cluster", emb.shape, eps, min_samples))
        return fo.dbscan(emb, eps, min_samples)


def _manager(tmp_path, frames, log, batch_size=2):
    from eioku_amd.model_manager import ModelManager

    return ModelManager(cache_dir=str(tmp_path), frame_source=lambda p: _Src(frames), detector_factory=lambda m, c: _Detector(),
                        batch_size=batch_size, face_embedder_factory=lambda c, m: (log.append(("factory", m)), _Embedder(log))[1])


def _frames():
    vals = [0, 1, 3, 0, 2, 6, 4, 1]  # identities val % 3: 0, 1, 0, 0, 2, 0, 1, 1
    f = np.zeros((len(vals), 16, 40, 3), np.uint8)
    for i, v in enumerate(vals):
        f[i, 0, 0, 0] = v
    return f


def test_detect_faces_without_cluster_faces_is_unchanged_and_loads_no_embedder(tmp_path):
    log = []
    out = asyncio.run(_manager(tmp_path, _frames(), log).detect_faces("/v.mp4", {"frame_interval": 1}))
    dets = out["detections"]
    assert len(dets) == 8 and all(d["cluster_id"] is None for d in dets) and not log
    assert [d["frame_index"] for d in dets] == list(range(8))
    assert set(dets[0]) == {"frame_index", "timestamp_ms", "label", "confidence", "bbox", "cluster_id"}


def test_detect_faces_with_cluster_faces_assigns_ids_in_detection_order(tmp_path):
    log = []
    frames = _frames()
    cfg = {"frame_interval": 1, "cluster_faces": True, "cluster_eps": 0.2, "cluster_min_samples": 3,
           "face_embedding_model": "arcface_r50.pth"}
    out = asyncio.run(_manager(tmp_path, frames, log).detect_faces("/v.mp4", cfg))
    dets = out["detections"]
    plain = asyncio.run(_manager(tmp_path, frames, []).detect_faces("/v.mp4", {"frame_interval": 1}))["detections"]
    assert [{k: v for k, v in d.items() if k != "cluster_id"} for d in dets] == \
           [{k: v for k, v in d.items() if k != "cluster_id"} for d in plain]
    # identities 0 (4 faces) and 1 (3 faces) are clusters, identity 2 (one face) is noise; ids by first core index
    assert [d["cluster_id"] for d in dets] == ["face_cluster_001", "face_cluster_002", "face_cluster_001", "face_cluster_001",
                                               None, "face_cluster_001", "face_cluster_002", "face_cluster_002"]
    assert log[0] == ("factory", "arcface_r50.pth")
    embeds = [e for e in log if e[0] == "embed"]
    assert len(embeds) == 4 and all(len(e[1]) == 2 for e in embeds)  # one call per batch of 2 frames, low-conf faces skipped
    assert np.array_equal(embeds[0][1], np.array([[0, 0, 2, 10, 14], [1, 1, 2, 11, 14]], np.float32))
    assert [e for e in log if e[0] == "cluster"] == [("cluster", (8, 32), 0.2, 3)]


def test_cluster_defaults_are_the_documented_ones(tmp_path):
    from eioku_amd.model_manager import ModelManager

    log = []
    asyncio.run(_manager(tmp_path, _frames(), log).detect_faces("/v.mp4", {"frame_interval": 1, "cluster_faces": True}))
    assert log[0] == ("factory", "arcface_r18.pth")
    assert [e for e in log if e[0] == "cluster"] == [("cluster", (8, 32), ModelManager.CLUSTER_EPS, ModelManager.CLUSTER_MIN_SAMPLES)]


def test_missing_checkpoint_is_an_error_without_a_seed(tmp_path):
    with pytest.raises(FileNotFoundError):
        faces.FaceEmbedder.from_cache(tmp_path, "arcface_r18.pth")


def test_process_ml_task_carries_cluster_id_into_the_face_clusters_projection(tmp_path):
    """ml task -> ModelManager.detect_faces(cluster_faces) -> envelope payload -> emit.py's face_clusters row."""
    import json
    import sqlite3

    from eioku_amd import emit, task_handler

    conn = sqlite3.connect(":memory:")
    conn.execute("CREATE TABLE face_clusters (artifact_id TEXT PRIMARY KEY, asset_id TEXT, cluster_id TEXT, confidence REAL, "
                 "start_ms INTEGER, end_ms INTEGER)")
    conn.execute("CREATE TABLE artifacts (" + ", ".join(emit.ARTIFACT_COLUMNS) + ")")
    w = emit.ArtifactBatchWriter(conn)
    sent = []
    out = asyncio.run(task_handler.process_ml_task(
        {"artifact_sink": lambda env: (sent.extend(env), w.write(env)),
         "model_manager_factory": lambda cache_dir: _manager(tmp_path, _frames(), [])},
        "t1", "face_detection", "vid", "/v.mp4", {"frame_interval": 1, "cluster_faces": True, "cluster_eps": 0.2}))
    assert out["status"] == "completed" and out["artifact_count"] == 8
    ids = [json.loads(e.payload_json)["cluster_id"] for e in sent]
    assert ids[:2] == ["face_cluster_001", "face_cluster_002"] and ids[4] is None
    rows = conn.execute("SELECT artifact_id, cluster_id, start_ms FROM face_clusters").fetchall()
    assert sorted((a, c) for a, c, _ in rows) == sorted((e.artifact_id, i) for e, i in zip(sent, ids))
