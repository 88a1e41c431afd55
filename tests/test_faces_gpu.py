"""GPU parity of K13 (face crop + ArcFace IResNet, csrc/faces.hip) and K14 (cosine DBSCAN) against tests/face_oracle.py,
scikit-learn's labels (tests/golden/face_dbscan.npz) and the ModelManager face path end to end."""
import asyncio
import json

import numpy as np
import pytest

import block_stats
import face_oracle as fo
from conftest import GOLDEN
from eioku_amd import _lib, faces
from eioku_amd._buffers import ptr

pytestmark = pytest.mark.gpu

FP32_MEAN, FP32_MAX = 1e-2, 5e-2   # of the activations' RMS: K11's fp16-network bound against the fp32 network
COS_FLOOR = 0.99                   # cosine between device and torch-fp32 r18 embeddings, every face


@pytest.fixture(scope="module")
def r18(gpu):
    sd = faces.random_state_dict(11)
    emb = faces.FaceEmbedder(faces.fold_state(sd))
    yield sd, emb
    emb.close()


def _frames(seed, n, h, w):
    rng = np.random.default_rng(seed)
    blobs = rng.integers(0, 256, (n, h // 6 + 1, w // 6 + 1, 3))
    f = np.repeat(np.repeat(blobs, 6, 1), 6, 2)[:, :h, :w] + rng.integers(-25, 26, (n, h, w, 3))
    return np.clip(f, 0, 255).astype(np.uint8)


BOXES = [(0, 10.0, 20.0, 60.0, 90.0), (1, -30.0, -10.0, 40.0, 50.0), (2, 150.0, 100.0, 400.0, 300.0),
         (0, 33.3, 44.4, 33.7, 44.5), (1, 0.0, 0.0, 160.0, 120.0), (2, 500.0, 500.0, 600.0, 560.0),
         (0, 159.5, 119.5, 161.0, 121.0), (2, 12.25, 7.75, 97.5, 31.125)]


def test_crop_is_the_numpy_restatement_bit_for_bit(gpu, r18):
    """Boxes inside, partly and wholly outside the frame, under a pixel, frame-sized; host and device frames."""
    import torch

    _, emb = r18
    frames = _frames(1, 3, 120, 160)
    want = fo.crop_input(frames, BOXES)
    for src in (frames, torch.from_numpy(frames).to(gpu)):
        got = emb.crop(src, BOXES).cpu().numpy()
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    assert not want[5].any() or np.all(want[5][..., :3] == np.float16(-1.0))  # wholly outside: zeros -> -1


def _torch_net(sd):
    return fo.iresnet(sd)


@pytest.mark.parametrize("upto", [0, 1, 2, 7])
def test_ibasicblock_matches_torch_fp32(gpu, r18, upto):
    """Stem + layer1.0 (downsample branch), + layer1.1 (identity shortcut), through layer2.0 (index depths[0]: the first block
    that halves a map the stem did not produce) and through the last block, on the device against torch-CPU fp32.  Besides the
    whole tensor: every channel against its own RMS and the border against the interior, each at most 2 x what the oracle's
    fp16 twin shows at the same point (tests/block_stats.py)."""
    import torch

    sd, emb = r18
    assert emb.depths[0] == 2 and sum(emb.depths) - 1 == 7
    frames = _frames(2, 3, 120, 160)
    crops = fo.crop_input(frames, BOXES[:6])
    got = emb.forward_raw(torch.from_numpy(crops).to(gpu), upto_block=upto).cpu().numpy().astype(np.float64)
    want = fo.forward_blocks(sd, crops, upto)  # torch-CPU fp32: net.stem, then the blocks in order
    rms = float(np.sqrt((want ** 2).mean()))
    err = np.abs(got - want)
    print(f"iresnet block {upto}: rms {rms:.3f} mean {err.mean() / rms:.2e} max {err.max() / rms:.2e}")
    assert rms > 0.1 and err.mean() <= FP32_MEAN * rms and err.max() <= FP32_MAX * rms, (err.mean() / rms, err.max() / rms)
    block_stats.check(f"iresnet block {upto}", got, fo.forward_blocks(sd, crops, upto, fp16=True), want)


def test_r18_embeddings_match_torch_fp32(gpu, r18):
    import torch

    sd, emb = r18
    frames = _frames(3, 3, 120, 160)
    crops = fo.crop_input(frames, BOXES)
    want = fo.embed_fp32(_torch_net(sd), crops)
    got = emb.embed(frames, BOXES)
    assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)
    cos = (got.astype(np.float64) * want).sum(1)
    print("r18 cosine device vs torch fp32: min", cos.min())
    assert cos.min() >= COS_FLOOR, cos
    # the raw network on the numpy crops gives the same vectors as embed() on the frames (the crop is bit-exact)
    raw = emb.forward_raw(torch.from_numpy(crops).to(gpu)).cpu().numpy()
    assert np.array_equal(raw, got)
    # more faces than one pass (256) and device frames: the same vectors
    big = [BOXES[i % len(BOXES)] for i in range(300)]
    got_big = emb.embed(torch.from_numpy(frames).to(gpu), big)
    assert np.array_equal(got_big[:len(BOXES)], got) and np.array_equal(got_big[256:256 + len(BOXES)], got[[i % 8 for i in range(256, 264)]])
    assert emb.last_flops() == pytest.approx(300 * 5.2e9, rel=0.05)


def _labels(e, eps, ms):
    return faces.dbscan_cosine(e, eps, ms)


def test_dbscan_equals_the_golden_sklearn_labels(gpu):
    g = np.load(GOLDEN / "face_dbscan.npz")
    names = sorted({k.split("__")[0] for k in g.files})
    for name in names:
        e, eps, ms, labels = (g[f"{name}__{f}"] for f in ("emb", "eps", "min_samples", "labels"))
        assert np.array_equal(_labels(e, float(eps), int(ms)), labels), name


def _oracle_labels_with_margin(e, eps, ms, gpu):
    """Numpy DBSCAN on neighbour lists from torch (rocBLAS fp32) distance chunks; asserts every distance is >= 1e-4
    away from eps (so float rounding cannot decide a neighbour)."""
    import torch

    n = len(e)
    et = torch.from_numpy(e).to(gpu)
    nbrs = []
    for lo in range(0, n, 2048):
        d = 1.0 - et[lo:lo + 2048] @ et.T
        idx = torch.arange(lo, min(lo + 2048, n), device=gpu)
        d[idx - lo, idx] = 0.0
        assert float((d - eps).abs().min()) >= 1e-4
        r, c = torch.nonzero(d <= eps, as_tuple=True)
        r, c = r.cpu().numpy() + lo, c.cpu().numpy()
        split = np.searchsorted(r, np.arange(lo, min(lo + 2048, n) + 1))
        nbrs += [c[split[i]:split[i + 1]] for i in range(len(split) - 1)]
    core = np.array([len(x) >= ms for x in nbrs])
    labels = np.full(n, -1, np.int32)
    nxt = 0
    for i in range(n):
        if not core[i] or labels[i] >= 0:
            continue
        labels[i] = nxt
        stack = [i]
        while stack:
            p = stack.pop()
            for q in nbrs[p][core[nbrs[p]]]:
                if labels[q] < 0:
                    labels[q] = nxt
                    stack.append(q)
        nxt += 1
    for i in np.nonzero(~core)[0]:
        lab = labels[nbrs[i][core[nbrs[i]]]]
        labels[i] = lab.min() if len(lab) else -1
    return labels


@pytest.mark.parametrize("n,k,ms", [(1, 1, 1), (1, 1, 2), (31, 3, 3), (1000, 20, 4), (65536, 2000, 5)])
def test_dbscan_equals_the_oracle_on_generated_sets(gpu, n, k, ms):
    e = fo.clustered_set(n + k, n, 512, k, 0.1, noise=n // 20)
    eps = 0.3
    want = _oracle_labels_with_margin(e, eps, ms, gpu)
    got = _labels(e, eps, ms)
    assert np.array_equal(got, want)
    if n == 1000:
        import torch

        again = _labels(torch.from_numpy(e).to(gpu), eps, ms).cpu().numpy()  # device input, repeated call: identical
        assert np.array_equal(again, got)
        assert len(set(got.tolist()) - {-1}) >= 10


def test_dbscan_border_ties_take_the_smallest_label(gpu):
    """Border points that reach cores of two and three clusters, at every position in the index order."""
    angles = [0.0, 0.01, 0.02, 0.5, 0.51, 0.52, 1.0, 1.01, 1.02, 0.26, 0.76]
    rng = np.random.default_rng(4)
    q, _ = np.linalg.qr(rng.standard_normal((64, 2)))
    base = (np.cos(angles)[:, None] * q[:, 0] + np.sin(angles)[:, None] * q[:, 1]).astype(np.float32)
    eps = float(np.float32(1 - np.cos(0.245)))
    for s in range(5):
        e = base[np.random.default_rng(s).permutation(len(base))]
        want = fo.dbscan(e, eps, 4)
        assert np.array_equal(_labels(e, eps, 4), want)
        assert (want >= 0).all()


def test_dbscan_invalid_arguments(gpu, built_lib):
    e = np.zeros((4, 48), np.float32)
    lab = np.zeros(65537, np.int32)
    big = np.zeros((1, 32), np.float32)
    assert built_lib.eioku_dbscan_cosine(ptr(e), 4, 48, 0.3, 2, ptr(lab), _lib.MEM_HOST, None) == -1
    assert built_lib.eioku_dbscan_cosine(ptr(big), 65537, 32, 0.3, 2, ptr(lab), _lib.MEM_HOST, None) == -1
    for eps in (-0.1, 2.5, float("nan")):
        assert built_lib.eioku_dbscan_cosine(ptr(big), 1, 32, eps, 2, ptr(lab), _lib.MEM_HOST, None) == -1
    assert built_lib.eioku_dbscan_cosine(ptr(big), 1, 32, 0.3, 0, ptr(lab), _lib.MEM_HOST, None) == -1
    assert len(faces.dbscan_cosine(np.zeros((0, 32), np.float32), 0.3, 2)) == 0


# ---- end to end ------------------------------------------------------------------------------------------------------
DET = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("conf", "<f4"), ("cls", "<i4"), ("pad", "V8")])


def _identity_clip(k=3, n=8, h=180, w=320, seed=21):
    """k 'identities' (distinct 48 x 48 textures) pasted into every frame at shifting positions over a textured
    background; known boxes (x1, y1, x2, y2) per frame."""
    rng = np.random.default_rng(seed)
    tex = [np.clip(np.repeat(np.repeat(rng.integers(0, 256, (8, 8, 3)), 6, 0), 6, 1) + rng.integers(-10, 11, (48, 48, 3)), 0, 255)
           for _ in range(k)]
    frames = _frames(seed + 1, n, h, w)
    boxes = []
    for i in range(n):
        row = []
        for j in range(k):
            x = 10 + j * 100 + (i * 7) % 40
            y = 20 + (i * 13 + j * 29) % 100
            frames[i, y:y + 48, x:x + 48] = tex[j]
            row.append((j, float(x), float(y), float(x + 48), float(y + 48)))
        boxes.append(row)
    return frames, boxes


class _KnownBoxes:
    names = {0: "face"}

    def __init__(self, frames, boxes):
        self.lookup = {f.tobytes(): b for f, b in zip(frames, boxes)}

    def detect(self, frames, conf=0.25):
        frames = frames.cpu().numpy() if hasattr(frames, "cpu") else frames
        out = np.zeros((len(frames), 8), DET)
        counts = np.zeros(len(frames), np.int32)
        for i, f in enumerate(frames):
            for t, (_, x1, y1, x2, y2) in enumerate(self.lookup[f.tobytes()]):
                out[i][t] = (x1, y1, x2, y2, 0.9, 0, b"")
            counts[i] = len(self.lookup[f.tobytes()])
        return out, counts


def test_detect_faces_clusters_identities_like_the_oracle_pipeline(gpu, tmp_path):
    """Known boxes around 3 textures that move from frame to frame (same scale: a random-init network does not promise
    scale invariance, so only the position varies).  eps is chosen from the oracle's measured distances and the margin
    max(intra) < eps < min(inter) is asserted; the device's cluster ids equal the oracle pipeline's (numpy crops ->
    torch fp32 embedder -> numpy DBSCAN)."""
    from eioku_amd.model_manager import ModelManager

    frames, boxes = _identity_clip()
    flat = [(i, *b[1:]) for i, row in enumerate(boxes) for b in row]
    ident = np.array([b[0] for row in boxes for b in row])
    sd = faces.random_state_dict(5)
    ref = fo.embed_fp32(fo.iresnet(sd), fo.crop_input(frames, flat))
    d = fo.cosine_distances(ref)
    same = ident[:, None] == ident[None, :]
    intra, inter = d[same].max(), d[~same].min()
    assert intra < inter, (intra, inter)
    eps = float((intra + inter) / 2)
    want_labels = fo.dbscan(ref, eps, 2)
    want = faces.cluster_ids(want_labels)
    assert len(set(want)) == 3 and None not in want

    class Src:
        def __init__(self):
            self.fps, self.total_frames, self.pos = 1.0, len(frames), 0

        def read(self):
            if self.pos >= len(frames):
                return False, None
            self.pos += 1
            return True, frames[self.pos - 1]

        def grab(self):
            self.pos += 1
            return self.pos <= len(frames)

        def release(self):
            pass

    mm = ModelManager(cache_dir=str(tmp_path), frame_source=lambda p: Src(), detector_factory=lambda m, c: _KnownBoxes(frames, boxes),
                      random_init_seed=5, batch_size=3)
    cfg = {"frame_interval": 1, "cluster_faces": True, "cluster_eps": eps, "cluster_min_samples": 2}
    out = asyncio.run(mm.detect_faces("/v.mp4", cfg))
    got = [d["cluster_id"] for d in out["detections"]]
    assert got == want
    plain = asyncio.run(mm.detect_faces("/v.mp4", {"frame_interval": 1}))
    assert [{k: v for k, v in d.items() if k != "cluster_id"} for d in out["detections"]] == \
           [{k: v for k, v in d.items() if k != "cluster_id"} for d in plain["detections"]]
    json.dumps(out)


def test_lane_path_embeds_the_detectors_device_batch(gpu, tmp_path):
    """Seeded random-init Yolov8Detector, calibrated so that its head answers on these frames (tests/wellcond.py; the
    PipelinedDetector device-batch accessor, not a fake): the embeddings of
    detect_faces(cluster_faces) are bit-identical to FaceEmbedder.embed on the same frames uploaded separately with the
    same boxes, hence the same ids; analyze_video returns the same dict; without cluster_faces the dict is today's."""
    import wellcond
    from oracle import prng
    from eioku_amd import detect as D, weights as W
    from eioku_amd.model_manager import ModelManager

    frames = prng.synth_frames_bgr(77, 40, 120, 160)
    p = tmp_path / "clip.npy"
    np.save(p, frames)
    (tmp_path / "clip.npy.json").write_text(json.dumps({"fps": 10.0}))
    calls = []

    class Recorder:
        def __init__(self, inner):
            self.inner = inner

        def embed(self, fr, boxes):
            out = self.inner.embed(fr, boxes)
            calls.append((fr.cpu().numpy() if hasattr(fr, "cpu") else np.asarray(fr), np.asarray(boxes, np.float32), out,
                          hasattr(fr, "is_cuda") and fr.is_cuda))
            return out

        def cluster(self, e, eps, ms):
            return self.inner.cluster(e, eps, ms)

        def close(self):
            self.inner.close()

    def factory(cache_dir, model_name):
        return Recorder(faces.FaceEmbedder.from_cache(cache_dir, model_name, seed=5))

    state = wellcond.calibrated_state(frames[:1], "n", 1, seed=8, frac=0.03, conf=0.3)

    def detector(model_name, cache_dir):
        return D.Yolov8Detector("n", 1, state, W.variant_from_model_name(model_name)[2])

    mm = ModelManager(cache_dir=str(tmp_path / "m"), detector_factory=detector, batch_size=8, face_embedder_factory=factory)
    base = {"frame_interval": 0.2, "confidence_threshold": 0.3}
    cfg = dict(base, cluster_faces=True, cluster_eps=0.2, cluster_min_samples=2)
    plain = asyncio.run(mm.detect_faces(str(p), base))
    out = asyncio.run(mm.detect_faces(str(p), cfg))
    n_faces = len(out["detections"])
    assert n_faces > 0 and calls and all(c[3] for c in calls)  # the crops read the lane's device copy
    assert sum(len(c[1]) for c in calls) == n_faces
    ref = faces.FaceEmbedder.from_cache(tmp_path / "m", "arcface_r18.pth", seed=5)
    emb = []
    for fr, bx, got, _ in calls:
        want = ref.embed(fr, bx)  # host frames: uploaded separately
        assert np.array_equal(got, want)
        emb.append(want)
    want_ids = faces.cluster_ids(ref.cluster(np.concatenate(emb), 0.2, 2))
    ref.close()
    assert [d["cluster_id"] for d in out["detections"]] == want_ids
    assert [{k: v for k, v in d.items() if k != "cluster_id"} for d in out["detections"]] == \
           [{k: v for k, v in d.items() if k != "cluster_id"} for d in plain["detections"]]
    assert all(d["cluster_id"] is None for d in plain["detections"])
    single = asyncio.run(mm.analyze_video(str(p), {"face_detection": cfg}))
    assert single == {"face_detection": out}
