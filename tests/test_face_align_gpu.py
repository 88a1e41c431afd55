"""Face alignment on the device: K13c bit for bit against ``align_oracle.warp_u8``, ``embed_aligned`` against the raw
network on the oracle's crops, a synthetic check that alignment does what it is for, and the public interface."""
import asyncio
import json

import numpy as np
import pytest

import align_oracle as ao
import face_oracle as fo
from eioku_amd import faces
from test_face_align_host import WARP_MATRICES
from test_faces_gpu import _frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def r18(gpu):
    sd = faces.random_state_dict(11)
    emb = faces.FaceEmbedder(faces.fold_state(sd))
    yield sd, emb
    emb.close()


def _landmarks_in_frame():
    """Five landmarks of a face about 60 px wide, tilted by 20 degrees, around (80, 60) of a 160 x 120 frame."""
    a = np.deg2rad(20.0)
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return (faces.ARCFACE_DST - 56.0) * 0.55 @ R.T + np.array([80.0, 60.0])


def _twelve():
    M, fallback = faces.align_matrices(_landmarks_in_frame()[None])
    assert not fallback[0]
    mats = [np.array(m, np.float64) for m in WARP_MATRICES.values()] + [M[0].reshape(6)]
    assert len(mats) == 12
    return np.stack(mats), np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2], np.int32)


def test_aligned_crop_is_the_numpy_restatement_bit_for_bit(gpu, r18):
    import torch

    _, emb = r18
    frames = _frames(1, 3, 120, 160)
    mats, slots = _twelve()
    want = ao.warp_input(frames, slots, mats)
    names = list(WARP_MATRICES) + ["align_matrices"]
    assert np.all(want[names.index("wholly outside")][..., :3] == np.float16(-1.0))
    assert len({want[i].tobytes() for i in range(12)}) == 12  # twelve different crops
    for src in (frames, torch.from_numpy(frames).to(gpu)):
        got = emb.crop_aligned(src, slots, mats.reshape(-1, 2, 3)).cpu().numpy()
        for i, name in enumerate(names):
            assert np.array_equal(got[i].view(np.uint16), want[i].view(np.uint16)), name
    # more faces than one network pass holds
    big = np.array([i % 12 for i in range(300)])
    got = emb.crop_aligned(torch.from_numpy(frames).to(gpu), slots[big], mats[big]).cpu().numpy()
    assert np.array_equal(got[:12].view(np.uint16), want.view(np.uint16))
    assert np.array_equal(got[256:268].view(np.uint16), want[big[256:268]].view(np.uint16))
    with pytest.raises(Exception, match="not finite"):
        emb.crop_aligned(frames, [0], np.full((1, 2, 3), np.nan))
    with pytest.raises(Exception, match="slot"):
        emb.crop_aligned(frames, [3], mats[:1])


def test_embed_aligned_is_the_network_on_the_oracles_crops(gpu, r18):
    import torch

    _, emb = r18
    frames = _frames(3, 3, 120, 160)
    rng = np.random.default_rng(4)
    lm = np.stack([_landmarks_in_frame() + rng.uniform(-6, 6, (5, 2)) + rng.uniform(-30, 30, 2) for _ in range(6)])
    lm[4] = np.array([70.0, 50.0])  # coincident landmarks: this face falls back to its box
    boxes = np.array([(i % 3, 40.0 + i, 20.0 + 2 * i, 120.0 - i, 100.0) for i in range(6)], np.float32)
    M, fallback = faces.align_matrices(lm)
    assert fallback.tolist() == [False] * 4 + [True, False]
    crops = ao.warp_input(frames, boxes[:, 0].astype(int), np.where(fallback[:, None, None], 0.0, M))
    crops[4] = fo.crop_input(frames, boxes[4:5])[0]
    want = emb.forward_raw(torch.from_numpy(crops).to(gpu)).cpu().numpy()
    for src in (frames, torch.from_numpy(frames).to(gpu)):
        got = emb.embed_aligned(src, boxes, lm)
        assert got.shape == (6, 512) and np.array_equal(got, want)
    assert np.array_equal(want[4], emb.embed(frames, boxes[4:5])[0])
    # landmarks with a confidence column, and more than one pass
    big = [i % 6 for i in range(300)]
    lm3 = np.concatenate([lm, np.ones((6, 5, 1))], axis=2)
    got = emb.embed_aligned(torch.from_numpy(frames).to(gpu), boxes[big], lm3[big])
    assert np.array_equal(got[:6], want) and np.array_equal(got[294:], want)
    assert emb.embed_aligned(frames, np.zeros((0, 5), np.float32), np.zeros((0, 5, 2))).shape == (0, 512)


# ---- alignment does its job --------------------------------------------------------------------------------------------
def _texture(seed):
    """An asymmetric 112 x 112 'identity' in template space: 7 x 7 colour blocks of 16 px, a brightness ramp, noise."""
    rng = np.random.default_rng(seed)
    t = np.repeat(np.repeat(rng.integers(0, 256, (7, 7, 3)), 16, 0), 16, 1).astype(np.float64)
    t = 0.75 * t + 0.25 * np.linspace(0, 255, 112)[None, :, None] + rng.integers(-8, 9, (112, 112, 3))
    return np.clip(t, 0, 255)


# template -> frame: (rotation in degrees, scale, offset of the template's origin)
TRANSFORMS = [(25.0, 1.6, (150.0, 40.0)), (-25.0, 0.6, (60.0, 130.0)), (10.0, 1.0, (120.0, 90.0)), (-17.0, 1.3, (40.0, 110.0)),
              (21.0, 0.8, (190.0, 60.0)), (-6.0, 1.45, (70.0, 75.0))]


def _paint(tex, deg, s, off, h=320, w=400, seed=0):
    """The texture under a similarity, bilinear, over a noisy background -> (frame BGR uint8, landmarks (5,2), box)."""
    a = np.deg2rad(deg)
    R = s * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    off = np.asarray(off, np.float64)
    frame = np.random.default_rng(seed).integers(90, 166, (h, w, 3)).astype(np.float64)
    yy, xx = np.mgrid[0:h, 0:w]
    p = np.stack([xx, yy], -1).astype(np.float64) - off
    q = p @ np.linalg.inv(R).T  # template coordinates of every frame pixel
    x0, y0 = np.floor(q[..., 0]).astype(int), np.floor(q[..., 1]).astype(int)
    fx, fy = (q[..., 0] - x0)[..., None], (q[..., 1] - y0)[..., None]
    inside = (x0 >= 0) & (x0 < 111) & (y0 >= 0) & (y0 < 111)
    xc, yc = np.clip(x0, 0, 110), np.clip(y0, 0, 110)
    v = (tex[yc, xc] * (1 - fx) * (1 - fy) + tex[yc, xc + 1] * fx * (1 - fy) + tex[yc + 1, xc] * (1 - fx) * fy + tex[yc + 1, xc + 1] * fx * fy)
    frame[inside] = v[inside]
    corners = np.array([[0, 0], [111, 0], [0, 111], [111, 111]], np.float64) @ R.T + off
    box = (*corners.min(0), *corners.max(0))
    return np.clip(np.rint(frame), 0, 255).astype(np.uint8), faces.ARCFACE_DST @ R.T + off, box


def _identity_set():
    frames, lms, boxes, ident = [], [], [], []
    for who, seed in enumerate((101, 202)):
        tex = _texture(seed)
        for k, (deg, s, off) in enumerate(TRANSFORMS):
            f, lm, box = _paint(tex, deg, s, off, seed=10 * who + k)
            frames.append(f)
            lms.append(lm)
            boxes.append((len(frames) - 1, *box))
            ident.append(who)
    return np.stack(frames), np.stack(lms), np.array(boxes, np.float32), np.array(ident)


def _gap(e, ident):
    cos = e.astype(np.float64) @ e.astype(np.float64).T
    same = ident[:, None] == ident[None, :]
    return float(cos[same].min() - cos[~same].max())


ORACLE_GAP = 0.05  # what the torch-fp32 oracle must show on these textures and transforms (it shows 0.382, see the test)


def test_aligned_embeddings_separate_identities(gpu, r18):
    """Two textures under six similarity transforms each, with their exact landmarks: aligned, every same-identity cosine
    exceeds every cross-identity one.  The torch-fp32 oracle on the oracle's aligned crops: minimum same-identity cosine
    0.982, maximum cross-identity cosine 0.600, gap 0.382.  On box crops of the same faces the oracle's gap is -0.055 (0.616
    against 0.671): unaligned, the two identities are not separable, which is what the alignment is for."""
    sd, emb = r18
    frames, lms, boxes, ident = _identity_set()
    M, fallback = faces.align_matrices(lms)
    assert not fallback.any()
    ref = fo.embed_fp32(fo.iresnet(sd), ao.warp_input(frames, boxes[:, 0].astype(int), M))
    assert _gap(ref, ident) >= ORACLE_GAP, _gap(ref, ident)
    got = emb.embed_aligned(frames, boxes, lms)
    box = emb.embed(frames, boxes)
    print(f"aligned gap: device {_gap(got, ident):.4f}, torch fp32 oracle {_gap(ref, ident):.4f}; box crops: device {_gap(box, ident):.4f}")
    assert _gap(got, ident) > 0


# ---- the public interface ---------------------------------------------------------------------------------------------
# Seeded, uncalibrated weights answer these frames with bimodal scores: about 190 of the 315 anchors per frame score ~1.0
# and the rest ~0 (the oracle network's figures), so any threshold in between selects the same anchors
E2E_CONF = 0.5


def test_detect_faces_end_to_end_with_a_seeded_pose_detector(gpu, tmp_path):
    from oracle import prng
    from eioku_amd.model_manager import ModelManager

    h, w = 120, 160
    frames = prng.synth_frames_bgr(77, 6, h, w)
    p = tmp_path / "clip.npy"
    np.save(p, frames)
    (tmp_path / "clip.npy.json").write_text(json.dumps({"fps": 10.0}))
    mm = ModelManager(cache_dir=str(tmp_path / "m"), random_init_seed=8, batch_size=4)
    base = {"frame_interval": 0.1, "confidence_threshold": E2E_CONF, "cluster_faces": True, "cluster_eps": 0.3, "cluster_min_samples": 1}
    pose = asyncio.run(mm.detect_faces(str(p), dict(base, keypoints=5)))["detections"]
    boxed = asyncio.run(mm.detect_faces(str(p), dict(base, keypoints=5, face_alignment=False)))["detections"]
    plain = asyncio.run(mm.detect_faces(str(p), base))["detections"]
    assert 0 < len(pose) == len(plain) == len(boxed)
    for d in pose:
        assert len(d["landmarks"]) == 5 and d["cluster_id"].startswith("face_cluster_")
        for pt in d["landmarks"]:
            assert set(pt) == {"x", "y", "confidence"} and all(type(v) is float for v in pt.values())
            assert 0 <= pt["x"] <= w and 0 <= pt["y"] <= h and 0 <= pt["confidence"] <= 1
    strip = lambda ds, *keys: [{k: v for k, v in d.items() if k not in keys} for d in ds]
    assert all("landmarks" not in d for d in plain)
    assert strip(pose, "landmarks", "cluster_id") == strip(plain, "cluster_id")  # the same boxes with and without the head
    assert strip(boxed, "landmarks") == plain                                    # box crops: the same labels too
    assert strip(boxed, "cluster_id") == strip(pose, "cluster_id")
    json.dumps(pose)
    both = asyncio.run(mm.analyze_video(str(p), {"face_detection": dict(base, keypoints=5)}))
    assert both["face_detection"]["detections"] == pose
    with pytest.raises(ValueError, match="5 keypoints"):
        asyncio.run(mm.detect_faces(str(p), dict(base, face_alignment=True)))
