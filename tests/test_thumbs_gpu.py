"""GPU parity of K18 (csrc/thumbs.hip) against tests/jpeg_oracle.py and Pillow's committed bytes: byte identity at every
stage (resize, coefficients, bitstream, file) and through ``ModelManager.generate_thumbnails``.  No tolerance anywhere:
every stage is integer arithmetic."""
import asyncio
import functools
import json

import numpy as np
import pytest

import jpeg_oracle as jo
import thumbs_cases as tc
from conftest import GOLDEN
from eioku_amd import _lib, thumbs

pytestmark = pytest.mark.gpu

N_IMAGES = 3  # different images per call: per-image offsets, DC predictor resets and stream packing are exercised


@functools.lru_cache(maxsize=None)
def oracle(content, h, w, q, variant):
    return jo.encode(tc.image(content, h, w, variant), q)


@functools.lru_cache(maxsize=None)
def device(case):
    """One device run per case, shared by the stage tests: (streams, nbits, coef) of the three images."""
    content, h, w, q = case
    enc = thumbs.ThumbnailEncoder()
    try:
        return enc.jpeg(np.stack([tc.image(content, h, w, v) for v in range(N_IMAGES)]), quality=q, with_coef=True)
    finally:
        enc.close()


@pytest.fixture(scope="module")
def enc(gpu):
    e = thumbs.ThumbnailEncoder()
    yield e
    e.close()


@pytest.mark.parametrize("case", tc.JPEG_CASES, ids=tc.case_id)
def test_block_stage_coefficients_are_libjpegs(gpu, case):
    content, h, w, q = case
    _, _, coef = device(case)
    assert coef.shape == (N_IMAGES, -(-h // 16) * -(-w // 16), 6, 64) and coef.dtype == np.int16
    for v in range(N_IMAGES):
        want = oracle(content, h, w, q, v)["coef"]
        bad = np.argwhere(coef[v] != want)
        assert not len(bad), f"image {v}: first differing (mcu, block, k) = {bad[0]}, {len(bad)} in all"


@pytest.mark.parametrize("case", tc.JPEG_CASES, ids=tc.case_id)
def test_entropy_stage_bitstream_and_file_are_libjpegs(gpu, case):
    content, h, w, q = case
    streams, nbits, _ = device(case)
    for v in range(N_IMAGES):
        want = oracle(content, h, w, q, v)
        assert nbits[v] == want["nbits"]
        assert streams[v] == want["stream"]
        assert thumbs.jpeg_file(streams[v], nbits[v], w, h, q) == want["file"]


def test_files_are_pillows_committed_bytes(gpu, enc):
    gold = np.load(GOLDEN / "thumbs_pillow.npz")
    for i, (content, h, w, q) in enumerate(tc.GOLDEN_JPEG):
        rgb = gold[f"jpeg{i}_rgb"]
        assert np.array_equal(rgb, tc.image(content, h, w))
        streams, nbits = enc.jpeg(rgb[None], quality=q)
        assert thumbs.jpeg_file(streams[0], nbits[0], w, h, q) == gold[f"jpeg{i}_file"].tobytes(), tc.case_id((content, h, w, q))
    for i, ((h, w), (th, tw)) in enumerate(tc.GOLDEN_RESIZE):
        bgr = np.ascontiguousarray(gold[f"resize{i}_rgb"][None, ..., ::-1])
        assert np.array_equal(enc.resize(bgr, (tw, th)).cpu().numpy()[0], gold[f"resize{i}_out"])


@pytest.mark.parametrize("src,dst", tc.RESIZE_CASES + [((1080, 1920), (180, 320))])
def test_resize_is_pillows_bicubic(gpu, enc, src, dst):
    import torch

    n = 1 if src[0] > 1000 else 2
    rgb = np.stack([tc.image("random", *src, variant=7 + v) for v in range(n)])
    if src[0] > 1000:  # a frame-like image: blobs and noise rather than white noise
        rgb = (np.repeat(np.repeat(rgb[:, ::8, ::8], 8, 1), 8, 2) // 2 + rgb // 2).astype(np.uint8)
    bgr = np.ascontiguousarray(rgb[..., ::-1])
    want = np.stack([jo.resize_bicubic(f, (dst[1], dst[0])) for f in rgb])
    for frames in (bgr, torch.from_numpy(bgr).to(gpu)):
        got = enc.resize(frames, (dst[1], dst[0]))
        assert got.is_cuda and tuple(got.shape) == (n, dst[0], dst[1], 3)
        assert np.array_equal(got.cpu().numpy(), want)


def test_encode_splits_long_batches(gpu):
    e = thumbs.ThumbnailEncoder(size=(16, 16), quality=90)
    try:
        frames = np.stack([tc.image("random", 16, 16, v) for v in range(thumbs.MAX_BATCH + 1)])
        files = e.encode(np.ascontiguousarray(frames[..., ::-1]))
        assert len(files) == thumbs.MAX_BATCH + 1
        for v in (0, 1, thumbs.MAX_BATCH - 1, thumbs.MAX_BATCH):  # a frame that fits its box is not resampled
            assert files[v] == jo.encode(frames[v], 90)["file"]
    finally:
        e.close()


def test_refusals_leave_the_handle_usable(gpu, enc):
    small = np.zeros((1, 8, 8, 3), np.uint8)
    with pytest.raises(_lib.EiokuHipError, match="1024"):
        enc.resize(small, (thumbs.MAX_SIDE + 1, 8))
    with pytest.raises(_lib.EiokuHipError, match="1024"):
        enc.resize(small, (8, thumbs.MAX_SIDE + 1))
    with pytest.raises(_lib.EiokuHipError, match="at most 64"):
        enc.resize(np.zeros((thumbs.MAX_BATCH + 1, 8, 8, 3), np.uint8), (4, 4))
    with pytest.raises(_lib.EiokuHipError, match="1024"):
        enc.jpeg(np.zeros((1, 8, thumbs.MAX_SIDE + 1, 3), np.uint8))
    with pytest.raises(_lib.EiokuHipError, match="at most 64"):
        enc.jpeg(np.zeros((thumbs.MAX_BATCH + 1, 8, 8, 3), np.uint8))
    rgb = tc.image("random", 31, 47)
    streams, nbits = enc.jpeg(rgb[None], quality=30)
    assert thumbs.jpeg_file(streams[0], nbits[0], 47, 31, 30) == oracle("random", 31, 47, 30, 0)["file"]
    assert np.array_equal(enc.resize(np.ascontiguousarray(rgb[None, ..., ::-1]), (23, 16)).cpu().numpy()[0],
                          jo.resize_bicubic(rgb, (23, 16)))
    # the largest thumbnail the library takes: 1024 x 1024 of a tiled 64 x 64 pattern, whose MCUs repeat the tile's
    big = np.tile(tc.image("random", 64, 64), (16, 16, 1))
    streams, nbits, coef = enc.jpeg(big[None], quality=75, with_coef=True)
    tile = oracle("random", 64, 64, 75, 0)["coef"].reshape(4, 4, 6, 64)
    assert np.array_equal(coef[0].reshape(64, 64, 6, 64), np.tile(tile, (16, 16, 1, 1)))
    assert nbits[0] > 0 and len(streams[0]) == (nbits[0] + 7) // 8


# ---- end to end ----------------------------------------------------------------------------------------------------
FPS = 30.0
CUT_FRAMES = (10, 20, 30)


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """40 frames of 96 x 128: four flat colours plus noise, hard cuts at frames 10, 20 and 30."""
    rng = np.random.default_rng(5)
    colours = [(20, 30, 25), (150, 140, 160), (250, 235, 240), (60, 70, 50)]
    frames = np.empty((40, 96, 128, 3), np.uint8)
    for i in range(40):
        frames[i] = np.clip(np.array(colours[i // 10])[None, None] + rng.integers(-12, 13, (96, 128, 3)), 0, 255)
    path = tmp_path_factory.mktemp("thumbs") / "clip.npy"
    np.save(path, frames)
    return str(path), frames


def quirk_scenes():
    """The reference's scene list for the three cuts: no scene before the first cut, last index = number of cuts."""
    ms = [int((f / FPS) * 1000) for f in CUT_FRAMES]
    return [{"scene_index": 0, "start_ms": ms[0], "end_ms": ms[1], "duration_ms": ms[1] - ms[0]},
            {"scene_index": 1, "start_ms": ms[1], "end_ms": ms[2], "duration_ms": ms[2] - ms[1]},
            {"scene_index": 3, "start_ms": ms[2], "end_ms": 1333, "duration_ms": 1333 - ms[2]}]


@pytest.mark.parametrize("position", ["start", "middle"])
def test_generate_thumbnails_end_to_end(gpu, clip, tmp_path, position):
    from eioku_amd.model_manager import ModelManager

    path, frames = clip
    scenes = quirk_scenes()
    out_dir = tmp_path / "out"
    mm = ModelManager(cache_dir=str(tmp_path / "models"), batch_size=2)  # three wanted frames: a full batch and a rest
    result = asyncio.run(mm.generate_thumbnails(path, {"scenes": scenes, "size": (64, 48), "position": position,
                                                       "output_dir": str(out_dir)}))
    rows = result["thumbnails"]
    assert [r["scene_index"] for r in rows] == [0, 1, 3]
    json.dumps(result)
    stamp = [int((i / FPS) * 1000) for i in range(40)]
    for r, sc in zip(rows, scenes):
        target = sc["start_ms"] if position == "start" else (sc["start_ms"] + sc["end_ms"]) // 2
        idx = next(i for i, t in enumerate(stamp) if t >= target)
        want = jo.encode(jo.resize_bicubic(frames[idx][..., ::-1], (64, 48)), 75)["file"]
        file = out_dir / f"scene_{sc['scene_index']:04d}.jpg"
        assert file.read_bytes() == want
        assert r == {"scene_index": sc["scene_index"], "start_ms": sc["start_ms"], "end_ms": sc["end_ms"], "timestamp_ms": stamp[idx],
                     "frame_index": idx, "width": 64, "height": 48, "thumbnail_path": str(file), "bytes": len(want)}
    assert [r["frame_index"] for r in rows] == ([10, 20, 30] if position == "start" else [15, 25, 35])
    assert sorted(p.name for p in out_dir.iterdir()) == ["scene_0000.jpg", "scene_0001.jpg", "scene_0003.jpg"]


def test_generate_thumbnails_detects_scenes_itself(gpu, clip, tmp_path):
    from eioku_amd.model_manager import ModelManager

    path, frames = clip
    mm = ModelManager(cache_dir=str(tmp_path / "models"))
    scfg = {"threshold": 0.3}
    scenes = asyncio.run(mm.detect_scenes(path, scfg))["scenes"]
    assert len(scenes) == 3  # the three cuts, in the reference's numbering
    rows = asyncio.run(mm.generate_thumbnails(path, {"scene_detection": scfg, "size": (64, 48), "quality": 60,
                                                     "output_dir": str(tmp_path / "auto")}))["thumbnails"]
    assert [(r["scene_index"], r["start_ms"], r["end_ms"]) for r in rows] == [(s["scene_index"], s["start_ms"], s["end_ms"]) for s in scenes]
    for r in rows:
        want = jo.encode(jo.resize_bicubic(frames[r["frame_index"]][..., ::-1], (64, 48)), 60)["file"]
        assert (tmp_path / "auto" / f"scene_{r['scene_index']:04d}.jpg").read_bytes() == want and r["bytes"] == len(want)
