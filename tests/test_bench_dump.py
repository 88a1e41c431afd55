"""bench.py --dump-outputs: the last timed step's results as float32 / float64 .npy files, detection rows past a frame's
count zeroed, integer results exact.  CPU tensors stand in for the device ones (dump_outputs only copies them to the host)."""
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
from eioku_amd import detect  # noqa: E402


def _dets(n, max_det, counts, rng):
    d = np.zeros((n, max_det), detect.DET_DTYPE)
    for f in ("x1", "y1", "x2", "y2", "conf"):
        d[f] = rng.standard_normal((n, max_det)).astype(np.float32)
    d["cls"] = rng.integers(0, 80, (n, max_det))
    d["anchor"] = rng.integers(0, 8400, (n, max_det))
    d["pad"] = -1
    raw = torch.from_numpy(d.view(np.uint8).reshape(n, max_det, 32).copy())
    return d, raw, torch.tensor(counts, dtype=torch.int32)


def test_dump_outputs_writes_the_last_steps_arrays(tmp_path):
    rng = np.random.default_rng(3)
    d, raw, counts = _dets(3, 5, [2, 0, 5], rng)
    hsv = np.array([[0, 1, 2], [2**40 + 7, 5, 6], [7, 8, 9]], np.uint64)
    sad = np.array([0, 2**33 + 1, 4], np.uint64)
    emb = [torch.randn(8, 384, generator=torch.Generator().manual_seed(1))]
    pipe = SimpleNamespace(last=[(raw, counts, None), torch.from_numpy(hsv.view(np.int64)), torch.from_numpy(sad.view(np.int64))],
                           embedded=emb)
    bench.dump_outputs(pipe, tmp_path / "out")
    got = {p.stem: np.load(p) for p in (tmp_path / "out").glob("*.npy")}
    assert set(got) == {"det_boxes_xyxy", "det_conf", "det_cls", "det_anchor", "det_counts", "scene_hsv_sums",
                        "scene_luma_sad", "embeddings"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    valid = np.arange(5)[None, :] < np.array([2, 0, 5])[:, None]
    box = np.stack([d["x1"], d["y1"], d["x2"], d["y2"]], -1)
    assert np.array_equal(got["det_boxes_xyxy"], np.where(valid[..., None], box, 0))
    assert np.array_equal(got["det_conf"], np.where(valid, d["conf"], 0))
    assert np.array_equal(got["det_cls"], np.where(valid, d["cls"], 0).astype(np.float32))
    assert np.array_equal(got["det_anchor"], np.where(valid, d["anchor"], 0).astype(np.float32))
    assert np.array_equal(got["det_counts"], [2, 0, 5])
    assert got["scene_hsv_sums"].dtype == np.float64 and np.array_equal(got["scene_hsv_sums"].astype(np.uint64), hsv)
    assert np.array_equal(got["scene_luma_sad"].astype(np.uint64), sad)
    assert np.array_equal(got["embeddings"], emb[0].numpy())


def test_steps_must_be_positive():
    assert bench.parse_args(["--steps", "3", "--dump-outputs", "d"]).dump_outputs == "d"
    try:
        bench.parse_args(["--steps", "0"])
    except SystemExit as e:
        assert e.code == 2
    else:
        raise AssertionError("--steps 0 accepted")
