"""GPU parity of K14h (csrc/hdbscan.hip: float64 core distances and the mutual-reachability MST by bounded Boruvka
rounds) against tests/hdbscan_oracle.py, and of eioku_amd.hdbscan.hdbscan_cosine against scikit-learn's labels and
probabilities (tests/golden/hdbscan.npz).

Bounds.  Rows are unit and d <= 512, so a float64 dot product is off by at most d * 2^-53 * sum|a_i b_i| <= 5.7e-14, plus a
few ulps of normalisation: core distances and edge weights are held to 1e-12 absolute (about 10x slack), an MST's total to
n * 1e-12.  The golden sets have no non-zero tree weight below 1e-4, so lambda = 1 / w is off by at most 1e-8 relative:
probabilities are held to 1e-7."""
import asyncio
import json

import numpy as np
import pytest

import hdbscan_oracle as ho
from conftest import GOLDEN
from eioku_amd import _lib, faces, hdbscan
from eioku_amd._buffers import ptr

pytestmark = pytest.mark.gpu

ABS = 1e-12
PROB = 1e-7

G = np.load(GOLDEN / "hdbscan.npz")
INDEX = json.loads(str(G["index"]))
CASES = sorted(INDEX)
_cache: dict = {}


def _emb(case):
    return G[f"{case}__emb"].astype(np.float32)


def _min_samples(kw):
    return kw.get("min_samples") or kw.get("min_cluster_size", 5)


def _case_ms(case):
    return sorted({_min_samples(kw) for kw in INDEX[case]["variants"].values()})


def _oracle(case, ms):
    """(dist, core, mutual reachability, oracle MST total): computed once per case and min_samples, never changed."""
    if (case, ms) not in _cache:
        d = ho.cosine_distances(_emb(case))
        core = ho.core_distances(d, ms)
        mr = ho.mutual_reachability(d, core)
        _cache[case, ms] = (d, core, mr, float(ho.boruvka(mr)[2].sum()))
    return _cache[case, ms]


def _device(case, ms):
    if ("dev", case, ms) not in _cache:
        _cache["dev", case, ms] = hdbscan.mst_cosine(_emb(case), ms)
    return _cache["dev", case, ms]


@pytest.mark.parametrize("case", CASES)
def test_core_distances_equal_the_oracle(gpu, case):
    for ms in _case_ms(case):
        core = _device(case, ms)[0]
        want = _oracle(case, ms)[1]
        err = float(np.abs(core - want).max())
        print(f"{case} min_samples {ms}: core max abs err {err:.3e}")
        assert core.dtype == np.float64 and err <= ABS


@pytest.mark.parametrize("case", CASES)
def test_mst_edges_span_and_weigh_what_the_oracle_says(gpu, case):
    for ms in _case_ms(case):
        _, u, v, w, rounds = _device(case, ms)
        n = len(_emb(case))
        _, _, mr, total = _oracle(case, ms)
        assert ho.spanning_and_acyclic(n, u, v)
        err = float(np.abs(w - mr[u, v]).max())
        print(f"{case} min_samples {ms}: edge weight max abs err {err:.3e}, total {w.sum():.15g} vs {total:.15g}, rounds {rounds}")
        assert err <= ABS
        assert abs(float(w.sum()) - total) <= n * ABS
        assert 1 <= rounds <= hdbscan.round_bound(n)


@pytest.mark.parametrize("case", CASES)
def test_labels_and_probabilities_equal_sklearns(gpu, case):
    emb = _emb(case)
    for name, kw in INDEX[case]["variants"].items():
        labels, prob = hdbscan.hdbscan_cosine(emb, **kw)
        want, want_p = G[f"{case}__{name}__labels"], G[f"{case}__{name}__prob"]
        assert labels.dtype == np.int32 and np.array_equal(labels, want), (case, name)
        if not INDEX[case]["labels_only"]:  # equal rows: sklearn's own lambda there is inf or 1e16 by accident of rounding
            err = float(np.abs(prob - want_p).max())
            print(f"{case}/{name}: probability max abs err {err:.3e}")
            assert err <= PROB, (case, name)


def test_identical_rows_end_within_the_round_bound(gpu):
    core, u, v, w, rounds = _device("identical", 5)
    assert rounds <= hdbscan.round_bound(40) and ho.spanning_and_acyclic(40, u, v)
    assert np.abs(core).max() <= ABS and np.abs(w).max() <= ABS
    # three groups of equal rows: every weight inside a group equal, every weight across groups equal
    emb = np.repeat(np.eye(32, dtype=np.float32)[:3], 50, axis=0)[np.random.default_rng(0).permutation(150)]
    core, u, v, w, rounds = hdbscan.mst_cosine(emb, 2)
    assert rounds <= hdbscan.round_bound(150) and ho.spanning_and_acyclic(150, u, v)
    assert sorted(np.round(w, 9).tolist()) == [0.0] * 147 + [1.0] * 2


def test_host_and_device_input_give_the_same_bits(gpu):
    import torch

    for case, ms in (("edge_129", 3), ("mixed_1000", 5)):
        emb = _emb(case)
        host = _device(case, ms)
        dev = hdbscan.mst_cosine(torch.from_numpy(emb).cuda(), ms)
        assert np.array_equal(host[0], dev[0]) and host[4] == dev[4]
        assert all(np.array_equal(a, b) for a, b in zip(hdbscan.sort_edges(*host[1:4]), hdbscan.sort_edges(*dev[1:4])))
    labels, prob = hdbscan.hdbscan_cosine(_emb("mixed_1000"))
    labels_d, prob_d = hdbscan.hdbscan_cosine(torch.from_numpy(_emb("mixed_1000")).cuda())
    assert isinstance(labels_d, np.ndarray) and np.array_equal(labels, labels_d) and np.array_equal(prob, prob_d)


def test_zero_one_and_two_rows(gpu):
    core, u, v, w, rounds = hdbscan.mst_cosine(np.zeros((0, 32), np.float32), 1)
    assert len(core) == 0 and len(u) == 0 and rounds == 0
    core, u, v, w, rounds = hdbscan.mst_cosine(np.ones((1, 32), np.float32), 1)
    assert core.tolist() == [0.0] and len(u) == len(v) == len(w) == 0 and rounds == 0
    emb = np.eye(2, 32, dtype=np.float32)
    core, u, v, w, rounds = hdbscan.mst_cosine(emb, 2)
    assert core.tolist() == [1.0, 1.0] and sorted((int(u[0]), int(v[0]))) == [0, 1] and w.tolist() == [1.0] and rounds == 1
    core, _, _, w, _ = hdbscan.mst_cosine(emb, 1)
    assert core.tolist() == [0.0, 0.0] and w.tolist() == [1.0]
    labels, prob = hdbscan.hdbscan_cosine(emb, min_cluster_size=2, min_samples=2)  # two faces: through the device, no error
    assert labels.tolist() == [-1, -1] and prob.tolist() == [0.0, 0.0]
    for n in (0, 1, 2):
        labels, prob = hdbscan.hdbscan_cosine(np.eye(n, 32, dtype=np.float32))
        assert labels.tolist() == [-1] * n and prob.tolist() == [0.0] * n


def test_invalid_arguments(gpu, built_lib):
    e = np.zeros((8, 64), np.float32)
    e[:, 0] = 1.0
    core, u, v, w, r = np.zeros(8), np.zeros(7, np.int32), np.zeros(7, np.int32), np.zeros(7), np.zeros(1, np.int32)

    def call(n, d, ms, mem=_lib.MEM_HOST):
        return built_lib.eioku_hdbscan_mst_cosine(ptr(e), n, d, ms, ptr(core), ptr(u), ptr(v), ptr(w), ptr(r), mem, None)

    assert call(8, 64, 2) == 0
    assert call(8, 48, 2) == -1 and b"multiple of 32" in built_lib.eioku_last_error()
    assert call(8, 0, 2) == -1
    assert call(-1, 64, 2) == -1 and call(65537, 64, 2) == -1
    assert call(8, 64, 0) == -1 and call(8, 64, 9) == -1 and call(8, 64, 33) == -1
    assert call(8, 64, 2, mem=7) == -1
    with pytest.raises(ValueError):
        hdbscan.hdbscan_cosine(np.zeros((8, 32, 1), np.float32))


def test_detect_faces_with_hdbscan_on_the_device(gpu, tmp_path):
    """The ModelManager face path with FaceEmbedder.cluster_hdbscan itself (fake detector and embeddings)."""
    import test_faces_host as tf
    from eioku_amd.model_manager import ModelManager

    class Embedder(tf._Embedder):
        cluster_hdbscan = faces.FaceEmbedder.cluster_hdbscan

    vals = [0, 1, 3, 0, 2, 6, 4, 1, 3, 4, 6, 7]
    frames = np.zeros((len(vals), 16, 40, 3), np.uint8)
    frames[:, 0, 0, 0] = vals
    mm = ModelManager(cache_dir=str(tmp_path), frame_source=lambda p: tf._Src(frames), detector_factory=lambda m, c: tf._Detector(),
                      batch_size=2, face_embedder_factory=lambda c, m: Embedder([]))
    cfg = {"frame_interval": 1, "cluster_faces": True, "face_cluster_method": "hdbscan", "cluster_min_size": 3}
    dets = asyncio.run(mm.detect_faces("/v.mp4", cfg))["detections"]
    want = [["face_cluster_001", "face_cluster_002", None][v % 3] for v in vals]
    assert [d["cluster_id"] for d in dets] == want
    assert [d["cluster_probability"] for d in dets] == [0.0 if w is None else 1.0 for w in want]
    json.dumps(dets)
