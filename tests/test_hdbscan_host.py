"""HDBSCAN without a GPU: the numpy tree code of eioku_amd/hdbscan.py against scikit-learn and against the golden arrays
(tests/golden/hdbscan.npz, fed by the float64 oracle of tests/hdbscan_oracle.py instead of the device), the bounded
Boruvka rounds, the option matrix, the two documented deviations, and the ModelManager wiring with fakes."""
import asyncio
import json
import re
from pathlib import Path

import numpy as np
import pytest

import hdbscan_oracle as ho
import test_faces_host as tf
from eioku_amd import _lib, faces, hdbscan

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "hdbscan.npz"


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    index = json.loads(str(g["index"]))
    return g, index


def _variants(golden):
    g, index = golden
    for case, info in index.items():
        emb = g[f"{case}__emb"].astype(np.float32)
        for name, kw in info["variants"].items():
            yield case, name, kw, emb, g[f"{case}__{name}__labels"], g[f"{case}__{name}__prob"], info["labels_only"]


# ---- the tree code is scikit-learn's ---------------------------------------------------------------------------------
def _sk_linkage(model):
    t = model._single_linkage_tree_
    return (t["left_node"].astype(np.int64), t["right_node"].astype(np.int64), t["value"].astype(np.float64),
            t["cluster_size"].astype(np.int64))


TREE_KEYS = ("min_cluster_size", "cluster_selection_method", "allow_single_cluster", "cluster_selection_epsilon", "max_cluster_size")


def _tree_kw(kw):
    return {k: v for k, v in kw.items() if k in TREE_KEYS}


def test_tree_code_on_sklearns_own_linkage_is_sklearn_on_the_golden_cases(golden):
    sk = pytest.importorskip("sklearn.cluster")
    for case, name, kw, emb, _, _, _ in _variants(golden):
        model = sk.HDBSCAN(metric="cosine", **kw).fit(emb)
        labels, prob = hdbscan.tree_to_labels(_sk_linkage(model), **_tree_kw(kw))
        assert np.array_equal(labels, model.labels_), (case, name)
        assert np.abs(prob - model.probabilities_).max() <= 1e-12, (case, name)


OPTIONS = [{}, {"cluster_selection_method": "leaf"}, {"cluster_selection_epsilon": 0.3}, {"allow_single_cluster": True},
           {"max_cluster_size": 30}, {"cluster_selection_method": "leaf", "cluster_selection_epsilon": 0.2, "allow_single_cluster": True},
           {"min_cluster_size": 12, "min_samples": 4}, {"cluster_selection_epsilon": 0.9, "allow_single_cluster": True}]


@pytest.mark.parametrize("seed,n,d,k", [(1, 200, 32, 4), (2, 500, 64, 8), (4, 64, 32, 2), (6, 40, 32, 1)])
def test_tree_code_on_sklearns_own_linkage_is_sklearn_on_generated_sets(seed, n, d, k):
    sk = pytest.importorskip("sklearn.cluster")
    emb = ho.clustered(seed, n, d, k)
    for kw in OPTIONS:
        model = sk.HDBSCAN(metric="cosine", **kw).fit(emb)
        labels, prob = hdbscan.tree_to_labels(_sk_linkage(model), **_tree_kw(kw))
        assert np.array_equal(labels, model.labels_), kw
        assert np.abs(prob - model.probabilities_).max() <= 1e-12, kw


def _tie_orders(u, v, w, rng):
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    rank = np.lexsort((hi, lo))
    pos = np.empty(len(w), np.int64)
    pos[rank] = np.arange(len(w))
    return [np.lexsort((tie, w)) for tie in (pos, -pos, *(rng.permutation(len(w)) for _ in range(3)))]


@pytest.mark.parametrize("seed,n,d,k", [(11, 150, 32, 3), (14, 300, 64, 5), (13, 96, 32, 2)])
def test_oracle_mst_and_tree_code_equal_sklearn_where_the_tie_order_does_not_matter(seed, n, d, k):
    """Guard (a) of the golden generator on a generated set: when five orders of the equal-weight edges agree, the answer
    is scikit-learn's partition and probabilities."""
    sk = pytest.importorskip("sklearn.cluster")
    emb = ho.clustered(seed, n, d, k)
    _, u, v, w, _ = ho.mst(emb, 5)
    u, v = u.astype(np.int64), v.astype(np.int64)
    results = []
    for order in _tie_orders(u, v, w, np.random.default_rng(seed)):
        labels, prob = hdbscan.tree_to_labels(hdbscan.make_single_linkage(u[order], v[order], w[order]))
        results.append((hdbscan.by_first_row(labels), prob))
    # these seeds were kept because the five orders agree; one that does not would say nothing about scikit-learn's answer
    assert all(np.array_equal(r[0], results[0][0]) and np.array_equal(r[1], results[0][1]) for r in results)
    model = sk.HDBSCAN(metric="cosine").fit(emb)
    labels, prob = hdbscan.hdbscan_cosine(emb, mst=ho.mst)
    assert ho.same_partition(labels, model.labels_)
    assert np.abs(prob - model.probabilities_).max() <= 1e-12


# ---- oracle + tree code = golden ------------------------------------------------------------------------------------------
def test_oracle_mst_plus_tree_code_equals_the_golden_arrays(golden):
    for case, name, kw, emb, want, want_p, labels_only in _variants(golden):
        labels, prob = hdbscan.hdbscan_cosine(emb, mst=ho.mst, **kw)
        assert labels.dtype == np.int32 and prob.dtype == np.float64
        assert np.array_equal(labels, want), (case, name)
        if not labels_only:
            assert np.abs(prob - want_p).max() <= 1e-12, (case, name)


def test_golden_holds_the_cases_the_feature_was_specified_with(golden):
    g, index = golden
    shapes = {c: g[f"{c}__emb"].shape for c in index}
    assert shapes == {"tiny": (12, 32), "all_noise": (50, 64), "one_cluster": (40, 32), "min_samples_1": (300, 128),
                      "min_samples_eq_n": (8, 32), "edge_127": (127, 32), "edge_129": (129, 32), "edge_257": (257, 512),
                      "duplicates": (35, 32), "identical": (40, 32), "mixed_1000": (1000, 128)}
    assert set(index["mixed_1000"]["variants"]) == {"eom", "leaf", "eps"}
    assert index["tiny"]["variants"]["v"]["min_samples"] == 2 and index["min_samples_eq_n"]["variants"]["v"]["min_samples"] == 8
    assert index["min_samples_1"]["variants"]["v"]["min_samples"] == 1
    assert len(np.unique(g["identical__emb"], axis=0)) == 1 and len(np.unique(g["duplicates__emb"], axis=0)) == 15
    assert g["mixed_1000__eom__labels"].max() == 19 and GOLDEN.stat().st_size < 1 << 20
    lab_off, lab_on = g["one_cluster__single_off__labels"], g["one_cluster__single_on__labels"]
    assert lab_off.max() == -1 and lab_on.max() == 0


def test_labels_are_numbered_by_first_row():
    assert hdbscan.by_first_row([3, -1, 3, 0, 0, 7]).tolist() == [0, -1, 0, 1, 1, 2]
    assert hdbscan.by_first_row(np.zeros(0, np.int64)).shape == (0,)


# ---- the round bound --------------------------------------------------------------------------------------------------------
def test_round_bound():
    assert [hdbscan.round_bound(n) for n in (1, 2, 3, 4, 5, 40, 1024, 1025, 65536)] == [1, 2, 3, 3, 4, 7, 11, 12, 17]


def test_three_components_with_all_weights_equal_end_within_the_bound():
    """Three groups of equal rows: inside a group every weight is 0, across groups every weight is the same value, so
    only the index tie-break keeps the picked edges a forest."""
    base = np.eye(32, dtype=np.float32)[:3]
    emb = np.repeat(base, 7, axis=0)[np.random.default_rng(0).permutation(21)]
    d = ho.cosine_distances(emb)
    mr = ho.mutual_reachability(d, ho.core_distances(d, 2))
    assert set(np.unique(mr)) == {0.0, 1.0}
    u, v, w, rounds = ho.boruvka(mr, max_rounds=hdbscan.round_bound(21))
    assert ho.spanning_and_acyclic(21, u, v) and rounds <= hdbscan.round_bound(21)
    assert sorted(w.tolist()) == [0.0] * 18 + [1.0] * 2
    every_weight_equal = np.ones((40, 40))
    u, v, w, rounds = ho.boruvka(every_weight_equal, max_rounds=hdbscan.round_bound(40))
    assert ho.spanning_and_acyclic(40, u, v) and rounds <= hdbscan.round_bound(40)


# ---- options ----------------------------------------------------------------------------------------------------------------
def _mixed(golden):
    g, _ = golden
    return g["mixed_1000__emb"].astype(np.float32)[:400]


def test_option_matrix_against_sklearn(golden):
    sk = pytest.importorskip("sklearn.cluster")
    emb = _mixed(golden)
    mst = ho.mst(emb, 5)
    for kw in ({"cluster_selection_method": "leaf"}, {"cluster_selection_epsilon": 0.95}, {"max_cluster_size": 18},
               {"allow_single_cluster": True}, {"cluster_selection_method": "leaf", "cluster_selection_epsilon": 0.95}):
        model = sk.HDBSCAN(metric="cosine", **kw).fit(emb)
        labels, prob = hdbscan.hdbscan_cosine(emb, mst=lambda e, ms: mst, **kw)
        assert ho.same_partition(labels, model.labels_), kw
        assert np.abs(prob - model.probabilities_).max() <= 1e-12, kw


def test_options_change_the_answer(golden):
    emb = _mixed(golden)
    mst = ho.mst(emb, 5)
    run = lambda **kw: hdbscan.hdbscan_cosine(emb, mst=lambda e, ms: mst, **kw)[0]  # noqa: E731
    eom = run()
    assert run(cluster_selection_epsilon=0.95).max() < eom.max()      # epsilon merges clusters
    assert run(max_cluster_size=18).max() != eom.max() or not np.array_equal(run(max_cluster_size=18), eom)
    assert run(cluster_selection_method="leaf").max() >= eom.max()


def test_bad_options_raise():
    e = np.zeros((10, 32), np.float32)
    for kw in ({"min_cluster_size": 1}, {"min_samples": 0}, {"min_samples": 33}, {"min_cluster_size": 40},
               {"cluster_selection_method": "best"}, {"cluster_selection_epsilon": -0.1}, {"max_cluster_size": 0}):
        with pytest.raises(ValueError):
            hdbscan.hdbscan_cosine(e, mst=ho.mst, **kw)


# ---- the two deviations ------------------------------------------------------------------------------------------------------
def test_one_row_and_fewer_rows_than_min_samples_are_all_noise_where_sklearn_raises():
    def never(e, ms):
        raise AssertionError("no MST is needed")

    for n, kw in ((0, {}), (1, {}), (2, {}), (4, {"min_samples": 5}), (2, {"min_cluster_size": 2, "min_samples": 3})):
        labels, prob = hdbscan.hdbscan_cosine(np.ones((n, 32), np.float32), mst=never, **kw)
        assert labels.tolist() == [-1] * n and prob.tolist() == [0.0] * n and labels.dtype == np.int32
    sk = pytest.importorskip("sklearn.cluster")
    with pytest.raises(ValueError):
        sk.HDBSCAN(metric="cosine").fit(np.ones((1, 32)))
    with pytest.raises(ValueError):
        sk.HDBSCAN(metric="cosine", min_samples=5).fit(np.eye(4, 32))


def test_two_rows_are_clustered_not_refused():
    labels, prob = hdbscan.hdbscan_cosine(np.eye(2, 32, dtype=np.float32), min_cluster_size=2, min_samples=1, mst=ho.mst)
    assert labels.tolist() == [-1, -1] and prob.tolist() == [0.0, 0.0]


def test_equal_weight_edges_are_merged_in_index_order():
    lo, hi, w = hdbscan.sort_edges([5, 0, 2, 1], [1, 3, 0, 0], [0.5, 0.5, 0.5, 0.25])
    assert list(zip(lo.tolist(), hi.tolist(), w.tolist())) == [(0, 1, 0.25), (0, 2, 0.5), (0, 3, 0.5), (1, 5, 0.5)]


# ---- wiring --------------------------------------------------------------------------------------------------------------------
class _HEmbedder(tf._Embedder):
    def cluster_hdbscan(self, emb, min_cluster_size, min_samples, selection_epsilon=0.0):
        self.log.append(("hdbscan", emb.shape, min_cluster_size, min_samples, selection_epsilon))
        return hdbscan.hdbscan_cosine(emb, min_cluster_size=min_cluster_size, min_samples=min_samples,
                                      cluster_selection_epsilon=selection_epsilon, mst=ho.mst)


def _manager(tmp_path, frames, log, embedder=_HEmbedder):
    from eioku_amd.model_manager import ModelManager

    return ModelManager(cache_dir=str(tmp_path), frame_source=lambda p: tf._Src(frames), detector_factory=lambda m, c: tf._Detector(),
                        batch_size=2, face_embedder_factory=lambda c, m: embedder(log))


def _frames():
    vals = [0, 1, 3, 0, 2, 6, 4, 1, 3, 4, 6, 7]  # identities val % 3: 0 x 5, 1 x 5, 2 x 1 ... eye rows: exact duplicates
    f = np.zeros((len(vals), 16, 40, 3), np.uint8)
    for i, v in enumerate(vals):
        f[i, 0, 0, 0] = v
    return f


def test_default_method_is_dbscan_and_its_output_is_unchanged(tmp_path):
    cfg = {"frame_interval": 1, "cluster_faces": True, "cluster_eps": 0.2, "cluster_min_samples": 3}
    log, log2 = [], []
    old = asyncio.run(tf._manager(tmp_path, tf._frames(), log).detect_faces("/v.mp4", cfg))  # an embedder with cluster() only
    new = asyncio.run(tf._manager(tmp_path, tf._frames(), log2).detect_faces("/v.mp4", dict(cfg, face_cluster_method="dbscan")))
    assert json.dumps(old, sort_keys=True) == json.dumps(new, sort_keys=True)
    assert all("cluster_probability" not in d for d in old["detections"])
    assert [d["cluster_id"] for d in old["detections"]] == ["face_cluster_001", "face_cluster_002", "face_cluster_001",
                                                            "face_cluster_001", None, "face_cluster_001", "face_cluster_002",
                                                            "face_cluster_002"]
    assert [e for e in log if e[0] == "cluster"] == [("cluster", (8, 32), 0.2, 3)]


def test_hdbscan_method_fills_cluster_id_and_probability(tmp_path):
    from eioku_amd.model_manager import ModelManager

    log = []
    cfg = {"frame_interval": 1, "cluster_faces": True, "face_cluster_method": "hdbscan", "cluster_min_size": 3}
    dets = asyncio.run(_manager(tmp_path, _frames(), log).detect_faces("/v.mp4", cfg))["detections"]
    assert [e for e in log if e[0] == "hdbscan"] == [("hdbscan", (12, 32), 3, ModelManager.CLUSTER_MIN_SAMPLES, 0.0)]
    assert not [e for e in log if e[0] == "cluster"]
    ids = [d["cluster_id"] for d in dets]
    ident = [v % 3 for v in [0, 1, 3, 0, 2, 6, 4, 1, 3, 4, 6, 7]]
    assert ids[0] == "face_cluster_001" and ids[1] == "face_cluster_002" and ids[4] is None
    assert all((a == b) == (ids[i] == ids[j]) for i, a in enumerate(ident) for j, b in enumerate(ident) if a != 2 and b != 2)
    for d in dets:
        assert isinstance(d["cluster_probability"], float)
        assert (d["cluster_probability"] == 0.0) if d["cluster_id"] is None else (0.0 < d["cluster_probability"] <= 1.0)


def test_hdbscan_defaults_and_cluster_eps_only_if_given(tmp_path):
    from eioku_amd.model_manager import ModelManager

    log = []
    base = {"frame_interval": 1, "cluster_faces": True, "face_cluster_method": "hdbscan"}
    asyncio.run(_manager(tmp_path, _frames(), log).detect_faces("/v.mp4", base))
    asyncio.run(_manager(tmp_path, _frames(), log).detect_faces("/v.mp4", dict(base, cluster_eps=0.25, cluster_min_samples=2)))
    assert [e for e in log if e[0] == "hdbscan"] == [
        ("hdbscan", (12, 32), ModelManager.CLUSTER_MIN_SIZE, ModelManager.CLUSTER_MIN_SAMPLES, 0.0),
        ("hdbscan", (12, 32), ModelManager.CLUSTER_MIN_SIZE, 2, 0.25)]
    assert ModelManager.CLUSTER_MIN_SIZE == 5 and ModelManager.CLUSTER_MIN_SAMPLES == 3


def test_bad_method_raises(tmp_path):
    cfg = {"frame_interval": 1, "cluster_faces": True, "face_cluster_method": "kmeans"}
    with pytest.raises(ValueError, match="face_cluster_method"):
        asyncio.run(_manager(tmp_path, _frames(), []).detect_faces("/v.mp4", cfg))
    with pytest.raises(ValueError, match="face_cluster_method"):
        faces.FaceClusterer(None, 0.5, 3, method="kmeans")


def test_analyze_video_and_process_ml_task_carry_the_keys(tmp_path):
    from eioku_amd import task_handler

    cfg = {"frame_interval": 1, "cluster_faces": True, "face_cluster_method": "hdbscan", "cluster_min_size": 3}
    # analyze_video builds its face lane's clusterer from the task's config by the same call as detect_faces (its
    # streams need a device: tests/test_hdbscan_gpu.py runs it)
    c = _manager(tmp_path, _frames(), [])._face_clusterer(dict(cfg, cluster_eps=0.4, cluster_min_samples=2))
    assert (c.method, c.min_cluster_size, c.min_samples, c.eps) == ("hdbscan", 3, 2, 0.4)
    c = _manager(tmp_path, _frames(), [])._face_clusterer({"cluster_faces": True})
    assert (c.method, c.min_samples, c.eps) == ("dbscan", 3, 0.5)
    sent = []
    res = asyncio.run(task_handler.process_ml_task(
        {"artifact_sink": lambda env: sent.extend(env), "model_manager_factory": lambda cache_dir: _manager(tmp_path, _frames(), [])},
        "t1", "face_detection", "vid", "/v.mp4", cfg))
    assert res["status"] == "completed" and res["artifact_count"] == 12
    payloads = [json.loads(e.payload_json) for e in sent]
    assert payloads[1]["cluster_id"] == "face_cluster_002" and payloads[1]["cluster_probability"] > 0.0
    assert payloads[4]["cluster_id"] is None and payloads[4]["cluster_probability"] == 0.0


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_prototype_and_header_declaration_present():
    header = (ROOT / "include" / "eioku_hip.h").read_text()
    m = re.search(r"int eioku_hdbscan_mst_cosine\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == 11
    assert "double* core_out" in m.group(1) and "int32_t* rounds_out" in m.group(1)
    restype, argtypes = _lib.SIGNATURES["eioku_hdbscan_mst_cosine"]
    assert len(argtypes) == 11
    assert "eioku_hdbscan_last_stage_ms" in _lib.SIGNATURES and "int eioku_hdbscan_last_stage_ms(" in header
