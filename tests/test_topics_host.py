"""topic_extraction on the host: the CountVectorizer restatement, record assembly, aggregation, config validation and the
task's error paths (no GPU)."""
import asyncio
import json

import numpy as np
import pytest

from eioku_amd import task_handler, topics

from conftest import GOLDEN


def test_vectorizer_equals_the_scikit_learn_fixture():
    fx = json.loads((GOLDEN / "topics_vectorizer.json").read_text(encoding="utf-8"))
    assert len(fx["cases"]) >= 8
    for case in fx["cases"]:
        v = topics.vectorize(case["texts"], tuple(case["ngram_range"]))
        if case.get("empty"):
            assert v.terms == [] and not v.cand.size and list(v.row_ptr) == [0] * (len(case["texts"]) + 1)
            continue
        assert v.terms == case["vocabulary"], case["ngram_range"]
        assert v.row_ptr.dtype == np.int32 and v.cand.dtype == np.int32
        assert v.row_ptr.tolist() == case["row_ptr"] and v.cand.tolist() == case["cand"] and v.counts.tolist() == case["counts"]


def test_vectorizer_equals_live_count_vectorizer_and_stop_words():
    sk = pytest.importorskip("sklearn.feature_extraction.text")
    assert topics.english_stop_words() == frozenset(sk.ENGLISH_STOP_WORDS) and len(topics.english_stop_words()) == 318
    rng = np.random.default_rng(3)
    words = sorted(sk.ENGLISH_STOP_WORDS)[:60] + ["gpu", "kernel", "wave", "Café", "naïve", "x1", "42", "a1b2", "東京", "don't",
                                                   "it's", "re-run", "MI355X", "topic", "video", "über", "ß", "_under"]
    for rng_ng in [(1, 1), (1, 2), (2, 3), (1, 3), (3, 3)]:
        texts = [" ".join(rng.choice(words, size=int(rng.integers(0, 25)))) for _ in range(40)]
        cv = sk.CountVectorizer(ngram_range=rng_ng, stop_words="english", lowercase=True)
        X = cv.fit_transform(texts).tocsr()
        X.sort_indices()
        v = topics.vectorize(texts, rng_ng)
        assert v.terms == list(cv.get_feature_names_out())
        assert v.row_ptr.tolist() == X.indptr.tolist() and v.cand.tolist() == X.indices.tolist() and v.counts.tolist() == X.data.tolist()


SEGS = [{"text": "gpu kernel", "start_ms": 0, "end_ms": 2000}, {"text": "video topic", "start": 2.0, "end": 4.5},
        {"text": "gpu video", "start_ms": 4500, "end_ms": 7000}, {"text": "the", "start": 7.0, "end": 8.0}]


def test_build_topics_records_from_hand_made_selections():
    v = topics.vectorize([s["text"] for s in SEGS])
    assert v.terms == ["gpu", "kernel", "topic", "video"]
    gpu, kernel, topic, video = range(4)
    seg_rows = [[(gpu, 0.812345), (kernel, 0.5)], [(video, 0.7), (topic, 0.69999)], [(video, 0.4), (gpu, 0.3)], []]
    video_row = [(video, 0.91234), (gpu, 0.88886), (kernel, 0.1)]
    kw_rows = [[(topic, 0.9), (gpu, 0.8)], [(kernel, 0.5)], []]
    r = topics.build_topics(SEGS, v, seg_rows, video_row, kw_rows)
    assert r["segment_keywords"] == [
        {"start_ms": 0, "end_ms": 2000, "keywords": [["gpu", 0.8123], ["kernel", 0.5]]},
        {"start_ms": 2000, "end_ms": 4500, "keywords": [["video", 0.7], ["topic", 0.7]]},
        {"start_ms": 4500, "end_ms": 7000, "keywords": [["video", 0.4], ["gpu", 0.3]]},
        {"start_ms": 7000, "end_ms": 8000, "keywords": []}]
    assert r["topics"] == [
        {"label": "video", "keywords": ["topic", "gpu"], "relevance_score": 0.9123, "frequency": 2, "timestamps": [2.0, 4.5],
         "start_ms": 2000, "end_ms": 7000},
        {"label": "gpu", "keywords": ["kernel"], "relevance_score": 0.8889, "frequency": 2, "timestamps": [0.0, 4.5],
         "start_ms": 0, "end_ms": 7000},
        {"label": "kernel", "keywords": [], "relevance_score": 0.1, "frequency": 1, "timestamps": [0.0], "start_ms": 0,
         "end_ms": 2000}]
    # timestamps ascend by start time even when the segments arrive out of order
    r2 = topics.build_topics([SEGS[2], SEGS[0]], topics.vectorize(["gpu video", "gpu kernel"]), [[], []], [(0, 0.5)], [[]])
    assert r2["topics"][0]["timestamps"] == [0.0, 4.5] and (r2["topics"][0]["start_ms"], r2["topics"][0]["end_ms"]) == (0, 7000)


def test_aggregate_topics_orders_by_video_count_then_label():
    per_video = {"v2": [{"label": "gpu"}, {"label": "music"}], "v1": [{"label": "gpu"}, {"label": "beach"}],
                 "v3": [{"label": "music"}, {"label": "gpu"}, {"label": "art"}], "v4": []}
    assert topics.aggregate_topics(per_video) == [
        {"label": "gpu", "frequency": 3, "video_ids": ["v1", "v2", "v3"]},
        {"label": "music", "frequency": 2, "video_ids": ["v2", "v3"]},
        {"label": "art", "frequency": 1, "video_ids": ["v3"]},
        {"label": "beach", "frequency": 1, "video_ids": ["v1"]}]
    assert topics.aggregate_topics({}) == []


def test_config_defaults_and_validation():
    assert topics.parse_config(None) == {"top_n": 5, "top_n_topics": 10, "keyphrase_ngram_range": (1, 1), "use_mmr": False,
                                         "diversity": 0.5}
    ok = topics.parse_config({"top_n": 32, "top_n_topics": 1, "keyphrase_ngram_range": [2, 3], "use_mmr": True, "diversity": 1,
                              "segments": []})
    assert ok == {"top_n": 32, "top_n_topics": 1, "keyphrase_ngram_range": (2, 3), "use_mmr": True, "diversity": 1.0}
    bad = [{"top_n": 0}, {"top_n": 33}, {"top_n": 2.0}, {"top_n": True}, {"top_n_topics": 0}, {"top_n_topics": 40},
           {"keyphrase_ngram_range": [0, 1]}, {"keyphrase_ngram_range": [2, 1]}, {"keyphrase_ngram_range": [1, 4]},
           {"keyphrase_ngram_range": [1]}, {"keyphrase_ngram_range": "1,2"}, {"use_mmr": 1}, {"use_mmr": "yes"},
           {"diversity": -0.1}, {"diversity": 1.5}, {"diversity": "0.5"}, {"diversity": float("nan")}]
    for c in bad:
        with pytest.raises(ValueError, match="topic_extraction"):
            topics.parse_config(c)


class _NoGpuEngine:
    """An engine whose encoder must never be reached: config errors are raised before any embedding."""

    class generator:
        encoder = None
        tokenizer = None


def test_process_ml_task_errors_name_topic_extraction():
    ctx = {"model_manager_factory": lambda cache_dir: object()}
    with pytest.raises(RuntimeError, match=r"topic_extraction needs config\['segments'\]"):
        asyncio.run(task_handler.process_ml_task(ctx, "t1", "topic_extraction", "v", "/v.mp4", {}))
    with pytest.raises(RuntimeError, match=r"topic_extraction needs ctx\['search_engine'\]"):
        asyncio.run(task_handler.process_ml_task(ctx, "t2", "topic_extraction", "v", "/v.mp4", {"segments": SEGS}))
    ctx["segment_source"] = lambda vid: SEGS
    with pytest.raises(RuntimeError, match=r"topic_extraction needs ctx\['search_engine'\]"):
        asyncio.run(task_handler.process_ml_task(ctx, "t3", "topic_extraction", "v", "/v.mp4", None))
    ctx["search_engine"] = _NoGpuEngine()
    with pytest.raises(RuntimeError, match="top_n must be"):
        asyncio.run(task_handler.process_ml_task(ctx, "t4", "topic_extraction", "v", "/v.mp4", {"top_n": 99}))
    assert task_handler.TASK_TO_ARTIFACT_TYPE["topic_extraction"] == "topic"
    assert task_handler.TASK_TO_RESULT_KEY["topic_extraction"] == "topics" and "topic_extraction" in task_handler.KNOWN_TASK_TYPES


def test_topic_envelopes_span_the_topic():
    result = {"topics": [{"label": "gpu", "keywords": [], "relevance_score": 0.5, "frequency": 2, "timestamps": [0.0, 4.5],
                          "start_ms": 0, "end_ms": 7000}], "segment_keywords": [{"start_ms": 0, "end_ms": 1, "keywords": []}]}
    env = task_handler.result_to_envelopes(result, "t", "topic_extraction", "vid", "run")
    assert len(env) == 1 and env[0].artifact_type == "topic" and (env[0].span_start_ms, env[0].span_end_ms) == (0, 7000)
    assert json.loads(env[0].payload_json)["label"] == "gpu"


def test_keyword_select_argument_checks_need_no_device(built_lib):
    """EIOKU_EINVAL for top_n 0 / 33, diversity > 1 and d % 4 != 0 before the device is touched."""
    x = np.zeros((1, 8), np.float32)
    rp = np.array([0, 1], np.int32)
    cand = np.zeros(1, np.int32)
    out_i, out_s, out_c = np.zeros(33, np.int32), np.zeros(33, np.float32), np.zeros(1, np.int32)
    args = lambda top_n, lam, d: (x.ctypes.data, 1, x.ctypes.data, 1, d, rp.ctypes.data, cand.ctypes.data, top_n, lam,
                                  out_i.ctypes.data, out_s.ctypes.data, out_c.ctypes.data, 0, None)
    for top_n, lam, d, what in [(0, -1.0, 8, b"top_n"), (33, -1.0, 8, b"top_n"), (5, 1.5, 8, b"diversity"),
                                (5, float("nan"), 8, b"diversity"), (5, 0.5, 6, b"d = 6"), (5, 0.5, 1028, b"d = 1028")]:
        assert built_lib.eioku_keyword_select(*args(top_n, lam, d)) == -1
        assert what in built_lib.eioku_last_error()
