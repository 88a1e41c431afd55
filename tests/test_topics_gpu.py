"""K17 (eioku_keyword_select) against the float64 oracle, and topic_extraction end to end on the HIP encoder."""
import asyncio
import json

import numpy as np
import pytest

import topics_oracle as to
from eioku_amd import _lib, embed, semantic, task_handler, topics

pytestmark = pytest.mark.gpu

NNZ = [0, 1, 3, 5, 63, 64, 65, 257, 4999]


def _unit(rng, n, d):
    a = rng.standard_normal((n, d))
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


@pytest.fixture(scope="module")
def rows():
    """5 k unit terms (d = 384) and ~300 rows whose candidate counts cycle through NNZ."""
    rng = np.random.default_rng(17)
    W = _unit(rng, 5000, 384)
    lens = [NNZ[i % len(NNZ)] for i in range(297)]
    X = _unit(rng, len(lens), 384)
    row_ptr = np.zeros(len(lens) + 1, np.int32)
    row_ptr[1:] = np.cumsum(lens)
    cand = np.concatenate([np.sort(rng.choice(5000, n, replace=False)) for n in lens]).astype(np.int32)
    return X, W, row_ptr, cand


def _dev(*a):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in a]


def _check_all(X, W, row_ptr, cand, idx, score, count, top_n, lam, tol=1e-5):
    """-> (picks compared, picks excluded as unstable)"""
    total = excluded = 0
    Wd = W.astype(np.float64)
    for r in range(len(X)):
        c = cand[row_ptr[r]:row_ptr[r + 1]]
        out, picks = to.select_row(X[r], W, c, top_n, lam)
        assert count[r] == min(top_n, len(c))
        assert list(idx[r, count[r]:]) == [-1] * (top_n - count[r]) and not score[r, count[r]:].any()
        excluded += to.check_row(idx[r, :count[r]], score[r, :count[r]], out, picks, tol, 2e-6,
                                 lambda i: float(Wd[i] @ X[r].astype(np.float64)))
        total += len(picks)
    return total, excluded


def _call(X, W, row_ptr, cand, top_n, lam):
    idx, score, count = topics.keyword_select(*_dev(X, W, row_ptr, cand), top_n, lam)
    return idx.cpu().numpy(), score.cpu().numpy(), count.cpu().numpy()


def test_k17_matches_oracle_plain_and_mmr(gpu, rows):
    X, W, row_ptr, cand = rows
    total = excluded = 0
    for top_n in (1, 5, 32):
        for lam in (None, 0.0, 0.3, 0.5, 1.0):
            t, e = _check_all(X, W, row_ptr, cand, *_call(X, W, row_ptr, cand, top_n, lam), top_n, lam)
            total += t
            excluded += e
    assert total > 20000 and excluded <= 0.05 * total, (excluded, total)


def test_k17_lambda_zero_equals_plain_and_calls_are_byte_identical(gpu, rows):
    X, W, row_ptr, cand = rows
    for top_n in (5, 32):
        plain = _call(X, W, row_ptr, cand, top_n, None)
        zero = _call(X, W, row_ptr, cand, top_n, 0.0)
        for a, b in zip(plain, zero):
            assert a.tobytes() == b.tobytes()
    first = _call(X, W, row_ptr, cand, 5, 0.5)
    again = _call(X, W, row_ptr, cand, 5, 0.5)
    host = topics.keyword_select(X, W, row_ptr, cand, 5, 0.5)
    for a, b, h in zip(first, again, host):
        assert a.tobytes() == b.tobytes() == h.tobytes()


def test_k17_row_past_lds(gpu):
    """One row of 100,000 candidates: scores and running maxima live in the call's scratch, not in LDS."""
    rng = np.random.default_rng(5)
    W = _unit(rng, 100_000, 256)
    X = _unit(rng, 2, 256)
    row_ptr = np.array([0, 100_000, 100_005], np.int32)
    cand = np.concatenate([np.arange(100_000), np.sort(rng.choice(100_000, 5, replace=False))]).astype(np.int32)
    for top_n, lam in ((32, None), (10, 0.5)):
        res = _call(X, W, row_ptr, cand, top_n, lam)
        total, excluded = _check_all(X, W, row_ptr, cand, *res, top_n, lam)
        assert excluded <= 3, (excluded, total)
        host = topics.keyword_select(X, W, row_ptr, cand, top_n, lam)
        assert all(a.tobytes() == h.tobytes() for a, h in zip(res, host))


def test_k17_argument_errors(gpu):
    rng = np.random.default_rng(0)
    W = _unit(rng, 10, 8)
    X = _unit(rng, 1, 8)
    rp, cand = np.array([0, 3], np.int32), np.array([1, 2, 3], np.int32)
    for top_n, lam in ((0, None), (33, None), (5, 1.5)):
        with pytest.raises(_lib.EiokuHipError, match="code -1"):
            topics.keyword_select(X, W, rp, cand, top_n, lam)
    with pytest.raises(_lib.EiokuHipError, match="multiple of 4"):
        topics.keyword_select(np.ones((1, 6), np.float32), np.ones((10, 6), np.float32), rp, cand, 5, None)
    with pytest.raises(_lib.EiokuHipError, match="outside"):  # checked in the kernel before the term row is read
        topics.keyword_select(X, W, rp, np.array([1, 10, 3], np.int32), 2, 0.5)
    with pytest.raises(_lib.EiokuHipError, match="decreases"):
        topics.keyword_select(np.ones((2, 8), np.float32), W, np.array([0, 3, 2], np.int32), cand, 2, None)


# ---- end to end ----------------------------------------------------------------------------------------------------
WORDS = ["the", "a", "of", "and", "on", "in", "is", "we", "it", "to", "gpu", "kernel", "wave", "memory", "cache", "music",
         "guitar", "solo", "drum", "ocean", "beach", "sunset", "waves", "pasta", "tomato", "sauce", "recipe", "cooking",
         "camera", "video", "scene", "light", "shadow", "travel", "tokyo", "train", "station", "city", "night", "market", "tune"]
SEGMENTS = [
    {"text": "We tune the gpu kernel and the wave memory cache", "start": 0.0, "end": 4.0},
    {"text": "a guitar solo and drum music on the beach", "start": 4.0, "end": 9.5},
    {"text": "ocean waves at sunset on the beach", "start_ms": 9500, "end_ms": 14000},
    {"text": "pasta recipe: tomato sauce cooking in the kitchen", "start": 14.0, "end": 20.0},
    {"text": "the camera video scene light and shadow", "start": 20.0, "end": 25.0},
    {"text": "travel to tokyo by train station at night", "start": 25.0, "end": 31.0},
    {"text": "night market in the city with music", "start": 31.0, "end": 36.0},
    {"text": "the gpu kernel memory and cache", "start": 36.0, "end": 40.0},
    {"text": "", "start": 40.0, "end": 41.0},
]


@pytest.fixture(scope="module")
def engine(tmp_path_factory):
    p = tmp_path_factory.mktemp("vocab") / "vocab.txt"
    lines = ["[PAD]", "[unused0]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", ":", "kitchen", "with", "by", "at"] + WORDS
    p.write_text("\n".join(lines) + "\n", encoding="utf-8")
    cfg = dict(embed.MINILM_L6_V2, vocab=len(lines))
    state = embed.random_state(cfg, 11)
    gen = semantic.EmbeddingGenerator(embed.MiniLMEncoder(state, cfg), semantic.WordPieceTokenizer(p))
    return semantic.SemanticSearchEngine(gen, semantic.VectorStore(384)), state, cfg


def _oracle_embed(gen, state, cfg, texts):
    from oracle import bert as obert

    ids, mask = gen.tokenizer.encode_batch(texts, 256)
    return obert.encode(state, cfg, ids, mask)


@pytest.mark.parametrize("conf", [{"keyphrase_ngram_range": [1, 1]},
                                  {"keyphrase_ngram_range": [1, 2], "use_mmr": True, "diversity": 0.3, "top_n": 4,
                                   "top_n_topics": 6}])
def test_topic_extraction_end_to_end(gpu, engine, conf, tmp_path, monkeypatch):
    import torch

    monkeypatch.setenv("MODEL_CACHE_DIR", str(tmp_path / "models"))
    eng, state, mcfg = engine
    gen = eng.generator
    sink = []
    out = asyncio.run(task_handler.process_ml_task({"artifact_sink": sink.extend, "search_engine": eng}, "t1",
                                                   "topic_extraction", "vidA", "/videos/a.mp4", dict(conf, segments=SEGMENTS)))
    res = topics.TopicExtractor(gen).extract(SEGMENTS, conf)
    cfg = topics.parse_config(conf)
    assert out == {"task_id": "t1", "status": "completed", "artifact_count": len(res["topics"])}
    assert len(res["topics"]) == cfg["top_n_topics"] and len(res["segment_keywords"]) == len(SEGMENTS)
    assert [e.artifact_type for e in sink] == ["topic"] * len(sink)
    for e, t in zip(sink, res["topics"]):
        p = json.loads(e.payload_json)
        assert set(p) == {"label", "keywords", "relevance_score", "frequency", "timestamps", "start_ms", "end_ms"}
        assert p == t and (e.span_start_ms, e.span_end_ms) == (t["start_ms"], t["end_ms"])
        assert t["frequency"] == len(t["timestamps"]) >= 1 and t["timestamps"] == sorted(t["timestamps"])
        assert t["start_ms"] == round(t["timestamps"][0] * 1000) and t["label"] not in t["keywords"]

    # the oracle on float64 embeddings; a pick is compared where its margin exceeds 4x the measured score drift
    vocab = topics.vectorize([s["text"] for s in SEGMENTS], cfg["keyphrase_ngram_range"])
    spans = [topics.segment_span_ms(s) for s in SEGMENTS]
    D = _oracle_embed(gen, state, mcfg, [s["text"] for s in SEGMENTS])
    W = _oracle_embed(gen, state, mcfg, vocab.terms)
    dev = torch.device("cuda:0")
    ext = topics.TopicExtractor(gen)
    Dg = ext.embed_segments([s["text"] for s in SEGMENTS], dev).double().cpu().numpy()
    Wg, calls = ext.embed_terms(vocab.terms, dev)
    Wg = Wg.double().cpu().numpy()
    assert sum(r for r, _ in calls) == len(vocab.terms)
    drift = max(np.abs(Dg @ Wg.T - D @ W.T).max(), np.abs(Wg @ Wg.T - W @ W.T).max(),
                np.abs(to.centroid(Dg) @ Wg.T - to.centroid(D) @ W.T).max())
    tol = 4 * drift + 1e-6
    seg, vid, kws = to.topics(spans, vocab.terms, vocab.row_ptr, vocab.cand, D, W, cfg)
    tid = {t: i for i, t in enumerate(vocab.terms)}
    total = excluded = 0
    for i, (r, (o, p)) in enumerate(zip(res["segment_keywords"], seg)):
        assert (r["start_ms"], r["end_ms"]) == spans[i]
        excluded += to.check_row([tid[k] for k, _ in r["keywords"]], [], o, p, tol)
        total += len(p)
        for k, v in r["keywords"]:  # rounded to 4 places
            assert abs(v - float(D[i] @ W[tid[k]])) <= 5e-5 + tol
    labels = [tid[t["label"]] for t in res["topics"]]
    excluded += to.check_row(labels, [], vid[0], vid[1], tol)
    total += len(vid[1])
    stable = {p[0] for p in vid[1][:to.stable_prefix(vid[1], tol)]}
    for t, (o, p), (l, _) in zip(res["topics"], kws, vid[0]):
        if tid[t["label"]] == l and l in stable:  # the keyword row of a label both sides picked
            excluded += to.check_row([tid[k] for k in t["keywords"]], [], o, p, tol)
            total += len(p)
    for t in res["topics"]:
        assert abs(t["relevance_score"] - float(to.centroid(D) @ W[tid[t["label"]]])) <= 5e-5 + tol
    print(f"topics e2e {conf}: drift {drift:.2e}, {excluded} of {total} picks excluded as unstable")
    assert excluded <= 0.5 * total, (excluded, total)
