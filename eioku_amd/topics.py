"""Topic-extraction stage of the semantic-video-search design: KeyBERT keywords with MMR on the HIP encoder and K17.

The reference schedules ``topic_extraction`` workers and has a ``topics`` table (label, keywords, relevance_score,
timestamps) but never built the stage (``.kiro/specs/semantic-video-search/``: requirement 9, tasks 12.1-12.3 "Use
KeyBERT", design §1.7).  KeyBERT's default model is all-MiniLM-L6-v2, which K8 already runs, so the stage is
``KeyBERT.extract_keywords`` with its defaults, restated:

* candidates: scikit-learn ``CountVectorizer(ngram_range, stop_words="english")`` fitted on the video's segment texts,
  restated in :func:`vectorize` (no scikit-learn at run time; the 318 stop words ship in ``data/english_stop_words.json``);
* embeddings: each segment text and each candidate term through K8 (unit vectors); the video vector is the normalised sum
  of the segment vectors;
* selection: K17 (``eioku_keyword_select``), plain top-n or MMR, on the device; the term embeddings never leave it.

Ties are broken by the smaller vocabulary index everywhere.  The output was not compared with KeyBERT itself (it is not
installed where this is built); ``tests/topics_oracle.py`` restates the contract in float64.
"""
from __future__ import annotations

import json
import re
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _lib
from ._buffers import current_stream, ptr

DEFAULTS = {"top_n": 5, "keyphrase_ngram_range": (1, 1), "use_mmr": False, "diversity": 0.5, "top_n_topics": 10}
MAX_TOP_N = 32
TOKEN_BUDGET = 65536  # tokens per K8 call when embedding terms

_TOKEN = re.compile(r"(?u)\b\w\w+\b")  # CountVectorizer's default token_pattern
_STOP_WORDS: frozenset[str] | None = None


def english_stop_words() -> frozenset[str]:
    """scikit-learn's ``ENGLISH_STOP_WORDS`` (318 words), from ``data/english_stop_words.json``."""
    global _STOP_WORDS
    if _STOP_WORDS is None:
        path = Path(__file__).resolve().parent / "data" / "english_stop_words.json"
        _STOP_WORDS = frozenset(json.loads(path.read_text(encoding="utf-8")))
    return _STOP_WORDS


def analyze(text: str, ngram_range=(1, 1)) -> list[str]:
    """CountVectorizer's analyzer: lower-case, ``\\b\\w\\w+\\b`` tokens, stop words dropped, then n-grams
    ``lo..hi`` joined by one space (so a bigram spans a removed stop word)."""
    lo, hi = ngram_range
    stop = english_stop_words()
    toks = [t for t in _TOKEN.findall(text.lower()) if t not in stop]
    out = list(toks) if lo == 1 else []
    for n in range(max(lo, 2), min(hi, len(toks)) + 1):
        out.extend(" ".join(toks[i:i + n]) for i in range(len(toks) - n + 1))
    return out


@dataclass
class Vocabulary:
    """The fitted vocabulary (sorted terms) and the segment x term count matrix as CSR: segment i's candidates are
    ``cand[row_ptr[i]:row_ptr[i + 1]]``, ascending term ids, with their counts."""

    terms: list[str]
    row_ptr: np.ndarray  # int32 (n_segments + 1,)
    cand: np.ndarray  # int32 (nnz,)
    counts: np.ndarray  # int32 (nnz,)


def vectorize(texts: list[str], ngram_range=(1, 1)) -> Vocabulary:
    """``CountVectorizer(ngram_range=ngram_range, stop_words="english").fit_transform(texts)``, as a :class:`Vocabulary`.
    Unlike scikit-learn, an empty vocabulary is returned rather than raised."""
    docs = []
    for t in texts:
        c: dict[str, int] = {}
        for term in analyze(t, ngram_range):
            c[term] = c.get(term, 0) + 1
        docs.append(c)
    terms = sorted(set().union(*docs)) if docs else []
    tid = {t: i for i, t in enumerate(terms)}
    row_ptr = np.zeros(len(docs) + 1, np.int32)
    cand, counts = [], []
    for i, c in enumerate(docs):
        ids = sorted(tid[t] for t in c)
        cand.extend(ids)
        counts.extend(c[terms[j]] for j in ids)
        row_ptr[i + 1] = len(cand)
    return Vocabulary(terms, row_ptr, np.asarray(cand, np.int32), np.asarray(counts, np.int32))


def _int_in(config: dict, key: str, lo: int, hi: int) -> int:
    v = config.get(key, DEFAULTS[key])
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"topic_extraction: {key} must be an integer in [{lo}, {hi}], got {v!r}")
    return int(v)


def parse_config(config: dict | None) -> dict:
    """The stage's keys with their defaults; a bad value raises ``ValueError``.  Other keys (``segments``) are ignored."""
    config = config or {}
    out = {"top_n": _int_in(config, "top_n", 1, MAX_TOP_N), "top_n_topics": _int_in(config, "top_n_topics", 1, MAX_TOP_N)}
    r = config.get("keyphrase_ngram_range", DEFAULTS["keyphrase_ngram_range"])
    if (not isinstance(r, (list, tuple)) or len(r) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in r)
            or not 1 <= r[0] <= r[1] <= 3):
        raise ValueError(f"topic_extraction: keyphrase_ngram_range must be [lo, hi] with 1 <= lo <= hi <= 3, got {r!r}")
    out["keyphrase_ngram_range"] = (int(r[0]), int(r[1]))
    mmr = config.get("use_mmr", DEFAULTS["use_mmr"])
    if not isinstance(mmr, bool):
        raise ValueError(f"topic_extraction: use_mmr must be true or false, got {mmr!r}")
    out["use_mmr"] = mmr
    dv = config.get("diversity", DEFAULTS["diversity"])
    if isinstance(dv, bool) or not isinstance(dv, (int, float, np.integer, np.floating)) or not 0.0 <= float(dv) <= 1.0:
        raise ValueError(f"topic_extraction: diversity must be a number in [0, 1], got {dv!r}")
    out["diversity"] = float(dv)
    return out


def segment_span_ms(s: dict) -> tuple[int, int]:
    """(start_ms, end_ms) of a transcript segment given in ms or in seconds (as ``segment_embedding`` reads it)."""
    start_ms = int(s["start_ms"]) if "start_ms" in s else int(float(s.get("start", 0.0)) * 1000)
    end_ms = int(s["end_ms"]) if "end_ms" in s else int(float(s.get("end", start_ms / 1000.0)) * 1000)
    return start_ms, end_ms


def keyword_select(x, terms, row_ptr, cand, top_n: int, diversity: float | None):
    """K17 over buffers that all live on one side (numpy arrays or CUDA tensors).  ``diversity`` None: plain top-n.
    -> (idx int32 (rows, top_n), score float32 (rows, top_n), count int32 (rows,)) on the same side."""
    n_rows, d = (int(s) for s in x.shape)
    n_terms = int(terms.shape[0])
    dev = hasattr(x, "is_cuda") and x.is_cuda
    if dev:
        import torch

        idx = torch.empty((n_rows, top_n), dtype=torch.int32, device=x.device)
        score = torch.empty((n_rows, top_n), dtype=torch.float32, device=x.device)
        count = torch.empty((n_rows,), dtype=torch.int32, device=x.device)
    else:
        idx = np.empty((n_rows, top_n), np.int32)
        score = np.empty((n_rows, top_n), np.float32)
        count = np.empty((n_rows,), np.int32)
    lam = -1.0 if diversity is None else float(diversity)
    _lib.check(_lib.load().eioku_keyword_select(ptr(x), n_rows, ptr(terms), n_terms, d, ptr(row_ptr), ptr(cand), top_n, lam,
                                                ptr(idx), ptr(score), ptr(count), _lib.MEM_DEVICE if dev else _lib.MEM_HOST,
                                                current_stream(x)), "eioku_keyword_select")
    return idx, score, count


def _rows(idx: np.ndarray, score: np.ndarray, count: np.ndarray) -> list[list[tuple[int, float]]]:
    return [[(int(idx[r, k]), float(score[r, k])) for k in range(int(count[r]))] for r in range(len(count))]


def build_topics(segments: list[dict], vocab: Vocabulary, seg_rows, video_row, keyword_rows) -> dict:
    """Assemble the stage's result from the three selections (host only).

    ``seg_rows``: per segment ``[(term id, s)]``; ``video_row``: ``[(label id, s(c, label))]``; ``keyword_rows``: per
    label ``[(term id, dot(w_label, w_term))]``; each ordered by s descending."""
    spans = [segment_span_ms(s) for s in segments]
    seg_kw = [{"start_ms": a, "end_ms": b, "keywords": [[vocab.terms[t], round(float(s), 4)] for t, s in row]}
              for (a, b), row in zip(spans, seg_rows)]
    holders: dict[int, list[int]] = {}
    for i in range(len(segments)):
        for t in vocab.cand[vocab.row_ptr[i]:vocab.row_ptr[i + 1]]:
            holders.setdefault(int(t), []).append(i)
    topics = []
    for (label, s), kws in zip(video_row, keyword_rows):
        segs = sorted(holders.get(label, []), key=lambda i: (spans[i][0], i))
        topics.append({"label": vocab.terms[label], "keywords": [vocab.terms[t] for t, _ in kws],
                       "relevance_score": round(float(s), 4), "frequency": len(segs),
                       "timestamps": [spans[i][0] / 1000.0 for i in segs],
                       "start_ms": spans[segs[0]][0] if segs else 0, "end_ms": spans[segs[-1]][1] if segs else 0})
    return {"topics": topics, "segment_keywords": seg_kw}


def aggregate_topics(per_video: dict) -> list[dict]:
    """Requirement 9.3 (TopicSummary): ``{video_id: topics}`` -> ``[{label, frequency, video_ids}]``, frequency = the
    number of videos whose topics carry the label; ordered by frequency descending, then label ascending."""
    seen: dict[str, set] = {}
    for vid, topics in per_video.items():
        for t in topics:
            seen.setdefault(t["label"], set()).add(vid)
    out = [{"label": k, "frequency": len(v), "video_ids": sorted(v)} for k, v in seen.items()]
    return sorted(out, key=lambda r: (-r["frequency"], r["label"]))


class TopicExtractor:
    """KeyBERT keywords and topics for one video's transcript on the GPU.  ``generator``: an
    :class:`eioku_amd.semantic.EmbeddingGenerator` (its encoder and WordPiece tokenizer).  Segment texts and candidate terms
    are tokenised as kind ``"clustering"``: with a nomic-embed-text generator both carry the ``"clustering: "`` task prefix,
    with K8 the prefix is empty."""

    def __init__(self, generator):
        self.generator = generator

    def _encode(self, ids: np.ndarray, mask: np.ndarray, dev):
        import torch

        return self.generator.encoder.encode_ids(torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev))

    def embed_segments(self, texts: list[str], dev):
        """(n, hidden) device tensor of the segment texts (max_seq_length of the generator, 256)."""
        import torch

        g = self.generator
        out = []
        for lo in range(0, len(texts), g.batch_size):
            ids, mask = g.tokenize(texts[lo:lo + g.batch_size], "clustering")
            out.append(self._encode(ids, mask, dev))
        return torch.cat(out) if out else torch.zeros((0, g.encoder.cfg["hidden"]), dtype=torch.float32, device=dev)

    def embed_terms(self, terms: list[str], dev):
        """(V, hidden) device tensor of the term strings in vocabulary order.  Terms are grouped by token count, so a
        batch pads nothing, and each K8 call holds about ``TOKEN_BUDGET`` tokens.  -> (tensor, [(rows, tokens) per call])"""
        import torch

        g = self.generator
        emb = torch.empty((len(terms), g.encoder.cfg["hidden"]), dtype=torch.float32, device=dev)
        calls = []
        if not terms:
            return emb, calls
        ids, mask = g.tokenize(terms, "clustering")
        lens = mask.sum(1).astype(np.int64)
        for L in np.unique(lens):
            rows = np.flatnonzero(lens == L)
            step = max(1, TOKEN_BUDGET // int(L))
            for lo in range(0, len(rows), step):
                r = rows[lo:lo + step]
                e = self._encode(np.ascontiguousarray(ids[r, :L]), np.ascontiguousarray(mask[r, :L]), dev)
                emb.index_copy_(0, torch.from_numpy(r).to(dev), e)
                calls.append((len(r), len(r) * int(L)))
        return emb, calls

    def extract(self, segments: list[dict], config: dict | None = None) -> dict:
        """``{"topics": [...], "segment_keywords": [...]}`` for one video."""
        import torch

        cfg = parse_config(config)
        texts = [s["text"] for s in segments]
        vocab = vectorize(texts, cfg["keyphrase_ngram_range"])
        V = len(vocab.terms)
        if V == 0:
            return build_topics(segments, vocab, [[] for _ in segments], [], [])
        dev = torch.device("cuda", torch.cuda.current_device())
        D = self.embed_segments(texts, dev)
        W, _ = self.embed_terms(vocab.terms, dev)
        c = D.sum(0, keepdim=True)
        c = (c / torch.linalg.vector_norm(c)).contiguous()

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)

        seg = keyword_select(D, W, up(vocab.row_ptr), up(vocab.cand), cfg["top_n"], cfg["diversity"] if cfg["use_mmr"] else None)
        all_terms = up(np.arange(V))
        vid = keyword_select(c, W, up([0, V]), all_terms, cfg["top_n_topics"], cfg["diversity"])
        vi, vs, vc = (t.cpu().numpy() for t in vid)
        video_row = _rows(vi, vs, vc)[0]
        labels = np.array([t for t, _ in video_row], np.int64)
        others = np.concatenate([np.delete(np.arange(V), l) for l in labels])
        kw = keyword_select(W[torch.from_numpy(labels).to(dev)].contiguous(), W, up(np.arange(len(labels) + 1) * (V - 1)),
                            up(others), cfg["top_n"], None)
        seg_rows = _rows(*(t.cpu().numpy() for t in seg))
        keyword_rows = _rows(*(t.cpu().numpy() for t in kw))
        return build_topics(segments, vocab, seg_rows, video_row, keyword_rows)
