"""Float64 numpy restatement of the topic_extraction contract (KeyBERT extract_keywords defaults).

Test infrastructure.  Selection of a row: plain (the top_n largest s) or MMR (argmax s, then argmax of
(1 - lambda) * s_t - lambda * max_k dot(w_t, w_k)); every argmax breaks ties by the smaller term id; the output is the
picks ordered by s descending.  Each pick also carries its deciding margin (chosen key minus the best other key at that
step), so a test can tell a pick that rounding may flip from one it may not.  Embeddings for the end-to-end check come
from ``oracle/bert.py`` in float64.
"""
from __future__ import annotations

import numpy as np


def select_row(x, W, cand, top_n: int, diversity: float | None):
    """-> (out [(id, s)] ordered by s desc / id asc, picks [(id, margin)] in pick order).  ``diversity`` None: plain."""
    cand = np.asarray(cand, np.int64)
    n = len(cand)
    if n == 0:
        return [], []
    Wc = np.asarray(W)[cand].astype(np.float64)
    s = Wc @ np.asarray(x, np.float64)
    m = np.full(n, -np.inf)
    taken = np.zeros(n, bool)
    picks = []
    for i in range(min(top_n, n)):
        if diversity is None or i == 0:
            key = s.copy()
        else:
            m = np.maximum(m, Wc @ Wc[picks[-1][2]])
            key = (1.0 - diversity) * s - diversity * m
        key[taken] = -np.inf
        order = np.lexsort((cand, -key))  # key desc, then term id asc
        j = order[0]
        # every unpicked key is finite and every picked one -inf, so the runner-up is order[1] while one is left
        margin = float(key[j] - key[order[1]]) if i + 1 < n else np.inf
        picks.append((int(cand[j]), margin, j))
        taken[j] = True
    sel = [p[2] for p in picks]
    out = sorted(((int(cand[j]), float(s[j])) for j in sel), key=lambda t: (-t[1], t[0]))
    return out, [(p[0], p[1]) for p in picks]


def centroid(D):
    c = np.asarray(D, np.float64).sum(0)
    return c / np.linalg.norm(c)


def stable_prefix(picks, tol: float) -> int:
    """Number of leading picks whose deciding margin exceeds ``tol`` (after the first unstable pick, MMR's later keys
    depend on it, so nothing after it is compared)."""
    k = 0
    while k < len(picks) and picks[k][1] > tol:
        k += 1
    return k


def check_row(got_ids, got_scores, out, picks, tol: float, score_tol: float | None = None, s_of=None):
    """Compare one row: the margin-stable picks must be among the returned ids; when every pick is stable, the returned
    ids equal the oracle's output in order wherever consecutive s differ by more than ``tol``.  -> picks excluded."""
    got_ids = [int(i) for i in got_ids]
    assert len(got_ids) == len(out), (got_ids, out)
    k = stable_prefix(picks, tol)
    assert {p[0] for p in picks[:k]} <= set(got_ids), (got_ids, picks, k)
    if k == len(picks):
        assert set(got_ids) == {o[0] for o in out}
        want = [o[0] for o in out]
        for a in range(len(want) - 1):
            if out[a][1] - out[a + 1][1] > tol:
                assert got_ids.index(want[a]) < got_ids.index(want[a + 1]), (got_ids, out)
    if score_tol is not None:
        for i, v in zip(got_ids, got_scores):
            assert abs(float(v) - s_of(i)) <= score_tol, (i, float(v), s_of(i))
    return len(picks) - k


def topics(segments_ms, vocab_terms, row_ptr, cand, D, W, cfg):
    """The whole stage on float64 embeddings D (segments) and W (terms): (segment rows, video row, keyword rows), each
    as select_row's (out, picks)."""
    V = len(vocab_terms)
    seg = [select_row(D[i], W, cand[row_ptr[i]:row_ptr[i + 1]], cfg["top_n"], cfg["diversity"] if cfg["use_mmr"] else None)
           for i in range(len(segments_ms))]
    if V == 0:
        return seg, ([], []), []
    c = centroid(D)
    vid = select_row(c, W, np.arange(V), cfg["top_n_topics"], cfg["diversity"])
    kws = [select_row(W[l], W, np.delete(np.arange(V), l), cfg["top_n"], None) for l, _ in vid[0]]
    return seg, vid, kws
