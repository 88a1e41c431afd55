"""float64 numpy oracle for K14h (csrc/hdbscan.hip): what the device half of HDBSCAN must compute, written the plain way
with the dense n x n matrix the device never stores.

- ``cosine_distances``: ``sklearn.metrics.pairwise.cosine_distances`` on ``emb.astype(float64)``.
- ``core_distances``: ``np.partition(D, min_samples - 1, axis=0)[min_samples - 1]``.
- ``mutual_reachability``: ``max(core_i, core_j, d_ij)``.
- ``boruvka``: a minimum spanning tree under the product's total order ``(w, min(i, j), max(i, j))``, round by round, with
  the round count; ``max_rounds`` bounds it as the device call is bounded.
- ``mst``: all of it from embeddings, with the signature ``hdbscan_cosine(mst=...)`` takes.
- ``clustered``: seeded unit-norm test sets.
"""
from __future__ import annotations

import numpy as np


def cosine_distances(emb) -> np.ndarray:
    x = np.asarray(emb, np.float64)
    nrm = np.sqrt(np.einsum("ij,ij->i", x, x))
    nrm[nrm == 0.0] = 1.0
    x = x / nrm[:, None]
    d = 1.0 - x @ x.T
    np.clip(d, 0.0, 2.0, out=d)
    np.fill_diagonal(d, 0.0)
    return d


def core_distances(dist: np.ndarray, min_samples: int) -> np.ndarray:
    return np.partition(dist, min_samples - 1, axis=0)[min_samples - 1].copy()


def mutual_reachability(dist: np.ndarray, core: np.ndarray) -> np.ndarray:
    return np.maximum(np.maximum(core[:, None], core[None, :]), dist)


def boruvka(weights: np.ndarray, max_rounds: int | None = None):
    """Dense symmetric ``weights`` -> ``(u, v, w, rounds)``: n - 1 edges, u < v.  Raises when ``max_rounds`` rounds leave
    more than one component."""
    n = len(weights)
    comp = np.arange(n)
    U, V, W = [], [], []
    rounds = 0
    idx = np.arange(n)
    while len(U) < n - 1:
        if max_rounds is not None and rounds >= max_rounds:
            raise RuntimeError(f"{n - len(U)} components left after {rounds} rounds")
        rounds += 1
        best: dict = {}
        for i in range(n):
            other = comp != comp[i]
            js = idx[other]
            w = weights[i, js]
            k = np.flatnonzero(w == w.min())[0]  # smallest j among the smallest weights
            j = int(js[k])
            key = (float(w[k]), min(i, j), max(i, j))
            c = int(comp[i])
            if c not in best or key < best[c]:
                best[c] = key
        for key in sorted(set(best.values())):
            w, a, b = key
            ca, cb = comp[a], comp[b]
            if ca == cb:
                raise AssertionError("the picked edges do not form a forest")
            comp[comp == cb] = ca
            U.append(a), V.append(b), W.append(w)
    return np.asarray(U, np.int32), np.asarray(V, np.int32), np.asarray(W, np.float64), rounds


def mst(emb, min_samples: int):
    """``(core, u, v, w, rounds)`` as ``eioku_amd.hdbscan.mst_cosine`` returns them."""
    d = cosine_distances(emb)
    core = core_distances(d, min_samples)
    return (core, *boruvka(mutual_reachability(d, core)))


def spanning_and_acyclic(n: int, u, v) -> bool:
    """n - 1 edges that join n nodes without closing a cycle."""
    if len(u) != n - 1:
        return False
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(np.asarray(u).tolist(), np.asarray(v).tolist()):
        if not (0 <= a < n and 0 <= b < n):
            return False
        ra, rb = find(a), find(b)
        if ra == rb:
            return False
        parent[ra] = rb
    return True


def same_partition(a, b) -> bool:
    """Two labelings put the same rows together and the same rows into noise (-1)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(a < 0, b < 0):
        return False
    fwd, back = {}, {}
    for x, y in zip(a.tolist(), b.tolist()):
        if x < 0:
            continue
        if fwd.setdefault(x, y) != y or back.setdefault(y, x) != x:
            return False
    return True


def clustered(seed: int, n: int, d: int, k: int, noise: float = 0.05, spread: float = 0.25) -> np.ndarray:
    """Unit-norm float32 rows: k directions with Gaussian spread, a fraction ``noise`` of random directions, shuffled."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((k, d))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    m = int(round(n * noise))
    which = rng.integers(0, k, n - m)
    x = centres[which] + spread / np.sqrt(d) * rng.standard_normal((n - m, d))
    x = np.concatenate([x, rng.standard_normal((m, d))])
    x = x[rng.permutation(n)]
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)
