"""HDBSCAN on cosine distance: scikit-learn's ``HDBSCAN(metric="cosine")`` without its dense n x n matrix.

The device (K14h, ``csrc/hdbscan.hip``) computes every row's core distance and the minimum spanning tree of the
mutual-reachability graph in float64; everything after the n - 1 tree edges is O(n log n) host work and is restated here
in numpy from scikit-learn 1.7's ``_hdbscan/_linkage.pyx`` (``make_single_linkage``) and ``_hdbscan/_tree.pyx``
(``tree_to_labels``: condensing, stability, excess-of-mass and leaf selection, the epsilon merge, ``max_cluster_size``,
``allow_single_cluster``, labelling, probabilities).  ``alpha`` is 1.

Two deviations from scikit-learn, both documented in INTEGRATION.md:

- ``n == 1`` or ``n < min_samples`` gives all -1 with probability 0 where scikit-learn raises.
- Tree edges of equal weight are merged in the order ``(w, min(u, v), max(u, v))``; scikit-learn's order is an unstable
  argsort over Prim's visiting order.  The partitions agree wherever the answer does not depend on that order.

Labels are scikit-learn's partition numbered by each cluster's smallest row index (as K14's DBSCAN numbers them).
No CPU fallback for the device half.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._buffers import current_stream, on_device, ptr

MAX_ROWS = 65536
MAX_MIN_SAMPLES = 32
NOISE = -1


def round_bound(n: int) -> int:
    """The Boruvka round limit of ``eioku_hdbscan_mst_cosine``: ``ceil(log2 n) + 1``."""
    return (max(int(n), 1) - 1).bit_length() + 1


# ---- device half -------------------------------------------------------------------------------------------------------
def mst_cosine(embeddings, min_samples: int):
    """float32 ``(n, d)`` rows (numpy or CUDA tensor; d % 32 == 0, n <= 65536, 1 <= min_samples <= min(n, 32)) ->
    ``(core float64 (n,), u int32 (n-1,), v int32 (n-1,), w float64 (n-1,), rounds)`` as numpy: the core distances, the
    mutual-reachability MST's edges in no particular order, and the number of Boruvka rounds."""
    lib = _lib.load()
    _lib.init()
    dev = on_device(embeddings)
    if dev:
        import torch

        e = embeddings.contiguous()
        if e.dtype != torch.float32:
            raise ValueError("expected float32 embeddings")
    else:
        e = np.ascontiguousarray(embeddings, dtype=np.float32)
    if len(e.shape) != 2:
        raise ValueError("expected (n, d) embeddings")
    n, d = int(e.shape[0]), int(e.shape[1])
    m = max(n - 1, 0)
    if dev:
        core = torch.empty((n,), dtype=torch.float64, device=e.device)
        u = torch.empty((m,), dtype=torch.int32, device=e.device)
        v = torch.empty((m,), dtype=torch.int32, device=e.device)
        w = torch.empty((m,), dtype=torch.float64, device=e.device)
    else:
        core, u, v, w = np.empty(n, np.float64), np.empty(m, np.int32), np.empty(m, np.int32), np.empty(m, np.float64)
    rounds = np.zeros(1, np.int32)
    _lib.check(lib.eioku_hdbscan_mst_cosine(ptr(e) if n else None, n, d, int(min_samples), ptr(core) if n else None,
                                            ptr(u) if m else None, ptr(v) if m else None, ptr(w) if m else None, ptr(rounds),
                                            _lib.MEM_DEVICE if dev else _lib.MEM_HOST, current_stream(e) if dev else None),
               "eioku_hdbscan_mst_cosine")
    if dev:
        core, u, v, w = (t.cpu().numpy() for t in (core, u, v, w))
    return core, u, v, w, int(rounds[0])


def last_stage_ms() -> list:
    """Device milliseconds of the last ``mst_cosine`` call: ``[core pass, Boruvka round 1, round 2, ...]``."""
    lib = _lib.load()
    buf = np.zeros(40, np.float64)
    k = lib.eioku_hdbscan_last_stage_ms(ptr(buf), len(buf))
    if k < 0:
        _lib.check(k, "eioku_hdbscan_last_stage_ms")
    return [float(x) for x in buf[:k]]


# ---- _linkage.pyx ------------------------------------------------------------------------------------------------------
def sort_edges(u, v, w):
    """Edges in the product's order ``(w, min(u, v), max(u, v))`` -> ``(lo, hi, w)``."""
    u, v, w = np.asarray(u, np.int64), np.asarray(v, np.int64), np.asarray(w, np.float64)
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    order = np.lexsort((hi, lo, w))
    return lo[order], hi[order], w[order]


def make_single_linkage(u, v, w):
    """``_linkage.pyx::make_single_linkage`` on edges in merge order -> ``(left, right, value, size)`` arrays of n - 1
    rows in scipy's hierarchy format (node n + i is the union made by row i)."""
    m = len(w)
    n = m + 1
    parent = [-1] * (2 * n - 1)
    size = [1] * n + [0] * (n - 1)
    left, right, csize = np.empty(m, np.int64), np.empty(m, np.int64), np.empty(m, np.int64)
    nxt = n
    for i, (a, b) in enumerate(zip(np.asarray(u).tolist(), np.asarray(v).tolist())):
        ra = a
        while parent[ra] != -1:
            ra = parent[ra]
        while parent[a] != -1 and parent[a] != ra:  # fast_find's path compression
            parent[a], a = ra, parent[a]
        rb = b
        while parent[rb] != -1:
            rb = parent[rb]
        while parent[b] != -1 and parent[b] != rb:
            parent[b], b = rb, parent[b]
        left[i], right[i], csize[i] = ra, rb, size[ra] + size[rb]
        parent[ra] = parent[rb] = nxt
        size[nxt] = size[ra] + size[rb]
        nxt += 1
    return left, right, np.asarray(w, np.float64).copy(), csize


# ---- _tree.pyx ---------------------------------------------------------------------------------------------------------
def _bfs_hierarchy(left, right, n, root):
    result, queue = [], [root]
    while queue:
        result.extend(queue)
        nxt = []
        for x in queue:
            if x >= n:
                nxt.append(left[x - n])
                nxt.append(right[x - n])
        queue = nxt
    return result


def condense_tree(linkage, min_cluster_size: int):
    """``_condense_tree`` -> ``(parent int64, child int64, lambda float64, size int64)`` rows in its order."""
    left, right, value, csize = (a.tolist() for a in linkage)
    m = len(value)
    n, root = m + 1, 2 * m
    next_label = n + 1
    relabel = [0] * (root + 1)
    relabel[root] = n
    ignore = [False] * (root + 1)
    P, Ch, L, S = [], [], [], []
    for node in _bfs_hierarchy(left, right, n, root):
        if ignore[node] or node < n:
            continue
        lft, rgt, dist = left[node - n], right[node - n], value[node - n]
        lam = 1.0 / dist if dist > 0.0 else np.inf
        lc = csize[lft - n] if lft >= n else 1
        rc = csize[rgt - n] if rgt >= n else 1
        if lc >= min_cluster_size and rc >= min_cluster_size:
            for side, cnt in ((lft, lc), (rgt, rc)):
                relabel[side] = next_label
                next_label += 1
                P.append(relabel[node]), Ch.append(relabel[side]), L.append(lam), S.append(cnt)
            continue
        drop = []
        if lc < min_cluster_size and rc < min_cluster_size:
            drop = [lft, rgt]
        elif lc < min_cluster_size:
            relabel[rgt] = relabel[node]
            drop = [lft]
        else:
            relabel[lft] = relabel[node]
            drop = [rgt]
        for side in drop:
            for sub in _bfs_hierarchy(left, right, n, side):
                if sub < n:
                    P.append(relabel[node]), Ch.append(sub), L.append(lam), S.append(1)
                ignore[sub] = True
    return np.asarray(P, np.int64), np.asarray(Ch, np.int64), np.asarray(L, np.float64), np.asarray(S, np.int64)


def compute_stability(condensed) -> dict:
    parent, child, lam, size = condensed
    smallest = int(parent.min())
    births = np.full(max(int(child.max()), smallest) + 1, np.nan)
    births[child] = lam
    births[smallest] = 0.0
    with np.errstate(invalid="ignore"):
        # np.bincount adds its weights row by row, as the loop of _compute_stability does
        res = np.bincount(parent - smallest, weights=(lam - births[parent]) * size, minlength=int(parent.max()) - smallest + 1)
    return {i + smallest: float(x) for i, x in enumerate(res)}


class _ClusterTree:
    """The rows of the condensed tree whose child is a cluster (``cluster_size > 1``), with the lookups that
    ``_get_clusters`` does by masking."""

    def __init__(self, condensed):
        parent, child, lam, size = condensed
        keep = size > 1
        self.parent, self.child, self.lam, self.size = (a[keep].tolist() for a in (parent, child, lam, size))
        self.children: dict = {}
        self.parent_of, self.lam_of = {}, {}
        for p, c, l in zip(self.parent, self.child, self.lam):
            self.children.setdefault(p, []).append(c)
            self.parent_of[c], self.lam_of[c] = p, l

    def __len__(self):
        return len(self.child)

    def root(self):
        return min(self.parent)

    def bfs(self, node):
        result, queue = [], [node]
        while queue:
            result.extend(queue)
            queue = [c for p in queue for c in self.children.get(p, ())]
        return result

    def leaves(self):
        if not len(self):
            return []
        out, stack = [], [self.root()]
        while stack:
            node = stack.pop()
            kids = self.children.get(node)
            if kids:
                stack.extend(reversed(kids))
            else:
                out.append(node)
        return out


def _traverse_upwards(tree: _ClusterTree, eps: float, leaf: int, allow_single_cluster: bool) -> int:
    root = tree.root()
    while True:
        parent = tree.parent_of[leaf]
        if parent == root:
            return parent if allow_single_cluster else leaf
        with np.errstate(divide="ignore"):
            parent_eps = float(1.0 / np.float64(tree.lam_of[parent]))
        if parent_eps > eps:
            return parent
        leaf = parent


def _epsilon_search(leaves, tree: _ClusterTree, eps: float, allow_single_cluster: bool) -> set:
    selected, processed = [], set()
    for leaf in leaves:
        with np.errstate(divide="ignore"):
            leaf_eps = float(1.0 / np.float64(tree.lam_of[leaf]))
        if leaf_eps < eps:
            if leaf not in processed:
                top = _traverse_upwards(tree, eps, leaf, allow_single_cluster)
                selected.append(top)
                processed.update(s for s in tree.bfs(top) if s != top)
        else:
            selected.append(leaf)
    return set(selected)


def get_clusters(condensed, stability: dict, method: str, allow_single_cluster: bool, eps: float, max_cluster_size):
    """``_get_clusters`` -> ``(labels int64 in scikit-learn's numbering, probabilities float64)``."""
    parent, child, lam, size = condensed
    node_list = sorted(stability, reverse=True)
    if not allow_single_cluster:
        node_list = node_list[:-1]
    tree = _ClusterTree(condensed)
    is_cluster = {c: True for c in node_list}
    n = int(child[size == 1].max()) + 1
    if max_cluster_size is None:
        max_cluster_size = n + 1
    sizes = dict(zip(tree.child, tree.size))
    if allow_single_cluster:
        sizes[node_list[-1]] = sum(s for p, s in zip(tree.parent, tree.size) if p == node_list[-1])
    if method == "eom":
        for node in node_list:
            with np.errstate(invalid="ignore"):
                subtree = float(np.sum([stability[c] for c in tree.children.get(node, ())]))
            if subtree > stability[node] or sizes[node] > max_cluster_size:
                is_cluster[node] = False
                stability[node] = subtree
            else:
                for sub in tree.bfs(node):
                    if sub != node:
                        is_cluster[sub] = False
        if eps != 0.0 and len(tree) > 0:
            eom = [c for c in is_cluster if is_cluster[c]]
            selected = []
            if len(eom) == 1 and eom[0] == tree.root():
                if allow_single_cluster:
                    selected = eom
            else:
                selected = _epsilon_search(set(eom), tree, eps, allow_single_cluster)
            for c in is_cluster:
                is_cluster[c] = c in selected
    elif method == "leaf":
        leaves = set(tree.leaves())
        if not leaves:
            for c in is_cluster:
                is_cluster[c] = False
            is_cluster[int(parent.min())] = True
        selected = _epsilon_search(leaves, tree, eps, allow_single_cluster) if eps != 0.0 else leaves
        for c in is_cluster:
            is_cluster[c] = c in selected
    else:
        raise ValueError(f"cluster_selection_method must be 'eom' or 'leaf', got {method!r}")
    clusters = {c for c in is_cluster if is_cluster[c]}
    cluster_map = {c: k for k, c in enumerate(sorted(clusters))}
    labels = _do_labelling(condensed, tree, clusters, cluster_map, allow_single_cluster, eps)
    return labels, _probabilities(condensed, {k: c for c, k in cluster_map.items()}, labels)


def _do_labelling(condensed, tree: _ClusterTree, clusters: set, cluster_map: dict, allow_single_cluster: bool, eps: float):
    """``_do_labelling``.  Its union-find joins a child to its parent unless the child is a selected cluster, and a
    child is always a fresh singleton there, so the representative of a point is its topmost ancestor below (or at) the
    nearest selected cluster: computed here top-down instead."""
    parent, child, lam, size = condensed
    root = int(parent.min())
    top = {root: root}
    for p, c in zip(tree.parent, tree.child):  # rows come parents first
        top[c] = c if c in clusters else top[p]
    pts = size == 1
    pp, pc, pl = parent[pts], child[pts], lam[pts]
    rep = np.array([top[p] for p in pp.tolist()], np.int64)
    lut = np.full(int(parent.max()) + 1, NOISE, np.int64)
    for c, k in cluster_map.items():
        lut[c] = k
    lab = np.where(rep != root, lut[rep], NOISE)
    if len(clusters) == 1 and allow_single_cluster:
        at_root = rep == root
        if at_root.any():
            threshold = 1.0 / eps if eps != 0.0 else lam[parent == root].max()
            lab = np.where(at_root & (pl >= threshold), lut[root], lab)
    result = np.full(root, NOISE, np.int64)
    result[pc] = lab
    return result


def _max_lambdas(parent, lam):
    """``max_lambdas``: per parent the largest lambda of its last run of consecutive rows."""
    deaths = np.zeros(int(parent.max()) + 1)
    starts = np.flatnonzero(np.r_[True, parent[1:] != parent[:-1]])
    for p, v in zip(parent[starts].tolist(), np.maximum.reduceat(lam, starts).tolist()):
        deaths[p] = v
    return deaths


def _probabilities(condensed, reverse_map: dict, labels):
    parent, child, lam, size = condensed
    root = int(parent.min())
    result = np.zeros(len(labels))
    deaths = _max_lambdas(parent, lam)
    pts = child < root
    pc, pl = child[pts], lam[pts]
    lab = labels[pc]
    ok = lab != NOISE
    pc, pl, lab = pc[ok], pl[ok], lab[ok]
    if len(pc):
        rev = np.zeros(max(reverse_map) + 1, np.int64)
        for k, c in reverse_map.items():
            rev[k] = c
        mx = deaths[rev[lab]]
        with np.errstate(invalid="ignore", divide="ignore"):
            result[pc] = np.where((mx == 0.0) | np.isinf(pl), 1.0, np.minimum(pl, mx) / mx)
    return result


def tree_to_labels(linkage, min_cluster_size=5, cluster_selection_method="eom", allow_single_cluster=False,
                   cluster_selection_epsilon=0.0, max_cluster_size=None):
    """``_tree.pyx::tree_to_labels`` on ``(left, right, value, size)`` -> ``(labels, probabilities)`` in scikit-learn's
    own numbering."""
    condensed = condense_tree(linkage, int(min_cluster_size))
    return get_clusters(condensed, compute_stability(condensed), cluster_selection_method, bool(allow_single_cluster),
                        float(cluster_selection_epsilon), max_cluster_size)


def by_first_row(labels) -> np.ndarray:
    """Any numbering of a partition -> int32 labels numbered by each cluster's smallest row index; -1 stays."""
    labels = np.asarray(labels)
    out = np.full(len(labels), NOISE, np.int32)
    seen: dict = {}
    for i, v in enumerate(labels.tolist()):
        if v >= 0:
            out[i] = seen.setdefault(v, len(seen))
    return out


def labels_from_mst(u, v, w, **options):
    """MST edges (any order) -> ``(labels int32 by first row, probabilities float64)``."""
    labels, prob = tree_to_labels(make_single_linkage(*sort_edges(u, v, w)), **options)
    return by_first_row(labels), prob


def check_options(min_cluster_size, min_samples, cluster_selection_method, cluster_selection_epsilon, max_cluster_size):
    if int(min_cluster_size) < 2:
        raise ValueError(f"min_cluster_size = {min_cluster_size} must be >= 2")
    if min_samples is not None and not 1 <= int(min_samples) <= MAX_MIN_SAMPLES:
        raise ValueError(f"min_samples = {min_samples} outside [1, {MAX_MIN_SAMPLES}]")
    if min_samples is None and int(min_cluster_size) > MAX_MIN_SAMPLES:
        raise ValueError(f"min_samples defaults to min_cluster_size = {min_cluster_size}, above {MAX_MIN_SAMPLES}: pass min_samples")
    if cluster_selection_method not in ("eom", "leaf"):
        raise ValueError(f"cluster_selection_method must be 'eom' or 'leaf', got {cluster_selection_method!r}")
    if not float(cluster_selection_epsilon) >= 0.0:
        raise ValueError(f"cluster_selection_epsilon = {cluster_selection_epsilon} must be >= 0")
    if max_cluster_size is not None and int(max_cluster_size) < 1:
        raise ValueError(f"max_cluster_size = {max_cluster_size} must be >= 1 or None")


def hdbscan_cosine(embeddings, min_cluster_size=5, min_samples=None, cluster_selection_method="eom",
                   cluster_selection_epsilon=0.0, allow_single_cluster=False, max_cluster_size=None, mst=None):
    """scikit-learn ``HDBSCAN(min_cluster_size, min_samples, metric="cosine", ...).fit(embeddings)`` -> ``(labels int32
    (n,), probabilities float64 (n,))``, numpy: the partition of ``labels_`` numbered by each cluster's smallest row
    index (-1 = noise) and ``probabilities_``.  ``embeddings`` float32 ``(n, d)``, numpy or CUDA tensor, d % 32 == 0,
    n <= 65536; ``min_samples`` (default ``min_cluster_size``) at most 32.  ``mst`` replaces the device half by a function
    ``(embeddings, min_samples) -> (core, u, v, w, rounds)`` (tests)."""
    check_options(min_cluster_size, min_samples, cluster_selection_method, cluster_selection_epsilon, max_cluster_size)
    ms = int(min_cluster_size if min_samples is None else min_samples)
    n = int(embeddings.shape[0])
    if n > MAX_ROWS:
        raise ValueError(f"n = {n} above {MAX_ROWS}")
    if n <= 1 or n < ms:  # scikit-learn raises; a video with two faces must not fail its task
        return np.full(n, NOISE, np.int32), np.zeros(n, np.float64)
    _, u, v, w, _ = (mst or mst_cosine)(embeddings, ms)
    return labels_from_mst(u, v, w, min_cluster_size=int(min_cluster_size), cluster_selection_method=cluster_selection_method,
                           allow_single_cluster=allow_single_cluster, cluster_selection_epsilon=cluster_selection_epsilon,
                           max_cluster_size=max_cluster_size)
