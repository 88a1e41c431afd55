"""Writes tests/golden/face_dbscan.npz: unit-norm embedding sets with scikit-learn's own DBSCAN(metric="cosine") labels,
which tests/test_faces_gpu.py compares eioku_dbscan_cosine with (scikit-learn need not be installed where that runs).

    python tests/golden/make_face_dbscan.py

Every pairwise cosine distance of every case stays at least 1e-4 away from its eps (checked here), so the labels do not
depend on float32 versus float64 rounding."""
from pathlib import Path

import numpy as np
from sklearn.cluster import DBSCAN

OUT = Path(__file__).resolve().parent / "face_dbscan.npz"


def on_circle(angles, d, seed):
    """Unit vectors at `angles` in a random 2-plane of R^d: cosine distance = 1 - cos(angle difference)."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, 2)))
    a = np.asarray(angles, np.float64)
    return (np.cos(a)[:, None] * q[:, 0] + np.sin(a)[:, None] * q[:, 1]).astype(np.float32)


def clustered(seed, n, d, k, spread, noise=0):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((k, d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = c[rng.integers(0, k, n - noise)] + np.sqrt(2 * spread / d) * rng.standard_normal((n - noise, d))
    x = np.concatenate([x, rng.standard_normal((noise, d))])[rng.permutation(n)]
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def cases():
    # two clusters of six sharing one border point (0.27 rad reaches the last point of each, and nothing else): the border
    # point comes first in index order and must take the smaller label; eps = 1 - cos(0.225)
    a = [0.00, 0.01, 0.02, 0.03, 0.04, 0.05]
    b = [0.49, 0.50, 0.51, 0.52, 0.53, 0.54]
    perm = np.random.default_rng(1).permutation(13)
    pts = on_circle([0.27] + b + a, 64, 2)
    yield "shared_border", np.concatenate([pts[:1], pts[1:][perm[:12] % 12]]), 1 - np.cos(0.225), 6
    yield "all_noise", clustered(3, 50, 64, 1, 0.0, noise=50), 0.1, 2
    yield "one_cluster", clustered(4, 40, 32, 1, 0.05), 0.3, 5
    yield "min_samples_1", clustered(5, 300, 128, 12, 0.1, noise=30), 0.3, 1
    base = clustered(6, 10, 32, 10, 0.0)
    dup = np.concatenate([base, base, base, clustered(7, 5, 32, 5, 0.0)])[np.random.default_rng(8).permutation(35)]
    yield "duplicates", dup, 0.01, 3
    yield "mixed_1000", clustered(9, 1000, 128, 20, 0.1, noise=50), 0.3, 4


def main():
    out = {}
    for name, e, eps, ms in cases():
        e = np.ascontiguousarray(e, np.float32)
        eps = float(np.float32(eps))  # the device compares in float32
        d = 1.0 - e.astype(np.float64) @ e.astype(np.float64).T
        np.fill_diagonal(d, 0.0)
        gap = np.abs(d - eps).min()
        assert gap >= 1e-4, (name, gap)
        labels = DBSCAN(eps=float(eps), min_samples=int(ms), metric="cosine").fit(e).labels_.astype(np.int32)
        out[f"{name}__emb"] = e
        out[f"{name}__eps"] = np.float32(eps)
        out[f"{name}__min_samples"] = np.int32(ms)
        out[f"{name}__labels"] = labels
        print(name, e.shape, "eps", float(np.float32(eps)), "clusters", labels.max() + 1, "noise", int((labels < 0).sum()),
              "gap", gap)
    np.savez_compressed(OUT, **out)


if __name__ == "__main__":
    main()
