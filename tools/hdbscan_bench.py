"""HDBSCAN (K14h) on one GPU, as one JSON object written to ``--out``: seeded clustered 512-d unit vectors (~33 points per
cluster, 5 % noise) at n = 1 000, 10 000 and 65 536, ``min_cluster_size`` 5, ``min_samples`` 5.

Per n: device milliseconds of the core-distance pass and of every Boruvka round (device events inside
``eioku_hdbscan_mst_cosine``, read back by ``last_stage_ms``; the median call of ``--reps``), the round count, the achieved
float64 TFLOP/s of each pass from ``2 n^2 d`` (the Gram products alone: what the pass needs, over the pass's device time),
the host milliseconds of the numpy tree code, the wall time of the whole ``hdbscan_cosine`` call, and for scale K14's
DBSCAN on the same vectors.  On the same box ``sklearn.cluster.HDBSCAN(metric="cosine")`` once at 1 000 and 10 000 with the
partition compared; at 65 536 its dense float64 matrix alone is 34 GB: "not run".

    python tools/hdbscan_bench.py [--reps 5] [--out profiles/hdbscan.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

D = 512


def clustered(seed, n, d, k, spread, noise):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((k, d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = c[rng.integers(0, k, n - noise)] + np.sqrt(2 * spread / d) * rng.standard_normal((n - noise, d))
    x = np.concatenate([x, rng.standard_normal((noise, d))])[rng.permutation(n)]
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a < 0, b < 0):
        return False
    pairs = {(x, y) for x, y in zip(a.tolist(), b.tolist()) if x >= 0}
    return len(pairs) == len({x for x, _ in pairs}) == len({y for _, y in pairs})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1000,10000,65536")
    ap.add_argument("--sklearn-max", type=int, default=10000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hdbscan.json"))
    args = ap.parse_args()
    import torch

    from eioku_amd import _lib, faces, hdbscan

    _lib.init()
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "d": D, "min_cluster_size": 5, "min_samples": 5, "reps": args.reps, "n": {}}
    for n in (int(s) for s in args.sizes.split(",")):
        host = clustered(n, n, D, max(1, n // 33), 0.1, n // 20)
        e = torch.from_numpy(host).to(dev)
        hdbscan.mst_cosine(e, 5)  # warm-up: workspace growth, code objects
        calls = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            core, u, v, w, rounds = hdbscan.mst_cosine(e, 5)  # synchronous
            calls.append((time.perf_counter() - t, hdbscan.last_stage_ms(), rounds))
        calls.sort(key=lambda c: c[0])
        wall, stages, rounds = calls[len(calls) // 2]
        flop = 2.0 * n * n * D
        t = time.perf_counter()
        labels, prob = hdbscan.labels_from_mst(u, v, w, min_cluster_size=5)
        tree_ms = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        labels2, _ = hdbscan.hdbscan_cosine(e, min_cluster_size=5, min_samples=5)
        total_ms = (time.perf_counter() - t) * 1e3
        assert np.array_equal(labels, labels2)
        row = {"rounds": rounds, "round_bound": hdbscan.round_bound(n), "mst_call_ms": round(wall * 1e3, 3),
               "core_pass_ms": round(stages[0], 3), "round_ms": [round(s, 3) for s in stages[1:]],
               "core_pass_fp64_tflops": round(flop / (stages[0] * 1e-3) / 1e12, 2),
               "round_fp64_tflops": [round(flop / (s * 1e-3) / 1e12, 2) for s in stages[1:]],
               "device_ms": round(sum(stages), 3), "host_tree_ms": round(tree_ms, 3), "hdbscan_cosine_ms": round(total_ms, 3),
               "clusters": int(labels.max() + 1), "noise": int((labels < 0).sum())}
        faces.dbscan_cosine(e, 0.3, 5)
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            faces.dbscan_cosine(e, 0.3, 5)  # synchronous
            ts.append(time.perf_counter() - t)
        row["k14_dbscan_ms"] = round(float(np.median(ts)) * 1e3, 3)
        if n <= args.sklearn_max:
            try:
                from sklearn.cluster import HDBSCAN
            except ImportError:
                row["sklearn"] = "not run: scikit-learn is not installed"
            else:
                t = time.perf_counter()
                model = HDBSCAN(min_cluster_size=5, min_samples=5, metric="cosine").fit(host)
                row["sklearn"] = {"ms": round((time.perf_counter() - t) * 1e3, 1), "clusters": int(model.labels_.max() + 1),
                                  "same_partition": bool(same_partition(labels, model.labels_)),
                                  "rows_labelled_differently": int((hdbscan.by_first_row(model.labels_) != labels).sum()),
                                  "max_probability_diff": float(np.abs(prob - model.probabilities_).max())}
        else:
            row["sklearn"] = f"not run: the dense float64 matrix is {n * n * 8 / 1e9:.0f} GB"
        out["n"][str(n)] = row
        del e
    print(json.dumps(out))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
