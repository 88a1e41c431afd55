"""Face clustering throughput on one GPU, as one JSON object: K13 embed (crop + ArcFace r18 on seeded random weights) at
m = 256 crops - faces/s and achieved TF/s from ``last_flops`` - and K14 DBSCAN milliseconds at n = 1 k, 10 k and 65,536
(d = 512, clustered unit vectors: ~33 points per cluster, 5 % noise, eps 0.3, min_samples 5).

    python tools/faces_bench.py [--reps 5]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def clustered(seed, n, d, k, spread, noise):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((k, d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = c[rng.integers(0, k, n - noise)] + np.sqrt(2 * spread / d) * rng.standard_normal((n - noise, d))
    x = np.concatenate([x, rng.standard_normal((noise, d))])[rng.permutation(n)]
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--m", type=int, default=256)
    args = ap.parse_args()
    import torch

    from eioku_amd import _lib, faces

    _lib.init()
    dev = torch.device("cuda", 0)
    emb = faces.FaceEmbedder(faces.fold_state(faces.random_state_dict(3)))
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, (16, 720, 1280, 3), dtype=np.uint8)).to(dev)
    xy = rng.uniform(0, 1100, (args.m, 2))
    side = rng.uniform(40, 300, args.m)
    boxes = np.stack([np.arange(args.m) % 16, xy[:, 0], xy[:, 1] * 0.5, xy[:, 0] + side, xy[:, 1] * 0.5 + side], 1).astype(np.float32)
    emb.embed(frames, boxes)  # warm-up: allocations, code objects
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        emb.embed(frames, boxes)  # synchronous
        ts.append(time.perf_counter() - t)
    t_embed = float(np.median(ts))
    flops = emb.last_flops()
    out = {"embed": {"m": args.m, "ms": round(t_embed * 1e3, 3), "faces_per_s": round(args.m / t_embed, 1),
                     "gflop_per_face": round(flops / args.m / 1e9, 3), "tflops": round(flops / t_embed / 1e12, 2)}}
    emb.close()
    db = {}
    for n in (1000, 10000, 65536):
        e = torch.from_numpy(clustered(n, n, 512, max(1, n // 33), 0.1, n // 20)).to(dev)
        labels = faces.dbscan_cosine(e, 0.3, 5)  # warm-up (workspace growth)
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            labels = faces.dbscan_cosine(e, 0.3, 5)  # synchronous
            ts.append(time.perf_counter() - t)
        lab = labels.cpu().numpy()
        db[str(n)] = {"ms": round(float(np.median(ts)) * 1e3, 3), "clusters": int(lab.max() + 1), "noise": int((lab < 0).sum()),
                      "gram_tflops": round(2.0 * n * n * 512 / float(np.median(ts)) / 1e12, 2)}
    out["dbscan"] = db
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
