"""Face clustering throughput on one GPU, as one JSON object: K13 embed (crop + ArcFace r18 on seeded random weights) at
m = 256 crops - faces/s and achieved TF/s from ``last_flops`` - and K14 DBSCAN milliseconds at n = 1 k, 10 k and 65,536
(d = 512, clustered unit vectors: ~33 points per cluster, 5 % noise, eps 0.3, min_samples 5).  With alignment: the same m
faces through K13c (``crop_aligned`` / ``embed_aligned``) against K13a (``crop`` / ``embed``), and ``detect`` of a seeded
``yolov8n-face`` on 64 x 1080p frames without a keypoint head, with one that does not run (``detect()`` on a Pose handle)
and with one that does (``with_kpts``: the dense cv4 branch + K6p).  The object is also written to ``--out``.

    python tools/faces_bench.py [--reps 5] [--out profiles/faces.json]
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
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "faces.json"))
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

    def timed(fn):
        fn()  # warm-up
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        return round(float(np.median(ts)) * 1e3, 3)

    # the same faces, aligned: five landmarks inside each box (the template scaled to the box, tilted by up to 30 degrees)
    ang = rng.uniform(-np.pi / 6, np.pi / 6, args.m)
    R = np.stack([np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang)], 1).reshape(-1, 2, 2)
    lm = np.einsum("mij,kj->mki", R, faces.ARCFACE_DST - 56.0) * (side / 112.0)[:, None, None] + (boxes[:, 1:3] + side[:, None] / 2)[:, None, :]
    M, fallback = faces.align_matrices(lm)
    slots = boxes[:, 0].astype(np.int32)
    out["align"] = {"m": args.m, "fallback": int(fallback.sum()),
                    "crop_box_ms": timed(lambda: emb.crop(frames, boxes)), "crop_aligned_ms": timed(lambda: emb.crop_aligned(frames, slots, M)),
                    "embed_box_ms": timed(lambda: emb.embed(frames, boxes)), "embed_aligned_ms": timed(lambda: emb.embed_aligned(frames, boxes, lm)),
                    "note": "crop_*: the synchronous entry points, host time around one launch (taps / matrices upload included)"}
    emb.close()

    from eioku_amd import detect as D, weights as W

    hd = torch.from_numpy(rng.integers(0, 256, (64, 1080, 1920, 3), dtype=np.uint8)).to(dev)
    pose_state = W.random_state("n", 1, 7, nk=15)
    det0 = D.Yolov8Detector("n", 1, {k: v for k, v in pose_state.items() if ".cv4." not in k})
    det5 = D.Yolov8Detector("n", 1, pose_state)
    for d in (det0, det5):
        d.calibrate_random_head(hd[:2])
    out["detect_64x1080p"] = {
        "detect_nk0_ms": timed(lambda: det0.detect(hd, conf=0.25, keep_on_device=True)),
        "detect_pose_handle_without_kpts_ms": timed(lambda: det5.detect(hd, conf=0.25, keep_on_device=True)),
        "detect_pose_with_kpts_ms": timed(lambda: det5.detect(hd, conf=0.25, keep_on_device=True, with_kpts=True))}
    det0.close()
    det5.close()
    del hd
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
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
