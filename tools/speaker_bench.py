"""Speaker labels (K24) cost on one GPU: one hour of 16 kHz synthetic audio with a synthetic transcript of about 1200
segments of 2-8 s through ``SpeakerLabeller`` with seeded r34 weights, written to ``profiles/speakers.json``.

Device time is split by the library's own events into features (``k_spk_fbank`` / ``k_spk_cmn``), the network (the conv
family) and pooling + ``seg_1``; the wall time of ``label`` (upload, window plan, clustering, labels' trip back) is reported
beside it.  The comparison is ``tests/speaker_oracle.py``'s torch-CPU fp32 path (float64 features, fp32 network) on the
same machine over the first ``--cpu-windows`` windows, as windows per second.  No number is an acceptance bar: there is no
earlier path to compare with.

    python tools/speaker_bench.py [--reps 3] [--seconds 3600] [--cpu-windows 32] [--out profiles/speakers.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def synthetic_transcript(seconds: int, rng) -> list:
    """Back-to-back segments of 2-8 s, short ones more often than long ones (3 s on average: about 1200 per hour)."""
    segments, t = [], 0
    while True:
        length = 2000 + min(6000, int(rng.exponential(1050)))
        if t + length > seconds * 1000:
            return segments
        segments.append({"start_ms": t, "end_ms": t + length})
        t += length


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--cpu-windows", type=int, default=32)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "speakers.json"))
    args = ap.parse_args()

    import torch

    import speaker_oracle as so
    from eioku_amd import _lib, speakers

    _lib.init()
    rng = np.random.default_rng(1)
    # voices change every 10 s; the weights are random, so the labels mean nothing - only the cost is measured
    block = 10 * so.RATE
    blocks = [so.voice(100 + i, *so.VOICES[i % 3], block) for i in range(6)]
    audio = np.concatenate([blocks[int(i)] for i in rng.integers(0, 6, -(-args.seconds * so.RATE // block))])[:args.seconds * so.RATE]
    segments = synthetic_transcript(args.seconds, rng)
    plan = [w for s in segments for w in speakers.plan_windows(s["start_ms"], s["end_ms"], audio.size)]
    sd = speakers.random_state_dict(3, speakers.DEPTHS["r34"])
    lab = speakers.SpeakerLabeller(speakers.fold_state(sd))
    lab.label(audio[:30 * so.RATE], [{"start_ms": 0, "end_ms": 9000}, {"start_ms": 9000, "end_ms": 20000}])  # warm-up
    best: dict = {}
    for _ in range(args.reps):
        t = time.perf_counter()
        vectors, index = lab.embed_segments(audio, segments)
        torch.cuda.synchronize()
        embed_wall = (time.perf_counter() - t) * 1e3
        f_ms, n_ms, h_ms = lab.last_ms()
        t = time.perf_counter()
        labels = lab.label(audio, segments)
        label_wall = (time.perf_counter() - t) * 1e3
        for k, v in (("features_device_ms", f_ms), ("network_device_ms", n_ms), ("pool_head_device_ms", h_ms),
                     ("embed_segments_wall_ms", embed_wall), ("label_wall_ms", label_wall)):
            best[k] = min(best.get(k, v), v)
    lab.close()
    device_ms = best["features_device_ms"] + best["network_device_ms"] + best["pool_head_device_ms"]

    cpu_plan = plan[:args.cpu_windows]
    net = so.resnet(sd)
    t = time.perf_counter()
    feats = so.features(audio, cpu_plan, speakers.WIN)
    cpu_feat = time.perf_counter() - t
    t = time.perf_counter()
    so.pooled(net, so.network_input(feats), [v for _, v in cpu_plan])
    cpu_net = time.perf_counter() - t

    result = {"what": "tools/speaker_bench.py on one MI355X: seeded r34 weights, synthetic voices and transcript; device ms from the "
                      f"library's events summed over the passes, wall ms around the synchronous calls (best of {args.reps} after a "
                      "warm-up); the CPU figure is tests/speaker_oracle.py (float64 features, torch fp32 network) on the same "
                      "machine; no number is an acceptance bar",
              "device": _lib.device_info(), "audio_seconds": args.seconds, "segments": len(segments), "embedded_segments": len(index),
              "windows": len(plan), "reps": args.reps, **{k: round(v, 3) for k, v in best.items()},
              "device_ms": round(device_ms, 3), "windows_per_second_device": round(len(plan) / device_ms * 1e3, 1),
              "windows_per_second_wall": round(len(plan) / best["embed_segments_wall_ms"] * 1e3, 1),
              "labels": {"speakers": len({v for v in labels if v}), "none": sum(v is None for v in labels),
                         "eps": speakers.DEFAULT_EPS, "assign_max": speakers.DEFAULT_ASSIGN_MAX},
              "cpu_oracle": {"windows": len(cpu_plan), "threads": torch.get_num_threads(), "features_s": round(cpu_feat, 3),
                             "network_s": round(cpu_net, 3),
                             "windows_per_second": round(len(cpu_plan) / (cpu_feat + cpu_net), 2)}}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
