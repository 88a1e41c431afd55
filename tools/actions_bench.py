"""Action recognition (K25) cost on one GPU: the base TimeSformer configuration (224 x 224, 8 frames, 12 layers, 400 labels)
with seeded weights on clips of 1080p frames already on the device, written to ``profiles/actions.json``.

Per batch size (1, 8 and 32 clips): clips per second from the wall time around ``classify`` (frames in HBM in, top-5 on the
host out), the device time per stage from the library's own events (``last_ms``: preprocess, encoder, head), and the
fraction of the fp16 MFMA dense peak (2.5 PFLOP/s) the encoder reaches, from ``last_flops``.  The comparison is
``tests/actions_oracle.py``'s torch-CPU fp32 forward on the same machine's threads, one clip.  No number is an acceptance
bar: there is no earlier path to compare with.

    python tools/actions_bench.py [--reps 5] [--batches 1,8,32] [--out profiles/actions.json]
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

PEAK_F16 = 2.5e15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "actions.json"))
    args = ap.parse_args()

    import torch

    import actions_oracle as ao
    from eioku_amd import _lib, actions

    _lib.init()
    cfg = ao.config_w(layers=12)
    hf = ao.hf_config(cfg)
    state = actions.random_state(hf, 5)
    rec = actions.ActionRecognizer(state, hf)
    gen = torch.Generator(device="cuda").manual_seed(1)
    rows = {}
    for B in [int(b) for b in args.batches.split(",")]:
        clips = torch.randint(0, 256, (B, cfg["frames"], args.height, args.width, 3), dtype=torch.uint8, device="cuda", generator=gen)
        rec.classify(clips, 5)  # warm-up: workspaces, tables
        torch.cuda.synchronize()
        best = {}
        for _ in range(args.reps):
            t = time.perf_counter()
            rec.classify(clips, 5)
            wall = (time.perf_counter() - t) * 1e3
            for k, v in {"wall_ms": wall, **{f"{k}_device_ms": v for k, v in rec.last_ms().items()}}.items():
                best[k] = min(best.get(k, v), v)
        flops = rec.last_flops()
        rows[str(B)] = {**{k: round(v, 3) for k, v in best.items()}, "clips_per_second": round(B / best["wall_ms"] * 1e3, 1),
                        "gflop_per_clip": round(flops / B / 1e9, 1),
                        "encoder_tflops": round(flops / best["encoder_device_ms"] / 1e9, 1),
                        "encoder_frac_fp16_peak": round(flops / (best["encoder_device_ms"] * 1e-3) / PEAK_F16, 4)}
        del clips
    rec.close()

    # the CPU oracle, one clip, fp32
    u8 = np.random.default_rng(2).integers(0, 256, (1, cfg["frames"], cfg["image"], cfg["image"], 3), dtype=np.uint8)
    x = ao.patch_rows(ao.normalise(u8))
    oracle = ao.Oracle(cfg, state, fp16=False)
    oracle.forward(x)
    t = time.perf_counter()
    oracle.forward(x)
    cpu_s = time.perf_counter() - t

    result = {"what": "tools/actions_bench.py on one MI355X: TimeSformer base (divided space-time attention, 12 layers, 8 frames of "
                      f"224 x 224, 400 labels), seeded weights, {args.height} x {args.width} BGR frames already on the device; wall ms "
                      f"around classify (top-5 back on the host), device ms from the library's events (best of {args.reps} after a "
                      "warm-up); the CPU figure is tests/actions_oracle.py (torch fp32) on the same machine, preprocessing not "
                      "included; no number is an acceptance bar",
              "device": _lib.device_info(), "reps": args.reps, "batch": rows,
              "cpu_oracle": {"threads": torch.get_num_threads(), "seconds_per_clip": round(cpu_s, 3),
                             "clips_per_second": round(1.0 / cpu_s, 2)}}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
