"""Sound tagging (K29) cost on one GPU: the published AST configuration (width 768, 12 layers, 12 heads, ffn 3072, 527 labels,
128 mel bins, max_length 1024: 1214 tokens per 10.24 s window) with seeded weights on one hour of synthetic 16 kHz audio
already on the device, written to ``profiles/sounds.json``.

Per windows-per-call (1 and 32): windows per second from the wall time around ``classify`` (audio in HBM in, top-5 on the
host out), the device time per stage from the library's own events (``last_ms``: features, encoder, head), and the encoder's
TFLOP/s from ``last_flops`` (K25 and K26 run the same GEMM and attention kernels at 105 to 107 TFLOP/s).  Then the whole hour
(360 windows, 10 s apart) at 32 windows per call.  The comparison is ``tests/sounds_oracle.py``'s torch-CPU fp32 forward on 16
threads of the same machine, one window, features not included.  No number is an acceptance bar: there is no earlier path.

    python tools/sounds_bench.py [--reps 5] [--batches 1,32] [--hours 1.0] [--out profiles/sounds.json]
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
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sounds.json"))
    args = ap.parse_args()

    import torch

    import sounds_oracle as so
    from eioku_amd import _lib, sounds

    _lib.init()
    state = sounds.random_state({}, 5)
    tagger = sounds.SoundTagger(state, {})
    n = int(args.hours * 3600 * sounds.SAMPLE_RATE)
    gen = torch.Generator(device="cuda").manual_seed(1)
    t = torch.arange(n, device="cuda", dtype=torch.float64) / sounds.SAMPLE_RATE
    audio = (0.05 * torch.randn(n, device="cuda", generator=gen) + (0.1 * torch.sin(2 * np.pi * 440.0 * t)).float()
             + (0.05 * torch.sin(2 * np.pi * 0.2 * t) * torch.sin(2 * np.pi * 2300.0 * t)).float())
    del t
    plan = sounds.plan_windows(n, tagger.max_length, 10 * sounds.SAMPLE_RATE)
    tagger.set_audio(audio)
    rows = {}
    for B in [int(b) for b in args.batches.split(",")]:
        part = plan[:B]
        tagger.classify(None, part, 5, batch_windows=B)  # warm-up: workspaces
        torch.cuda.synchronize()
        best = {}
        for _ in range(args.reps):
            t0 = time.perf_counter()
            tagger.classify(None, part, 5, batch_windows=B)
            wall = (time.perf_counter() - t0) * 1e3
            for k, v in {"wall_ms": wall, **{f"{k}_device_ms": v for k, v in tagger.last_ms().items()}}.items():
                best[k] = min(best.get(k, v), v)
        flops = tagger.last_flops()
        rows[str(B)] = {**{k: round(v, 3) for k, v in best.items()}, "windows_per_second": round(len(part) / best["wall_ms"] * 1e3, 1),
                        "gflop_per_window": round(flops / len(part) / 1e9, 1),
                        "encoder_tflops": round(flops / best["encoder_device_ms"] / 1e9, 1),
                        "encoder_frac_fp16_peak": round(flops / (best["encoder_device_ms"] * 1e-3) / PEAK_F16, 4)}
    t0 = time.perf_counter()
    scores, ids = tagger.classify(None, plan, 5, batch_windows=32)
    whole = time.perf_counter() - t0
    ms = tagger.last_ms()
    hour = {"windows": len(plan), "wall_s": round(whole, 3), "audio_seconds_per_second": round(n / sounds.SAMPLE_RATE / whole, 1),
            **{f"{k}_device_ms": round(v, 1) for k, v in ms.items()}, "tflop": round(tagger.last_flops() / 1e12, 1)}
    tagger.close()
    del audio

    # the CPU oracle, one window, fp32, 16 threads
    torch.set_num_threads(16)
    cfg = {**so.config_w(layers=12), "max_length": 1024}
    x = so.patch_rows(np.random.default_rng(2).standard_normal((1, 1024, 128)).astype(np.float32), cfg)
    oracle = so.Oracle(cfg, state, fp16=False)
    oracle.forward(x)
    t0 = time.perf_counter()
    oracle.forward(x)
    cpu_s = time.perf_counter() - t0

    result = {"what": "tools/sounds_bench.py on one MI355X: AST base (12 layers, width 768, 1214 tokens per 10.24 s window, 527 labels), "
                      f"seeded weights, {args.hours} h of synthetic 16 kHz audio already on the device; wall ms around classify (top-5 "
                      f"back on the host), device ms from the library's events (best of {args.reps} after a warm-up); hour: all windows "
                      "10 s apart at 32 per call, one run; the CPU figure is tests/sounds_oracle.py (torch fp32, 16 threads) on the "
                      "same machine, features not included; no number is an acceptance bar",
              "device": _lib.device_info(), "reps": args.reps, "windows_per_call": rows, "hour": hour,
              "cpu_oracle": {"threads": torch.get_num_threads(), "seconds_per_window": round(cpu_s, 3),
                             "windows_per_second": round(1.0 / cpu_s, 2)}}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
