"""CLIP frame and text embeddings (K26) cost on one GPU: the ViT-B/32 and ViT-B/16 configurations (224 x 224, 12 + 12 layers,
projection 512) with seeded weights, written to ``profiles/clip.json``.

Images: 64 frames of 1080p already on the device, embedded 1 and 64 per call: images per second from the wall time around
``encode_images`` (frames in HBM in, unit vectors in HBM out, synchronised), the device time per stage from the library's
own events (``last_ms``: preprocess, encoder, head) and the encoder's achieved TFLOP/s from ``last_flops``.  Text: queries
per second at 1 and 64 per call (ids on the host in, vectors on the host out; 8 real tokens per query, so 10 positions are
run).  The comparison is ``tests/clip_oracle.py``'s torch-CPU fp32 forward on the same machine's threads, one image and one
query.  No number is an acceptance bar: there is no earlier path to compare with.

    python tools/clip_bench.py [--reps 5] [--out profiles/clip.json]
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
FRAMES = 64


def config(patch: int) -> dict:
    return {"vision": {"image": 224, "patch": patch, "hidden": 768, "layers": 12, "heads": 12, "ffn": 3072},
            "text": {"vocab": 49408, "positions": 77, "hidden": 512, "layers": 12, "heads": 8, "ffn": 2048},
            "projection": 512, "ln_eps": 1e-5, "act": "quick_gelu", "eos_token_id": 49407}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "clip.json"))
    args = ap.parse_args()

    import torch

    import clip_oracle as co
    from eioku_amd import _lib, visual

    _lib.init()
    gen = torch.Generator(device="cuda").manual_seed(1)
    frames = torch.randint(0, 256, (FRAMES, args.height, args.width, 3), dtype=torch.uint8, device="cuda", generator=gen)
    rng = np.random.default_rng(2)
    ids = np.full((FRAMES, 77), 49407, np.int32)
    ids[:, 0] = 49406
    ids[:, 1:9] = rng.integers(0, 49000, (FRAMES, 8))
    models = {}
    for name, patch in (("vit-b-32", 32), ("vit-b-16", 16)):
        cfg = config(patch)
        hf = co.hf_config(cfg)
        state = visual.random_state(hf, 5)
        clip = visual.ClipModel(state, hf)
        row = {"images": {}, "text": {}}
        for per_call in (1, FRAMES):
            calls = [frames[i:i + per_call] for i in range(0, FRAMES, per_call)]
            clip.encode_images(calls[0])  # warm-up: workspaces, tables
            torch.cuda.synchronize()
            best = {}
            for _ in range(args.reps):
                t = time.perf_counter()
                for c in calls:
                    clip.encode_images(c)
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t) * 1e3
                for k, v in {"wall_ms_64_frames": wall, **{f"{k}_device_ms_per_call": v for k, v in clip.last_ms().items()}}.items():
                    best[k] = min(best.get(k, v), v)
            flops = clip.last_flops()
            enc = best["encoder_device_ms_per_call"]
            row["images"][str(per_call)] = {**{k: round(v, 3) for k, v in best.items()},
                                            "images_per_second": round(FRAMES / best["wall_ms_64_frames"] * 1e3, 1),
                                            "gflop_per_image": round(flops / per_call / 1e9, 2),
                                            "encoder_tflops": round(flops / enc / 1e9, 1),
                                            "encoder_frac_fp16_peak": round(flops / (enc * 1e-3) / PEAK_F16, 4)}
        for per_call in (1, FRAMES):
            calls = [ids[i:i + per_call] for i in range(0, FRAMES, per_call)]
            clip.encode_ids(calls[0])
            best = {}
            for _ in range(args.reps):
                t = time.perf_counter()
                for c in calls:
                    clip.encode_ids(c)
                wall = (time.perf_counter() - t) * 1e3
                for k, v in {"wall_ms_64_queries": wall, **{f"{k}_device_ms_per_call": v for k, v in clip.last_ms().items()}}.items():
                    best[k] = min(best.get(k, v), v)
            best.pop("preprocess_device_ms_per_call")
            row["text"][str(per_call)] = {**{k: round(v, 3) for k, v in best.items()},
                                          "queries_per_second": round(FRAMES / best["wall_ms_64_queries"] * 1e3, 1)}
        clip.close()
        # the CPU oracle, fp32: one image, one query
        oracle = co.Oracle(cfg, state, fp16=False)
        u8 = rng.integers(0, 256, (1, 224, 224, 3), dtype=np.uint8)
        x = co.patch_rows(co.normalise(u8), patch)
        cpu = {}
        for what, run in (("image", lambda: oracle.vision(x)), ("query", lambda: oracle.text(ids[:1], 10))):
            run()
            t = time.perf_counter()
            run()
            cpu[f"seconds_per_{what}"] = round(time.perf_counter() - t, 4)
        row["cpu_oracle"] = {"threads": torch.get_num_threads(), **cpu}
        models[name] = row

    result = {"what": "tools/clip_bench.py on one MI355X: CLIP ViT-B/32 and ViT-B/16 (Hugging Face CLIPModel layout, 12 + 12 layers, "
                      f"projection 512), seeded weights; images: {FRAMES} BGR frames of {args.height} x {args.width} already on the "
                      "device, embedded 1 and 64 per call, vectors left on the device; text: 64 queries of 8 tokens (10 positions "
                      "run), ids on the host in, vectors on the host out; wall ms around the calls, device ms of the last call from "
                      f"the library's events (best of {args.reps} after a warm-up); the CPU figures are tests/clip_oracle.py (torch "
                      "fp32) on the same machine, preprocessing and tokenising not included; no number is an acceptance bar",
              "device": _lib.device_info(), "reps": args.reps, "models": models}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
