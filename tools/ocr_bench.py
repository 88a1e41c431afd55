"""OCR throughput on one GPU, as one JSON object, with seeded random weights of the real shapes: K15 CRAFT milliseconds per
frame at 640 x 480, 1080p and 4K (the resize path), device time of score_maps on frames already on the device, with
FLOPs from ``last_flops`` and the fraction of the fp16 MFMA dense peak (2.5 PFLOP/s); K16 recogniser crops/s at padded
widths 128 / 256 / 512 (batches of 64 crops); the host post-processing (boxes + crops) ms per frame on 1080p maps.

    python tools/ocr_bench.py [--reps 5]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

PEAK_F16 = 2.5e15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch

    from eioku_amd import ocr
    from eioku_amd.synth import ocr_crops as crops, ocr_frames as frames

    r = ocr.OcrReader(ocr.random_craft_state(5), ocr.random_crnn_state(6))
    out = {"device": torch.cuda.get_device_name(0), "craft": {}, "crnn": {}}
    for name, (h, w) in {"480p": (480, 640), "1080p": (1080, 1920), "4k": (2160, 3840)}.items():
        f = torch.from_numpy(frames(1, 1, h, w)).cuda()
        r.score_maps(f)
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r.score_maps(f)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ms = 1e3 * float(np.median(ts))
        fl = r.last_flops()[0]
        out["craft"][name] = {"ms_per_frame": round(ms, 3), "gflop": round(fl / 1e9, 1), "tflops": round(fl / ms / 1e9, 1),
                              "frac_fp16_peak": round(fl / (ms * 1e-3) / PEAK_F16, 3)}
    for wdt in (128, 256, 512):
        imgs = crops(wdt, [wdt] * 64)
        r.recognize_raw(imgs)
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r.recognize_raw(imgs)
            ts.append(time.perf_counter() - t0)
        s = float(np.median(ts))
        out["crnn"][f"w{wdt}"] = {"crops_per_s": round(64 / s, 1), "ms_per_64": round(1e3 * s, 3),
                                  "gflop_per_crop": round(r.last_flops()[1] / 64 / 1e9, 3)}
    f = frames(3, 1, 1080, 1920)
    t, l, _ = r.score_maps(f)
    t, l = t.cpu().numpy()[0], l.cpu().numpy()[0]
    bias = (0.75 - float(np.quantile(t, 0.995)), 0.45 - float(np.quantile(l, 0.98)))  # components that clear the thresholds
    grey = ocr.bgr_to_gray(f[0])
    t0 = time.perf_counter()
    hl, fl = ocr.boxes_from_maps(t + bias[0], l + bias[1], 1.0)
    t1 = time.perf_counter()
    items = ocr.image_list(hl, fl, grey)
    prep = [ocr.align_collate(c, wdt) for _, c, wdt in items]
    t2 = time.perf_counter()
    out["host_1080p"] = {"boxes": len(items), "post_ms": round(1e3 * (t1 - t0), 2), "crop_prep_ms": round(1e3 * (t2 - t1), 2),
                         "crops": len(prep)}
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
