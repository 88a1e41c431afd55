"""Motion-JPEG decode (K28) measured: 64 frames of 1080p at quality 75 and 90, 4:2:0 and 4:2:2, with and without restart
intervals, for subsequence sizes S in {256, 512, 1024, 2048} -> profiles/mjpeg.json.

Per configuration and S: device milliseconds per stage and synchronisation rounds (``MjpegDecoder.last``), and frames per
second of the whole ``decode`` call (host marker parsing and packing included, the result left in HBM).  Next to them:
Pillow (libjpeg-turbo) decoding the same bytes on 16 threads of the same machine, and ``cv2.imdecode`` where cv2 exists.

The inputs are synthetic frames (gradients, rectangles, texture) encoded with Pillow: ``--distinct`` different frames per
configuration, repeated to ``--frames``.  ``--make-inputs`` writes them to ``--inputs`` and stops, for a machine without
Pillow: the file is then read instead of being generated.

    python tools/mjpeg_bench.py [--frames 64] [--inputs build/mjpeg_bench_inputs.npz] [--out profiles/mjpeg.json]
"""
from __future__ import annotations

import argparse
import io
import json
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

H, W = 1080, 1920
CONFIGS = [(q, s, r) for q in (75, 90) for s in ("420", "422") for r in (False, True)]
SIZES = (256, 512, 1024, 2048)


def config_name(q, s, r):
    return f"q{q}-{s}-{'rst' if r else 'norst'}"


def synthetic_frame(seed: int) -> np.ndarray:
    """A frame with the statistics of camera footage rather than of noise: smooth shading, hard edges, some texture."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([128 + 90 * np.sin(xx / (150 + 20 * seed) + c) * np.cos(yy / (110 + 10 * c)) for c in range(3)], -1)
    for _ in range(40):
        x0, y0 = int(rng.integers(0, W - 64)), int(rng.integers(0, H - 64))
        w, h = int(rng.integers(32, 480)), int(rng.integers(32, 320))
        img[y0:y0 + h, x0:x0 + w] = 0.5 * img[y0:y0 + h, x0:x0 + w] + 0.5 * rng.integers(0, 256, 3)
    img += rng.normal(0, 6, (H, W, 1)).astype(np.float32) + rng.normal(0, 2, (H, W, 3)).astype(np.float32)
    return np.clip(img, 0, 255).astype(np.uint8)


def make_inputs(distinct: int) -> dict:
    from PIL import Image

    frames = [Image.fromarray(synthetic_frame(i)) for i in range(distinct)]
    out = {}
    for q, s, r in CONFIGS:
        for i, im in enumerate(frames):
            buf = io.BytesIO()
            im.save(buf, "JPEG", quality=q, subsampling={"420": 2, "422": 1}[s], **({"restart_marker_rows": 1} if r else {}))
            out[f"{config_name(q, s, r)}/{i}"] = np.frombuffer(buf.getvalue(), np.uint8)
    return out


def best_of(fn, repeats: int = 3) -> float:
    fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--inputs", default=str(ROOT / "build" / "mjpeg_bench_inputs.npz"))
    ap.add_argument("--make-inputs", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mjpeg.json"))
    args = ap.parse_args()

    inputs = Path(args.inputs)
    if args.make_inputs or not inputs.exists():
        inputs.parent.mkdir(parents=True, exist_ok=True)
        np.savez(inputs, **make_inputs(args.distinct))
        if args.make_inputs:
            print(f"{inputs}: {inputs.stat().st_size} bytes")
            return
    with np.load(inputs) as z:
        data = {k: z[k].tobytes() for k in z.files}

    import torch

    from eioku_amd import _lib
    from eioku_amd.mjpeg import MjpegDecoder

    try:
        from PIL import Image
    except ImportError:
        Image = None
    try:
        import cv2
    except ImportError:
        cv2 = None

    _lib.init(0)
    result = {"device": _lib.device_info()["name"], "frames": args.frames, "height": H, "width": W, "cpu_threads": 16, "configs": {}}
    pool = ThreadPoolExecutor(16)
    for q, s, r in CONFIGS:
        name = config_name(q, s, r)
        distinct = [data[k] for k in sorted(data) if k.startswith(name + "/")]
        files = [distinct[i % len(distinct)] for i in range(args.frames)]
        row = {"distinct_frames": len(distinct), "bytes_per_frame": int(np.mean([len(f) for f in files])), "S": {}}
        dec = MjpegDecoder()
        for bits in SIZES:
            dec.set_subseq_bits(bits)

            def call():
                dec.decode(files, "bgr")
                torch.cuda.synchronize()

            sec = best_of(call)
            row["S"][str(bits)] = {**{k: round(v, 3) if isinstance(v, float) else v for k, v in dec.last().items()},
                                   "wall_ms": round(sec * 1e3, 2), "frames_per_s": round(args.frames / sec, 1)}
        dec.close()
        if Image is not None:
            sec = best_of(lambda: list(pool.map(lambda f: np.asarray(Image.open(io.BytesIO(f)).convert("RGB")), files)))
            row["pillow_16_threads"] = {"wall_ms": round(sec * 1e3, 2), "frames_per_s": round(args.frames / sec, 1)}
        if cv2 is not None:
            sec = best_of(lambda: list(pool.map(lambda f: cv2.imdecode(np.frombuffer(f, np.uint8), cv2.IMREAD_COLOR), files)))
            row["cv2_imdecode_16_threads"] = {"wall_ms": round(sec * 1e3, 2), "frames_per_s": round(args.frames / sec, 1)}
        result["configs"][name] = row
        print(name, json.dumps(row), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
