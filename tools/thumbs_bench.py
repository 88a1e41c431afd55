"""thumbnail_generation cost on one GPU: 64 synthetic 1080p frames already in HBM -> 320 x 180 JPEGs at quality 75,
written to ``profiles/thumbs.json``.

Device time is split by the library's own events into resize (K18a), block stage (K18b), entropy stage (K18c) and the
bitstream's trip back to the host; the wall time of ``ThumbnailEncoder.encode`` (tables, launches, host padding /
stuffing / markers) and the bytes returned are reported beside it.  The CPU path on the same box is what the device path
replaces: the frames' D2H copy, then per frame BGR -> RGB, Pillow ``resize(BICUBIC)`` and ``save("JPEG")``; ``null`` when
Pillow is not importable.

    python tools/thumbs_bench.py [--reps 5] [--frames 64] [--out profiles/thumbs.json]
"""
import argparse
import io
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def frames_1080p(n: int, seed: int) -> np.ndarray:
    """Frame-like content: 8 x 8 blobs of random colour plus noise."""
    rng = np.random.default_rng(seed)
    blobs = rng.integers(0, 256, (n, 135, 240, 3))
    f = np.repeat(np.repeat(blobs, 8, 1), 8, 2) + rng.integers(-20, 21, (n, 1080, 1920, 3))
    return np.clip(f, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "thumbs.json"))
    args = ap.parse_args()
    import torch

    from eioku_amd import _lib, thumbs

    _lib.init()
    dev = torch.device("cuda", 0)
    host = frames_1080p(args.frames, 1)
    frames = torch.from_numpy(host).to(dev)
    enc = thumbs.ThumbnailEncoder((320, 180), 75)
    tw, th = thumbs.thumbnail_size(1920, 1080, enc.size)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t) * 1e3

    files = enc.encode(frames)  # warm-up: tables, buffers
    best: dict = {}
    for _ in range(args.reps):
        files, wall = timed(lambda: enc.encode(frames))
        row = {"encode_wall_ms": wall, **{f"device_{k}_ms": v for k, v in enc.last_ms().items()}}
        for k, v in row.items():
            best[k] = min(best.get(k, v), v)
    streams, nbits = enc.jpeg(enc.resize(frames, (tw, th)))
    result = {"frames": args.frames, "source": [1080, 1920], "thumbnail": [th, tw], "quality": 75, "reps": args.reps,
              **{k: round(v, 4) for k, v in best.items()},
              "device_total_ms": round(sum(v for k, v in best.items() if k.startswith("device_")), 4),
              "bitstream_bytes_returned": sum((b + 31) // 32 * 4 for b in nbits), "file_bytes": sum(len(f) for f in files),
              "frame_bytes_not_returned": int(host.nbytes)}

    cpu = None
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        cpu_best: dict = {}
        for _ in range(max(1, min(args.reps, 3))):
            back, t_d2h = timed(lambda: frames.cpu().numpy())
            t = time.perf_counter()
            cpu_files = []
            for f in back:
                buf = io.BytesIO()
                Image.fromarray(np.ascontiguousarray(f[..., ::-1])).resize((tw, th), Image.Resampling.BICUBIC).save(buf, "JPEG", quality=75)
                cpu_files.append(buf.getvalue())
            row = {"frame_d2h_ms": t_d2h, "pillow_resize_save_ms": (time.perf_counter() - t) * 1e3}
            for k, v in row.items():
                cpu_best[k] = min(cpu_best.get(k, v), v)
        cpu = {**{k: round(v, 3) for k, v in cpu_best.items()}, "total_ms": round(sum(cpu_best.values()), 3),
               "files_identical_to_device": cpu_files == files}
    result["cpu_path"] = cpu
    enc.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
