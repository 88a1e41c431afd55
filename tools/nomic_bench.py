"""nomic-embed-text (K27) cost on one GPU: the base configuration (768 wide, 12 layers, 12 heads, ffn 3072, vocab 30528) with
seeded weights, written to ``profiles/nomic.json``.

Shapes: 512 texts of 128 tokens (the token count K8's 7.2 ms in README.md is for), 8 texts of 2048, and a seeded ragged batch
of 512 texts whose lengths are log-normal between 3 and 2048, run once packed (``encode_packed``, ids and cu on the device) and
once as the padded rectangle a tokenizer hands over (``encode_ids``, which packs on the device).  Per shape: the device time
from the library's own events (``last_ms``, first kernel to pooled vectors), the wall time around the call, tokens per second
from the device time, and the achieved TFLOP/s from ``last_flops``.  The comparison is ``tests/nomic_oracle.py``'s torch-CPU fp32
forward on this machine's threads (``--threads``, 16) over a smaller sample.  These are records, not acceptance bars.

    python tools/nomic_bench.py [--reps 5] [--out profiles/nomic.json]
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


def ragged_lengths(n: int, seed: int) -> np.ndarray:
    """log-normal with median 40 tokens (a transcript segment) and sigma 1.2, clipped to [3, 2048]; one text is the whole
    document at 2048"""
    lengths = np.clip(np.exp(np.random.default_rng(seed).normal(np.log(40.0), 1.2, n)), 3, 2048).astype(np.int64)
    lengths[0] = 2048
    return lengths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "nomic.json"))
    args = ap.parse_args()

    import torch

    import nomic_oracle as no
    from eioku_amd import _lib, embed

    _lib.init()
    cfg = embed.NOMIC_EMBED_TEXT_V1_5
    state = embed.nomic_random_state(cfg, 5)
    enc = embed.NomicEncoder(state, cfg, matryoshka_dim=512)
    rng = np.random.default_rng(2)

    def batch(lengths):
        seqs = [rng.integers(1, cfg["vocab"], int(n)).astype(np.int32) for n in lengths]
        return seqs, no.pack(seqs)

    def measure(call, tokens):
        call()  # warm-up: workspaces
        torch.cuda.synchronize()
        dev_ms, wall_ms = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            call()
            torch.cuda.synchronize()
            wall_ms.append((time.perf_counter() - t) * 1e3)
            dev_ms.append(enc.last_ms())
        d = min(dev_ms)
        return {"tokens": int(tokens), "device_ms": round(d, 3), "wall_ms": round(min(wall_ms), 3), "tokens_per_second": round(tokens / d * 1e3),
                "gflop": round(enc.last_flops() / 1e9, 1), "tflops": round(enc.last_flops() / d / 1e9, 1)}

    shapes = {}
    for name, lengths in (("512x128", [128] * 512), ("8x2048", [2048] * 8), ("ragged_512", ragged_lengths(512, 7))):
        seqs, (ids, cu) = batch(lengths)
        d_ids, d_cu = torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda()
        row = {"texts": len(seqs), "longest": int(max(lengths)), "packed": measure(lambda: enc.encode_packed(d_ids, d_cu), len(ids))}
        if name.startswith("ragged"):
            p_ids, p_mask = (torch.from_numpy(a).cuda() for a in no.pad(seqs))
            row["padded_rectangle_through_encode_ids"] = {"rectangle_tokens": int(p_ids.numel()),
                                                          **measure(lambda: enc.encode_ids(p_ids, p_mask), len(ids))}
        shapes[name] = row
        print(name, json.dumps(row), flush=True)
    enc.close()

    # the torch-CPU fp32 oracle over a sample: 32 texts of 128 tokens, and one of 2048
    torch.set_num_threads(args.threads)
    o32 = no.Oracle(cfg, state, False)
    oracle = {}
    for name, lengths in (("32x128", [128] * 32), ("1x2048", [2048])):
        seqs, _ = batch(lengths)
        o32.encode(seqs[:1], 512)
        t = time.perf_counter()
        o32.encode(seqs, 512)
        s = time.perf_counter() - t
        oracle[name] = {"tokens": int(sum(lengths)), "seconds": round(s, 3), "tokens_per_second": round(sum(lengths) / s)}
        print("oracle", name, json.dumps(oracle[name]), flush=True)
    out = {"device": _lib.device_info()["name"], "config": cfg, "matryoshka_dim": 512, "reps": args.reps, "shapes": shapes,
           "torch_cpu_fp32_oracle": {"threads": args.threads, **oracle},
           "note": "seeded weights; device_ms is the library's own event pair (first kernel to pooled vectors), wall_ms includes the "
                   "read-back of ids / cu that validates them and sizes the launches; best of reps"}
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
