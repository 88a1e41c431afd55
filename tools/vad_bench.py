"""Voice activity (K22) cost on one GPU: one hour of 16 kHz noise (112 500 chunks of 512 samples, plus the padding chunk)
through ``SileroVad.speech_probs`` with seeded weights, written to ``profiles/vad.json``.

Device time is split by the library's own events into the batched stages (``k_vad_encode``: STFT, encoder, LSTM input
projection) and the recurrence (``k_vad_lstm``), summed over the slabs; the wall time of the call (staging the audio,
launches, the probabilities' trip back) is reported beside it.  Two slab sizes: the product default and one other.  For
scale, the greedy decode of one 30 s window at the ``base`` dimensions is read from ``profiles/whisper.json``; it is not
measured again here.

    python tools/vad_bench.py [--reps 3] [--seconds 3600] [--slabs 16384,2048] [--out profiles/vad.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--slabs", default="16384,2048")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vad.json"))
    args = ap.parse_args()

    from eioku_amd import _lib, vad

    _lib.init()
    rng = np.random.default_rng(1)
    audio = (0.1 * rng.standard_normal(args.seconds * vad.SAMPLE_RATE, dtype=np.float32)).astype(np.float32)
    chunks = vad.num_chunks(audio.size)
    runs = []
    reference = None
    for slab in (int(s) for s in args.slabs.split(",")):
        model = vad.SileroVad(vad.seeded_weights(3), slab_chunks=slab)
        probs = model.speech_probs(audio[:vad.WINDOW * 64])  # warm-up: code objects, buffers
        best: dict = {}
        for _ in range(args.reps):
            t = time.perf_counter()
            probs = model.speech_probs(audio)
            wall = (time.perf_counter() - t) * 1e3
            encode_ms, lstm_ms = model.last_ms()
            for k, v in (("call_wall_ms", wall), ("encode_device_ms", encode_ms), ("lstm_device_ms", lstm_ms)):
                best[k] = min(best.get(k, v), v)
        model.close()
        if reference is None:
            reference = probs
        runs.append({"slab_chunks": slab, "slabs": -(-chunks // slab), **{k: round(v, 3) for k, v in best.items()},
                     "lstm_us_per_step": round(best["lstm_device_ms"] * 1e3 / chunks, 4),
                     "encode_us_per_chunk": round(best["encode_device_ms"] * 1e3 / chunks, 4),
                     "probs_bit_identical_to_first_slab_size": bool(np.array_equal(probs.view(np.uint32), reference.view(np.uint32))),
                     "probs_min_max": [float(probs.min()), float(probs.max())]})

    scale = None
    whisper_profile = ROOT / "profiles" / "whisper.json"
    if whisper_profile.exists():
        for shape in json.loads(whisper_profile.read_text()).get("shapes", []):
            wa = shape.get("word_alignment") or {}
            if shape.get("shape") == "base" and "greedy_decode_ms" in wa:
                scale = {"source": "profiles/whisper.json, shape base, word_alignment.greedy_decode_ms",
                         "greedy_decode_ms_one_window": wa["greedy_decode_ms"], "greedy_decode_steps": wa["greedy_decode_steps"]}
    result = {"what": "tools/vad_bench.py on one MI355X: seeded weights, noise; device ms from the library's events, wall ms around "
                      f"the synchronous call (best of {args.reps} after a warm-up); no number is an acceptance bar",
              "device": _lib.device_info(), "audio_seconds": args.seconds, "chunks": chunks, "reps": args.reps, "runs": runs,
              "whisper_base_for_scale": scale}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
