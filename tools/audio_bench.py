"""Audio front end (K23) cost on one GPU: one hour of 48 kHz and one hour of 44.1 kHz stereo 16-bit PCM (seeded noise)
through ``AudioFrontEnd.resample``, written to ``profiles/audio.json``.

Per rate: the kernel time from the library's own events, summed over the slabs; the wall time of the synchronous call
(staging the PCM to the device slab by slab, the kernels, the samples' trip back); the bytes the kernel has to move (PCM in,
fp32 out) and the rate they give over the kernel time; and, on the same machine's CPU, the same work done by
``scipy.signal.resample_poly`` after a numpy decode and downmix (the numpy oracle of tests/audio_oracle.py where scipy is
absent; the file says which).  The device result is compared with the CPU one over the first and last seconds.

    python tools/audio_bench.py [--reps 3] [--seconds 3600] [--out profiles/audio.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "audio.json"))
    args = ap.parse_args()

    from eioku_amd import _lib, audio

    try:
        from scipy.signal import resample_poly
        cpu_name = "scipy.signal.resample_poly on float32 mono, after a numpy decode and downmix"
    except ImportError:
        resample_poly = None
        cpu_name = "tests/audio_oracle.py (numpy fp32 loop over the taps), after a numpy decode and downmix; scipy is absent"
    import audio_oracle as ao

    _lib.init()
    fe = audio.AudioFrontEnd()
    runs = []
    for rate in (48000, 44100):
        up, down = audio.resample_ratio(rate)
        frames = args.seconds * rate
        pcm = np.random.default_rng(rate).integers(-32768, 32768, 2 * frames, dtype=np.int16)
        fe.resample(pcm[:2 * rate], "s16", 2, rate)      # warm-up: code object, handle, bank
        fe.resample(pcm, "s16", 2, rate)                 # and the full-size buffers
        best: dict = {}
        for _ in range(args.reps):
            t = time.perf_counter()
            out = fe.resample(pcm, "s16", 2, rate)
            wall = (time.perf_counter() - t) * 1e3
            for k, v in (("call_wall_ms", wall), ("kernel_ms", fe.last_ms())):
                best[k] = min(best.get(k, v), v)
        t = time.perf_counter()
        mono = ao.decode(pcm, "s16", 2)
        decode_ms = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        cpu = resample_poly(mono, up, down) if resample_poly else ao.resample(mono, rate)
        cpu_ms = (time.perf_counter() - t) * 1e3
        edge = 16000
        diff = max(float(np.abs(out[:edge].astype(np.float64) - cpu[:edge]).max()),
                   float(np.abs(out[-edge:].astype(np.float64) - cpu[-edge:]).max()))
        moved = pcm.nbytes + out.nbytes
        runs.append({"rate": rate, "channels": 2, "format": "s16", "up": up, "down": down,
                     "taps_per_phase": int(audio.filter_bank(rate).shape[1]), "frames": frames, "samples_out": int(out.size),
                     "slabs": len(audio.plan_slabs(frames, rate, fe.slab_out)),
                     "kernel_ms": round(best["kernel_ms"], 3), "call_wall_ms": round(best["call_wall_ms"], 3),
                     "bytes_in": int(pcm.nbytes), "bytes_out": int(out.nbytes),
                     "kernel_gb_per_s": round(moved / best["kernel_ms"] / 1e6, 1),
                     "cpu_decode_downmix_ms": round(decode_ms, 1), "cpu_resample_ms": round(cpu_ms, 1),
                     "largest_difference_from_cpu_first_and_last_second": diff})
        del pcm, out, mono, cpu
    fe.close()
    result = {"what": "tools/audio_bench.py on one MI355X: seeded full-scale noise; kernel ms from the library's events, wall ms "
                      f"around the synchronous call from pageable host memory (best of {args.reps} after two warm-up calls); the CPU "
                      "figures are single runs on the same machine; no number is an acceptance bar",
              "device": _lib.device_info(), "audio_seconds": args.seconds, "reps": args.reps, "slab_out": audio.DEFAULT_SLAB_OUT,
              "cpu_reference": cpu_name, "runs": runs}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
