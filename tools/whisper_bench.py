#!/usr/bin/env python
"""Whisper on the HIP path: device time of the log-mel front end, the encoder and a decoder step, with seeded weights.

    python tools/whisper_bench.py [--shapes base small] [--windows 64] [--out profiles/whisper.json]
    python tools/whisper_bench.py --beam 5 [--shapes base]      # adds a beam block to the shapes already in --out
    python tools/whisper_bench.py --prompted [--shapes base]    # adds a prompted block (K20c) in the same way
    python tools/whisper_bench.py --align [--shapes base]       # adds a word-alignment block (K21) in the same way

For each shape (the openai `base` and `small` dimensions, vocabulary 51865, ctx 1500): log-mel over `--windows` windows of
30 s, the encoder per window at batch 8, a decoder step at B = 1, 8 and 32 (greedy, 32 sampled tokens, lanes never end
early with random weights unless EOT wins), kernel launches per step, and the CPU oracle (tests/whisper_oracle.py, fp32,
torch-CPU) on the same box for one window and a few steps.  Calls are synchronous, so wall-clock time around them is device
time plus one launch-queue drain.  No number here is an acceptance bar.

`--beam W` measures beam search only (K20b): a decoder step and the launches per step at B = 1 and 8 windows (W lanes each),
with the greedy step of the same run next to it, and merges the block into the shape's row of `--out`, leaving the rest.

`--prompted` measures K20c only: a 227-token prompt (``<|startofprev|>`` + 223 previous tokens + 3) through the one-pass
prefill (`decode_prompted`, one new token) against the same prompt walked position by position by `decode` with one new
token, at 1 and 8 windows; and a sampled step (temperature 1) against a greedy step of the same entry at 8 lanes.

`--align` measures K21 only: one 30 s window with 224 text tokens (F = 1500 frames, the default alignment heads) through
`align`: the device time (hipEvent) of the teacher-forced pass with the token probabilities, of the cost kernels and of the
DTW, the wall-clock time of the whole call, and next to them the greedy decode of 224 tokens on the same window.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

SHAPES = {"base": (512, 8, 6, 2048), "small": (768, 12, 12, 3072)}


def dims_for(name: str) -> dict:
    d, heads, layers, ffn = SHAPES[name]
    return {"n_mels": 80, "d_model": d, "heads": heads, "enc_layers": layers, "dec_layers": layers, "enc_ffn": ffn, "dec_ffn": ffn,
            "vocab": 51865, "max_source_positions": 1500, "max_target_positions": 448, "sot": 50258, "eot": 50257,
            "transcribe": 50359, "translate": 50358, "no_speech": 50362, "no_timestamps": 50363, "timestamp_begin": 50364,
            "max_initial_timestamp_index": 50, "suppress": [50258, 50358, 50359, 50360, 50361, 50362],
            "begin_suppress": [220, 50257], "lang_ids": list(range(50259, 50358)), "lang_codes": [f"l{i}" for i in range(99)]}


def timed(fn, reps: int = 3) -> float:
    fn()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def beam_block(t, dims: dict, audio: np.ndarray, beam: int, steps: int) -> dict:
    prompt = [dims["sot"], dims["lang_ids"][0], dims["transcribe"]]
    t.set_audio(audio)
    block = {"beam": beam, "patience": 1.0, "sampled_tokens": steps}
    for b in (1, 8):
        t.logmel([i * 480000 for i in range(b)], fetch=False)
        t.encode(b)
        ms = timed(lambda: t.decode_beam(prompt, b, steps, beam, sync_every=steps))
        launches, n = t.last_launches()
        block[f"decode_ms_per_step_b{b}"] = ms / n
        block[f"decode_steps_b{b}"] = n
        block[f"launches_per_step_b{b}"] = launches / n
        ms = timed(lambda: t.decode(prompt, b, steps, sync_every=steps))
        launches, n = t.last_launches()
        block[f"greedy_ms_per_step_b{b}"] = ms / n
        block[f"greedy_launches_per_step_b{b}"] = launches / n
    return block


def prompted_block(t, dims: dict, audio: np.ndarray, steps: int) -> dict:
    base = [dims["sot"], dims["lang_ids"][0], dims["transcribe"]]
    rng = np.random.default_rng(2)
    long = [dims["no_speech"] - 1] + [int(v) for v in rng.integers(1000, 40000, size=223)] + base
    t.set_audio(audio)
    block = {"prompt_tokens": len(long), "sampled_tokens": steps}
    for b in (1, 8):
        t.logmel([i * 480000 for i in range(b)], fetch=False)
        t.encode(b)
        block[f"prefill_prompt_ms_b{b}"] = timed(lambda: t.decode_prompted([long] * b, len(long) - 3, 1))
        block[f"prefill_launches_b{b}"] = t.last_launches()[0]
        block[f"walked_prompt_ms_b{b}"] = timed(lambda: t.decode(long, b, 1))
        block[f"walked_launches_b{b}"] = t.last_launches()[0]
    seeds = np.arange(1, 9, dtype=np.uint64).reshape(8, 1)
    ms = timed(lambda: t.decode_prompted([base] * 8, 0, steps, sync_every=steps))
    block["greedy_ms_per_token_b8"] = ms / steps
    ms = timed(lambda: t.decode_prompted([base] * 8, 0, steps, temperature=1.0, seeds=seeds, sync_every=steps))
    block["sampled_ms_per_token_b8"] = ms / steps
    return block


def align_block(t, dims: dict, audio: np.ndarray, n_text: int = 224) -> dict:
    base = [dims["sot"], dims["lang_ids"][0], dims["transcribe"]]
    rng = np.random.default_rng(3)
    seq = base + [dims["no_timestamps"]] + [int(v) for v in rng.integers(1000, 40000, size=n_text)] + [dims["eot"]]
    t.set_audio(audio)
    t.logmel([0], fetch=False)
    t.encode(1)
    block = {"windows": 1, "text_tokens": n_text, "frames": dims["max_source_positions"],
             "alignment_heads": dims["dec_layers"] - dims["dec_layers"] // 2, "heads_per_layer": dims["heads"]}
    parts = []

    def run():
        t.align([seq], [len(seq)], len(base), [2 * dims["max_source_positions"]])
        parts.append(t.last_align_ms())

    block["align_call_ms"] = timed(run)
    best = min(parts[1:], key=sum)
    block["pass_device_ms"], block["cost_device_ms"], block["dtw_device_ms"] = best
    block["align_launches"] = t.last_launches()[0]
    ms = timed(lambda: t.decode(base, 1, n_text, sync_every=n_text))
    block["greedy_decode_ms"] = ms
    block["greedy_decode_steps"] = t.last_launches()[1]
    return block


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["base", "small"], choices=sorted(SHAPES))
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--beam", type=int, default=0, help="measure beam search at this beam size and merge it into --out")
    ap.add_argument("--prompted", action="store_true", help="measure the prompt prefill and the sampled step and merge them into --out")
    ap.add_argument("--align", action="store_true", help="measure the word alignment (K21) and merge it into --out")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "whisper.json"))
    args = ap.parse_args()

    from eioku_amd import _lib
    from eioku_amd.transcribe import WhisperTranscriber, seeded_weights

    info = _lib.device_info()
    rng = np.random.default_rng(0)
    if args.beam or args.prompted or args.align:
        out = Path(args.out)
        result = json.loads(out.read_text()) if out.exists() else {"what": "tools/whisper_bench.py --beam", "device": info, "shapes": []}
        audio = (0.1 * rng.standard_normal(8 * 480000)).astype(np.float32)
        for name in args.shapes:
            dims = dims_for(name)
            t = WhisperTranscriber(dims, seeded_weights(dims, 1))
            key = "beam_search" if args.beam else ("prompted" if args.prompted else "word_alignment")
            if args.align:
                block = align_block(t, dims, audio)
            else:
                block = beam_block(t, dims, audio, args.beam, args.steps) if args.beam else prompted_block(t, dims, audio, args.steps)
            t.close()
            print(json.dumps({"shape": name, **block}))
            rows = [r for r in result["shapes"] if r.get("shape") == name]
            if not rows:
                rows = [{"shape": name, "d_model": dims["d_model"], "layers": dims["enc_layers"]}]
                result["shapes"].append(rows[0])
            rows[0][key] = block
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(result, indent=1) + "\n")
        print("wrote", args.out)
        return
    audio = (0.1 * rng.standard_normal(args.windows * 480000)).astype(np.float32)
    result = {"what": "tools/whisper_bench.py on one MI355X: seeded weights, wall-clock ms around synchronous calls (best of 3 "
                      "after a warm-up); no number is an acceptance bar", "device": info, "windows": args.windows, "shapes": []}
    for name in args.shapes:
        dims = dims_for(name)
        t = WhisperTranscriber(dims, seeded_weights(dims, 1))
        t.set_audio(audio)
        row = {"shape": name, "d_model": dims["d_model"], "layers": dims["enc_layers"]}
        offsets = [i * 480000 for i in range(args.windows)]
        row["logmel_ms_per_window"] = timed(lambda: [t.logmel(offsets[i:i + 8], fetch=False) for i in range(0, len(offsets), 8)]) / args.windows
        t.logmel(offsets[:8], fetch=False)
        row["encoder_ms_per_window_b8"] = timed(lambda: t.encode(8)) / 8
        row["encoder_tflops_b8"] = t.last_flops() / (row["encoder_ms_per_window_b8"] * 8 * 1e-3) / 1e12
        prompt = [dims["sot"], dims["lang_ids"][0], dims["transcribe"]]
        for b in (1, 8, 32):
            t.logmel(offsets[:b], fetch=False)
            t.encode(b)
            holder = {}

            def run():
                holder["res"] = t.decode(prompt, b, args.steps, sync_every=args.steps)

            ms = timed(run)
            launches, steps = t.last_launches()
            row[f"decode_ms_per_step_b{b}"] = ms / steps
            row[f"decode_steps_b{b}"] = steps
            row["launches_per_step"] = launches / steps
        if not args.no_cpu:
            import torch
            import whisper_oracle as wo

            weights = {}
            make = seeded_weights(dims, 1)
            for n, rows, cols in t._h.tensors():
                arr = torch.from_numpy(make(n, rows, cols).copy())
                if "conv" in n and n.endswith(".weight"):
                    arr = arr.view(rows, cols // 3, 3)
                elif not (n.endswith(".bias") or "layer_norm" in n):
                    arr = arr.view(rows, cols)
                weights[n] = arr
            oracle = wo.Oracle(dims, weights, fp16=False)
            mel = wo.log_mel(audio, 0, 3000, 80)[None]
            t0 = time.perf_counter()
            wo.log_mel(audio, 0, 3000, 80)
            row["cpu_logmel_ms_per_window"] = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            enc = oracle.encode(mel)
            row["cpu_encoder_ms_per_window"] = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            oracle.greedy(enc, prompt, 4)
            row["cpu_decode_ms_per_step_b1"] = (time.perf_counter() - t0) * 1e3 / 4
            row["cpu_threads"] = torch.get_num_threads()
        t.close()
        print(json.dumps(row))
        result["shapes"].append(row)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
