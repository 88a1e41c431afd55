"""Fixtures shared by tests/test_whisper_beam_host.py (CPU) and tests/test_whisper_beam_gpu.py: the beam-search test model,
the windows of the parity cases, and the scripted one-step cases.

The model is model A of tests/whisper_oracle.py with the q / k projections scaled back by 1 / 4.  ``random_weights`` scales
them by 4, which makes the softmaxes so sharp that one flipped fp16 rounding moves a logit by up to 0.2 (DESIGN.md "K19 /
K20"); a beam step's margin is the smallest of W or more gaps between adjacent candidates and is a few 1e-2 at best, so on
the sharp model no window of 400 reaches eight compared steps at W = 5.  With the projections at He scale the fp16 oracle's
drift against the fp32 oracle falls from 6e-2 to 4e-3 (median of the per-position maximum) and the margin rule has steps
to compare.  The windows below were picked on the CPU alone: beam steps whose margin exceeds 4 x that fp16-against-fp32
drift, which is about twice the drift the device shows against the fp16 oracle (2.0e-3 at the median, 3.1e-3 at the worst
step, measured by tests/test_whisper_beam_gpu.py).
"""
from __future__ import annotations

import numpy as np

import whisper_beam_oracle as wb
import whisper_oracle as wo

NEW_TOKENS = 24
MODEL_SEED = 5
BOOST = 1.2       # EOT and timestamp rows, as in tests/test_whisper_gpu.py
QK_SCALE = 0.25

# End to end against the oracle: (audio seed, max_new_tokens) of 2 s clips whose first window is a parity window cut to the
# steps the margin rule covers (the oracle's margins over those steps: 0.0105 and 0.0138 at the thinnest step).
E2E_CASES = ((376, 12), (203, 8))

# name -> (beam, audio seeds of the windows).  15 lanes, 15 lanes, and 20 lanes (past k_logits's 16-lane tile).
PARITY_CASES = {"w3_b3": (3, (33, 65, 121)), "w5_b3": (5, (203, 376, 355)), "w5_b4": (5, (27, 282, 355, 140))}


def audio(seed: int, seconds: float) -> np.ndarray:
    rng = np.random.default_rng(seed)
    t = np.arange(int(seconds * 16000)) / 16000.0
    x = sum(rng.uniform(0.05, 0.3) * np.sin(2 * np.pi * rng.uniform(80, 4000) * t + rng.uniform(0, 6)) for _ in range(6))
    return (x + 0.01 * rng.standard_normal(len(t))).astype(np.float32)


def model_a_weights(qk_scale: float = QK_SCALE) -> tuple[dict, dict]:
    """The beam fixture's model; ``qk_scale=1.0`` is model A exactly as tests/test_whisper_gpu.py builds it (the sharp model)."""
    cfg = wo.model_a_config()
    tb = cfg["timestamp_begin"]
    w = wo.random_weights(cfg, MODEL_SEED, {cfg["eot"]: BOOST, **{tb + i: BOOST for i in range(cfg["vocab"] - tb)}})
    for k in w:
        if k.endswith(("q_proj.weight", "q_proj.bias", "k_proj.weight")):
            w[k] = w[k] * qk_scale
    return cfg, w


def prompt_of(cfg: dict) -> list[int]:
    return [cfg["sot"], cfg["lang_ids"][0], cfg["transcribe"]]


def mel_of(cfg: dict, seeds) -> np.ndarray:
    return np.stack([wo.log_mel(audio(s, 2.0), 0, 2 * cfg["max_source_positions"], cfg["n_mels"]) for s in seeds])


def live_slots(step: dict) -> list[int]:
    return [j for j, s in enumerate(step["slots"]) if s["sum_logprob"] > wb.NEG_INF]


def fixture_report(results: list[dict], compared_steps: list[int]) -> dict:
    """What the parity fixture has to show inside the compared steps of its windows: windows with >= 8 compared steps, a
    compared step (after the first) whose sources are not the identity, and a hypothesis finishing on EOT."""
    forks = finishes = 0
    for r, n in zip(results, compared_steps):
        for i, st in enumerate(r["steps"][:n]):
            src = [s for s, _, _ in st["live"]]
            forks += i > 0 and src != list(range(len(src)))
            finishes += len(st["finished"])
    return {"windows_with_8": sum(n >= 8 for n in compared_steps), "forks": forks, "finishes": finishes}


# ---- one beam step on supplied logits -------------------------------------------------------------------------------------
def select_case(cfg: dict, W: int, patience: float = 1.0) -> dict:
    """Two windows of W slots.  Prefixes: the scripted prefixes mixed across the slots of a window; logits:
    ``scripted_logits`` with both timestamp shifts; one dead slot per window; EOT raised on two slots per window so that EOT
    candidates are walked; the finished counts are 0 and C - 1 (the second window can take only one more)."""
    C = wb.finish_count(W, patience)
    prefixes_all = list(wo.scripted_prefixes(cfg).values())
    rng = np.random.default_rng(1000 + W)
    L = 2 * W
    prefixes = [prefixes_all[(i + 1 + i // W) % len(prefixes_all)] for i in range(L)]
    logits = np.stack([wo.scripted_logits(cfg, 300 + i, -4.0 if i % 2 else 6.0) for i in range(L)])
    sums = -rng.uniform(0.0, 3.0, L)
    sums[W - 1] = sums[W + 1] = wb.NEG_INF
    for i in (0, 1, W, W + 2):
        logits[i, cfg["eot"]] = 14.0
    return {"W": W, "C": C, "prefixes": prefixes, "logits": logits.astype(np.float32), "sums": sums.astype(np.float32),
            "fin_count": [0, C - 1]}


def select_reference(case: dict, cfg: dict) -> list[dict]:
    W = case["W"]
    return [wb.beam_step(case["logits"][b * W:(b + 1) * W].astype(np.float64), case["prefixes"][b * W:(b + 1) * W],
                         case["sums"][b * W:(b + 1) * W].astype(np.float64), case["fin_count"][b], cfg, W, case["C"])
            for b in range(len(case["fin_count"]))]


def tie_case(cfg: dict, W: int) -> dict:
    """One window.  Slots 0 and 1: the same prefix, sum and logits, so every score appears twice and goes to the lower
    slot first.  Slot 2: five equal values, at ids in three workgroups (20, 333, 700) and across a workgroup edge (63, 64):
    they are walked in id order, 20, 63, 64, 333, 700."""
    tb = cfg["timestamp_begin"]
    prefix = [tb + 3, 10, 11]
    z = np.full((W, cfg["vocab"]), -5.0, dtype=np.float32)
    z[0] = z[1] = wo.scripted_logits(cfg, 77, -4.0)
    z[2, [700, 20, 333, 64, 63]] = 2.0
    sums = np.full(W, wb.NEG_INF, dtype=np.float32)
    sums[:3] = [-1.0, -1.0, -0.25]
    return {"W": W, "C": W, "prefixes": [prefix] * W, "logits": z, "sums": sums, "fin_count": [0]}


# ---- end to end -----------------------------------------------------------------------------------------------------------
def oracle_transcriber(cfg: dict, o16: wo.Oracle, log: list):
    """WhisperTranscriber's host loop over the CPU oracle's beam search instead of the device (the ``_OracleTranscriber``
    pattern of tests/test_whisper_gpu.py with ``decode_beam`` added); ``log`` collects (mel, oracle results, sample offsets) per decode."""
    from eioku_amd.transcribe import ByteDecoder, WhisperTranscriber

    frames = 2 * cfg["max_source_positions"]

    class T(WhisperTranscriber):
        def __init__(self):
            self.dims, self.decoder, self.window_frames, self.sync_every = dict(cfg), ByteDecoder({}), frames, 8

        def set_audio(self, samples):
            self._samples = samples

        def logmel(self, offsets, fetch=True):
            self._offsets = [int(o) for o in offsets]
            self._mel = np.stack([wo.log_mel(self._samples, o, frames, cfg["n_mels"]) for o in self._offsets])

        def encode(self, n, mel=None):
            self._enc = o16.encode(self._mel)

        def decode_beam(self, prompt, n_windows, max_new_tokens, beam_size, patience=1.0, sync_every=None, trace=False):
            rs = wb.beam_search(o16, self._enc, list(prompt), max_new_tokens, beam_size, patience)
            log.append((self._mel, rs, self._offsets))
            toks = np.full((n_windows, beam_size, max_new_tokens), cfg["eot"], dtype=np.int32)
            sums = np.full((n_windows, beam_size), -np.inf)
            for b, r in enumerate(rs):
                for h, hyp in enumerate(r["hyps"]):
                    toks[b, h, :len(hyp["tokens"])] = hyp["tokens"]
                    sums[b, h] = hyp["sum_logprob"]
            return {"tokens": toks, "sum_logprob": sums, "best": np.array([r["best"] for r in rs]),
                    "no_speech_prob": np.array([r["no_speech_prob"] for r in rs])}

        def close(self):
            pass

    return T()
