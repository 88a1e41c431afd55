"""CPU oracle for K20b (Whisper beam search): OpenAI Whisper's ``BeamSearchDecoder`` + ``MaximumLikelihoodRanker`` with
faster-whisper's parameters (``beam_size``, ``patience``, length penalty 1), restated on top of tests/whisper_oracle.py.

Per window: ``W`` slots, ``C = max(1, round(W * patience))`` finished hypotheses end the search.  At the first sampled step
only slot 0 is live (sum 0); a dead slot has the sum -inf and contributes nothing.  One step (``beam_step``):

1. per live slot j in slot order: z = rules 1-6 on its logits; if lse(z[timestamps]) > max(z[text]) the text ids go to -inf
   (rule 7); lp = z - lse(z);
2. the slot's candidates are its W + 1 largest finite lp entries (value descending, id ascending): (sum_j + lp[t], j, t);
3. all candidates sorted by score descending, then j, then t;
4. walk: a candidate with t == EOT is newly finished, any other becomes the next live slot (slot order = walk order,
   source slot j); stop when W live slots are filled;
5. the newly finished are appended, in walk order, to the window's finished list while it has fewer than C entries;
6. the window is complete when the list has C entries or no live slot is left.

After completion or the last step the live slots are appended, in slot order and with their sums as they are, while there
are fewer than W hypotheses.  Ranking: sum_logprob / max(1, tokens before EOT), the highest first, ties to the earlier one.

The margin of a step is the smallest gap a perturbation would have to close to change its outcome: the gaps between
adjacent candidates in the walked part of the sorted list plus the first unwalked one, and each live slot's rule-7 gap.
"""
from __future__ import annotations

import numpy as np
import torch

import whisper_oracle as wo

NEG_INF = float("-inf")


def finish_count(W: int, patience: float) -> int:
    return max(1, round(W * patience))


def beam_step(logits, prefixes, sums, n_finished: int, cfg: dict, W: int, C: int) -> dict:
    """Steps 1-6 on given logits [W][vocab].  ``prefixes[j]``: the tokens slot j has sampled; ``sums[j]``: its sum (-inf =
    dead); ``n_finished``: entries the window's finished list already has.  Returns ``live`` [(src, token, sum)], ``walked_eot``
    [(src, sum)] (every EOT candidate of the walk, in walk order), ``finished`` (the ones step 5 appends), ``fin_count``,
    ``complete`` and ``margin``."""
    tb, eot = cfg["timestamp_begin"], cfg["eot"]
    cands, gaps = [], []
    for j in range(W):
        if not sums[j] > NEG_INF:
            continue
        z = wo.apply_rules(logits[j], list(prefixes[j]), cfg)
        lse_ts, max_text = wo._lse(z[tb:]), z[:tb].max()
        if np.isfinite(lse_ts) and np.isfinite(max_text):
            gaps.append(abs(lse_ts - max_text))
        if lse_ts > max_text:
            z[:tb] = NEG_INF
        lp = z - wo._lse(z)
        ids = np.flatnonzero(np.isfinite(lp))
        ids = ids[np.lexsort((ids, -lp[ids]))][:W + 1]
        cands += [(float(sums[j]) + float(lp[t]), j, int(t)) for t in ids]
    cands.sort(key=lambda c: (-c[0], c[1], c[2]))
    live, walked_eot, walked = [], [], 0
    for score, j, t in cands:
        walked += 1
        if t == eot:
            walked_eot.append((j, score))
        else:
            live.append((j, t, score))
            if len(live) == W:
                break
    upto = min(walked + 1, len(cands))
    gaps += [cands[i][0] - cands[i + 1][0] for i in range(upto - 1)]
    finished = walked_eot[:max(0, C - n_finished)]
    fin_count = n_finished + len(finished)
    return {"live": live, "walked_eot": walked_eot, "finished": finished, "fin_count": fin_count,
            "complete": fin_count >= C or not live, "margin": float(min(gaps)) if gaps else float("inf")}


def rank(hyps: list[dict]) -> int:
    """Index of the best hypothesis: sum_logprob / max(1, tokens before EOT); the first of equals."""
    scores = [h["sum_logprob"] / max(1, len(h["tokens"])) for h in hyps]
    return int(np.argmax(scores))  # the first maximum


def finalize(finished: list[dict], slots: list[dict], W: int) -> list[dict]:
    hyps = [dict(h) for h in finished]
    for s in slots:
        if len(hyps) >= W:
            break
        if s["sum_logprob"] > NEG_INF:
            hyps.append({"tokens": list(s["tokens"]), "sum_logprob": s["sum_logprob"], "ended": False})
    return hyps


def search_logits(step_logits, cfg: dict, max_new: int, W: int, patience: float = 1.0) -> dict:
    """Beam search over scripted logits: ``step_logits(i, slots) -> [W][vocab]`` gives the logits of step i for the current
    slots.  The loop of ``beam_search`` without a network."""
    C = finish_count(W, patience)
    dead = {"tokens": [], "sum_logprob": NEG_INF}
    slots = [{"tokens": [], "sum_logprob": 0.0}] + [dict(dead) for _ in range(W - 1)]
    finished, steps = [], []
    for i in range(max_new):
        logits = np.asarray(step_logits(i, slots))
        r = beam_step(logits, [s["tokens"] for s in slots], [s["sum_logprob"] for s in slots], len(finished), cfg, W, C)
        steps.append({"slots": slots, "logits": logits, **r})
        for j, score in r["finished"]:
            finished.append({"tokens": list(slots[j]["tokens"]), "sum_logprob": score, "ended": True})
        slots = [{"tokens": slots[j]["tokens"] + [t], "sum_logprob": score} for j, t, score in r["live"]]
        slots += [dict(dead) for _ in range(W - len(slots))]
        if r["complete"]:
            break
    hyps = finalize(finished, slots, W)
    return {"hyps": hyps, "best": rank(hyps), "steps": steps}


@torch.no_grad()
def beam_search(oracle: wo.Oracle, enc: torch.Tensor, prompt: list[int], max_new: int, W: int, patience: float = 1.0) -> list[dict]:
    """Beam search of every window of ``enc``.  Per window: ``hyps`` [{tokens (before EOT), sum_logprob, ended}], ``best``,
    ``tokens`` / ``n`` of the hypotheses in the device's layout (EOT-filled to max_new; n counts the EOT), ``no_speech_prob``,
    ``lang``, ``lang_margin`` and ``steps``: per sampled step the slots before it, each slot's rule-free logits, the result
    of ``beam_step`` and its margin."""
    cfg = oracle.cfg
    out = []
    for b in range(enc.shape[0]):
        e = enc[b:b + 1]
        kv = oracle.cross_kv(e)
        info = {}

        def step_logits(i, slots):
            live = [j for j, s in enumerate(slots) if s["sum_logprob"] > NEG_INF]
            ids = [list(prompt) + slots[j]["tokens"] for j in live]
            n = len(live)
            kvn = kv if n == 1 else [(k.repeat(n, 1, 1), v.repeat(n, 1, 1)) for k, v in kv]
            lg = oracle.forced_logits(e if n == 1 else e.repeat(n, 1, 1), ids, kvn).double().numpy()
            if not info:
                first = lg[0][0]
                info["no_speech_prob"] = float(np.exp(first[cfg["no_speech"]] - wo._lse(first)))
                info["lang"] = int(cfg["lang_ids"][int(np.argmax(first[cfg["lang_ids"]]))])
                info["lang_margin"] = float(np.diff(np.sort(first[cfg["lang_ids"]])[-2:])[0])
            z = np.zeros((W, lg.shape[-1]))
            for k, j in enumerate(live):
                z[j] = lg[k][-1]
            return z

        res = search_logits(step_logits, cfg, max_new, W, patience)
        res.update(info)
        res["tokens"] = [h["tokens"] + [cfg["eot"]] * (max_new - len(h["tokens"])) for h in res["hyps"]]
        res["n"] = [len(h["tokens"]) + (1 if h["ended"] else 0) for h in res["hyps"]]
        out.append(res)
    return out
