"""CPU oracle for K21 (word alignment): Whisper's ``find_alignment`` restated in numpy / torch-CPU on top of
tests/whisper_oracle.py.

Steps (the numbering of DESIGN.md "K21 word alignment"): 1 the sequence, 2 one teacher-forced causal pass, 3 the
cross-attention probabilities of the alignment heads, 4 normalisation over the token rows, 5 the width-7 median filter, 6 the
head mean, row slice and sign, 7 dynamic time warping, 8 the forced-token probabilities, 9 token times and words.  Nothing
here imports the product or ``transformers``; tests/golden/whisper_align_hf.json pins the filter and the warping to the
``transformers`` implementation.
"""
from __future__ import annotations

import numpy as np
import torch

import whisper_oracle as wo

FILTER_WIDTH = 7
MS_PER_JUMP = 20


# ---- 4 - 6: the cost ----------------------------------------------------------------------------------------------------------
def median_filter(x: np.ndarray, width: int = FILTER_WIDTH) -> np.ndarray:
    """Median of width ``width`` along the last axis with reflect padding; returned unchanged when the axis is not longer
    than the padding."""
    pad = width // 2
    if x.shape[-1] <= pad:
        return x
    p = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(pad, pad)], mode="reflect")
    win = np.stack([p[..., k:k + x.shape[-1]] for k in range(width)], axis=-1)
    return np.sort(win, axis=-1)[..., pad]


def cost_from_weights(a: np.ndarray, sot_len: int) -> np.ndarray:
    """a [H][T][F] -> cost [T - sot_len - 1][F] in a's dtype: (a - mean_t) / std_t (population std, no guard), median
    filter along F, mean over the heads, rows sot_len .. T - 2, negated."""
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (a - a.mean(axis=1, keepdims=True)) / a.std(axis=1, keepdims=True)
    z = median_filter(z)
    return -z.mean(axis=0)[sot_len:-1]


# ---- 7: dynamic time warping ---------------------------------------------------------------------------------------------------
def dtw(cost: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(text_idx, time_idx) of the path from (0, 0) to (N - 1, F - 1).  fp32, one add per cell.  D is bordered by +inf with
    D[0][0] = 0; a cell takes the diagonal when it is below both others, else the cell above when it is below both others,
    else the cell to the left.  The border's trace is left along row 0 and up along column 0.  Cells are filled one
    anti-diagonal at a time (every cell depends on the two diagonals before its own)."""
    m = np.asarray(cost, dtype=np.float32)
    N, F = m.shape
    D = np.full((N + 1, F + 1), np.inf, dtype=np.float32)
    tr = -np.ones((N + 1, F + 1), dtype=np.int8)
    D[0, 0] = 0
    with np.errstate(invalid="ignore"):
        for k in range(2, N + F + 1):
            i = np.arange(max(1, k - F), min(N, k - 1) + 1)
            j = k - i
            c0, c1, c2 = D[i - 1, j - 1], D[i - 1, j], D[i, j - 1]
            diag = (c0 < c1) & (c0 < c2)
            up = ~diag & (c1 < c0) & (c1 < c2)
            c = np.where(diag, c0, np.where(up, c1, c2))
            D[i, j] = m[i - 1, j - 1] + c
            tr[i, j] = np.where(diag, 0, np.where(up, 1, 2))
    tr[0, :] = 2
    tr[:, 0] = 1
    i, j, ti, fi = N, F, [], []
    while i > 0 or j > 0:
        ti.append(i - 1)
        fi.append(j - 1)
        t = tr[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return np.array(ti[::-1], dtype=np.int64), np.array(fi[::-1], dtype=np.int64)


def jumps(text_idx: np.ndarray, time_idx: np.ndarray, n_rows: int) -> np.ndarray:
    """jump[i]: the frame index of the first path cell in token row i."""
    out = np.full(n_rows, -1, dtype=np.int64)
    for t, f in zip(text_idx[::-1], time_idx[::-1]):
        if t >= 0:
            out[t] = f
    return out


# ---- 1 - 3 and 8: the pass -----------------------------------------------------------------------------------------------------
def default_heads(cfg: dict) -> list[tuple[int, int]]:
    return [(l, h) for l in range(cfg["dec_layers"] // 2, cfg["dec_layers"]) for h in range(cfg["heads"])]


def sequence(cfg: dict, sot_sequence: list[int], text: list[int]) -> list[int]:
    return list(sot_sequence) + [cfg["no_timestamps"]] + list(text) + [cfg["eot"]]


class AlignOracle(wo.Oracle):
    """``Oracle`` with a decoder pass that keeps the cross-attention probabilities."""

    @torch.no_grad()
    def forced_pass(self, enc: torch.Tensor, ids: list[int]):
        """One window (enc [1][ctx][d]) and one sequence -> (logits [T][vocab], {layer: probabilities [heads][T][ctx]}).
        The block is ``Oracle._block`` with the cross-attention softmax kept: scores from the rounded q and k, x 0.125, fp32
        softmax over all ctx keys."""
        cfg, w = self.cfg, self.w
        kv = self.cross_kv(enc)
        idt = torch.as_tensor(np.asarray([ids]), dtype=torch.long)
        T, h = idt.shape[1], cfg["heads"]
        x = w["model.decoder.embed_tokens.weight"][idt] + w["model.decoder.embed_positions.weight"][:T][None]
        probs = {}
        for i in range(cfg["dec_layers"]):
            p = f"model.decoder.layers.{i}."
            hh = self._ln(x, p + "self_attn_layer_norm")
            q, k, v = (self.r(self._lin(hh, p + f"self_attn.{n}_proj")) for n in "qkv")
            x = x + self._lin(self._attend(q, k, v, True), p + "self_attn.out_proj")
            hh = self._ln(x, p + "encoder_attn_layer_norm")
            q = self.r(self._lin(hh, p + "encoder_attn.q_proj"))
            qh = q.view(1, T, h, 64).transpose(1, 2)
            kh = kv[i][0].view(1, -1, h, 64).transpose(1, 2)
            probs[i] = torch.softmax((qh @ kh.transpose(-1, -2)) * 0.125, dim=-1)[0]
            x = x + self._lin(self._attend(q, kv[i][0], kv[i][1], False), p + "encoder_attn.out_proj")
            hh = self._ln(x, p + "final_layer_norm")
            x = x + self._lin(self.r(torch.nn.functional.gelu(self._lin(hh, p + "fc1"))), p + "fc2")
        logits = self._ln(x, "model.decoder.layer_norm") @ w["model.decoder.embed_tokens.weight"].T
        return logits[0], probs

    def align(self, enc: torch.Tensor, sot_sequence: list[int], text: list[int], n_frames: int, heads=None) -> dict:
        """Steps 1 - 8 for one window: ``cost`` [N][F] float64 (from the pass's fp32 probabilities), ``jump`` [N] from the
        warping of the fp32-rounded cost, ``prob`` [len(text)]."""
        cfg = self.cfg
        seq = sequence(cfg, sot_sequence, text)
        S, F = len(sot_sequence), n_frames // 2
        logits, probs = self.forced_pass(enc, seq)
        heads = list(heads) if heads else default_heads(cfg)
        a = np.stack([probs[l][h].double().numpy()[:, :F] for l, h in heads])
        cost = cost_from_weights(a, S)
        ti, fi = dtw(cost.astype(np.float32))
        lg = logits.double().numpy()
        prob = np.array([float(np.exp(lg[S + i, tok] - wo._lse(lg[S + i, :cfg["eot"]]))) for i, tok in enumerate(text)])
        return {"cost": cost, "jump": jumps(ti, fi, len(text) + 1), "prob": prob, "text_idx": ti, "time_idx": fi}


# ---- 9: times ----------------------------------------------------------------------------------------------------------------
def word_times(word_token_counts: list[int], jump, prob, window_start_ms: int) -> list[tuple[int, int, float]]:
    """(start_ms, end_ms, confidence) per word: a word over token rows [a, b) starts at row a's time, ends at row b's (the
    EOT row ends the last word) and has the mean probability of its tokens."""
    out, a = [], 0
    for n in word_token_counts:
        b = a + n
        out.append((window_start_ms + MS_PER_JUMP * int(jump[a]), window_start_ms + MS_PER_JUMP * int(jump[b]),
                    float(np.mean(prob[a:b]))))
        a = b
    return out
