"""Float64 references and input recipes for the OCR stage entry points (``eioku_craft_canvas``, ``eioku_ocr_maxpool_f16``,
``eioku_ocr_im2col_dil_f16``, ``eioku_ocr_up2x_f16``, ``eioku_ctc_probs``, ``eioku_crnn_tail``).

Each reference is the plain torch / numpy operation in float64 on the very values the kernel reads.  The recipes build
inputs whose reference is decided (no near-ties, exact fp32 arithmetic) so that the GPU tests can ask for equality;
``tests/test_ocr_host.py`` checks on the CPU that the recipes deliver what they promise.
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

import ocr_oracle
from eioku_amd import ocr

SENTINEL = 1234.0  # fills the channels a strided kernel must not touch (exact in fp16)


# ---- CRAFT canvas --------------------------------------------------------------------------------------------------
def canvas_f16(frames_bgr: np.ndarray, canvas: int) -> np.ndarray:
    """``ocr_oracle.craft_input`` as the network reads it: fp16 (n, H, W, 8), channels 3..7 zero."""
    x, _ = ocr_oracle.craft_input(frames_bgr, canvas)
    x = x.permute(0, 2, 3, 1).numpy()
    out = np.zeros(x.shape[:3] + (8,), np.float16)
    out[..., :3] = x.astype(np.float16)
    return out


def pad_value_f16() -> np.ndarray:
    """The canvas' padding: zero, then normalised in float32 -> ``-mean / std`` as fp16 (3,)."""
    m = np.array([v * 255.0 for v in ocr_oracle.MEAN], np.float32)
    s = np.array([v * 255.0 for v in ocr_oracle.STD], np.float32)
    return ((np.float32(0) - m) / s).astype(np.float16)


def canvas_frames(seed: int, n: int, h: int, w: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


# ---- glue kernels over fp16 NHWC -----------------------------------------------------------------------------------
def f16_values(seed: int, shape, negative: bool = False) -> np.ndarray:
    """fp16 normals; ``negative``: all below zero (a zero-initialised or zero-padded maximum then shows)."""
    x = np.random.default_rng(seed).standard_normal(shape)
    return (-np.abs(x) - 0.25 if negative else x).astype(np.float16)


def _nchw64(x16: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(x16.astype(np.float64)).permute(0, 3, 1, 2)


def maxpool(x16: np.ndarray, kernel, stride, pad) -> np.ndarray:
    """``F.max_pool2d`` in float64 on fp16 values (n, h, w, c) -> fp16 (n, ho, wo, c); a maximum of fp16 values is one."""
    y = F.max_pool2d(_nchw64(x16), tuple(kernel), tuple(stride), tuple(pad))
    return y.permute(0, 2, 3, 1).numpy().astype(np.float16)


def im2col_dil(x16: np.ndarray, d: int) -> np.ndarray:
    """``F.unfold(kernel 3, dilation d, padding d)`` (channel-major [c][tap]) rearranged to tap-major (n, h, w, 9, c)."""
    n, h, w, c = x16.shape
    u = F.unfold(_nchw64(x16), 3, dilation=d, padding=d)  # (n, c * 9, h * w)
    return u.reshape(n, c, 9, h, w).permute(0, 3, 4, 2, 1).numpy().astype(np.float16)


def up2x_values(seed: int, shape) -> np.ndarray:
    """fp16 normals clamped to |x| < 4 with |x| < 2^-6 replaced by 0.5: multiples of 2^-16 below 4.  The bilinear weights
    of an exact 2x are products of 1/4 and 3/4 (sixteenths), so every product and sum of the fp32 evaluation fits 24 bits:
    fp32 is exact, and one rounding to fp16 equals the float64 reference's."""
    x = np.random.default_rng(seed).standard_normal(shape).astype(np.float16)
    x = np.clip(x, np.float16(-3.998), np.float16(3.998))
    x[np.abs(x) < np.float16(2.0 ** -6)] = np.float16(0.5)
    return x


def up2x(x16: np.ndarray, dtype=torch.float64) -> np.ndarray:
    """``F.interpolate(scale_factor=2, bilinear, align_corners=False)`` in ``dtype``, rounded once to fp16."""
    y = F.interpolate(_nchw64(x16).to(dtype), scale_factor=2, mode="bilinear", align_corners=False)
    return y.permute(0, 2, 3, 1).numpy().astype(np.float16)  # numpy rounds float64 -> fp16 in one step


def strided(dense16: np.ndarray, stride: int, off: int) -> np.ndarray:
    """``dense16`` as channels off.. of a sentinel-filled (n, h, w, stride) tensor."""
    out = np.full(dense16.shape[:3] + (stride,), SENTINEL, np.float16)
    out[..., off:off + dense16.shape[3]] = dense16
    return out


# ---- CTC probabilities ---------------------------------------------------------------------------------------------
CTC_MARGIN = 1e-4  # the float64 top-2 margin (logits, kept classes) above which idx must equal the reference's


def ctc(logits: np.ndarray, ignore: np.ndarray):
    """Float64 ``softmax -> p[ignored] = 0 -> p / sum p`` -> (idx: first argmax, prob, top-2 kept logit margin)."""
    l = logits.astype(np.float64)
    p = np.exp(l - l.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    p[:, ignore != 0] = 0.0
    p /= p.sum(-1, keepdims=True)
    kept = np.where(ignore != 0, -np.inf, l)
    if kept.shape[1] - int((ignore != 0).sum()) >= 2:
        top = np.sort(kept, -1)
        margin = top[:, -1] - top[:, -2]
    else:
        margin = np.full(len(l), np.inf)
    return p.argmax(-1).astype(np.int32), p.max(-1), margin


CTC_MASKS = ("none", "top", "all_but_one")


def ctc_case(C: int, rows: int, mask: str, seed: int = 0):
    """float32 logits (rows, C) and u8 ignore (C,).  Rows are normal with sigma 4; every odd row is rescaled to a spread
    (max - min) of 60, where most terms vanish beside the largest.  Masks: ``none``; ``top``: a third of the classes
    ignored (at least one) and every row's largest logit planted on one of them; ``all_but_one``: one class kept.  The
    winner among the kept classes is raised until it leads by 0.5, so no row is a near-tie."""
    rng = np.random.default_rng(1000 * C + 10 * rows + CTC_MASKS.index(mask) + seed)
    l = 4.0 * rng.standard_normal((rows, C))
    for r in range(1, rows, 2):
        l[r] *= 60.0 / (l[r].max() - l[r].min())
    ignore = np.zeros(C, np.uint8)
    if mask == "top":
        ign = rng.choice(C, max(1, C // 3), replace=False)
        ignore[ign] = 1
        for r in range(rows):
            l[r, ign[r % len(ign)]] = l[r].max() + 1.0
    elif mask == "all_but_one":
        ignore[:] = 1
        ignore[rng.integers(C)] = 0
    kept = np.flatnonzero(ignore == 0)
    for r in range(rows):
        k = kept[np.argmax(l[r, kept])]
        l[r, k] += 0.5
    return l.astype(np.float32), ignore


def ctc_tie_cases(C: int):
    """Rows with one float planted twice above everything else -> ``(logits (k, C), names, lower class (k,), upper (k,))``.
    One wave reads class c on lane c % 64: ties inside a lane (c, c + 64), on neighbouring lanes, on lanes 0 and 63, and a
    tie whose lower class is ignored (the upper must win)."""
    rng = np.random.default_rng(77 + C)
    pairs = [("neighbouring lanes", C // 2 - 1, C // 2)] if C > 2 else [("neighbouring lanes", 0, 1)]
    if C > 64:
        pairs.append(("one lane (c, c + 64)", (C - 65) // 2, (C - 65) // 2 + 64))
    if C >= 64:
        pairs.append(("lanes 0 and 63", 64 * ((C - 64) // 64), 64 * ((C - 64) // 64) + 63))
    l = (4.0 * rng.standard_normal((len(pairs), C))).astype(np.float32)
    for r, (_, a, b) in enumerate(pairs):
        l[r, a] = l[r, b] = np.float32(l[r].max() + 2.0)
    return l, [n for n, _, _ in pairs], np.array([a for _, a, _ in pairs], np.int32), np.array([b for _, _, b in pairs], np.int32)


# ---- the recogniser's tail -----------------------------------------------------------------------------------------
TAIL_SETS = {
    "one step": (1,),
    "1 2 3 17": (1, 2, 3, 17),
    "five sequences, partial last tile": (16, 1, 15, 2, 63),
    "equal lengths": (3, 3, 3, 3),
    "nine of 24": (24,) * 9,
    "15 rows": (7, 8),
    "17 rows": (9, 8),
}
TAIL_SEED = 6
TAIL_IGNORE = tuple(range(3, 97, 5))


def tail_state() -> dict:
    """The seeded recogniser weights the tail tests use (``ocr.random_crnn_state``: nn.LSTM's own initialisation, Linear
    twice that, Prediction 0.25 x normal, which leaves the float64 top-2 margins far above the float32 drift)."""
    return ocr.random_crnn_state(TAIL_SEED)


def tail_inputs(lens) -> list:
    """Standard normal features: W_ih is U(-1/16, 1/16) over 256 inputs, so gate pre-activations have variance 1/3."""
    rng = np.random.default_rng(sum(lens) * 31 + len(lens))
    return [rng.standard_normal((t, 256)).astype(np.float32) for t in lens]


def tail_logits(sd: dict, seqs: list, dtype) -> list:
    """``SequenceModeling`` + ``Prediction`` of english_g2 on each sequence alone, in ``dtype``: logits (T_i, classes)."""
    sd = ocr._np_state(sd)
    t = lambda k: torch.from_numpy(np.asarray(sd[k], np.float32)).to(dtype)
    out = []
    with torch.no_grad():
        for s in seqs:
            v = torch.from_numpy(np.asarray(s, np.float32)).to(dtype)[None]
            for l in range(2):
                q = f"SequenceModeling.{l}."
                rnn = torch.nn.LSTM(256, 256, bidirectional=True, batch_first=True).to(dtype)
                rnn.load_state_dict({k[len(q + "rnn."):]: t(k) for k in sd if k.startswith(q + "rnn.")})
                v = F.linear(rnn(v)[0], t(q + "linear.weight"), t(q + "linear.bias"))
            out.append(F.linear(v, t("Prediction.weight"), t("Prediction.bias"))[0].numpy())
    return out


@functools.lru_cache(maxsize=None)
def tail_reference(name: str):
    """Computed once per sequence set and shared: ``(seqs, float64 logits, d_ref, idx, prob, margin)``.  ``d_ref`` = the
    largest |float32 torch - float64 torch| of the logits as a fraction of max |logit|; idx / prob after
    ``ocr.ignore_renormalise`` on the float64 softmax; margin = the float64 top-2 logit margin over the kept classes."""
    seqs = tail_inputs(TAIL_SETS[name])
    sd = tail_state()
    l64 = np.concatenate(tail_logits(sd, seqs, torch.float64))
    l32 = np.concatenate(tail_logits(sd, seqs, torch.float32))
    d_ref = float(np.abs(l32 - l64).max() / np.abs(l64).max())
    p = ocr.ignore_renormalise(F.softmax(torch.from_numpy(l64), dim=-1).numpy(), TAIL_IGNORE)
    kept = l64.copy()
    kept[:, list(TAIL_IGNORE)] = -np.inf
    top = np.sort(kept, -1)
    return seqs, l64, d_ref, p.argmax(-1).astype(np.int32), p.max(-1), top[:, -1] - top[:, -2]
