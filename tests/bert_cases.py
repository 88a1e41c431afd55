"""Case tables of tests/test_bert_routes_gpu.py: the shapes, masks and switches that reach every kernel route of the K8
encoder (csrc/bert.hip), with the route log each case must leave behind (``embed.routes``) written down as data.

Run as a program (``python tests/bert_cases.py OUT.npz``) this file is the child process of the switch cases: the
encoder reads EIOKU_GEMM_BF16 / EIOKU_GEMM_S / EIOKU_ATTN_MFMA / EIOKU_GEMM_PLANES once per process, so each set of
switches gets a process of its own, which encodes CHILD_SHAPES and saves outputs and route logs for the parent.

The split-K factors below are pick_splits' for the 256 compute units of an MI355X (the only target of this library).
"""
from __future__ import annotations

import functools
import json
import sys
from collections import Counter, namedtuple
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from eioku_amd import embed  # noqa: E402

RTOL = 1e-4  # BASELINE.json: embeddings within 1e-4 relative; max|got - want| <= RTOL * max|want|

# ---------------------------------------------------------------------------------------------------------------------
# configurations
# ---------------------------------------------------------------------------------------------------------------------
MINILM = dict(embed.MINILM_L6_V2, vocab=3000, max_pos=512)
MINILM_2L = dict(MINILM, layers=2)  # all four GEMMs of a layer, a third of the oracle's cost


def width_cfg(hidden: int, ffn: int) -> dict:
    return dict(embed.MINILM_L6_V2, vocab=500, max_pos=160, layers=2, hidden=hidden, heads=hidden // 32, ffn=ffn)


CONFIGS = {"minilm": MINILM, "minilm_2l": MINILM_2L}
STATE_SEED = 3


@functools.lru_cache(maxsize=None)
def _state(key: str):
    return embed.random_state(config(key), STATE_SEED)


def config(key: str) -> dict:
    if key in CONFIGS:
        return CONFIGS[key]
    hidden, ffn = (int(v) for v in key[1:].split("x"))  # "w512x384"
    return width_cfg(hidden, ffn)


def state(key: str) -> dict:
    """The seeded weights of a configuration: drawn once, shared by every test of the session, never written to."""
    return _state(key)


# ---------------------------------------------------------------------------------------------------------------------
# inputs.  The ids under masked positions are random NON-ZERO ids: a kernel that ignores the mask cannot pass.
# ---------------------------------------------------------------------------------------------------------------------
def prefix_inputs(vocab: int, B: int, S: int, seed: int):
    """Ragged prefix masks: the LAST row keeps all S tokens - the last position row is live, and so is the last token row
    of the batch, the one a GEMM's row tail ends on - the others a random 1..S.  With S == 1 there is no prefix to cut: one
    row in ten is masked altogether."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(1, vocab, (B, S)).astype(np.int32)
    mask = np.ones((B, S), dtype=np.uint8)
    if S == 1:
        mask[:-1, 0] = rng.random(B - 1) < 0.9
    else:
        for b in range(B - 1):
            mask[b, int(rng.integers(1, S + 1)):] = 0
    return ids, mask


MASK_ROWS = ("all live", "only token 0", "only the last token", "token 0 masked", "random holes p=0.6", "every second token",
             "all masked")


def shaped_masks(vocab: int, S: int, seed: int):
    """One row per entry of MASK_ROWS."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(1, vocab, (len(MASK_ROWS), S)).astype(np.int32)
    mask = np.zeros((len(MASK_ROWS), S), dtype=np.uint8)
    mask[0] = 1
    mask[1, 0] = 1
    mask[2, S - 1] = 1
    mask[3, 1:] = 1
    mask[4] = rng.random(S) < 0.6
    mask[4, S // 2] = 1  # never empty
    mask[5, ::2] = 1
    return ids, mask


def redraw_masked(vocab: int, ids: np.ndarray, mask: np.ndarray, seed: int) -> np.ndarray:
    """The same ids where the mask is 1, other non-zero ids where it is 0."""
    other = np.random.default_rng(seed).integers(1, vocab - 1, ids.shape).astype(np.int32)
    other += other >= ids  # 1 .. vocab - 1 without ids itself
    return np.where(mask.astype(bool), ids, other).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# the route log of one encode call, as data
#   attn: attention kernel; gemm: bf_as1 (split bf16, A operand as planes), bf_as0 (split in the staging threads), f32
#   (exact-fp32 k_gemm_f32), f32_s (exact-fp32 k_gemm_f32_s); tile: rows of the GEMM tile; ln / pool: the LayerNorm and
#   pooling kernels; sp_o / sp_f: split-K factor of the attention-output and the FFN2 GEMM (QKV and FFN1 never split).
# ---------------------------------------------------------------------------------------------------------------------
Route = namedtuple("Route", "attn gemm tile ln pool sp_o sp_f")


def expected_log(route: Route, layers: int) -> dict[str, int]:
    """Every non-zero counter of the log after ONE encode call: per layer one attention launch, the QKV, output and
    FFN2 GEMMs (EPI0) and FFN1 (EPI1, GELU), two LayerNorms; one pooling launch."""
    T = f"T{route.tile}"
    epi0, epi1 = {"bf_as1": (f"gemm_bf<EPI0,{T},AS1>", f"gemm_bf<EPI1,{T},AS1>"),
                  "bf_as0": (f"gemm_bf<EPI0,{T},AS0>", f"gemm_bf<EPI1,{T},AS0>"),
                  "f32": (f"gemm_f32<EPI0,{T}>", f"gemm_f32<EPI1,{T}>"),
                  "f32_s": ("gemm_f32_s<EPI0>", "gemm_f32_s<EPI1>")}[route.gemm]
    log = Counter({route.attn: layers, epi0: 3 * layers, epi1: layers, route.ln: 2 * layers, route.pool: 1})
    log["splits<1>"] += 2 * layers
    log[f"splits<{route.sp_o}>"] += layers
    log[f"splits<{route.sp_f}>"] += layers
    return dict(log)


# MiniLM (hidden 384 = 3 stages of 128, ffn 1536 = 12): up to 1792 tokens the output GEMM splits 3 ways and FFN2 4 ways
MINI = Route("attn_bf", "bf_as1", 64, "add_ln_fixed<6>", "pool<G2>", 3, 4)
MINI8, MINI1 = MINI._replace(attn="attn8"), MINI._replace(attn="attn1")
BIG = MINI._replace(tile=128, sp_o=1, sp_f=1)  # M >= 8192: 128 x 128 tiles, no split-K

# Measured drift max|got - want| / max|want| against the float64 oracle on an MI355X, worst case of each group (the bar is
# 1e-4; the float32 restatement of the oracle itself sits 1.1e-6 from float64):
#   a. sequence-length edges  9.6e-6 (3 x 128)
#   b. mask shapes            1.5e-5 (S = 33; by row 1.6e-5, "only token 0")
#   c. large-M tile tails     8.5e-6 (8191 x 1, 8192 x 1)
#   d. switch children        1.1e-5 default = no_planes (3 x 33); fma_s 2.9e-6; fma 5.4e-7
#   e. other widths           7.3e-6 (1024 x 1536, 3 x 130)
# a. sequence-length edges: (B, S, route).  S = 257 and 300 both launch k_attention<1> with 320 threads; S = 512 reads the
# last position row and asks for the largest LDS block (133 KB).
SEQ_EDGES = [
    (3, 127, MINI), (3, 128, MINI), (3, 129, MINI8), (2, 255, MINI8), (2, 256, MINI8), (2, 257, MINI1), (2, 300, MINI1),
    (2, 511, MINI1), (2, 512, MINI1),
]

# b. mask shapes: (S, route) - one 7-row batch (MASK_ROWS) per attention kernel plus a sub-wave length.  2100 tokens at
# S = 300: FFN2 splits 3 ways.
MASK_SHAPES = [(33, MINI), (128, MINI), (200, MINI8), (300, MINI1._replace(sp_f=3))]

# c. large-M tile tails, 2-layer MiniLM: (B, S, route)
#   65 x 127 = 8255 tokens: 64 full 128-row blocks + a 63-row tail, 65 row blocks padded to 72
#   129 x 64 = 8256: a tail of exactly 64 rows (the wm = 1 waves of the last block are entirely out of range)
#   8191 x 1 / 8192 x 1: either side of the M >= 8192 switch, and S = 1
LARGE_M = [
    (65, 127, BIG), (129, 64, BIG), (8191, 1, MINI._replace(sp_o=1, sp_f=1)), (8192, 1, BIG),
]

# d. switches (read once per process -> one child process each): name -> environment
CHILD_ENVS = {
    "default": {},
    "fma": {"EIOKU_GEMM_BF16": "0", "EIOKU_GEMM_S": "0", "EIOKU_ATTN_MFMA": "0"},
    "fma_s": {"EIOKU_GEMM_BF16": "0"},
    "no_planes": {"EIOKU_GEMM_PLANES": "0"},
}
CHILD_SHAPES = [("minilm", 3, 33), ("minilm", 5, 100), ("minilm", 2, 200), ("minilm", 2, 300), ("minilm_2l", 65, 127)]
_DEFAULT_CHILD = [MINI, MINI, MINI8, MINI1, BIG]
CHILD_ROUTES = {  # per child, one Route per entry of CHILD_SHAPES
    "default": _DEFAULT_CHILD,
    # EIOKU_ATTN_MFMA=0: k_attention8 up to S = 256; EIOKU_GEMM_S=0: k_gemm_f32 in both tile sizes
    "fma": [MINI8._replace(gemm="f32"), MINI8._replace(gemm="f32"), MINI8._replace(gemm="f32"), MINI1._replace(gemm="f32"),
            BIG._replace(attn="attn8", gemm="f32")],
    # EIOKU_GEMM_BF16=0: k_gemm_f32_s below 8192 rows, the 128 x 128 k_gemm_f32 from there
    "fma_s": [r._replace(gemm="f32_s") for r in _DEFAULT_CHILD[:4]] + [BIG._replace(gemm="f32")],
    "no_planes": [r._replace(gemm="bf_as0") for r in _DEFAULT_CHILD],
}

# e. other widths: (hidden, ffn, sp_o, sp_f), each at WIDTH_SHAPES.  At most 7 x 16 = 112 tiles: every split that divides
# the K / 128 stages is taken, so the factor is the largest of 2, 3, 4 that divides them (else 1).
#   generic k_add_ln everywhere but 768 (k_add_ln_fixed<12>); two pooling groups up to 512, one from 640 (1024: a
#   1024-thread block).  Split factors reached: 1, 2, 3 and 4.
WIDTHS = [
    (128, 128, 1, 1), (256, 640, 2, 1), (512, 384, 4, 3), (640, 1280, 1, 2), (768, 3072, 3, 4), (1024, 1536, 4, 4),
]
WIDTH_SHAPES = [(5, 33, "attn_bf"), (3, 130, "attn8")]  # 130: k_attention8 on a row stride other than MiniLM's
WIDTH_MAXPOS = (256, 640, 2, 160)  # (hidden, ffn, B, S): S == max_pos, the last row of the position table


def width_route(hidden: int, sp_o: int, sp_f: int, attn: str) -> Route:
    return Route(attn, "bf_as1", 64, "add_ln_fixed<12>" if hidden == 768 else "add_ln", "pool<G2>" if hidden <= 512 else "pool<G1>",
                 sp_o, sp_f)


# f. handle reuse: one encoder, this order; (40, 128) = 5120 tokens: 480 tiles, FFN2 splits 2 ways
REUSE_ORDER = [(2, 512, MINI1), (3, 7, MINI), (2, 300, MINI1), (40, 128, MINI._replace(sp_f=2)), (3, 7, MINI)]

# g. routes no public entry point reaches: name -> one line of reason.  (pick_splits' second branch, for K % 128 != 0,
# was dead - eioku_bert_create requires hidden and ffn to be multiples of 128 - and is gone.)
UNREACHABLE: dict[str, str] = {}


def all_expected_routes() -> set[str]:
    """Union of the route names the cases above expect."""
    routes = [(r, 6) for _, _, r in SEQ_EDGES] + [(r, 6) for _, r in MASK_SHAPES] + [(r, 2) for _, _, r in LARGE_M]
    routes += [(r, 6) for rs in CHILD_ROUTES.values() for r in rs] + [(r, 6) for _, _, r in REUSE_ORDER]
    routes += [(width_route(h, so, sf, attn), 2) for h, _, so, sf in WIDTHS for _, _, attn in WIDTH_SHAPES]
    routes.append((width_route(WIDTH_MAXPOS[0], 2, 1, "attn8"), 2))
    names: set[str] = set()
    for r, layers in routes:
        names |= set(expected_log(r, layers))
    return names


def child_inputs(i: int):
    key, B, S = CHILD_SHAPES[i]
    return prefix_inputs(config(key)["vocab"], B, S, 7000 + i)


def _child(out_path: str) -> None:
    outs = {}
    for i, (key, B, S) in enumerate(CHILD_SHAPES):
        enc = embed.MiniLMEncoder(state(key), config(key))
        ids, mask = child_inputs(i)
        embed.routes(reset=True)
        outs[f"out{i}"] = enc.encode_ids(ids, mask)
        outs[f"log{i}"] = np.array(json.dumps(embed.routes(reset=True)))
        enc.close()
    np.savez(out_path, **outs)


if __name__ == "__main__":
    _child(sys.argv[1])
