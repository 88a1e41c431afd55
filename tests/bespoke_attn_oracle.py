"""CPU restatements of the attention kernels two models keep to themselves - Whisper's k_attn<QPW, ANC, CAUSAL> and
k_attn_weights (csrc/whisper.hip), TimeSformer's k_attn_time (csrc/actions.hip) - and of the index movers of Whisper's prompt
prefill and front end, for tests/test_bespoke_attn_host.py and tests/test_bespoke_attn_gpu.py.

As in transformer_core_oracle.py each operation comes twice, on the exact fp16 inputs the device gets:
  * the reference: plain float64, no rounding anywhere;
  * the emulation, which follows the source: the dot as 64 multiply-then-add steps in fp32 in c * 8 + e order (the build has
    -ffp-contract=off; the fp16 x fp16 products are exact in fp32), x 0.125, causal -inf, the fp32 maximum, exp of the fp32
    difference computed in float64 and rounded once to fp32, the lane-strided partial sums folded by the xor butterfly, PV
    sequential in j in fp32, one division, one rounding to fp16 (k_attn, k_attn_time) or an fp32 p / sum (k_attn_weights).
    Its `mutant` argument switches on one deliberate error at a time.
Which key row a query reads is one table for all of them: key_source().  The movers are numpy indexing.

Nothing here imports the package or needs a GPU."""
from __future__ import annotations

import numpy as np

from transformer_core_oracle import (ATTN_GENERATORS, _wave_sum, attn_blocks, attn_inputs, attn_qkv, attn_within_bar,  # noqa: F401
                                     block_errors, half_ulp16, to_f16)

HEADS = 2
D = 64 * HEADS
TM = 448  # Whisper's max_target_positions: the lane stride of the self-attention cache and of the ancestry table

KEY_MUTANTS = ["kv_div_ignored", "kvmap_ignored", "ancestry_ignored", "ancestry_transposed"]
SOFTMAX_MUTANTS = ["causal_off_by_one", "causal_wave_bound_q0", "qpw2_second_reads_first"]
WEIGHT_MUTANTS = ["weights_over_nF"]
TIME_MUTANTS = ["time_drops_keys_from_64", "time_k_from_v_third"]
MOVER_MUTANTS = ["cache_lane_r_G_g"]
MUTANTS = KEY_MUTANTS + SOFTMAX_MUTANTS + WEIGHT_MUTANTS + TIME_MUTANTS + MOVER_MUTANTS


# ---- whose keys ----------------------------------------------------------------------------------------------------------------
def key_source(B, n_keys, W, kv_div=1, kvmap=None, anc=None, mutant=None):
    """[B][n_keys]: the window / lane (of W) whose row j query batch b reads as key j.  k_attn: b / kv_div, kvmap[b] where there
    is a map, and under an ancestry table anc [B][anc_ld] the lane anc[b][j], key by key.  A mutant that forgets an indirection
    reads its own batch b (wrapped into the W there are)."""
    b = np.arange(B)
    if anc is not None:
        anc = np.asarray(anc)
        if mutant == "ancestry_ignored":
            return np.repeat(b[:, None] % W, n_keys, axis=1)
        if mutant == "ancestry_transposed":  # the table read as [anc_ld][B]
            return anc.reshape(-1)[np.arange(n_keys)[None, :] * B + b[:, None]].astype(np.int64)
        return anc[:, :n_keys].astype(np.int64)
    if kvmap is not None and mutant != "kvmap_ignored":
        w = np.asarray(kvmap)[b]
    else:
        w = (b if mutant == "kv_div_ignored" else b // kv_div) % W
    return np.repeat(w[:, None], n_keys, axis=1)


def gather_keys(K, src_b):
    """K [W][rows][64 ...] -> the rows [n_keys][...] batch b reads, src_b = key_source(...)[b]"""
    return K[src_b, np.arange(len(src_b))]


# ---- float64 references --------------------------------------------------------------------------------------------------------
def _scores64(q, k, causal):
    s = np.asarray(q, np.float64) @ np.asarray(k, np.float64).T / 8
    if causal:
        s = np.where(np.arange(s.shape[1])[None, :] > np.arange(s.shape[0])[:, None], -np.inf, s)
    return s


def attn_ref(q, k, v, causal=False):
    """softmax(q k^T / 8) v of one head; q [n_q][64], k, v [n_keys][64] fp16 -> float64 [n_q][64]"""
    s = _scores64(q, k, causal)
    p = np.exp(s - s.max(axis=1, keepdims=True))
    return (p / p.sum(axis=1, keepdims=True)) @ np.asarray(v, np.float64)


def weights_ref(q, k, nF):
    """the softmax over ALL the keys, then its first nF columns; float64 [n_q][nF]"""
    s = _scores64(q, k, False)
    p = np.exp(s - s.max(axis=1, keepdims=True))
    return (p / p.sum(axis=1, keepdims=True))[:, :nF]


# ---- fp32 emulations -------------------------------------------------------------------------------------------------------------
def _scores32(q, k):
    q, k = np.asarray(q, np.float32), np.asarray(k, np.float32)
    s = np.zeros((q.shape[0], k.shape[0]), np.float32)
    for c in range(64):
        s += q[:, c, None] * k[None, :, c]
    return s * np.float32(0.125)


def _softmax32(q, k, causal=False, qpw=1, mutant=None):
    """-> (p [n_q][n_keys] fp32 numerators, 0 at the keys a query's wave never visits; sum [n_q][1] fp32 as the wave folds it)"""
    s = _scores32(q, k)
    n_q, n_keys = s.shape
    qi, j = np.arange(n_q)[:, None], np.arange(n_keys)[None, :]
    if mutant == "qpw2_second_reads_first" and qpw == 2:
        s = s[np.arange(n_q) - np.arange(n_q) % 2]
    seen = np.ones((n_q, n_keys), bool)
    if causal:  # the wave of queries q0 .. q0 + QPW - 1 stops at its last query's key
        q0 = qi - qi % qpw
        seen = j < (q0 if mutant == "causal_wave_bound_q0" else np.minimum(q0 + qpw, n_keys))
        s = np.where(j > qi + (mutant == "causal_off_by_one"), np.float32(-np.inf), s)
    with np.errstate(invalid="ignore"):
        mx = np.where(seen, s, np.float32(-np.inf)).max(axis=1, keepdims=True)
        diff = (s - mx).astype(np.float32)
        p = np.where(seen, np.exp(diff.astype(np.float64)).astype(np.float32), np.float32(0))
    return p, _wave_sum(p)


def attn_emulate(q, k, v, causal=False, qpw=1, mutant=None):
    """k_attn (and, causal False, k_attn_time) on one head -> fp16 [n_q][64]"""
    if mutant == "time_drops_keys_from_64":
        k, v = k[:64], v[:64]
    if mutant == "time_k_from_v_third":
        k = v
    p, total = _softmax32(q, k, causal, qpw, mutant)
    v = np.asarray(v, np.float32)
    o = np.zeros((p.shape[0], 64), np.float32)
    for j in range(p.shape[1]):
        o += p[:, j, None] * v[None, j]
    with np.errstate(invalid="ignore", divide="ignore"):
        return to_f16(o / total)


def weights_emulate(q, k, nF, mutant=None):
    """k_attn_weights on one head -> fp32 [n_q][nF]"""
    p, total = _softmax32(q, k)
    if mutant == "weights_over_nF":
        total = _wave_sum(p[:, :nF])
    return (p / total)[:, :nF]


def weights_bar(ref, emu):
    """fp32 output: 4 x the emulation's largest error on the case"""
    return 4 * float(np.abs(emu.astype(np.float64) - ref).max())


# ---- Whisper attention: inputs and cases ---------------------------------------------------------------------------------------
NQ_GRID = [1, 2, 3, 7, 8, 9]
NK_GRID = [1, 2, 63, 64, 65, 100, 200, 1500]
ALL_GENERATORS_AT = (65, 200)
CAUSAL_P = [1, 2, 7, 8, 9, 63, 64, 65, 130]
ANC_STEPS = [0, 1, 63, 64, 65, 447]
LDS_EDGE_KEYS = 1984  # 4 waves x QPW 2 x (1984 + 64) floats = 64 KB exactly

_inputs = {}


def wh_inputs(gen, B, W, n_q, n_keys, seed):
    """Q [B][n_q][D], K, V [W][n_keys][D] fp16: every batch's queries and every window's keys and values are their own draw of
    the generator (the structured columns of a generator are the same in every draw, so a query meets the score profile the
    generator is named for in whichever window it reads)."""
    key = (gen, B, W, n_q, n_keys, seed)
    if key not in _inputs:
        n = max(n_q, n_keys)
        Q, K, V = np.zeros((B, n_q, D), np.float16), np.zeros((W, n_keys, D), np.float16), np.zeros((W, n_keys, D), np.float16)
        for h in range(HEADS):
            c = slice(64 * h, 64 * h + 64)
            for b in range(B):
                Q[b, :, c] = attn_inputs(gen, n, seed + 1000 * h + b)[0][:n_q]
            for w in range(W):
                _, k, v = attn_inputs(gen, n, seed + 1000 * h + (w if W == B else 500 + w))
                K[w, :, c], V[w, :, c] = k[:n_keys], v[:n_keys]
        _inputs[key] = (Q, K, V)
    return _inputs[key]


def _case(name, qpw, n_q, n_keys, B, W, gen, seed, kv_div=1, kvmap=None, anc=False, causal=False, layout="encoder", nq_drawn=None):
    return dict(name=name, qpw=qpw, n_q=n_q, n_keys=n_keys, B=B, W=W, gen=gen, seed=seed, kv_div=kv_div, kvmap=kvmap, anc=anc,
                causal=causal, layout=layout, nq_drawn=nq_drawn or n_q)


def anc_table(B, seed=77):
    """[B][TM] uint8: random ancestors, with column blocks where every lane is its own ancestor and where all share lane 3"""
    t = np.random.default_rng(seed).integers(0, B, (B, TM)).astype(np.uint8)
    t[:, 8:12] = np.arange(B, dtype=np.uint8)[:, None]
    t[:, 60:66] = 3
    t[:, 0] = (np.arange(B) + 1) % B
    return t


def wh_cases():
    """Every k_attn call of the GPU test.  layout "encoder": batch stride n x D, as the encoder and the prefill call it; "decoder":
    one query per lane, q and o batch stride D, keys in a cache of TM rows per lane; "padded": encoder with o_rs = D + 8."""
    out = []
    for nk in NK_GRID:
        for gen in (ATTN_GENERATORS if nk in ALL_GENERATORS_AT else ["flat", "peaked"]):
            seed = 100000 * ATTN_GENERATORS.index(gen) + 10 * nk
            for qpw in (1, 2):
                for nq in NQ_GRID:
                    out.append(_case(f"dense {gen} qpw {qpw} n_q {nq} n_keys {nk}", qpw, nq, nk, 2, 2, gen, seed, nq_drawn=max(NQ_GRID)))
                if nk <= TM:
                    out.append(_case(f"dense-decoder {gen} qpw {qpw} n_keys {nk}", qpw, 1, nk, 2, 2, gen, seed, layout="decoder",
                                     nq_drawn=max(NQ_GRID)))
    out.append(_case("dense padded rows qpw 2 n_q 7 n_keys 65", 2, 7, 65, 2, 2, "flat", 10 * 65, layout="padded", nq_drawn=max(NQ_GRID)))
    out.append(_case(f"lds-edge qpw 2 n_keys {LDS_EDGE_KEYS}", 2, 1, LDS_EDGE_KEYS, 1, 1, "flat", 4242))
    for qpw in (1, 2):
        out.append(_case(f"kv_div qpw {qpw}", qpw, 3, 65, 6, 2, "flat", 5000, kv_div=3))
        out.append(_case(f"kvmap qpw {qpw}", qpw, 3, 65, 5, 3, "flat", 6000, kvmap=[2, 0, 2, 1, 0]))
    for s in ANC_STEPS:
        out.append(_case(f"ancestry step {s}", 1, 1, s + 1, 6, 6, "flat", 7000, anc=True, layout="decoder"))
    for P in CAUSAL_P:
        out.append(_case(f"causal P {P}", 2, P, P, 2, 2, "flat", 8000 + P, causal=True))
    return out


def wh_case_inputs(c):
    Q, K, V = wh_inputs(c["gen"], c["B"], c["W"], c["nq_drawn"], c["n_keys"], c["seed"])
    return Q[:, :c["n_q"]], K, V


def wh_case_source(c, mutant=None):
    return key_source(c["B"], c["n_keys"], c["W"], c["kv_div"], c["kvmap"], anc_table(c["B"]) if c["anc"] else None, mutant)


_expect = {}


def wh_case_expect(c):
    """[b][head] -> (ref64 [n_q][64], emulated fp16 [n_q][64]).  A query's result does not depend on the queries around it or,
    without the causal wave bound, on QPW: the cases of one draw share one computation over all the drawn queries."""
    key = (c["gen"], c["B"], c["W"], c["nq_drawn"], c["n_keys"], c["seed"], c["kv_div"], tuple(c["kvmap"] or ()), c["anc"], c["causal"],
           c["qpw"] if c["causal"] else 0)
    if key not in _expect:
        Q, K, V = wh_inputs(c["gen"], c["B"], c["W"], c["nq_drawn"], c["n_keys"], c["seed"])
        _expect[key] = _compute(c, Q, K, V, wh_case_source(c), None)
    return [[(r[:c["n_q"]], e[:c["n_q"]]) for r, e in row] for row in _expect[key]]


def _compute(c, Q, K, V, src, mutant):
    out = []
    for b in range(c["B"]):
        k, v = gather_keys(K, src[b]), gather_keys(V, src[b])
        out.append([(attn_ref(Q[b][:, h], k[:, h], v[:, h], c["causal"]),
                     attn_emulate(Q[b][:, h], k[:, h], v[:, h], c["causal"], c["qpw"], mutant))
                    for h in (slice(64 * i, 64 * i + 64) for i in range(HEADS))])
    return out


def wh_case_mutant(c, mutant):
    """[b][head] -> the mutant emulation's fp16 output on the case's own queries"""
    Q, K, V = wh_case_inputs(c)
    src = wh_case_source(c, mutant if mutant in KEY_MUTANTS else None)
    return [[e for _, e in row] for row in _compute(c, Q, K, V, src, mutant)]


# ---- k_attn_weights ----------------------------------------------------------------------------------------------------------------
W_P = [1, 4, 5, 23]
W_KEYS = [64, 100, 200, 1500]
W_ROWS, W_WINDOWS = 3, 3


def weight_cases():
    """(P, n_keys, head, nF [3], kvmap [3]) of every k_attn_weights call: nF walks through {1, 63, 64, 65, n_keys}"""
    out = []
    for i, (P, nk) in enumerate((P, nk) for P in W_P for nk in W_KEYS):
        opts = sorted({f for f in (1, 63, 64, 65, nk) if f <= nk})
        for head in (0, HEADS - 1):
            n = i + head
            out.append((P, nk, head, [opts[(n + r) % len(opts)] for r in range(W_ROWS)], [[2, 0, 1], [1, 1, 0]][n % 2]))
    return out


def weight_inputs(P, nk):
    Q, K, _ = wh_inputs("flat" if P != 5 else "peaked", W_ROWS, W_WINDOWS, P, nk, 9000 + P)
    return Q, K


def weight_expect(P, nk, head, nF, kvmap, mutant=None):
    """per row r: (ref64 [P][nF[r]], emulated fp32 [P][nF[r]])"""
    Q, K = weight_inputs(P, nk)
    c = slice(64 * head, 64 * head + 64)
    return [(weights_ref(Q[r][:, c], K[kvmap[r]][:, c], nF[r]), weights_emulate(Q[r][:, c], K[kvmap[r]][:, c], nF[r], mutant))
            for r in range(W_ROWS)]


# ---- k_attn_time ---------------------------------------------------------------------------------------------------------------
TIME_T = [1, 2, 3, 8, 63, 64, 65, 96]
TIME_HEADS = [1, 3]
TIME_SEQS = 5
TIME_ALL_GENERATORS_AT = (65, 96)


def time_cases():
    return [(g, T, heads) for T in TIME_T for heads in TIME_HEADS
            for g in (ATTN_GENERATORS if T in TIME_ALL_GENERATORS_AT else ["flat"])]


def time_qkv(gen, T, heads):
    """[TIME_SEQS][T][3 * 64 heads] fp16: q | k | v, every sequence and head its own draw, the three thirds independent"""
    return np.stack([attn_qkv(gen, T, heads, 200000 + 1000 * ATTN_GENERATORS.index(gen) + 10 * T + 100 * s) for s in range(TIME_SEQS)])


_time = {}


def time_expect(gen, T, heads):
    """[sequence][head] -> (ref64 [T][64], emulated fp16 [T][64])"""
    if (gen, T, heads) not in _time:
        _time[(gen, T, heads)] = [[(attn_ref(q, k, v), attn_emulate(q, k, v)) for q, k, v in attn_blocks(x, heads)]
                                  for x in time_qkv(gen, T, heads)]
    return _time[(gen, T, heads)]


# ---- the movers ----------------------------------------------------------------------------------------------------------------
MOVER_D = [128, 384, 1280]
MOVER_RGL = [(1, 1, 1), (2, 3, 3), (3, 1, 2)]  # (R rows, G lanes per row, lane stride from row to row)
MOVER_P = [1, 5]


def im2col_mel_ref(mel, ldk):
    """mel [B][C][T] fp32 -> col [B T][ldk] fp16: col[(b, t)][tap C + c] = mel[b][c][t + tap - 1], zero outside and from 3 C on"""
    B, C, T = mel.shape
    pad = np.zeros((B, C, T + 2), np.float32)
    pad[:, :, 1:T + 1] = mel
    col = np.zeros((B, T, ldk), np.float16)
    for tap in range(3):
        col[:, :, tap * C:(tap + 1) * C] = to_f16(pad[:, :, tap:tap + T].transpose(0, 2, 1))
    return col.reshape(B * T, ldk)


def im2col_s2_ref(h):
    """h [B][T][C] fp16 -> col [B T / 2][3 C]: col[(b, t)][tap C + c] = h[b][2 t + tap - 1][c]"""
    B, T, C = h.shape
    pad = np.zeros((B, T + 2, C), np.float16)
    pad[:, 1:T + 1] = h
    col = np.stack([pad[:, tap:tap + 2 * (T // 2):2] for tap in range(3)], axis=2)  # [B][T / 2][3][C]
    return col.reshape(B * (T // 2), 3 * C)


def embed_ref(tok, emb, pos_row):
    """x = fp32(emb[clamped id]) + pos row, one fp32 addition"""
    tok = np.clip(np.asarray(tok), 0, emb.shape[0] - 1)
    return emb[tok].astype(np.float32) + np.asarray(pos_row, np.float32)


def kv_to_cache_ref(pk, cache, R, P, G, lstride, mutant=None):
    """pk [R][P][d] into rows 0 .. P - 1 of lanes r * lstride + g of cache [lanes][Tm][d]; returns the cache after the call"""
    out = cache.copy()
    for r in range(R):
        for g in range(G):
            out[r * G + g if mutant == "cache_lane_r_G_g" else r * lstride + g, :P] = pk[r]
    return out


def gather_rows_ref(h, L, t, G):
    """h [R][P][d] -> out [L][d] = h[l / G][t]"""
    return h[np.arange(L) // G, t]
