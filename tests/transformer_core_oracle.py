"""CPU restatements of the three kernels the transformer models share (csrc/gemm_f16.h, attn_f16.h, layernorm.h), for
tests/test_transformer_core_host.py and tests/test_transformer_core_gpu.py.

Each operation comes twice, on the exact fp16 / fp32 inputs the device gets:
  * the reference: plain float64, no rounding anywhere;
  * the emulation: the same arithmetic rounded where the device rounds (fp32 accumulation, exp(s - max) rounded to fp16 before
    the PV product, the softmax sum built from the rounded values, one rounding at each fp16 output, the two-pass mean and
    variance in fp32).  Its distance from the reference is what the bars of the GPU tests are made of, and its `mutant`
    argument switches on one deliberate error at a time: the host test shows that every one of them leaves the bars.

Nothing here imports the package or needs a GPU."""
from __future__ import annotations

import numpy as np
import torch

EPI_F16, EPI_GELU_F16, EPI_RESID, EPI_GELU_POS, EPI_F32, EPI_POS, EPI_QGELU_F16, EPI_ROPE_F16, EPI_SWIGLU_F16 = range(9)
EPI_NAMES = ["EPI_F16", "EPI_GELU_F16", "EPI_RESID", "EPI_GELU_POS", "EPI_F32", "EPI_POS", "EPI_QGELU_F16", "EPI_ROPE_F16",
             "EPI_SWIGLU_F16"]
F16_OUT = {EPI_F16, EPI_GELU_F16, EPI_QGELU_F16, EPI_ROPE_F16, EPI_SWIGLU_F16}
PAIR = {EPI_ROPE_F16, EPI_SWIGLU_F16}

GEMM_MUTANTS = ["rope_pairs_adjacent", "rope_rotates_v", "pos_not_wrapped", "swiglu_swapped", "resid_overwrites"]
ATTN_MUTANTS = ["no_alpha", "pad_key_scored", "causal_off_by_one", "sum_unrounded"]
LN_MUTANTS = ["one_pass_variance", "ignores_pick"]


def half_ulp16(x):
    """Half the spacing of fp16 at the float64 values x (the subnormal spacing 2^-24 below 2^-14)."""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 11)


def to_f16(t):
    """One round-to-nearest-even to fp16, as a numpy array."""
    return torch.as_tensor(t).to(torch.float16).numpy()


# ---- GEMM ------------------------------------------------------------------------------------------------------------------
def gemm_sum(A, W, emulate):
    """A [M][K] . W [N][K]^T.  float64, or fp32: the fp16 products are exact in fp32 and are added one k after the other."""
    if not emulate:
        return A.astype(np.float64) @ W.astype(np.float64).T
    a, w = A.astype(np.float32), W.astype(np.float32)
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    for k in range(A.shape[1]):
        acc += a[:, k, None] * w[None, :, k]
    return acc


def _gelu(v):
    return 0.5 * v * (1 + torch.erf(v * 0.70710678118654752))


def _rope(C, table, row_pos, mutant):
    """Packed q | k | v, N = 3 d.  Within each 64-row head of q and k, stored row 2j is the head's dimension j and stored row
    2j + 1 its dimension j + 32: take the head to its own order, rotate as rotate_half does (x cos + rotate_half(x) sin with
    the angle of (row_pos[m], j) for dimensions j and j + 32), and put it back in the stored order.  v passes through."""
    M, N = C.shape
    d = N // 3
    stored = torch.cat([torch.arange(0, 64, 2), torch.arange(1, 64, 2)])  # stored row of dimension 0 .. 63
    ang = table[row_pos.long()]  # [M][64]: cos | sin
    cos, sin = ang[:, None, :32], ang[:, None, 32:]
    out = C.clone()
    thirds = 3 if mutant == "rope_rotates_v" else 2
    x = C[:, :thirds * d].reshape(M, thirds * d // 64, 64)[:, :, stored]
    if mutant == "rope_pairs_adjacent":  # partners (2i, 2i + 1) with the angle i
        lo, hi = x[:, :, 0::2], x[:, :, 1::2]
        y = torch.stack([lo * cos - hi * sin, hi * cos + lo * sin], dim=-1).reshape(x.shape)
    else:
        lo, hi = x[:, :, :32], x[:, :, 32:]
        y = torch.cat([lo * cos - hi * sin, hi * cos + lo * sin], dim=-1)
    back = torch.empty_like(y)
    back[:, :, stored] = y
    out[:, :thirds * d] = back.reshape(M, thirds * d)
    return out


def gemm_epilogue(epi, C, bias=None, out0=None, pos=None, pos_rows=1, row_pos=None, mutant=None):
    """The value each epilogue stores, before any rounding to fp16, in C's precision (float64: the reference; float32: the
    emulation, every operation rounded to fp32 in the kernel's order).  C [M][N] is the k-sum; returns [M][N], or [M][N / 2]
    for EPI_SWIGLU_F16."""
    C = torch.as_tensor(C)
    dt = C.dtype
    cast = lambda a: None if a is None else torch.as_tensor(a).to(dt)
    bias, out0, pos = cast(bias), cast(out0), cast(pos)
    M, N = C.shape
    if epi == EPI_ROPE_F16:
        return _rope(C, pos, torch.as_tensor(row_pos), mutant)
    if epi == EPI_SWIGLU_F16:  # stored row 2i is gate row i, 2i + 1 up row i
        gate, up = C[:, 0::2], C[:, 1::2]
        if mutant == "swiglu_swapped":
            gate, up = up, gate
        return gate / (1 + torch.exp(-gate)) * up
    v = C if bias is None else C + bias
    if epi in (EPI_F16, EPI_F32):
        return v
    if epi == EPI_GELU_F16:
        return _gelu(v)
    if epi == EPI_QGELU_F16:
        return v / (1 + torch.exp(torch.tensor(-1.702, dtype=dt) * v))
    if epi == EPI_RESID:
        return v.clone() if mutant == "resid_overwrites" else out0 + v
    rows = torch.arange(M)
    rows = rows.clamp(max=pos_rows - 1) if mutant == "pos_not_wrapped" else rows % pos_rows
    table = pos.reshape(pos_rows, N)[rows]
    return (_gelu(v) if epi == EPI_GELU_POS else v) + table


# ---- attention ---------------------------------------------------------------------------------------------------------------
def attn_ref(q, k, v, causal):
    """softmax(q k^T / 8) v of one head of one sequence; q, k, v fp16 [n][64] -> float64 [n][64]"""
    q, k, v = (torch.as_tensor(t).double() for t in (q, k, v))
    s = q @ k.T / 8
    if causal:
        n = s.shape[0]
        s = s.masked_fill(torch.arange(n)[None, :] > torch.arange(n)[:, None], -np.inf)
    return (torch.softmax(s, dim=1) @ v).numpy()


def attn_emulate(q, k, v, causal, mutant=None):
    """The kernel's online softmax, 32 keys at a time: fp32 scores, the running maximum, alpha = exp(old max - new max) on the
    accumulator and the sum, p = exp(s - max) rounded to fp16 for both the PV product and the sum, fp32 accumulation, one
    rounding of acc / sum to fp16.  -> fp16 [n][64]"""
    q, k, v = (torch.as_tensor(t).float() for t in (q, k, v))
    n = q.shape[0]
    seen_n = n
    if mutant == "pad_key_scored":  # the zero row staged after the last key takes part: score 0, value 0
        k, v, seen_n = torch.cat([k, torch.zeros(1, 64)]), torch.cat([v, torch.zeros(1, 64)]), n + 1
    qi = torch.arange(n)[:, None]
    acc, total = torch.zeros(n, 64), torch.zeros(n)
    mx = torch.full((n,), -np.inf)
    for j0 in range(0, seen_n, 32):
        j1 = min(j0 + 32, seen_n)
        s = (q @ k[j0:j1].T) * 0.125
        if causal:
            s = s.masked_fill(torch.arange(j0, j1)[None, :] > qi + (1 if mutant == "causal_off_by_one" else 0), -np.inf)
        m_new = torch.maximum(mx, s.max(dim=1).values)
        alpha = torch.ones(n) if mutant == "no_alpha" and j0 else torch.exp(mx - m_new)
        mx = m_new
        e = torch.exp(s - m_new[:, None])
        p = e.half().float()
        total = total * alpha + (e if mutant == "sum_unrounded" else p).sum(dim=1)
        acc = acc * alpha[:, None] + p @ v[j0:j1]
    return (acc / total[:, None]).half().numpy()


ATTN_GENERATORS = ["flat", "peaked", "rising", "falling", "late_spike", "offset_v", "half_bias"]


def attn_inputs(gen, n, seed):
    """One head of one sequence, fp16 q, k, v [n][64]:
      flat        scores with std ~ 1: the regime of the random models
      peaked      q and k scaled by sqrt(8): scores with std ~ 8, most numerators fp16-subnormal or zero
      rising      the score of key j grows by 0.25 per key: the running maximum moves in every 32-key group and stage
      falling     falls by 0.25 per key: the maximum is at key 0
      late_spike  one key of the last 32-key group exceeds every other by about 30
      offset_v    flat scores, values 100 + unit noise
      half_bias   every query scores key 0 at 0 and every other key at ln(0.5 + 0.9 * 2^-12): each numerator rounds DOWN to
                  0.5 in fp16, and every value is 128.  With the sum built from the rounded numerators the result is 128 exactly
                  (the emulation's error is zero); with the unrounded ones it falls below 128 (1 - 2^-12), to the next fp16."""
    rng = np.random.default_rng(seed)
    q, k, v = (rng.standard_normal((n, 64)) for _ in range(3))
    j = np.arange(n)
    if gen == "peaked":
        q, k = q * np.sqrt(8), k * np.sqrt(8)
    elif gen in ("rising", "falling"):
        q[:, 0], k[:, 0] = 8, (0.25 if gen == "rising" else -0.25) * j
    elif gen == "late_spike":
        q[:, 0], k[:, 0] = 4, 0
        k[n - 1 - ((n - 1) % 32) // 2, 0] = 64  # 4 * 64 / 8 = 32 above its neighbours' level
    elif gen == "offset_v":
        v = v + 100
    elif gen == "half_bias":
        target = 8 * np.log(0.5 + 0.9 * 2.0 ** -12)  # q . k of every key but key 0
        a = float(np.float16(target))
        b = float(np.float16((target - a) * 64))
        q, k, v = np.zeros((n, 64)), np.zeros((n, 64)), np.full((n, 64), 128.0)
        q[:, 0], q[:, 1] = 1, 1 / 64
        k[1:, 0], k[1:, 1] = a, b
    elif gen != "flat":
        raise ValueError(gen)
    return tuple(t.astype(np.float16) for t in (q, k, v))


def attn_qkv(gen, n, heads, seed):
    """qkv [n][3 * 64 heads] of one sequence: head h from attn_inputs(gen, n, seed + h)"""
    parts = [attn_inputs(gen, n, seed + h) for h in range(heads)]
    return np.concatenate([np.concatenate([p[i] for p in parts], axis=1) for i in range(3)], axis=1)


def attn_blocks(qkv, heads):
    """the (q, k, v) of every head of a sequence's qkv rows"""
    d = 64 * heads
    return [tuple(qkv[:, i * d + 64 * h:i * d + 64 * h + 64] for i in range(3)) for h in range(heads)]


def block_errors(got, ref):
    """(mean, max) of |got - ref| as fractions of the block's reference RMS: the project's fp16 rule on one head of one sequence"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    rms = float(np.sqrt((ref ** 2).mean()))
    return float(err.mean()) / rms, float(err.max()) / rms


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------
def ln_ref(x, g, b, eps, pick=None):
    """float64 LayerNorm of the fp32 rows x [.][d]; output row r normalises row pick[r]"""
    x = np.asarray(x, np.float64)
    if pick is not None:
        x = x[np.asarray(pick)]
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
    return (x - mean) / np.sqrt(var + np.float64(np.float32(eps))) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def _wave_sum(x):
    """The sum of the rows of x [rows][d] as one wave forms it: lane l adds elements l, l + 64, ... in order, then the xor
    butterfly 32, 16, ... 1.  fp32 throughout."""
    rows, d = x.shape
    pad = np.zeros((rows, -(-d // 64) * 64), np.float32)
    pad[:, :d] = x
    lanes = np.zeros((rows, 64), np.float32)
    for c in range(pad.shape[1] // 64):
        lanes += pad[:, 64 * c:64 * c + 64]
    o = 32
    while o:
        lanes = lanes + lanes[:, np.arange(64) ^ o]
        o >>= 1
    return lanes[:, :1]


def ln_emulate(x, g, b, eps, pick=None, mutant=None):
    """fp32 as the kernel does it: the mean first, then the centred sum of squares, 1 / sqrt(var + eps), (x - mean) * inv * g + b.
    -> fp32 [M][d] before the store (the fp16 output is its one rounding)"""
    x = np.asarray(x, np.float32)
    if pick is not None and mutant != "ignores_pick":
        x = x[np.asarray(pick)]
    elif pick is not None:
        x = x[:len(pick)]
    d = np.float32(x.shape[1])
    mean = _wave_sum(x) / d
    if mutant == "one_pass_variance":
        var = _wave_sum(x * x) / d - mean * mean
    else:
        c = x - mean
        var = _wave_sum(c * c) / d
    inv = np.float32(1) / np.sqrt(var + np.float32(eps))
    return (x - mean) * inv * np.asarray(g, np.float32) + np.asarray(b, np.float32)


LN_INPUTS = ["unit", "offset", "constant", "var_eps"]


def ln_inputs(kind, rows, d, eps, seed):
    """fp32 rows [rows][d]: unit normal; mean = 1000 x std; constant rows (2.5: every partial sum is exact, so the mean is
    the value and the output is b); rows whose variance is eps x (0.5 .. 2)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, d))
    if kind == "offset":
        x += 1000
    elif kind == "constant":
        x[:] = 2.5
    elif kind == "var_eps":
        x -= x.mean(axis=1, keepdims=True)
        x *= np.sqrt(eps * np.linspace(0.5, 2.0, rows))[:, None] / x.std(axis=1, keepdims=True)
    elif kind != "unit":
        raise ValueError(kind)
    return x.astype(np.float32)


# ---- the case tables, shared by the host test (emulation and mutants against the bars) and the GPU test (the device) ----------
# the (MT, EPI) pairs the models instantiate; the host test pins it to the probe's table and to the models' sources
GEMM_TABLE = [(1, EPI_F16), (4, EPI_F16), (1, EPI_GELU_F16), (4, EPI_GELU_F16), (1, EPI_RESID), (4, EPI_RESID), (4, EPI_GELU_POS),
              (1, EPI_F32), (4, EPI_F32), (4, EPI_POS), (4, EPI_QGELU_F16), (4, EPI_ROPE_F16), (4, EPI_SWIGLU_F16)]
GEMM_M = [0, 1, 15, 16, 17, 63, 64, 65, 130]
GEMM_N = [7, 16, 48, 64, 80, 200]
GEMM_K = [32, 96, 608]
GEMM_ROWS = max(GEMM_M)
ROPE_ROWS = 40


def gemm_widths(epi):
    if epi == EPI_ROPE_F16:
        return [192, 384]  # d = 64 and 128: one and two heads per third
    if epi == EPI_SWIGLU_F16:
        return [n for n in GEMM_N if n % 16 == 0] + [256]  # F = 8, 24, 32, 40, 128
    return GEMM_N


_problems = {}


def gemm_problem(N, K):
    """The inputs every epilogue shares at one (N, K), and the k-sums of all GEMM_ROWS rows in both precisions: a case with M
    rows uses the first M (a row's sum does not depend on the rows around it)."""
    if (N, K) not in _problems:
        rng = np.random.default_rng(1000 * N + K)
        p = dict(A=rng.standard_normal((GEMM_ROWS, K)).astype(np.float16),
                 W=(rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float16),
                 bias=rng.standard_normal(N).astype(np.float32),
                 out0=rng.standard_normal((GEMM_ROWS, N)).astype(np.float32),
                 pos=rng.standard_normal((GEMM_ROWS, N)).astype(np.float32))  # the first pos_rows rows are the table
        ang = rng.uniform(0, 2 * np.pi, (ROPE_ROWS, 32))
        p["rope"] = np.concatenate([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)
        p["row_pos"] = rng.integers(0, ROPE_ROWS, GEMM_ROWS).astype(np.int32)  # shuffled, with repeats
        p["row_pos"][0] = ROPE_ROWS - 1
        p["C64"], p["C32"] = gemm_sum(p["A"], p["W"], False), gemm_sum(p["A"], p["W"], True)
        _problems[(N, K)] = p
    return _problems[(N, K)]


def gemm_cases(epi):
    """(M, N, K, pos_rows, lda, ldc) of every case of one epilogue: the grid, then lda = K + 8 and ldc = N + 24 once each"""
    out = []
    for N in gemm_widths(epi):
        for K in GEMM_K:
            for M in GEMM_M:
                ldc = N // 2 if epi == EPI_SWIGLU_F16 else N
                if epi in (EPI_POS, EPI_GELU_POS) and M:
                    out += [(M, N, K, pr, K, ldc) for pr in sorted({1, 5, M})]
                else:
                    out.append((M, N, K, ROPE_ROWS if epi == EPI_ROPE_F16 else 1, K, ldc))
    N = gemm_widths(epi)[-2]  # 80; 192 for ROPE
    pr = ROPE_ROWS if epi == EPI_ROPE_F16 else 5
    return out + [(65, N, 96, pr, 96 + 8, N // 2 if epi == EPI_SWIGLU_F16 else N), (65, N, 96, pr, 96, N + 24)]


def gemm_expect(epi, M, N, K, pos_rows, mutant=None):
    """-> (ref64, bar32, emulated output) of one case: ref64 [M][columns] float64, bar32 = 4 x the fp32 emulation's largest
    error against it, and what the emulation (or its mutant) stores"""
    p = gemm_problem(N, K)
    kw = {}
    if epi not in PAIR:
        kw["bias"] = p["bias"]
    if epi == EPI_RESID:
        kw["out0"] = p["out0"][:M]
    if epi in (EPI_POS, EPI_GELU_POS):
        kw.update(pos=p["pos"][:pos_rows], pos_rows=pos_rows)
    if epi == EPI_ROPE_F16:
        kw.update(pos=p["rope"], pos_rows=ROPE_ROWS, row_pos=p["row_pos"][:M])
    ref = gemm_epilogue(epi, p["C64"][:M], **kw).numpy()
    e32 = gemm_epilogue(epi, p["C32"][:M], **kw).numpy()
    bar32 = 4 * float(np.abs(e32.astype(np.float64) - ref).max()) if M else 0.0
    em = e32 if mutant is None else gemm_epilogue(epi, p["C32"][:M], mutant=mutant, **kw).numpy()
    return ref, bar32, (to_f16(em) if epi in F16_OUT else em)


def gemm_within_bar(epi, got, ref, bar32):
    """fp32 outputs: max error <= bar32.  fp16 outputs: per element, half an fp16 ulp of the reference more.
    -> (ok, largest error, the bar at that element)"""
    if got.size == 0:
        return True, 0.0, 0.0
    err = np.abs(got.astype(np.float64) - ref)
    bar = bar32 + (half_ulp16(ref) if epi in F16_OUT else 0.0) + np.zeros_like(err)
    i = np.unravel_index(np.argmax(err - bar), err.shape)
    return bool((err <= bar).all()), float(err[i]), float(bar[i])


ATTN_HEADS = 2
ATTN_N = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 160, 257]
ATTN_ALL_GENERATORS_AT = (33, 129, 257)
RAGGED_LENGTHS = [(1, 3, 17, 65, 130, 64, 128), (130, 1, 128, 3, 64, 17, 65), (64, 65, 3, 128, 1, 130, 17)]
SPACETIME_SHAPES = [(2, 9, 3), (1, 4, 5), (1, 196, 2)]


def attn_dense_cases():
    """(generator, n) of every dense call (3 sequences, 2 heads, causal and not)"""
    return [(g, n) for n in ATTN_N for g in (ATTN_GENERATORS if n in ATTN_ALL_GENERATORS_AT else ["flat"])]


def attn_seed(gen, n, s):
    return 100000 * ATTN_GENERATORS.index(gen) + 100 * n + 10 * s


_attn = {}


def attn_expect(qkv, causal, key=None):
    """Per head of one sequence's qkv rows: (ref64, the emulation's fp16 output).  `key` caches the result."""
    if key is None or (key, causal) not in _attn:
        r = [(attn_ref(q, k, v, causal), attn_emulate(q, k, v, causal)) for q, k, v in attn_blocks(qkv, ATTN_HEADS)]
        if key is None:
            return r
        _attn[(key, causal)] = r
    return _attn[(key, causal)]


def attn_within_bar(got, ref, emu):
    """One head of one sequence: mean and max error as fractions of the block's RMS <= 2 x the emulation's; where the emulation
    has no error at all, the bits of fp16(ref).  -> (ok, (mean, max) of got, (mean, max) of the emulation)"""
    g, e = block_errors(got, ref), block_errors(emu, ref)
    if e[1] == 0.0:
        return bool(np.array_equal(np.asarray(got, np.float16).view(np.uint16), to_f16(ref).view(np.uint16))), g, e
    return g[0] <= 2 * e[0] and g[1] <= 2 * e[1], g, e


def spacetime_qkv(B, P, T, seed):
    """flat qkv [B P T + B][3 * 64 heads] in TimeSformer's stream order and, per problem z = b T + t, the rows of its tokens"""
    rows = B * P * T + B
    qkv = attn_qkv("flat", rows, ATTN_HEADS, seed)
    idx = [[B * P * T + b] + [(b * P + p) * T + t for p in range(P)] for b in range(B) for t in range(T)]
    return qkv, idx


LN_D = [64, 96, 128, 768, 1280]
LN_M = [1, 3, 4, 5, 9]
LN_EPS = [1e-5, 1e-6, 1e-12]
LN_PICKS = ["none", "reversed", "repeated"]
LN_SRC_ROWS = 12


def ln_pick(kind, M):
    if kind == "none":
        return None
    if kind == "reversed":
        return np.arange(LN_SRC_ROWS - 1, LN_SRC_ROWS - 1 - M, -1).astype(np.int32)
    return np.array([(7 * r // 2) % LN_SRC_ROWS if r % 3 else 5 for r in range(M)], np.int32)  # row 5 again and again


def ln_case(kind, d, eps, seed=0):
    """x [LN_SRC_ROWS][d], g, b of one LayerNorm input"""
    rng = np.random.default_rng(7 * d + seed)
    x = ln_inputs(kind, LN_SRC_ROWS, d, eps, 13 * d + LN_INPUTS.index(kind))
    return x, (1 + 0.5 * rng.standard_normal(d)).astype(np.float32), rng.standard_normal(d).astype(np.float32)


def ln_expect(x, g, b, eps, pick, M, mutant=None):
    """-> (ref64 [M][d], bar32 = 4 x the fp32 emulation's largest error, the emulation's (or mutant's) fp32 values)"""
    src = x if pick is not None else x[:M]
    ref = ln_ref(src, g, b, eps, pick)
    e32 = ln_emulate(src, g, b, eps, pick)
    bar32 = 4 * float(np.abs(e32.astype(np.float64) - ref).max())
    return ref, bar32, (e32 if mutant is None else ln_emulate(src, g, b, eps, pick, mutant))


def ln_within_bar(f16, got, ref, bar32):
    err = np.abs(got.astype(np.float64) - ref)
    bar = bar32 + (half_ulp16(ref) if f16 else 0.0) + np.zeros_like(err)
    i = np.unravel_index(np.argmax(err - bar), err.shape)
    return bool((err <= bar).all()), float(err[i]), float(bar[i])
