"""GPU: k_gemm, k_attn_tiles and k_ln (csrc/gemm_f16.h, attn_f16.h, layernorm.h), one kernel at a time, against the float64
restatements of tests/transformer_core_oracle.py.  libeioku_hip_probe.so (csrc/probe/transformer_probe.hip) includes the three
headers unchanged and exports one entry point per kernel; the product never loads it.

Bars (tests/test_transformer_core_host.py shows that the emulation keeps them and that eleven wrong kernels would not):
  fp32 outputs   max |got - ref64| <= 4 x the largest error of the fp32 emulation on the same case (K22's rule)
  fp16 outputs   per element, half an fp16 ulp of ref64 more
  attention      per head and per sequence: mean and max of |got - ref64| as fractions of the block's reference RMS <= 2 x the
                 emulation's on the same block; equal bits where the emulation has no error
Stores: every output buffer is larger than the result and pre-filled with a NaN bit pattern; whatever lies outside the
documented region (rows >= M, columns >= N up to ldc, rows of no sequence, the other output of SpaceTimeSeq) must still hold it."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import transformer_core_oracle as o

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "eioku_amd" / "libeioku_hip_probe.so"
pytestmark = pytest.mark.gpu

S16, S32 = 0x7DDD, 0x7FC0DEAD  # fp16 / fp32 NaNs no kernel produces
EINVAL = -1
DENSE, RAGGED, SPACETIME = 0, 1, 2


@pytest.fixture(scope="module")
def probe(gpu):
    assert LIB.exists(), "build it: make -C eioku_amd/csrc (target all builds the probe library too)"
    lib = C.CDLL(str(LIB))
    p, i, ll, f = C.c_void_p, C.c_int, C.c_longlong, C.c_float
    lib.eioku_probe_gemm.argtypes = [i, i, p, i, p, i, p, i, i, i, p, ll, p, i, p, p]
    lib.eioku_probe_attn.argtypes = [i, i, p, i, i, i, i, p, i, i, i, p, p, p]
    lib.eioku_probe_ln.argtypes = [i, p, i, i, p, p, f, p, p, p]
    lib.eioku_last_error.restype = C.c_char_p
    assert lib.eioku_init(0) == 0, lib.eioku_last_error()  # the probe links its own core.o: its own state
    return lib


@pytest.fixture(scope="module")
def report():
    """name -> [largest device figure, largest bar]; printed once the module is through (pytest -s)"""
    rows = {}
    yield rows
    for name in sorted(rows):
        print(f"\n[transformer core] {name}: " + ", ".join(f"{k} {v:.3e}" for k, v in rows[name].items()), end="")
    print()


def _note(report, name, **figures):
    r = report.setdefault(name, {})
    for k, v in figures.items():
        r[k] = max(r.get(k, 0.0), float(v))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _sentinel(n, f16):
    return torch.full((n,), S16 if f16 else S32, dtype=torch.int16 if f16 else torch.int32, device="cuda")


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint16 if a.dtype == np.int16 else np.uint32)


def _values(bits):
    return bits.view(np.float16 if bits.dtype == np.uint16 else np.float32)


# ---- GEMM -------------------------------------------------------------------------------------------------------------------
_gemm_dev = {}


def _gemm_inputs(N, K, lda):
    """device copies of gemm_problem(N, K); the columns K .. lda of A hold NaN"""
    if (N, K, lda) not in _gemm_dev:
        p = o.gemm_problem(N, K)
        A = np.full((o.GEMM_ROWS, lda), np.nan, np.float16)
        A[:, :K] = p["A"]
        _gemm_dev[(N, K, lda)] = {k: _dev(v) for k, v in dict(p, A=A).items() if k not in ("C64", "C32")}
    return _gemm_dev[(N, K, lda)]


def _gemm(probe, mt, epi, M, N, K, pos_rows, lda, ldc, row0=0):
    """One call on rows row0 .. row0 + M - 1 of the problem.  -> (rc, bits of the whole output buffer [M + 3][ldc], columns)"""
    d = _gemm_inputs(N, K, lda)
    f16 = epi in o.F16_OUT
    cols = N // 2 if epi == o.EPI_SWIGLU_F16 else N
    out = _sentinel((M + 3) * ldc, f16).view(M + 3, ldc)
    if epi == o.EPI_RESID and cols <= ldc:
        out[:M, :cols] = d["out0"][row0:row0 + M].view(torch.int32)
    pos, row_pos = None, None
    if epi in (o.EPI_POS, o.EPI_GELU_POS):
        pos = d["pos"]
    if epi == o.EPI_ROPE_F16:
        pos, row_pos = d["rope"], d["row_pos"][row0:]
    rc = probe.eioku_probe_gemm(mt, epi, _ptr(d["A"][row0:]), lda, _ptr(d["W"]), K, _ptr(None if epi in o.PAIR else d["bias"]), M, N, K,
                                _ptr(out), ldc, _ptr(pos), pos_rows, _ptr(row_pos), None)
    return rc, _bits(out), cols


def _only_sentinel(bits):
    return bool((bits == (S16 if bits.dtype == np.uint16 else S32)).all())


@pytest.mark.parametrize("mt,epi", o.GEMM_TABLE, ids=[f"MT{m}-{o.EPI_NAMES[e]}" for m, e in o.GEMM_TABLE])
def test_gemm_matches_float64_on_the_grid(probe, report, mt, epi):
    name = f"k_gemm<{mt}, {o.EPI_NAMES[epi]}>"
    for M, N, K, pos_rows, lda, ldc in o.gemm_cases(epi):
        case = f"{name} M {M} N {N} K {K} pos_rows {pos_rows} lda {lda} ldc {ldc}"
        rc, bits, cols = _gemm(probe, mt, epi, M, N, K, pos_rows, lda, ldc)
        assert rc == 0, f"{case}: {probe.eioku_last_error()}"
        assert _only_sentinel(bits[M:]) and _only_sentinel(bits[:, cols:]), f"{case}: a store outside [M][{cols}]"
        if M == 0:
            continue
        ref, bar32, _ = o.gemm_expect(epi, M, N, K, pos_rows)
        ok, err, bar = o.gemm_within_bar(epi, _values(bits[:M, :cols]), ref, bar32)
        _note(report, name, err=err, bar=bar)
        assert ok, f"{case}: error {err:.3e} > bar {bar:.3e} (4 x fp32 emulation {bar32:.3e})"


@pytest.mark.parametrize("mt,epi", o.GEMM_TABLE, ids=[f"MT{m}-{o.EPI_NAMES[e]}" for m, e in o.GEMM_TABLE])
def test_gemm_row_does_not_depend_on_the_batch_around_it(probe, mt, epi):
    """gemm_f16.h: "each output element is one k-ordered sum whatever M is".  In bits: a row of the M = 130 call equals the row
    computed alone, and the whole call equals the other MT's where the models use both."""
    N, K, M = o.gemm_widths(epi)[-2], 96, 130
    pos_rows = o.ROPE_ROWS if epi == o.EPI_ROPE_F16 else 1
    ldc = N // 2 if epi == o.EPI_SWIGLU_F16 else N
    rc, whole, cols = _gemm(probe, mt, epi, M, N, K, pos_rows, K, ldc)
    assert rc == 0
    for m in (0, 17, 64, 129):
        rc, alone, _ = _gemm(probe, mt, epi, 1, N, K, pos_rows, K, ldc, row0=m)
        assert rc == 0 and np.array_equal(alone[0], whole[m]), f"row {m} alone differs from row {m} of M = 130"
    other = 5 - mt
    if (other, epi) in o.GEMM_TABLE:
        rc, twin, _ = _gemm(probe, other, epi, M, N, K, pos_rows, K, ldc)
        assert rc == 0 and np.array_equal(twin, whole), f"MT {other} differs from MT {mt}"


@pytest.mark.parametrize("N", [192, 384])
def test_rope_writes_the_v_third_as_epi_f16_does(probe, N):
    M, K = 65, 96
    _, rope, _ = _gemm(probe, 4, o.EPI_ROPE_F16, M, N, K, o.ROPE_ROWS, K, N)
    d = _gemm_inputs(N, K, K)
    out = _sentinel(M * N, True).view(M, N)
    assert probe.eioku_probe_gemm(4, o.EPI_F16, _ptr(d["A"]), K, _ptr(d["W"]), K, None, M, N, K, _ptr(out), N, None, 1, None, None) == 0
    plain = _bits(out)
    assert np.array_equal(rope[:M, 2 * N // 3:], plain[:, 2 * N // 3:])
    assert not np.array_equal(rope[:M, :2 * N // 3], plain[:, :2 * N // 3])


@pytest.mark.parametrize("mt,epi", o.GEMM_TABLE, ids=[f"MT{m}-{o.EPI_NAMES[e]}" for m, e in o.GEMM_TABLE])
def test_gemm_refuses_what_the_kernel_cannot_address(probe, mt, epi):
    N = 192 if epi == o.EPI_ROPE_F16 else 64
    ldc = N // 2 if epi == o.EPI_SWIGLU_F16 else N
    big = _dev(np.zeros((o.GEMM_ROWS, 1024), np.float16))  # large enough for whatever a refused call might have read
    cases = [(dict(K=48), "GEMM K 48 / lda 48 / ldw 48 misaligned"),
             (dict(K=96, lda=100), "GEMM K 96 / lda 100 / ldw 96 misaligned"),
             (dict(K=96, ldw=100), "GEMM K 96 / lda 96 / ldw 100 misaligned")]
    if epi in o.PAIR:
        cases += [(dict(K=96, N=40, ldc=40), "GEMM K 96 / N 40 / ldc 40 misaligned"),
                  (dict(K=96, ldc=N + 2), f"GEMM K 96 / N {N} / ldc {N + 2} misaligned")]
    for kw, message in cases:
        K = kw["K"]
        n = kw.get("N", N)
        d = _gemm_inputs(192 if epi == o.EPI_ROPE_F16 else 64, 96, 96)
        out = _sentinel(20 * 512, epi in o.F16_OUT)
        rc = probe.eioku_probe_gemm(mt, epi, _ptr(big), kw.get("lda", K), _ptr(big), kw.get("ldw", K), None, 16, n, K, _ptr(out),
                                    kw.get("ldc", ldc), _ptr(d["pos"] if epi != o.EPI_ROPE_F16 else d["rope"]), 1, _ptr(d["row_pos"]), None)
        assert rc == EINVAL and probe.eioku_last_error().decode() == message, (kw, rc, probe.eioku_last_error())
        assert _only_sentinel(_bits(out)), kw


def test_probe_dispatches_only_what_the_models_instantiate(probe):
    d = _gemm_inputs(64, 96, 96)
    out = _sentinel(16 * 64, False)
    for mt, epi in [(2, o.EPI_F16), (1, o.EPI_POS), (1, o.EPI_ROPE_F16), (4, 9), (8, o.EPI_F32)]:
        rc = probe.eioku_probe_gemm(mt, epi, _ptr(d["A"]), 96, _ptr(d["W"]), 96, None, 16, 64, 96, _ptr(out), 64, _ptr(d["pos"]), 1,
                                    _ptr(d["row_pos"]), None)
        assert rc == EINVAL and b"no model instantiates" in probe.eioku_last_error(), (mt, epi)
        assert _only_sentinel(_bits(out))


# ---- attention -----------------------------------------------------------------------------------------------------------------
D = 64 * o.ATTN_HEADS


def _attn(probe, policy, causal, qkv, sequences, longest, out_rows, cu=None, shape=(0, 0, 0), cls_rows=0):
    """-> (bits of out [out_rows + 2][D], bits of out_cls [cls_rows + 2][D])"""
    x = _dev(qkv)
    out, cls = _sentinel((out_rows + 2) * D, True).view(-1, D), _sentinel((cls_rows + 2) * D, True).view(-1, D)
    cu_dev = None if cu is None else _dev(np.asarray(cu, np.int32))
    rc = probe.eioku_probe_attn(policy, int(causal), _ptr(x), o.ATTN_HEADS, sequences, longest, longest if policy == DENSE else 0,
                                _ptr(cu_dev), *shape, _ptr(out), _ptr(cls), None)
    assert rc == 0, probe.eioku_last_error()
    return _bits(out), _bits(cls)


def _check_blocks(report, name, label, got_bits, qkv, causal, key):
    """one sequence: both heads' columns against their own reference"""
    for h, (ref, emu) in enumerate(o.attn_expect(qkv, causal, key)):
        ok, g, e = o.attn_within_bar(_values(got_bits[:, 64 * h:64 * h + 64]), ref, emu)
        _note(report, name, mean=g[0], mean_bar=2 * e[0], max=g[1], max_bar=2 * e[1])
        assert ok, f"{label} head {h}: mean / max error over the block's RMS {g[0]:.3e} / {g[1]:.3e}, emulation {e[0]:.3e} / {e[1]:.3e}"


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("gen,n", o.attn_dense_cases(), ids=[f"{g}-{n}" for g, n in o.attn_dense_cases()])
def test_dense_attention_matches_float64_per_head_and_sequence(probe, report, gen, n, causal):
    seqs = [o.attn_qkv(gen, n, o.ATTN_HEADS, o.attn_seed(gen, n, s)) for s in range(3)]
    out, cls = _attn(probe, DENSE, causal, np.concatenate(seqs), 3, n, 3 * n)
    assert _only_sentinel(out[3 * n:]) and _only_sentinel(cls)
    for s in range(3):
        _check_blocks(report, f"k_attn_tiles dense {'causal' if causal else 'full'} {gen}", f"{gen} n {n} sequence {s}",
                      out[s * n:(s + 1) * n], seqs[s], causal, (gen, n, o.attn_seed(gen, n, s)))


def _ragged_seq(n):
    return o.attn_qkv("flat", n, o.ATTN_HEADS, o.attn_seed("flat", n, 7))


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_ragged_attention_matches_float64_and_does_not_depend_on_the_packing(probe, report, causal):
    """The three packings hold the same sequences in different orders, the third from row 2 on (rows 0 and 1 belong to no
    sequence): every sequence within its bar, and with the same bits in all three and alone."""
    first = {}
    for i, lengths in enumerate(o.RAGGED_LENGTHS):
        start = 2 if i == 2 else 0
        cu = np.concatenate([[start], start + np.cumsum(lengths)])
        qkv = np.concatenate([np.zeros((start, 3 * D), np.float16)] + [_ragged_seq(n) for n in lengths])
        out, _ = _attn(probe, RAGGED, causal, qkv, len(lengths), max(lengths), cu[-1], cu=cu)
        assert _only_sentinel(out[:start]) and _only_sentinel(out[cu[-1]:])
        for z, n in enumerate(lengths):
            got = out[cu[z]:cu[z + 1]]
            if i == 0:
                _check_blocks(report, f"k_attn_tiles ragged {'causal' if causal else 'full'}", f"ragged n {n}", got, _ragged_seq(n), causal,
                              ("flat", n, o.attn_seed("flat", n, 7)))
                first[n] = got
            assert np.array_equal(got, first[n]), f"packing {i}: the sequence of {n} tokens differs from packing 0"
    for n in (17, 130):
        out, _ = _attn(probe, RAGGED, causal, _ragged_seq(n), 1, n, n, cu=[0, n])
        assert np.array_equal(out[:n], first[n]), f"the sequence of {n} tokens alone differs from itself in the batch"


@pytest.mark.parametrize("i", range(len(o.SPACETIME_SHAPES)), ids=[str(s) for s in o.SPACETIME_SHAPES])
def test_spacetime_attention_matches_float64_and_keeps_its_two_outputs_apart(probe, report, i):
    B, P, T = o.SPACETIME_SHAPES[i]
    qkv, idx = o.spacetime_qkv(B, P, T, 50 + i)
    out, cls = _attn(probe, SPACETIME, False, qkv, B * T, 1 + P, B * P * T + B, shape=(B, P, T), cls_rows=B * T)
    assert _only_sentinel(out[B * P * T:]) and _only_sentinel(cls[B * T:])  # the CLS rows of the stream are no patch output
    for z, rows in enumerate(idx):
        got = np.concatenate([cls[z:z + 1], out[rows[1:]]])
        _check_blocks(report, "k_attn_tiles space-time", f"(B, P, T) {(B, P, T)} problem {z}", got, qkv[rows], False, ("st", i, z))


@pytest.mark.parametrize("n", [17, 65, 130])
def test_the_three_policies_give_the_same_bits_for_the_same_tokens(probe, n):
    X, Y = _ragged_seq(n), o.attn_qkv("flat", n, o.ATTN_HEADS, 999 + n)
    dense, _ = _attn(probe, DENSE, False, np.concatenate([Y, X]), 2, n, 2 * n)
    want = dense[n:2 * n]
    ragged, _ = _attn(probe, RAGGED, False, np.concatenate([Y[:5], X]), 2, n, 5 + n, cu=[0, 5, 5 + n])
    assert np.array_equal(ragged[5:5 + n], want), "RaggedSeq at offset 5 differs from DenseSeq"
    P, T = n - 1, 2  # frame 0 holds X's patches, frame 1 Y's; both share X's first token as CLS
    stream = np.zeros((P * T + 1, 3 * D), np.float16)
    stream[0:P * T:2], stream[1:P * T:2], stream[P * T] = X[1:], Y[1:], X[0]
    patch, cls = _attn(probe, SPACETIME, False, stream, T, n, P * T + 1, shape=(1, P, T), cls_rows=T)
    assert np.array_equal(np.concatenate([cls[0:1], patch[0:P * T:2]]), want), "SpaceTimeSeq differs from DenseSeq"


def test_causal_row_equals_full_attention_on_its_prefix(probe):
    """In bits: a causal query's masked keys score -inf, exactly as the keys past the end of the prefix do, in the same 32-key
    groups."""
    n = 129
    X = o.attn_qkv("flat", n, o.ATTN_HEADS, o.attn_seed("flat", n, 0))
    causal, _ = _attn(probe, DENSE, True, X, 1, n, n)
    for q in (0, 16, 63, 64, 128):
        prefix, _ = _attn(probe, DENSE, False, X[:q + 1], 1, q + 1, q + 1)
        assert np.array_equal(prefix[q], causal[q]), f"query {q}"


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", o.LN_INPUTS)
@pytest.mark.parametrize("f16", [False, True], ids=["fp32", "fp16"])
def test_layernorm_matches_float64(probe, report, f16, kind):
    for d in o.LN_D:
        for eps in o.LN_EPS:
            x, g, b = o.ln_case(kind, d, eps)
            xd, gd, bd = _dev(x), _dev(g), _dev(b)
            for M in o.LN_M:
                for pk in o.LN_PICKS:
                    case = f"{kind} d {d} eps {eps} M {M} pick {pk}"
                    pick = o.ln_pick(pk, M)
                    out = _sentinel((M + 2) * d, f16).view(M + 2, d)
                    pd = None if pick is None else _dev(pick)
                    rc = probe.eioku_probe_ln(int(f16), _ptr(xd), M, d, _ptr(gd), _ptr(bd), eps, _ptr(pd), _ptr(out), None)
                    assert rc == 0, probe.eioku_last_error()
                    bits = _bits(out)
                    assert _only_sentinel(bits[M:]), f"{case}: a store past row M"
                    ref, bar32, _ = o.ln_expect(x, g, b, eps, pick, M)
                    ok, err, bar = o.ln_within_bar(f16, _values(bits[:M]), ref, bar32)
                    _note(report, f"k_ln<{'h16' if f16 else 'float'}> {kind}", err=err, bar=bar)
                    assert ok, f"{case}: error {err:.3e} > bar {bar:.3e}"
                    if kind == "constant":
                        want = np.broadcast_to(b.astype(np.float16) if f16 else b, (M, d))
                        assert np.array_equal(_values(bits[:M]), want), f"{case}: a constant row must give b exactly"
