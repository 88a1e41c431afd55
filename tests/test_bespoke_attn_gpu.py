"""GPU: the attention kernels two models keep to themselves - Whisper's k_attn<QPW, ANC, CAUSAL> through the model's own attn<QPW>
wrapper, k_attn_weights (csrc/whisper.hip) and TimeSformer's k_attn_time (csrc/actions.hip) - and the index movers of Whisper's
prefill and front end, one kernel at a time, against the float64 restatements of tests/bespoke_attn_oracle.py.
libeioku_hip_probe.so (csrc/probe/whisper_probe.hip, actions_probe.hip) includes the two model sources unchanged and exports one
entry point per kernel; the product never loads it.

Bars (tests/test_bespoke_attn_host.py shows that the emulations keep them and that eleven wrong kernels would not):
  fp16 outputs   per head and per sequence: mean and max of |got - ref64| as fractions of the block's reference RMS <= 2 x the
                 emulation's on the same block; equal bits where the emulation has no error (the attention rule)
  fp32 output    k_attn_weights: max |got - ref64| <= 4 x the largest error of the fp32 emulation on the same call
  movers         equal in bits to numpy indexing
Stores: every output lives in a larger buffer pre-filled with a NaN bit pattern that must survive outside the documented region
(rows >= n_q, columns d .. o_rs, weight columns nF[b] .. ldf, cache rows the mover does not own).  Loads: what a kernel must
not read holds NaN too (K / V rows >= n_keys, Q rows >= n_q, under an ancestry table row j of every lane but anc[b][j]), so a
stray read shows as NaN in the output."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import bespoke_attn_oracle as o

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "eioku_amd" / "libeioku_hip_probe.so"
pytestmark = pytest.mark.gpu

S16, S32 = 0x7DDD, 0x7FC0DEAD  # fp16 / fp32 NaNs no kernel produces
EINVAL = -1
D, TM = o.D, o.TM
CASES = o.wh_cases()


class Cfg(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("n_mels", "d_model", "heads", "enc_layers", "dec_layers", "enc_ffn", "dec_ffn", "vocab",
                                       "max_source_positions", "max_target_positions", "eot", "no_timestamps", "timestamp_begin",
                                       "no_speech", "max_initial_timestamp_index", "n_suppress", "n_begin_suppress", "n_langs")]
    _fields_ += [(n, C.c_void_p) for n in ("suppress", "begin_suppress", "lang_ids", "mel_filters")]


@pytest.fixture(scope="module")
def probe(gpu):
    assert LIB.exists(), "build it: make -C eioku_amd/csrc (target all builds the probe library too)"
    lib = C.CDLL(str(LIB))
    p, i, ll = C.c_void_p, C.c_int, C.c_longlong
    lib.eioku_probe_wh_attn.argtypes = [p, i, p, ll, i, p, p, ll, i, i, i, i, p, ll, i, i, p, i, p, i, p]
    lib.eioku_probe_wh_attn_weights.argtypes = [p, ll, i, p, ll, i, i, i, i, i, p, p, p, ll, ll, p]
    lib.eioku_probe_attn_time.argtypes = [p, i, i, i, p, p]
    lib.eioku_probe_wh_embed.argtypes = [p, i, i, i, i, i, p, p, p, i, p]
    lib.eioku_probe_wh_embed_seq.argtypes = [p, i, i, i, i, p, p, p, p]
    lib.eioku_probe_wh_kv_to_cache.argtypes = [p, p, i, i, i, i, i, i, p, p, p]
    lib.eioku_probe_wh_gather_rows.argtypes = [p, i, i, i, i, i, p, p]
    lib.eioku_probe_wh_im2col_mel.argtypes = [p, i, i, i, i, p, p]
    lib.eioku_probe_wh_im2col_s2.argtypes = [p, i, i, i, p, p]
    lib.eioku_whisper_create.argtypes = [C.POINTER(Cfg), C.POINTER(p)]
    lib.eioku_whisper_destroy.argtypes = [p]
    lib.eioku_whisper_destroy.restype = None
    lib.eioku_last_error.restype = C.c_char_p
    assert lib.eioku_init(0) == 0, lib.eioku_last_error()  # the probe links its own core.o: its own state
    return lib


@pytest.fixture(scope="module")
def handle(probe):
    """the probe library's own Whisper of two heads: attn<QPW> takes the grid's head count from it and nothing else"""
    filters = (C.c_double * (8 * 201))()
    cfg = Cfg(n_mels=8, d_model=D, heads=o.HEADS, enc_layers=1, dec_layers=1, enc_ffn=32, dec_ffn=32, vocab=16, max_source_positions=8,
              max_target_positions=8, eot=10, no_timestamps=11, timestamp_begin=12, no_speech=9, max_initial_timestamp_index=1,
              mel_filters=C.cast(filters, C.c_void_p))
    m = C.c_void_p()
    assert probe.eioku_whisper_create(C.byref(cfg), C.byref(m)) == 0, probe.eioku_last_error()
    yield m
    probe.eioku_whisper_destroy(m)


@pytest.fixture(scope="module")
def report():
    """name -> the largest device figures and bars; printed once the module is through (pytest -s)"""
    rows = {}
    yield rows
    for name in sorted(rows):
        print(f"\n[bespoke attention] {name}: " + ", ".join(f"{k} {v:.3e}" for k, v in rows[name].items()), end="")
    print()


def _note(report, name, **figures):
    r = report.setdefault(name, {})
    for k, v in figures.items():
        r[k] = max(r.get(k, 0.0), float(v))


def _tally(report, name, got, emu):
    """reported, not asserted: how many fp16 outputs differ in bits from the emulation's (the device's expf is not the
    emulation's correctly rounded exp)"""
    r = report.setdefault(name, {})
    r["outputs"] = r.get("outputs", 0) + got.size
    r["bits_off_emulation"] = r.get("bits_off_emulation", 0) + int((np.asarray(got).view(np.uint16) != np.asarray(emu).view(np.uint16)).sum())


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


def _only_sentinel(bits):
    return bool((bits == (S16 if bits.dtype == np.uint16 else S32)).all())


def _nan_tail(a, rows=2):
    """a [..][cols] flattened to rows of cols, followed by rows of NaN the kernel has no business reading"""
    flat = np.asarray(a).reshape(-1, a.shape[-1])
    return np.concatenate([flat, np.full((rows, a.shape[-1]), np.nan, flat.dtype)])


# ---- k_attn -------------------------------------------------------------------------------------------------------------------
def _wh_run(probe, handle, qpw, Q, K, V, layout="encoder", kv_div=1, kvmap=None, anc=None, causal=False, n_keys=None, n_q=None):
    """One attn<QPW> call on Q [B][n_q][D], K, V [W][n_keys][D].  -> (rc, bits of the whole output buffer [B n_q + 2][o_rs]).
    encoder / padded: batch strides n x row stride, o_rs = D (padded: D + 8), two NaN rows behind the last batch.
    decoder: n_q = 1 with batch stride D; keys in a cache of TM rows per lane, NaN from row n_keys on and, under an ancestry
    table, in row j of every lane that is nobody's ancestor at step j."""
    B, W = Q.shape[0], K.shape[0]
    n_q, n_keys = n_q or Q.shape[1], n_keys or K.shape[1]
    o_rs = D + 8 if layout == "padded" else D
    q = _dev(_nan_tail(Q))
    if layout == "decoder":
        assert Q.shape[1] == 1
        cache = []
        for t in (K, V):
            c = np.full((W, TM, D), np.nan, np.float16)
            c[:, :K.shape[1]] = t
            if anc is not None:
                used = np.zeros((W, TM), bool)
                used[anc[:, :n_keys].astype(np.int64), np.arange(n_keys)[None, :]] = True
                c[~used] = np.nan
            cache.append(_dev(c))
        k, v, kv_bs = cache[0], cache[1], TM * D
    else:
        k, v, kv_bs = _dev(_nan_tail(K)), _dev(_nan_tail(V)), K.shape[1] * D
    out = _sentinel((B * n_q + 2) * o_rs, True).view(-1, o_rs)
    anc_dev = None if anc is None else _dev(anc)
    map_dev = None if kvmap is None else _dev(np.asarray(kvmap, np.int32))
    rc = probe.eioku_probe_wh_attn(handle, qpw, _ptr(q), Q.shape[1] * D, D, _ptr(k), _ptr(v), kv_bs, D, n_q, n_keys, B, _ptr(out),
                                   n_q * o_rs, o_rs, kv_div, _ptr(anc_dev), 0 if anc is None else anc.shape[1], _ptr(map_dev), int(causal), None)
    torch.cuda.synchronize()
    return rc, _bits(out)


def _run_case(probe, handle, c, qpw=None):
    Q, K, V = o.wh_case_inputs(c)
    rc, bits = _wh_run(probe, handle, qpw or c["qpw"], Q, K, V, c["layout"], c["kv_div"], c["kvmap"], o.anc_table(c["B"]) if c["anc"] else None,
                       c["causal"])
    assert rc == 0, f"{c['name']}: {probe.eioku_last_error()}"
    return bits


def _check_case(report, c, bits):
    n_q, B = c["n_q"], c["B"]
    assert _only_sentinel(bits[B * n_q:]), f"{c['name']}: a store to a row >= n_q"
    assert _only_sentinel(bits[:, D:]), f"{c['name']}: a store to the columns d .. o_rs"
    name = f"k_attn {c['name'].split()[0]}" + (f" {c['gen']}" if c["gen"] == "peaked" else "")
    for b, row in enumerate(o.wh_case_expect(c)):
        for h, (ref, emu) in enumerate(row):
            got = _values(bits[b * n_q:(b + 1) * n_q, 64 * h:64 * h + 64])
            ok, g, e = o.attn_within_bar(got, ref, emu)
            _tally(report, name, got, emu)
            _note(report, name, mean=g[0], mean_bar=2 * e[0], max=g[1], max_bar=2 * e[1],
                  mean_over_bar=g[0] / (2 * e[0]) if e[0] else 0.0, max_over_bar=g[1] / (2 * e[1]) if e[1] else 0.0)
            assert ok, (f"{c['name']} batch {b} head {h}: mean / max error over the block's RMS {g[0]:.3e} / {g[1]:.3e}, "
                        f"emulation {e[0]:.3e} / {e[1]:.3e}")


DENSE = sorted({(c["gen"], c["n_keys"]) for c in CASES if c["name"].startswith("dense")}, key=lambda t: (t[1], o.ATTN_GENERATORS.index(t[0])))


@pytest.mark.parametrize("gen,n_keys", DENSE, ids=[f"{g}-{n}" for g, n in DENSE])
def test_dense_attention_matches_float64_and_qpw_1_equals_qpw_2(probe, handle, report, gen, n_keys):
    """every n_q of the grid in both QPW (a wave with no query, a QPW 2 wave with one live query), in the encoder's strides, the
    decoder step's and once with padded output rows; in bits, QPW 2 gives what QPW 1 gives"""
    seen = {}
    for c in CASES:
        if c["name"].startswith("dense") and (c["gen"], c["n_keys"]) == (gen, n_keys):
            bits = _run_case(probe, handle, c)
            _check_case(report, c, bits)
            twin = seen.setdefault((c["layout"], c["n_q"]), bits)
            assert np.array_equal(twin, bits), f"{c['name']}: QPW 2 differs from QPW 1"
    assert len(seen) >= len(o.NQ_GRID)


OTHERS = [c for c in CASES if not c["name"].startswith("dense")]


@pytest.mark.parametrize("c", OTHERS, ids=[c["name"].replace(" ", "-") for c in OTHERS])
def test_attention_reads_the_keys_of_the_right_window_lane_and_prefix(probe, handle, report, c):
    """the 64 KB LDS edge, kv_div, kvmap, the per-key ancestry of beam search and the causal prefill"""
    _check_case(report, c, _run_case(probe, handle, c))


def test_attention_refuses_what_the_wrapper_refuses_and_launches_nothing(probe, handle):
    Q, K, V = o.wh_inputs("flat", 1, 1, 1, o.LDS_EDGE_KEYS + 1, 4243)
    rc, bits = _wh_run(probe, handle, 2, Q, K, V)
    assert rc == EINVAL and probe.eioku_last_error().decode() == "attention over 1985 keys needs 65568 bytes of LDS", probe.eioku_last_error()
    assert _only_sentinel(bits)
    rc, bits = _wh_run(probe, handle, 1, Q, K, V)  # QPW 1 has room for twice as many
    assert rc == 0 and not _only_sentinel(bits[:1, :D])
    causal = "causal attention needs as many keys as queries and no ancestry table"
    Q, K, V = o.wh_inputs("flat", 2, 2, 9, 9, 4244)
    rc, bits = _wh_run(probe, handle, 2, Q, K, V, causal=True, n_q=8)
    assert rc == EINVAL and probe.eioku_last_error().decode() == causal and _only_sentinel(bits)
    rc, bits = _wh_run(probe, handle, 2, Q, K, V, causal=True, n_keys=8)
    assert rc == EINVAL and probe.eioku_last_error().decode() == causal and _only_sentinel(bits)
    Q1, K1, V1 = o.wh_inputs("flat", 2, 2, 1, 1, 4245)
    rc, bits = _wh_run(probe, handle, 1, Q1, K1, V1, layout="decoder", anc=o.anc_table(2), causal=True)
    assert rc == EINVAL and probe.eioku_last_error().decode() == causal and _only_sentinel(bits)
    for qpw in (0, 3, 4):
        rc, bits = _wh_run(probe, handle, qpw, Q, K, V)
        assert rc == EINVAL and b"attn<1> and attn<2>" in probe.eioku_last_error() and _only_sentinel(bits)
    rc, bits = _wh_run(probe, None, 2, Q, K, V)
    assert rc == EINVAL and b"NULL" in probe.eioku_last_error() and _only_sentinel(bits)


# ---- identities, in bits ---------------------------------------------------------------------------------------------------------
def test_causal_query_equals_plain_attention_on_its_prefix(probe, handle):
    """a masked key contributes exp(-inf) = 0 to the sum and 0 x v to the output, in the slot it would not have had"""
    c = next(c for c in CASES if c["name"] == "causal P 130")
    Q, K, V = o.wh_case_inputs(c)
    causal = _run_case(probe, handle, c)
    for q in (0, 1, 2, 63, 64, 65, 128, 129):
        for qpw in (1, 2):
            rc, prefix = _wh_run(probe, handle, qpw, Q[:, q:q + 1], K[:, :q + 1], V[:, :q + 1])
            assert rc == 0
            for b in range(2):
                assert np.array_equal(prefix[b, :D], causal[b * 130 + q, :D]), f"query {q} of row {b}, QPW {qpw}"


def test_identity_ancestry_equals_the_plain_call(probe, handle):
    B, n = 6, 66
    Q, K, V = o.wh_inputs("flat", B, B, 1, n, 7000)
    own = np.repeat(np.arange(B, dtype=np.uint8)[:, None], TM, axis=1)
    rc, a = _wh_run(probe, handle, 1, Q, K, V, layout="decoder", anc=own)
    rc2, plain = _wh_run(probe, handle, 1, Q, K, V, layout="decoder")
    assert rc == 0 and rc2 == 0 and np.array_equal(a, plain)
    rc, other = _wh_run(probe, handle, 1, Q, K, V, layout="decoder", anc=o.anc_table(B))
    assert rc == 0 and not np.array_equal(other[:B], plain[:B])


def test_a_repeating_kvmap_equals_kv_div(probe, handle):
    c = next(c for c in CASES if c["name"] == "kv_div qpw 2")
    Q, K, V = o.wh_case_inputs(c)
    rc, div = _wh_run(probe, handle, 2, Q, K, V, kv_div=3)
    rc2, mapped = _wh_run(probe, handle, 2, Q, K, V, kvmap=[0, 0, 0, 1, 1, 1])
    assert rc == 0 and rc2 == 0 and np.array_equal(div, mapped)


def _weights(probe, Q, K, head, nF, kvmap, ldf):
    """-> bits of A [R][P + 1][ldf]"""
    R, P = Q.shape[:2]
    q, k = _dev(_nan_tail(Q)), _dev(_nan_tail(K))
    A = _sentinel(R * (P + 1) * ldf, False).view(R, P + 1, ldf)
    map_dev, nf_dev = _dev(np.asarray(kvmap, np.int32)), _dev(np.asarray(nF, np.int32))
    rc = probe.eioku_probe_wh_attn_weights(_ptr(q), P * D, D, _ptr(k), K.shape[1] * D, D, P, K.shape[1], R, head, _ptr(map_dev), _ptr(nf_dev),
                                           _ptr(A), (P + 1) * ldf, ldf, None)
    assert rc == 0, probe.eioku_last_error()
    torch.cuda.synchronize()
    return _bits(A)


@pytest.mark.parametrize("n_keys", [37, 64])
def test_attention_on_identity_values_is_the_weights_rounded_to_fp16(probe, handle, n_keys):
    """whisper.hip: k_attn_weights is "the score and softmax half of k_attn ... the same fp32 dot in the same order".  With value
    row j the unit vector e_j the PV pass adds p_j to zeros: k_attn stores fp16(p_lane / sum), k_attn_weights p_j / sum."""
    Q, K, _ = o.wh_inputs("flat", 3, 3, 5, n_keys, 9100)
    V = np.zeros((3, n_keys, D), np.float16)
    for h in range(o.HEADS):
        V[:, np.arange(n_keys), 64 * h + np.arange(n_keys)] = 1
    for qpw in (1, 2):
        rc, out = _wh_run(probe, handle, qpw, Q, K, V, kvmap=[2, 0, 1])
        assert rc == 0
        got = _values(out[:15, :D]).reshape(3, 5, D)
        for h in range(o.HEADS):
            A = _values(_weights(probe, Q, K, h, [n_keys] * 3, [2, 0, 1], n_keys + 8))[:, :5, :n_keys]
            assert np.array_equal(got[:, :, 64 * h:64 * h + n_keys].view(np.uint16), o.to_f16(A).view(np.uint16)), f"QPW {qpw} head {h}"
            assert not got[:, :, 64 * h + n_keys:64 * h + 64].any()


# ---- k_attn_weights -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,n_keys", [(P, nk) for P in o.W_P for nk in o.W_KEYS])
def test_attention_weights_match_float64_over_all_keys(probe, report, P, n_keys):
    for case in o.weight_cases():
        if case[:2] != (P, n_keys):
            continue
        _, _, head, nF, kvmap = case
        Q, K = o.weight_inputs(P, n_keys)
        ldf = n_keys + 8
        bits = _weights(probe, Q, K, head, nF, kvmap, ldf)
        want = o.weight_expect(*case)
        bar = max(o.weights_bar(ref, emu) for ref, emu in want)
        assert _only_sentinel(bits[:, P]), f"{case}: a store to a row >= n_q"
        for r, (ref, _) in enumerate(want):
            assert _only_sentinel(bits[r, :, nF[r]:]), f"{case} row {r}: a store to the columns nF .. ldf"
            err = float(np.abs(_values(bits[r, :P, :nF[r]]).astype(np.float64) - ref).max())
            _note(report, "k_attn_weights", err=err, bar=bar, err_over_bar=err / bar)
            assert err <= bar, f"{case} row {r}: error {err:.3e} > bar {bar:.3e}"


# ---- k_attn_time -----------------------------------------------------------------------------------------------------------------
def _time(probe, qkv, T, heads):
    """qkv [n_seq][T][3 d] -> bits of out [n_seq T + 2][d]"""
    n_seq, d = qkv.shape[0], 64 * heads
    out = _sentinel((n_seq * T + 2) * d, True).view(-1, d)
    x = _dev(_nan_tail(qkv))
    rc = probe.eioku_probe_attn_time(_ptr(x), n_seq, T, heads, _ptr(out), None)
    assert rc == 0, probe.eioku_last_error()
    torch.cuda.synchronize()
    return _bits(out)


@pytest.mark.parametrize("gen,T,heads", o.time_cases(), ids=[f"{g}-T{T}-h{h}" for g, T, h in o.time_cases()])
def test_time_attention_matches_float64_and_a_sequence_alone_equals_itself_among_five(probe, report, gen, T, heads):
    qkv = o.time_qkv(gen, T, heads)
    bits = _time(probe, qkv, T, heads)
    assert _only_sentinel(bits[o.TIME_SEQS * T:]), "a store past the last sequence"
    for s, row in enumerate(o.time_expect(gen, T, heads)):
        for h, (ref, emu) in enumerate(row):
            got = _values(bits[s * T:(s + 1) * T, 64 * h:64 * h + 64])
            ok, g, e = o.attn_within_bar(got, ref, emu)
            _tally(report, "k_attn_time" + (" second key slot" if T > 64 else ""), got, emu)
            _note(report, "k_attn_time" + (" second key slot" if T > 64 else ""), mean=g[0], mean_bar=2 * e[0], max=g[1], max_bar=2 * e[1],
                  mean_over_bar=g[0] / (2 * e[0]) if e[0] else 0.0, max_over_bar=g[1] / (2 * e[1]) if e[1] else 0.0)
            assert ok, f"{gen} T {T} sequence {s} head {h}: {g[0]:.3e} / {g[1]:.3e}, emulation {e[0]:.3e} / {e[1]:.3e}"
    for s in (0, 3):
        alone = _time(probe, qkv[s:s + 1], T, heads)
        assert np.array_equal(alone[:T], bits[s * T:(s + 1) * T]), f"sequence {s} alone differs from itself among {o.TIME_SEQS}"


def test_time_attention_refuses_more_frames_than_its_lds_holds(probe):
    out = _sentinel(128 * 64, True)
    x = _dev(np.zeros((128, 192), np.float16))
    for T in (0, 97):
        assert probe.eioku_probe_attn_time(_ptr(x), 1, T, 1, _ptr(out), None) == EINVAL and b"bad shape" in probe.eioku_last_error()
    assert probe.eioku_probe_attn_time(None, 1, 8, 1, _ptr(out), None) == EINVAL and b"NULL" in probe.eioku_last_error()
    assert _only_sentinel(_bits(out))


# ---- the movers: equal in bits to numpy indexing -----------------------------------------------------------------------------------------
def _same_bits(got_bits, want):
    return np.array_equal(got_bits, np.ascontiguousarray(want).view(got_bits.dtype).reshape(got_bits.shape))


@pytest.mark.parametrize("C_,ldk", [(80, 256), (80, 384), (128, 384)])
def test_im2col_mel(probe, C_, ldk):
    for T in (2, 7, 200):
        mel = np.random.default_rng(C_ + T).standard_normal((2, C_, T)).astype(np.float32)
        src = _dev(np.concatenate([mel.reshape(-1), np.full(64, np.nan, np.float32)]))
        col = _sentinel((2 * T + 1) * ldk, True).view(-1, ldk)
        assert probe.eioku_probe_wh_im2col_mel(_ptr(src), 2, C_, T, ldk, _ptr(col), None) == 0, probe.eioku_last_error()
        bits = _bits(col)
        want = o.im2col_mel_ref(mel, ldk)
        assert _same_bits(bits[:2 * T], want) and _only_sentinel(bits[2 * T:]), (C_, ldk, T)
        assert not bits[:2 * T, 3 * C_:].any(), "the columns from 3 C on are zero"


@pytest.mark.parametrize("C_", [128, 384])
def test_im2col_s2(probe, C_):
    for T in (2, 8, 200):
        h = np.random.default_rng(C_ + T).standard_normal((2, T, C_)).astype(np.float16)
        col = _sentinel((T + 1) * 3 * C_, True).view(-1, 3 * C_)
        src = _dev(_nan_tail(h))
        assert probe.eioku_probe_wh_im2col_s2(_ptr(src), 2, C_, T, _ptr(col), None) == 0, probe.eioku_last_error()
        bits = _bits(col)
        assert _same_bits(bits[:T], o.im2col_s2_ref(h)) and _only_sentinel(bits[T:]), (C_, T)
    assert probe.eioku_probe_wh_im2col_s2(_ptr(col), 2, C_, 7, _ptr(col), None) == EINVAL


@pytest.mark.parametrize("d", o.MOVER_D)
def test_embed_and_embed_seq(probe, d):
    vocab, rng = 11, np.random.default_rng(d)
    emb, pos = rng.standard_normal((vocab, d)).astype(np.float16), rng.standard_normal((6, d)).astype(np.float32)
    emb_dev, pos_dev = _dev(_nan_tail(emb)), _dev(_nan_tail(pos))
    B, s, tstride = 4, 2, 3
    toks = np.full(B * tstride, 7, np.int32)
    toks[::tstride] = [-1, vocab, 3, vocab - 1]
    for ids, uniform in ((toks, 0), (None, 5), (None, vocab + 3), (None, -2)):
        x = _sentinel((B + 1) * d, False).view(-1, d)
        ids_dev = None if ids is None else _dev(ids)
        rc = probe.eioku_probe_wh_embed(_ptr(ids_dev), tstride, uniform, vocab, d, s, _ptr(emb_dev), _ptr(pos_dev), _ptr(x), B, None)
        assert rc == 0, probe.eioku_last_error()
        bits = _bits(x)
        want = o.embed_ref(toks[::tstride] if ids is not None else np.full(B, uniform), emb, pos[s])
        assert _same_bits(bits[:B], want) and _only_sentinel(bits[B:]), (d, uniform)
    for P in o.MOVER_P:
        R = 3
        ids = rng.integers(0, vocab, (R, P)).astype(np.int32)
        ids[0, 0], ids[R - 1, P - 1], ids[1, 0] = -1, vocab, vocab - 1
        x = _sentinel((R * P + 1) * d, False).view(-1, d)
        ids_dev = _dev(ids)
        assert probe.eioku_probe_wh_embed_seq(_ptr(ids_dev), R, P, vocab, d, _ptr(emb_dev), _ptr(pos_dev), _ptr(x), None) == 0
        bits = _bits(x)
        want = o.embed_ref(ids, emb, pos[:P][None])
        assert _same_bits(bits[:R * P], want.reshape(R * P, d)) and _only_sentinel(bits[R * P:]), (d, P)


@pytest.mark.parametrize("d", o.MOVER_D)
def test_kv_to_cache_and_gather_rows(probe, d):
    Tm = 8
    for R, G, ls in o.MOVER_RGL:
        for P in o.MOVER_P:
            rng = np.random.default_rng(d + 10 * R + P)
            pk, pv = (rng.standard_normal((R, P, d)).astype(np.float16) for _ in range(2))
            lanes = (R - 1) * ls + G + 1
            ck, cv = (_sentinel(lanes * Tm * d, True).view(lanes, Tm, d) for _ in range(2))
            pk_dev, pv_dev = _dev(_nan_tail(pk)), _dev(_nan_tail(pv))
            rc = probe.eioku_probe_wh_kv_to_cache(_ptr(pk_dev), _ptr(pv_dev), R, P, d, G, ls, Tm, _ptr(ck), _ptr(cv), None)
            assert rc == 0, probe.eioku_last_error()
            empty = np.full((lanes, Tm, d), S16, np.uint16).view(np.float16)
            for got, src in ((ck, pk), (cv, pv)):
                assert _same_bits(_bits(got), o.kv_to_cache_ref(src, empty, R, P, G, ls)), f"d {d} (R, G, lstride) {(R, G, ls)} P {P}"
            L = R * G
            for t in sorted({0, P - 1}):
                out = _sentinel((L + 1) * d, True).view(-1, d)
                assert probe.eioku_probe_wh_gather_rows(_ptr(pk_dev), L, P, t, G, d, _ptr(out), None) == 0
                bits = _bits(out)
                assert _same_bits(bits[:L], o.gather_rows_ref(pk, L, t, G)) and _only_sentinel(bits[L:]), (d, R, G, P, t)
    assert probe.eioku_probe_wh_kv_to_cache(_ptr(ck), _ptr(cv), 1, 1, d + 4, 1, 1, Tm, _ptr(ck), _ptr(cv), None) == EINVAL
