"""Host side of the transformer-core parity net (tests/transformer_core_oracle.py, tests/test_transformer_core_gpu.py): no GPU.

1. The emulation (fp32 accumulation, fp16 numerators, one rounding per fp16 output, two-pass fp32 statistics) stays inside the
   bars of the GPU tests on every case of their tables: the inputs and the bars fit together.
2. Every deliberately wrong emulation leaves the bars on at least one case: the GPU tests can fail.
3. The probe's (MT, EPI) dispatch table is the set of k_gemm instantiations of the four models' sources."""
import re
from pathlib import Path

import numpy as np
import pytest

import transformer_core_oracle as o

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "eioku_amd" / "csrc"
EPIS = sorted({e for _, e in o.GEMM_TABLE})


# ---- 1. the emulation within the bars -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", EPIS, ids=lambda e: o.EPI_NAMES[e])
def test_gemm_emulation_is_within_the_bars(epi):
    worst = (0.0, 0.0)
    for M, N, K, pos_rows, _, _ in o.gemm_cases(epi):
        ref, bar32, emu = o.gemm_expect(epi, M, N, K, pos_rows)
        ok, err, bar = o.gemm_within_bar(epi, emu, ref, bar32)
        assert ok, f"{o.EPI_NAMES[epi]} M {M} N {N} K {K} pos_rows {pos_rows}: emulation error {err:.3e} > bar {bar:.3e}"
        assert M == 0 or bar32 > 0 or epi in o.F16_OUT, "an fp32 case whose bar is zero checks bits, not the rule"
        worst = max(worst, (err, bar))
    print(f"{o.EPI_NAMES[epi]}: {len(o.gemm_cases(epi))} cases, largest emulation error {worst[0]:.3e} (bar there {worst[1]:.3e})")


def _attn_sequences():
    """(label, causal, qkv rows of one sequence, cache key) of every sequence of the GPU attention tables"""
    for gen, n in o.attn_dense_cases():
        for causal in (False, True):
            for s in range(3):
                seed = o.attn_seed(gen, n, s)
                yield f"dense {gen} n {n} causal {causal} seq {s}", causal, o.attn_qkv(gen, n, o.ATTN_HEADS, seed), (gen, n, seed)
    for n in o.RAGGED_LENGTHS[0]:  # the permutations hold the same sequences
        seed = o.attn_seed("flat", n, 7)
        yield f"ragged n {n}", False, o.attn_qkv("flat", n, o.ATTN_HEADS, seed), ("flat", n, seed)
    for i, (B, P, T) in enumerate(o.SPACETIME_SHAPES):
        qkv, idx = o.spacetime_qkv(B, P, T, 50 + i)
        for z, rows in enumerate(idx):
            yield f"space-time {(B, P, T)} problem {z}", False, qkv[rows], ("st", i, z)


def test_attention_emulation_is_within_the_bars():
    """Trivially (it is its own bar) except for what the bar assumes: a finite, non-zero reference block and an emulation whose
    zero error means equal bits."""
    worst = {}
    for label, causal, qkv, key in _attn_sequences():
        for h, (ref, emu) in enumerate(o.attn_expect(qkv, causal, key)):
            ok, g, e = o.attn_within_bar(emu, ref, emu)
            assert np.isfinite(ref).all() and np.isfinite(emu.astype(np.float64)).all() and (ref ** 2).mean() > 0, label
            assert ok, f"{label} head {h}: {g} against {e}"
            w = worst.setdefault(label.split()[1] if label.startswith("dense") else label.split()[0], [0.0, 0.0])
            w[0], w[1] = max(w[0], e[0]), max(w[1], e[1])
    for k, (mean, mx) in worst.items():
        print(f"attention {k}: emulation error / block RMS, largest mean {mean:.3e}, largest max {mx:.3e}")
        assert mx < 0.01, "the emulation itself is an fp16 attention: within 1 % of the block's RMS"


def _ln_cases():
    for kind in o.LN_INPUTS:
        for d in o.LN_D:
            for eps in o.LN_EPS:
                x, g, b = o.ln_case(kind, d, eps)
                for M in o.LN_M:
                    for pk in o.LN_PICKS:
                        yield kind, d, eps, M, pk, x, g, b


def test_layernorm_emulation_is_within_the_bars():
    for kind, d, eps, M, pk, x, g, b in _ln_cases():
        pick = o.ln_pick(pk, M)
        ref, bar32, e32 = o.ln_expect(x, g, b, eps, pick, M)
        for f16 in (False, True):
            ok, err, bar = o.ln_within_bar(f16, o.to_f16(e32) if f16 else e32, ref, bar32)
            assert ok, f"{kind} d {d} eps {eps} M {M} pick {pk} fp16 {f16}: emulation error {err:.3e} > bar {bar:.3e}"
        if kind == "constant":
            assert np.array_equal(e32, np.broadcast_to(b, e32.shape)), "a constant row must give b exactly"
        if kind == "var_eps":
            var = x.astype(np.float64).var(axis=1)
            assert ((var > 0.45 * eps) & (var < 2.2 * eps)).all()


# ---- 2. the mutants outside the bars ------------------------------------------------------------------------------------------
GEMM_MUTANT_EPIS = {"rope_pairs_adjacent": [o.EPI_ROPE_F16], "rope_rotates_v": [o.EPI_ROPE_F16],
                    "pos_not_wrapped": [o.EPI_POS, o.EPI_GELU_POS], "swiglu_swapped": [o.EPI_SWIGLU_F16],
                    "resid_overwrites": [o.EPI_RESID]}


def _gemm_rejections(mutant):
    n = 0
    for epi in GEMM_MUTANT_EPIS[mutant]:
        for M, N, K, pos_rows, _, _ in o.gemm_cases(epi):
            if M:
                ref, bar32, out = o.gemm_expect(epi, M, N, K, pos_rows, mutant=mutant)
                n += not o.gemm_within_bar(epi, out, ref, bar32)[0]
    return n


def _attn_rejections(mutant):
    n = 0
    for label, causal, qkv, key in _attn_sequences():
        for (q, k, v), (ref, emu) in zip(o.attn_blocks(qkv, o.ATTN_HEADS), o.attn_expect(qkv, causal, key)):
            n += not o.attn_within_bar(o.attn_emulate(q, k, v, causal, mutant), ref, emu)[0]
    return n


def _ln_rejections(mutant):
    n = 0
    for kind, d, eps, M, pk, x, g, b in _ln_cases():
        pick = o.ln_pick(pk, M)
        ref, bar32, out = o.ln_expect(x, g, b, eps, pick, M, mutant=mutant)
        n += not o.ln_within_bar(False, out, ref, bar32)[0]
        n += not o.ln_within_bar(True, o.to_f16(out), ref, bar32)[0]
    return n


def test_every_mutant_is_rejected_by_at_least_one_case():
    assert set(GEMM_MUTANT_EPIS) == set(o.GEMM_MUTANTS)
    counts = {m: _gemm_rejections(m) for m in o.GEMM_MUTANTS}
    counts.update({m: _attn_rejections(m) for m in o.ATTN_MUTANTS})
    counts.update({m: _ln_rejections(m) for m in o.LN_MUTANTS})
    for m, n in counts.items():
        print(f"mutant {m}: outside the bar on {n} cases")
    survivors = [m for m, n in counts.items() if n == 0]
    assert not survivors, f"no case rejects {survivors}: extend the case tables"


def test_the_unrounded_sum_is_caught_by_the_case_built_for_it():
    """Random numerators round up as often as down, so the sum of the unrounded ones differs from the sum of the rounded ones by
    far less than the output's own rounding.  half_bias makes every numerator round down: the correct kernel returns 128
    exactly, the mutant the fp16 below it."""
    q, k, v = o.attn_inputs("half_bias", 33, 1)
    assert np.array_equal(o.attn_emulate(q, k, v, False), np.full((33, 64), 128, np.float16))
    assert (o.attn_emulate(q, k, v, False, "sum_unrounded")[1:] < 128).all()


# ---- 3. the dispatch table -----------------------------------------------------------------------------------------------------
def _instantiations(path):
    """The (MT, EPI) of every launch_gemm<MT, EPI> a model source instantiates.  The sources reach it through function
    templates (gemm<MT, EPI>, mlp<MT>, cross_attn<MT, QPW> ...): a call with literal arguments instantiates its callee, a call
    inside a function template instantiates it once per instantiation of that template, to a fixed point.  A source that
    includes encoder.h is read together with it (Enc::gemm and the sublayers are defined there); a definition ends at the
    closing brace of its own indentation, so a member template ends inside its struct."""
    text = path.read_text()
    if '#include "encoder.h"' in text:
        text += (CSRC / "encoder.h").read_text()
    text = re.sub(r"//[^\n]*", "", text)
    defs = {}
    for m in re.finditer(r"^([ \t]*)template <([^>]*)>\s*int (\w+)\(", text, re.M):
        params = [p.split()[-1] for p in m.group(2).split(",")]
        defs[m.group(3)] = (params, m.end(), text.index("\n" + m.group(1) + "}\n", m.end()))
    calls = []  # (callee, arguments, enclosing function template or None)
    for m in re.finditer(r"\b(\w+)<([\w\s,]+)>\s*\(", text):
        if m.group(1) in defs or m.group(1) == "launch_gemm":
            inside = [f for f, (_, a, b) in defs.items() if a <= m.start() < b]
            calls.append((m.group(1), [a.strip() for a in m.group(2).split(",")], inside[0] if inside else None))
    inst = {f: set() for f in list(defs) + ["launch_gemm"]}
    changed = True
    while changed:
        changed = False
        for callee, args, inside in calls:
            envs = [dict(zip(defs[inside][0], t)) for t in inst[inside]] if inside else [{}]
            for env in envs:
                t = tuple(env.get(a, a) for a in args)
                if all(re.fullmatch(r"\d+|EPI_\w+|true|false", a) for a in t) and t not in inst[callee]:
                    inst[callee].add(t)
                    changed = True
    return {(int(mt), epi) for mt, epi in inst["launch_gemm"]}


def test_probe_dispatch_table_is_the_models_instantiations():
    found = set().union(*(_instantiations(CSRC / f) for f in ("whisper.hip", "actions.hip", "clip.hip", "nomic.hip", "sounds.hip")))
    assert len(found) >= 13 and all(epi in o.EPI_NAMES for _, epi in found), found
    probe = (CSRC / "probe" / "transformer_probe.hip").read_text()
    table = {(int(mt), epi) for mt, epi in re.findall(r"^\s*X\((\d+), (EPI_\w+)\)", probe, re.M)}
    assert table == found, f"probe only: {sorted(table - found)}, models only: {sorted(found - table)}"
    assert {(mt, o.EPI_NAMES[e]) for mt, e in o.GEMM_TABLE} == found, "transformer_core_oracle.GEMM_TABLE is out of date"
    header = (CSRC / "gemm_f16.h").read_text()
    enum = re.search(r"enum \{([^}]*)\}", header).group(1)
    assert {n.strip(): int(v) for n, v in (e.split("=") for e in enum.split(","))} == {n: i for i, n in enumerate(o.EPI_NAMES)}


def test_product_does_not_reference_the_probe():
    sources = sorted((CSRC / "probe").glob("*.hip"))
    assert {"whisper_probe.hip", "actions_probe.hip", "transformer_probe.hip"} <= {p.name for p in sources}
    names = [n for p in sources for n in re.findall(r"int (eioku_probe_\w+)\(", p.read_text())] + [p.stem for p in sources]
    assert "eioku_probe_wh_attn" in names and "eioku_probe_attn_time" in names
    for path in list((ROOT / "eioku_amd").glob("*.py")) + [ROOT / "include" / "eioku_hip.h", ROOT / "bench.py"]:
        assert "libeioku_hip_probe" not in path.read_text() and "eioku_probe_" not in path.read_text(), path
        assert not any(n in path.read_text() for n in names), path
