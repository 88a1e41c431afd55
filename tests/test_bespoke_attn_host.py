"""Host side of the bespoke-attention parity net (tests/bespoke_attn_oracle.py, tests/test_bespoke_attn_gpu.py): no GPU.

1. The emulations of k_attn, k_attn_weights and k_attn_time stay inside the bars of the GPU tests on every case of their tables.
2. Every deliberately wrong emulation leaves the bars on at least one case, and the reference alone tells the windows, lanes and
   thirds apart: the GPU tests can fail.
3. The probes launch what the models launch: the attn<QPW> calls of whisper.hip are the probe's dispatch and the cases' flags,
   and the launch lines the probes repeat carry the models' grid, block and LDS size."""
import re
from pathlib import Path

import numpy as np
import pytest

import bespoke_attn_oracle as o

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "eioku_amd" / "csrc"
CASES = o.wh_cases()


# ---- 1. the emulations within the bars ----------------------------------------------------------------------------------------
def test_case_tables_hold_what_the_kernels_branch_on():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    dense = {(c["qpw"], c["n_q"], c["n_keys"]) for c in CASES if c["name"].startswith("dense ")}
    assert dense == {(q, a, b) for q in (1, 2) for a in o.NQ_GRID for b in o.NK_GRID}
    for nk in o.NK_GRID:
        gens = {c["gen"] for c in CASES if c["name"].startswith("dense ") and c["n_keys"] == nk}
        assert gens == (set(o.ATTN_GENERATORS) if nk in (65, 200) else {"flat", "peaked"})
    assert 4 * 2 * (o.LDS_EDGE_KEYS + 64) * 4 == 64 * 1024
    table = o.anc_table(6)
    assert table.shape == (6, o.TM) and table.max() == 5
    assert (table[:, 8] == np.arange(6)).all() and (table[:, 60] == 3).all(), "self and repeated ancestors"
    assert all((table[:, :s + 1] != np.arange(6)[:, None]).any() for s in o.ANC_STEPS), "every step reads another lane somewhere"


def test_whisper_attention_emulation_is_within_the_bars():
    worst = {}
    for c in CASES:
        for b, row in enumerate(o.wh_case_expect(c)):
            for h, (ref, emu) in enumerate(row):
                assert ref.shape == (c["n_q"], 64) and np.isfinite(ref).all() and (ref ** 2).mean() > 0, c["name"]
                assert np.isfinite(emu.astype(np.float64)).all(), c["name"]
                ok, g, e = o.attn_within_bar(emu, ref, emu)
                assert ok, f"{c['name']} batch {b} head {h}: {g} against {e}"
                w = worst.setdefault(c["name"].split()[0], [0.0, 0.0])
                w[0], w[1] = max(w[0], e[0]), max(w[1], e[1])
    for k, (mean, mx) in worst.items():
        print(f"k_attn {k}: emulation error / block RMS, largest mean {mean:.3e}, largest max {mx:.3e}")
        assert mx < 0.01, "fp32 scores and one fp16 rounding: within 1 % of the block's RMS"


def test_one_key_is_its_value_exactly():
    for c in CASES:
        if c["n_keys"] == 1 and not c["anc"]:
            Q, K, V = o.wh_case_inputs(c)
            for b, row in enumerate(o.wh_case_expect(c)):
                for h, (ref, emu) in enumerate(row):
                    assert np.array_equal(emu, np.broadcast_to(V[b, 0, 64 * h:64 * h + 64], emu.shape)), c["name"]


def test_weights_emulation_is_within_the_bar():
    worst = 0.0
    for P, nk, head, nF, kvmap in o.weight_cases():
        bar = max(o.weights_bar(ref, emu) for ref, emu in o.weight_expect(P, nk, head, nF, kvmap))
        assert bar > 0, "a case whose bar is zero checks bits, not the rule"
        for r, (ref, emu) in enumerate(o.weight_expect(P, nk, head, nF, kvmap)):
            assert ref.shape == (P, nF[r]) and emu.dtype == np.float32
            assert np.abs(emu.astype(np.float64) - ref).max() <= bar
        worst = max(worst, bar / 4)
    print(f"k_attn_weights: {len(o.weight_cases())} cases, largest emulation error {worst:.3e}")
    used = {f for _, nk, _, nF, _ in o.weight_cases() for f in nF}
    assert {1, 63, 64, 65, 100, 200, 1500} <= used
    assert any(f < nk for _, nk, _, nF, _ in o.weight_cases() for f in nF if nk == 1500)


def test_time_attention_emulation_is_within_the_bars():
    worst = [0.0, 0.0]
    for gen, T, heads in o.time_cases():
        for s, row in enumerate(o.time_expect(gen, T, heads)):
            assert len(row) == heads
            for ref, emu in row:
                assert np.isfinite(ref).all() and (ref ** 2).mean() > 0
                ok, g, e = o.attn_within_bar(emu, ref, emu)
                assert ok, (gen, T, heads, s)
                worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    print(f"k_attn_time: emulation error / block RMS, largest mean {worst[0]:.3e}, largest max {worst[1]:.3e}")
    assert worst[1] < 0.01


# ---- 2. the mutants outside the bars ------------------------------------------------------------------------------------------
def _applies(mutant, c):
    return {"kv_div_ignored": c["kv_div"] > 1, "kvmap_ignored": c["kvmap"] is not None, "ancestry_ignored": c["anc"],
            "ancestry_transposed": c["anc"], "causal_off_by_one": c["causal"], "causal_wave_bound_q0": c["causal"],
            "qpw2_second_reads_first": c["qpw"] == 2 and c["n_q"] >= 2 and c["n_keys"] <= 200}[mutant]


def _wh_rejections(mutant):
    n = 0
    for c in CASES:
        if _applies(mutant, c):
            got, want = o.wh_case_mutant(c, mutant), o.wh_case_expect(c)
            n += any(not o.attn_within_bar(got[b][h], *want[b][h])[0] for b in range(c["B"]) for h in range(o.HEADS))
    return n


def _weight_rejections(mutant):
    n = 0
    for case in o.weight_cases():
        good = o.weight_expect(*case)
        bar = max(o.weights_bar(ref, emu) for ref, emu in good)
        n += any(np.abs(out.astype(np.float64) - ref).max() > bar for (ref, _), (_, out) in zip(good, o.weight_expect(*case, mutant=mutant)))
    return n


def _time_rejections(mutant):
    n = 0
    for gen, T, heads in o.time_cases():
        qkv, want = o.time_qkv(gen, T, heads), o.time_expect(gen, T, heads)
        n += any(not o.attn_within_bar(o.attn_emulate(q, k, v, mutant=mutant), *want[s][h])[0]
                 for s in range(o.TIME_SEQS) for h, (q, k, v) in enumerate(o.attn_blocks(qkv[s], heads)))
    return n


def _mover_rejections(mutant):
    n = 0
    for d in o.MOVER_D:
        for R, G, ls in o.MOVER_RGL:
            for P in o.MOVER_P:
                pk, cache = _cache_problem(d, R, G, ls, P)
                n += not np.array_equal(o.kv_to_cache_ref(pk, cache, R, P, G, ls, mutant).view(np.uint16),
                                        o.kv_to_cache_ref(pk, cache, R, P, G, ls).view(np.uint16))
    return n


def _cache_problem(d, R, G, ls, P):
    rng = np.random.default_rng(d + 10 * R + P)
    lanes = (R - 1) * ls + G + 1
    return rng.standard_normal((R, P, d)).astype(np.float16), np.full((lanes, 8, d), np.nan, np.float16)


def test_every_mutant_is_rejected_by_at_least_one_case():
    counts = {m: _wh_rejections(m) for m in o.KEY_MUTANTS + o.SOFTMAX_MUTANTS}
    counts.update({m: _weight_rejections(m) for m in o.WEIGHT_MUTANTS})
    counts.update({m: _time_rejections(m) for m in o.TIME_MUTANTS})
    counts.update({m: _mover_rejections(m) for m in o.MOVER_MUTANTS})
    assert list(counts) == o.MUTANTS
    for m, n in counts.items():
        print(f"mutant {m}: outside the bar on {n} cases")
    survivors = [m for m, n in counts.items() if n == 0]
    assert not survivors, f"no case rejects {survivors}: extend the case tables"


def test_the_reference_alone_tells_the_key_sources_apart():
    """Different windows and lanes hold different data: reading the wrong one moves the float64 result by far more than any bar."""
    for c in CASES:
        for m in o.KEY_MUTANTS:
            if _applies(m, c):
                Q, K, V = o.wh_case_inputs(c)
                right, wrong = o.wh_case_source(c), o.wh_case_source(c, m)
                moved = 0
                for b in range(c["B"]):
                    if (right[b] != wrong[b]).any():
                        a = o.attn_ref(Q[b][:, :64], o.gather_keys(K, right[b])[:, :64], o.gather_keys(V, right[b])[:, :64])
                        z = o.attn_ref(Q[b][:, :64], o.gather_keys(K, wrong[b])[:, :64], o.gather_keys(V, wrong[b])[:, :64])
                        assert o.block_errors(z, a)[1] > 0.05, (c["name"], m, b)
                        moved += 1
                assert moved, (c["name"], m)


# ---- 3. the probes launch what the models launch -----------------------------------------------------------------------------------
def _split_args(text, start):
    """the top-level comma-separated arguments of the call whose opening parenthesis ends at `start`"""
    args, depth, a = [], 0, start
    for i in range(start, len(text)):
        ch = text[i]
        if ch == ")" and depth == 0:
            return args + [" ".join(text[a:i].split())]
        depth += (ch == "(") - (ch == ")")
        if ch == "," and depth == 0:
            args.append(" ".join(text[a:i].split()))
            a = i + 1
    raise AssertionError("unbalanced call")


def _attn_uses(text):
    """(QPW, ancestry table passed, causal passed) of every attn<...> call of whisper.hip, QPW resolved through cross_attn<MT, QPW>"""
    text = re.sub(r"//[^\n]*", "", text)
    cross = {int(q) for q in re.findall(r"cross_attn<\d+, (\d+)>\(", text)}
    uses = set()
    for m in re.finditer(r"\(attn<(\w+)>\(", text):
        args = _split_args(text, m.end())
        assert len(args) in (14, 17, 18, 19), args  # kv_div, anc, anc_ld, kvmap, causal have defaults
        anc = len(args) > 15 and args[15] != "nullptr"
        causal = len(args) > 18 and args[18] == "true"
        for qpw in (cross if m.group(1) == "QPW" else {int(m.group(1))}):
            uses.add((qpw, anc, causal))
    return uses


def test_probe_dispatch_is_the_models_attn_calls():
    uses = _attn_uses((CSRC / "whisper.hip").read_text())
    # decoder_step's anc is NULL without beam search: the ancestry call is also a plain one
    assert uses == {(1, True, False), (1, False, False), (2, False, False), (2, False, True)}, uses
    probe = (CSRC / "probe" / "whisper_probe.hip").read_text()
    assert sorted((int(a), int(b)) for a, b in re.findall(r"if \(qpw == (\d)\) return attn<(\d)>", probe)) == [(1, 1), (2, 2)]
    assert {q for q, _, _ in uses} == {1, 2}
    driven = {(c["qpw"], c["anc"], c["causal"]) for c in CASES}
    assert driven == uses, f"cases only: {driven - uses}, model only: {uses - driven}"
    # the kernel instantiations behind the wrapper: k_attn<QPW, ANC, CAUSAL> chosen by causal first, then anc
    wrapper = (CSRC / "whisper.hip").read_text()
    wrapper = wrapper[wrapper.index("int attn(eioku_whisper* m"):wrapper.index("// ---- the Whisper layer")]
    assert re.findall(r"k_attn<QPW, (\w+)(?:, (\w+))?>", wrapper) == [("false", "true"), ("true", ""), ("false", "")]


def _launches(path):
    """{kernel: {(grid, block, LDS bytes)}} of every hipLaunchKernelGGL of a plain kernel name in a source, as written"""
    text = re.sub(r"//[^\n]*", "", path.read_text())
    out = {}
    for m in re.finditer(r"hipLaunchKernelGGL\((\w+),\s*", text):
        out.setdefault(m.group(1), set()).add(tuple(_split_args(text, m.end())[:3]))
    return out


PROBED = {"whisper_probe.hip": ("whisper.hip", ["k_attn_weights", "k_embed", "k_embed_seq", "k_kv_to_cache", "k_gather_rows", "k_im2col_mel",
                                                "k_im2col_s2"]),
          "actions_probe.hip": ("actions.hip", ["k_attn_time"])}


@pytest.mark.parametrize("probe", list(PROBED))
def test_probe_launch_lines_are_the_models(probe):
    model, kernels = PROBED[probe]
    mine, theirs = _launches(CSRC / "probe" / probe), _launches(CSRC / model)
    assert sorted(mine) == sorted(kernels), f"{probe} launches {sorted(mine)}"
    for k in kernels:
        assert len(theirs[k]) == 1 and mine[k] == theirs[k], f"{k}: probe {mine[k]}, {model} {theirs[k]}"
    assert f'#include "../{model}"' in (CSRC / "probe" / probe).read_text()


def test_probe_names_behind_the_launch_lines_mean_the_same():
    """the launch lines are compared as text, so the names in them must mean the same on both sides"""
    wp, wh = (CSRC / "probe" / "whisper_probe.hip").read_text(), (CSRC / "whisper.hip").read_text()
    ap, ac = (CSRC / "probe" / "actions_probe.hip").read_text(), (CSRC / "actions.hip").read_text()
    lds = "const size_t lds = (size_t)4 * (ctx + 64) * sizeof(float);"
    assert lds in wp and lds in wh[wh.index("int cross_attn("):wh.index("// ---- workspaces")]
    lds = "const size_t lds = (size_t)3 * T * 66 * sizeof(h16) + 96 * sizeof(float);"
    assert lds in ap and lds in ac
    assert "const long long probs = (long long)n_seq * heads;" in ap and "const long long probs = (long long)B * P * m->heads;" in ac
    # prefill: M = R * P; encode: n1 over k1pad columns, n2 over M = B * ctx rows of 3 d, T2 = 2 * ctx
    assert "const int d = c.d_model, Tm = c.max_target_positions, M = R * P;" in wh and "const int M = R * P;" in wp
    assert "const size_t n1 = (size_t)B * T2 * m->k1pad, n2 = (size_t)M * 3 * d;" in wh
    assert "const int d = c.d_model, ctx = c.max_source_positions, T2 = 2 * ctx, M = B * ctx;" in wh
    assert "const size_t n1 = (size_t)B * T2 * k1pad;" in wp
    assert "const int ctx = T2 / 2, M = B * ctx;" in wp and "const size_t n2 = (size_t)M * 3 * d;" in wp
    # k_attn itself goes through the model's wrapper: the probe has no launch line for it
    assert "k_attn<" not in re.sub(r"//[^\n]*", "", wp)


def test_product_does_not_reference_the_new_probes():
    names = re.findall(r"int (eioku_probe_\w+)\(", "".join((CSRC / "probe" / p).read_text() for p in PROBED))
    assert sorted(names) == sorted(["eioku_probe_wh_attn", "eioku_probe_wh_attn_weights", "eioku_probe_attn_time", "eioku_probe_wh_embed",
                                    "eioku_probe_wh_embed_seq", "eioku_probe_wh_kv_to_cache", "eioku_probe_wh_gather_rows",
                                    "eioku_probe_wh_im2col_mel", "eioku_probe_wh_im2col_s2"])
    for path in list((ROOT / "eioku_amd").glob("*.py")) + [ROOT / "include" / "eioku_hip.h", ROOT / "bench.py", ROOT / "__graft_entry__.py"]:
        text = path.read_text()
        assert not any(n in text for n in names + ["libeioku_hip_probe", "whisper_probe", "actions_probe"]), path
    for f in ("whisper.hip", "actions.hip"):
        assert "probe" not in (CSRC / f).read_text().lower(), f
