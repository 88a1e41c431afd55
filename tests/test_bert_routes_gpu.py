"""GPU parity of the K8 encoder on EVERY kernel route, hidden width and mask shape (tests/bert_cases.py), against the
float64 numpy oracle at the project's bar (max|got - want| <= 1e-4 max|want|), with the launch code's own route log
(``embed.routes``) asserted for every case: the set of routes with non-zero counts AND the counts.  A retune that moves a
shape to another kernel fails here by name instead of quietly testing something else."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bert_cases as bc
from oracle import bert as obert
from eioku_amd import embed

pytestmark = pytest.mark.gpu


def _drift(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def _same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _nonzero(log):
    return {k: v for k, v in log.items() if v}


def _encode_logged(enc, ids, mask):
    embed.routes(reset=True)
    out = enc.encode_ids(ids, mask)
    return out, _nonzero(embed.routes(reset=True))


def _check(group, name, got, want, mask):
    d = _drift(got, want)
    print(f"bert-drift {group} {name}: {d:.3e}")
    assert d <= bc.RTOL, (group, name, d)
    live = mask.any(axis=1)
    assert np.allclose(np.linalg.norm(got[live], axis=1), 1.0, atol=1e-5)
    assert not got[~live].any() and not want[~live].any()  # a fully masked segment pools to the zero vector


def _run_case(group, key, B, S, route, ids, mask):
    cfg = bc.config(key)
    enc = embed.MiniLMEncoder(bc.state(key), cfg)
    got, log = _encode_logged(enc, ids, mask)
    enc.close()
    assert got.shape == (B, cfg["hidden"])
    assert log == bc.expected_log(route, cfg["layers"])
    _check(group, f"{key} {B}x{S}", got, obert.encode(bc.state(key), cfg, ids, mask), mask)


def test_log_lists_every_route_with_zeros(gpu):
    log = embed.routes(reset=True)
    assert len(log) == 26 and not any(embed.routes().values())
    for must in ("attn_bf", "attn8", "attn1", "gemm_bf<EPI1,T128,AS0>", "gemm_f32<EPI0,T128>", "gemm_f32_s<EPI1>", "add_ln",
                 "add_ln_fixed<6>", "add_ln_fixed<12>", "pool<G1>", "pool<G2>", "splits<1>", "splits<4>"):
        assert must in log


@pytest.mark.parametrize("B,S,route", bc.SEQ_EDGES, ids=[f"{b}x{s}" for b, s, _ in bc.SEQ_EDGES])
def test_sequence_length_edges(gpu, B, S, route):
    ids, mask = bc.prefix_inputs(bc.MINILM["vocab"], B, S, 1000 + S)
    assert mask[-1].all() and not mask.all() and ids.min() >= 1
    _run_case("a", "minilm", B, S, route, ids, mask)


@pytest.mark.parametrize("S,route", bc.MASK_SHAPES, ids=[f"S{s}" for s, _ in bc.MASK_SHAPES])
def test_mask_shapes(gpu, S, route):
    cfg, st = bc.MINILM, bc.state("minilm")
    ids, mask = bc.shaped_masks(cfg["vocab"], S, 2000 + S)
    enc = embed.MiniLMEncoder(st, cfg)
    got, log = _encode_logged(enc, ids, mask)
    assert log == bc.expected_log(route, cfg["layers"])
    want = obert.encode(st, cfg, ids, mask)
    for r, name in enumerate(bc.MASK_ROWS):
        print(f"bert-drift b S{S} {name}: {_drift(got[r], want[r]) if mask[r].any() else 0.0:.3e}")
    _check("b", f"S{S}", got, want, mask)
    # what lies under the mask cannot reach the result: other ids there, the same bytes
    ids2 = bc.redraw_masked(cfg["vocab"], ids, mask, 2500 + S)
    assert (ids2 != ids).sum() == (mask == 0).sum() and np.array_equal(ids2[mask == 1], ids[mask == 1])
    assert _same_bytes(enc.encode_ids(ids2, mask), got)
    enc.close()


@pytest.mark.parametrize("B,S,route", bc.LARGE_M, ids=[f"{b}x{s}" for b, s, _ in bc.LARGE_M])
def test_large_m_tile_tails(gpu, B, S, route):
    ids, mask = bc.prefix_inputs(bc.MINILM_2L["vocab"], B, S, 3000 + B)
    _run_case("c", "minilm_2l", B, S, route, ids, mask)


# ---------------------------------------------------------------------------------------------------------------------
# d. the switches, one child process each (they are read once per process)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def children(gpu, tmp_path_factory):
    """name -> (outputs, logs) of the child run with CHILD_ENVS[name].  One child at a time, each under its own time
    limit; the first one that does not exit 0 ends the fixture (and with it every test below): nothing is started after it."""
    tmp = tmp_path_factory.mktemp("bert_children")
    res = {}
    for name, env in bc.CHILD_ENVS.items():
        path = tmp / f"{name}.npz"
        clean = {k: v for k, v in os.environ.items() if k not in ("EIOKU_GEMM_BF16", "EIOKU_GEMM_S", "EIOKU_ATTN_MFMA",
                                                                  "EIOKU_GEMM_PLANES")}
        subprocess.run([sys.executable, bc.__file__, str(path)], check=True, env=dict(clean, **env), timeout=300)
        z = np.load(path)
        n = len(bc.CHILD_SHAPES)
        res[name] = ([z[f"out{i}"] for i in range(n)], [_nonzero(json.loads(str(z[f"log{i}"]))) for i in range(n)])
    return res


@pytest.fixture(scope="module")
def child_want():
    return [obert.encode(bc.state(key), bc.config(key), *bc.child_inputs(i)) for i, (key, _, _) in enumerate(bc.CHILD_SHAPES)]


@pytest.mark.parametrize("name", list(bc.CHILD_ENVS))
def test_switch_routes_match_the_oracle(children, child_want, name):
    outs, logs = children[name]
    for i, (key, B, S) in enumerate(bc.CHILD_SHAPES):
        assert logs[i] == bc.expected_log(bc.CHILD_ROUTES[name][i], bc.config(key)["layers"]), (name, key, B, S)
        _check("d", f"{name} {key} {B}x{S}", outs[i], child_want[i], bc.child_inputs(i)[1])


def test_switch_routes_take_the_kernels_they_name(children):
    def seen(name):
        return set().union(*children[name][1])

    fma = seen("fma")
    assert {"gemm_f32<EPI0,T64>", "gemm_f32<EPI1,T64>", "gemm_f32<EPI0,T128>", "gemm_f32<EPI1,T128>", "attn8", "attn1"} <= fma
    assert not any(r.startswith("gemm_bf") or r == "attn_bf" for r in fma)
    assert {"gemm_f32_s<EPI0>", "gemm_f32_s<EPI1>"} <= seen("fma_s")
    assert {"gemm_bf<EPI0,T64,AS0>", "gemm_bf<EPI1,T64,AS0>", "gemm_bf<EPI0,T128,AS0>", "gemm_bf<EPI1,T128,AS0>"} <= seen("no_planes")
    assert not any("AS0" in r for r in seen("default"))


def test_planes_and_staging_split_give_the_same_bytes(children):
    """Activations as bf16 planes written by their producers vs fp32 activations split in the GEMM's staging threads: the
    same split of the same values, at one tile, several tiles with a tail, and the 128-row tile with a tail."""
    for i, shape in enumerate(bc.CHILD_SHAPES):
        assert _same_bytes(children["no_planes"][0][i], children["default"][0][i]), shape


# ---------------------------------------------------------------------------------------------------------------------
# e. other widths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,attn", bc.WIDTH_SHAPES, ids=[f"{b}x{s}" for b, s, _ in bc.WIDTH_SHAPES])
@pytest.mark.parametrize("hidden,ffn,sp_o,sp_f", bc.WIDTHS, ids=[f"w{h}x{f}" for h, f, _, _ in bc.WIDTHS])
def test_other_widths(gpu, hidden, ffn, sp_o, sp_f, B, S, attn):
    ids, mask = bc.prefix_inputs(500, B, S, 4000 + hidden + S)
    _run_case("e", f"w{hidden}x{ffn}", B, S, bc.width_route(hidden, sp_o, sp_f, attn), ids, mask)


def test_sequence_as_long_as_the_position_table(gpu):
    hidden, ffn, B, S = bc.WIDTH_MAXPOS
    assert S == bc.width_cfg(hidden, ffn)["max_pos"]
    ids, mask = bc.prefix_inputs(500, B, S, 4999)
    _run_case("e", f"w{hidden}x{ffn}", B, S, bc.width_route(hidden, 2, 1, "attn8"), ids, mask)


# ---------------------------------------------------------------------------------------------------------------------
# f. one handle across shapes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_handle_reuse_across_shapes(gpu, on_device):
    """The grow() buffers and the plane pointers (their offsets depend on the token count) keep nothing of an earlier
    call: every result of a reused encoder is, byte for byte, a fresh encoder's."""
    import torch

    cfg, st = bc.MINILM, bc.state("minilm")

    def run(enc, ids, mask):
        if not on_device:
            return _encode_logged(enc, ids, mask)
        out, log = _encode_logged(enc, torch.from_numpy(ids).to(gpu), torch.from_numpy(mask).to(gpu))
        return out.cpu().numpy(), log

    reused = embed.MiniLMEncoder(st, cfg)
    got = []
    for i, (B, S, route) in enumerate(bc.REUSE_ORDER):
        ids, mask = bc.prefix_inputs(cfg["vocab"], B, S, 5000 + 10 * B + S)
        out, log = run(reused, ids, mask)
        assert log == bc.expected_log(route, cfg["layers"]), (B, S)
        fresh = embed.MiniLMEncoder(st, cfg)
        assert _same_bytes(out, run(fresh, ids, mask)[0]), (i, B, S)
        fresh.close()
        got.append(out)
    reused.close()
    assert bc.REUSE_ORDER[1][:2] == bc.REUSE_ORDER[4][:2] and _same_bytes(got[1], got[4])


# ---------------------------------------------------------------------------------------------------------------------
# g. closure
# ---------------------------------------------------------------------------------------------------------------------
def test_every_route_of_the_log_has_a_case(gpu):
    """The union of the route sets the cases above assert is the full list of names the log reports: a route added
    later without a case fails here by name (or is listed in UNREACHABLE with its reason)."""
    known = set(embed.routes())
    covered = bc.all_expected_routes()
    assert not (set(bc.UNREACHABLE) & covered), "listed as unreachable but expected by a case"
    assert set(bc.UNREACHABLE) <= known
    assert covered | set(bc.UNREACHABLE) == known, (sorted(known - covered - set(bc.UNREACHABLE)), sorted(covered - known))
