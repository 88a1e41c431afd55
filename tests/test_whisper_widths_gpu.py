"""K19 / K20 / K20b / K21 on the device at the widths, mel bins and id layout of real checkpoints, against the CPU oracles.

Model C (tests/whisper_oracle.py): the large-v3 layout - 128 mel bins, 51866 ids, 100 languages, every special id one above
model B's - at d 384 (a second, partial trip of the 256-thread loops over d), 6 heads, 2 + 3 layers, ffn 1536 / 768 and
ctx 200 (3 x 64 + 8 keys).  Model D: model A's ids and ctx at d 1280, 20 heads and ffn 5120 (K = 1280 and K = 5120 in the
GEMMs).  The model class, the drift bar and the margin rule are those of tests/test_whisper_gpu.py.  "C soft" / "D soft" are
the same models with the q / k projections x 2 instead of x 4: the fixtures of the free-running comparison (see there).

The figures these tests print, as measured on an MI355X, are in DESIGN.md "K19 / K20".
"""
import asyncio

import numpy as np
import pytest

import whisper_align_oracle as wa
import whisper_oracle as wo
from test_whisper_gpu import Model, _assert_within_2_ulps, _audio, _check_drift, _compare_greedy, _fixture_is_useful, _forced_ids, _info_checks
from whisper_testlib import forced_rows, recomputed_sums, sums_from_logits, write_checkpoint

pytestmark = pytest.mark.gpu

NEW = 16
SUM_BAR = 1e-4  # per token, the bar of tests/test_whisper_beam_gpu.py: fp32 log-sum-exp over <= 51866 terms against float64
SOT_LEN = 3


@pytest.fixture(scope="module")
def model_c(gpu):
    m = Model(wo.model_c_config(), seed=5, audio_seeds=(3, 5, 6), seconds=4.0, new_tokens=NEW)
    yield m
    m.dev.close()


@pytest.fixture(scope="module")
def model_d(gpu):
    m = Model(wo.model_d_config(), seed=5, audio_seeds=(3, 5, 6), seconds=2.0, new_tokens=NEW)
    yield m
    m.dev.close()


# The free-running comparison needs oracle margins above 4 x the device's logit drift.  With q / k projections x 4 the drift
# of an fp16 realisation is far above the margins at these widths (the CPU fp16 oracle against the fp32 one over the first 8
# sampled positions: 0.7 - 1.2 at model C against margins of 0.04 - 0.16; 0.12 - 0.14 at model D against 0.05 - 0.15).  At
# q / k x 2 that drift is 0.02 - 0.035 (C) and 0.017 - 0.023 (D), and these audio seeds are the ones whose smallest margin
# among the first 8 steps is 0.229 / 0.123 / 0.245 (C) and 0.400 / 0.548 / 0.249 (D): all chosen on the CPU, from the oracle.
@pytest.fixture(scope="module")
def model_c_soft(gpu):
    m = Model(wo.model_c_config(), seed=5, audio_seeds=(8, 20, 43), seconds=4.0, new_tokens=NEW, qk_scale=2.0)
    yield m
    m.dev.close()


@pytest.fixture(scope="module")
def model_d_soft(gpu):
    m = Model(wo.model_d_config(), seed=5, audio_seeds=(3, 5, 6), seconds=2.0, new_tokens=NEW, qk_scale=2.0)
    yield m
    m.dev.close()


@pytest.fixture(params=["C", "D", "C soft", "D soft"])
def either(request):
    return request.param, request.getfixturevalue("model_" + request.param.lower().replace(" ", "_"))


@pytest.fixture(params=["C soft", "D", "D soft"])
def greedy_model(request):
    return request.param, request.getfixturevalue("model_" + request.param.lower().replace(" ", "_"))


def test_fixtures_decode_varied_audio_dependent_tokens(model_c, model_d, model_c_soft, model_d_soft):
    for m in (model_c, model_d, model_c_soft, model_d_soft):
        assert m.frames == 2 * m.cfg["max_source_positions"] and all(len(g["tokens"]) == NEW for g in m.greedy16)
        _fixture_is_useful(m)
        tb = m.cfg["timestamp_begin"]
        for g in m.greedy16:  # timestamps and text, from both halves of the vocabulary
            text = [t for t in g["tokens"] if t < m.cfg["eot"]]
            assert any(t >= tb for t in g["tokens"]) and min(text) < m.cfg["eot"] // 2 <= max(text)


# ---- 1. log-mel at 128 bins -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["full", "short", "silence", "offsets"])
def test_log_mel_at_128_bins_equals_the_float64_oracle(model_c, case):
    dev, frames = model_c.dev, model_c.frames
    assert frames == 400
    if case == "full":
        audio, offsets = _audio(21, 5.0), [0]
    elif case == "short":
        audio, offsets = _audio(22, 2.5), [0]                       # zeros past the clip's end
    elif case == "silence":
        audio, offsets = np.zeros(16000 * 3, dtype=np.float32), [0]
    else:
        audio, offsets = _audio(23, 9.0), [0, 12345, 80000]          # 12345 is no multiple of the hop; the last window ends the audio
    dev.set_audio(audio)
    got = dev.logmel(offsets)
    ref = np.stack([wo.log_mel(audio, o, frames, 128) for o in offsets])
    assert got.shape == ref.shape == (len(offsets), 128, frames)
    _assert_within_2_ulps(got, ref)
    if case == "silence":
        assert np.all(got == np.float32(-1.5))
    else:  # rows 80 .. 127 carry signal of their own: the floor (max - 8) is not what is compared there
        assert np.ptp(ref[:, 80:]) > 0.5 and np.all(ref[:, 80:].max(axis=(0, 2)) > ref.max() - 2.0 + 1e-3)


# ---- 2. encoder output and teacher-forced logits ----------------------------------------------------------------------------------
def test_encoder_and_logits_drift(either):
    """Three windows at once, then each alone: the 2 x CPU-fp16-drift bar on the encoder output and on the logits of both
    device routes (position by position, and the one-pass prefill), and the same bits per lane at B = 1 and B = 3."""
    name, m = either
    ids = _forced_ids(m, 3)
    assert ids.shape == (3, 8)
    ref32 = m.o32.forced_logits(m.enc32, ids).numpy()
    ref16 = m.o16.forced_logits(m.enc16, ids).numpy()
    m.dev.encode(3, m.mel)
    enc3 = m.dev.encoder_output(3)
    step3 = m.dev.forced_logits(ids)
    pre3 = m.dev.prefill_logits(ids)
    _check_drift(f"{name} encoder", enc3.astype(np.float32), m.enc32.numpy(), m.enc16.numpy())
    _check_drift(f"{name} logits, stepwise", step3, ref32, ref16)
    _check_drift(f"{name} logits, prefill", pre3, ref32, ref16)
    for lane in range(3):
        m.dev.encode(1, m.mel[lane:lane + 1])
        assert np.array_equal(m.dev.encoder_output(1)[0].view(np.uint16), enc3[lane].view(np.uint16)), f"lane {lane}"
        step1, pre1 = m.dev.forced_logits(ids[lane:lane + 1]), m.dev.prefill_logits(ids[lane:lane + 1])
        assert np.array_equal(step1[0].view(np.uint32), step3[lane].view(np.uint32)), f"lane {lane}, stepwise"
        assert np.array_equal(pre1[0].view(np.uint32), pre3[lane].view(np.uint32)), f"lane {lane}, prefill"
        _check_drift(f"{name} logits, stepwise, lane {lane} alone", step1, ref32[lane:lane + 1], ref16[lane:lane + 1])
        _check_drift(f"{name} logits, prefill, lane {lane} alone", pre1, ref32[lane:lane + 1], ref16[lane:lane + 1])


# ---- 3. greedy decode ------------------------------------------------------------------------------------------------------------
def test_greedy_decode(greedy_model):
    name, m = greedy_model
    lanes = [0, 1, 2]
    m.position_drift()
    m.dev.encode(3, m.mel)
    res = m.dev.decode(m.prompt, 3, NEW)
    compared, stops = _compare_greedy(m, res, lanes)
    reached = [m.greedy16[b]["n"] if s is None else s for b, s in enumerate(stops)]
    print(f"model {name}: {compared} compared steps, thin-margin stops {stops}, steps compared per lane {reached}; "
          f"smallest oracle margin among the first 8 steps {[round(min(g['margins'][:8]), 4) for g in m.greedy16]}, "
          f"largest 4 x drift among them {[round(4 * max(m.step_drift(b, i) for i in range(8)), 4) for b in lanes]}")
    assert sum(r >= 8 for r in reached) >= 2, "fewer than two lanes compare their first 8 steps: the fixture is too thin"
    _info_checks(m, res, lanes)
    assert len(m.cfg["lang_ids"]) == (100 if name[0] == "C" else 4)
    assert all(int(t) in m.cfg["lang_ids"] for t in res["lang"])


# ---- 4. lanes alone and in a batch -------------------------------------------------------------------------------------------------
def test_lanes_in_a_batch_equal_the_same_lanes_alone(model_c):
    m = model_c
    m.dev.encode(3, m.mel)
    batch = m.dev.decode(m.prompt, 3, NEW, sync_every=8)
    other = m.dev.decode(m.prompt, 3, NEW, sync_every=3)
    for key in ("tokens", "n", "sum_logprob", "no_speech_prob", "lang"):
        assert np.array_equal(batch[key], other[key]), key
    for lane in range(3):
        m.dev.encode(1, m.mel[lane:lane + 1])
        alone = m.dev.decode(m.prompt, 1, NEW)
        assert np.array_equal(alone["tokens"][0], batch["tokens"][lane]), f"lane {lane}"
        assert alone["n"][0] == batch["n"][lane]
        assert alone["sum_logprob"][0].tobytes() == batch["sum_logprob"][lane].tobytes()
        assert alone["no_speech_prob"][0].tobytes() == batch["no_speech_prob"][lane].tobytes()
    assert len({tuple(t) for t in batch["tokens"].tolist()}) == 3  # three different lanes, not one lane three times


# ---- 5. rules and argmax on supplied logits ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [-4.0, 6.0])
def test_rules_and_argmax_on_supplied_logits(model_c, shift):
    m, cfg = model_c, model_c.cfg
    prefixes = list(wo.scripted_prefixes(cfg).values())
    logits = np.stack([wo.scripted_logits(cfg, 100 + i, shift) for i in range(len(prefixes))])
    tok, lp, masked = m.dev.select(logits, prefixes)
    for i, prefix in enumerate(prefixes):
        ref = wo.apply_rules(logits[i], prefix, cfg)
        assert np.array_equal(np.isneginf(masked[i]), np.isneginf(ref)), f"mask differs for prefix {prefix}"
        keep = np.isfinite(ref)
        assert np.array_equal(masked[i][keep], logits[i][keep])
        rtok, rlp, _ = wo.select(ref, cfg)
        assert tok[i] == rtok, f"prefix {prefix}: device {tok[i]}, oracle {rtok}"
        assert abs(lp[i] - rlp) <= 1e-4  # fp32 log-sum-exp over <= 51866 terms against float64


def test_argmax_ties_across_the_last_workgroup_edge_go_to_the_lower_id(model_c):
    """51866 = 810 x 64 + 26: ids 51839 | 51840 straddle the edge of the last, partial workgroup, whose last id is 51865."""
    cfg = model_c.cfg
    tb, last = cfg["timestamp_begin"], cfg["vocab"] - 1
    assert last == 51865 and 51840 % 64 == 0 and cfg["vocab"] % 64 == 26 and tb < 51839
    z = np.full((3, cfg["vocab"]), -5.0, dtype=np.float32)
    z[0, [last, 51840, 51839]] = 9.0             # all three
    z[1, [last, 51840]] = 9.0                    # both inside the partial workgroup
    z[2, [last, 51839]] = 9.0                    # the first and the last workgroup of the pair
    prefix = [tb + 3, 10, 11]
    tok, lp, _ = model_c.dev.select(z, [prefix] * 3)
    assert tok.tolist() == [51839, 51840, 51839]
    for i in range(3):
        rtok, rlp, margin = wo.select(wo.apply_rules(z[i], prefix, cfg), cfg)
        assert rtok == tok[i] and margin == 0.0 and abs(lp[i] - rlp) <= 1e-4


# ---- 6. beam search over 6 heads ---------------------------------------------------------------------------------------------------
def _rule_7_gaps(m: Model, logits, toks) -> float:
    """The smallest |lse(timestamps) - max(text)| over a row's steps where both sides are finite (inf: rule 7 never decides)."""
    cfg, P, tb, gap = m.cfg, len(m.prompt), m.cfg["timestamp_begin"], np.inf
    for i in range(len(toks)):
        z = wo.apply_rules(logits[P - 1 + i], list(toks[:i]), cfg)
        a, b = wo._lse(z[tb:]), z[:tb].max()
        if np.isfinite(a) and np.isfinite(b):
            gap = min(gap, abs(a - b))
    return gap


@pytest.mark.parametrize("which", ["C", "C soft"])
def test_beam_hypotheses_and_the_greedy_yardstick_are_self_consistent(request, which):
    """What tests/test_whisper_beam_gpu.py asserts of every hypothesis, at 6 heads and beam 3: the returned sum of
    log-probabilities is the sum recomputed by teacher-forcing the hypothesis's tokens, (a) on the device (whisper_testlib.
    recomputed_sums: the device's forced_logits, then the oracle's rules and log-softmax in float64) within that test's bar,
    and (b) on the fp16 oracle.  (b) would still notice a mistake that every attention launch shares.  Its bar, per token:
    log-softmax moves by at most 2 x what the logits move by; the device's logits are within 3 D of the fp16 oracle's, D =
    max |fp16 oracle - fp32 oracle| on the row's own logits (|device - fp32| <= 2 D is the drift rule of test 2, and |fp32 -
    fp16| = D), so 6 D + the bar of (a) - provided rule 7 decides the same way under both logits, which it does where the
    fp16 oracle's rule-7 gap is above 6 D at every step of the row; rows with a thinner gap are left to (a).  At q / k x 4
    D is of the order of 1 and (b) says little; at q / k x 2 it is 0.03."""
    m = request.getfixturevalue("model_" + which.lower().replace(" ", "_"))
    W, B = 3, 2
    mel = m.mel[:B]
    m.dev.encode(B, mel)
    res = m.dev.decode_beam(m.prompt, B, NEW, W)
    greedy = m.dev.decode(m.prompt, B, NEW)
    slots = [(b, h) for b in range(B) for h in range(res["n_hyp"][b])]
    rows = [(b, [int(t) for t in res["tokens"][b, h, :res["n"][b, h]]]) for b, h in slots]
    assert len(rows) == B * W and len({tuple(t) for _, t in rows}) == B * W
    worst = 0.0
    for (b, toks), ref, (_, h) in zip(rows, recomputed_sums(m, mel, rows), slots):
        assert (toks[-1] == m.cfg["eot"]) == bool(res["ended"][b, h]) and m.cfg["eot"] not in toks[:-1]
        err = abs(float(res["sum_logprob"][b, h]) - ref) / len(toks)
        worst = max(worst, err)
        assert err <= SUM_BAR, f"window {b} hypothesis {h}: returned {res['sum_logprob'][b, h]}, recomputed {ref}, {len(toks)} tokens"
    grows = [(b, [int(t) for t in greedy["tokens"][b, :greedy["n"][b]]]) for b in range(B)]
    gworst = max(abs(float(greedy["sum_logprob"][b]) - ref) / len(toks) for (b, toks), ref in zip(grows, recomputed_sums(m, mel, grows)))
    print(f"model {which} beam 3: self-consistency, worst |returned - recomputed| per token: beam {worst:.3e}, greedy yardstick {gworst:.3e}; "
          f"hypothesis lengths {[len(t) for _, t in rows]}")
    assert gworst <= SUM_BAR
    for b in range(B):  # the best index is the ranking of the returned sums
        n = res["n_hyp"][b]
        score = res["sum_logprob"][b, :n].astype(np.float64) / np.maximum(1, res["n"][b, :n] - res["ended"][b, :n])
        assert int(res["best"][b]) == int(np.argmax(score))
    # (b) the same sums through the fp16 oracle
    ids, win, P = forced_rows(m, rows), [b for b, _ in rows], len(m.prompt)
    l16 = m.o16.forced_logits(m.enc16[win], ids).numpy().astype(np.float64)
    l32 = m.o32.forced_logits(m.enc32[win], ids).numpy().astype(np.float64)
    compared = []
    for r, ((b, toks), s16, (_, h)) in enumerate(zip(rows, sums_from_logits(m, l16, rows), slots)):
        D = float(np.abs(l16[r, P - 1:P - 1 + len(toks)] - l32[r, P - 1:P - 1 + len(toks)]).max())
        gap, err = _rule_7_gaps(m, l16[r], toks), abs(float(res["sum_logprob"][b, h]) - s16) / len(toks)
        print(f"window {b} hypothesis {h}: |returned - fp16 oracle| per token {err:.3e}, bar 6 D + {SUM_BAR} = {6 * D + SUM_BAR:.3e}, "
              f"smallest rule-7 gap {gap:.3e}{'' if gap > 6 * D else ' (not compared)'}")
        if gap > 6 * D:
            compared.append(r)
            assert err <= 6 * D + SUM_BAR
    if which == "C soft":
        assert len(compared) >= len(rows) // 2, "fewer than half the hypotheses have rule-7 gaps above 6 D: the fixture is too thin"


# ---- 7. word alignment with heads >= 2 ----------------------------------------------------------------------------------------------
class _AlignCase:
    """Two rows on model C: a full window (400 frames) and one with 260 content frames, text of 18 and 4 tokens."""

    def __init__(self, m: Model):
        cfg = m.cfg
        self.n_frames = [m.frames, 260]
        self.mel = np.stack([m.mel[0], wo.log_mel(m.audios[1][:260 * 160], 0, m.frames, cfg["n_mels"])])
        rng = np.random.default_rng(77)
        self.text = [[int(t) for t in rng.integers(10, 290, size=n)] for n in (18, 4)]
        seqs = [wa.sequence(cfg, m.prompt, t) for t in self.text]
        self.n_tok = [len(q) for q in seqs]
        self.seqs = [q + [cfg["eot"]] * (max(self.n_tok) - len(q)) for q in seqs]
        self.o32, self.o16 = wa.AlignOracle(cfg, m.weights, fp16=False), wa.AlignOracle(cfg, m.weights, fp16=True)
        self.enc32, self.enc16 = self.o32.encode(self.mel), self.o16.encode(self.mel)

    def refs(self, m: Model, row: int, heads):
        args = (m.prompt, self.text[row], self.n_frames[row], heads)
        return self.o32.align(self.enc32[row:row + 1], *args), self.o16.align(self.enc16[row:row + 1], *args)


@pytest.fixture(scope="module")
def align_cases():
    return {}


@pytest.mark.parametrize("heads", [[(2, 5), (1, 3), (2, 0)], None], ids=["three-heads", "default"])
@pytest.mark.parametrize("which", ["C", "C soft"])
def test_align_with_heads_above_1(request, align_cases, which, heads):
    """The drift rule on the alignment pass: device against the fp32 oracle within twice what the fp16 oracle shows against
    it on the same rows, for the cost and for the token probabilities; the jumps are the warping of the device's own cost."""
    m = request.getfixturevalue("model_" + which.lower().replace(" ", "_"))
    if which not in align_cases:
        align_cases[which] = _AlignCase(m)
    c = align_cases[which]
    assert wa.default_heads(m.cfg) == [(l, h) for l in (1, 2) for h in range(6)] and c.n_tok == [23, 9]
    m.dev.encode(2, c.mel)
    m.dev.set_alignment_heads(heads)
    try:
        got = m.dev.align(c.seqs, c.n_tok, SOT_LEN, c.n_frames, cost=True)
        assert got["cost"].shape == (2, 19, 200) and got["jump"].shape == (2, 19)
        dev_cost = dev_prob = bar_cost = bar_prob = 0.0
        dev_cells, bar_cells = [], []
        for r in range(2):
            r32, r16 = c.refs(m, r, heads)
            N, F = len(c.text[r]) + 1, c.n_frames[r] // 2
            cost = got["cost"][r, :N, :F]
            assert np.all(got["cost"][r, N:] == 0) and np.all(got["cost"][r, :, F:] == 0)
            dev_cost = max(dev_cost, float(np.abs(cost.astype(np.float64) - r32["cost"]).max()))
            bar_cost = max(bar_cost, 2 * float(np.abs(r16["cost"] - r32["cost"]).max()))
            dev_cells.append(np.abs(cost.astype(np.float64) - r32["cost"]).ravel())
            bar_cells.append(2 * np.abs(r16["cost"] - r32["cost"]).ravel())
            ti, fi = wa.dtw(cost)
            assert got["jump"][r, :N].tolist() == wa.jumps(ti, fi, N).tolist() and np.all(got["jump"][r, N:] == -1)
            assert np.all(np.diff(got["jump"][r, :N]) >= 0) and 0 <= got["jump"][r, 0] and got["jump"][r, N - 1] < F
            dev_prob = max(dev_prob, float(np.abs(got["prob"][r, :N - 1].astype(np.float64) - r32["prob"]).max()))
            bar_prob = max(bar_prob, 2 * float(np.abs(r16["prob"] - r32["prob"]).max()))
            assert np.all(got["prob"][r, N - 1:] == 0) and np.all(got["prob"][r, :N - 1] > 0) and np.all(got["prob"][r] <= 1)
        dev_mean, bar_mean = float(np.concatenate(dev_cells).mean()), float(np.concatenate(bar_cells).mean())
        print(f"align at model {which} ({'default heads' if heads is None else heads}): |cost - fp32 oracle| largest {dev_cost:.3e}, bar (2 x CPU "
              f"fp16 drift) {bar_cost:.3e}, mean {dev_mean:.3e}, bar {bar_mean:.3e}; largest |prob - fp32 oracle| {dev_prob:.3e}, bar {bar_prob:.3e}")
        # the padded row alone, picked through the window list: the same bits
        alone = m.dev.align([c.seqs[1][:c.n_tok[1]]], [c.n_tok[1]], SOT_LEN, [c.n_frames[1]], windows=[1], cost=True)
        N, F = c.n_tok[1] - SOT_LEN - 1, c.n_frames[1] // 2
        assert alone["cost"].shape == (1, N, F)
        assert alone["cost"][0].tobytes() == np.ascontiguousarray(got["cost"][1, :N, :F]).tobytes()
        assert alone["jump"][0].tolist() == got["jump"][1, :N].tolist()
        assert alone["prob"][0].tobytes() == np.ascontiguousarray(got["prob"][1, :N]).tobytes()
    finally:
        m.dev.set_alignment_heads(None)
    # the largest cell is one flipped fp16 rounding under a sharp softmax; the mean over the cells is the informative figure
    assert dev_cost <= bar_cost and dev_mean <= bar_mean and dev_prob <= bar_prob


# ---- 8. the product path on large-v3-shaped files ------------------------------------------------------------------------------------
def test_transcribe_video_through_model_manager_on_a_large_v3_shaped_checkpoint(model_c, tmp_path, monkeypatch):
    from eioku_amd import transcribe
    from eioku_amd.model_manager import ModelManager

    m = model_c
    write_checkpoint(tmp_path / "whisper" / "c-test", m.cfg, m.weights)
    loaded = []
    real = transcribe.WhisperTranscriber.from_cache.__func__

    def from_cache(cls, *a, **k):
        t = real(cls, *a, **k)
        loaded.append(dict(t.dims))
        return t

    monkeypatch.setattr(transcribe.WhisperTranscriber, "from_cache", classmethod(from_cache))
    audio = m.audios[0]
    mm = ModelManager(cache_dir=str(tmp_path), gpu_transcription=True, audio_source=lambda path: (audio, 16000))
    out = asyncio.run(mm.transcribe_video("clip.mp4", {"model_name": "c-test", "languages": ["en"]}))
    assert len(loaded) == 1
    for key, want in m.cfg.items():
        if key != "translate":
            assert loaded[0][key] == want, key
    assert list(out) == ["segments"] and len(out["segments"]) >= 1
    for seg in out["segments"]:
        assert set(seg) == {"start_ms", "end_ms", "text", "language", "confidence", "words"}
        # seek mode: a window may start anywhere before the audio's end (4 s); the layout's 1501 timestamp ids reach 30 s past
        # a window's start whatever the window's length (model C keeps large-v3's ids on a 4 s window)
        assert 0 <= seg["start_ms"] < seg["end_ms"] <= 4000 + 30000 and seg["language"] == "en" and seg["text"].startswith(" w")
