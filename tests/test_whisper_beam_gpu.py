"""K20b on the device: beam search against tests/whisper_beam_oracle.py.

Model A (vocab 1003, ctx 100, 64 positions) in two forms: the beam fixture of tests/whisper_beam_cases.py (q / k
projections at He scale) wherever the margin rule is used, and the unmodified model of tests/test_whisper_gpu.py as well
for the tests that need no margin argument.  Model B (51865 ids, 811 blocks, the block straddling timestamp_begin) for
the supplied-logits test only.  Beams 3 and 5; 15 lanes and 20 lanes (past k_logits's 16-lane tile).

The figures these tests print, as measured on an MI355X, are in DESIGN.md "K20b beam search".
"""
import asyncio

import numpy as np
import pytest

import whisper_beam_cases as cases
import whisper_beam_oracle as wb
import whisper_oracle as wo
from whisper_testlib import recomputed_sums as _recomputed_sums, write_checkpoint as _write_checkpoint

pytestmark = pytest.mark.gpu

NEW = cases.NEW_TOKENS
SUM_BAR = 1e-4  # per token: fp32 log-sum-exp over <= 51865 terms against float64 (the bar of the greedy select test)


class BeamModel:
    def __init__(self, qk_scale=cases.QK_SCALE):
        from eioku_amd.transcribe import WhisperTranscriber

        self.soft = qk_scale != 1.0
        self.cfg, self.weights = cases.model_a_weights(qk_scale)
        self.o16 = wo.Oracle(self.cfg, self.weights, fp16=True)
        self.dev = WhisperTranscriber(dict(self.cfg), {k: v.numpy() for k, v in self.weights.items()})
        self.prompt = cases.prompt_of(self.cfg)
        self.frames = 2 * self.cfg["max_source_positions"]
        self._cases = {}

    def mel(self, name):
        return cases.mel_of(self.cfg, cases.PARITY_CASES[name][1])

    def case(self, name):
        """(W, mel, enc16, the oracle's beam search) of a parity case, computed once."""
        if name not in self._cases:
            W, seeds = cases.PARITY_CASES[name]
            mel = cases.mel_of(self.cfg, seeds)
            enc = self.o16.encode(mel)
            self._cases[name] = (W, mel, enc, wb.beam_search(self.o16, enc, self.prompt, NEW, W))
        return self._cases[name]


@pytest.fixture(scope="module")
def model(gpu):
    m = BeamModel()
    yield m
    m.dev.close()


@pytest.fixture(scope="module")
def sharp_model(gpu):
    """Model A with its q / k projections as tests/test_whisper_gpu.py has them: the tests that need no margin argument
    run on it too."""
    m = BeamModel(qk_scale=1.0)
    yield m
    m.dev.close()


@pytest.fixture(params=["soft", "sharp"])
def either_model(request, model, sharp_model):
    return model if request.param == "soft" else sharp_model


@pytest.fixture(scope="module")
def dev_b(gpu):
    from eioku_amd.transcribe import WhisperTranscriber

    cfg = wo.model_b_config()
    dev = WhisperTranscriber(dict(cfg), {k: v.numpy() for k, v in wo.random_weights(cfg, 7).items()})
    yield cfg, dev
    dev.close()


# ---- 1. one step on supplied logits ----------------------------------------------------------------------------------------------
def _check_step(got: dict, ref: dict, where: str):
    assert [(s, t) for s, t, _ in got["live"]] == [(s, t) for s, t, _ in ref["live"]], where
    assert [s for s, _ in got["finished"]] == [s for s, _ in ref["walked_eot"]], where
    err = [abs(a[2] - b[2]) for a, b in zip(got["live"], ref["live"])] + [abs(a[1] - b[1]) for a, b in zip(got["finished"], ref["walked_eot"])]
    assert max(err) <= SUM_BAR, (where, max(err))
    assert got["fin_count"] == ref["fin_count"] and got["complete"] == ref["complete"], where
    return max(err)


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("W", [3, 5])
def test_selection_is_exact_on_supplied_logits(model, dev_b, which, W):
    cfg, dev = (model.cfg, model.dev) if which == "a" else dev_b
    case = cases.select_case(cfg, W)
    got = dev.beam_select(case["logits"], case["prefixes"], case["sums"], case["fin_count"], W)
    worst = max(_check_step(g, r, f"model {which} W {W} window {b}") for b, (g, r) in enumerate(zip(got, cases.select_reference(case, cfg))))
    print(f"model {which} W {W}: largest sum error {worst:.3e}")


@pytest.mark.parametrize("W", [3, 5])
def test_ties_go_to_the_lower_slot_and_the_lower_id(model, W):
    case = cases.tie_case(model.cfg, W)
    (got,) = model.dev.beam_select(case["logits"], case["prefixes"], case["sums"], case["fin_count"], W)
    (ref,) = cases.select_reference(case, model.cfg)
    _check_step(got, ref, f"ties W {W}")
    live = [(s, t) for s, t, _ in got["live"]]
    assert live[0][0] == 0 and live[1] == (1, live[0][1]) and live[2:] == [(2, 20), (2, 63), (2, 64)][:W - 2]


def test_more_than_64_lanes_is_an_argument_error(model):
    case = cases.select_case(model.cfg, 5)
    with pytest.raises(RuntimeError, match="64 lanes"):
        model.dev.beam_select(np.tile(case["logits"][:5], (13, 1)), case["prefixes"][:5] * 13, np.tile(case["sums"][:5], 13), [0] * 13, 5)


# ---- 2. every hypothesis is self-consistent ----------------------------------------------------------------------------------------
def test_every_hypothesis_and_the_greedy_yardstick_are_self_consistent(either_model):
    m = either_model
    W, mel = 5, m.mel("w5_b4")
    B = len(mel)
    m.dev.encode(B, mel)
    res = m.dev.decode_beam(m.prompt, B, NEW, W)
    greedy = m.dev.decode(m.prompt, B, NEW)
    rows = [(b, [int(t) for t in res["tokens"][b, h, :res["n"][b, h]]]) for b in range(B) for h in range(res["n_hyp"][b])]
    assert len(rows) == B * W
    if m.soft:  # the fixture's windows: hypotheses that ended on EOT and hypotheses that ran to the last step
        assert any(res["ended"].ravel()) and not all(res["ended"].ravel())
    worst = 0.0
    for (b, toks), ref, h in zip(rows, _recomputed_sums(m, mel, rows), [h for b in range(B) for h in range(res["n_hyp"][b])]):
        assert (toks[-1] == m.cfg["eot"]) == bool(res["ended"][b, h]) and m.cfg["eot"] not in toks[:-1]
        err = abs(float(res["sum_logprob"][b, h]) - ref) / len(toks)
        worst = max(worst, err)
        assert err <= SUM_BAR, f"window {b} hypothesis {h}: returned {res['sum_logprob'][b, h]}, recomputed {ref}, {len(toks)} tokens"
    grows = [(b, [int(t) for t in greedy["tokens"][b, :greedy["n"][b]]]) for b in range(B)]
    gworst = max(abs(float(greedy["sum_logprob"][b]) - ref) / len(toks) for (b, toks), ref in zip(grows, _recomputed_sums(m, mel, grows)))
    print(f"{'soft' if m.soft else 'sharp'} model: self-consistency, worst |returned - recomputed| per token: beam {worst:.3e}, greedy yardstick {gworst:.3e}")
    assert gworst <= SUM_BAR
    for b in range(B):  # the best index is the ranking of the returned sums
        n = res["n_hyp"][b]
        score = res["sum_logprob"][b, :n].astype(np.float64) / np.maximum(1, res["n"][b, :n] - res["ended"][b, :n])
        assert int(res["best"][b]) == int(np.argmax(score))


# ---- 3. beam 1 is greedy ---------------------------------------------------------------------------------------------------------
def test_beam_1_equals_greedy(either_model):
    m = either_model
    mel = m.mel("w5_b4")
    B = len(mel)
    m.dev.encode(B, mel)
    greedy = m.dev.decode(m.prompt, B, NEW)
    beam = m.dev.decode_beam(m.prompt, B, NEW, 1)
    assert beam["tokens"].shape == (B, 1, NEW) and np.all(beam["n_hyp"] == 1) and np.all(beam["best"] == 0)
    assert np.array_equal(beam["tokens"][:, 0], greedy["tokens"]) and np.array_equal(beam["n"][:, 0], greedy["n"])
    assert np.array_equal(beam["ended"][:, 0] == 1, np.any(greedy["tokens"] == m.cfg["eot"], axis=1))
    err = np.abs(beam["sum_logprob"][:, 0].astype(np.float64) - greedy["sum_logprob"]) / greedy["n"]
    print(f"beam 1 against greedy: largest sum difference per token {err.max():.3e}")
    assert err.max() <= SUM_BAR
    assert beam["no_speech_prob"].tobytes() == greedy["no_speech_prob"].tobytes() and np.array_equal(beam["lang"], greedy["lang"])
    if m.soft:
        assert len(set(greedy["n"].tolist())) > 1  # lanes end at different steps


# ---- 4. free-running parity under the margin rule ------------------------------------------------------------------------------
def _step_drifts(m: BeamModel, W, mel, results):
    """[window][step]: the largest |device - fp16 oracle| over the vocabulary and the step's live slots, teacher-forced on
    the oracle's slot histories.  While the device has followed the oracle, its free-running logits ARE these."""
    B, P, eot = len(mel), len(m.prompt), m.cfg["eot"]
    m.dev.encode(B * W, np.repeat(mel, W, axis=0))
    drifts = [[] for _ in range(B)]
    for i in range(max(len(r["steps"]) for r in results)):
        ids = np.full((B * W, P + i), eot, dtype=np.int32)
        ids[:, :P] = m.prompt
        for b, r in enumerate(results):
            if i < len(r["steps"]):
                for j in cases.live_slots(r["steps"][i]):
                    ids[b * W + j, P:] = r["steps"][i]["slots"][j]["tokens"]
        logits = m.dev.forced_logits(ids)[:, -1]
        for b, r in enumerate(results):
            if i < len(r["steps"]):
                st = r["steps"][i]
                drifts[b].append(max(float(np.abs(logits[b * W + j] - st["logits"][j]).max()) for j in cases.live_slots(st)))
    return drifts


def test_free_running_parity_with_the_fp16_oracle(model):
    """Every next slot's (source, token) equals the oracle's while the oracle's margin exceeds 4 x the logit drift of the
    step (the maximum over the window's live beams); at the first thinner step the window stops being compared."""
    m = model
    all_results, all_compared, all_drift = [], [], []
    for name in cases.PARITY_CASES:
        W, mel, _, results = m.case(name)
        B = len(mel)
        drifts = _step_drifts(m, W, mel, results)
        m.dev.encode(B, mel)
        got = m.dev.decode_beam(m.prompt, B, NEW, W, trace=True)
        compared = []
        for b, r in enumerate(results):
            n = 0
            for i, st in enumerate(r["steps"]):
                if not st["margin"] > 4 * drifts[b][i]:
                    break
                want = [(s, t) for s, t, _ in st["live"]] + [(-1, -1)] * (W - len(st["live"]))
                have = list(zip(got["trace_src"][i, b].tolist(), got["trace_tok"][i, b].tolist()))
                have = [(s, t) if s >= 0 else (-1, -1) for s, t in have]
                assert have == want, f"{name} window {b} step {i}: device {have}, oracle {want} (margin {st['margin']:.4f}, drift {drifts[b][i]:.4f})"
                n += 1
            compared.append(n)
            if n == len(r["steps"]):  # the whole search was compared: the hypotheses and the ranking follow
                nh = len(r["hyps"])
                assert int(got["n_hyp"][b]) == nh and got["tokens"][b, :nh].tolist() == r["tokens"]
                assert got["n"][b, :nh].tolist() == r["n"]
        print(f"{name}: compared steps per window {compared} of {[len(r['steps']) for r in results]}")
        all_results += results
        all_compared += compared
        all_drift += [d for ds in drifts for d in ds]
    report = cases.fixture_report(all_results, all_compared)
    print(f"per-step logit drift device vs fp16 oracle: median {np.median(all_drift):.3e}, largest {max(all_drift):.3e}; {report}")
    assert report["windows_with_8"] >= 3, "fewer than three windows with 8 compared steps: the fixture is too thin"
    assert report["forks"] >= 1 and report["finishes"] >= 1


# ---- 5. batch and sync invariance -----------------------------------------------------------------------------------------------
KEYS = ("tokens", "n", "ended", "sum_logprob", "n_hyp", "best", "no_speech_prob", "lang")


def test_windows_in_a_batch_equal_the_same_windows_alone(either_model):
    m = either_model
    W, mel = 5, m.mel("w5_b4")
    B = len(mel)
    m.dev.encode(B, mel)
    batch = m.dev.decode_beam(m.prompt, B, NEW, W, sync_every=8)
    other = m.dev.decode_beam(m.prompt, B, NEW, W, sync_every=3)
    for key in KEYS:
        assert batch[key].tobytes() == other[key].tobytes(), key
    for b in range(B):
        m.dev.encode(1, mel[b:b + 1])
        alone = m.dev.decode_beam(m.prompt, 1, NEW, W)
        for key in KEYS:
            assert alone[key][0].tobytes() == batch[key][b].tobytes(), f"window {b}: {key}"
    # one window completes early (all W hypotheses ended well before the last step) while another runs to the last step
    done = [bool(np.all(batch["ended"][b, :batch["n_hyp"][b]])) for b in range(B)]
    early = [b for b in range(B) if done[b] and batch["n"][b].max() < NEW - 8]
    if m.soft:
        assert early and not all(done)


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------
def _segments_by_hand(m: BeamModel, calls, content_frames: int, seek_mode: bool):
    """The segments and the next seek per window from recorded ``decode_beam`` results: the best row's tokens, sum and the
    window's no-speech probability through skip_window / cut_window, written out here independently of transcribe()."""
    from eioku_amd.transcribe import cut_window, skip_window

    cfg, segments, nexts = m.cfg, [], []
    for offsets, res in calls:
        for lane, off in enumerate(offsets):
            seek = off // 160
            size = min(m.frames, content_frames - seek)
            h = int(res["best"][lane])
            toks = res["tokens"][lane, h].tolist()
            n_text = int(res["n"][lane, h] - res["ended"][lane, h])
            assert toks[:n_text].count(cfg["eot"]) == 0 and all(t == cfg["eot"] for t in toks[n_text:])
            advance = size
            if not skip_window(float(res["no_speech_prob"][lane]), float(res["sum_logprob"][lane, h]), n_text):
                pieces, adv = cut_window(toks, cfg["eot"], cfg["timestamp_begin"], seek * 10, size)
                segments += [{"start_ms": a, "end_ms": b, "text": "", "language": "en", "confidence": None, "words": None, "tokens": ids}
                             for a, b, ids in pieces if a != b and ids]
                if seek_mode:
                    advance = max(1, min(adv, size))
            nexts.append(seek + advance)
    return segments, nexts


@pytest.mark.parametrize("mode", ["seek", "fixed"])
def test_transcribe_wires_the_best_hypothesis_into_segments_and_seek(either_model, mode, monkeypatch):
    """transcribe(beam_size=5) on the device against skip_window / cut_window run by hand on the best hypotheses of the
    very decode_beam calls it made: which row is taken, with which sum and no-speech probability, and where seek mode
    starts the next window.  No drift argument is needed: both sides read the same device results."""
    m = either_model
    audio = np.concatenate([cases.audio(s, 2.0) for s in (140, 355, 27)])      # three windows' worth; best rows 4, 1, 0 in the oracle
    content = len(audio) // 160
    calls, offs = [], []
    real_logmel, real_beam = m.dev.logmel, m.dev.decode_beam
    monkeypatch.setattr(m.dev, "logmel", lambda offsets, fetch=True: (offs.append([int(o) for o in offsets]), real_logmel(offsets, fetch))[1])

    def beam(*a, **k):
        res = real_beam(*a, **k)
        calls.append((offs[-1], res))
        return res

    monkeypatch.setattr(m.dev, "decode_beam", beam)
    monkeypatch.setattr(m.dev, "decode", lambda *a, **k: pytest.fail("beam_size=5 took the greedy call"))
    got = m.dev.transcribe(audio, "en", window_mode=mode, batch_windows=2, max_new_tokens=NEW, beam_size=5)
    want, nexts = _segments_by_hand(m, calls, content, mode == "seek")
    assert got["segments"] == want and len(want) >= 1 and got["language"] == "en"
    starts = [o // 160 for os_, _ in calls for o in os_]
    if mode == "seek":
        assert all(len(os_) == 1 for os_, _ in calls) and starts == [0] + nexts[:-1] and nexts[-1] >= content
        assert not m.soft or any(0 < n % m.frames for n in nexts[:-1])        # a window that started where a pair ended
    else:
        assert [len(os_) for os_, _ in calls] == [2, 1] and starts == [0, m.frames, 2 * m.frames]
    best = [int(b) for _, res in calls for b in res["best"]]
    ended = [bool(res["ended"][i, b]) for _, res in calls for i, b in enumerate(res["best"])]
    print(f"{'soft' if m.soft else 'sharp'} {mode}: best rows {best}, ended {ended}")
    if m.soft:  # taking row 0, or only ended rows, would not pass
        assert any(b != 0 for b in best) and not all(ended)


def _comparable(r: dict, ds: list) -> bool:
    """The margin rule for a whole search: every step's margin above 4 x its drift, and the best hypothesis ahead of every
    other by more than the two scores can have moved (a sum moves by at most 2 x the summed drift)."""
    if not all(st["margin"] > 4 * d for st, d in zip(r["steps"], ds)):
        return False
    score = [h["sum_logprob"] / max(1, len(h["tokens"])) for h in r["hyps"]]
    move = [2 * sum(ds) / max(1, len(h["tokens"])) for h in r["hyps"]]
    b = r["best"]
    return all(i == b or score[b] - score[i] > 2 * (move[b] + move[i]) for i in range(len(score)))


@pytest.mark.parametrize("mode", ["seek", "fixed"])
@pytest.mark.parametrize("seed,max_new", cases.E2E_CASES)
def test_end_to_end_segments_equal_the_cutter_on_the_oracles_best_hypotheses(model, mode, seed, max_new):
    """transcribe(beam_size=5) on the device against the same host loop over the oracle's beam search.  A window is
    comparable when its whole search is above the margin (_comparable, with the drift the device shows teacher-forced on
    the oracle's slots).  The first window of each clip has to be comparable: its best hypothesis on the device is the
    oracle's and its segments are the oracle's.  In fixed mode that window is the whole clip and the whole result is
    compared.  Seek mode starts a second window inside the clip whose search has a step with a margin of 2e-4 to 1.2e-3:
    there only the first window's segments are compared with the oracle, and the wiring test above covers the rest."""
    m = model
    audio = cases.audio(seed, 2.0)
    log: list = []
    want = cases.oracle_transcriber(m.cfg, m.o16, log).transcribe(audio, "en", window_mode=mode, batch_windows=2,
                                                                  max_new_tokens=max_new, beam_size=5)
    ok = []
    for mel, rs, _ in log:
        drifts = _step_drifts(m, 5, mel, rs)
        ok.append([_comparable(r, ds) for r, ds in zip(rs, drifts)])
        m.dev.encode(len(rs), mel)
        res = m.dev.decode_beam(m.prompt, len(rs), max_new, 5)
        for b, r in enumerate(rs):
            if ok[-1][b]:
                h = int(res["best"][b])
                assert res["tokens"][b, h].tolist() == r["tokens"][r["best"]] and int(res["n"][b, h]) == r["n"][r["best"]]
    print(f"audio {seed} {mode}: comparable windows {ok}")
    assert ok[0][0], "the first window of this fixture is too thin to compare segments"
    got = m.dev.transcribe(audio, "en", window_mode=mode, batch_windows=2, max_new_tokens=max_new, beam_size=5)
    if mode == "fixed":  # one window, comparable: the whole result is the oracle's
        assert len(log) == 1 and got == want
    limit = log[1][2][0] // 16 if len(log) > 1 else 10 ** 9      # ms at which the second window starts
    first = [s for s in want["segments"] if s["end_ms"] <= limit]
    assert len(first) >= 1 and got["segments"][:len(first)] == first


def test_transcribe_video_with_beam_size_5_through_model_manager(model, tmp_path):
    from eioku_amd.model_manager import ModelManager

    m = model
    _write_checkpoint(tmp_path / "whisper" / "tiny-test", m.cfg, m.weights)
    audio = cases.audio(27, 2.0)
    mm = ModelManager(cache_dir=str(tmp_path), gpu_transcription=True, audio_source=lambda path: (audio, 16000))
    out = asyncio.run(mm.transcribe_video("clip.mp4", {"model_name": "tiny-test", "languages": ["en"], "beam_size": 5}))
    assert list(out) == ["segments"] and len(out["segments"]) >= 1
    for seg in out["segments"]:
        assert set(seg) == {"start_ms", "end_ms", "text", "language", "confidence", "words"}
        assert 0 <= seg["start_ms"] < seg["end_ms"] < 4000 and seg["language"] == "en" and seg["text"].startswith(" w")
    with pytest.raises(ValueError):
        asyncio.run(mm.transcribe_video("clip.mp4", {"model_name": "tiny-test", "languages": ["en"], "beam_size": 9}))
