"""K20b, host side (no GPU): the beam-search oracle against the greedy oracle and a hand-computed search, and the
conditions the GPU fixtures of tests/test_whisper_beam_gpu.py have to meet, checked on the oracle alone."""
import asyncio
import math

import numpy as np
import pytest

import whisper_beam_cases as cases
import whisper_beam_oracle as wb
import whisper_oracle as wo
from eioku_amd import transcribe
from eioku_amd.model_manager import ModelManager


@pytest.fixture(scope="module")
def model():
    cfg, w = cases.model_a_weights()
    return cfg, wo.Oracle(cfg, w, fp16=True), wo.Oracle(cfg, w, fp16=False)


def test_beam_1_equals_the_greedy_oracle_token_for_token(model):
    cfg, o16, _ = model
    enc = o16.encode(cases.mel_of(cfg, (33, 140, 27)))
    prompt = cases.prompt_of(cfg)
    greedy = o16.greedy(enc, prompt, 12)
    beam = wb.beam_search(o16, enc, prompt, 12, 1)
    assert any(g["n"] < 12 for g in greedy) and any(g["n"] == 12 and cfg["eot"] not in g["tokens"] for g in greedy)
    for g, r in zip(greedy, beam):
        assert len(r["hyps"]) == 1 and r["best"] == 0
        assert r["tokens"][0] == g["tokens"] and r["n"][0] == g["n"]
        assert r["hyps"][0]["ended"] == (cfg["eot"] in g["tokens"])
        assert abs(r["hyps"][0]["sum_logprob"] - g["sum_logprob"]) <= 1e-9
        assert r["no_speech_prob"] == g["no_speech_prob"] and r["lang"] == g["lang"]


# ---- a search small enough to do by hand --------------------------------------------------------------------------------------
# 12 ids: text 0..5, EOT 6, SOT 7, <|nospeech|> 8, <|notimestamps|> 9, timestamps 10 and 11.
TINY = {"vocab": 12, "eot": 6, "sot": 7, "no_speech": 8, "no_timestamps": 9, "timestamp_begin": 10, "suppress": [7, 8],
        "begin_suppress": [], "max_initial_timestamp_index": None, "lang_ids": []}


def _logits(probs: dict) -> np.ndarray:
    z = np.full(TINY["vocab"], -np.inf)
    for t, p in probs.items():
        z[t] = math.log(p)
    return z


def _script(steps):
    """steps[i]: {history as a tuple: {id: probability}}; the probabilities of a slot sum to 1, so lp = log p."""
    def step_logits(i, slots):
        return np.stack([_logits(steps[i].get(tuple(s["tokens"]), {0: 1.0})) for s in slots])
    return step_logits


STEP0 = {(): {10: 0.6, 11: 0.4}}                                       # first position: timestamps only (rule 4)
STEP1 = {(10,): {6: 0.5, 0: 0.3, 1: 0.2}, (11,): {2: 0.9, 6: 0.1}}
# step 1, sorted: .36 (slot 1, id 2) live; .30 (slot 0, EOT) finishes mid-list; .18 (slot 0, id 0) live -> full, stop.
#   .12 (slot 0, id 1) and .04 (slot 1, EOT) are never walked.  Next slots: [11, 2] from slot 1, [10, 0] from slot 0.


def test_hand_computed_search_reaches_c_and_ranks_by_normalised_score():
    steps = [STEP0, STEP1, {(11, 2): {6: 0.6, 3: 0.4}, (10, 0): {4: 0.7, 11: 0.2, 6: 0.1}}]
    r = wb.search_logits(_script(steps), TINY, 3, 2)
    s0, s1, s2 = r["steps"]
    assert [(j, t) for j, t, _ in s0["live"]] == [(0, 10), (0, 11)] and not s0["finished"]
    assert [(j, t) for j, t, _ in s1["live"]] == [(1, 2), (0, 0)]
    assert [j for j, _ in s1["finished"]] == [0] and s1["fin_count"] == 1 and not s1["complete"]
    np.testing.assert_allclose([sc for _, _, sc in s1["live"]], [math.log(0.36), math.log(0.18)], atol=1e-12)
    # gaps of the walked part and the first unwalked candidate: log .36/.30, log .30/.18, log .18/.12; the first is the smallest
    assert s1["margin"] == pytest.approx(math.log(0.36) - math.log(0.30))
    # step 2: .216 (slot 0, EOT) finishes: the list has C = 2 entries -> complete; .144 and .126 still fill the slots
    assert [j for j, _ in s2["finished"]] == [0] and s2["fin_count"] == 2 and s2["complete"]
    assert [(j, t) for j, t, _ in s2["live"]] == [(0, 3), (1, 4)]
    assert [(h["tokens"], h["ended"]) for h in r["hyps"]] == [([10], True), ([11, 2], True)]
    np.testing.assert_allclose([h["sum_logprob"] for h in r["hyps"]], [math.log(0.30), math.log(0.216)], atol=1e-12)
    assert r["best"] == 1                      # log(.216) / 2 = -0.77 beats log(.30) / 1 = -1.20 although its sum is lower


def test_hand_computed_search_fills_up_with_live_slots_at_max_new():
    steps = [STEP0, STEP1, {(11, 2): {3: 0.6, 5: 0.4}, (10, 0): {4: 0.7, 11: 0.2, 6: 0.1}}]
    r = wb.search_logits(_script(steps), TINY, 3, 2)
    assert [(j, t) for j, t, _ in r["steps"][2]["live"]] == [(0, 3), (0, 5)] and not r["steps"][2]["complete"]
    # one finished hypothesis < W = 2: the first live slot follows, its sum as it is (no EOT log-probability)
    assert [(h["tokens"], h["ended"]) for h in r["hyps"]] == [([10], True), ([11, 2, 3], False)]
    assert r["hyps"][1]["sum_logprob"] == pytest.approx(math.log(0.216))
    assert r["best"] == 1
    # nothing is appended once the list has C entries: with C = 1 the EOT of step 2 is walked but not recorded
    steps[2] = {(11, 2): {6: 0.6, 3: 0.4}, (10, 0): {4: 0.7, 6: 0.3}}
    r = wb.search_logits(_script(steps), TINY, 3, 2, patience=0.5)
    assert len(r["steps"]) == 2 and r["steps"][1]["complete"]      # C = 1 was reached at step 1
    assert [(h["tokens"], h["ended"]) for h in r["hyps"]] == [([10], True), ([11, 2], False)]


def test_rule_7_and_dead_slots_in_one_step():
    z = np.stack([_logits({4: 0.3, 11: 0.7}), _logits({5: 1.0})])
    r = wb.beam_step(z, [[10, 0], [10, 1]], [-1.0, wb.NEG_INF], 0, TINY, 2, 2)
    # lse(timestamps) = log .7 > max text = log .3: text goes, the timestamp's log-probability is 0; the dead slot is silent
    assert r["live"] == [(0, 11, -1.0)] and not r["finished"] and not r["complete"]
    assert r["margin"] == pytest.approx(math.log(0.7) - math.log(0.3))
    r = wb.beam_step(z, [[10, 0], [10, 1]], [wb.NEG_INF, wb.NEG_INF], 0, TINY, 2, 2)
    assert r["live"] == [] and r["complete"]


def test_ranking_ties_go_to_the_earlier_hypothesis():
    hyps = [{"tokens": [1, 2], "sum_logprob": -2.0}, {"tokens": [3], "sum_logprob": -1.0}, {"tokens": [], "sum_logprob": -0.5}]
    assert wb.rank(hyps) == 2                  # max(1, 0) tokens: -0.5
    hyps[2]["sum_logprob"] = -1.0
    assert wb.rank(hyps) == 0


# ---- the GPU fixtures, on the oracle alone ----------------------------------------------------------------------------------
def test_supplied_logit_cases_have_margins_far_above_fp32_error(model):
    """The GPU test asks for the exact outcome of these steps; fp32 log-sum-exp error is below 1e-4, so every gap that
    is not a scripted tie has to be well above it.  Both rule-7 outcomes, EOT candidates and the C - 1 cut occur."""
    for cfg in (wo.model_a_config(), wo.model_b_config()):
        for W in (3, 5):
            case = cases.select_case(cfg, W)
            refs = cases.select_reference(case, cfg)
            assert all(r["margin"] > 1e-2 for r in refs), [r["margin"] for r in refs]
            assert len(refs[0]["finished"]) >= 1 and len(refs[1]["walked_eot"]) >= 2 and len(refs[1]["finished"]) == 1
            assert refs[1]["complete"] and not refs[0]["complete"]
            assert all(len(r["live"]) == W for r in refs)
            assert any(s != j for r in refs for j, (s, _, _) in enumerate(r["live"]))
    cfg = wo.model_a_config()
    tb = cfg["timestamp_begin"]
    for W in (3, 5):
        case = cases.tie_case(cfg, W)
        (r,) = cases.select_reference(case, cfg)
        live = [(s, t) for s, t, _ in r["live"]]
        assert live[0][0] == 0 and live[1] == (1, live[0][1])      # equal scores in slots 0 and 1: the lower slot first
        assert live[2:] == [(2, 20), (2, 63), (2, 64)][:W - 2]     # equal values in slot 2: the lower id first
        assert r["margin"] == 0.0 and tb > 700


def _parity_results(model):
    cfg, o16, o32 = model
    out = {}
    for name, (W, seeds) in cases.PARITY_CASES.items():
        mel = cases.mel_of(cfg, seeds)
        enc16, enc32 = o16.encode(mel), o32.encode(mel)
        res = wb.beam_search(o16, enc16, cases.prompt_of(cfg), cases.NEW_TOKENS, W)
        compared = []
        for b, r in enumerate(res):
            n = 0
            for st in r["steps"]:
                live = cases.live_slots(st)
                ids = [cases.prompt_of(cfg) + st["slots"][j]["tokens"] for j in live]
                l32 = o32.forced_logits(enc32[b:b + 1].repeat(len(live), 1, 1), ids).double().numpy()[:, -1]
                drift = max(np.abs(l32[k] - st["logits"][j]).max() for k, j in enumerate(live))
                if not st["margin"] > 4 * drift:
                    break
                n += 1
            compared.append(n)
        out[name] = (res, compared)
    return out


def test_parity_fixture_meets_its_conditions_on_the_oracle_alone(model):
    """Stand-in for the device's drift: the fp16 oracle against the fp32 oracle at the same position, which is about
    twice what the device shows against the fp16 oracle.  Under 4 x that drift the windows of the three parity cases give
    at least three windows with >= 8 compared steps, a compared step that forks, and a hypothesis finishing on EOT."""
    results = _parity_results(model)
    res = [r for rs, _ in results.values() for r in rs]
    compared = [n for _, ns in results.values() for n in ns]
    report = cases.fixture_report(res, compared)
    print({k: v[1] for k, v in results.items()}, report)
    assert report["windows_with_8"] >= 3 and report["forks"] >= 1 and report["finishes"] >= 1
    assert sum(n >= 8 for n in results["w5_b3"][1] + results["w5_b4"][1]) >= 3     # beam 5 alone has three such windows
    # the invariance test needs a window of the 20-lane case that completes early and one that runs to the last step
    steps = [len(r["steps"]) for r in results["w5_b4"][0]]
    assert min(steps) < cases.NEW_TOKENS - 8 and max(steps) == cases.NEW_TOKENS


# ---- the public interface -----------------------------------------------------------------------------------------------------
class _Scripted(transcribe.WhisperTranscriber):
    def __init__(self):
        self.dims = {"max_source_positions": 1500, "max_target_positions": 448, "sot": 901, "eot": 900, "transcribe": 950,
                     "timestamp_begin": 1000, "lang_ids": [910], "lang_codes": ["en"], "no_speech": 960}
        self.decoder, self.window_frames, self.sync_every, self.calls = transcribe.ByteDecoder({"Ġa": 5, "Ġb": 6}), 3000, 8, []

    def set_audio(self, samples):
        pass

    def logmel(self, offsets, fetch=True):
        self.calls.append(("logmel", len(offsets)))

    def encode(self, n, mel=None):
        pass

    def decode(self, prompt, n_windows, max_new_tokens, sync_every=None):
        raise AssertionError("beam_size > 1 must not take the greedy call")

    def decode_beam(self, prompt, n_windows, max_new_tokens, beam_size, patience=1.0, sync_every=None, trace=False):
        self.calls.append(("beam", n_windows, beam_size, patience))
        toks = np.full((n_windows, beam_size, max_new_tokens), 900, dtype=np.int32)
        toks[:, 0, :3] = [1000, 5, 1100]          # row 0: " a"
        toks[:, 1, :3] = [1000, 6, 1200]          # row 1: " b", the best
        return {"tokens": toks, "sum_logprob": np.tile(np.float32([-3.0, -1.0] + [-9.0] * (beam_size - 2)), (n_windows, 1)),
                "best": np.ones(n_windows, dtype=np.int32), "no_speech_prob": np.zeros(n_windows, dtype=np.float32)}


def test_transcribe_takes_the_best_hypothesis_and_splits_fixed_batches_to_64_lanes():
    t = _Scripted()
    out = t.transcribe(np.zeros(16000 * 30 * 20, dtype=np.float32), "en", window_mode="fixed", batch_windows=16, beam_size=5)
    assert [c for c in t.calls if c[0] == "beam"] == [("beam", 12, 5, 1.0), ("beam", 8, 5, 1.0)]     # 12 x 5 <= 64 lanes
    assert len(out["segments"]) == 20 and all(s["text"] == " b" and s["end_ms"] - s["start_ms"] == 4000 for s in out["segments"])
    with pytest.raises(ValueError):
        t.transcribe(np.zeros(16000, dtype=np.float32), "en", beam_size=9)
    with pytest.raises(ValueError):
        t.transcribe(np.zeros(16000, dtype=np.float32), "en", beam_size=5, patience=0.0)


class _Fake:
    def __init__(self):
        self.kw = None

    def transcribe(self, samples, language, **kw):
        self.kw = kw
        return {"language": "en", "segments": []}


def _video(config, fake):
    mm = ModelManager(cache_dir="/tmp", gpu_transcription=True, transcriber_factory=lambda cache, name: fake,
                      audio_source=lambda path: (np.zeros(1600, dtype=np.float32), 16000))
    return asyncio.run(mm.transcribe_video("v.mp4", config))


def test_transcribe_video_passes_beam_keys_only_when_the_config_sets_them(tmp_path):
    fake = _Fake()
    _video({}, fake)
    assert fake.kw == {"window_mode": "seek", "batch_windows": 8}
    _video({"beam_size": 5}, fake)
    assert fake.kw == {"window_mode": "seek", "batch_windows": 8, "beam_size": 5}
    _video({"beam_size": 3, "patience": 2}, fake)
    assert fake.kw == {"window_mode": "seek", "batch_windows": 8, "beam_size": 3, "patience": 2.0}
    for bad in ({"beam_size": 9}, {"beam_size": 0}, {"beam_size": 2.5}, {"patience": 0}, {"beam_size": 5, "patience": -1.0},
                {"beam_size": None}, {"beam_size": "5"}, {"beam_size": float("nan")}, {"patience": None}, {"patience": "1"}):
        with pytest.raises(ValueError):
            _video(bad, fake)
