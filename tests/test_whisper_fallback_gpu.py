"""K20c on the device: sampling at a temperature inside the selection path, the one-pass prompt prefill with causal
attention, the prompted greedy / sampled / beam decodes and the temperature fallback end to end, against
tests/whisper_fallback_oracle.py, tests/whisper_oracle.py and tests/whisper_beam_oracle.py.

Model A (d 128, 1003 ids, 64 positions) and model B (51865 ids, 448 positions) of tests/whisper_oracle.py.
"""
import asyncio

import numpy as np
import pytest

import whisper_beam_cases as cases
import whisper_beam_oracle as wb
import whisper_fallback_oracle as wf
import whisper_oracle as wo

pytestmark = pytest.mark.gpu

NEW = 24
BOOST = 1.2


class Model:
    def __init__(self, cfg, weights, audio_seeds, seconds):
        from eioku_amd.transcribe import WhisperTranscriber

        self.cfg, self.weights = cfg, weights
        self.o32, self.o16 = wo.Oracle(cfg, weights, fp16=False), wo.Oracle(cfg, weights, fp16=True)
        self.dev = WhisperTranscriber(dict(cfg), {k: v.numpy() for k, v in weights.items()})
        self.frames = 2 * cfg["max_source_positions"]
        self.base = [cfg["sot"], cfg["lang_ids"][0], cfg["transcribe"]]
        self.mel = np.stack([wo.log_mel(wf.audio(s, seconds), 0, self.frames, cfg["n_mels"]) for s in audio_seeds])
        self.enc32, self.enc16 = self.o32.encode(self.mel), self.o16.encode(self.mel)


def _boosted(cfg, seed):
    tb = cfg["timestamp_begin"]
    return wo.random_weights(cfg, seed, {cfg["eot"]: BOOST, **{tb + i: BOOST for i in range(cfg["vocab"] - tb)}})


@pytest.fixture(scope="module")
def model_a(gpu):
    cfg = wo.model_a_config()
    m = Model(cfg, _boosted(cfg, 5), (20, 28, 10, 42), 2.0)     # lanes 4..7 of tests/test_whisper_gpu.py's fixture
    yield m
    m.dev.close()


@pytest.fixture(scope="module")
def model_b(gpu):
    cfg = wo.model_b_config()
    m = Model(cfg, _boosted(cfg, 7), (11,), 30.0)
    yield m
    m.dev.close()


@pytest.fixture(scope="module")
def soft_model(gpu):
    """The beam fixture's model A (q / k projections at He scale), where the margin rule has beam steps to compare."""
    cfg, w = cases.model_a_weights()
    m = Model(cfg, w, cases.PARITY_CASES["w5_b3"][1], 2.0)
    yield m
    m.dev.close()


# ---- 1. sampling on supplied logits -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("temperature", [0.2, 1.0])
def test_sampling_on_supplied_logits(model_a, model_b, which, temperature):
    m = model_a if which == "a" else model_b
    cfg = m.cfg
    prefixes = list(wo.scripted_prefixes(cfg).values()) * 2
    logits = np.stack([wo.scripted_logits(cfg, 100 + i, -4.0 if i < len(prefixes) // 2 else 6.0) for i in range(len(prefixes))])
    logits[:, cfg["suppress"][2]] = 60.0                      # masked ids carry the largest logits of every row
    logits[:, cfg["no_timestamps"]] = 55.0
    seeds = [977 * (i + 1) + 13 for i in range(len(prefixes))]
    cases_n = near = 0
    worst_lp = 0.0
    for idx in range(8):
        tok, lp = m.dev.sample(logits, prefixes, temperature, seeds, [idx] * len(prefixes))
        for r, prefix in enumerate(prefixes):
            ref = wf.sample(logits[r], prefix, cfg, temperature, seeds[r], idx)
            cases_n += 1
            assert np.isfinite(ref["final"][tok[r]]), f"row {r} idx {idx}: masked id {tok[r]} was sampled"
            if ref["gap"] < ref["near"]:
                near += 1
                assert int(tok[r]) in ref["top2"]
            else:
                assert int(tok[r]) == ref["token"], f"row {r} idx {idx}: device {tok[r]}, oracle {ref['token']} (gap {ref['gap']:.3e})"
            err = abs(float(lp[r]) - float(ref["final"][tok[r]] - wo._lse(ref["final"])))
            worst_lp = max(worst_lp, err)
            assert err <= 1e-4
    print(f"model {which} T {temperature}: {cases_n} cases, {near} near-ties, worst log-probability error {worst_lp:.3e}")
    assert near <= 0.01 * cases_n


@pytest.mark.parametrize("seed", wf.TIE_SEEDS)
def test_equal_scores_go_to_the_lower_id(model_a, seed):
    cfg = model_a.cfg
    u = wf.uniforms(seed, 0, cfg["vocab"])
    assert u[63] == u[64]                                      # the same noise: equal logits are equal scores, bit for bit
    z = np.full((2, cfg["vocab"]), -5.0, dtype=np.float32)
    z[:, [64, 63]] = 30.0                                      # neighbours across a workgroup edge, far above the rest
    prefix = [cfg["timestamp_begin"] + 3, 10, 11]
    tok, _ = model_a.dev.sample(z, [prefix, prefix], 0.7, [seed, seed], [0, 0])
    assert tok.tolist() == [63, 63]
    z[0, 64] = 30.5                                            # and the larger score wins where they differ
    tok, _ = model_a.dev.sample(z, [prefix, prefix], 0.7, [seed, seed], [0, 0])
    assert tok.tolist() == [64, 63]


# ---- 2. the distribution --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temperature", [1.0, 0.5])
def test_sampled_tokens_follow_the_tempered_softmax(model_a, temperature):
    """4096 draws (64 lanes x 64 sample indices) over four ids with p = softmax(l / T) = .4, .3, .2, .1 and every other id
    30 below: each count within 5 standard deviations of N p.  A temperature that is ignored gives p ~ sqrt(p) at T = 0.5."""
    cfg = model_a.cfg
    ids, p = [20, 333, 700, 64], np.array([0.4, 0.3, 0.2, 0.1])
    row = np.full(cfg["vocab"], 0.0, dtype=np.float32)
    row[ids] = (temperature * np.log(p)).astype(np.float32)
    row[[i for i in range(cfg["vocab"]) if i not in ids]] = row[ids].min() - 30.0
    logits = np.tile(row, (64, 1))
    prefix = [cfg["timestamp_begin"] + 3, 10, 11]
    seeds = [50021 * (i + 1) for i in range(64)]
    counts = {i: 0 for i in ids}
    for idx in range(64):
        tok, _ = model_a.dev.sample(logits, [prefix] * 64, temperature, seeds, [idx] * 64)
        for t in tok.tolist():
            assert t in counts, f"id {t} has probability e^-30"
            counts[t] += 1
    N = 64 * 64
    print(f"T {temperature}: counts {counts}, expected {(N * p).tolist()}")
    for i, pi in zip(ids, p):
        assert abs(counts[i] - N * pi) <= 5 * np.sqrt(N * pi * (1 - pi)), (i, counts[i], N * pi)


# ---- 3. prefill logits ---------------------------------------------------------------------------------------------------------
def _drift(x, ref32):
    ref = np.asarray(ref32, dtype=np.float64)
    e = np.abs(np.asarray(x, dtype=np.float64) - ref) / np.sqrt(np.mean(ref ** 2))
    return float(e.mean()), float(e.max())


def _check_drift(name, got, ref32, ref16):
    """The bar of tests/test_whisper_gpu.py: 2 x the CPU fp16 oracle's drift against the fp32 oracle."""
    bar_mean, bar_max = (2 * v for v in _drift(ref16, ref32))
    mean, mx = _drift(got, ref32)
    print(f"{name}: device drift mean {mean:.3e} max {mx:.3e} of the rms; bar (2 x CPU fp16 drift) mean {bar_mean:.3e} max {bar_max:.3e}")
    assert mean <= bar_mean and mx <= bar_max


def _ids(m: Model, B: int, T: int) -> np.ndarray:
    rng = np.random.default_rng(1000 + T)
    ids = rng.integers(0, m.cfg["vocab"], size=(B, T))
    ids[:, :min(T, 3)] = m.base[:min(T, 3)]
    return ids.astype(np.int32)


@pytest.mark.parametrize("T", [1, 5, 17, 33, 40])
def test_prefill_logits_model_a(model_a, T):
    m = model_a
    ids = _ids(m, 3, T)
    m.dev.encode(3, m.mel[:3])
    got3 = m.dev.prefill_logits(ids)
    _check_drift(f"A prefill T {T} B 3", got3, m.o32.forced_logits(m.enc32[:3], ids).numpy(), m.o16.forced_logits(m.enc16[:3], ids).numpy())
    for lane in range(3):                                      # B = 1 and B = 3 give the same bits per lane
        m.dev.encode(1, m.mel[lane:lane + 1])
        got1 = m.dev.prefill_logits(ids[lane:lane + 1])
        assert np.array_equal(got1[0].view(np.uint32), got3[lane].view(np.uint32)), f"lane {lane}"
        if lane == 0:
            _check_drift(f"A prefill T {T} B 1", got1, m.o32.forced_logits(m.enc32[:1], ids[:1]).numpy(),
                         m.o16.forced_logits(m.enc16[:1], ids[:1]).numpy())


def test_prefill_logits_model_b(model_b):
    m = model_b
    ids = _ids(m, 1, 227)
    m.dev.encode(1, m.mel[:1])
    _check_drift("B prefill T 227", m.dev.prefill_logits(ids), m.o32.forced_logits(m.enc32[:1], ids).numpy(),
                 m.o16.forced_logits(m.enc16[:1], ids).numpy())


@pytest.mark.parametrize("P", [5, 33])
def test_a_decoder_step_runs_on_the_keys_and_values_the_prefill_left(model_a, P):
    m = model_a
    ids = _ids(m, 3, P + 1)
    m.dev.encode(3, m.mel[:3])
    got = m.dev.prefill_logits(ids, n_prefill=P)[:, P]         # position P is one decoder step over the prefill's cache
    _check_drift(f"A step after a prefill of {P}", got, m.o32.forced_logits(m.enc32[:3], ids).numpy()[:, P],
                 m.o16.forced_logits(m.enc16[:3], ids).numpy()[:, P])


# ---- 4. greedy with a long prompt ------------------------------------------------------------------------------------------------
def test_greedy_with_a_previous_text_prompt(model_a):
    m = model_a
    prompt, sot_index = wf.previous_text_prompt(m.cfg, 16)
    assert len(prompt) == 20 and prompt[sot_index] == m.cfg["sot"]
    B = len(m.mel)
    greedy = m.o16.greedy(m.enc16, prompt, NEW)
    drift = wf.position_drift(m.dev, m.o16, m.mel, m.enc16, np.array([prompt + g["tokens"][:-1] for g in greedy]))
    m.dev.encode(B, m.mel)
    res = m.dev.decode_prompted([prompt] * B, sot_index, NEW)
    assert res["tokens"].shape == (B, 1, NEW) and np.all(res["best"] == 0)
    compared = []
    for b, g in enumerate(greedy):
        n, stop = wf.compare_greedy(m.cfg, res["tokens"][b, 0], g, lambda i: drift[b][len(prompt) - 1 + i])
        compared.append(n)
        if stop is None:
            assert int(res["n"][b, 0]) == g["n"]
            assert abs(float(res["sum_logprob"][b, 0]) - g["sum_logprob"]) <= sum(drift[b][len(prompt) - 1 + i] for i in range(g["n"]))
            assert np.all(res["tokens"][b, 0, g["n"]:] == m.cfg["eot"])
        ref = wf.no_speech_at(m.o16, m.enc16[b:b + 1], prompt, sot_index)
        assert abs(float(res["no_speech_prob"][b]) - ref) <= drift[b][sot_index]
    print(f"20-token prompt: compared steps per lane {compared} of {[g['n'] for g in greedy]}")
    assert sum(compared) >= 8, "the fixture is too thin: fewer than 8 compared steps"


def test_the_plain_prompt_gives_the_tokens_of_decode(model_a):
    m = model_a
    B = len(m.mel)
    greedy = m.o16.greedy(m.enc16, m.base, NEW)
    drift = wf.position_drift(m.dev, m.o16, m.mel, m.enc16, np.array([m.base + g["tokens"][:-1] for g in greedy]))
    m.dev.encode(B, m.mel)
    old = m.dev.decode(m.base, B, NEW)
    new = m.dev.decode_prompted([m.base] * B, 0, NEW)
    compared = 0
    for b, g in enumerate(greedy):
        for i in range(g["n"]):
            if not g["margins"][i] > 4 * drift[b][len(m.base) - 1 + i]:
                break
            assert int(new["tokens"][b, 0, i]) == int(old["tokens"][b, i]) == g["tokens"][i], f"lane {b} step {i}"
            compared += 1
        assert abs(float(new["no_speech_prob"][b]) - float(old["no_speech_prob"][b])) <= 2 * drift[b][0]
    print(f"plain prompt: {compared} steps equal in decode, decode_prompted and the oracle")
    assert compared >= 8


# ---- 5. rows, windows, groups -----------------------------------------------------------------------------------------------------
def _best_of(res, b, eot):
    n, total = res["n"][b], res["sum_logprob"][b].astype(np.float64)
    ended = np.array([eot in row[:k] for row, k in zip(res["tokens"][b].tolist(), n)])
    return int(np.argmax(total / np.maximum(1, n - ended)))


def test_a_sampled_row_alone_equals_the_row_in_a_batch(model_a):
    m = model_a
    prompt, sot_index = wf.previous_text_prompt(m.cfg, 9)
    seeds = np.array([[1000 * b + g + 1 for g in range(3)] for b in range(4)], dtype=np.uint64)
    m.dev.encode(4, m.mel)
    batch = m.dev.decode_prompted([prompt] * 4, sot_index, NEW, group=3, temperature=0.8, seeds=seeds, sync_every=8)
    other = m.dev.decode_prompted([prompt] * 4, sot_index, NEW, group=3, temperature=0.8, seeds=seeds, sync_every=3)
    for key in ("tokens", "n", "sum_logprob", "best", "no_speech_prob"):
        assert batch[key].tobytes() == other[key].tobytes(), key
    n = batch["n"]
    print(f"sampled rows end after {n.tolist()} tokens")
    assert n.min() < NEW - 8 and n.max() > n.min() + 3, "no row ends early next to one that runs on: pick other seeds"
    for b in range(4):
        for g in range(3):
            row, k = batch["tokens"][b, g], int(n[b, g])
            assert np.all(row[k:] == m.cfg["eot"]) and m.cfg["eot"] not in row[:k - 1].tolist()     # a finished row keeps emitting EOT
        assert int(batch["best"][b]) == _best_of(batch, b, m.cfg["eot"])
    assert len({tuple(batch["tokens"][0, g].tolist()) for g in range(3)}) > 1                      # the rows of a window differ
    for b in range(4):
        m.dev.encode(1, m.mel[b:b + 1])
        for g in range(3):
            alone = m.dev.decode_prompted([prompt], sot_index, NEW, group=1, temperature=0.8, seeds=seeds[b:b + 1, g:g + 1])
            assert np.array_equal(alone["tokens"][0, 0], batch["tokens"][b, g]), (b, g)
            assert alone["n"][0, 0] == batch["n"][b, g]
            assert alone["sum_logprob"][0, 0].tobytes() == batch["sum_logprob"][b, g].tobytes()
        assert alone["no_speech_prob"][0].tobytes() == batch["no_speech_prob"][b].tobytes()


def test_the_window_list_picks_encoded_windows(model_a):
    m = model_a
    prompt, sot_index = wf.previous_text_prompt(m.cfg, 9)
    m.dev.encode(3, m.mel[:3])
    seeds = np.array([[7, 8], [9, 10], [11, 12]], dtype=np.uint64)
    for kw, pick in (({}, {}), ({"group": 2, "temperature": 0.6}, {"seeds": seeds})):
        full = m.dev.decode_prompted([prompt] * 3, sot_index, NEW, **kw, **pick)
        part = m.dev.decode_prompted([prompt] * 2, sot_index, NEW, windows=[2, 0], **kw,
                                     **({"seeds": seeds[[2, 0]]} if pick else {}))
        for key in ("tokens", "n", "sum_logprob", "best", "no_speech_prob"):
            assert part[key].tobytes() == full[key][[2, 0]].tobytes(), key
    assert not np.array_equal(full["tokens"][2], full["tokens"][0])
    with pytest.raises(RuntimeError, match="outside the 3 encoded windows"):
        m.dev.decode_prompted([prompt], sot_index, NEW, windows=[3])
    with pytest.raises(RuntimeError, match="64 lanes"):
        m.dev.decode_prompted([prompt] * 3, sot_index, NEW, group=22, temperature=0.5, seeds=np.zeros((3, 22), dtype=np.uint64))
    with pytest.raises(RuntimeError, match="max_target_positions"):
        m.dev.decode_prompted([prompt] * 3, sot_index, 64 - len(prompt) + 1)
    with pytest.raises(RuntimeError, match="greedy rule"):
        m.dev.decode_prompted([prompt] * 3, sot_index, NEW, group=2)


# ---- 6. beam search with a prompt ---------------------------------------------------------------------------------------------------
def test_beam_search_with_a_previous_text_prompt(soft_model):
    """The comparison of tests/test_whisper_beam_gpu.py's free-running parity test, driven from a 20-token prompt: every next
    slot's (source, token) equals the oracle's while the oracle's margin exceeds 4 x the step's logit drift."""
    m, W = soft_model, 5
    prompt, sot_index = wf.previous_text_prompt(m.cfg, 16)
    B, P, eot = len(m.mel), len(prompt), m.cfg["eot"]
    results = wb.beam_search(m.o16, m.enc16, prompt, NEW, W)
    m.dev.encode(B * W, np.repeat(m.mel, W, axis=0))
    drifts = [[] for _ in range(B)]
    for i in range(max(len(r["steps"]) for r in results)):
        ids = np.full((B * W, P + i), eot, dtype=np.int32)
        ids[:, :P] = prompt
        for b, r in enumerate(results):
            if i < len(r["steps"]):
                for j in cases.live_slots(r["steps"][i]):
                    ids[b * W + j, P:] = r["steps"][i]["slots"][j]["tokens"]
        logits = m.dev.forced_logits(ids)[:, -1]
        for b, r in enumerate(results):
            if i < len(r["steps"]):
                st = r["steps"][i]
                drifts[b].append(max(float(np.abs(logits[b * W + j] - st["logits"][j]).max()) for j in cases.live_slots(st)))
    m.dev.encode(B, m.mel)
    got = m.dev.decode_beam_prompted([prompt] * B, sot_index, NEW, W, trace=True)
    compared = []
    for b, r in enumerate(results):
        n = 0
        for i, st in enumerate(r["steps"]):
            if not st["margin"] > 4 * drifts[b][i]:
                break
            want = [(s, t) for s, t, _ in st["live"]] + [(-1, -1)] * (W - len(st["live"]))
            have = [(s, t) if s >= 0 else (-1, -1) for s, t in zip(got["trace_src"][i, b].tolist(), got["trace_tok"][i, b].tolist())]
            assert have == want, f"window {b} step {i}: device {have}, oracle {want} (margin {st['margin']:.4f}, drift {drifts[b][i]:.4f})"
            n += 1
        compared.append(n)
        if n == len(r["steps"]):
            nh = len(r["hyps"])
            assert int(got["n_hyp"][b]) == nh and got["tokens"][b, :nh].tolist() == r["tokens"] and got["n"][b, :nh].tolist() == r["n"]
        ref = wf.no_speech_at(m.o16, m.enc16[b:b + 1], prompt, sot_index)
        assert abs(float(got["no_speech_prob"][b]) - ref) <= 2 * max(drifts[b])
    report = cases.fixture_report(results, compared)
    print(f"beam 5 with a 20-token prompt: compared steps per window {compared} of {[len(r['steps']) for r in results]}; {report}")
    assert sum(compared) >= 8 and report["forks"] >= 1, "the fixture is too thin"
    # the windows of a batch equal the same windows alone, picked through the window list
    m.dev.encode(B, m.mel)
    part = m.dev.decode_beam_prompted([prompt] * 2, sot_index, NEW, W, windows=[2, 0])
    for key in ("tokens", "n", "ended", "sum_logprob", "n_hyp", "best", "no_speech_prob"):
        assert part[key].tobytes() == got[key][[2, 0]].tobytes(), key


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------------
def test_transcribe_video_with_the_reference_call(model_a, tmp_path):
    from eioku_amd import transcribe
    from eioku_amd.model_manager import ModelManager

    m = model_a
    wf.write_checkpoint(tmp_path / "whisper" / "tiny-test", m.cfg, m.weights)
    audio = wf.audio(20, 6.0)                                   # three 2 s windows
    log, raws = [], []

    def factory(cache, name):
        t = transcribe.WhisperTranscriber.from_cache(cache, name)
        for method in ("decode_prompted", "decode_beam_prompted"):
            def spy(prompts, sot_index, max_new, *a, _f=getattr(t, method), _m=method, **kw):
                res = _f(prompts, sot_index, max_new, *a, **kw)
                row = [int(x) for x in res["tokens"][0][int(res["best"][0])]]
                text = t.decoder.decode([x for x in row[:row.index(m.cfg["eot"]) if m.cfg["eot"] in row else len(row)] if x < m.cfg["eot"]])
                log.append({"method": _m, "prompts": [list(p) for p in prompts], "sot_index": sot_index, "res": res,
                            "temperature": kw.get("temperature", 0.0), "ratio": transcribe.compression_ratio(text)})
                return res
            setattr(t, method, spy)
        full = t.transcribe

        def keep(*a, **kw):
            raws.append(full(*a, **kw))
            return raws[-1]
        t.transcribe = keep
        return t

    def run(**extra):
        del log[:]
        mm = ModelManager(cache_dir=str(tmp_path), gpu_transcription=True, audio_source=lambda path: (audio, 16000),
                          transcriber_factory=factory)
        cfg = dict(transcribe.REFERENCE_CALL, model_name="tiny-test", languages=["en"], seed=3, **extra)
        return asyncio.run(mm.transcribe_video("clip.mp4", cfg)), raws[-1], list(log)

    out, raw, calls = run(log_prob_threshold=None, compression_ratio_threshold=None)
    assert list(out) == ["segments"] and len(out["segments"]) >= 2
    for seg in out["segments"]:
        assert set(seg) == {"start_ms", "end_ms", "text", "language", "confidence", "words"}
        assert 0 <= seg["start_ms"] < seg["end_ms"] <= 8000 and seg["language"] == "en" and seg["text"].startswith(" w")
    assert all(s["temperature"] == 0.0 for s in raw["segments"]) and all(c["method"] == "decode_beam_prompted" for c in calls)
    assert len(calls) >= 2 and calls[0]["prompts"] == [m.base] and calls[0]["sot_index"] == 0
    # the prompt of window 2 carries window 1's tokens behind <|startofprev|>
    first = calls[0]["res"]
    toks = transcribe.emitted_tokens(first["tokens"][0][int(first["best"][0])], m.cfg["eot"], m.cfg["timestamp_begin"])
    assert len(toks) >= 2
    assert calls[1]["prompts"] == [[m.cfg["no_speech"] - 1] + toks[-31:] + m.base] and calls[1]["sot_index"] == 1 + len(toks[-31:])
    # a threshold just above window 1's T = 0 average forces the fallback on it
    a0 = raw["windows"][0]["avg_logprob"]
    assert raw["windows"][0]["start_frame"] == 0 and len(raw["windows"]) >= 3
    out2, raw2, calls2 = run(log_prob_threshold=a0 + 1e-3, compression_ratio_threshold=None)
    assert calls2[0]["method"] == "decode_beam_prompted" and calls2[1]["method"] == "decode_prompted"
    assert calls2[1]["temperature"] == 0.2 and calls2[1]["res"]["tokens"].shape[1] == 5 and calls2[1]["prompts"] == [m.base]

    def window_1_tries(calls):                                  # everything before window 2's T = 0 call
        tries = []
        for c in calls:
            if c["temperature"] == 0.0 and tries:
                break
            row = int(c["res"]["best"][0])
            t = [int(x) for x in c["res"]["tokens"][0][row]]
            n_text = t.index(m.cfg["eot"]) if m.cfg["eot"] in t else len(t)
            tries.append((c["temperature"], float(c["res"]["sum_logprob"][0][row]) / (n_text + 1), c["ratio"]))
        return tries

    tries = [(t, avg) for t, avg, _ in window_1_tries(calls2)]
    passed = [t for t, avg in tries if avg >= a0 + 1e-3]
    want = passed[0] if passed else max(tries, key=lambda x: x[1])[0]
    print(f"window 1 tries (temperature, average log-probability): {tries}; accepted at {want}")
    assert tries[0][1] == pytest.approx(a0) and len(tries) >= 2
    assert raw2["windows"][0]["temperature"] == pytest.approx(want)
    assert raw2["windows"][0]["avg_logprob"] == pytest.approx(dict(tries)[want])
    for seg in raw2["segments"]:
        assert set(seg) >= {"temperature", "avg_logprob", "compression_ratio", "tokens"}
        assert (seg["temperature"], seg["avg_logprob"]) in {(w["temperature"], w["avg_logprob"]) for w in raw2["windows"]}
    assert all(set(seg) == {"start_ms", "end_ms", "text", "language", "confidence", "words"} for seg in out2["segments"])
    # a schedule that starts above the reset temperature: every window is accepted at 0.6 and none hands tokens on
    _, raw3, calls3 = run(temperature=[0.6, 0.2], log_prob_threshold=None, compression_ratio_threshold=None)
    assert all(w["temperature"] == 0.6 for w in raw3["windows"]) and all(c["prompts"] == [m.base] for c in calls3)
    assert all(c["method"] == "decode_prompted" and c["res"]["tokens"].shape[1] == 5 for c in calls3)
    # with a threshold just above window 1's average at 0.6 it is sampled again at 0.2, accepted there when that average
    # reaches the threshold, and hands its tokens on because 0.2 is below the reset temperature
    a6 = raw3["windows"][0]["avg_logprob"]
    _, raw4, calls4 = run(temperature=[0.6, 0.2], log_prob_threshold=a6 + 1e-3, compression_ratio_threshold=None)
    tries4 = window_1_tries(calls4[:2])
    print(f"window 1 tries from 0.6 (temperature, average log-probability, compression ratio): {tries4}")
    assert [t for t, _, _ in tries4] == [0.6, 0.2] and tries4[0][1] == pytest.approx(a6)
    assert tries4[1][1] >= a6 + 1e-3, "sampling at 0.2 does not beat sampling at 0.6 on this window: pick another seed"
    assert raw4["windows"][0]["temperature"] == 0.2 and raw4["windows"][0]["avg_logprob"] == pytest.approx(tries4[1][1])
    res = calls4[1]["res"]
    toks = transcribe.emitted_tokens(res["tokens"][0][int(res["best"][0])], m.cfg["eot"], m.cfg["timestamp_begin"])
    assert calls4[2]["temperature"] == 0.6 and calls4[2]["prompts"] == [[m.cfg["no_speech"] - 1] + toks[-31:] + m.base]
