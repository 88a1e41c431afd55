"""K19 / K20 on the device against tests/whisper_oracle.py (the CPU oracle; transformers is not needed here).

Model A: d 128, 2 heads, 2 + 2 layers, ffn 512, ctx 100 (a tile tail), 1003 ids with its own special-id layout (a
vocabulary tail).  Model B: the same widths with the real layout, 51865 ids and ctx 1500 (the real tails and strides).

Measured on an MI355X (printed by the tests, copied into DESIGN.md "K19 / K20"): see the table there.
"""
import asyncio

import numpy as np
import pytest
import torch

import whisper_oracle as wo
from whisper_testlib import write_checkpoint as _write_checkpoint

pytestmark = pytest.mark.gpu

NEW_TOKENS = 24
BOOST = 1.2  # EOT and timestamp rows raised along the final LayerNorm's bias: lanes end at different steps


def _audio(seed: int, seconds: float) -> np.ndarray:
    rng = np.random.default_rng(seed)
    t = np.arange(int(seconds * 16000)) / 16000.0
    x = sum(rng.uniform(0.05, 0.3) * np.sin(2 * np.pi * rng.uniform(80, 4000) * t + rng.uniform(0, 6)) for _ in range(6))
    return (x + 0.01 * rng.standard_normal(len(t))).astype(np.float32)


def _dims(cfg: dict) -> dict:
    return dict(cfg)  # the oracle's config carries every key WhisperTranscriber reads


class Model:
    """One test model: the device transcriber, both oracles, and the oracle's greedy decode of the fixture audio."""

    def __init__(self, cfg, seed, audio_seeds, seconds, new_tokens=NEW_TOKENS, qk_scale=4.0):
        from eioku_amd.transcribe import WhisperTranscriber

        self.cfg, self.new_tokens = cfg, new_tokens
        tb = cfg["timestamp_begin"]
        boost = {cfg["eot"]: BOOST, **{tb + i: BOOST for i in range(cfg["vocab"] - tb)}}
        self.weights = wo.random_weights(cfg, seed, boost, qk_scale)
        self.o32 = wo.Oracle(cfg, self.weights, fp16=False)
        self.o16 = wo.Oracle(cfg, self.weights, fp16=True)
        self.dev = WhisperTranscriber(_dims(cfg), {k: v.numpy() for k, v in self.weights.items()})
        self.frames = 2 * cfg["max_source_positions"]
        self.prompt = [cfg["sot"], cfg["lang_ids"][0], cfg["transcribe"]]
        self.audios = [_audio(s, seconds) for s in audio_seeds]
        self.mel = np.stack([wo.log_mel(a, 0, self.frames, cfg["n_mels"]) for a in self.audios])
        self.enc32 = self.o32.encode(self.mel)
        self.enc16 = self.o16.encode(self.mel)
        self.greedy16 = self.o16.greedy(self.enc16, self.prompt, new_tokens)
        self._drift = None

    def position_drift(self) -> np.ndarray:
        """[lane][position]: max over the vocabulary of |device - fp16 oracle| on the teacher-forced logits of the oracle's own
        greedy sequence (prompt positions included).  While the device has sampled the oracle's tokens, its free-running
        logits at a step ARE these teacher-forced logits, so a margin above 2 x this drift cannot flip; the tests ask 4 x."""
        if self._drift is None:
            ids = np.array([self.prompt + g["tokens"][:-1] for g in self.greedy16])
            self.dev.encode(len(ids), self.mel)
            diff = np.abs(self.dev.forced_logits(ids) - self.o16.forced_logits(self.enc16, ids).numpy())
            self._drift = diff.max(axis=2).astype(np.float64)
            print(f"teacher-forced logit drift device vs fp16 oracle: mean {diff.mean():.3e}, per-position max: median "
                  f"{np.median(self._drift):.3e}, largest {self._drift.max():.3e}")
        return self._drift

    def step_drift(self, lane: int, step: int) -> float:
        return float(self.position_drift()[lane][len(self.prompt) - 1 + step])


@pytest.fixture(scope="module")
def model_a(gpu):
    m = Model(wo.model_a_config(), seed=5, audio_seeds=(3, 5, 6, 8, 20, 28, 10, 42, 43), seconds=2.0)
    yield m
    m.dev.close()


@pytest.fixture(scope="module")
def model_b(gpu):
    m = Model(wo.model_b_config(), seed=7, audio_seeds=(11, 12), seconds=30.0)
    yield m
    m.dev.close()


def _fixture_is_useful(m: Model):
    toks = [g["tokens"] for g in m.greedy16]
    for t in toks:
        assert len(set(t)) >= 8, "fewer than 8 distinct tokens in a window"
    for i in range(len(toks)):
        for j in range(i + 1, len(toks)):
            same = sum(a == b for a, b in zip(toks[i], toks[j]))
            assert same < m.new_tokens / 2, f"audios {i} and {j} agree in {same} positions"


def test_fixtures_decode_varied_audio_dependent_tokens(model_a, model_b):
    _fixture_is_useful(model_a)
    _fixture_is_useful(model_b)


# ---- K19 --------------------------------------------------------------------------------------------------------------------
def _assert_within_2_ulps(got, ref):
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / ulp
    print(f"log-mel: max {err.max():.2f} ulp, {np.count_nonzero(err)} of {err.size} elements differ")
    assert err.max() <= 2.0


@pytest.mark.parametrize("case", ["full", "short", "silence", "batch3"])
def test_log_mel_equals_the_float64_oracle(model_b, case):
    dev, frames, n = model_b.dev, model_b.frames, model_b.frames * 160
    if case == "full":
        audio, offsets = _audio(21, 31.0), [0]
    elif case == "short":
        audio, offsets = _audio(22, 7.3), [0]
    elif case == "silence":
        audio, offsets = np.zeros(16000 * 3, dtype=np.float32), [0]
    else:
        audio, offsets = _audio(23, 65.0), [0, n - 12345, 2 * n]
    dev.set_audio(audio)
    got = dev.logmel(offsets)
    ref = np.stack([wo.log_mel(audio, o, frames, 80) for o in offsets])
    assert got.shape == ref.shape == (len(offsets), 80, frames)
    _assert_within_2_ulps(got, ref)
    if case == "silence":
        assert np.all(got == np.float32(-1.5))  # log10(1e-10) = -10 everywhere: (-10 + 4) / 4


# ---- K20: encoder output and teacher-forced logits --------------------------------------------------------------------------
def _drift(x, ref32):
    """mean and max |x - ref| as fractions of the reference's RMS"""
    ref = np.asarray(ref32, dtype=np.float64)
    rms = np.sqrt(np.mean(ref ** 2))
    e = np.abs(np.asarray(x, dtype=np.float64) - ref) / rms
    return float(e.mean()), float(e.max())


def _check_drift(name, got, ref32, ref16):
    bar_mean, bar_max = (2 * v for v in _drift(ref16, ref32))
    mean, mx = _drift(got, ref32)
    print(f"{name}: device drift mean {mean:.3e} max {mx:.3e} of the rms; bar (2 x CPU fp16 drift) mean {bar_mean:.3e} max {bar_max:.3e}")
    assert mean <= bar_mean and mx <= bar_max


def _forced_ids(m: Model, n: int):
    return np.array([m.prompt + g["tokens"][:5] for g in m.greedy16[:n]])


def test_encoder_and_logits_drift_model_a(model_a):
    m = model_a
    ids = _forced_ids(m, 3)
    m.dev.encode(3, m.mel[:3])
    enc3 = m.dev.encoder_output(3)
    log3 = m.dev.forced_logits(ids)
    _check_drift("A encoder", enc3.astype(np.float32), m.enc32[:3].numpy(), m.enc16[:3].numpy())
    _check_drift("A logits", log3, m.o32.forced_logits(m.enc32[:3], ids).numpy(), m.o16.forced_logits(m.enc16[:3], ids).numpy())
    for lane in range(3):  # B = 1 and B = 3 give the same bits per lane
        m.dev.encode(1, m.mel[lane:lane + 1])
        assert np.array_equal(m.dev.encoder_output(1)[0].view(np.uint16), enc3[lane].view(np.uint16))
        assert np.array_equal(m.dev.forced_logits(ids[lane:lane + 1])[0].view(np.uint32), log3[lane].view(np.uint32))


def test_encoder_and_logits_drift_model_b(model_b):
    m = model_b
    ids = _forced_ids(m, 1)
    m.dev.encode(1, m.mel[:1])
    _check_drift("B encoder", m.dev.encoder_output(1).astype(np.float32), m.enc32[:1].numpy(), m.enc16[:1].numpy())
    _check_drift("B logits", m.dev.forced_logits(ids), m.o32.forced_logits(m.enc32[:1], ids).numpy(),
                 m.o16.forced_logits(m.enc16[:1], ids).numpy())


# ---- K20: rules and argmax on supplied logits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("shift", [-4.0, 6.0])
def test_rules_and_argmax_on_supplied_logits(model_a, model_b, which, shift):
    m = model_a if which == "a" else model_b
    cfg = m.cfg
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
        assert abs(lp[i] - rlp) <= 1e-4  # fp32 log-sum-exp over <= 51865 terms against float64


def test_argmax_ties_go_to_the_lower_id(model_a):
    cfg = model_a.cfg
    tb = cfg["timestamp_begin"]
    z = np.full((3, cfg["vocab"]), -5.0, dtype=np.float32)
    z[0, [700, 20, 333]] = 2.0                  # three equal text logits in different workgroups
    z[1, [tb + 60, tb + 30, tb + 45]] = 9.0     # equal timestamps, timestamp mass above any text id
    z[2, [64, 63]] = 1.0                        # neighbours across a workgroup edge
    tok, _, _ = model_a.dev.select(z, [[tb + 3, 10, 11], [tb + 3, 10, 11], [tb + 3, 10, 11]])
    assert tok.tolist() == [20, tb + 30, 63]


# ---- K20: greedy decode -------------------------------------------------------------------------------------------------------
def _compare_greedy(m: Model, res: dict, lanes):
    """The margin rule, with the drift taken per position (Model.position_drift): a lane's tokens equal the oracle's while
    every earlier oracle step had a margin above 4 x the logit drift of that step; at the first thinner step the device
    token must be one of the oracle's two best (or, where rule 7 is the thin decision, the best of either branch), and the
    lane stops.  Returns (compared steps, first thin step per lane)."""
    cfg = m.cfg
    tb = cfg["timestamp_begin"]
    compared, stops = 0, []
    for lane, fix in enumerate(lanes):
        g, stop, sampled = m.greedy16[fix], None, []
        for i in range(g["n"]):
            got, thr = int(res["tokens"][lane][i]), 4 * m.step_drift(fix, i)
            if g["margins"][i] > thr:
                assert got == g["tokens"][i], (f"lane {fix} step {i}: device {got}, oracle {g['tokens'][i]} "
                                               f"(margin {g['margins'][i]:.4f}, 4 x drift {thr:.4f})")
                compared += 1
                sampled.append(got)
                continue
            masked = wo.apply_rules(g["logits"][i], sampled, cfg)
            final = masked.copy()
            if wo.text_suppressed(masked, cfg):
                final[:tb] = -np.inf
            ok = set(np.argsort(final)[-2:].tolist())
            if abs(wo._lse(masked[tb:]) - masked[:tb].max()) <= thr:  # rule 7 itself is the thin decision
                ok |= {int(np.argmax(masked)), tb + int(np.argmax(masked[tb:]))}
            assert got in ok, f"lane {fix} step {i}: device {got} is not among the oracle's best {ok}"
            stop = i
            break
        stops.append(stop)
        if stop is None:  # the lane ran its whole length equal: sums and lengths are comparable too
            assert int(res["n"][lane]) == g["n"]
            bar = sum(m.step_drift(fix, i) for i in range(g["n"]))
            err = abs(float(res["sum_logprob"][lane]) - g["sum_logprob"])
            print(f"lane {fix}: sum of log-probabilities differs by {err:.3e}, bar (drift summed over {g['n']} steps) {bar:.3e}")
            assert err <= bar
            assert all(int(t) == cfg["eot"] for t in res["tokens"][lane][g["n"]:])
    return compared, stops


def _info_checks(m: Model, res: dict, lanes):
    for lane, fix in enumerate(lanes):
        g, drift = m.greedy16[fix], float(m.position_drift()[fix][0])
        assert abs(float(res["no_speech_prob"][lane]) - g["no_speech_prob"]) <= drift
        if g["lang_margin"] > 4 * drift:
            assert int(res["lang"][lane]) == g["lang"]
        else:
            assert int(res["lang"][lane]) in m.cfg["lang_ids"]


GREEDY_LANES_A = [4, 5, 6, 7, 8]  # the fixture's lanes whose first ten oracle steps all have margins above 0.1


def test_greedy_decode_model_a(model_a):
    m = model_a
    lanes = GREEDY_LANES_A
    m.position_drift()
    m.dev.encode(len(lanes), m.mel[lanes])
    res = m.dev.decode(m.prompt, len(lanes), NEW_TOKENS)
    compared, stops = _compare_greedy(m, res, lanes)
    print(f"model A: {compared} compared steps, thin-margin stops {stops}")
    assert all(s is None or s >= 8 for s in stops), "a lane stops before step 8: the fixture is too thin"
    assert compared >= 48
    _info_checks(m, res, lanes)


def test_greedy_decode_model_b(model_b):
    m = model_b
    m.position_drift()
    m.dev.encode(2, m.mel)
    res = m.dev.decode(m.prompt, 2, NEW_TOKENS)
    compared, stops = _compare_greedy(m, res, [0, 1])
    print(f"model B: {compared} compared steps, thin-margin stops {stops}")
    _info_checks(m, res, [0, 1])


def test_lanes_in_a_batch_equal_the_same_lanes_alone(model_a):
    """The fixture's lanes end at different steps (one on EOT early, one late, two run into max_new_tokens), and 24 steps
    cross the sync_every = 8 boundary twice.  Each lane alone, and the batch at another sync interval, give the same bits."""
    m = model_a
    ends = sorted(g["n"] for g in m.greedy16[:4])
    assert ends[0] < ends[1] < NEW_TOKENS and ends[-1] == NEW_TOKENS and m.cfg["eot"] not in m.greedy16[3]["tokens"]
    m.dev.encode(4, m.mel[:4])
    batch = m.dev.decode(m.prompt, 4, NEW_TOKENS, sync_every=8)
    other = m.dev.decode(m.prompt, 4, NEW_TOKENS, sync_every=3)
    for key in ("tokens", "n", "sum_logprob", "no_speech_prob", "lang"):
        assert np.array_equal(batch[key], other[key]), key
    for lane in range(4):
        m.dev.encode(1, m.mel[lane:lane + 1])
        alone = m.dev.decode(m.prompt, 1, NEW_TOKENS)
        assert np.array_equal(alone["tokens"][0], batch["tokens"][lane]), f"lane {lane}"
        assert alone["n"][0] == batch["n"][lane]
        assert alone["sum_logprob"][0].tobytes() == batch["sum_logprob"][lane].tobytes()
        assert alone["no_speech_prob"][0].tobytes() == batch["no_speech_prob"][lane].tobytes()
    early = int(np.argmin(batch["n"]))
    assert np.all(batch["tokens"][early][batch["n"][early]:] == m.cfg["eot"])  # a finished lane keeps emitting EOT


# ---- end to end ---------------------------------------------------------------------------------------------------------------
class _OracleTranscriber:
    """WhisperTranscriber's host loop over the CPU oracle instead of the device; ``log`` collects (mel, prompt, greedy
    result) of every decode."""

    def __new__(cls, m: Model, log: list):
        from eioku_amd.transcribe import ByteDecoder, WhisperTranscriber

        class T(WhisperTranscriber):
            def __init__(self):
                self.dims, self.decoder, self.window_frames, self.sync_every = _dims(m.cfg), ByteDecoder({}), m.frames, 8

            def set_audio(self, samples):
                self._samples = samples

            def logmel(self, offsets, fetch=True):
                self._mel = np.stack([wo.log_mel(self._samples, int(o), m.frames, m.cfg["n_mels"]) for o in offsets])

            def encode(self, n, mel=None):
                self._enc = m.o16.encode(self._mel)

            def decode(self, prompt, n_windows, max_new_tokens, sync_every=None):
                gs = m.o16.greedy(self._enc, list(prompt), max_new_tokens)
                log.append((self._mel, self._enc, list(prompt), gs))
                return {"tokens": np.array([g["tokens"] for g in gs]), "n": np.array([g["n"] for g in gs]),
                        "sum_logprob": np.array([g["sum_logprob"] for g in gs]), "lang": np.array([g["lang"] for g in gs]),
                        "no_speech_prob": np.array([g["no_speech_prob"] for g in gs])}

            def close(self):
                pass

        return T()


E2E_TOKENS = 10


@pytest.mark.parametrize("mode", ["seek", "fixed"])
def test_end_to_end_segments_equal_the_cutter_on_the_oracles_tokens(model_a, mode):
    """Two 2 s windows of model A through WhisperTranscriber.transcribe; in seek mode the first window's last pair lands
    mid-window.  Precondition (the margin rule): every oracle step of every window has a margin above 4 x the logit drift
    the device shows at that step, teacher-forced on the oracle's tokens."""
    m = model_a
    audio = _audio(20, 3.6)
    log: list = []
    want = _OracleTranscriber(m, log).transcribe(audio, "en", window_mode=mode, batch_windows=2, max_new_tokens=E2E_TOKENS)
    for mel, enc, prompt, gs in log:
        ids = np.array([prompt + g["tokens"][:-1] for g in gs])
        m.dev.encode(len(gs), mel)
        drift = np.abs(m.dev.forced_logits(ids) - m.o16.forced_logits(enc, ids).numpy()).max(axis=2)
        for lane, g in enumerate(gs):
            for i in range(g["n"]):
                assert g["margins"][i] > 4 * drift[lane][len(prompt) - 1 + i], "a step of this fixture is too thin to compare segments"
    got = m.dev.transcribe(audio, "en", window_mode=mode, batch_windows=2, max_new_tokens=E2E_TOKENS)
    assert len(want["segments"]) >= 2
    if mode == "seek":
        assert len(log) >= 2 and any(0 < s["end_ms"] < 2000 for s in want["segments"])
        assert want["segments"][-1]["start_ms"] > 2000
    assert got == want


# ---- smoke: the public entry point -----------------------------------------------------------------------------------------------
def test_smoke_transcribe_video_through_model_manager(model_a, tmp_path):
    from eioku_amd.model_manager import ModelManager

    m = model_a
    _write_checkpoint(tmp_path / "whisper" / "tiny-test", m.cfg, m.weights)
    audio = m.audios[0]
    mm = ModelManager(cache_dir=str(tmp_path), gpu_transcription=True, audio_source=lambda path: (audio, 16000))
    out = asyncio.run(mm.transcribe_video("clip.mp4", {"model_name": "tiny-test", "languages": ["en"]}))
    assert list(out) == ["segments"] and len(out["segments"]) >= 1
    for seg in out["segments"]:
        assert set(seg) == {"start_ms", "end_ms", "text", "language", "confidence", "words"}
        # seek mode: a window may start anywhere before the audio's end (2 s) and its timestamps reach 2 s further
        assert 0 <= seg["start_ms"] < seg["end_ms"] < 4000 and seg["language"] == "en" and seg["text"].startswith(" w")
    with pytest.raises(NotImplementedError):
        asyncio.run(ModelManager(cache_dir=str(tmp_path)).transcribe_video("clip.mp4", {}))
