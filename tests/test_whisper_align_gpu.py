"""K21 on the device: dynamic time warping, the cost kernel, the alignment pass end to end, the product path with
``word_timestamps`` and the rejections, against tests/whisper_align_oracle.py.  Model A of tests/whisper_oracle.py (d 128,
2 heads, ctx 100, 64 positions).

Measured on an MI355X (the bars below are 4 x these figures; every test prints its own before it asserts):
  cost kernel against the float64 oracle, largest absolute difference over the 12 cases      2.15e-7
  end-to-end cost against the fp16-mode oracle, the larger of the two head sets               sharp 3.33e-1, soft 8.22e-3
  end-to-end token probability against the fp16-mode oracle                                   sharp 9.7e-5,  soft 8.1e-6
The end-to-end figures are per model.  "sharp" is model A as tests/test_whisper_gpu.py builds it (q / k projections x 4):
its cross-attention scores reach tens, one fp16 ulp of q moves a probability by percents, and a cost cell - a z-score over
the token rows - moves by tenths, on the device and in the oracle alike.  "soft" is the beam fixture's model A (q / k at He
scale, tests/whisper_beam_cases.py), where the same comparison is tight and pins the attention-weights kernel.
"""
import numpy as np
import pytest

import whisper_align_oracle as wa
import whisper_beam_cases as cases
import whisper_fallback_oracle as wf
import whisper_oracle as wo

pytestmark = pytest.mark.gpu

COST_KERNEL_MEASURED = 2.2e-7
COST_E2E_MEASURED = {"sharp": 3.33e-1, "soft": 8.22e-3}
PROB_E2E_MEASURED = {"sharp": 9.7e-5, "soft": 8.1e-6}

BOOST = 1.2
SOT_LEN = 3


class Model:
    def __init__(self, kind: str = "sharp"):
        from eioku_amd.transcribe import WhisperTranscriber

        self.kind = kind
        cfg = self.cfg = wo.model_a_config()
        tb = cfg["timestamp_begin"]
        if kind == "sharp":
            self.weights = wo.random_weights(cfg, 5, {cfg["eot"]: BOOST, **{tb + i: BOOST for i in range(cfg["vocab"] - tb)}})
        else:
            self.weights = cases.model_a_weights()[1]
        self.o16 = wa.AlignOracle(cfg, self.weights, fp16=True)
        self.vocab = {f"Ġw{i}": i for i in range(cfg["eot"])}
        self.dev = WhisperTranscriber(dict(cfg), {k: v.numpy() for k, v in self.weights.items()}, self.vocab)
        self.base = [cfg["sot"], cfg["lang_ids"][0], cfg["transcribe"]]
        self.frames = 2 * cfg["max_source_positions"]
        # window 0: 2 s of audio (200 frames); window 1: 1.3 s (130 frames of content, the rest of the window is silence)
        self.n_frames = [200, 130]
        self.mel = np.stack([wo.log_mel(wf.audio(20, 2.0), 0, self.frames, cfg["n_mels"]),
                             wo.log_mel(wf.audio(28, 1.3), 0, self.frames, cfg["n_mels"])])
        self.enc16 = self.o16.encode(self.mel)
        rng = np.random.default_rng(77)
        self.text = [[int(t) for t in rng.integers(10, 290, size=n)] for n in (18, 4)]      # sequences of 23 and 9 tokens
        self.refs = {}

    def ref(self, row: int, heads):
        key = (row, tuple(heads) if heads else None)
        if key not in self.refs:
            self.refs[key] = self.o16.align(self.enc16[row:row + 1], self.base, self.text[row], self.n_frames[row], heads)
        return self.refs[key]


@pytest.fixture(scope="module")
def model(gpu):
    m = Model()
    yield m
    m.dev.close()


@pytest.fixture(scope="module")
def soft_model(gpu):
    m = Model("soft")
    yield m
    m.dev.close()


# ---- 1. DTW, exact ---------------------------------------------------------------------------------------------------------------
DTW_SHAPES = [(1, 1), (2, 7), (63, 100), (64, 2), (65, 100), (257, 1), (1, 1500), (257, 1500)]


def _dtw_cost(kind: str, n: int, f: int) -> np.ndarray:
    rng = np.random.default_rng(1000 * n + f)
    if kind == "random":
        return rng.standard_normal((n, f)).astype(np.float32)
    if kind == "zeros":
        return np.zeros((n, f), dtype=np.float32)
    return rng.integers(-1, 2, size=(n, f)).astype(np.float32)            # three levels: ties everywhere


@pytest.mark.parametrize("kind", ["random", "zeros", "levels"])
@pytest.mark.parametrize("shape", DTW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dtw_equals_the_oracle_bit_for_bit(model, shape, kind):
    cost = _dtw_cost(kind, *shape)
    got = model.dev.dtw(cost)
    ti, fi = wa.dtw(cost)
    assert got["text_idx"].tolist() == ti.tolist() and got["time_idx"].tolist() == fi.tolist()
    assert got["jump"].tolist() == wa.jumps(ti, fi, shape[0]).tolist()
    assert model.dev.last_launches()[0] == 1


# ---- 2. the cost kernel ------------------------------------------------------------------------------------------------------------
COST_CASES = [(H, T, F) for H in (1, 3) for T in (5, 37) for F in (3, 4, 50)]


def _weights(H, T, F):
    return np.random.default_rng(100 * H + 10 * T + F).random((H, T, F)).astype(np.float32)


def test_cost_kernel_against_the_float64_oracle(model):
    worst = {}
    for H, T, F in COST_CASES:
        a = _weights(H, T, F)
        got = model.dev.align_cost(a, 2)
        ref = wa.cost_from_weights(a.astype(np.float64), 2)
        assert got.shape == ref.shape == (T - 3, F)
        worst[(H, T, F)] = float(np.abs(got.astype(np.float64) - ref).max())
    figure = max(worst.values())
    print(f"cost kernel: largest |device - float64 oracle| {figure:.3e} (per case {worst})")
    assert COST_KERNEL_MEASURED is not None, "not measured yet"
    assert figure <= 4 * COST_KERNEL_MEASURED


@pytest.mark.parametrize("H,F", [(1, 3), (1, 50), (3, 50), (3, 4)])
def test_the_median_adds_no_error_of_its_own(model, H, F):
    """Two token rows of +-1: mean 0 and std 1 exactly, so the normalised values are the inputs, the median selects one of
    them and the head mean is a sum of +-1 over H: the fp32 oracle is met bit for bit."""
    s = np.where(np.random.default_rng(F + H).random((H, 1, F)) < 0.5, -1.0, 1.0).astype(np.float32)
    a = np.concatenate([s, -s], axis=1)
    got = model.dev.align_cost(a, 0)
    ref = wa.cost_from_weights(a, 0)
    assert ref.dtype == np.float32 and got.shape == (1, F)
    assert np.array_equal(got, ref)
    if H == 1 and F > 3:
        assert np.array_equal(got[0], -wa.median_filter(s[0, 0]))


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------------
def _rows(m: Model):
    cfg = m.cfg
    seqs = [wa.sequence(cfg, m.base, t) for t in m.text]
    T = max(len(q) for q in seqs)
    assert [len(q) for q in seqs] == [23, 9]
    return [q + [cfg["eot"]] * (T - len(q)) for q in seqs], [len(q) for q in seqs]


@pytest.mark.parametrize("heads", [[(1, 0), (0, 1)], None], ids=["two-heads", "default"])
@pytest.mark.parametrize("which", ["sharp", "soft"])
def test_align_end_to_end(model, soft_model, which, heads):
    m = model if which == "sharp" else soft_model
    seqs, n_tok = _rows(m)
    m.dev.encode(2, m.mel)
    m.dev.set_alignment_heads(heads)
    got = m.dev.align(seqs, n_tok, SOT_LEN, m.n_frames, cost=True)
    launches = m.dev.last_launches()[0]
    assert got["cost"].shape == (2, 19, 100) and got["jump"].shape == (2, 19) and launches > 0 and m.dev.last_flops() > 0
    worst_cost = worst_prob = 0.0
    for r in range(2):
        ref = m.ref(r, heads)
        N, F = len(m.text[r]) + 1, m.n_frames[r] // 2
        cost = got["cost"][r, :N, :F]
        assert np.all(got["cost"][r, N:] == 0) and np.all(got["cost"][r, :, F:] == 0)
        worst_cost = max(worst_cost, float(np.abs(cost.astype(np.float64) - ref["cost"]).max()))            # (a)
        ti, fi = wa.dtw(cost)                                                                                  # (b)
        assert got["jump"][r, :N].tolist() == wa.jumps(ti, fi, N).tolist() and np.all(got["jump"][r, N:] == -1)
        assert np.all(np.diff(got["jump"][r, :N]) >= 0) and 0 <= got["jump"][r, 0] and got["jump"][r, N - 1] < F
        worst_prob = max(worst_prob, float(np.abs(got["prob"][r, :N - 1].astype(np.float64) - ref["prob"]).max()))   # (c)
        assert np.all(got["prob"][r, N - 1:] == 0) and np.all(got["prob"][r, :N - 1] > 0) and np.all(got["prob"][r] <= 1)
    print(f"align end to end, {which} model ({'default heads' if heads is None else heads}): largest |cost - fp16 oracle| {worst_cost:.3e}, "
          f"largest |prob - fp16 oracle| {worst_prob:.3e}; oracle prob range "
          f"{min(m.ref(r, heads)['prob'].min() for r in range(2)):.3e} .. {max(m.ref(r, heads)['prob'].max() for r in range(2)):.3e}")
    # (d) the padded row alone, picked through the window list: the same bits
    alone = m.dev.align([seqs[1][:n_tok[1]]], [n_tok[1]], SOT_LEN, [m.n_frames[1]], windows=[1], cost=True)
    N, F = n_tok[1] - SOT_LEN - 1, m.n_frames[1] // 2
    assert alone["cost"].shape == (1, N, F)
    assert alone["cost"][0].tobytes() == np.ascontiguousarray(got["cost"][1, :N, :F]).tobytes()
    assert alone["jump"][0].tolist() == got["jump"][1, :N].tolist()
    assert alone["prob"][0].tobytes() == np.ascontiguousarray(got["prob"][1, :N]).tobytes()
    m.dev.set_alignment_heads(None)
    assert COST_E2E_MEASURED[which] is not None and PROB_E2E_MEASURED[which] is not None, "not measured yet"
    assert worst_cost <= 4 * COST_E2E_MEASURED[which] and worst_prob <= 4 * PROB_E2E_MEASURED[which]


# ---- 4. the product path ---------------------------------------------------------------------------------------------------------------
def _strip(segments):
    return [{k: v for k, v in s.items() if k != "words"} for s in segments]


@pytest.mark.parametrize("extra", [{}, {"temperature": 0.0, "condition_on_previous_text": True}], ids=["greedy", "fallback-path"])
def test_transcribe_with_word_timestamps(model, extra):
    from eioku_amd import transcribe

    m = model
    audio = wf.audio(20, 6.0)                                               # three 2 s windows
    m.dev.set_alignment_heads(None)
    log = []
    inner = m.dev._window_words

    def spy(items, lang_id, code):
        out = inner(items, lang_id, code)
        log.append((items, out))
        return out

    m.dev._window_words = spy
    try:
        by_mode = {}
        for mode in ("seek", "fixed") if not extra else ("seek",):
            plain = m.dev.transcribe(audio, "en", window_mode=mode, **extra)
            assert not log and all(s["words"] is None for s in plain["segments"])
            out = m.dev.transcribe(audio, "en", window_mode=mode, word_timestamps=True, **extra)
            assert _strip(out["segments"]) == _strip(plain["segments"]) and len(out["segments"]) >= 2
            assert len(log) == 1 if mode == "fixed" else len(log) >= 1            # one align call per batch / per window
            for seg in out["segments"]:
                assert isinstance(seg["words"], list)
                assert sum(len(w["tokens"]) for w in seg["words"]) == len(seg["tokens"])
                assert [t for w in seg["words"] for t in w["tokens"]] == seg["tokens"]
                for w in seg["words"]:
                    assert 0.0 <= w["confidence"] <= 1.0 and w["start"] == w["start_ms"] / 1000 and w["end"] == w["end_ms"] / 1000
            for items, words in log:
                for (_, seek, size, _), per_seg in zip(items, words):
                    times = [t for seg in per_seg for w in seg for t in (w["start_ms"], w["end_ms"])]
                    assert times == sorted(times), f"window at frame {seek}: {times}"
                    assert all(10 * seek <= t <= 10 * (seek + size) for t in times)
            public = transcribe.transcribe_result(out)["segments"]
            assert all(set(w) == {"word", "start", "end", "confidence"} for s in public for w in s["words"])
            by_mode[mode] = out["segments"]
            del log[:]
        if len(by_mode) == 2:       # windows that start at the same frame give the same segments, and then the same words
            key = lambda s: (s["start_ms"], s["end_ms"], tuple(s["tokens"]))       # noqa: E731
            fixed = {key(s): s["words"] for s in by_mode["fixed"]}
            common = [s for s in by_mode["seek"] if key(s) in fixed and s["start_ms"] < 2000]
            assert common, "no segment of the first window is common to both modes"
            for s in common:
                assert s["words"] == fixed[key(s)]
    finally:
        del m.dev._window_words


# ---- 5. rejections ---------------------------------------------------------------------------------------------------------------------
def test_rejections_carry_a_message_and_launch_nothing(model):
    m = model
    seqs, n_tok = _rows(m)
    m.dev.encode(2, m.mel)
    m.dev.align(seqs, n_tok, SOT_LEN, m.n_frames)
    before = m.dev.last_launches()[0]
    assert before > 0
    with pytest.raises(RuntimeError, match="alignment head"):
        m.dev.set_alignment_heads([(2, 0)])
    with pytest.raises(RuntimeError, match="alignment head"):
        m.dev.set_alignment_heads([(0, 2)])
    assert m.dev.last_launches()[0] == before
    eot = m.cfg["eot"]
    with pytest.raises(RuntimeError, match="max_target_positions"):
        m.dev.align([q + [eot] * (65 - len(q)) for q in seqs], n_tok, SOT_LEN, m.n_frames)
    assert m.dev.last_launches()[0] == 0
    m.dev.align(seqs, n_tok, SOT_LEN, m.n_frames)
    with pytest.raises(RuntimeError, match="at least one text token"):
        m.dev.align(seqs, [n_tok[0], SOT_LEN + 2], SOT_LEN, m.n_frames)
    assert m.dev.last_launches()[0] == 0
    for bad, match in (({"n_frames": [200, 1]}, "mel frames"), ({"windows": [0, 2]}, "encoded windows")):
        with pytest.raises(RuntimeError, match=match):
            m.dev.align(seqs, n_tok, SOT_LEN, bad.get("n_frames", m.n_frames), windows=bad.get("windows"))
    bad_ids = [list(q) for q in seqs]
    bad_ids[0][5] = m.cfg["vocab"]
    with pytest.raises(RuntimeError, match="outside the vocabulary"):
        m.dev.align(bad_ids, n_tok, SOT_LEN, m.n_frames)
    assert m.dev.last_launches()[0] == 0
