"""K22 on the device against tests/vad_oracle.py (the float64 CPU oracle).

Shape: 37 chunks + 100 samples = 38 chunks after padding, handles with ``slab_chunks = 8`` (four slab edges and a ragged
last slab of 6) and ``slab_chunks = 64`` (one slab); the tile of ``k_vad_encode`` (4 chunks) divides neither 38 nor 6."""
import ctypes as C

import numpy as np
import pytest
import torch

import vad_oracle as vo
import whisper_oracle as wo

pytestmark = pytest.mark.gpu

SEED = 13
N_SAMPLES = 37 * 512 + 100
BURSTS = [(3 * 512 + 17, 11 * 512 + 300, 0.3), (16 * 512, 24 * 512 + 5, 0.05), (30 * 512 + 250, 35 * 512, 0.5)]
# largest |device - float64 oracle| over the 38 probabilities, measured on the MI355X (the fp32-mode oracle's own drift on
# the same input, on that machine's CPU: 1.2e-07); the bar is 4 x the measurement
MEASURED_DRIFT = 3.35e-07
DRIFT_BAR = 4 * MEASURED_DRIFT


class Fixture:
    def __init__(self):
        from eioku_amd.vad import SileroVad

        self.weights = vo.random_weights(SEED)
        self.audio = vo.burst_audio(100 + SEED, N_SAMPLES, BURSTS)
        self.o64 = vo.Oracle(self.weights)
        self.ref = self.o64.probs(self.audio)
        self.ref32 = vo.Oracle(self.weights, torch.float32).probs(self.audio)
        self.dev8 = SileroVad(self.weights, slab_chunks=8)
        self.dev64 = SileroVad(self.weights, slab_chunks=64)
        self.got8 = self.dev8.speech_probs(self.audio)

    def close(self):
        self.dev8.close()
        self.dev64.close()


@pytest.fixture(scope="module")
def fx(gpu):
    f = Fixture()
    yield f
    f.close()


def test_the_fixture_exercises_both_decisions(fx):
    """Conditions on the seeded weights and audio, against the oracle alone."""
    p = fx.ref
    assert p.shape == (38,)
    assert (p >= 0.5).any() and (p < 0.5).any() and p.std() >= 0.1
    assert np.abs(p - 0.5).min() > 1e-3 and np.abs(p - 0.35).min() > 1e-3


def test_probabilities_against_the_float64_oracle(fx):
    """Measured on the MI355X: largest |device - float64 oracle| 3.350e-07 (fp32-mode oracle vs float64: 1.211e-07)."""
    assert fx.got8.dtype == np.float32 and fx.got8.shape == (38,)
    drift = float(np.abs(fx.got8.astype(np.float64) - fx.ref).max())
    own = float(np.abs(fx.ref32 - fx.ref).max())
    print(f"VAD probabilities: device vs float64 oracle {drift:.3e}; fp32-mode oracle vs float64 {own:.3e}; bar {DRIFT_BAR:.3e}")
    assert own < 1e-5, "the fp32-mode oracle itself is off: the fixture is ill-conditioned"
    assert drift <= DRIFT_BAR


def test_slabs_of_8_and_one_slab_are_bit_identical(fx):
    one = fx.dev64.speech_probs(fx.audio)
    assert np.array_equal(fx.got8.view(np.uint32), one.view(np.uint32))
    assert np.array_equal(fx.dev8.speech_probs(fx.audio).view(np.uint32), fx.got8.view(np.uint32)), "a second call differs"


def test_first_chunk_context_is_zeros_and_state_is_reset_between_files(fx):
    """A second file on a used handle, starting inside a burst: chunk 0 equals the oracle's called with an explicit zero
    context, and differs from the oracle's under the context the previous samples would have given."""
    start = 5 * 512
    tail = fx.audio[start:]
    got = fx.dev8.speech_probs(tail)
    zero = fx.o64.probs(tail, context=np.zeros(64, dtype=np.float32))
    carried = fx.o64.probs(tail, context=fx.audio[start - 64:start])
    print(f"chunk 0: device {got[0]:.7f}, oracle with zero context {zero[0]:.7f}, with the file's context {carried[0]:.7f}")
    assert abs(carried[0] - zero[0]) > 100 * DRIFT_BAR, "the fixture cannot tell the two contexts apart"
    assert abs(float(got[0]) - zero[0]) <= DRIFT_BAR
    assert np.abs(got.astype(np.float64) - zero).max() <= DRIFT_BAR


def test_decisions_equal_the_oracles(fx):
    from eioku_amd import vad

    for options in (vad.VadOptions(), vad.VadOptions(min_silence_duration_ms=64, speech_pad_ms=30),
                    vad.VadOptions(min_silence_duration_ms=0, speech_pad_ms=0, max_speech_duration_s=0.2)):
        want = vad.speech_timestamps(fx.ref, N_SAMPLES, options)
        assert want, "the fixture has speech"
        assert vad.speech_timestamps(fx.got8, N_SAMPLES, options) == want


def test_a_multiple_of_512_samples_gets_a_whole_zero_chunk(fx):
    x = fx.audio[4 * 512:6 * 512]
    got = fx.dev8.speech_probs(x)
    assert got.shape == (3,)
    assert np.abs(got.astype(np.float64) - fx.o64.probs(x)).max() <= DRIFT_BAR
    assert fx.dev8.speech_probs(np.zeros(0, dtype=np.float32)).shape == (1,)


def test_probs_is_refused_before_the_tensors_are_set_and_with_too_small_a_buffer(fx):
    from eioku_amd import _lib

    lib = _lib.load()
    h = C.c_void_p()
    assert lib.eioku_vad_create(0, C.byref(h)) != 0 and b"slab_chunks" in lib.eioku_last_error()
    _lib.check(lib.eioku_vad_create(8, C.byref(h)), "eioku_vad_create")
    try:
        out, n = np.full(64, -1.0, dtype=np.float32), C.c_longlong(0)
        rc = lib.eioku_vad_probs(h, fx.audio.ctypes.data, fx.audio.size, out.ctypes.data, out.size, C.byref(n))
        assert rc != 0 and b"has not been set" in lib.eioku_last_error() and (out == -1.0).all()
    finally:
        lib.eioku_vad_destroy(h)
    out, n = np.full(37, -1.0, dtype=np.float32), C.c_longlong(0)
    rc = lib.eioku_vad_probs(fx.dev8._h, fx.audio.ctypes.data, fx.audio.size, out.ctypes.data, out.size, C.byref(n))
    assert rc != 0 and b"holds 37" in lib.eioku_last_error() and n.value == 38 and (out == -1.0).all()
    assert np.array_equal(fx.dev8.speech_probs(fx.audio), fx.got8), "the handle still works after a refusal"


# ---- coexistence: a VAD handle and a Whisper handle in one transcribe_video ---------------------------------------------------
E2E_SAMPLES = 9 * 16000
E2E_AUDIO_SEED = 26      # of the noise seeds tried on the CPU oracles, one whose windows both decode to a segment
E2E_BURSTS = [(16000, 16000 + 16500, 0.3), (80000, 80000 + 19000, 0.3)]   # 1 s of zeros, burst, 2.97 s of zeros, burst, 2.8 s of zeros


def _by_hand(t_ms, chunks, is_end):
    """File time of ``t_ms`` in the concatenation of ``chunks``: walk the chunks' lengths."""
    before = 0
    for k, c in enumerate(chunks):
        length = c["end"] - c["start"]
        inside = 16 * t_ms < before + length or (is_end and 16 * t_ms == before + length)
        if inside or k == len(chunks) - 1:
            assert c["start"] % 16 == 0 and before % 16 == 0
            return c["start"] // 16 + t_ms - before // 16
        before += length


def test_vad_and_whisper_together_through_transcribe_video(fx):
    """The oracle's chunks of this audio are (9472, 40192) and (73472, 106752): 64000 samples, exactly two 2 s windows of
    model A in fixed mode, so every decoded time lies inside the collected audio."""
    from eioku_amd import transcribe, vad

    cfg = wo.model_a_config()
    tb = cfg["timestamp_begin"]
    weights = wo.random_weights(cfg, 5, {cfg["eot"]: 1.2, **{tb + i: 1.2 for i in range(cfg["vocab"] - tb)}})
    audio = vo.burst_audio(E2E_AUDIO_SEED, E2E_SAMPLES, E2E_BURSTS)
    config = {"languages": ["en"], "window_mode": "fixed", "batch_windows": 2}
    whisper = transcribe.WhisperTranscriber(dict(cfg), {k: v.numpy() for k, v in weights.items()})
    try:
        chunks = vad.speech_timestamps(fx.dev8.speech_probs(audio), audio.size)
        assert chunks == vad.speech_timestamps(fx.o64.probs(audio), audio.size)
        assert len(chunks) == 2 and sum(c["end"] - c["start"] for c in chunks) == 64000
        assert chunks[1]["start"] - chunks[0]["end"] > 2 * 16000
        raw = whisper.transcribe(vad.collect_chunks(audio, chunks), "en", window_mode="fixed", batch_windows=2)
        got = transcribe.transcribe_video("clip.mp4", config, transcriber=whisper, audio_source=lambda path: (audio, 16000),
                                          vad=fx.dev8)
        unfiltered = transcribe.transcribe_video("clip.mp4", config, transcriber=whisper, audio_source=lambda path: (audio, 16000))
    finally:
        whisper.close()
    assert len(raw["segments"]) >= 2 and len(got["segments"]) == len(raw["segments"])
    assert any(16 * s["start_ms"] >= chunks[0]["end"] - chunks[0]["start"] for s in raw["segments"]), "nothing in the second chunk"
    previous = 0
    for g, r in zip(got["segments"], raw["segments"]):
        want = {"start_ms": _by_hand(r["start_ms"], chunks, False), "end_ms": _by_hand(r["end_ms"], chunks, True),
                "text": r["text"], "language": r["language"], "confidence": r["confidence"], "words": None}
        assert g == want
        for t in (g["start_ms"], g["end_ms"]):
            assert any(c["start"] <= 16 * t <= c["end"] for c in chunks), f"{t} ms is outside every speech chunk"
            assert t >= previous
            previous = t
    assert got != unfiltered, "the filter changed nothing"
