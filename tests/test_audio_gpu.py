"""K23 on the device against tests/audio_oracle.py: the same fp32 operations in numpy, so every comparison is of bits.

Rows: the rates and layouts below.  Lengths per row: 1 frame, T - 1 frames (shorter than one phase of the filter), 4001 frames
(several tiles and a ragged last one) and the shortest input whose output is the least above two whole tiles of the
kernel: 2 * tile + 1 outputs wherever the ratio reaches that count, 2 * tile + 2 at 8000 Hz, where every count is even."""
import asyncio
import wave

import numpy as np
import pytest

import audio_oracle as ao
import vad_oracle as vo
import whisper_oracle as wo

pytestmark = pytest.mark.gpu

ROWS = [(48000, 2, "s16"), (44100, 2, "s16"), (48000, 6, "s24"), (8000, 1, "u8"), (22050, 1, "f32"), (96000, 2, "s32"),
        (11025, 1, "s16")]
IDS = [f"{r}-{c}ch-{f}" for r, c, f in ROWS]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Fixture:
    def __init__(self):
        from eioku_amd.audio import AudioFrontEnd

        self.fe = AudioFrontEnd()
        self.fe1000 = AudioFrontEnd(slab_out=1000)
        self.cache = {}

    def case(self, rate, channels, fmt, frames):
        """(raw PCM, the oracle's 16 kHz samples), computed once."""
        key = (rate, channels, fmt, frames)
        if key not in self.cache:
            raw = ao.encode(ao.make_signal(rate + 31 * channels + frames, frames, channels, rate), fmt)
            self.cache[key] = (raw, ao.resample(ao.decode(raw, fmt, channels), rate))
        return self.cache[key]

    def close(self):
        self.fe.close()
        self.fe1000.close()


@pytest.fixture(scope="module")
def fx(gpu):
    f = Fixture()
    yield f
    f.close()


def just_above_two_tiles(rate, tile):
    """(frames, outputs): the fewest outputs above 2 * tile that some whole number of input frames gives."""
    up, down = ao.geometry(rate)[:2]
    n = 2 * tile * down // up
    while -(-n * up // down) <= 2 * tile:
        n += 1
    return n, -(-n * up // down)


@pytest.mark.parametrize("rate,channels,fmt", ROWS, ids=IDS)
def test_bit_equality_with_the_oracle(fx, rate, channels, fmt):
    T = ao.geometry(rate)[5]
    tile = fx.fe.tile(rate)
    edge, edge_out = just_above_two_tiles(rate, tile)
    assert tile == 256 and edge_out == 2 * tile + (2 if rate == 8000 else 1)
    for frames in (1, T - 1, 4001, edge):
        raw, want = fx.case(rate, channels, fmt, frames)
        got = fx.fe.resample(raw, fmt, channels, rate)
        assert got.dtype == np.float32 and got.shape == want.shape
        wrong = np.flatnonzero(bits(got) != bits(want))
        print(f"{rate} Hz {channels} ch {fmt}, {frames} frames -> {got.size} samples: {wrong.size} differ"
              + (f", first at {wrong[0]}: device {got[wrong[0]]!r}, oracle {want[wrong[0]]!r}" if wrong.size else ""))
        assert wrong.size == 0
        assert np.abs(want).max() > 0.05, "the case is silent"
    assert fx.fe.last_ms() > 0


@pytest.mark.parametrize("rate,channels,fmt", [ROWS[1], ROWS[3]], ids=[IDS[1], IDS[3]])
def test_slabs_of_1000_and_one_slab_are_bit_identical(fx, rate, channels, fmt):
    from eioku_amd import audio

    raw, want = fx.case(rate, channels, fmt, 4001)
    slabs = audio.plan_slabs(4001, rate, 1000)
    assert len(slabs) >= 2 and slabs[-1]["n_out"] not in (0, 1000) and len(audio.plan_slabs(4001, rate)) == 1
    small = fx.fe1000.resample(raw, fmt, channels, rate)
    assert np.array_equal(bits(small), bits(fx.fe.resample(raw, fmt, channels, rate)))
    assert np.array_equal(bits(small), bits(want))
    assert np.array_equal(bits(fx.fe1000.resample(raw, fmt, channels, rate)), bits(small)), "a second call differs"


def test_16000_hz_is_a_passthrough_equal_to_read_wav(fx, tmp_path):
    from eioku_amd import transcribe

    v = np.random.default_rng(16).integers(-32768, 32768, 2 * 2777).astype("<i2")
    path = tmp_path / "a.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2), w.setsampwidth(2), w.setframerate(16000)
        w.writeframes(v.tobytes())
    want, rate = transcribe.read_wav(path)
    for fe in (fx.fe, fx.fe1000):
        got, got_rate = fe.load(path)
        assert got_rate == rate == 16000 and got.shape == (2777,) and np.array_equal(bits(got), bits(want))


def test_float_samples_zero_frames_and_refusals(fx):
    from eioku_amd import _lib

    x = np.random.default_rng(5).uniform(-1, 1, 700).astype(np.float32)
    assert np.array_equal(bits(fx.fe.resample_float(x, 8000)), bits(ao.resample(x, 8000)))
    assert fx.fe.resample(np.zeros(0, np.uint8), "s16", 2, 48000).shape == (0,)
    lib = _lib.load()
    import ctypes as C

    h, bank = C.c_void_p(), np.zeros((1, 61), np.float32)
    assert lib.eioku_audio_create(1, 3, 60, bank.ctypes.data, 1000, C.byref(h)) != 0 and b"taps per phase" in lib.eioku_last_error()
    assert lib.eioku_audio_create(2, 6, 61, bank.ctypes.data, 1000, C.byref(h)) != 0 and b"lowest terms" in lib.eioku_last_error()
    assert lib.eioku_audio_create(1, 3, 61, bank.ctypes.data, 0, C.byref(h)) != 0 and b"slab_out" in lib.eioku_last_error()
    raw, want = fx.case(48000, 2, "s16", 4001)
    out, n = np.full(10, -1.0, np.float32), C.c_longlong(0)
    h48 = fx.fe._handle(48000, 1, 3)
    rc = lib.eioku_audio_resample(h48, raw.ctypes.data, 1, 2, 4001, out.ctypes.data, out.size, C.byref(n))
    assert rc != 0 and b"holds 10" in lib.eioku_last_error() and n.value == want.size and (out == -1.0).all()
    assert lib.eioku_audio_resample(h48, raw.ctypes.data, 7, 2, 4001, out.ctypes.data, out.size, C.byref(n)) != 0
    assert lib.eioku_audio_resample(h48, raw.ctypes.data, 1, 9, 4001, out.ctypes.data, out.size, C.byref(n)) != 0
    assert np.array_equal(bits(fx.fe.resample(raw, "s16", 2, 48000)), bits(want)), "the handle still works after a refusal"


# ---- end to end: a 48 kHz stereo 24-bit WAV through ModelManager -----------------------------------------------------------------
def test_a_48_khz_24_bit_stereo_wav_through_the_model_manager(fx, tmp_path):
    """The audio is the speech the VAD end-to-end test collects (two 2 s windows of model A that both decode to a segment),
    interpolated to 48 kHz, the right channel at half the level.  On the MI355X: three segments, (900, 1320), (1920, 1940)
    and (2120, 3100) ms, from the file and from the oracle's samples alike."""
    from eioku_amd import transcribe
    from eioku_amd.model_manager import ModelManager

    cfg = wo.model_a_config()
    tb = cfg["timestamp_begin"]
    weights = {k: v.numpy() for k, v in
               wo.random_weights(cfg, 5, {cfg["eot"]: 1.2, **{tb + i: 1.2 for i in range(cfg["vocab"] - tb)}}).items()}
    audio16 = vo.burst_audio(26, 9 * 16000, [(16000, 16000 + 16500, 0.3), (80000, 80000 + 19000, 0.3)])
    speech = np.concatenate([audio16[9472:40192], audio16[73472:106752]]).astype(np.float64)
    left = np.interp(np.arange(3 * speech.size) / 3.0, np.arange(speech.size), speech)
    raw = ao.encode(np.stack([left, 0.5 * left], axis=1).reshape(-1), "s24")
    wav = tmp_path / "clip.wav"
    with wave.open(str(wav), "wb") as w:
        w.setnchannels(2), w.setsampwidth(3), w.setframerate(48000)
        w.writeframes(raw.tobytes())
    want16 = ao.resample(ao.decode(raw, "s24", 2), 48000)
    assert want16.shape == (speech.size,)
    np.save(tmp_path / "oracle.npy", want16)

    seen = []

    class Recording(transcribe.WhisperTranscriber):
        def transcribe(self, samples, language, **kw):
            seen.append(np.array(samples, dtype=np.float32))
            return super().transcribe(samples, language, **kw)

    def manager(**kw):
        return ModelManager(cache_dir=str(tmp_path / "cache"), gpu_transcription=True,
                            transcriber_factory=lambda cache, name: Recording(dict(cfg), weights), **kw)

    config = {"languages": ["en"], "window_mode": "fixed", "batch_windows": 2}
    got = asyncio.run(manager(gpu_audio=True).transcribe_video(str(wav), config))
    want = asyncio.run(manager(gpu_audio=True).transcribe_video(str(tmp_path / "oracle.npy"), config))
    assert len(seen) == 2 and np.array_equal(bits(seen[0]), bits(want16)) and np.array_equal(bits(seen[1]), bits(want16))
    print(f"{len(got['segments'])} segments: {[(s['start_ms'], s['end_ms']) for s in got['segments']]}")
    assert got["segments"] and got == want
    with pytest.raises(ValueError, match="only 16-bit PCM WAV is read"):
        asyncio.run(manager().transcribe_video(str(wav), config))
    assert len(seen) == 2
