"""K23 on the host: the filter design, the numpy oracle against scipy, the RIFF parser, the slab plan and the seams."""
import asyncio
import struct
import wave

import numpy as np
import pytest

import audio_oracle as ao
from eioku_amd import audio, task_handler, transcribe
from eioku_amd.model_manager import ModelManager

RATES = (48000, 44100, 8000, 22050, 32000, 96000, 11025, 24000, 12000)
STANDARD = (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000)


# ---- the filter -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_taps_equal_scipys_firwin(rate):
    """Bar 1e-14: thirty times the 3.4e-16 measured between the two designs, room for another libm, nine orders below the
    fp32 rounding of the taps."""
    signal = pytest.importorskip("scipy.signal")
    up, down = audio.resample_ratio(rate)
    m = max(up, down)
    want = signal.firwin(20 * m + 1, 1.0 / m, window=("kaiser", 5.0)) * up
    got = audio.filter_taps(rate)
    diff = float(np.abs(got - want).max())
    print(f"{rate} Hz: up {up} down {down}, {got.size} taps, largest difference from firwin {diff:.2e}")
    assert got.shape == want.shape and diff <= 1e-14


@pytest.mark.parametrize("rate", RATES)
def test_bank_is_the_taps_by_phase_in_fp32_and_equals_the_oracles(rate):
    up, down = audio.resample_ratio(rate)
    h = audio.filter_taps(rate)
    B = audio.filter_bank(rate)
    T = -(-h.size // up)
    assert B.dtype == np.float32 and B.shape == (up, T) and B.flags.c_contiguous
    for p in sorted({0, up // 2, up - 1}):
        for q in (0, T // 2, T - 1):
            want = np.float32(h[p + q * up]) if p + q * up < h.size else np.float32(0)
            assert B[p, q] == want
    assert np.array_equal(B.view(np.uint32), ao.bank(rate).view(np.uint32))
    assert ao.geometry(rate)[:2] == (up, down)


def test_ratio_limits():
    assert audio.resample_ratio(48000) == (1, 3) and audio.resample_ratio(44100) == (160, 441)
    assert audio.resample_ratio(16000) == (1, 1) and audio.resample_ratio(np.int32(8000)) == (2, 1)
    for rate in STANDARD:
        up, down = audio.resample_ratio(rate)
        assert 20 * max(up, down) + 1 <= audio.MAX_TAPS and audio.kernel_tile(up, down) == 256
    assert 20 * 640 + 1 == 12801 == audio.filter_taps(11025).size
    for bad in (0, -16000, 44100.0, "48000", None, True):
        with pytest.raises(ValueError, match="positive integer"):
            audio.resample_ratio(bad)
    with pytest.raises(ValueError, match="15999 Hz"):
        audio.resample_ratio(15999)
    with pytest.raises(ValueError, match="16000000 Hz"):     # 1 / 1000: 20001 taps
        audio.resample_ratio(16_000_000)
    with pytest.raises(ValueError, match="8000000 Hz.*LDS"):    # 1 / 500: 10001 taps fit, a tile's input does not
        audio.resample_ratio(8_000_000)


# ---- the oracle against scipy -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_oracle_against_resample_poly(rate):
    """Equal length, and within (T + 2) 2^-24 max_p sum_q |B[p][q]| max|x| of resample_poly on float64."""
    signal = pytest.importorskip("scipy.signal")
    x = np.random.default_rng(rate).uniform(-1, 1, 4001).astype(np.float32)
    up, down = audio.resample_ratio(rate)
    want = signal.resample_poly(x.astype(np.float64), up, down)
    got = ao.resample(x, rate)
    assert got.dtype == np.float32 and got.shape == want.shape == (audio.output_length(4001, rate),)
    diff, bar = float(np.abs(got - want).max()), ao.bound(x, rate)
    print(f"{rate} Hz: oracle vs resample_poly {diff:.2e}, bound {bar:.2e}")
    assert diff <= bar


@pytest.mark.parametrize("rate", (48000, 44100))
def test_oracle_passes_1_khz_and_stops_12_khz(rate):
    """Measured: a 1 kHz tone keeps 1.0010 / 1.0011 of its RMS, a 12 kHz tone 4.1e-4 / 3.3e-4."""
    t = np.arange(rate) / rate
    rms = lambda v: float(np.sqrt(np.mean(np.square(v.astype(np.float64)))))  # noqa: E731
    kept = {}
    for f in (1000, 12000):
        x = np.sin(2 * np.pi * f * t).astype(np.float32)
        kept[f] = rms(ao.resample(x, rate)[200:-200]) / rms(x[200:-200])
    print(f"{rate} Hz: 1 kHz keeps {kept[1000]:.4f} of its RMS, 12 kHz {kept[12000]:.2e}")
    assert abs(kept[1000] - 1.0) <= 0.01
    assert kept[12000] < 1e-3


def test_oracle_edges():
    assert ao.resample(np.zeros(0, np.float32), 48000).shape == (0,)
    x = np.arange(5, dtype=np.float32)
    y = ao.resample(x, 16000)
    assert np.array_equal(y, x) and y is not x
    assert ao.resample(np.ones(1, np.float32), 8000).shape == (2,)


@pytest.mark.parametrize("channels", (2, 6, 7))
def test_oracle_downmix_of_s16_is_read_wavs_mean(channels, tmp_path):
    v = np.random.default_rng(channels).integers(-32768, 32768, 501 * channels).astype("<i2")
    path = tmp_path / "a.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels), w.setsampwidth(2), w.setframerate(16000)
        w.writeframes(v.tobytes())
    want, _ = transcribe.read_wav(path)
    assert np.array_equal(ao.decode(v.view(np.uint8), "s16", channels).view(np.uint32), want.view(np.uint32))


def test_oracle_decode_values():
    assert list(ao.decode(np.array([0, 128, 255, 64], np.uint8), "u8", 1)) == [-1.0, 0.0, 127 / 128, -0.5]
    s24 = np.array([0x00, 0x00, 0x80, 0xFF, 0xFF, 0x7F, 0xFF, 0xFF, 0xFF, 0x00, 0x00, 0x40], np.uint8)
    assert list(ao.decode(s24, "s24", 1)) == [-1.0, np.float32(8388607 / 8388608), np.float32(-1 / 8388608), 0.5]
    s32 = np.array([-2 ** 31, 2 ** 31 - 1, 2 ** 30, 3], "<i4")
    assert list(ao.decode(s32.view(np.uint8), "s32", 1)) == [-1.0, 1.0, 0.5, np.float32(3 * 2.0 ** -31)]
    f = np.array([0.25, -0.0, 3.0], "<f4")
    assert np.array_equal(ao.decode(f.view(np.uint8), "f32", 1).view(np.uint32), f.view(np.uint32))
    three = np.array([1, 2, 4, 3, 3, 3], "<i2")     # a division, not a reciprocal: (1 + 2 + 4) / 32768 / 3
    want = (np.float32(1 / 32768) + np.float32(2 / 32768) + np.float32(4 / 32768)) / np.float32(3)
    assert ao.decode(three.view(np.uint8), "s16", 3)[0] == want
    for fmt in ao.WIDTH:
        x = ao.make_signal(1, 64, 2, 48000)
        back = ao.decode(ao.encode(x, fmt), fmt, 1)
        assert np.abs(back - x).max() <= (2.0 ** -7 if fmt == "u8" else 2.0 ** -15) and back.min() == -1.0


# ---- read_pcm -----------------------------------------------------------------------------------------------------------------
def _wav(path, tag, bits, channels, rate, payload, *, extensible=False, chunks_before=(), data_size=None, chunks_after=()):
    block = channels * bits // 8
    fmt = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * block, block, bits)
    if extensible:
        fmt += struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", tag) + bytes.fromhex("000000001000800000AA00389B71")
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt
    for cid, data in chunks_before:
        body += cid + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")
    body += b"data" + struct.pack("<I", len(payload) if data_size is None else data_size) + payload
    for cid, data in chunks_after:
        body += (b"\0" if len(payload) & 1 else b"") + cid + struct.pack("<I", len(data)) + data
    path.write_bytes(b"RIFF" + struct.pack("<I", len(body) if data_size is None else 0xFFFFFFFF) + body)
    return path


@pytest.mark.parametrize("tag,bits,fmt", [(1, 8, "u8"), (1, 16, "s16"), (1, 24, "s24"), (1, 32, "s32"), (3, 32, "f32")])
@pytest.mark.parametrize("extensible", (False, True))
def test_read_pcm_every_format(tag, bits, fmt, extensible, tmp_path):
    payload = ao.encode(ao.make_signal(bits, 37, 3, 44100), fmt).tobytes()
    raw, got_fmt, channels, rate, frames = audio.read_pcm(_wav(tmp_path / "a.wav", tag, bits, 3, 44100, payload, extensible=extensible))
    assert (got_fmt, channels, rate, frames) == (fmt, 3, 44100, 37)
    assert raw.dtype == np.uint8 and raw.tobytes() == payload


def test_read_pcm_skips_an_odd_sized_chunk_and_its_pad_byte(tmp_path):
    payload = ao.encode(ao.make_signal(3, 20, 2, 48000), "s16").tobytes()
    p = _wav(tmp_path / "a.wav", 1, 16, 2, 48000, payload, chunks_before=[(b"LIST", b"INFOabc"), (b"fact", b"\1\0\0\0")],
             chunks_after=[(b"LIST", b"tail")])
    raw, fmt, channels, rate, frames = audio.read_pcm(p)
    assert (fmt, channels, rate, frames) == ("s16", 2, 48000, 20) and raw.tobytes() == payload


@pytest.mark.parametrize("size", (0, 0xFFFFFFFF))
def test_read_pcm_takes_a_piped_data_size_as_to_the_end_of_the_file(size, tmp_path):
    payload = ao.encode(ao.make_signal(4, 33, 1, 8000), "s24").tobytes()
    raw, fmt, channels, rate, frames = audio.read_pcm(_wav(tmp_path / "a.wav", 1, 24, 1, 8000, payload, data_size=size))
    assert (fmt, frames) == ("s24", 33) and raw.tobytes() == payload


def test_read_pcm_drops_a_truncated_frame(tmp_path):
    payload = ao.encode(ao.make_signal(5, 10, 2, 48000), "s24").tobytes()
    raw, _, _, _, frames = audio.read_pcm(_wav(tmp_path / "a.wav", 1, 24, 2, 48000, payload[:-2]))
    assert frames == 9 and raw.tobytes() == payload[:54]
    raw, _, _, _, frames = audio.read_pcm(_wav(tmp_path / "b.wav", 1, 24, 2, 48000, payload[:-8], data_size=len(payload)))
    assert frames == 8 and raw.tobytes() == payload[:48], "a data size past the end of the file is clipped to the file"
    assert audio.read_pcm(_wav(tmp_path / "c.wav", 1, 16, 2, 48000, b""))[4] == 0


def test_read_pcm_refusals(tmp_path):
    with pytest.raises(ValueError, match="0x0003.*64 bits"):
        audio.read_pcm(_wav(tmp_path / "a.wav", 3, 64, 1, 48000, bytes(64)))
    with pytest.raises(ValueError, match="0x0002"):
        audio.read_pcm(_wav(tmp_path / "b.wav", 2, 4, 2, 48000, bytes(64)))
    with pytest.raises(ValueError, match="0x0055"):
        audio.read_pcm(_wav(tmp_path / "c.wav", 0x55, 16, 2, 48000, bytes(64), extensible=True))
    with pytest.raises(ValueError, match="9 channels"):
        audio.read_pcm(_wav(tmp_path / "d.wav", 1, 16, 9, 48000, bytes(18)))
    (tmp_path / "e.wav").write_bytes(b"RIFF\x04\0\0\0AVI ")
    with pytest.raises(ValueError, match="not a RIFF/WAVE"):
        audio.read_pcm(tmp_path / "e.wav")
    (tmp_path / "f.wav").write_bytes(b"RIFF\x04\0\0\0WAVE")
    with pytest.raises(ValueError, match="no data chunk"):
        audio.read_pcm(tmp_path / "f.wav")


def test_read_pcm_and_the_oracles_decode_equal_read_wav(tmp_path):
    v = np.random.default_rng(8).integers(-32768, 32768, 2 * 999).astype("<i2")
    path = tmp_path / "a.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2), w.setsampwidth(2), w.setframerate(16000)
        w.writeframes(v.tobytes())
    raw, fmt, channels, rate, frames = audio.read_pcm(path)
    want, want_rate = transcribe.read_wav(path)
    assert (fmt, channels, rate, frames) == ("s16", 2, want_rate, 999)
    assert np.array_equal(ao.decode(raw, fmt, channels).view(np.uint32), want.view(np.uint32))


# ---- the slab plan ------------------------------------------------------------------------------------------------------------
def _check_plan(n_frames, rate, slab_out):
    up, down, m, half, L, T = ao.geometry(rate)
    if rate == 16000:          # the passthrough: output n is frame n
        half, T = 0, 1
    slabs = audio.plan_slabs(n_frames, rate, slab_out)
    n_out = -(-n_frames * up // down)
    at = 0
    for s in slabs:
        assert s["out_start"] == at and 1 <= s["n_out"] <= slab_out
        at += s["n_out"]
        first_t, last_t = s["out_start"] * down + half, (at - 1) * down + half
        assert s["phase"] == first_t % up
        lo, hi = first_t // up - (T - 1), last_t // up           # the first and the last frame any output of the slab reads
        assert s["lead"] >= 0 and s["trail"] >= 0 and s["frames"] >= 0
        assert s["first_frame"] - s["lead"] == lo and s["first_frame"] + s["frames"] + s["trail"] == hi + 1
        assert 0 <= s["first_frame"] and s["first_frame"] + s["frames"] <= n_frames
        assert s["lead"] == max(0, -lo) or s["frames"] == 0
        assert s["frames"] == 0 or s["trail"] == max(0, hi + 1 - n_frames)
        # what the kernel computes, relative to the slab: phase + n * down, and frame indices counted from lo
        assert s["phase"] + (s["n_out"] - 1) * down < 2 ** 31
        assert s["lead"] + s["frames"] + s["trail"] < 2 ** 31 and s["frames"] * 32 < 2 ** 40
    assert at == n_out
    return slabs


def test_plan_slabs_at_three_billion_frames_of_44100_hz():
    slabs = _check_plan(3 * 10 ** 9, 44100, audio.DEFAULT_SLAB_OUT)
    assert len(slabs) == -(-(-(-3 * 10 ** 9 * 160 // 441)) // audio.DEFAULT_SLAB_OUT)
    assert slabs[-1]["out_start"] * 441 + 4410 > 2 ** 31, "the fixture never leaves 31 bits"
    assert slabs[0]["lead"] == 55 - 4410 // 160 and slabs[-1]["trail"] > 0
    assert all(s["lead"] == 0 and s["trail"] == 0 for s in slabs[1:-1])


@pytest.mark.parametrize("rate", RATES + (16000,))
def test_plan_slabs_small_and_ragged(rate):
    for n_frames, slab_out in ((0, 10), (1, 10), (4001, 1000), (4001, 10 ** 6), (20, 7)):
        slabs = _check_plan(n_frames, rate, slab_out)
        assert (not slabs) == (n_frames == 0)


def test_plan_slabs_clamps_the_slab_to_31_bits():
    slabs = audio.plan_slabs(10 ** 10, 192000, 1 << 30)        # down = 12: 2^30 outputs would reach 12 * 2^30
    assert max(s["n_out"] for s in slabs) == (2 ** 31 - 2 - 241) // 12        # T = 241 frames of filter behind the last output
    _check_plan(10 ** 10, 192000, 1 << 30)


def test_plan_slabs_equals_the_librarys(built_lib):
    """``eioku_audio_plan`` is the host function ``eioku_audio_resample`` walks its slabs with."""
    for n_frames, rate, slab_out in ((3 * 10 ** 9, 44100, 1 << 22), (4001, 8000, 1000), (4001, 11025, 333), (5, 16000, 2),
                                     (10 ** 10, 192000, 1 << 26)):
        up, down, half, T = audio._geometry(rate)
        slabs = audio.plan_slabs(n_frames, rate, slab_out)
        row = np.zeros(7, dtype=np.int64)
        for k in sorted({0, 1, len(slabs) // 2, len(slabs) - 1} & set(range(len(slabs)))):
            assert built_lib.eioku_audio_plan(up, down, T, slab_out, n_frames, k, row.ctypes.data) == 0
            assert dict(zip(audio.PLAN_KEYS, (int(v) for v in row))) == slabs[k]
        assert built_lib.eioku_audio_plan(up, down, T, slab_out, n_frames, len(slabs), row.ctypes.data) == 1


# ---- seams --------------------------------------------------------------------------------------------------------------------
class _FakeTranscriber:
    def __init__(self):
        self.calls, self.closed = [], False

    def transcribe(self, samples, language, **kw):
        self.calls.append((np.array(samples), language, kw))
        return {"language": "en", "segments": [{"start_ms": 0, "end_ms": 500, "text": " a", "language": "en",
                                                "confidence": None, "words": None}]}

    def close(self):
        self.closed = True


class _FakeFrontEnd:
    """Doubles or halves by repetition: enough to see what went through it."""

    def __init__(self):
        self.loads, self.floats, self.closed = [], [], False

    def load(self, path):
        self.loads.append(path)
        return np.full(321, 0.5, dtype=np.float32), 16000

    def resample_float(self, samples, rate):
        self.floats.append((np.array(samples), rate))
        return np.repeat(np.asarray(samples, dtype=np.float32), 16000 // rate)

    def close(self):
        self.closed = True


AUDIO = (np.arange(3000, dtype=np.float32) % 100) / 100


def test_a_source_at_8000_hz_reaches_the_transcriber_as_twice_the_samples():
    t, fe = _FakeTranscriber(), _FakeFrontEnd()
    out = transcribe.transcribe_video("v.mp4", {"vad_filter": False}, transcriber=t, audio_source=lambda path: (AUDIO, 8000),
                                      audio_frontend=fe)
    assert len(fe.floats) == 1 and fe.floats[0][1] == 8000 and np.array_equal(fe.floats[0][0], AUDIO) and fe.loads == []
    assert t.calls[0][0].size == 2 * AUDIO.size and t.calls[0][0].dtype == np.float32
    assert [(s["start_ms"], s["end_ms"]) for s in out["segments"]] == [(0, 500)]


def test_a_source_at_16000_hz_does_not_touch_the_front_end_and_no_source_means_load():
    t, fe = _FakeTranscriber(), _FakeFrontEnd()
    transcribe.transcribe_video("v.mp4", {}, transcriber=t, audio_source=lambda path: (AUDIO, 16000), audio_frontend=fe)
    assert fe.floats == [] and fe.loads == [] and t.calls[0][0].size == AUDIO.size
    transcribe.transcribe_video("clip.mp4", {}, transcriber=t, audio_frontend=fe)
    assert fe.loads == ["clip.mp4"] and t.calls[1][0].size == 321


def test_without_the_front_end_the_old_error_remains():
    t = _FakeTranscriber()
    with pytest.raises(ValueError, match="8000 Hz: Whisper needs 16000 Hz and resampling is not built"):
        transcribe.transcribe_video("v.mp4", {}, transcriber=t, audio_source=lambda path: (AUDIO, 8000))
    assert t.calls == []


@pytest.mark.parametrize("rate", (15999, 0, -8000, 44100.5, 16_000_000))
def test_the_limits_raise_before_any_call(rate):
    t, fe = _FakeTranscriber(), audio.AudioFrontEnd()
    with pytest.raises(ValueError):
        transcribe.transcribe_video("v.mp4", {}, transcriber=t, audio_source=lambda path: (AUDIO, rate), audio_frontend=fe)
    assert t.calls == [] and fe.lib is None, "the library was loaded for a refusal"


def test_bad_channels_and_formats_raise_before_any_device_work():
    fe = audio.AudioFrontEnd()
    raw = np.zeros(64, np.uint8)
    for fmt, channels in (("s16", 0), ("s16", 9), ("s16", 2.0), ("s20", 2), ("f64", 1), (None, 1)):
        with pytest.raises(ValueError):
            fe.resample(raw, fmt, channels, 48000)
    assert fe.lib is None
    assert fe.resample(np.zeros(3, np.uint8), "s16", 2, 48000).shape == (0,) and fe.lib is None, "zero frames give zero samples"
    with pytest.raises(ValueError):
        audio.AudioFrontEnd(slab_out=0)


def test_load_hands_npy_and_missing_files_to_the_default_source(tmp_path):
    fe = audio.AudioFrontEnd()
    np.save(tmp_path / "a.npy", AUDIO)
    samples, rate = fe.load(tmp_path / "a.npy")
    assert rate == 16000 and np.array_equal(samples, AUDIO)
    with pytest.raises(FileNotFoundError, match="no audio for"):
        fe.load(tmp_path / "video.mp4")
    assert fe.lib is None


def _manager(tmp_path, t, fe, made, **kw):
    def factory():
        made.append(1)
        return fe

    return ModelManager(cache_dir=str(tmp_path), gpu_transcription=True, transcriber_factory=lambda cache, name: t,
                        audio_frontend_factory=factory, **kw)


def test_model_manager_hands_the_front_end_through_and_closes_it(tmp_path):
    t, fe, made = _FakeTranscriber(), _FakeFrontEnd(), []
    out = asyncio.run(_manager(tmp_path, t, fe, made, gpu_audio=True).transcribe_video("v.mp4", {"languages": "en"}))
    assert made == [1] and fe.loads == ["v.mp4"] and t.calls[0][0].size == 321 and fe.closed and t.closed
    assert len(out["segments"]) == 1
    t, fe, made = _FakeTranscriber(), _FakeFrontEnd(), []
    mm = _manager(tmp_path, t, fe, made, gpu_audio=True, audio_source=lambda path: (AUDIO, 8000))
    asyncio.run(mm.transcribe_video("v.mp4", {}))
    assert fe.loads == [] and len(fe.floats) == 1 and t.calls[0][0].size == 2 * AUDIO.size


def test_model_manager_without_gpu_audio_builds_no_front_end_and_refuses_as_before(tmp_path):
    t, fe, made = _FakeTranscriber(), _FakeFrontEnd(), []
    mm = _manager(tmp_path, t, fe, made, audio_source=lambda path: (AUDIO, 8000))
    with pytest.raises(ValueError, match="resampling is not built"):
        asyncio.run(mm.transcribe_video("v.mp4", {}))
    assert made == [] and t.calls == [] and t.closed


def test_process_ml_task_honours_gpu_audio(tmp_path, monkeypatch):
    monkeypatch.setenv("MODEL_CACHE_DIR", str(tmp_path))
    t, fe, made, kwargs, got = _FakeTranscriber(), _FakeFrontEnd(), [], [], []

    def factory(cache_dir, **kw):
        kwargs.append(kw)
        return _manager(tmp_path, t, fe, made, gpu_audio=kw.get("gpu_audio", False), audio_source=lambda path: (AUDIO, 8000))

    ctx = {"gpu_transcription": True, "gpu_audio": True, "model_manager_factory": factory, "artifact_sink": got.extend}
    res = asyncio.run(task_handler.process_ml_task(ctx, "t1", "transcription", "vid", "v.mp4", {"languages": "en"}))
    assert kwargs == [{"gpu_transcription": True, "gpu_audio": True}]
    assert res == {"task_id": "t1", "status": "completed", "artifact_count": 1} and len(fe.floats) == 1
    ctx = {"gpu_transcription": True, "gpu_vad": True, "gpu_audio": True, "model_manager_factory": factory, "artifact_sink": got.extend}
    asyncio.run(task_handler.process_ml_task(ctx, "t2", "transcription", "vid", "v.mp4", {}))
    assert kwargs[1] == {"gpu_transcription": True, "gpu_vad": True, "gpu_audio": True}
    ctx = {"gpu_transcription": True, "model_manager_factory": factory, "artifact_sink": got.extend}
    with pytest.raises(RuntimeError, match="resampling is not built"):
        asyncio.run(task_handler.process_ml_task(ctx, "t3", "transcription", "vid", "v.mp4", {}))
    assert kwargs[2] == {"gpu_transcription": True}
