"""Transcription, host side (no GPU): the CPU oracle against Hugging Face, segment cutting and seek, BPE decode, audio
sources, the result dict and the opt-in switches."""
import asyncio
import json
import wave

import numpy as np
import pytest
import torch

import whisper_oracle as wo
from whisper_testlib import checkpoint_json, write_checkpoint
from eioku_amd import task_handler, transcribe
from eioku_amd.model_manager import ModelManager


def _audio(seed: int, seconds: float) -> np.ndarray:
    rng = np.random.default_rng(seed)
    t = np.arange(int(seconds * 16000)) / 16000.0
    x = sum(rng.uniform(0.05, 0.3) * np.sin(2 * np.pi * rng.uniform(80, 4000) * t + rng.uniform(0, 6)) for _ in range(6))
    return (x + 0.01 * rng.standard_normal(len(t))).astype(np.float32)


# ---- the oracle against Hugging Face ----------------------------------------------------------------------------------------
def test_product_mel_filters_equal_the_oracles_and_hf():
    audio_utils = pytest.importorskip("transformers.audio_utils")
    for n_mels in (80, 128):
        ours = transcribe.mel_filter_bank(n_mels)
        hf = audio_utils.mel_filter_bank(num_frequency_bins=201, num_mel_filters=n_mels, min_frequency=0.0, max_frequency=8000.0,
                                         sampling_rate=16000, norm="slaney", mel_scale="slaney").T
        assert ours.shape == (n_mels, 201) and ours.dtype == np.float64
        np.testing.assert_allclose(ours, wo.mel_filters(n_mels), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(ours, hf, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("n_mels", [80, 128])
def test_oracle_log_mel_matches_whisper_feature_extractor(n_mels):
    """Against the extractor's numpy path, which keeps the waveform in float64, its STFT in complex64 (relative error
    2^-24 per component, 1.2e-7 on the power, 5.2e-8 on log10) and casts the log spectrum to float32 before the clamp and
    (x + 4) / 4 (values up to |-10|: steps of 9.5e-7, a few roundings, divided by 4): the bound is 2e-6 absolute.

    The public call uses torch.stft in float32 when torch is importable.  An fp32 FFT of N = 400 points carries an error of
    about log2(N) u ||frame||_2 (u = 2^-24) in every bin, whatever the bin's own size, so bins far below the frame's peak
    are noise-dominated; the bound for that path is per element: 2e-6 + dE / (4 ln(10) E) with dE = sum_k f_mk (2 |X_k| d +
    d^2), d = 9 u ||frame||_2."""
    transformers = pytest.importorskip("transformers")
    fe = transformers.WhisperFeatureExtractor(feature_size=n_mels)
    x = _audio(3, 4.0)
    ours = wo.log_mel(x, 0, 3000, n_mels).astype(np.float64)
    chunk = np.zeros(480000, dtype=np.float32)
    chunk[:len(x)] = x
    hf64 = np.asarray(fe._np_extract_fbank_features(chunk[None], "cpu"))[0]
    assert hf64.shape == ours.shape == (n_mels, 3000)
    err = np.abs(ours - hf64).max()
    print("log-mel max abs difference to the extractor's numpy path:", err)
    assert err <= 2e-6
    hf = fe(x, sampling_rate=16000, return_tensors="np")["input_features"][0].astype(np.float64)
    padded = np.pad(chunk.astype(np.float64), 200, mode="reflect")
    frames = padded[np.arange(3000)[:, None] * 160 + np.arange(400)[None, :]] * (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(400) / 400))
    amp = np.abs(np.fft.rfft(frames, axis=1))                                        # [T][201]
    d = 9 * 2.0 ** -24 * np.linalg.norm(frames, axis=1)[:, None]
    filt = wo.mel_filters(n_mels)
    energy = np.maximum(filt @ (amp ** 2).T, 1e-10)
    tol = 2e-6 + (filt @ (2 * amp * d + d * d).T) / (4 * np.log(10) * energy)
    clamped = ours <= (ours.max() - 2.0) + 1e-6   # at the max - 8 floor both sides hold the same constant
    excess = np.where(clamped, 0.0, np.abs(ours - hf) - tol)
    print("public call: max abs difference", np.abs(ours - hf).max(), "largest excess over the per-element bound", excess.max())
    assert excess.max() <= 0 and np.abs(ours - hf)[clamped].max() <= 2e-6


def _hf_model(cfg, weights):
    transformers = pytest.importorskip("transformers")
    hf_cfg = transformers.WhisperConfig(
        vocab_size=cfg["vocab"], num_mel_bins=cfg["n_mels"], d_model=cfg["d_model"], encoder_layers=cfg["enc_layers"],
        decoder_layers=cfg["dec_layers"], encoder_attention_heads=cfg["heads"], decoder_attention_heads=cfg["heads"],
        encoder_ffn_dim=cfg["enc_ffn"], decoder_ffn_dim=cfg["dec_ffn"], max_source_positions=cfg["max_source_positions"],
        max_target_positions=cfg["max_target_positions"], pad_token_id=cfg["eot"], bos_token_id=cfg["eot"],
        eos_token_id=cfg["eot"], decoder_start_token_id=cfg["sot"], dropout=0.0, attention_dropout=0.0, activation_dropout=0.0)
    model = transformers.WhisperForConditionalGeneration(hf_cfg).eval()
    state = {k: v.clone() for k, v in weights.items()}
    state["proj_out.weight"] = state["model.decoder.embed_tokens.weight"]
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not unexpected and all("proj_out" in m for m in missing), (missing, unexpected)
    return model


@pytest.mark.parametrize("which", ["a", "c"])
def test_oracle_fp32_logits_match_whisper_for_conditional_generation(which):
    """Model A, and model C: 128 mel bins, 6 heads, 2 + 3 layers, unequal ffn sizes, ids from the large-v3 layout.

    The bar compares two fp32 programs, so the weights must leave fp32 rounding below it.  With q / k projections x 4 model
    C's three decoder layers amplify it past the bar: run in float64 the oracle and the HF model agree to 7e-13, while either
    fp32 run sits 2.0e-3 (1e-3 of the rms) from that float64 result and the two fp32 runs 2.7e-4 from each other.  At q / k x 2
    an fp32 run is 2.4e-5 from float64, so a difference above the bar is a difference in the arithmetic, which is what
    this test is for; model A keeps its weights."""
    cfg = wo.model_a_config() if which == "a" else wo.model_c_config()
    weights = wo.random_weights(cfg, seed=11, qk_scale=4.0 if which == "a" else 2.0)
    model = _hf_model(cfg, weights)
    frames, tb = 2 * cfg["max_source_positions"], cfg["timestamp_begin"]
    mel = np.stack([wo.log_mel(_audio(s, frames / 100.0), 0, frames, cfg["n_mels"]) for s in (1, 2)])
    lang, last = cfg["lang_ids"], cfg["vocab"] - 1
    ids = np.array([[cfg["sot"], lang[0], cfg["transcribe"], tb + 3, 10, 11, 12, tb + 28],
                    [cfg["sot"], lang[-1], cfg["transcribe"], tb, 400, 401, last, last]])
    oracle = wo.Oracle(cfg, weights, fp16=False)
    ours = oracle.forced_logits(oracle.encode(mel), ids).numpy()
    with torch.no_grad():
        hf = model(input_features=torch.from_numpy(mel), decoder_input_ids=torch.from_numpy(ids)).logits.numpy()
    assert ours.shape == hf.shape == (2, 8, cfg["vocab"])
    rms = float(np.sqrt(np.mean(hf.astype(np.float64) ** 2)))
    err = float(np.abs(ours - hf).max())
    print(f"model {which}: logit rms {rms:.4f}, max abs difference {err:.3e} ({err / rms:.3e} of the rms)")
    assert err <= 1e-4 * rms


@pytest.mark.parametrize("shift", [-4.0, 6.0])
def test_oracle_rule_masks_equal_the_hf_logits_processors(shift):
    transformers = pytest.importorskip("transformers")
    from transformers.generation.logits_process import (SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor,
                                                        WhisperTimeStampLogitsProcessor)

    cfg = wo.model_a_config()
    prompt = [cfg["sot"], 892, 897]
    gen = transformers.GenerationConfig(eos_token_id=cfg["eot"], bos_token_id=cfg["eot"])
    gen.no_timestamps_token_id = cfg["no_timestamps"]
    gen.max_initial_timestamp_index = cfg["max_initial_timestamp_index"]
    procs = [SuppressTokensLogitsProcessor(cfg["suppress"]), SuppressTokensAtBeginLogitsProcessor(cfg["begin_suppress"], len(prompt)),
             WhisperTimeStampLogitsProcessor(gen, begin_index=len(prompt))]
    for i, (name, prefix) in enumerate(wo.scripted_prefixes(cfg).items()):
        z = wo.scripted_logits(cfg, 100 + i, shift)
        scores = torch.from_numpy(z)[None].clone()
        ids = torch.tensor([prompt + prefix])
        for p in procs:
            scores = p(ids, scores)
        hf_mask = np.isneginf(scores[0].numpy())
        masked = wo.apply_rules(z, prefix, cfg)
        full = masked.copy()
        rule7 = wo.text_suppressed(masked, cfg)
        if rule7:
            full[:cfg["timestamp_begin"]] = -np.inf
        assert np.array_equal(np.isneginf(full), hf_mask), name
        assert wo.select(masked, cfg)[0] == int(np.argmax(scores[0].numpy())), name


def test_rule_7_goes_both_ways_on_the_scripted_cases():
    cfg = wo.model_a_config()
    outcomes = set()
    for shift in (-4.0, 6.0):
        for i, prefix in enumerate(wo.scripted_prefixes(cfg).values()):
            m = wo.apply_rules(wo.scripted_logits(cfg, 100 + i, shift), prefix, cfg)
            if np.isfinite(m[:cfg["timestamp_begin"]]).any() and np.isfinite(m[cfg["timestamp_begin"]:]).any():
                outcomes.add(wo.text_suppressed(m, cfg))
    assert outcomes == {True, False}


def test_select_breaks_ties_by_the_lower_id():
    cfg = wo.model_a_config()
    z = np.full(cfg["vocab"], -5.0)
    z[[40, 20, 30]] = 2.0
    tok, lp, margin = wo.select(wo.apply_rules(z, [cfg["timestamp_begin"] + 3, 10, 11], cfg), cfg)
    assert tok == 20 and margin == 0.0 and lp < 0


# ---- segment cutting and seek -----------------------------------------------------------------------------------------------
TB, EOT = 1000, 900


def _cut(tokens, start_ms=0, frames=3000):
    return transcribe.cut_window(tokens, EOT, TB, start_ms, frames)


def test_cut_window_ending_in_a_pair_seeks_to_the_pair():
    segs, adv = _cut([TB + 0, 5, 6, TB + 100, TB + 100, 7, TB + 250, TB + 250, EOT, EOT], start_ms=60000)
    assert segs == [(60000, 62000, [5, 6]), (62000, 65000, [7])]
    assert adv == 500  # timestamp 250 = 5.00 s = 500 frames


def test_cut_window_ending_in_a_single_timestamp_takes_the_whole_window():
    segs, adv = _cut([TB + 0, 5, TB + 100, TB + 100, 7, 8, TB + 400, EOT])
    assert segs == [(0, 2000, [5]), (2000, 8000, [7, 8])]
    assert adv == 3000


def test_cut_window_without_a_pair_is_one_segment_to_the_last_timestamp():
    segs, adv = _cut([TB + 10, 5, 6, 7, EOT], start_ms=1000)
    assert segs == [(1000, 1200, [5, 6, 7])] and adv == 3000
    segs, adv = _cut([TB + 0, 5, 6, 7], start_ms=1000, frames=1234)   # the only timestamp is <|0.00|>: up to the window's end
    assert segs == [(1000, 13340, [5, 6, 7])] and adv == 1234


def test_cut_window_with_only_eot_has_no_text():
    segs, adv = _cut([EOT, EOT, EOT], start_ms=30000)
    assert segs == [(30000, 60000, [])] and adv == 3000


def test_no_speech_rule():
    assert transcribe.skip_window(0.7, -12.0, 5)          # avg -2.0
    assert not transcribe.skip_window(0.7, -3.0, 5)       # avg -0.5: confident text survives
    assert not transcribe.skip_window(0.5, -12.0, 5)      # below the no-speech threshold
    assert not transcribe.skip_window(0.6, -12.0, 5)      # strictly greater


class _ScriptedTranscriber(transcribe.WhisperTranscriber):
    """The host loop of WhisperTranscriber over scripted decode results (no device)."""

    def __init__(self, script, dims, vocab):
        self.dims, self.script, self.calls = dims, list(script), []
        self.decoder = transcribe.ByteDecoder(vocab)
        self.window_frames = 2 * dims["max_source_positions"]
        self.sync_every = 8

    def set_audio(self, samples):
        pass

    def logmel(self, offsets, fetch=True):
        self.calls.append([int(o) for o in offsets])

    def encode(self, n, mel=None):
        pass

    def close(self):
        pass

    def decode(self, prompt, n_windows, max_new_tokens, sync_every=None):
        if max_new_tokens == 0:
            return {"lang": np.array([self.dims["lang_ids"][1]] * n_windows)}
        rows = [self.script.pop(0) for _ in range(n_windows)]
        toks = np.full((n_windows, max_new_tokens), self.dims["eot"], dtype=np.int32)
        for b, (t, _, _) in enumerate(rows):
            toks[b, :len(t)] = t
        return {"tokens": toks, "n": np.array([len(r[0]) + 1 for r in rows]), "lang": np.zeros(n_windows, dtype=np.int32),
                "sum_logprob": np.array([r[1] for r in rows], dtype=np.float32),
                "no_speech_prob": np.array([r[2] for r in rows], dtype=np.float32)}


def _dims():
    return {"max_source_positions": 1500, "max_target_positions": 448, "sot": 901, "eot": EOT, "transcribe": 950,
            "timestamp_begin": TB, "lang_ids": [910, 911], "lang_codes": ["en", "de"], "no_speech": 960}


VOCAB = {"Ġhello": 5, "Ġworld": 6, "Ġagain": 7, "!": 8}


def test_seek_mode_walks_the_audio_by_the_seek_rule_and_skips_silence():
    script = [([TB, 5, 6, TB + 500, TB + 500, 7, TB + 1000, TB + 1000], -2.0, 0.1),   # ends in a pair: seek to 20.00 s
              ([TB, 7], -20.0, 0.9),                                                    # skipped by the no-speech rule
              ([TB + 50, 8, TB + 200], -1.0, 0.9)]                                      # no-speech prob high but confident
    t = _ScriptedTranscriber(script, _dims(), VOCAB)
    out = t.transcribe(np.zeros(16000 * 70, dtype=np.float32), None)
    assert t.calls == [[0], [2000 * 160], [5000 * 160]]
    assert out["language"] == "de"
    assert [(s["start_ms"], s["end_ms"], s["text"]) for s in out["segments"]] == [
        (0, 10000, " hello world"), (10000, 20000, " again"), (50000, 54000, "!")]
    assert all(s["language"] == "de" and s["confidence"] is None and s["words"] is None for s in out["segments"])


def test_fixed_mode_batches_back_to_back_windows():
    script = [([TB, 5, TB + 100], -1.0, 0.0), ([TB + 10, 6, TB + 20, TB + 20], -1.0, 0.0), ([TB, 7, TB + 50], -1.0, 0.0)]
    t = _ScriptedTranscriber(script, _dims(), VOCAB)
    out = t.transcribe(np.zeros(16000 * 70, dtype=np.float32), "en", window_mode="fixed", batch_windows=2)
    assert t.calls == [[0, 3000 * 160], [6000 * 160]]
    assert [(s["start_ms"], s["end_ms"], s["text"]) for s in out["segments"]] == [
        (0, 2000, " hello"), (30200, 30400, " world"), (60000, 61000, " again")]
    with pytest.raises(ValueError):
        t.transcribe(np.zeros(16000, dtype=np.float32), "xx")


# ---- BPE decode ---------------------------------------------------------------------------------------------------------
def test_byte_level_bpe_decode_joins_a_character_split_across_tokens():
    # "é" is 0xC3 0xA9: GPT-2's table writes those bytes as "Ã" and "©"; " " as "Ġ"
    dec = transcribe.ByteDecoder({"Ġcaf": 0, "Ã": 1, "©": 2, "!": 3, "Ġ": 4})
    assert dec.decode([0, 1, 2, 3]) == " café!"
    assert dec.decode([0, 1]) == " caf�"            # a dangling lead byte is replaced, not an error
    assert dec.decode([999, 3]) == "!"                   # ids outside vocab.json (special tokens) decode to nothing
    assert len(transcribe._gpt2_byte_table()) == 256 and sorted(transcribe._gpt2_byte_table().values()) == list(range(256))


# ---- audio sources ------------------------------------------------------------------------------------------------------
def _write_wav(path, data, rate, channels):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(data, dtype="<i2").tobytes())


def test_default_audio_source_reads_wav_npy_and_the_sibling_wav(tmp_path):
    stereo = np.array([[16384, 0], [-16384, -16384], [32767, -32767]], dtype=np.int16)
    _write_wav(tmp_path / "clip.wav", stereo, 16000, 2)
    for name in ("clip.wav", "clip.mp4"):
        samples, rate = transcribe.default_audio_source(tmp_path / name)
        assert rate == 16000 and samples.dtype == np.float32
        np.testing.assert_allclose(samples, [0.25, -0.5, 0.0], atol=1e-7)
    np.save(tmp_path / "a.npy", np.array([0.5, -0.25], dtype=np.float64))
    samples, rate = transcribe.default_audio_source(tmp_path / "a.npy")
    assert rate == 16000 and samples.dtype == np.float32 and samples.tolist() == [0.5, -0.25]
    with pytest.raises(FileNotFoundError):
        transcribe.default_audio_source(tmp_path / "missing.mp4")


def test_wrong_sample_rate_and_sample_width_are_refused(tmp_path):
    _write_wav(tmp_path / "r.wav", np.zeros(10, dtype=np.int16), 44100, 1)
    with pytest.raises(ValueError, match="resampling is not built"):
        transcribe.transcribe_video(str(tmp_path / "r.wav"), {}, transcriber=None)
    with wave.open(str(tmp_path / "b.wav"), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(1)
        w.setframerate(16000)
        w.writeframes(bytes(10))
    with pytest.raises(ValueError, match="16-bit"):
        transcribe.read_wav(tmp_path / "b.wav")


def test_missing_checkpoint_files_fail_loudly(tmp_path):
    (tmp_path / "whisper" / "base").mkdir(parents=True)
    (tmp_path / "whisper" / "base" / "config.json").write_text("{}")
    with pytest.raises(FileNotFoundError, match="model.safetensors"):
        transcribe.WhisperTranscriber.from_cache(tmp_path, "base")


def test_safetensors_reader_and_dims(tmp_path):
    a = np.arange(6, dtype=np.float32).reshape(2, 3)
    b = np.array([1.5, -2.0], dtype=np.float16)
    header = {"a": {"dtype": "F32", "shape": [2, 3], "data_offsets": [0, 24]}, "b": {"dtype": "F16", "shape": [2], "data_offsets": [24, 28]},
              "__metadata__": {"format": "pt"}}
    h = json.dumps(header).encode()
    (tmp_path / "m.safetensors").write_bytes(len(h).to_bytes(8, "little") + h + a.tobytes() + b.tobytes())
    out = transcribe.read_safetensors(tmp_path / "m.safetensors")
    assert out["a"].tolist() == a.tolist() and out["b"].tolist() == [1.5, -2.0] and out["b"].dtype == np.float32
    dims = transcribe.whisper_dims(
        {"d_model": 384, "encoder_attention_heads": 6, "decoder_attention_heads": 6, "encoder_layers": 4, "decoder_layers": 4,
         "encoder_ffn_dim": 1536, "decoder_ffn_dim": 1536, "vocab_size": 51865, "max_source_positions": 1500,
         "max_target_positions": 448, "num_mel_bins": 80, "decoder_start_token_id": 50258, "eos_token_id": 50257},
        {"no_timestamps_token_id": 50363, "lang_to_id": {"<|de|>": 50261, "<|en|>": 50259}, "task_to_id": {"transcribe": 50359},
         "suppress_tokens": [1, 2], "begin_suppress_tokens": [220, 50257], "max_initial_timestamp_index": 50})
    assert dims["timestamp_begin"] == 50364 and dims["no_speech"] == 50362 and dims["lang_codes"] == ["en", "de"]
    assert dims["lang_ids"] == [50259, 50261] and dims["sot"] == 50258 and dims["eot"] == 50257 and dims["transcribe"] == 50359


def test_whisper_dims_read_the_large_v3_layout_from_checkpoint_files(tmp_path):
    """config.json / generation_config.json written from model C: every id (each one above model B's), the 100 languages in id
    order, 128 mel bins and the unequal layer and ffn counts come back."""
    cfg = wo.model_c_config()
    write_checkpoint(tmp_path / "c", cfg)
    config, generation = (json.loads((tmp_path / "c" / f).read_text()) for f in ("config.json", "generation_config.json"))
    assert (config, generation) == checkpoint_json(cfg)
    generation["lang_to_id"] = dict(reversed(list(generation["lang_to_id"].items())))      # file order is not id order
    dims = transcribe.whisper_dims(config, generation)
    for key, want in cfg.items():
        if key != "translate":                                                             # the library has no use for it
            assert dims[key] == want, key
    assert len(dims["lang_ids"]) == len(dims["lang_codes"]) == 100 and dims["lang_ids"] == sorted(dims["lang_ids"])
    assert dims["lang_codes"][0] == "en" and dims["lang_codes"][99] == "l99" and dims["lang_ids"][99] == 50358
    assert (dims["n_mels"], dims["enc_layers"], dims["dec_layers"], dims["enc_ffn"], dims["dec_ffn"]) == (128, 2, 3, 1536, 768)
    assert (dims["sot"], dims["eot"], dims["transcribe"], dims["no_speech"], dims["no_timestamps"], dims["timestamp_begin"]) == (
        50258, 50257, 50360, 50363, 50364, 50365)
    assert dims["sot_prev"] == 50362 and dims["alignment_heads"] is None
    b = wo.model_b_config()
    assert all(dims[k] == b[k] + 1 for k in ("transcribe", "no_speech", "no_timestamps", "timestamp_begin"))


# ---- result dict and opt-in ---------------------------------------------------------------------------------------------
class _FakeTranscriber:
    def __init__(self):
        self.args = None
        self.closed = False

    def transcribe(self, samples, language, *, window_mode="seek", batch_windows=8):
        self.args = (len(samples), language, window_mode, batch_windows)
        return {"language": "en", "segments": [
            {"start_ms": 0, "end_ms": 1500, "text": " one", "language": "en", "confidence": None, "words": None, "tokens": [1]},
            {"start_ms": 1500, "end_ms": 4020, "text": " two", "language": "en", "confidence": None, "words": None, "tokens": [2]}]}

    def close(self):
        self.closed = True


def _manager(tmp_path, fake, **kw):
    return ModelManager(cache_dir=str(tmp_path), gpu_transcription=True, transcriber_factory=lambda cache, name: fake,
                        audio_source=lambda path: (np.zeros(32000, dtype=np.float32), 16000), **kw)


def test_default_model_manager_still_refuses_transcription(tmp_path):
    with pytest.raises(NotImplementedError):
        asyncio.run(ModelManager(cache_dir=str(tmp_path)).transcribe_video("v.mp4", {}))


def test_enabled_model_manager_returns_the_reference_dict(tmp_path):
    fake = _FakeTranscriber()
    out = asyncio.run(_manager(tmp_path, fake).transcribe_video("v.mp4", {"languages": ["en", "de"], "vad_filter": True,
                                                                          "window_mode": "fixed", "batch_windows": 4}))
    assert fake.args == (32000, "en", "fixed", 4) and fake.closed
    assert list(out) == ["segments"] and len(out["segments"]) == 2
    for seg in out["segments"]:
        assert set(seg) == {"start_ms", "end_ms", "text", "language", "confidence", "words"}
        assert type(seg["start_ms"]) is int and type(seg["end_ms"]) is int and isinstance(seg["text"], str)
        assert seg["confidence"] is None and seg["words"] is None and seg["language"] == "en"
    out = asyncio.run(_manager(tmp_path, fake).transcribe_video("v.mp4", {"languages": "de"}))
    assert fake.args == (32000, "de", "seek", 8)


def test_process_ml_task_transcription_is_opt_in(tmp_path, monkeypatch):
    monkeypatch.setenv("MODEL_CACHE_DIR", str(tmp_path))
    with pytest.raises(RuntimeError, match="outside the MI355X hot path"):
        asyncio.run(task_handler.process_ml_task({}, "t1", "transcription", "vid", "v.mp4", {}))
    fake, got, made = _FakeTranscriber(), [], []

    def factory(cache_dir, **kw):
        made.append(kw)
        return _manager(tmp_path, fake)

    ctx = {"gpu_transcription": True, "model_manager_factory": factory, "artifact_sink": got.extend}
    res = asyncio.run(task_handler.process_ml_task(ctx, "t2", "transcription", "vid", "v.mp4", {"languages": "en"}))
    assert made == [{"gpu_transcription": True}]
    assert res == {"task_id": "t2", "status": "completed", "artifact_count": 2}
    assert [e.artifact_type for e in got] == ["transcript.segment"] * 2
    assert [(e.span_start_ms, e.span_end_ms) for e in got] == [(0, 1500), (1500, 4020)]
    assert json.loads(got[1].payload_json)["text"] == " two"
