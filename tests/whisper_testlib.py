"""Helpers the Whisper test files share: the checkpoint writer and the teacher-forced recomputation of a hypothesis's sum of
log-probabilities.  Nothing here imports the product at module level."""
from __future__ import annotations

import json

import numpy as np

import whisper_oracle as wo


def checkpoint_json(cfg: dict) -> tuple[dict, dict]:
    """(config.json, generation_config.json) of a test model, in the Hugging Face ``openai/whisper-*`` layout."""
    config = {
        "d_model": cfg["d_model"], "encoder_attention_heads": cfg["heads"], "decoder_attention_heads": cfg["heads"],
        "encoder_layers": cfg["enc_layers"], "decoder_layers": cfg["dec_layers"], "encoder_ffn_dim": cfg["enc_ffn"],
        "decoder_ffn_dim": cfg["dec_ffn"], "vocab_size": cfg["vocab"], "num_mel_bins": cfg["n_mels"],
        "max_source_positions": cfg["max_source_positions"], "max_target_positions": cfg["max_target_positions"],
        "decoder_start_token_id": cfg["sot"], "eos_token_id": cfg["eot"]}
    generation = {
        "no_timestamps_token_id": cfg["no_timestamps"], "no_speech_token_id": cfg["no_speech"],
        "lang_to_id": {f"<|{c}|>": i for c, i in zip(cfg["lang_codes"], cfg["lang_ids"])},
        "task_to_id": {"transcribe": cfg["transcribe"], "translate": cfg["translate"]}, "suppress_tokens": cfg["suppress"],
        "begin_suppress_tokens": cfg["begin_suppress"], "max_initial_timestamp_index": cfg["max_initial_timestamp_index"]}
    return config, generation


def write_checkpoint(root, cfg, weights=None):
    """``config.json``, ``generation_config.json``, ``vocab.json`` and, with ``weights``, an fp32 ``model.safetensors``."""
    root.mkdir(parents=True)
    config, generation = checkpoint_json(cfg)
    (root / "config.json").write_text(json.dumps(config))
    (root / "generation_config.json").write_text(json.dumps(generation))
    (root / "vocab.json").write_text(json.dumps({f"Ġw{i}": i for i in range(cfg["eot"])}))
    if weights is None:
        return
    header, blobs, off = {}, [], 0
    for k, v in weights.items():
        raw = v.numpy().astype("<f4").tobytes()
        header[k] = {"dtype": "F32", "shape": list(v.shape), "data_offsets": [off, off + len(raw)]}
        blobs.append(raw)
        off += len(raw)
    h = json.dumps(header).encode()
    (root / "model.safetensors").write_bytes(len(h).to_bytes(8, "little") + h + b"".join(blobs))


def forced_rows(m, rows) -> np.ndarray:
    """ids [rows][T] that teacher-force prompt + tokens of every row (EOT-padded to the longest)."""
    P = len(m.prompt)
    T = P + max(len(t) for _, t in rows) - 1
    ids = np.full((len(rows), T), m.cfg["eot"], dtype=np.int32)
    for r, (_, toks) in enumerate(rows):
        ids[r, :P + len(toks) - 1] = (m.prompt + list(toks))[:-1]
    return ids


def sums_from_logits(m, logits, rows) -> list[float]:
    """The sum of the rows' token log-probabilities under the oracle's rules and log-softmax in float64, from teacher-forced
    logits [rows][T][vocab] of ``forced_rows``."""
    cfg, P = m.cfg, len(m.prompt)
    logits = np.asarray(logits, dtype=np.float64)
    sums = []
    for r, (_, toks) in enumerate(rows):
        total = 0.0
        for i, t in enumerate(toks):
            z = wo.apply_rules(logits[r, P - 1 + i], list(toks[:i]), cfg)
            if wo.text_suppressed(z, cfg):
                z[:cfg["timestamp_begin"]] = -np.inf
            total += z[t] - wo._lse(z)
        sums.append(total)
    return sums


def recomputed_sums(m, mel, rows):
    """rows: [(window, tokens sampled incl. a closing EOT)].  Teacher-forces prompt + tokens on the device (``m.dev``, with
    ``m.cfg`` and ``m.prompt``) and sums the log-probabilities of the tokens under the oracle's rules and log-softmax in
    float64."""
    m.dev.encode(len(rows), mel[[b for b, _ in rows]])
    return sums_from_logits(m, m.dev.forced_logits(forced_rows(m, rows)), rows)
