"""The launch sequence of every Whisper entry, as a count: `last_launches()` after each call against the closed form that
the layer structure gives.  A layer, a start or a select that is written twice and drifts apart shows up here as a count.

Model A of tests/whisper_oracle.py (d 128, 2 heads, 2 + 2 layers, ctx 100, 1003 ids: a tile tail and a vocabulary tail),
two windows of 2 s.  `sync_every = max_new` everywhere, so no early stop changes a count.
"""
import numpy as np
import pytest

import whisper_fallback_oracle as wf
import whisper_oracle as wo

pytestmark = pytest.mark.gpu

CFG = wo.model_a_config()
DL = CFG["dec_layers"]
# embedding, then per layer: LayerNorm + q / k / v GEMMs + attention + out-projection (6), LayerNorm + q + attention +
# out-projection (4), LayerNorm + fc1 + fc2 (3); the final LayerNorm
STEP = 1 + 13 * DL + 1
PAIR = 2                       # logits + select
NEW = 4
BOOST = 1.2                    # EOT and timestamp rows raised, as in test_whisper_gpu.py


def prefill(captured_heads: int = 0) -> int:
    """A step's launches plus k_kv_to_cache per layer, plus one k_attn_weights per captured alignment head."""
    return 1 + 14 * DL + captured_heads + 1


START = prefill() + (1 + PAIR) + 1   # prefill, no-speech (gather + info pair), gather of the last prompt position


@pytest.fixture(scope="module")
def dev(gpu):
    from eioku_amd.transcribe import WhisperTranscriber

    tb = CFG["timestamp_begin"]
    boost = {CFG["eot"]: BOOST, **{tb + i: BOOST for i in range(CFG["vocab"] - tb)}}
    weights = wo.random_weights(CFG, 5, boost)
    t = WhisperTranscriber(dict(CFG), {k: v.numpy() for k, v in weights.items()})
    frames = 2 * CFG["max_source_positions"]
    mel = np.stack([wo.log_mel(wf.audio(s, 2.0), 0, frames, CFG["n_mels"]) for s in (3, 5)])
    t.encode(2, mel)
    t.mel = mel
    yield t
    t.close()


PROMPT3 = [CFG["sot"], CFG["lang_ids"][0], CFG["transcribe"]]
PROMPT5 = [CFG["no_speech"] - 1, 11] + PROMPT3   # <|startofprev|>, one previous token, then the sot sequence at index 2


def test_decode_walks_the_prompt_and_selects_once_per_token(dev):
    dev.decode(PROMPT3, 2, NEW, sync_every=NEW)
    steps = len(PROMPT3) - 1 + NEW
    assert dev.last_launches() == (steps * STEP + PAIR + NEW * PAIR, steps)


def test_the_language_call_is_one_step_and_one_info_pair(dev):
    dev.decode([CFG["sot"]], 2, 0)
    assert dev.last_launches() == (STEP + PAIR, 1)


def test_a_one_token_prompt_merges_the_info_select_into_step_0(dev):
    dev.decode([CFG["sot"]], 2, 2, sync_every=2)
    assert dev.last_launches() == (2 * STEP + 2 * PAIR, 2)


def test_decode_beam(dev):
    dev.decode_beam(PROMPT3, 2, NEW, 2, sync_every=NEW)
    steps = len(PROMPT3) - 1 + NEW
    assert dev.last_launches() == (steps * STEP + PAIR + NEW * PAIR, steps)


@pytest.mark.parametrize("sampled", [False, True])
def test_decode_prompted(dev, sampled):
    kw = {"group": 2, "temperature": 1.0, "seeds": [[1, 2], [3, 4]]} if sampled else {}
    dev.decode_prompted([PROMPT5] * 2, 2, NEW, sync_every=NEW, **kw)
    assert dev.last_launches() == (START + (NEW - 1) * STEP + NEW * PAIR, NEW - 1)


def test_decode_beam_prompted(dev):
    dev.decode_beam_prompted([PROMPT5] * 2, 2, NEW, 2, sync_every=NEW)
    assert dev.last_launches() == (START + (NEW - 1) * STEP + NEW * PAIR, NEW - 1)


def test_prefill_logits(dev):
    ids = np.asarray([PROMPT5, PROMPT5[:3] + [20, 21]], dtype=np.int32)
    dev.prefill_logits(ids, 3)
    # the per-row logits of the prefilled positions are not counted; the two walked positions are a step + logits each
    assert dev.last_launches() == (prefill() + 2 * (STEP + 1), 0)


def test_align(dev):
    seq = PROMPT3 + [CFG["no_timestamps"], 20, 21, 22, CFG["eot"]]
    dev.align([seq], [len(seq)], len(PROMPT3), [2 * CFG["max_source_positions"]], windows=[0])
    # the default heads: every head of the upper half of the decoder layers = 1 layer x 2 heads; then the token logits and
    # probabilities (2), the cost (2) and the DTW (1)
    captured = (DL - DL // 2) * CFG["heads"]
    assert dev.last_launches() == (prefill(captured) + 2 + 2 + 1, 0)


def test_encode_counts_the_same_flops_twice(dev):
    dev.encode(2, dev.mel)
    first = dev.last_flops()
    dev.encode(2, dev.mel)
    assert first > 0 and dev.last_flops() == first
