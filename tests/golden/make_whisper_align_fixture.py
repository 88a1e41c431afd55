"""Writes tests/golden/whisper_align_hf.json: what the installed ``transformers`` computes for the pieces of Whisper's word
alignment that tests/whisper_align_oracle.py and eioku_amd/transcribe.py restate - ``_median_filter``,
``_dynamic_time_warping``, ``_split_tokens_on_unicode``, ``_split_tokens_on_spaces`` and ``_merge_punctuations`` - on small
inputs.  Run on a CPU:  python tests/golden/make_whisper_align_fixture.py.  The test that reads the file
(tests/test_transcribe_words_host.py) needs no ``transformers``.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch
from transformers.models.whisper.generation_whisper import _dynamic_time_warping, _median_filter
from transformers.models.whisper.tokenization_whisper import _merge_punctuations, _split_tokens_on_spaces, _split_tokens_on_unicode

OUT = Path(__file__).resolve().parent / "whisper_align_hf.json"
PREPEND = "\"'“¿([{-"
APPEND = "\"'.。,，!！?？:：”)]}、"
NO_SPACE = ("zh", "ja", "th", "lo", "my", "yue")

# a hand-made byte-level vocabulary: id -> the bytes it stands for.  é (c3 a9) and 中 (e4 b8 ad) are split across two ids.
EOT = 30
VOCAB = {0: b" Hello", 1: b",", 2: b" world", 3: b"!", 4: b" (", 5: b"a", 6: b"side", 7: b")", 8: b" caf", 9: b"\xc3", 10: b"\xa9",
         11: b" \"", 12: b"quoted", 13: b"\"", 14: b" -", 15: b"dash", 16: b".", 17: b"\xe4\xb8", 18: b"\xad",
         19: "文".encode(), 20: b" ", 21: b"'s", 22: b" it", 23: b"?", 24: " ¿".encode(), 25: "Qué".encode(),
         26: "。".encode(), 27: b" so", 28: b"-", 29: b"so"}
SPLIT_CASES = [
    ("en", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 16, 11, 12, 13, 14, 15, 22, 21, 23], True),
    ("es", [24, 25, 23, 0, 27, 28, 29, 16], True),
    ("ja", [17, 18, 19, 26, 0, 17, 18], True),
    ("en", [9, 10, 0, 1, 20, 2], True),
    ("en", [0, 31, 2, 16], False),          # a special id opens a word of its own (split only)
]


class Tokenizer:
    """What the split functions ask of a tokenizer: ``decode`` and ``eos_token_id``.  Special ids decode to nothing."""

    eos_token_id = EOT

    def decode(self, tokens, decode_with_timestamps=True):
        return b"".join(VOCAB.get(int(t), b"") for t in tokens).decode("utf-8", errors="replace")


def f32(a) -> list:
    return [float(v) for v in np.asarray(a, dtype=np.float32).reshape(-1)]


def main() -> None:
    rng = np.random.default_rng(21)
    median = []
    for shape in ((2, 3, 1), (2, 3, 3), (1, 4, 4), (2, 5, 7), (3, 2, 12), (1, 1, 50)):
        x = rng.standard_normal(shape).astype(np.float32)
        if shape[-1] == 12:
            x = np.round(x)                                           # repeated values inside a window
        y = _median_filter(torch.from_numpy(x)[None], 7)[0].numpy()
        median.append({"shape": list(shape), "x": f32(x), "y": f32(y)})
    dtw = []
    for name, n, f in (("random", 5, 9), ("random", 12, 20), ("random", 1, 1), ("random", 1, 6), ("random", 6, 1), ("random", 4, 3),
                       ("random", 9, 4), ("zeros", 5, 7), ("zeros", 1, 1), ("zeros", 3, 3), ("levels", 8, 11), ("levels", 7, 3),
                       ("levels", 1, 5), ("levels", 6, 1), ("levels", 20, 33)):
        if name == "random":
            c = rng.standard_normal((n, f)).astype(np.float32)
        elif name == "zeros":
            c = np.zeros((n, f), dtype=np.float32)
        else:
            c = rng.integers(-1, 2, size=(n, f)).astype(np.float32)   # three levels: ties everywhere
        ti, fi = _dynamic_time_warping(c)
        dtw.append({"name": name, "N": n, "F": f, "cost": f32(c), "text_idx": [int(v) for v in ti], "time_idx": [int(v) for v in fi]})
    tok, split = Tokenizer(), []
    for lang, ids, merge in SPLIT_CASES:
        uw, ut, _ = _split_tokens_on_unicode(tok, list(ids))
        if lang in NO_SPACE:
            w, t, ix = uw, ut, [[0]] * len(uw)
        else:
            w, t, ix = _split_tokens_on_spaces(tok, list(ids))
        case = {"language": lang, "ids": ids, "unicode": {"words": uw, "tokens": ut}, "split": {"words": list(w), "tokens": [list(g) for g in t]}}
        if merge:
            w, t, ix = list(w), [list(g) for g in t], [list(g) for g in ix]
            _merge_punctuations(w, t, ix, PREPEND, APPEND)
            case["merged"] = {"words": w, "tokens": t}
        split.append(case)
    OUT.write_text(json.dumps({"filter_width": 7, "median": median, "dtw": dtw, "eot": EOT, "prepend": PREPEND, "append": APPEND,
                               "vocab": {str(i): b.hex() for i, b in VOCAB.items()}, "split": split}, ensure_ascii=False, indent=1) + "\n")
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
