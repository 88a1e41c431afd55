"""topic_extraction cost per video on one GPU, one JSON object per n-gram range: a synthetic one-hour transcript (720
segments of ~30 words drawn by a Zipf law over a generated 30,522-entry vocab.txt whose most frequent ranks are the
English stop words), random-init all-MiniLM-L6-v2.

For ``[1, 1]`` and ``[1, 2]`` it prints the host vectorizer time, the K8 segment and term embedding times with their token
counts, the time of each K17 call (segment rows, video row, keyword rows) and the wall time of ``TopicExtractor.extract``.

    python tools/topics_bench.py [--reps 3]
"""
import argparse
import json
import string
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def make_vocab(path: Path, size: int, seed: int) -> list[str]:
    """[PAD] [unused0] [UNK] [CLS] [SEP] [MASK], the stop words, then distinct lower-case words of 3-9 letters."""
    from eioku_amd import topics

    rng = np.random.default_rng(seed)
    words = sorted(topics.english_stop_words())
    seen = set(words)
    letters = np.array(list(string.ascii_lowercase))
    while len(words) < size - 6:
        w = "".join(rng.choice(letters, int(rng.integers(3, 10))))
        if w not in seen:
            seen.add(w)
            words.append(w)
    path.write_text("\n".join(["[PAD]", "[unused0]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words) + "\n", encoding="utf-8")
    return words


def transcript(words: list[str], n_seg: int, seed: int) -> list[dict]:
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, len(words) + 1) ** 1.07
    p /= p.sum()
    segs = []
    for i in range(n_seg):
        k = int(rng.integers(24, 37))
        segs.append({"text": " ".join(np.asarray(words)[rng.choice(len(words), k, p=p)]), "start_ms": 5000 * i,
                     "end_ms": 5000 * (i + 1)})
    return segs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--segments", type=int, default=720)
    args = ap.parse_args()
    import torch

    from eioku_amd import _lib, embed, semantic, topics

    _lib.init()
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as tmp:
        vocab_path = Path(tmp) / "vocab.txt"
        words = make_vocab(vocab_path, embed.MINILM_L6_V2["vocab"], 1)
        gen = semantic.EmbeddingGenerator(embed.MiniLMEncoder(embed.random_state(embed.MINILM_L6_V2, 11)),
                                          semantic.WordPieceTokenizer(vocab_path))
    segs = transcript(words, args.segments, 2)
    texts = [s["text"] for s in segs]
    ext = topics.TopicExtractor(gen)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t) * 1e3

    for ngr in ([1, 1], [1, 2]):
        conf = {"keyphrase_ngram_range": ngr}
        ext.extract(segs, conf)  # warm-up: workspaces, tokenizer
        best: dict = {}
        for _ in range(args.reps):
            vocab, t_vec = timed(lambda: topics.vectorize(texts, tuple(ngr)))
            V = len(vocab.terms)
            ids, mask = gen.tokenizer.encode_batch(texts, gen.max_seq_length)
            D, t_seg = timed(lambda: ext.embed_segments(texts, dev))
            (W, calls), t_term = timed(lambda: ext.embed_terms(vocab.terms, dev))
            c = D.sum(0, keepdim=True)
            c = (c / torch.linalg.vector_norm(c)).contiguous()
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
            rp, cd, allv = up(vocab.row_ptr), up(vocab.cand), up(np.arange(V))
            _, t_k_seg = timed(lambda: topics.keyword_select(D, W, rp, cd, 5, None))
            vid, t_k_vid = timed(lambda: topics.keyword_select(c, W, up([0, V]), allv, 10, 0.5))
            labels = vid[0][0, :int(vid[2][0])].cpu().numpy().astype(np.int64)
            others = up(np.concatenate([np.delete(np.arange(V), l) for l in labels]))
            X = W[torch.from_numpy(labels).to(dev)].contiguous()
            krp = up(np.arange(len(labels) + 1) * (V - 1))
            _, t_k_kw = timed(lambda: topics.keyword_select(X, W, krp, others, 5, None))
            _, t_total = timed(lambda: ext.extract(segs, conf))
            row = {"vectorize_ms": t_vec, "k8_segments_ms": t_seg, "k8_terms_ms": t_term, "k17_segment_rows_ms": t_k_seg,
                   "k17_video_row_ms": t_k_vid, "k17_keyword_rows_ms": t_k_kw, "extract_total_ms": t_total}
            for k, v in row.items():
                best[k] = min(best.get(k, v), v)
        k17 = best["k17_segment_rows_ms"] + best["k17_video_row_ms"] + best["k17_keyword_rows_ms"]
        print(json.dumps({"ngram_range": ngr, "segments": len(segs), "vocabulary": V, "segment_tokens": int(mask.sum()),
                          "segment_padded_tokens": int(mask.size), "term_tokens": sum(t for _, t in calls),
                          "term_k8_calls": len(calls), "nnz": int(vocab.cand.size), "reps": args.reps,
                          **{k: round(v, 3) for k, v in best.items()}, "k17_share_of_total": round(k17 / best["extract_total_ms"], 4)}),
              flush=True)


if __name__ == "__main__":
    main()
