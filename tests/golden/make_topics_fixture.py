"""Regenerate tests/golden/topics_vectorizer.json: scikit-learn's CountVectorizer on awkward transcript texts.

    python tests/golden/make_topics_fixture.py

Each case is a list of texts and an ngram_range; the fixture holds scikit-learn's sorted vocabulary and the count matrix
as CSR (row_ptr, cand = term ids ascending per row, counts), or "empty": true where scikit-learn refuses an empty
vocabulary.  It lets a machine without scikit-learn check ``eioku_amd.topics.vectorize``.
"""
import json
from pathlib import Path

import sklearn
from sklearn.feature_extraction.text import CountVectorizer

TEXTS = [
    "The café's résumé was naïve, wasn't it?",
    "Don't stop believin' -- it's rock'n'roll",
    "Call 911 or 1-800-555-0199 before 2024; x1 y2 z 3d",
    "東京 タワー and 北京 are CJK words: 東京タワー",
    "",
    "   ",
    "the and of to in is it that",
    "and then there were none, yet nobody else",
    "Machine learning, MACHINE Learning, machine-learning!",
    "GPU kernels on the MI355X: HIP, gfx950, wave64",
    "naïve NAÏVE naive Naive",
    "ﬁnancial ligatures and Straße ß",
    "a_b snake_case __dunder__ _x x_",
    "one two three four five six seven eight",
    "neural network neural network neural",
    "Über über ÜBER",
    "emoji 😀 between words 🚀 rocket",
    "tab\tseparated\nnew\nlines\r\nhere",
    "it's its it is",
    "x y z a b c",
]
CASES = [(TEXTS, (1, 1)), (TEXTS, (1, 2)), (TEXTS, (2, 3)), (TEXTS, (1, 3)),
         (["", "   "], (1, 1)), (["the and of", "is it"], (1, 2)), (["single"], (2, 3)),
         (["only one bigram here"], (2, 2))]


def main():
    out = {"_source": f"scikit-learn {sklearn.__version__} CountVectorizer(ngram_range, stop_words='english', lowercase=True)",
           "cases": []}
    for texts, rng in CASES:
        case = {"texts": texts, "ngram_range": list(rng)}
        cv = CountVectorizer(ngram_range=rng, stop_words="english", lowercase=True)
        try:
            X = cv.fit_transform(texts).tocsr()
        except ValueError:
            case["empty"] = True
        else:
            X.sort_indices()
            case.update(vocabulary=list(cv.get_feature_names_out()), row_ptr=X.indptr.tolist(), cand=X.indices.tolist(),
                        counts=X.data.tolist())
        out["cases"].append(case)
    path = Path(__file__).resolve().parent / "topics_vectorizer.json"
    path.write_text(json.dumps(out, ensure_ascii=False) + "\n", encoding="utf-8")
    print(f"wrote {path} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
