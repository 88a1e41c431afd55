"""Search & index layer of the semantic-video-search design, on the HIP encoder and index.

The reference specifies this layer but never built it (``.kiro/specs/semantic-video-search/design.md:1092-1133``:
Embedding Generator / Vector Store / Semantic Search Engine; ``tasks.md:297-325``: task 13 unchecked).  The three
classes below carry the interfaces that design names - ``generateEmbedding / generateBatchEmbeddings``,
``indexSegment / search / deleteByVideoId`` + "save/load index from file" (``tasks.md:306``), ``search(query, filters)
-> SearchResult`` - with Python spelling, over K8 (all-MiniLM-L6-v2 on ``libeioku_hip``) and K9 (flat L2 kNN; on unit
vectors L2^2 = 2 - 2 cos, so the ranking IS the cosine ranking the design asks for and ``relevance_score`` is the cosine).

Tokenisation stays on the host: WordPiece over the model's own ``vocab.txt`` with BERT's uncased normalisation, built
from the ``tokenizers`` library (no network: the vocabulary file ships with the checkpoint directory).
"""
from __future__ import annotations

import json
import logging
import struct
from dataclasses import asdict, dataclass
from datetime import datetime, timezone
from pathlib import Path

import numpy as np

logger = logging.getLogger(__name__)

MAGIC = b"EIOKUIDX1\n"


class WordPieceTokenizer:
    """``[CLS] wordpieces [SEP]`` ids + attention mask, as sentence-transformers feeds all-MiniLM-L6-v2
    (``BertTokenizer``: lower-case, strip accents, split punctuation / CJK, greedy longest-match WordPiece,
    ``[UNK]`` for words over 100 characters; truncation at ``max_seq_length`` 256 word pieces incl. the specials)."""

    def __init__(self, vocab_path: str | Path, lowercase: bool = True):
        from tokenizers import Tokenizer, normalizers, pre_tokenizers, processors
        from tokenizers.models import WordPiece

        vocab = {}
        with open(vocab_path, encoding="utf-8") as f:
            for i, line in enumerate(f):
                vocab[line.rstrip("\n")] = i
        for tok in ("[PAD]", "[UNK]", "[CLS]", "[SEP]"):
            if tok not in vocab:
                raise ValueError(f"{vocab_path}: vocabulary has no {tok}")
        self.vocab = vocab
        self.pad_id = vocab["[PAD]"]
        tk = Tokenizer(WordPiece(vocab, unk_token="[UNK]", max_input_chars_per_word=100))
        tk.normalizer = normalizers.BertNormalizer(clean_text=True, handle_chinese_chars=True, strip_accents=None,
                                                   lowercase=lowercase)
        tk.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
        tk.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", special_tokens=[("[CLS]", vocab["[CLS]"]),
                                                                                                 ("[SEP]", vocab["[SEP]"])])
        self._tk = tk

    def encode_batch(self, texts: list[str], max_seq_length: int = 256):
        """-> (ids int32 (B,S), mask uint8 (B,S)), padded to the longest sequence of the batch."""
        self._tk.enable_truncation(max_length=max_seq_length)
        enc = self._tk.encode_batch(list(texts))
        S = max((len(e.ids) for e in enc), default=2)
        ids = np.full((len(enc), S), self.pad_id, np.int32)
        mask = np.zeros((len(enc), S), np.uint8)
        for i, e in enumerate(enc):
            ids[i, :len(e.ids)] = e.ids
            mask[i, :len(e.ids)] = 1
        return ids, mask


class EmbeddingGenerator:
    """design.md 2.1: text -> unit vector.  ``encoder``: a loaded :class:`eioku_amd.embed.MiniLMEncoder` (K8, 384-d) or
    :class:`eioku_amd.embed.NomicEncoder` (K27).  ``document_prefix`` / ``query_prefix`` / ``clustering_prefix`` go in front of
    a text of that ``kind`` before it is tokenised (nomic-embed-text's task prefixes); empty prefixes change nothing."""

    def __init__(self, encoder, tokenizer: WordPieceTokenizer, max_seq_length: int = 256, batch_size: int = 512,
                 document_prefix: str = "", query_prefix: str = "", clustering_prefix: str = ""):
        self.encoder, self.tokenizer = encoder, tokenizer
        self.max_seq_length, self.batch_size = max_seq_length, batch_size
        self.prefixes = {"document": document_prefix, "query": query_prefix, "clustering": clustering_prefix}

    @classmethod
    def from_directory(cls, model_dir: str | Path, state=None, matryoshka_dim: int | None = 512, **kw):
        """``model_dir``: a model snapshot (``model.safetensors`` / ``pytorch_model.bin`` + ``vocab.txt``).  A ``config.json``
        whose ``model_type`` is ``nomic_bert`` builds nomic-embed-text: the model card's task prefixes, ``max_seq_length`` 2048
        (or the config's ``max_position_embeddings`` if smaller) and vectors cut to ``matryoshka_dim`` (512 fits
        ``IndexFlatL2``; ``None``, or a model no wider than that, keeps the full width).  Any other directory is
        all-MiniLM-L6-v2.  ``state``: weights to use instead of the directory's file."""
        from . import embed

        model_dir = Path(model_dir)
        tokenizer = WordPieceTokenizer(model_dir / "vocab.txt")
        config = json.loads((model_dir / "config.json").read_text(encoding="utf-8")) if (model_dir / "config.json").exists() else {}
        if config.get("model_type") == "nomic_bert":
            cfg = embed.nomic_config(config)
            if matryoshka_dim is not None and matryoshka_dim >= cfg["hidden"]:
                matryoshka_dim = None
            enc = embed.NomicEncoder(state if state is not None else embed.nomic_load_state(model_dir, cfg), cfg, tokenizer, matryoshka_dim)
            p = embed.NOMIC_PREFIXES
            kw = {"max_seq_length": min(2048, cfg["max_pos"]), "document_prefix": p["document"], "query_prefix": p["query"],
                  "clustering_prefix": p["clustering"], **kw}
            return cls(enc, tokenizer, **kw)
        return cls(embed.MiniLMEncoder(state if state is not None else embed.load_state(model_dir, embed.MINILM_L6_V2)), tokenizer, **kw)

    def tokenize(self, texts: list[str], kind: str = "document"):
        """-> (ids int32 (B,S), mask uint8 (B,S)) of ``prefix(kind) + text``, truncated at ``max_seq_length``"""
        if kind not in self.prefixes:
            raise ValueError(f"kind must be one of {sorted(self.prefixes)}, got {kind!r}")
        prefix = self.prefixes[kind]
        return self.tokenizer.encode_batch([prefix + t for t in texts] if prefix else texts, self.max_seq_length)

    def generate_batch_embeddings(self, texts: list[str], kind: str = "document") -> np.ndarray:
        out = []
        for lo in range(0, len(texts), self.batch_size):
            ids, mask = self.tokenize(texts[lo:lo + self.batch_size], kind)
            out.append(np.asarray(self.encoder.encode_ids(ids, mask)))
        H = self.encoder.cfg["hidden"]
        return np.concatenate(out) if out else np.zeros((0, H), np.float32)

    def generate_embedding(self, text: str, kind: str = "query") -> np.ndarray:
        return self.generate_batch_embeddings([text], kind)[0]


@dataclass
class SearchResult:
    """design.md 2.3 output format."""

    video_id: str
    segment_id: str
    start_time: float
    end_time: float
    relevance_score: float
    matched_text: str
    thumbnail_path: str | None = None


FILTER_KEYS = ("video_id", "created_from", "created_to", "min_duration", "max_duration", "start_time", "end_time")


def _epoch(value, end_of_day: bool = False) -> float:
    """ISO-8601 date / datetime string (or epoch seconds) -> epoch seconds; NaN when it cannot be read.  A naive value is
    UTC.  ``end_of_day``: a date without a time stands for its last instant (an inclusive upper bound covers the day)."""
    if value is None:
        return float("nan")
    if isinstance(value, (int, float)):
        return float(value)
    try:
        text = str(value).strip()
        dt = datetime.fromisoformat(text[:-1] + "+00:00" if text.endswith(("Z", "z")) else text)
    except ValueError:
        return float("nan")
    if dt.tzinfo is None:
        dt = dt.replace(tzinfo=timezone.utc)
    t = dt.timestamp()
    if end_of_day and len(text) <= 10:
        t += 86400.0 - 1e-3
    return t


def _number(value) -> float:
    try:
        return float(value)
    except (TypeError, ValueError):
        return float("nan")


class VectorStore:
    """design.md 2.2 + "single .index file per library" (design.md:37): embeddings and segment metadata.

    The authoritative copy lives on the host (fp32 rows + metadata, what the file holds) and is COMPACT: live rows only,
    in insertion order.  The HIP index over it is built lazily by the first search; from then on ``index_segment(s)``
    appends to it (``IndexFlatL2.add``) and ``delete_by_video_id`` takes rows out of it (``remove_ids``: device ids never
    shift), so the store keeps the device row of every host row.  When removed device rows outnumber the live ones the
    device index is dropped once and rebuilt compactly by the next search: a search streams dead rows too, and this
    policy keeps that within 2x of a compact index.  Indexing / deleting / persistence need no GPU before the first
    search.

    ``filters`` (all optional, combined with AND; a row whose metadata lacks a filtered key does not match):
    ``video_id`` (id or list of ids); ``created_from`` / ``created_to`` (ISO-8601 date or datetime strings, inclusive,
    against metadata ``file_created_at``); ``min_duration`` / ``max_duration`` (seconds, inclusive, against metadata
    ``video_duration``); ``start_time`` / ``end_time`` (seconds: the segment's own span overlaps ``[start_time,
    end_time]``).  Unknown keys are ignored with a logged warning.  The filter is evaluated on host columns, packed
    into one :class:`eioku_amd.search.RowSelector` and applied inside ONE ``search_many`` call on the GPU."""

    def __init__(self, d: int = 384, index_factory=None):
        self.d = d
        self._rows: list[np.ndarray] = []
        self._meta: list[dict] = []
        # host columns beside _meta (what filters are evaluated on)
        self._vid: list[int] = []          # video ordinal
        self._created: list[float] = []    # file_created_at, epoch seconds (NaN: absent)
        self._duration: list[float] = []   # video_duration, seconds (NaN: absent)
        self._span: list[tuple[float, float]] = []  # the segment's own start / end
        self._video_ord: dict = {}
        self._cols = None                  # numpy views of the columns, rebuilt after a change
        # device side
        self._index_factory = index_factory
        self._index = None
        self._dev_row: list[int] = []      # device row of every host row (valid while _index is not None)
        self._dev_removed = 0              # device rows taken out by remove_ids

    def __len__(self) -> int:
        return len(self._meta)

    def _append_host(self, segment_id: str, e: np.ndarray, metadata: dict) -> None:
        m = dict(metadata, segment_id=segment_id)
        self._rows.append(e)
        self._meta.append(m)
        self._vid.append(self._video_ord.setdefault(m.get("video_id"), len(self._video_ord)) if m.get("video_id") is not None else -1)
        self._created.append(_epoch(m.get("file_created_at")))
        self._duration.append(_number(m.get("video_duration")) if m.get("video_duration") is not None else float("nan"))
        self._span.append((_number(m.get("start_time")) if m.get("start_time") is not None else float("nan"),
                           _number(m.get("end_time")) if m.get("end_time") is not None else float("nan")))
        self._cols = None

    def index_segment(self, segment_id: str, embedding, metadata: dict) -> bool:
        return self.index_segments([segment_id], np.asarray(embedding, dtype=np.float32).reshape(1, -1), [metadata]) == 1

    def index_segments(self, segment_ids: list[str], embeddings, metadata: list[dict]) -> int:
        emb = np.asarray(embeddings, dtype=np.float32)
        emb = emb.reshape(len(segment_ids), -1) if len(segment_ids) else emb.reshape(0, self.d)
        if emb.shape[1] != self.d:
            raise ValueError(f"expected a {self.d}-d embedding, got {emb.shape[1]}")
        for s, e, m in zip(segment_ids, emb, metadata):
            self._append_host(s, e.copy(), m)
        if self._index is not None and len(segment_ids):  # one upload of the new rows; the rest of the index stays
            base = int(self._index.ntotal)
            self._index.add(np.ascontiguousarray(emb))
            self._dev_row.extend(range(base, base + len(segment_ids)))
        return len(segment_ids)

    def delete_by_video_id(self, video_id: str) -> bool:
        gone = [i for i, m in enumerate(self._meta) if m.get("video_id") == video_id]
        if not gone:
            return False
        if self._index is not None:
            self._index.remove_ids(np.asarray([self._dev_row[i] for i in gone], dtype=np.int64))
            self._dev_removed += len(gone)
        dead = set(gone)
        for name in ("_rows", "_meta", "_vid", "_created", "_duration", "_span") + (("_dev_row",) if self._index is not None else ()):
            col = getattr(self, name)
            setattr(self, name, [v for i, v in enumerate(col) if i not in dead])
        self._cols = None
        if self._index is not None and self._dev_removed > len(self._meta):
            self._drop_index()  # more dead rows than live ones: rebuild compactly at the next search
        return True

    def _drop_index(self):
        if self._index is not None:
            self._index.close()
            self._index = None
        self._dev_row = []
        self._dev_removed = 0

    def _ensure_index(self):
        if self._index is None:
            if self._index_factory is not None:
                self._index = self._index_factory(self.d)
            else:
                from .search import IndexFlatL2

                self._index = IndexFlatL2(self.d)
            self._index.add(self.matrix())
            self._dev_row = list(range(len(self._meta)))
            self._dev_removed = 0
        return self._index

    def device_to_host_rows(self) -> np.ndarray:
        """int64 ``[device rows]``: the host row of every device row, -1 for rows that were removed."""
        n_dev = len(self._dev_row) + self._dev_removed
        out = np.full(n_dev, -1, np.int64)
        out[np.asarray(self._dev_row, dtype=np.int64)] = np.arange(len(self._dev_row), dtype=np.int64)
        return out

    def matrix(self) -> np.ndarray:
        return np.stack(self._rows).astype(np.float32) if self._rows else np.zeros((0, self.d), np.float32)

    def _columns(self):
        if self._cols is None:
            span = np.asarray(self._span, dtype=np.float64).reshape(-1, 2)
            self._cols = (np.asarray(self._vid, dtype=np.int64), np.asarray(self._created, dtype=np.float64),
                          np.asarray(self._duration, dtype=np.float64), span[:, 0], span[:, 1])
        return self._cols

    def eligible_rows(self, filters: dict | None):
        """Boolean mask over the host rows that ``filters`` admits, or ``None`` when nothing is filtered."""
        if not filters:
            return None
        for key in filters:
            if key not in FILTER_KEYS:
                logger.warning("VectorStore.search: unknown filter key %r ignored (known: %s)", key, ", ".join(FILTER_KEYS))
        active = {k: v for k, v in filters.items() if k in FILTER_KEYS and v is not None}
        if not active:
            return None
        vid, created, duration, seg_start, seg_end = self._columns()
        ok = np.ones(len(self._meta), dtype=bool)
        with np.errstate(invalid="ignore"):  # NaN (absent metadata) compares false: the row does not match
            if "video_id" in active:
                v = active["video_id"]
                wanted = v if isinstance(v, (list, tuple, set)) else [v]
                ords = [self._video_ord[w] for w in wanted if w in self._video_ord]
                ok &= np.isin(vid, np.asarray(ords, dtype=np.int64))
            if "created_from" in active:
                ok &= created >= _epoch(active["created_from"])
            if "created_to" in active:
                ok &= created <= _epoch(active["created_to"], end_of_day=True)
            if "min_duration" in active:
                ok &= duration >= float(active["min_duration"])
            if "max_duration" in active:
                ok &= duration <= float(active["max_duration"])
            if "start_time" in active:
                ok &= seg_end >= float(active["start_time"])
            if "end_time" in active:
                ok &= seg_start <= float(active["end_time"])
        return ok

    def search(self, query_embedding, top_k: int = 10, filters: dict | None = None) -> list[tuple[float, dict]]:
        """``[(squared L2 distance, metadata)]`` ascending, up to ``top_k`` entries (any ``top_k``: rounds of 32 chained by
        ``IndexFlatL2.search_many``).  ``filters``: see the class; the matching rows become a row selector and the GPU
        returns the exact top-k of those rows in one ``search_many`` call, however narrow the filter is."""
        if top_k < 1:
            raise ValueError(f"top_k must be >= 1, got {top_k}")
        if not self._meta:
            return []
        ok = self.eligible_rows(filters)
        n_ok = len(self._meta) if ok is None else int(ok.sum())
        if n_ok == 0:
            return []
        index = self._ensure_index()
        q = np.asarray(query_embedding, dtype=np.float32).reshape(1, self.d)
        if ok is None:
            D, I = index.search_many(q, min(n_ok, top_k))
        else:
            from .search import RowSelector

            dev_rows = np.asarray(self._dev_row, dtype=np.int64)[ok]
            D, I = index.search_many(q, min(n_ok, top_k), sel=RowSelector.from_ids(dev_rows, int(index.ntotal)))
        host = self.device_to_host_rows() if self._dev_removed else None
        out = []
        for dist, i in zip(D[0], I[0]):
            if i < 0:
                break
            out.append((float(dist), self._meta[int(i) if host is None else int(host[int(i)])]))
        return out

    # ---- the .index file -----------------------------------------------------------------------------
    def save(self, path: str | Path) -> None:
        """``EIOKUIDX1\\n`` | u64 n | u32 d | u64 len(meta json) | n*d fp32 rows | metadata JSON (UTF-8)."""
        meta = json.dumps(self._meta, ensure_ascii=False).encode("utf-8")
        x = self.matrix()
        with open(path, "wb") as f:
            f.write(MAGIC)
            f.write(struct.pack("<QIQ", x.shape[0], self.d, len(meta)))
            f.write(np.ascontiguousarray(x).tobytes())
            f.write(meta)

    @classmethod
    def load(cls, path: str | Path) -> "VectorStore":
        with open(path, "rb") as f:
            if f.read(len(MAGIC)) != MAGIC:
                raise ValueError(f"{path}: not an eioku .index file")
            n, d, mlen = struct.unpack("<QIQ", f.read(20))
            x = np.frombuffer(f.read(n * d * 4), dtype=np.float32).reshape(n, d)
            meta = json.loads(f.read(mlen).decode("utf-8"))
        if len(meta) != n:
            raise ValueError(f"{path}: {n} rows but {len(meta)} metadata records")
        st = cls(d)
        for r, m in zip(x, meta):
            st._append_host(m.get("segment_id"), r.copy(), m)
        return st


class SemanticSearchEngine:
    """design.md 2.3: query text -> ranked SearchResults."""

    def __init__(self, generator: EmbeddingGenerator, store: VectorStore):
        self.generator, self.store = generator, store

    def index_transcript(self, video_id: str, segments: list[dict]) -> int:
        """``segments``: what ``transcribe_video`` returns (``model_manager.py:409-467``): dicts with ``text`` and
        ``start`` / ``end`` seconds (or ``start_ms`` / ``end_ms``); optional ``file_created_at`` / ``video_duration`` make
        the segment filterable by date and duration (see :class:`VectorStore`)."""
        texts = [s["text"] for s in segments]
        emb = self.generator.generate_batch_embeddings(texts)  # kind "document", the generator's default
        meta = []
        for i, s in enumerate(segments):
            start = s["start_ms"] / 1000.0 if "start_ms" in s else float(s.get("start", 0.0))
            end = s["end_ms"] / 1000.0 if "end_ms" in s else float(s.get("end", start))
            meta.append({"video_id": video_id, "start_time": start, "end_time": end, "text": s["text"],
                         "thumbnail_path": s.get("thumbnail_path")})
            for key in ("file_created_at", "video_duration"):
                if s.get(key) is not None:
                    meta[-1][key] = s[key]
        return self.store.index_segments([f"{video_id}_seg{i}" for i in range(len(segments))], emb, meta)

    def search(self, query: str, filters: dict | None = None, top_k: int = 10) -> list[SearchResult]:
        q = self.generator.generate_embedding(query, kind="query")
        return [SearchResult(m["video_id"], m["segment_id"], m["start_time"], m["end_time"], 1.0 - dist / 2.0, m["text"],
                             m.get("thumbnail_path")) for dist, m in self.store.search(q, top_k, filters)]

    def search_dicts(self, query: str, filters: dict | None = None, top_k: int = 10) -> list[dict]:
        return [asdict(r) for r in self.search(query, filters, top_k)]
