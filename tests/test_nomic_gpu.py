"""K27 on the device against tests/nomic_oracle.py (the CPU oracle; transformers is not needed here).

Configurations, the smallest at which each kernel can still go wrong:
  NS   vocab 300, hidden 128 (2 heads), ffn 256, 2 layers; lengths (1, 3, 17, 65, 130) in ONE packed call: a one-key softmax,
       either side of the 16- and 64-query edges, two 128-key LDS stages; sequences start at packed rows 1, 4, 21 and 86
  NW   the base width: hidden 768, 12 heads, ffn 3072, vocab 30528, 2 layers; lengths (197, 9)
  NL   hidden 128, 1 layer; lengths (2048, 5): rotary angles at far positions, 16 key stages
  N0   NS with zero layers: the embedding, its LayerNorm and the pooling alone
"""
import json

import numpy as np
import pytest
import torch

import nomic_oracle as no

pytestmark = pytest.mark.gpu


def _device(cfg, weights, **kw):
    from eioku_amd.embed import NomicEncoder

    return NomicEncoder({k: v.numpy() for k, v in weights.items()}, cfg, **kw)


class Model:
    """One test model: the device model, both oracles, and the results of all three on one seeded packed batch."""

    def __init__(self, cfg, lengths, seed):
        self.cfg, self.weights = cfg, no.random_weights(cfg, seed)
        self.dev = _device(cfg, self.weights)
        self.o32, self.o16 = no.Oracle(cfg, self.weights, False), no.Oracle(cfg, self.weights, True)
        self.seqs = no.random_ids(cfg, lengths, seed + 1)
        self.ids, self.cu = no.pack(self.seqs)
        h32 = [self.o32.hidden(s) for s in self.seqs]
        h16 = [self.o16.hidden(s) for s in self.seqs]
        self.h32, self.h16 = torch.cat(h32).numpy(), torch.cat(h16).numpy()
        self.u32, self.u16 = (torch.stack([no.Oracle.pool(h) for h in hs]).numpy() for hs in (h32, h16))
        self.m32, self.m16 = (torch.stack([no.Oracle.pool(h, 64) for h in hs]).numpy() for hs in (h32, h16))
        self.unit, self.hidden = self.dev.encode_packed(self.ids, self.cu, with_hidden=True)
        self.m64 = self.dev.encode_packed(self.ids, self.cu, matryoshka_dim=64)


@pytest.fixture(scope="module")
def model_ns(gpu):
    m = Model(no.config_ns(), no.LENGTHS_NS, 11)
    yield m
    m.dev.close()


def _drift(got, ref):
    """(mean, max) of |got - ref| as fractions of the reference RMS"""
    rms = float(np.sqrt(np.mean(np.square(ref, dtype=np.float64))))
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    return float(d.mean()) / rms, float(d.max()) / rms


def _check_drift(name, got, ref32, ref16):
    """The project's rule (tests/test_clip_gpu.py): the device may drift from the fp32 oracle by at most twice what the
    oracle's own fp16 mode does on the same input."""
    assert got.shape == ref32.shape and np.isfinite(got).all()
    bar_mean, bar_max = (2 * v for v in _drift(ref16, ref32))
    mean, mx = _drift(got, ref32)
    print(f"{name}: device drift mean {mean:.3e} max {mx:.3e} of the rms; bar (2 x CPU fp16 drift) mean {bar_mean:.3e} max {bar_max:.3e}")
    assert mean <= bar_mean and mx <= bar_max


def _check_unit(name, got, ref32, ref16):
    _check_drift(name, got, ref32, ref16)
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max() <= 1e-6


def _check_model(name, m):
    _check_drift(f"{name} hidden", m.hidden, m.h32, m.h16)
    _check_unit(f"{name} unit", m.unit, m.u32, m.u16)
    _check_unit(f"{name} matryoshka-64", m.m64, m.m32, m.m16)


# ---- 1. drift ------------------------------------------------------------------------------------------------------------------
def test_hidden_and_vector_drift_ns(model_ns):
    """Measured values: DESIGN.md "K27"."""
    assert model_ns.cu.tolist() == [0, 1, 4, 21, 86, 216] and model_ns.hidden.shape == (216, 128)
    assert model_ns.unit.shape == (5, 128) and model_ns.m64.shape == (5, 64)
    _check_model("NS", model_ns)


def test_hidden_and_vector_drift_nw(gpu):
    m = Model(no.config_nw(), no.LENGTHS_NW, 17)
    try:
        _check_model("NW", m)
    finally:
        m.dev.close()


def test_hidden_and_vector_drift_nl(gpu):
    m = Model(no.config_nl(), no.LENGTHS_NL, 19)
    try:
        assert m.hidden.shape == (2053, 128)
        _check_model("NL", m)
        # the far positions on their own: the last 64 rows of the long sequence
        _check_drift("NL hidden, positions 1984 ..", m.hidden[1984:2048], m.h32[1984:2048], m.h16[1984:2048])
    finally:
        m.dev.close()


def test_embedding_layernorm_and_pooling_alone_n0(gpu, model_ns):
    """Zero layers with NS's embedding weights: hidden_out is LayerNorm(word + type 0) and the vectors are its pooling.  Nothing
    in this path is fp16, so the oracle's fp16 mode equals its fp32 mode bit for bit and the 2 x rule would ask for a drift of
    exactly zero (asserted below, so this stays true).  The bar is therefore the one test_nomic_host.py holds two fp32
    evaluations of the same arithmetic to when only their summation order differs: 1e-4 of the reference RMS."""
    cfg = no.config_ns(layers=0)
    weights = {k: v for k, v in model_ns.weights.items() if not k.startswith("layers.")}
    dev = _device(cfg, weights)
    try:
        unit, hidden = dev.encode_packed(model_ns.ids, model_ns.cu, with_hidden=True)
        m64 = dev.encode_packed(model_ns.ids, model_ns.cu, matryoshka_dim=64)
        h32, u32 = no.Oracle(cfg, weights, False).encode(model_ns.seqs)
        h16, u16 = no.Oracle(cfg, weights, True).encode(model_ns.seqs)
        assert np.array_equal(h16, h32) and np.array_equal(u16, u32)
        _, m32 = no.Oracle(cfg, weights, False).encode(model_ns.seqs, 64)
        for name, got, ref in (("hidden", hidden, h32), ("unit", unit, u32), ("matryoshka-64", m64, m32)):
            mean, mx = _drift(got, ref)
            print(f"N0 {name}: device drift mean {mean:.3e} max {mx:.3e} of the rms; bar 1e-4 (fp32 against fp32)")
            assert got.shape == ref.shape and mx <= 1e-4
        for v in (unit, m64):
            assert np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    finally:
        dev.close()


# ---- 2. bit-for-bit identities ---------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_a_sequence_alone_equals_the_same_sequence_in_the_mixed_batch(model_ns):
    m = model_ns
    for b, s in enumerate(m.seqs):
        unit, hidden = m.dev.encode_packed(*no.pack([s]), with_hidden=True)
        assert np.array_equal(_bits(unit[0]), _bits(m.unit[b])), b
        assert np.array_equal(_bits(hidden), _bits(m.hidden[m.cu[b]:m.cu[b + 1]])), b
        m64 = m.dev.encode_packed(*no.pack([s]), matryoshka_dim=64)
        assert np.array_equal(_bits(m64[0]), _bits(m.m64[b])), b


def test_padded_rectangle_equals_packed_and_pad_ids_do_not_matter(gpu, model_ns):
    m = model_ns
    ids, mask = no.pad(m.seqs)
    assert ids.shape == (5, 130)
    assert np.array_equal(_bits(m.dev.encode_ids(ids, mask)), _bits(m.unit))
    noisy = np.where(mask == 0, np.random.default_rng(2).integers(1, 300, ids.shape), ids).astype(np.int32)
    assert not np.array_equal(noisy, ids)
    assert np.array_equal(_bits(m.dev.encode_ids(noisy, mask)), _bits(m.unit))
    # from the device: packed there, returned there
    got = m.dev.encode_ids(torch.from_numpy(noisy).to(gpu), torch.from_numpy(mask).to(gpu))
    assert got.is_cuda and np.array_equal(_bits(got.cpu().numpy()), _bits(m.unit))
    got = m.dev.encode_packed(torch.from_numpy(m.ids).to(gpu), torch.from_numpy(m.cu).to(gpu))
    assert got.is_cuda and np.array_equal(_bits(got.cpu().numpy()), _bits(m.unit))
    # SegmentBatcher takes the encoder as it takes K8's: rows added in two pieces, encoded as one batch
    from eioku_amd.embed import SegmentBatcher

    sb = SegmentBatcher(m.dev, 130, batch_segments=8, device=gpu)
    d_ids, d_mask = torch.from_numpy(ids).to(gpu), torch.from_numpy(mask).to(gpu)
    assert sb.add(d_ids[:2], d_mask[:2]) == [] and sb.add(d_ids[2:], d_mask[2:]) == []
    (got,) = sb.flush()
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(m.unit))
    bad = mask.copy()
    bad[4, 7] = 0
    with pytest.raises(ValueError, match="prefix of ones"):
        m.dev.encode_ids(ids, bad)
    with pytest.raises(ValueError, match="prefix of ones"):
        m.dev.encode_ids(torch.from_numpy(ids).to(gpu), torch.from_numpy(bad).to(gpu))


def test_reordering_the_batch_permutes_the_outputs(model_ns):
    m = model_ns
    order = [3, 0, 4, 2, 1]
    seqs = [m.seqs[i] for i in order]
    ids, cu = no.pack(seqs)
    unit, hidden = m.dev.encode_packed(ids, cu, with_hidden=True)
    for at, b in enumerate(order):
        assert np.array_equal(_bits(unit[at]), _bits(m.unit[b]))
        assert np.array_equal(_bits(hidden[cu[at]:cu[at + 1]]), _bits(m.hidden[m.cu[b]:m.cu[b + 1]]))
    assert m.dev.last_flops() > 0 and m.dev.last_ms() > 0


# ---- 3. retrieval end to end -------------------------------------------------------------------------------------------------------
RETRIEVAL_SEED = 61  # chosen on the CPU: gap 3.8e-3 against an fp16-oracle drift of 5.5e-5; the long text is the oracle's second, 24th at 256
WORDS = ("the a of and to in is it on for with as at by from this that be are was or an we you they he she not but all can had her one "
         "our out day get has him his how man new now old see two way who boy did its let put say too use red car lake blue tree "
         "house dog cat road river hill stone bird fish sun moon rain snow wind fire").split()
QUERY = "red car by the lake"
LATE = "red car lake"


def _retrieval_dir(root):
    """a snapshot directory without weights (they are seeded): config.json with model_type nomic_bert, and a vocab.txt"""
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "search", "_", "query", "document", "clustering", ":"] + sorted(set(WORDS))
    cfg = no.config_ns()
    cfg["vocab"] = len(vocab)
    root.mkdir(parents=True)
    (root / "config.json").write_text(json.dumps(no.hf_config(cfg)))
    (root / "vocab.txt").write_text("\n".join(vocab) + "\n")
    return cfg


def _retrieval_texts(seed=RETRIEVAL_SEED):
    """40 texts of 4 .. 40 seeded words; text 13 is long: 300 words without the query's nouns, then ``LATE`` 150 times, so its
    first 256 word pieces say nothing about what it is about"""
    rng = np.random.default_rng(seed)
    plain = [w for w in WORDS if w not in LATE.split()]
    texts = [" ".join(rng.choice(WORDS, rng.integers(4, 41))) for _ in range(40)]
    texts[13] = " ".join(rng.choice(plain, 300)) + " " + " ".join([LATE] * 150)
    return texts


def _oracle_cosines(o32, gen, texts, max_seq_length):
    """the fp32 oracle on the product's own token ids (pinned on the host): cosine of every text with the query"""
    ids, mask = gen.tokenizer.encode_batch([gen.prefixes["document"] + t for t in texts], max_seq_length)
    docs = o32.encode([row[:n] for row, n in zip(ids, mask.sum(1))], 64)[1]
    qi, qm = gen.tokenizer.encode_batch([gen.prefixes["query"] + QUERY], max_seq_length)
    return docs @ o32.encode([qi[0][:qm[0].sum()]], 64)[1][0], int(mask.sum(1).max())


def test_retrieval_end_to_end(gpu, tmp_path):
    """``from_directory`` on a nomic_bert snapshot -> ``SemanticSearchEngine``; 40 texts indexed, one of them 756 word pieces long
    with its distinguishing words after position 256; the query's top five are the fp32 oracle's.  The ranking is only
    meaningful while the oracle's six best cosines are further apart than the device may drift, so that is asserted, not
    assumed (the seed was chosen on the CPU so that it holds, with the oracle's fp16 mode standing in for the device)."""
    from eioku_amd import embed, semantic

    cfg = _retrieval_dir(tmp_path / "nomic")
    state = embed.nomic_random_state(cfg, RETRIEVAL_SEED)
    texts = _retrieval_texts()
    gen = semantic.EmbeddingGenerator.from_directory(tmp_path / "nomic", state=state, matryoshka_dim=64)
    try:
        assert isinstance(gen.encoder, embed.NomicEncoder) and gen.max_seq_length == 2048 and gen.encoder.cfg["hidden"] == 64
        assert gen.prefixes == {"document": "search_document: ", "query": "search_query: ", "clustering": "clustering: "}
        engine = semantic.SemanticSearchEngine(gen, semantic.VectorStore(d=64))
        assert engine.index_transcript("v", [{"text": t, "start": float(i), "end": i + 1.0} for i, t in enumerate(texts)]) == 40
        got = engine.search(QUERY, top_k=40)
        o32 = no.Oracle(cfg, state, False)
        cos32, longest = _oracle_cosines(o32, gen, texts, 2048)
        assert longest == 300 + 450 + 4 + 2  # the long text went through whole: words, the prefix's 4 pieces, [CLS] and [SEP]
        cos_dev = np.empty(40)
        for r in got:
            cos_dev[int(r.segment_id.removeprefix("v_seg"))] = r.relevance_score
        drift = float(np.abs(cos_dev - cos32).max())
        top6 = np.sort(cos32)[::-1][:6]
        gap = float(np.min(top6[:-1] - top6[1:]))
        print(f"retrieval: max cosine drift {drift:.3e}, smallest gap among the oracle's six best cosines {gap:.3e}; "
              f"device ms {gen.encoder.last_ms():.3f}")
        assert gap > 4 * drift
        order32 = np.argsort(-cos32, kind="stable")
        assert [int(r.segment_id.removeprefix("v_seg")) for r in got[:5]] == order32[:5].tolist()
        # the long text is found by its late words ...
        assert 13 in order32[:5].tolist()
        # ... which a 256-piece limit never sees: there the oracle ranks it outside the top five
        cos256, longest = _oracle_cosines(o32, gen, texts, 256)
        assert longest == 256 and 13 not in np.argsort(-cos256, kind="stable")[:5].tolist()
    finally:
        gen.encoder.close()


def test_topics_carry_the_clustering_prefix(gpu, tmp_path):
    """TopicExtractor on a nomic generator: segment texts and candidate terms are embedded as ``clustering: `` + text."""
    from eioku_amd import embed, semantic, topics

    cfg = _retrieval_dir(tmp_path / "nomic")
    gen = semantic.EmbeddingGenerator.from_directory(tmp_path / "nomic", state=embed.nomic_random_state(cfg, 3))
    try:
        assert gen.encoder.cfg["hidden"] == 128  # a model no wider than 512 keeps its width
        ext = topics.TopicExtractor(gen)
        emb, _ = ext.embed_terms(["lake", "red car"], gpu)
        want = gen.encoder.encode(["lake", "red car"], kind="clustering")
        assert np.array_equal(_bits(emb.cpu().numpy()), _bits(want))
        assert not np.array_equal(_bits(want), _bits(gen.encoder.encode(["lake", "red car"], kind="document")))
        res = ext.extract([{"text": "red car lake road", "start": 0.0, "end": 1.0}, {"text": "blue bird tree", "start": 1.0, "end": 2.0}])
        assert len(res["segment_keywords"]) == 2 and res["topics"]
    finally:
        gen.encoder.close()


# ---- 4. limits -------------------------------------------------------------------------------------------------------------------
def test_limits_and_handle_lifecycle(gpu, model_ns):
    from eioku_amd._handle import Handle
    from eioku_amd._lib import EiokuHipError

    def create(vocab=300, hidden=128, layers=1, heads=2, ffn=256, max_pos=2048, type_vocab=2, eps=1e-12, theta=1000.0):
        return Handle("nomic", vocab, hidden, layers, heads, ffn, max_pos, type_vocab, eps, theta)

    for kw, match in [({"heads": 4}, "head_dim must be 64"), ({"ffn": 100}, "intermediate_size must be a positive multiple of 32"),
                      ({"max_pos": 8193}, r"max_position_embeddings must be in \[1, 8192\]"), ({"theta": 0.0}, "bad config")]:
        with pytest.raises(EiokuHipError, match=match):
            create(**kw)
    h = create()
    names = [n for n, _, _ in h.tensors()]
    assert names == list(no.random_weights(no.config_ns(layers=1), 0))
    shapes = dict((n, (r, c)) for n, r, c in h.tensors())
    assert shapes["layers.0.self_attn.q_proj.weight"] == (128, 128) and shapes["layers.0.mlp.gate_proj.weight"] == (256, 128)
    ids, cu, vec = np.ones(4, np.int32), np.array([0, 4], np.int32), np.empty((1, 128), np.float32)
    rc = h.eioku_nomic_encode(ids.ctypes.data, cu.ctypes.data, 1, 0, vec.ctypes.data, None, 0, None)
    assert rc != 0 and b"has no weights" in h.lib.eioku_last_error()
    h.close()
    h.close()  # idempotent
    with pytest.raises(EiokuHipError, match="closed"):
        h.eioku_nomic_num_tensors()
    # a loaded model refuses what it cannot run, each with its own message, and clamps nothing
    dev = model_ns.dev
    for bad_ids, bad_cu, match in [(np.ones(3, np.int32), np.array([0, 0, 3], np.int32), "at least one token"),
                                   (np.array([1, 300, 2], np.int32), np.array([0, 3], np.int32), "outside the vocabulary of 300"),
                                   (np.array([1, -1, 2], np.int32), np.array([0, 3], np.int32), "outside the vocabulary of 300"),
                                   (np.ones(2049, np.int32), np.array([0, 2049], np.int32), "exceeds max_position_embeddings 2048")]:
        with pytest.raises(EiokuHipError, match=match):
            dev.encode_packed(bad_ids, bad_cu)
    with pytest.raises(EiokuHipError, match="matryoshka_dim must be in"):
        dev.encode_packed(np.ones(3, np.int32), np.array([0, 3], np.int32), matryoshka_dim=129)
    with pytest.raises(ValueError, match="matryoshka_dim must be in"):
        _device(model_ns.cfg, model_ns.weights, matryoshka_dim=129)
    assert dev.encode_packed(np.zeros(0, np.int32), np.zeros(1, np.int32)).shape == (0, 128)  # an empty batch is no error
    m = _device(no.config_ns(layers=0), {k: v for k, v in model_ns.weights.items() if not k.startswith("layers.")})
    m.close()
    m.close()
    with pytest.raises(EiokuHipError, match="closed"):
        m.encode_packed(np.ones(3, np.int32), np.array([0, 3], np.int32))
