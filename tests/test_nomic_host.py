"""K27 on the host: the oracle against ``transformers.NomicBertModel``, the checkpoint layouts and config checks, the row orders
of the packed device weights, the task prefixes, and the mask rule.  No GPU."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nomic_oracle as no
from eioku_amd import embed, semantic


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def _rel(got, ref):
    """max |got - ref| as a fraction of the reference RMS"""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.sqrt(np.mean(ref ** 2)))


@pytest.mark.parametrize("name,cfg,lengths", [("NS", no.config_ns(), no.LENGTHS_NS), ("NW", no.config_nw(), no.LENGTHS_NW)])
def test_fp32_oracle_equals_transformers(name, cfg, lengths):
    """The installed ``NomicBertModel`` (eager attention) on the padded batch with its mask, against the oracle that runs each
    sequence alone: the last hidden state on live rows, the pooled unit vector and the Matryoshka vector at 64, each within 1e-4
    of the reference RMS.  Both sides are fp32, only the summation order differs.  Measured: DESIGN.md "K27"."""
    tr = pytest.importorskip("transformers")
    w = no.random_weights(cfg, 3)
    config = tr.NomicBertConfig(**{k: v for k, v in no.hf_config(cfg).items() if k != "model_type"})
    config._attn_implementation = "eager"
    model = tr.NomicBertModel(config).eval()
    res = model.load_state_dict(w, strict=False)
    assert not res.unexpected_keys and not res.missing_keys
    seqs = no.random_ids(cfg, lengths, 5)
    ids, mask = no.pad(seqs)
    with torch.no_grad():
        last = model(input_ids=torch.from_numpy(ids.astype(np.int64)), attention_mask=torch.from_numpy(mask.astype(np.int64))).last_hidden_state
    m = torch.from_numpy(mask).float()[..., None]
    mean = (last * m).sum(1) / m.sum(1)  # the model card's mean_pooling
    ref_unit = F.normalize(mean, dim=-1).numpy()
    ref_m64 = F.normalize(F.layer_norm(mean, (mean.shape[-1],))[:, :64], dim=-1).numpy()
    ref_hidden = torch.cat([last[b, :len(s)] for b, s in enumerate(seqs)]).numpy()
    o = no.Oracle(cfg, w, fp16=False)
    hidden, unit = o.encode(seqs)
    _, m64 = o.encode(seqs, 64)
    d = (_rel(hidden, ref_hidden), _rel(unit, ref_unit), _rel(m64, ref_m64))
    print(f"{name}: oracle vs transformers, of the reference rms: hidden {d[0]:.3e} unit {d[1]:.3e} matryoshka-64 {d[2]:.3e}")
    assert hidden.shape == (sum(lengths), cfg["hidden"]) and unit.shape == (len(lengths), cfg["hidden"]) and m64.shape == (len(lengths), 64)
    assert max(d) <= 1e-4


# ---- checkpoint layouts and configs ------------------------------------------------------------------------------------------
def test_both_checkpoint_layouts_load_to_the_same_tensors(tmp_path):
    cfg = no.config_ns()
    w = {k: v.numpy() for k, v in no.random_weights(cfg, 7).items()}
    native = embed.nomic_convert_state(w, cfg)
    assert list(native) == [n for n, _ in embed.nomic_tensor_table(cfg)] == list(w)
    orig = {k: np.asarray(v) for k, v in no.original_layout(no.random_weights(cfg, 7)).items()}
    assert "encoder.layers.1.attn.Wqkv.weight" in orig and "encoder.layers.0.mlp.fc12.weight" in orig and "emb_ln.bias" in orig
    assert orig["encoder.layers.1.attn.Wqkv.weight"].shape == (384, 128) and not any("q_proj" in k or "gate_proj" in k for k in orig)
    back = embed.nomic_convert_state(orig, cfg)
    assert list(back) == list(native) and all(np.array_equal(back[k], native[k]) for k in native)
    # fc11 is up, fc12 is gate
    assert np.array_equal(back["layers.0.mlp.up_proj.weight"], orig["encoder.layers.0.mlp.fc11.weight"])
    # through a file, with the prefix a *ForMaskedLM checkpoint carries
    from safetensors.numpy import save_file

    save_file({"nomic_bert." + k: np.ascontiguousarray(v) for k, v in orig.items()}, str(tmp_path / "model.safetensors"))
    disk = embed.nomic_load_state(tmp_path, cfg)
    assert all(np.array_equal(disk[k], native[k]) for k in native)
    with pytest.raises(KeyError, match="checkpoint has no layers.1.self_attn.o_proj.weight"):
        embed.nomic_convert_state({k: v for k, v in orig.items() if "layers.1.attn.out_proj" not in k}, cfg)
    with pytest.raises(ValueError, match="no Linear bias"):
        embed.nomic_convert_state(dict(w, **{"layers.0.self_attn.o_proj.bias": np.zeros(128, np.float32)}), cfg)


def test_config_json_forms_and_refusals(tmp_path):
    cfg = no.config_nw()
    assert embed.nomic_config(no.hf_config(cfg)) == cfg
    assert embed.nomic_config({"model_type": "nomic_bert"}) == embed.NOMIC_EMBED_TEXT_V1_5  # NomicBertConfig's defaults
    (tmp_path / "config.json").write_text(json.dumps(no.hf_config(no.config_ns())))
    assert embed.nomic_config(tmp_path) == no.config_ns()
    # the original remote-code keys, where they map one to one
    old = {"n_embd": 768, "n_layer": 12, "n_head": 12, "n_inner": 3072, "n_positions": 8192, "rotary_emb_base": 1000, "vocab_size": 30528,
           "layer_norm_epsilon": 1e-12, "type_vocab_size": 2, "qkv_proj_bias": False, "mlp_fc1_bias": False, "mlp_fc2_bias": False,
           "prenorm": False, "rotary_emb_interleaved": False, "rotary_emb_fraction": 1.0, "rotary_scaling_factor": None,
           "activation_function": "swiglu"}
    assert embed.nomic_config(old) == dict(embed.NOMIC_EMBED_TEXT_V1_5, max_pos=8192)
    for key, value in [("qkv_proj_bias", True), ("mlp_fc1_bias", True), ("mlp_fc2_bias", True), ("prenorm", True),
                       ("rotary_emb_interleaved", True), ("rotary_emb_fraction", 0.5), ("rotary_scaling_factor", 2.0),
                       ("rope_scaling", {"type": "linear", "factor": 2.0}), ("activation_function", "gelu"), ("hidden_act", "gelu")]:
        with pytest.raises(ValueError, match=key):
            embed.nomic_config(dict(old, **{key: value}))
    for rope in ({"rope_type": "dynamic", "rope_theta": 1000.0, "factor": 2.0}, {"rope_type": "default", "rope_theta": 1000.0, "factor": 2.0}):
        with pytest.raises(ValueError, match="plain RoPE only"):
            embed.nomic_config(dict(no.hf_config(cfg), rope_parameters=rope))


# ---- the row orders of the packed weights ----------------------------------------------------------------------------------------
def test_permuted_and_rotated_q_dot_k_equals_the_unpermuted_one():
    """What the GEMM epilogue does, in numpy: weights in the stored row order, the rotation on neighbouring pairs (2j, 2j + 1)
    with the angle of j, against rotate_half on the original order.  The scores must agree; so must the interleaved gate / up
    product with silu(gate) * up."""
    rng = np.random.default_rng(0)
    d, n = 128, 9
    order = no.rope_row_order(d)
    assert sorted(order.tolist()) == list(range(d))
    assert order[:6].tolist() == [0, 32, 1, 33, 2, 34] and order[64:68].tolist() == [64, 96, 65, 97] and order[63] == 63 and order[127] == 127
    h = rng.standard_normal((n, d))
    wq, wk = rng.standard_normal((d, d)), rng.standard_normal((d, d))
    cos, sin = (t.double().numpy() for t in no.rope_tables(no.config_ns(), n))
    ref = []
    for w in (wq, wk):
        x = torch.from_numpy((h @ w.T).reshape(n, 2, 64).transpose(1, 0, 2))
        ref.append(no.rotate(x, torch.from_numpy(cos), torch.from_numpy(sin)).numpy())
    s_ref = ref[0] @ ref[1].transpose(0, 2, 1)
    got = []
    for w in (wq, wk):
        y = (h @ w[order].T).reshape(n, 2, 32, 2).transpose(1, 0, 2, 3)  # head, row, j, (lo, hi)
        lo, hi = y[..., 0], y[..., 1]
        got.append(np.stack([lo * cos - hi * sin, hi * cos + lo * sin], -1).reshape(2, n, 64))
    assert np.abs(got[0] @ got[1].transpose(0, 2, 1) - s_ref).max() <= 1e-12 * np.abs(s_ref).max()
    # the stored q itself is the reference q in the stored order
    assert np.abs(got[0] - ref[0][:, :, order[:64]]).max() <= 1e-12
    gate, up = rng.standard_normal((32, d)), rng.standard_normal((32, d))
    y = h @ no.gate_up_interleave(gate, up).T
    g, u = y[:, 0::2], y[:, 1::2]
    want = F.silu(torch.from_numpy(h @ gate.T)).numpy() * (h @ up.T)
    assert np.abs(g / (1 + np.exp(-g)) * u - want).max() <= 1e-12


# ---- prefixes ----------------------------------------------------------------------------------------------------------------
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "search", "_", "query", "document", ":", "the", "lake", "clustering", "red", "car"]


class _Recorder:
    """stands in for an encoder: keeps the ids it was given"""
    cfg = {"hidden": 4}

    def encode_ids(self, ids, mask):
        self.ids, self.mask = ids.copy(), mask.copy()
        return np.tile(np.eye(1, 4, dtype=np.float32), (len(ids), 1))


def test_task_prefixes_reach_the_tokenizer(tmp_path):
    (tmp_path / "vocab.txt").write_text("\n".join(VOCAB) + "\n")
    tok = semantic.WordPieceTokenizer(tmp_path / "vocab.txt")
    v = {t: i for i, t in enumerate(VOCAB)}
    lake = [v["[CLS]"], v["the"], v["lake"], v["[SEP]"]]
    query = [v["[CLS]"], v["search"], v["_"], v["query"], v[":"], v["the"], v["lake"], v["[SEP]"]]
    ids, mask = tok.encode_batch(["search_query: the lake"])
    assert ids[0].tolist() == query and mask.all()
    enc = _Recorder()
    p = embed.NOMIC_PREFIXES
    assert p == no.PREFIXES
    gen = semantic.EmbeddingGenerator(enc, tok, document_prefix=p["document"], query_prefix=p["query"], clustering_prefix=p["clustering"])
    gen.generate_embedding("the lake")  # a single text is a query
    assert enc.ids[0].tolist() == query
    gen.generate_batch_embeddings(["the lake"])  # a batch is documents
    assert enc.ids[0].tolist() == [v["[CLS]"], v["search"], v["_"], v["document"], v[":"], v["the"], v["lake"], v["[SEP]"]]
    gen.generate_batch_embeddings(["the lake"], kind="query")
    assert enc.ids[0].tolist() == query
    assert gen.tokenize(["the lake"], "clustering")[0][0].tolist() == [v["[CLS]"], v["clustering"], v[":"], v["the"], v["lake"], v["[SEP]"]]
    with pytest.raises(ValueError, match="kind must be one of"):
        gen.generate_batch_embeddings(["the lake"], kind="classification")
    # the search engine embeds a query as a query and a transcript as documents
    class NoStore:  # the kNN behind a real store needs the GPU
        def index_segments(self, ids, emb, meta):
            return len(ids)

        def search(self, q, top_k, filters):
            return []

    engine = semantic.SemanticSearchEngine(gen, NoStore())
    assert engine.index_transcript("v", [{"text": "the lake", "start": 0.0, "end": 1.0}]) == 1
    assert enc.ids[0][3] == v["document"]
    assert engine.search("the lake") == [] and enc.ids[0].tolist() == query
    # empty prefixes: today's ids, whatever the kind
    plain = semantic.EmbeddingGenerator(enc, tok)
    for kind in ("document", "query", "clustering"):
        plain.generate_batch_embeddings(["the lake"], kind=kind)
        assert enc.ids[0].tolist() == lake
    plain.generate_embedding("the lake")
    assert enc.ids[0].tolist() == lake
    # the sequence limit of the generator is the tokenizer's truncation
    long = semantic.EmbeddingGenerator(enc, tok, max_seq_length=2048, document_prefix=p["document"])
    long.generate_batch_embeddings(["the lake " * 400])
    assert enc.ids.shape == (1, 6 + 800) and enc.ids[0, -2] == v["lake"]
    gen.generate_batch_embeddings(["the lake " * 400])
    assert enc.ids.shape == (1, 256)


# ---- the mask rule ---------------------------------------------------------------------------------------------------------------
def test_only_prefix_masks_are_accepted():
    assert embed.prefix_lengths(np.array([[1, 1, 0], [1, 0, 0], [1, 1, 1]], np.uint8)).tolist() == [2, 1, 3]
    assert embed.prefix_lengths(np.ones((2, 1), np.uint8)).tolist() == [1, 1]
    for bad in ([[1, 0, 1]], [[0, 1, 1]], [[1, 1, 1], [0, 0, 1]]):
        with pytest.raises(ValueError, match="prefix of ones"):
            embed.prefix_lengths(np.array(bad, np.uint8))
    t = torch.tensor([[1, 1, 0], [1, 0, 1]], dtype=torch.uint8)
    with pytest.raises(ValueError, match="prefix of ones"):
        embed.prefix_lengths(t)
