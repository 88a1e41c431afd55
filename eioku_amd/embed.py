"""Segment-embedding stage: all-MiniLM-L6-v2 on the HIP encoder (``eioku_bert_t``), and nomic-embed-text on the packed
RoPE encoder (``eioku_nomic_t``, the second half of this file).

The reference planned this stage but never built it (``.kiro/specs/semantic-video-search/tasks.md:
297-302``); the surface mirrored here is sentence-transformers' ``SentenceTransformer.encode`` for
that model: WordPiece tokens -> BERT(6 x 384) -> attention-mask mean pooling -> L2 normalise.
PyTorch / safetensors are used only to read the checkpoint; tokenisation stays on the host.
"""

from __future__ import annotations

import ctypes as C
import json
from pathlib import Path

import numpy as np

from . import _lib
from ._buffers import current_stream, on_device, ptr
from ._handle import Handle

MINILM_L6_V2 = dict(vocab=30522, hidden=384, layers=6, heads=12, ffn=1536, max_pos=512, type_vocab=2, ln_eps=1e-12)


def tensor_table(cfg: dict) -> list[tuple[str, tuple[int, ...]]]:
    """(state-dict name, shape) of every tensor the encoder needs (Hugging Face ``BertModel`` names)."""
    H, F = cfg["hidden"], cfg["ffn"]
    t = [("embeddings.word_embeddings.weight", (cfg["vocab"], H)),
         ("embeddings.position_embeddings.weight", (cfg["max_pos"], H)),
         ("embeddings.token_type_embeddings.weight", (cfg["type_vocab"], H)),
         ("embeddings.LayerNorm.weight", (H,)), ("embeddings.LayerNorm.bias", (H,))]
    for l in range(cfg["layers"]):
        p = f"encoder.layer.{l}."
        t += [(p + "attention.self.query.weight", (H, H)), (p + "attention.self.key.weight", (H, H)),
              (p + "attention.self.value.weight", (H, H)), (p + "attention.self.query.bias", (H,)),
              (p + "attention.self.key.bias", (H,)), (p + "attention.self.value.bias", (H,)),
              (p + "attention.output.dense.weight", (H, H)), (p + "attention.output.dense.bias", (H,)),
              (p + "attention.output.LayerNorm.weight", (H,)), (p + "attention.output.LayerNorm.bias", (H,)),
              (p + "intermediate.dense.weight", (F, H)), (p + "intermediate.dense.bias", (F,)),
              (p + "output.dense.weight", (H, F)), (p + "output.dense.bias", (H,)),
              (p + "output.LayerNorm.weight", (H,)), (p + "output.LayerNorm.bias", (H,))]
    return t


def random_state(cfg: dict, seed: int) -> dict[str, np.ndarray]:
    """Random-init weights of the exact shapes (BERT init: N(0, 0.02^2) x a gain that keeps
    post-LayerNorm activations O(1); LayerNorm gamma ~ 1, beta ~ 0)."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in tensor_table(cfg):
        if name.endswith("LayerNorm.weight"):
            out[name] = (1.0 + 0.1 * rng.standard_normal(shape)).astype(np.float32)
        elif name.endswith(".bias"):
            out[name] = (0.02 * rng.standard_normal(shape)).astype(np.float32)
        elif "embeddings" in name:
            out[name] = (0.05 * rng.standard_normal(shape)).astype(np.float32)
        else:
            out[name] = (rng.standard_normal(shape) / np.sqrt(shape[1])).astype(np.float32)
    return out


def load_state(path: str | Path, cfg: dict) -> dict[str, np.ndarray]:
    """``model.safetensors`` / ``pytorch_model.bin`` of all-MiniLM-L6-v2 (keys with or without ``bert.``)."""
    path = Path(path)
    if path.is_dir():
        for cand in ("model.safetensors", "pytorch_model.bin"):
            if (path / cand).exists():
                path = path / cand
                break
    if not path.exists():
        raise FileNotFoundError(f"encoder weights not found: {path}")
    if path.suffix == ".safetensors":
        from safetensors.numpy import load_file

        raw = load_file(str(path))
    else:
        import torch

        raw = {k: v.float().numpy() for k, v in torch.load(str(path), map_location="cpu", weights_only=True).items()}
    raw = {k.removeprefix("bert.").removeprefix("0.auto_model."): v for k, v in raw.items()}
    out = {}
    for name, shape in tensor_table(cfg):
        if name not in raw:
            raise KeyError(f"checkpoint has no {name}")
        a = np.asarray(raw[name], dtype=np.float32)
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"{name}: shape {a.shape} != {shape}")
        out[name] = a
    return out


def routes(reset: bool = False) -> dict[str, int]:
    """Route log of the encoder: {route name: launches} in this process since the last reset, as counted by the launch
    code itself (``eioku_debug_bert_routes``).  Every known route is present, zeros included, e.g.
    ``{"attn_bf": 6, "attn8": 0, ..., "gemm_bf<EPI0,T64,AS1>": 18, ..., "splits<3>": 6}``."""
    buf = C.create_string_buffer(1 << 12)
    _lib.check(_lib.load().eioku_debug_bert_routes(buf, len(buf), int(reset)), "eioku_debug_bert_routes")
    out = {}
    for line in buf.value.decode().splitlines():
        name, count = line.rsplit(" ", 1)
        out[name] = int(count)
    return out


class MiniLMEncoder:
    """BERT sentence encoder resident on one GPU."""

    def __init__(self, state: dict[str, np.ndarray] | None = None, cfg: dict = MINILM_L6_V2, tokenizer=None):
        self.cfg, self.tokenizer = dict(cfg), tokenizer
        self._h = Handle("bert", cfg["vocab"], cfg["hidden"], cfg["layers"], cfg["heads"], cfg["ffn"], cfg["max_pos"],
                         cfg["type_vocab"], float(cfg["ln_eps"]))
        if state is not None:
            self._h.or_close(self.load_state, state)

    def load_state(self, state: dict[str, np.ndarray]) -> None:
        self._h.set_tensors(state)

    def encode_ids(self, ids, mask):
        """int32 ids / uint8 mask ``(B,S)`` -> float32 ``(B,hidden)`` unit vectors (numpy in -> numpy out)."""
        B, S = (int(s) for s in ids.shape)
        H = self.cfg["hidden"]
        dev = on_device(ids)
        if dev:
            import torch

            ids = ids.to(torch.int32).contiguous()
            mask = mask.to(torch.uint8).contiguous()
            out = torch.empty((B, H), dtype=torch.float32, device=ids.device)
        else:
            ids = np.ascontiguousarray(ids, dtype=np.int32)
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
            out = np.empty((B, H), dtype=np.float32)
        _lib.check(self._h.eioku_bert_embed(ptr(ids), ptr(mask), B, S, ptr(out),
                                            _lib.MEM_DEVICE if dev else _lib.MEM_HOST, current_stream(ids)),
                   "eioku_bert_embed")
        return out

    def encode(self, texts: list[str], max_seq_length: int = 256):
        """sentence-transformers style entry: needs a WordPiece tokenizer (``tokenizers.Tokenizer`` or HF fast
        tokenizer) supplied at construction - the vocabulary file is not part of this repository."""
        if self.tokenizer is None:
            raise RuntimeError("MiniLMEncoder.encode() needs a tokenizer (vocab.txt of all-MiniLM-L6-v2); "
                               "use encode_ids() with pre-tokenised input otherwise")
        if hasattr(self.tokenizer, "encode_batch"):  # eioku_amd.semantic.WordPieceTokenizer
            return self.encode_ids(*self.tokenizer.encode_batch(texts, max_seq_length))
        enc = self.tokenizer(texts, padding=True, truncation=True, max_length=max_seq_length, return_tensors="np")
        return self.encode_ids(enc["input_ids"].astype(np.int32), enc["attention_mask"].astype(np.uint8))

    def last_flops(self) -> float:
        return self._h.doubles("last_flops")[0]

    def close(self):
        self._h.close()


class SegmentBatcher:
    """Collects tokenised transcript segments on the device and encodes them ``batch_segments`` at a time.

    K8's cost per 128-token segment falls from 54 us at 8 segments per call to 19 us at 128 (``tools/embed_batch_sweep.py``:
    at 8 x 128 tokens the ~44 launches of the encoder are latency bound, at 128 x 128 the GEMMs take the 128 x 128-tile
    path), and segment embedding is not latency critical - the reference design indexes a video's segments after its
    transcription task has finished (``.kiro/specs/semantic-video-search/tasks.md:297-302``) - so the ingest path hands the
    encoder whole batches.  ``add`` copies the rows into a device staging buffer (no host round trip) and returns the
    embeddings of every batch it completed; ``flush`` encodes what is left.
    """

    def __init__(self, encoder: "MiniLMEncoder", seq_len: int, batch_segments: int = 128, device=None):
        import torch

        self.enc, self.S, self.cap = encoder, int(seq_len), int(batch_segments)
        dev = device or torch.device("cuda", torch.cuda.current_device())
        self._ids = torch.zeros((self.cap, self.S), dtype=torch.int32, device=dev)
        self._mask = torch.zeros((self.cap, self.S), dtype=torch.uint8, device=dev)
        self.fill = 0
        self.encoded = 0  # segments encoded so far

    def add(self, ids, mask) -> list:
        """ids int32 / mask uint8 ``(b, S)`` CUDA tensors -> list of ``(n, hidden)`` embedding tensors (often empty)."""
        out = []
        b, at = int(ids.shape[0]), 0
        while at < b:
            n = min(self.cap - self.fill, b - at)
            self._ids[self.fill:self.fill + n].copy_(ids[at:at + n], non_blocking=True)
            self._mask[self.fill:self.fill + n].copy_(mask[at:at + n], non_blocking=True)
            self.fill += n
            at += n
            if self.fill == self.cap:
                out.extend(self.flush())
        return out

    def flush(self) -> list:
        if not self.fill:
            return []
        n, self.fill = self.fill, 0
        self.encoded += n
        return [self.enc.encode_ids(self._ids[:n], self._mask[:n])]


# ---- nomic-embed-text (K27) ---------------------------------------------------------------------------------------------------
NOMIC_EMBED_TEXT_V1_5 = dict(vocab=30528, hidden=768, layers=12, heads=12, ffn=3072, max_pos=2048, type_vocab=2, ln_eps=1e-12,
                             rope_theta=1000.0)
# the task prefixes of the model card; the text that follows is what the task is about
NOMIC_PREFIXES = {"document": "search_document: ", "query": "search_query: ", "clustering": "clustering: ",
                  "classification": "classification: "}

# original nomic_bert checkpoint names -> NomicBertModel names, as transformers' conversion_mapping.py "nomic_bert" lists them
_NOMIC_RENAMES = (("encoder.layers", "layers"), ("emb_ln", "embeddings.LayerNorm"), ("attn.out_proj", "self_attn.o_proj"),
                  ("fc11", "up_proj"), ("fc12", "gate_proj"), ("fc2", "down_proj"), ("norm1", "post_attention_layernorm"),
                  ("norm2", "post_mlp_layernorm"))


def nomic_tensor_table(cfg: dict) -> list[tuple[str, tuple[int, ...]]]:
    """(state-dict name, shape) of every tensor the encoder needs (Hugging Face ``NomicBertModel`` names and order)."""
    H, F = cfg["hidden"], cfg["ffn"]
    t = [("embeddings.word_embeddings.weight", (cfg["vocab"], H)), ("embeddings.token_type_embeddings.weight", (cfg["type_vocab"], H)),
         ("embeddings.LayerNorm.weight", (H,)), ("embeddings.LayerNorm.bias", (H,))]
    for l in range(cfg["layers"]):
        p = f"layers.{l}."
        t += [(p + "post_attention_layernorm.weight", (H,)), (p + "post_attention_layernorm.bias", (H,)),
              (p + "mlp.gate_proj.weight", (F, H)), (p + "mlp.up_proj.weight", (F, H)), (p + "mlp.down_proj.weight", (H, F)),
              (p + "self_attn.q_proj.weight", (H, H)), (p + "self_attn.k_proj.weight", (H, H)),
              (p + "self_attn.v_proj.weight", (H, H)), (p + "self_attn.o_proj.weight", (H, H)),
              (p + "post_mlp_layernorm.weight", (H,)), (p + "post_mlp_layernorm.bias", (H,))]
    return t


def nomic_random_state(cfg: dict, seed: int) -> dict[str, np.ndarray]:
    """Seeded weights of the exact shapes: matrices N(0, 1 / fan_in), tables N(0, 0.5^2), LayerNorm gamma ~ 1, beta ~ 0."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in nomic_tensor_table(cfg):
        if name.lower().endswith("norm.weight"):
            out[name] = (1.0 + 0.1 * rng.standard_normal(shape)).astype(np.float32)
        elif name.endswith(".bias"):
            out[name] = (0.05 * rng.standard_normal(shape)).astype(np.float32)
        elif "embeddings" in name:
            out[name] = (0.5 * rng.standard_normal(shape)).astype(np.float32)
        else:
            out[name] = (rng.standard_normal(shape) / np.sqrt(shape[1])).astype(np.float32)
    return out


def _nomic_refuse(config: dict, key: str, allowed: tuple) -> None:
    if key in config and config[key] not in allowed:
        raise ValueError(f"nomic_bert config: {key}={config[key]!r} is not supported (this encoder has no Linear bias, post-LN "
                         "layers, SwiGLU, and plain non-interleaved RoPE over the whole head)")


def nomic_config(config: dict | str | Path) -> dict:
    """``config.json`` (a dict, the file, or its directory) -> the encoder's config dict.

    Read in the ``NomicBertConfig`` form of transformers (``hidden_size``, ``num_hidden_layers``, ``rope_parameters``, ...).  The
    keys of the original ``nomic_bert`` remote-code config (``n_embd``, ``n_layer``, ``n_head``, ``n_inner``, ``n_positions``,
    ``rotary_emb_base``, ``layer_norm_epsilon``; [PUBLIC-LIB], recalled from the public checkpoint's config, not read here) are
    accepted where they map one to one.  Anything that asks for a bias, pre-norm, interleaved or fractional rotary, RoPE scaling
    or another activation raises ``ValueError``."""
    if not isinstance(config, dict):
        p = Path(config)
        config = json.loads((p / "config.json" if p.is_dir() else p).read_text(encoding="utf-8"))
    c = NOMIC_EMBED_TEXT_V1_5

    def pick(new, old, default):
        return config.get(new, config.get(old, default)) if old else config.get(new, default)

    for key in ("qkv_proj_bias", "mlp_fc1_bias", "mlp_fc2_bias", "prenorm", "rotary_emb_interleaved", "use_rms_norm", "attention_bias",
                "mlp_bias"):
        _nomic_refuse(config, key, (False, None))
    _nomic_refuse(config, "rotary_emb_fraction", (1, 1.0, None))
    _nomic_refuse(config, "partial_rotary_factor", (1, 1.0, None))
    _nomic_refuse(config, "rotary_scaling_factor", (None,))
    _nomic_refuse(config, "rope_scaling", (None,))
    _nomic_refuse(config, "activation_function", ("swiglu", None))
    _nomic_refuse(config, "hidden_act", ("silu", None))
    rope = config.get("rope_parameters") or {}
    if rope.get("rope_type", "default") != "default" or any(k in rope for k in ("factor", "partial_rotary_factor")):
        raise ValueError(f"nomic_bert config: rope_parameters={rope!r} is not supported (plain RoPE only)")
    hidden, heads = int(pick("hidden_size", "n_embd", c["hidden"])), int(pick("num_attention_heads", "n_head", c["heads"]))
    if config.get("head_dim") not in (None, hidden // heads):
        raise ValueError(f"nomic_bert config: head_dim={config['head_dim']!r} is not hidden_size / num_attention_heads")
    ffn = pick("intermediate_size", "n_inner", None)
    return dict(vocab=int(config.get("vocab_size", c["vocab"])), hidden=hidden, layers=int(pick("num_hidden_layers", "n_layer", c["layers"])),
                heads=heads, ffn=int(ffn) if ffn is not None else 4 * hidden,
                max_pos=int(pick("max_position_embeddings", "n_positions", c["max_pos"])),
                type_vocab=int(config.get("type_vocab_size", c["type_vocab"])),
                ln_eps=float(pick("layer_norm_eps", "layer_norm_epsilon", c["ln_eps"])),
                rope_theta=float(rope.get("rope_theta", pick("rope_theta", "rotary_emb_base", c["rope_theta"]))))


def nomic_convert_state(raw: dict, cfg: dict) -> dict[str, np.ndarray]:
    """A checkpoint's tensors under either naming -> ``nomic_tensor_table`` names.  The transformers-native names pass through;
    the original names are renamed as ``conversion_mapping.py`` does and the fused ``attn.Wqkv`` is cut in three along dim 0."""
    named = {}
    for k, v in raw.items():
        k = k.removeprefix("nomic_bert.").removeprefix("bert.").removeprefix("0.auto_model.")
        for old, new in _NOMIC_RENAMES:
            k = k.replace(old, new)
        v = np.asarray(v, dtype=np.float32)
        if "attn.Wqkv" in k:
            if v.shape[0] % 3:
                raise ValueError(f"{k}: {v.shape[0]} rows cannot be cut into q, k and v")
            for part, rows in zip(("q_proj", "k_proj", "v_proj"), np.split(v, 3, axis=0)):
                named[k.replace("attn.Wqkv", "self_attn." + part)] = rows
        else:
            named[k] = v
    out = {}
    for name, shape in nomic_tensor_table(cfg):
        if name not in named:
            raise KeyError(f"checkpoint has no {name}")
        if tuple(named[name].shape) != tuple(shape):
            raise ValueError(f"{name}: shape {named[name].shape} != {shape}")
        out[name] = np.ascontiguousarray(named[name])
    for name in named:
        if name.startswith("layers.") and name.endswith(".bias") and "norm" not in name:
            raise ValueError(f"checkpoint carries {name}: this encoder has no Linear bias")
    return out


def nomic_load_state(path: str | Path, cfg: dict) -> dict[str, np.ndarray]:
    """``model.safetensors`` / ``pytorch_model.bin`` of nomic-embed-text, in the transformers-native or the original layout."""
    path = Path(path)
    if path.is_dir():
        for cand in ("model.safetensors", "pytorch_model.bin"):
            if (path / cand).exists():
                path = path / cand
                break
    if not path.exists() or path.is_dir():
        raise FileNotFoundError(f"encoder weights not found: {path}")
    if path.suffix == ".safetensors":
        from safetensors.numpy import load_file

        raw = load_file(str(path))
    else:
        import torch

        raw = {k: v.float().numpy() for k, v in torch.load(str(path), map_location="cpu", weights_only=True).items()}
    return nomic_convert_state(raw, cfg)


def prefix_lengths(mask) -> "np.ndarray":
    """Row lengths of a (B, S) attention mask whose rows are ones followed by zeros; anything else raises ``ValueError``
    (the packed encoder has no way to skip a token in the middle of a sequence)."""
    if on_device(mask):
        m = mask != 0
        ok = bool((m[:, :-1] | ~m[:, 1:]).all()) if m.shape[1] > 1 else True
        lengths = m.sum(1)
    else:
        m = np.asarray(mask) != 0
        ok = bool((m[:, :-1] | ~m[:, 1:]).all())
        lengths = m.sum(1)
    if not ok:
        raise ValueError("NomicEncoder: every attention-mask row must be a prefix of ones (ones, then zeros)")
    return lengths


class NomicEncoder:
    """nomic-embed-text resident on one GPU: packed variable-length sequences in, unit vectors out.

    ``matryoshka_dim``: keep the first that many columns (after the affine-free LayerNorm of the model card's recipe);
    ``cfg["hidden"]`` then reports that OUTPUT width, ``width`` the model's.  ``encode_ids`` has :class:`MiniLMEncoder`'s
    signature, so :class:`SegmentBatcher` and the search layer take either encoder."""

    def __init__(self, state: dict[str, np.ndarray] | None = None, cfg: dict = NOMIC_EMBED_TEXT_V1_5, tokenizer=None,
                 matryoshka_dim: int | None = None):
        self.width = int(cfg["hidden"])
        if matryoshka_dim is not None and not 1 <= int(matryoshka_dim) <= self.width:
            raise ValueError(f"matryoshka_dim must be in [1, {self.width}], got {matryoshka_dim}")
        self.matryoshka_dim = int(matryoshka_dim) if matryoshka_dim is not None else None
        self.model_cfg, self.tokenizer = dict(cfg), tokenizer
        self.cfg = dict(cfg, hidden=self.matryoshka_dim or self.width)
        self.prefixes = dict(NOMIC_PREFIXES)
        self._h = Handle("nomic", cfg["vocab"], self.width, cfg["layers"], cfg["heads"], cfg["ffn"], cfg["max_pos"], cfg["type_vocab"],
                         float(cfg["ln_eps"]), float(cfg["rope_theta"]))
        if state is not None:
            self._h.or_close(self.load_state, state)

    def load_state(self, state: dict[str, np.ndarray]) -> None:
        self._h.set_tensors(state)

    def encode_packed(self, ids, cu, with_hidden: bool = False, matryoshka_dim=...):
        """int32 ids ``(T,)`` and cu ``(B + 1,)`` (sequence b = ids[cu[b]:cu[b + 1]]) -> float32 ``(B, cfg["hidden"])`` unit vectors,
        with ``with_hidden`` also the last hidden state ``(T, width)``; numpy in -> numpy out, CUDA tensors in -> CUDA out.
        ``matryoshka_dim`` overrides the encoder's own for this call (``None``: the plain full-width vector)."""
        dev = on_device(ids)
        mdim = self.matryoshka_dim if matryoshka_dim is ... else matryoshka_dim
        B, T, dim = int(cu.shape[0]) - 1, int(ids.shape[0]), mdim or self.width
        if dev:
            import torch

            ids, cu = ids.to(torch.int32).contiguous(), cu.to(device=ids.device, dtype=torch.int32).contiguous()
            out = torch.empty((B, dim), dtype=torch.float32, device=ids.device)
            hidden = torch.empty((T, self.width), dtype=torch.float32, device=ids.device) if with_hidden else None
        else:
            ids, cu = np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(cu, dtype=np.int32)
            out = np.empty((B, dim), dtype=np.float32)
            hidden = np.empty((T, self.width), dtype=np.float32) if with_hidden else None
        if B > 0 and int(cu[-1]) != T:
            raise ValueError(f"cu[-1] = {int(cu[-1])} but {T} ids were given")
        _lib.check(self._h.eioku_nomic_encode(ptr(ids), ptr(cu), B, mdim or 0, ptr(out), ptr(hidden),
                                              _lib.MEM_DEVICE if dev else _lib.MEM_HOST, current_stream(ids)), "eioku_nomic_encode")
        return (out, hidden) if with_hidden else out

    def encode_ids(self, ids, mask):
        """int32 ids / uint8 mask ``(B,S)`` -> float32 ``(B, cfg["hidden"])`` unit vectors (numpy in -> numpy out).  The rows are
        packed (on the device when they are there); the mask must be a prefix of ones per row."""
        lengths = prefix_lengths(mask)
        if on_device(ids):
            import torch

            cu = torch.zeros(int(ids.shape[0]) + 1, dtype=torch.int32, device=ids.device)
            cu[1:] = torch.cumsum(lengths, 0)
            return self.encode_packed(ids[mask.to(ids.device) != 0], cu)
        cu = np.zeros(len(lengths) + 1, np.int32)
        cu[1:] = np.cumsum(lengths)
        return self.encode_packed(np.asarray(ids)[np.asarray(mask) != 0], cu)

    def encode(self, texts: list[str], kind: str = "document", max_seq_length: int | None = None):
        """Model-card entry: the task prefix of ``kind`` + text -> WordPiece -> unit vectors.  Needs the checkpoint's tokenizer."""
        if self.tokenizer is None:
            raise RuntimeError("NomicEncoder.encode() needs a tokenizer (vocab.txt of the checkpoint); use encode_ids() or "
                               "encode_packed() with pre-tokenised input otherwise")
        prefix = self.prefixes[kind]
        return self.encode_ids(*self.tokenizer.encode_batch([prefix + t for t in texts], max_seq_length or self.model_cfg["max_pos"]))

    def last_flops(self) -> float:
        return self._h.doubles("last_flops")[0]

    def last_ms(self) -> float:
        return self._h.doubles("last_ms")[0]

    def close(self):
        self._h.close()
