"""Torch-CPU restatement of K27 (nomic-embed-text, Hugging Face ``NomicBertModel`` layout, and the model card's pooling recipe).

Independent of the product and of ``transformers``: the forward pass is written from the layer description in DESIGN.md "K27
nomic-embed-text: ragged RoPE encoder", one sequence at a time, so there is no padding and no mask in it.  ``fp16=False`` is the
fp32 model (``tests/test_nomic_host.py`` pins it against ``transformers.NomicBertModel``); ``fp16=True`` rounds to fp16 where the
device stores fp16: matrix weights, the LayerNorm outputs as GEMM operands (the fp32 stream keeps the unrounded value), q / k
(after the rotation) / v, the softmax numerators, the attention output and the SwiGLU output.  The tables, LayerNorm parameters,
the residual stream, pooling and norms are fp32.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

PREFIXES = {"document": "search_document: ", "query": "search_query: ", "clustering": "clustering: ", "classification": "classification: "}


# ---- configurations (tests/test_nomic_gpu.py says why these) ----------------------------------------------------------------
def _cfg(**kw) -> dict:
    return {**dict(vocab=300, hidden=128, layers=2, heads=2, ffn=256, max_pos=2048, type_vocab=2, ln_eps=1e-12, rope_theta=1000.0), **kw}


def config_ns(layers: int = 2) -> dict:
    return _cfg(layers=layers)


def config_nw() -> dict:
    return _cfg(vocab=30528, hidden=768, heads=12, ffn=3072)


def config_nl() -> dict:
    return _cfg(layers=1)


LENGTHS_NS = (1, 3, 17, 65, 130)
LENGTHS_NW = (197, 9)
LENGTHS_NL = (2048, 5)


def hf_config(cfg: dict) -> dict:
    """The ``config.json`` keys of a configuration above (``NomicBertConfig`` form)."""
    return {"model_type": "nomic_bert", "vocab_size": cfg["vocab"], "hidden_size": cfg["hidden"], "num_hidden_layers": cfg["layers"],
            "num_attention_heads": cfg["heads"], "intermediate_size": cfg["ffn"], "hidden_act": "silu",
            "max_position_embeddings": cfg["max_pos"], "type_vocab_size": cfg["type_vocab"], "layer_norm_eps": cfg["ln_eps"],
            "rope_parameters": {"rope_type": "default", "rope_theta": cfg["rope_theta"]}, "pad_token_id": 0}


# ---- weights ------------------------------------------------------------------------------------------------------------------
def random_weights(cfg: dict, seed: int) -> dict:
    """Seeded ``NomicBertModel.state_dict()`` of the exact shapes and order (torch tensors)."""
    g = torch.Generator().manual_seed(seed)
    d, ffn = cfg["hidden"], cfg["ffn"]
    w = {}

    def lin(name, out, inp):
        w[name + ".weight"] = torch.randn(out, inp, generator=g) / inp ** 0.5

    def lnorm(name):
        w[name + ".weight"] = 1.0 + 0.2 * (torch.rand(d, generator=g) - 0.5)
        w[name + ".bias"] = 0.05 * torch.randn(d, generator=g)

    w["embeddings.word_embeddings.weight"] = 0.5 * torch.randn(cfg["vocab"], d, generator=g)
    w["embeddings.token_type_embeddings.weight"] = 0.2 * torch.randn(cfg["type_vocab"], d, generator=g)
    lnorm("embeddings.LayerNorm")
    for layer in range(cfg["layers"]):
        p = f"layers.{layer}."
        lnorm(p + "post_attention_layernorm")
        lin(p + "mlp.gate_proj", ffn, d)
        lin(p + "mlp.up_proj", ffn, d)
        lin(p + "mlp.down_proj", d, ffn)
        for proj in ("q_proj", "k_proj", "v_proj", "o_proj"):
            lin(p + "self_attn." + proj, d, d)
        lnorm(p + "post_mlp_layernorm")
    return w


def original_layout(weights: dict) -> dict:
    """The same tensors under the names of the original ``nomic_bert`` checkpoint: ``encoder.layers``, fused ``attn.Wqkv``,
    ``fc11`` (up) / ``fc12`` (gate) / ``fc2`` (down), ``norm1`` / ``norm2``, ``emb_ln``."""
    out, qkv = {}, {}
    for k, v in weights.items():
        if ".self_attn.q_proj" in k or ".self_attn.k_proj" in k or ".self_attn.v_proj" in k:
            qkv.setdefault(k.split(".self_attn.")[0], {})[k.split(".self_attn.")[1][0]] = v
            continue
        k = k.replace("embeddings.LayerNorm", "emb_ln").replace("self_attn.o_proj", "attn.out_proj")
        k = k.replace("up_proj", "fc11").replace("gate_proj", "fc12").replace("down_proj", "fc2")
        k = k.replace("post_attention_layernorm", "norm1").replace("post_mlp_layernorm", "norm2")
        out[("encoder." + k) if k.startswith("layers.") else k] = v
    for p, parts in qkv.items():
        out[f"encoder.{p}.attn.Wqkv.weight"] = torch.cat([torch.as_tensor(parts[c]) for c in "qkv"], 0)
    return out


# ---- the row orders of the packed device weights (DESIGN.md "K27"), restated for the host test ------------------------------------
def rope_row_order(d: int) -> np.ndarray:
    """order[s] = the q_proj / k_proj row stored at row s: within each 64-row head, 2j <- j and 2j + 1 <- j + 32"""
    s = np.arange(d)
    j = s % 64
    return s - j + np.where(j % 2 == 0, j // 2, 32 + j // 2)


def gate_up_interleave(gate: np.ndarray, up: np.ndarray) -> np.ndarray:
    out = np.empty((2 * gate.shape[0],) + gate.shape[1:], gate.dtype)
    out[0::2], out[1::2] = gate, up
    return out


def rope_tables(cfg: dict, n: int):
    """cos, sin (n, 32) in fp32 as transformers computes them"""
    inv_freq = 1.0 / (cfg["rope_theta"] ** (torch.arange(0, 64, 2, dtype=torch.float) / 64))
    ang = torch.arange(n, dtype=torch.float)[:, None] * inv_freq[None, :]
    return ang.cos(), ang.sin()


def rotate(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """rotate_half RoPE on (..., n, 64): x'_j = x_j cos_j - x_(j+32) sin_j, x'_(j+32) = x_(j+32) cos_j + x_j sin_j"""
    lo, hi = x[..., :32], x[..., 32:]
    return torch.cat([lo * cos - hi * sin, hi * cos + lo * sin], -1)


class Oracle:
    def __init__(self, cfg: dict, weights: dict, fp16: bool):
        self.cfg, self.fp16 = cfg, fp16
        self.w = {}
        for k, v in weights.items():
            v = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).detach().float().clone()
            matrix = v.dim() == 2 and "embeddings" not in k
            self.w[k] = v.half().float() if (fp16 and matrix) else v

    def r(self, t: torch.Tensor) -> torch.Tensor:
        return t.half().float() if self.fp16 else t

    def _ln(self, x, name):
        return F.layer_norm(x, (x.shape[-1],), self.w[name + ".weight"], self.w[name + ".bias"], self.cfg["ln_eps"])

    def _lin(self, x, name):
        return x @ self.w[name + ".weight"].T

    @torch.no_grad()
    def hidden(self, ids) -> torch.Tensor:
        """one sequence of ids (n,) -> the last hidden state (n, d)"""
        cfg = self.cfg
        heads, n = cfg["heads"], len(ids)
        idx = torch.from_numpy(np.asarray(ids).astype(np.int64))
        x = self._ln(self.w["embeddings.word_embeddings.weight"][idx] + self.w["embeddings.token_type_embeddings.weight"][0],
                     "embeddings.LayerNorm")
        cos, sin = rope_tables(cfg, n)
        for layer in range(cfg["layers"]):
            p = f"layers.{layer}."
            h = self.r(x)
            q, k, v = (self._lin(h, p + "self_attn." + name).view(n, heads, 64).transpose(0, 1) for name in ("q_proj", "k_proj", "v_proj"))
            q, k, v = self.r(rotate(q, cos, sin)), self.r(rotate(k, cos, sin)), self.r(v)
            s = (q @ k.transpose(-1, -2)) * 0.125
            if self.fp16:
                e = self.r(torch.exp(s - s.amax(-1, keepdim=True)))
                a = (e @ v) / e.sum(-1, keepdim=True)
            else:
                a = torch.softmax(s, dim=-1) @ v
            a = self.r(a.transpose(0, 1).reshape(n, -1))
            x = self._ln(x + self._lin(a, p + "self_attn.o_proj"), p + "post_attention_layernorm")
            h = self.r(x)
            mid = self.r(F.silu(self._lin(h, p + "mlp.gate_proj")) * self._lin(h, p + "mlp.up_proj"))
            x = self._ln(x + self._lin(mid, p + "mlp.down_proj"), p + "post_mlp_layernorm")
        return x

    @staticmethod
    def pool(hidden: torch.Tensor, matryoshka_dim: int | None = None) -> torch.Tensor:
        """the model card's recipe on one sequence's rows: mean, [affine-free LayerNorm eps 1e-5, slice], L2 normalise"""
        e = hidden.mean(0)
        if matryoshka_dim:
            e = F.layer_norm(e, (e.shape[0],))[:matryoshka_dim]
        return e / e.norm()

    @torch.no_grad()
    def encode(self, seqs, matryoshka_dim: int | None = None):
        """list of id arrays -> ``(hidden (T, d) packed in order, unit vectors (B, dim))`` as numpy"""
        hs = [self.hidden(s) for s in seqs]
        return torch.cat(hs).numpy(), torch.stack([self.pool(h, matryoshka_dim) for h in hs]).numpy()


def random_ids(cfg: dict, lengths, seed: int) -> list:
    rng = np.random.default_rng(seed)
    return [rng.integers(1, cfg["vocab"], n).astype(np.int32) for n in lengths]


def pack(seqs):
    """-> (ids (T,), cu (B + 1,)) int32"""
    cu = np.zeros(len(seqs) + 1, np.int32)
    cu[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs).astype(np.int32), cu


def pad(seqs, width: int | None = None, fill: int = 0):
    """-> (ids (B, S) int32, mask (B, S) uint8)"""
    S = width or max(len(s) for s in seqs)
    ids, mask = np.full((len(seqs), S), fill, np.int32), np.zeros((len(seqs), S), np.uint8)
    for b, s in enumerate(seqs):
        ids[b, :len(s)], mask[b, :len(s)] = s, 1
    return ids, mask
