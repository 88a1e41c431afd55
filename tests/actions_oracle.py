"""Torch-CPU restatement of K25 (TimeSformer, divided space-time attention) and of its clip preprocessing.

Independent of the product and of ``transformers``: the forward pass is written from the layer description in DESIGN.md
"K25 action recognition", the preprocessing from Pillow's two-pass resample as ``oracle/places.py`` restates it.  ``fp16=False``
is the fp32 model (``tests/test_actions_host.py`` pins it against ``TimesformerForVideoClassification``); ``fp16=True``
rounds to fp16 where the device stores fp16: matrix weights, the patch rows, LayerNorm outputs, q / k / v, attention
outputs, the temporal out-projection, GELU outputs, and the softmax numerators of the spatial attention.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle.places import _pass, resize_coeffs

PATCH = 16


def config_s() -> dict:
    return {"image": 48, "frames": 3, "hidden": 128, "layers": 2, "heads": 2, "ffn": 256, "labels": 7, "ln_eps": 1e-6}


def config_s1() -> dict:
    return {**config_s(), "frames": 1}


def config_s96() -> dict:
    return {"image": 32, "frames": 96, "hidden": 128, "layers": 1, "heads": 2, "ffn": 256, "labels": 7, "ln_eps": 1e-6}


def config_w(layers: int = 2) -> dict:
    return {"image": 224, "frames": 8, "hidden": 768, "layers": layers, "heads": 12, "ffn": 3072, "labels": 400, "ln_eps": 1e-6}


def hf_config(cfg: dict) -> dict:
    """The ``config.json`` keys of a configuration above."""
    return {"image_size": cfg["image"], "patch_size": PATCH, "num_channels": 3, "num_frames": cfg["frames"],
            "hidden_size": cfg["hidden"], "num_hidden_layers": cfg["layers"], "num_attention_heads": cfg["heads"],
            "intermediate_size": cfg["ffn"], "hidden_act": "gelu", "layer_norm_eps": cfg["ln_eps"], "qkv_bias": True,
            "attention_type": "divided_space_time", "num_labels": cfg["labels"],
            "id2label": {str(i): f"LABEL_{i}" for i in range(cfg["labels"])}}


# ---- preprocessing ----------------------------------------------------------------------------------------------------------
def resized_size(h: int, w: int, edge: int):
    """short edge -> ``edge``, long edge -> ``int(edge * long / short)``"""
    return (edge, int(edge * w / h)) if h <= w else (int(edge * h / w), edge)


def preprocess(frames_bgr: np.ndarray, edge: int, crop: int, mean=(0.45,) * 3, std=(0.225,) * 3):
    """BGR uint8 (n, h, w, 3) -> ``(uint8 (n, crop, crop, 3) RGB, float32 (n, crop, crop, 3))``: the whole frame through
    Pillow's horizontal then vertical 8-bit pass, the centre crop at ``(dim - crop) // 2``, then
    ``(v * (1 / 255) - mean) / std`` in float32."""
    n, h, w, _ = frames_bgr.shape
    rh, rw = resized_size(h, w, edge)
    top, left = (rh - crop) // 2, (rw - crop) // 2
    u8 = np.empty((n, crop, crop, 3), np.uint8)
    for i, f in enumerate(frames_bgr):
        img = np.ascontiguousarray(f[..., ::-1])
        if rw != w:
            img = _pass(img, *resize_coeffs(w, rw), axis=1)
        if rh != h:
            img = _pass(img, *resize_coeffs(h, rh), axis=0)
        u8[i] = img[top:top + crop, left:left + crop]
    return u8, normalise(u8, mean, std)


def normalise(u8: np.ndarray, mean=(0.45,) * 3, std=(0.225,) * 3) -> np.ndarray:
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    return (u8.astype(np.float32) * np.float32(1.0 / 255.0) - m) / s


def patch_rows(x: np.ndarray) -> np.ndarray:
    """(B, T, S, S, 3) channel-last values -> (B, P, T, 768) patch rows, column ``c * 256 + ky * 16 + kx``"""
    B, T, S, _, _ = x.shape
    g = S // PATCH
    x = x.reshape(B, T, g, PATCH, g, PATCH, 3)             # b t py ky px kx c
    return np.ascontiguousarray(x.transpose(0, 2, 4, 1, 6, 3, 5)).reshape(B, g * g, T, 3 * PATCH * PATCH)


def pixel_values(rows: np.ndarray, image: int) -> np.ndarray:
    """The inverse relayout: (B, P, T, 768) patch rows -> (B, T, 3, S, S) as ``transformers`` takes them"""
    B, P, T, _ = rows.shape
    g = image // PATCH
    x = rows.reshape(B, g, g, T, 3, PATCH, PATCH)          # b py px t c ky kx
    return np.ascontiguousarray(x.transpose(0, 3, 4, 1, 5, 2, 6)).reshape(B, T, 3, image, image)


# ---- weights ----------------------------------------------------------------------------------------------------------------
def random_weights(cfg: dict, seed: int, classifier_gain: float = 8.0) -> dict:
    """Seeded ``state_dict()`` of the exact shapes (torch tensors)."""
    g = torch.Generator().manual_seed(seed)
    d, P, T = cfg["hidden"], (cfg["image"] // PATCH) ** 2, cfg["frames"]
    w = {}

    def lin(name, out, inp, gain=1.0):
        w[name + ".weight"] = gain * torch.randn(out, inp, generator=g) / inp ** 0.5
        w[name + ".bias"] = 0.05 * torch.randn(out, generator=g)

    def lnorm(name):
        w[name + ".weight"] = 1.0 + 0.2 * (torch.rand(d, generator=g) - 0.5)
        w[name + ".bias"] = 0.05 * torch.randn(d, generator=g)

    e = "timesformer.embeddings."
    w[e + "cls_token"] = 0.2 * torch.randn(1, 1, d, generator=g)
    w[e + "position_embeddings"] = 0.2 * torch.randn(1, 1 + P, d, generator=g)
    w[e + "time_embeddings"] = 0.2 * torch.randn(1, T, d, generator=g)
    w[e + "patch_embeddings.projection.weight"] = torch.randn(d, 3, PATCH, PATCH, generator=g) / (3 * PATCH * PATCH) ** 0.5
    w[e + "patch_embeddings.projection.bias"] = 0.05 * torch.randn(d, generator=g)
    for layer in range(cfg["layers"]):
        p = f"timesformer.encoder.layer.{layer}."
        lnorm(p + "temporal_layernorm")
        lin(p + "temporal_attention.attention.qkv", 3 * d, d)
        lin(p + "temporal_attention.output.dense", d, d)
        lin(p + "temporal_dense", d, d)
        lnorm(p + "layernorm_before")
        lin(p + "attention.attention.qkv", 3 * d, d)
        lin(p + "attention.output.dense", d, d)
        lnorm(p + "layernorm_after")
        lin(p + "intermediate.dense", cfg["ffn"], d)
        lin(p + "output.dense", d, cfg["ffn"])
    lnorm("timesformer.layernorm")
    lin("classifier", cfg["labels"], d, classifier_gain)
    return w


class Oracle:
    def __init__(self, cfg: dict, weights: dict, fp16: bool):
        self.cfg, self.fp16 = cfg, fp16
        self.w = {}
        for k, v in weights.items():
            v = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).detach().float().clone()
            matrix = k.endswith(".weight") and v.dim() >= 2
            self.w[k] = v.half().float() if (fp16 and matrix) else v

    def r(self, t: torch.Tensor) -> torch.Tensor:
        return t.half().float() if self.fp16 else t

    def _ln(self, x, name):
        return self.r(F.layer_norm(x, (x.shape[-1],), self.w[name + ".weight"], self.w[name + ".bias"], self.cfg["ln_eps"]))

    def _lin(self, x, name):
        return x @ self.w[name + ".weight"].T + self.w[name + ".bias"]

    def _attend(self, h, name, round_probs: bool):
        """h [n][L][d] (LayerNorm output) -> attention output [n][L][d] before the out-projection"""
        n, L, d = h.shape
        heads = self.cfg["heads"]
        qkv = self.r(self._lin(h, name + ".attention.qkv")).view(n, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
        s = (qkv[0] @ qkv[1].transpose(-1, -2)) * 0.125
        if round_probs:
            p = self.r(torch.exp(s - s.amax(-1, keepdim=True)))
            a = (p @ qkv[2]) / p.sum(-1, keepdim=True)
        else:
            a = torch.softmax(s, dim=-1) @ qkv[2]
        return self.r(a.transpose(1, 2).reshape(n, L, d))

    @torch.no_grad()
    def embed(self, rows: np.ndarray):
        """(B, P, T, 768) patch rows -> cls [B][d], patch tokens [B][P][T][d]"""
        w = self.w
        e = "timesformer.embeddings."
        x = self.r(torch.from_numpy(np.ascontiguousarray(rows)).float())
        B, P, T, K = x.shape
        tok = x @ w[e + "patch_embeddings.projection.weight"].reshape(-1, K).T + w[e + "patch_embeddings.projection.bias"]
        pos, time = w[e + "position_embeddings"][0], w[e + "time_embeddings"][0]
        tok = tok + (pos[1:, None, :] + time[None, :, :])
        cls = (w[e + "cls_token"][0, 0] + pos[0]).expand(B, -1)
        return cls, tok

    @torch.no_grad()
    def forward(self, rows: np.ndarray):
        """(B, P, T, 768) patch rows -> ``(hidden [B][1 + P T][d] before the final LayerNorm, logits [B][labels])``"""
        cls, tok = self.embed(rows)
        B, P, T, d = tok.shape
        for layer in range(self.cfg["layers"]):
            p = f"timesformer.encoder.layer.{layer}."
            # temporal attention over the T tokens of each (clip, patch)
            h = self._ln(tok.reshape(B * P, T, d), p + "temporal_layernorm")
            a = self._attend(h, p + "temporal_attention", round_probs=False)
            a = self.r(self._lin(a, p + "temporal_attention.output.dense"))
            tok = tok + self._lin(a, p + "temporal_dense").view(B, P, T, d)
            # spatial attention over [CLS, the P tokens of frame t] of each (clip, frame)
            seq = torch.cat([cls[:, None, None, :].expand(B, T, 1, d), tok.transpose(1, 2)], 2).reshape(B * T, 1 + P, d)
            h = self._ln(seq, p + "layernorm_before")
            a = self._attend(h, p + "attention", round_probs=self.fp16)
            out = self._lin(a, p + "attention.output.dense").view(B, T, 1 + P, d)
            tok = tok + out[:, :, 1:].transpose(1, 2)
            acc = torch.zeros(B, d)
            for t in range(T):
                acc = acc + out[:, t, 0]
            cls = cls + acc / T
            # MLP over every token
            x = torch.cat([cls[:, None, :], tok.reshape(B, P * T, d)], 1)
            h = self._ln(x, p + "layernorm_after")
            mid = self.r(F.gelu(self._lin(h, p + "intermediate.dense")))
            x = x + self._lin(mid, p + "output.dense")
            cls, tok = x[:, 0], x[:, 1:].reshape(B, P, T, d)
        hidden = torch.cat([cls[:, None, :], tok.reshape(B, P * T, d)], 1)
        logits = self._lin(self._ln(cls, "timesformer.layernorm"), "classifier")
        return hidden, logits


def softmax_topk(logits: np.ndarray, top_k: int):
    """float32 softmax and a stable descending sort: ``(probs (n, top_k), ids (n, top_k))``, ties to the smaller index.
    Every stage is a float32 value rounded once: ``x - max``, ``exp`` of it (numpy's float32 ``exp`` may be 2.5 ulp off,
    so it is taken in float64 and rounded), the sum of the exponentials (likewise: no summation order), the quotient."""
    logits = np.asarray(logits, np.float32)
    e = np.exp((logits - logits.max(-1, keepdims=True)).astype(np.float64)).astype(np.float32)
    total = e.astype(np.float64).sum(-1, keepdims=True).astype(np.float32)
    p = (e / total).astype(np.float32)
    ids = np.argsort(-p, axis=-1, kind="stable")[:, :top_k]
    return np.take_along_axis(p, ids, -1), ids.astype(np.int32)
