"""Torch-CPU restatement of K26 (CLIP image and text towers, Hugging Face ``CLIPModel`` layout) and of its preprocessing.

Independent of the product and of ``transformers``: the forward pass is written from the layer description in DESIGN.md
"K26 CLIP frame and text embeddings", the preprocessing from Pillow's two-pass resample (``oracle/places.py`` restates the
8-bit pass; the bicubic coefficient function here is Pillow's formula).  ``fp16=False`` is the fp32 model
(``tests/test_clip_host.py`` pins it against ``transformers.CLIPModel``); ``fp16=True`` rounds to fp16 where the device
stores fp16: matrix weights, the patch rows, LayerNorm outputs (not ``pre_layrnorm``, which writes the fp32 stream), q / k /
v, attention outputs, activation outputs, and the softmax numerators.  The projection, the norm and the outputs are fp32.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.places import PRECISION_BITS, _pass

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


# ---- configurations (tests/test_clip_gpu.py says why these) ---------------------------------------------------------------
def _text_tiny() -> dict:
    return {"vocab": 300, "positions": 77, "hidden": 64, "layers": 0, "heads": 1, "ffn": 32}


def _vision_tiny() -> dict:
    return {"image": 32, "patch": 32, "hidden": 64, "layers": 0, "heads": 1, "ffn": 32}


def config_vs() -> dict:
    return {"vision": {"image": 64, "patch": 32, "hidden": 128, "layers": 2, "heads": 2, "ffn": 256}, "text": _text_tiny(),
            "projection": 64, "ln_eps": 1e-5, "act": "quick_gelu", "eos_token_id": 299}


def config_v14() -> dict:
    return {"vision": {"image": 56, "patch": 14, "hidden": 128, "layers": 1, "heads": 2, "ffn": 256}, "text": _text_tiny(),
            "projection": 64, "ln_eps": 1e-5, "act": "gelu", "eos_token_id": 299}


def config_vw(layers: int = 2) -> dict:
    return {"vision": {"image": 224, "patch": 16, "hidden": 768, "layers": layers, "heads": 12, "ffn": 3072}, "text": _text_tiny(),
            "projection": 512, "ln_eps": 1e-5, "act": "quick_gelu", "eos_token_id": 299}


def config_ts(layers: int = 2, eos_token_id: int = 299) -> dict:
    return {"vision": _vision_tiny(), "text": {"vocab": 300, "positions": 77, "hidden": 128, "layers": layers, "heads": 2, "ffn": 256},
            "projection": 64, "ln_eps": 1e-5, "act": "quick_gelu", "eos_token_id": eos_token_id}


def config_tw() -> dict:
    return {"vision": _vision_tiny(), "text": {"vocab": 49408, "positions": 77, "hidden": 512, "layers": 2, "heads": 8, "ffn": 2048},
            "projection": 512, "ln_eps": 1e-5, "act": "quick_gelu", "eos_token_id": 49407}


def config_vs_ts() -> dict:
    """VS's vision tower and TS's text tower behind one model (the retrieval test)."""
    return {**config_vs(), "text": config_ts()["text"]}


def hf_config(cfg: dict) -> dict:
    """The ``config.json`` keys of a configuration above."""
    v, t = cfg["vision"], cfg["text"]
    return {"model_type": "clip", "projection_dim": cfg["projection"],
            "vision_config": {"image_size": v["image"], "patch_size": v["patch"], "num_channels": 3, "hidden_size": v["hidden"],
                              "num_hidden_layers": v["layers"], "num_attention_heads": v["heads"], "intermediate_size": v["ffn"],
                              "hidden_act": cfg["act"], "layer_norm_eps": cfg["ln_eps"], "projection_dim": cfg["projection"]},
            "text_config": {"vocab_size": t["vocab"], "max_position_embeddings": t["positions"], "hidden_size": t["hidden"],
                            "num_hidden_layers": t["layers"], "num_attention_heads": t["heads"], "intermediate_size": t["ffn"],
                            "hidden_act": cfg["act"], "layer_norm_eps": cfg["ln_eps"], "projection_dim": cfg["projection"],
                            "eos_token_id": cfg["eos_token_id"], "bos_token_id": 0, "pad_token_id": 1}}


# ---- preprocessing ----------------------------------------------------------------------------------------------------------
def bicubic(x: float) -> float:
    """Pillow's ``bicubic_filter`` (a = -0.5, support 2)"""
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def bicubic_coeffs(in_size: int, out_size: int):
    """Pillow ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for the bicubic filter over the whole axis: per output
    position the first input index, the tap count, and int32 coefficients scaled by 2**22 (negative taps round away from
    zero, as the C cast of ``-0.5 + v`` does)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def resized_size(h: int, w: int, edge: int):
    """short edge -> ``edge``, long edge -> ``int(edge * long / short)``"""
    return (edge, int(edge * w / h)) if h <= w else (int(edge * h / w), edge)


def normalise(u8: np.ndarray, mean=CLIP_MEAN, std=CLIP_STD) -> np.ndarray:
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    return (u8.astype(np.float32) * np.float32(1.0 / 255.0) - m) / s


def preprocess(frames_bgr: np.ndarray, edge: int, crop: int, mean=CLIP_MEAN, std=CLIP_STD):
    """BGR uint8 (n, h, w, 3) -> ``(uint8 (n, crop, crop, 3) RGB, float32 (n, crop, crop, 3))``: the whole frame through
    Pillow's horizontal then vertical 8-bit bicubic pass (a pass whose size does not change is skipped, as Pillow skips it),
    the centre crop at ``(dim - crop) // 2``, then ``(v * (1 / 255) - mean) / std`` in float32."""
    n, h, w, _ = frames_bgr.shape
    rh, rw = resized_size(h, w, edge)
    top, left = (rh - crop) // 2, (rw - crop) // 2
    u8 = np.empty((n, crop, crop, 3), np.uint8)
    for i, f in enumerate(frames_bgr):
        img = np.ascontiguousarray(f[..., ::-1])
        if rw != w:
            img = _pass(img, *bicubic_coeffs(w, rw), axis=1)
        if rh != h:
            img = _pass(img, *bicubic_coeffs(h, rh), axis=0)
        u8[i] = img[top:top + crop, left:left + crop]
    return u8, normalise(u8, mean, std)


def padded_k(patch: int) -> int:
    return (3 * patch * patch + 31) // 32 * 32


def patch_rows(x: np.ndarray, patch: int) -> np.ndarray:
    """(B, S, S, 3) channel-last values -> (B, 1 + P, Kp) patch rows: token 0 zeros, column ``c p p + ky p + kx``, the
    columns from 3 p p to Kp zeros"""
    B, S, _, _ = x.shape
    g, K = S // patch, 3 * patch * patch
    x = x.reshape(B, g, patch, g, patch, 3).transpose(0, 1, 3, 5, 2, 4).reshape(B, g * g, K)  # b py px c ky kx
    out = np.zeros((B, 1 + g * g, padded_k(patch)), x.dtype)
    out[:, 1:, :K] = x
    return out


def pixel_values(rows: np.ndarray, image: int, patch: int) -> np.ndarray:
    """The inverse relayout: (B, 1 + P, Kp) patch rows -> (B, 3, S, S) as ``transformers`` takes them"""
    B = rows.shape[0]
    g = image // patch
    x = rows[:, 1:, :3 * patch * patch].reshape(B, g, g, 3, patch, patch)  # b py px c ky kx
    return np.ascontiguousarray(x.transpose(0, 3, 1, 4, 2, 5)).reshape(B, 3, image, image)


# ---- weights ----------------------------------------------------------------------------------------------------------------
def random_weights(cfg: dict, seed: int) -> dict:
    """Seeded ``CLIPModel.state_dict()`` of the exact shapes (torch tensors; no ``logit_scale``, no ``position_ids``)."""
    g = torch.Generator().manual_seed(seed)
    w = {}

    def lin(name, out, inp):
        w[name + ".weight"] = torch.randn(out, inp, generator=g) / inp ** 0.5
        w[name + ".bias"] = 0.05 * torch.randn(out, generator=g)

    def lnorm(name, d):
        w[name + ".weight"] = 1.0 + 0.2 * (torch.rand(d, generator=g) - 0.5)
        w[name + ".bias"] = 0.05 * torch.randn(d, generator=g)

    def layers(model, t):
        d = t["hidden"]
        for layer in range(t["layers"]):
            p = f"{model}.encoder.layers.{layer}."
            for proj in ("k_proj", "v_proj", "q_proj", "out_proj"):
                lin(p + "self_attn." + proj, d, d)
            lnorm(p + "layer_norm1", d)
            lin(p + "mlp.fc1", t["ffn"], d)
            lin(p + "mlp.fc2", d, t["ffn"])
            lnorm(p + "layer_norm2", d)

    t, v = cfg["text"], cfg["vision"]
    w["text_model.embeddings.token_embedding.weight"] = 0.5 * torch.randn(t["vocab"], t["hidden"], generator=g)
    w["text_model.embeddings.position_embedding.weight"] = 0.2 * torch.randn(t["positions"], t["hidden"], generator=g)
    layers("text_model", t)
    lnorm("text_model.final_layer_norm", t["hidden"])
    P, K = (v["image"] // v["patch"]) ** 2, 3 * v["patch"] ** 2
    w["vision_model.embeddings.class_embedding"] = 0.5 * torch.randn(v["hidden"], generator=g)
    w["vision_model.embeddings.patch_embedding.weight"] = torch.randn(v["hidden"], 3, v["patch"], v["patch"], generator=g) / K ** 0.5
    w["vision_model.embeddings.position_embedding.weight"] = 0.2 * torch.randn(1 + P, v["hidden"], generator=g)
    lnorm("vision_model.pre_layrnorm", v["hidden"])
    layers("vision_model", v)
    lnorm("vision_model.post_layernorm", v["hidden"])
    w["visual_projection.weight"] = torch.randn(cfg["projection"], v["hidden"], generator=g) / v["hidden"] ** 0.5
    w["text_projection.weight"] = torch.randn(cfg["projection"], t["hidden"], generator=g) / t["hidden"] ** 0.5
    return w


def eot_positions(ids: np.ndarray, eos_token_id: int) -> np.ndarray:
    """The pooled position of each text: the first position holding ``eos_token_id``; for the legacy configurations whose
    ``eos_token_id`` is 2, the position of the largest id."""
    ids = np.asarray(ids)
    if eos_token_id == 2:
        return ids.argmax(-1).astype(np.int32)
    return (ids == eos_token_id).argmax(-1).astype(np.int32)


_TABLES = ("token_embedding.weight", "position_embedding.weight")


class Oracle:
    def __init__(self, cfg: dict, weights: dict, fp16: bool):
        self.cfg, self.fp16 = cfg, fp16
        self.w = {}
        for k, v in weights.items():
            v = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).detach().float().clone()
            matrix = k.endswith(".weight") and v.dim() >= 2 and not k.endswith(_TABLES)
            self.w[k] = v.half().float() if (fp16 and matrix) else v

    def r(self, t: torch.Tensor) -> torch.Tensor:
        return t.half().float() if self.fp16 else t

    def _ln(self, x, name):
        return F.layer_norm(x, (x.shape[-1],), self.w[name + ".weight"], self.w[name + ".bias"], self.cfg["ln_eps"])

    def _lin(self, x, name):
        return x @ self.w[name + ".weight"].T + self.w[name + ".bias"]

    def _act(self, x):
        return x * torch.sigmoid(1.702 * x) if self.cfg["act"] == "quick_gelu" else F.gelu(x)

    def _layers(self, x, model: str, tower: dict, causal: bool):
        B, n, d = x.shape
        heads = tower["heads"]
        for layer in range(tower["layers"]):
            p = f"{model}.encoder.layers.{layer}."
            h = self.r(self._ln(x, p + "layer_norm1"))
            q, k, v = (self.r(self._lin(h, p + "self_attn." + name)).view(B, n, heads, 64).transpose(1, 2)
                       for name in ("q_proj", "k_proj", "v_proj"))
            s = (q @ k.transpose(-1, -2)) * 0.125
            if causal:
                s = s.masked_fill(torch.triu(torch.ones(n, n, dtype=torch.bool), 1), float("-inf"))
            if self.fp16:
                e = self.r(torch.exp(s - s.amax(-1, keepdim=True)))
                a = (e @ v) / e.sum(-1, keepdim=True)
            else:
                a = torch.softmax(s, dim=-1) @ v
            a = self.r(a.transpose(1, 2).reshape(B, n, d))
            x = x + self._lin(a, p + "self_attn.out_proj")
            h = self.r(self._ln(x, p + "layer_norm2"))
            mid = self.r(self._act(self._lin(h, p + "mlp.fc1")))
            x = x + self._lin(mid, p + "mlp.fc2")
        return x

    def _head(self, rows, ln_name: str, proj_name: str):
        pooled = self.r(self._ln(rows, ln_name)) @ self.w[proj_name].T
        return pooled / pooled.norm(dim=-1, keepdim=True)

    @torch.no_grad()
    def vision(self, rows: np.ndarray):
        """(B, 1 + P, Kp) patch rows -> ``(hidden [B][1 + P][d] before post_layernorm, unit vectors [B][projection])``"""
        v, e = self.cfg["vision"], "vision_model.embeddings."
        K = 3 * v["patch"] ** 2
        x = self.r(torch.from_numpy(np.ascontiguousarray(rows)).float())[:, 1:, :K]
        pos = self.w[e + "position_embedding.weight"]
        tok = x @ self.w[e + "patch_embedding.weight"].reshape(-1, K).T + pos[1:]
        cls = (self.w[e + "class_embedding"] + pos[0]).expand(x.shape[0], 1, -1)
        x = self._ln(torch.cat([cls, tok], 1), "vision_model.pre_layrnorm")  # the fp32 stream: not rounded
        x = self._layers(x, "vision_model", v, causal=False)
        return x, self._head(x[:, 0], "vision_model.post_layernorm", "visual_projection.weight")

    @torch.no_grad()
    def text(self, ids: np.ndarray, n: int | None = None):
        """ids (B, positions) -> ``(hidden [B][n][d] before final_layer_norm, unit vectors [B][projection])`` over the first
        ``n`` positions (default: all)"""
        t, e = self.cfg["text"], "text_model.embeddings."
        ids = np.asarray(ids)
        eot = eot_positions(ids, self.cfg["eos_token_id"])
        n = ids.shape[1] if n is None else n
        assert int(eot.max()) < n
        idx = torch.from_numpy(ids[:, :n].astype(np.int64))
        x = self.w[e + "token_embedding.weight"][idx] + self.w[e + "position_embedding.weight"][:n]
        x = self._layers(x, "text_model", t, causal=True)
        rows = x[torch.arange(x.shape[0]), torch.from_numpy(eot.astype(np.int64))]
        return x, self._head(rows, "text_model.final_layer_norm", "text_projection.weight")

    @torch.no_grad()
    def text_final(self, hidden: torch.Tensor) -> torch.Tensor:
        """``final_layer_norm`` of every row: what ``transformers`` calls the text model's ``last_hidden_state``"""
        return self._ln(hidden, "text_model.final_layer_norm")
