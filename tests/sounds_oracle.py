"""Numpy / torch-CPU restatement of K29 (Audio Spectrogram Transformer sound tagging): the fbank, the patch gather, the
network and the head.

Independent of the product and of ``transformers``: written from the steps in DESIGN.md "K29 sound events".
``tests/test_sounds_host.py`` pins the float64 fbank against ``ASTFeatureExtractor`` and the fp32 network against
``ASTForAudioClassification``.  ``Oracle(fp16=True)`` rounds to fp16 where the device stores fp16: matrix weights, the
patch rows, LayerNorm outputs that feed a GEMM (the classifier's included), q / k / v, attention outputs, GELU outputs, and
the softmax numerators of the attention.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

PATCH = 16
FRAME, SHIFT, NFFT = 400, 160, 512
MEL_FLOOR = 1.192092955078125e-07
MEAN, STD = -4.2677393, 4.5689974
PREFIX = "audio_spectrogram_transformer."


def config_s() -> dict:
    return {"mel": 32, "max_length": 48, "fstride": 10, "tstride": 10, "hidden": 128, "layers": 2, "heads": 2, "ffn": 256, "labels": 7,
            "ln_eps": 1e-12}


def config_r() -> dict:
    return {**config_s(), "mel": 40, "max_length": 70, "fstride": 8, "tstride": 12, "layers": 1}


def config_w(layers: int = 2) -> dict:
    return {"mel": 128, "max_length": 176, "fstride": 10, "tstride": 10, "hidden": 768, "layers": layers, "heads": 12, "ffn": 3072,
            "labels": 527, "ln_eps": 1e-12}


def config_l() -> dict:
    return {**config_s(), "mel": 128, "max_length": 1024, "layers": 1}


def grid(cfg: dict):
    """(frequency patches, time patches)"""
    return (cfg["mel"] - PATCH) // cfg["fstride"] + 1, (cfg["max_length"] - PATCH) // cfg["tstride"] + 1


def hf_config(cfg: dict) -> dict:
    """The ``config.json`` keys of a configuration above."""
    return {"hidden_size": cfg["hidden"], "num_hidden_layers": cfg["layers"], "num_attention_heads": cfg["heads"],
            "intermediate_size": cfg["ffn"], "hidden_act": "gelu", "layer_norm_eps": cfg["ln_eps"], "qkv_bias": True,
            "patch_size": PATCH, "frequency_stride": cfg["fstride"], "time_stride": cfg["tstride"], "max_length": cfg["max_length"],
            "num_mel_bins": cfg["mel"], "hidden_dropout_prob": 0.0, "attention_probs_dropout_prob": 0.0,
            "num_labels": cfg["labels"], "id2label": {str(i): f"LABEL_{i}" for i in range(cfg["labels"])}}


# ---- fbank --------------------------------------------------------------------------------------------------------------------
def hann(dtype=np.float64) -> np.ndarray:
    i = np.arange(FRAME, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * i / (FRAME - 1))).astype(dtype)


def mel_matrix(n_mels: int, dtype=np.float64) -> np.ndarray:
    """[257][n_mels]: triangles between 20 Hz and 8 kHz, equally spaced on mel = 1127 ln(1 + f / 700) and triangular there"""
    mel = lambda f: 1127.0 * np.log(1.0 + np.asarray(f, np.float64) / 700.0)  # noqa: E731
    edges = np.linspace(mel(20.0), mel(8000.0), n_mels + 2)
    centre = mel(np.arange(NFFT // 2 + 1) * (16000.0 / NFFT))
    out = np.zeros((NFFT // 2 + 1, n_mels))
    for j in range(n_mels):
        lo, mid, hi = edges[j], edges[j + 1], edges[j + 2]
        out[:, j] = np.maximum(0.0, np.minimum((centre - lo) / (mid - lo), (hi - centre) / (hi - mid)))
    return out.astype(dtype)


def fbank(samples: np.ndarray, first: int, valid: int, max_length: int, n_mels: int, dtype=np.float64, mean: float = MEAN,
          std: float = STD) -> np.ndarray:
    """One window's normalised log-mel spectrogram [max_length][n_mels] float32.  Frame j = samples first + 160 j .. + 399
    of the [-1, 1] waveform: mean removed, pre-emphasis 0.97, Hann, zero-padded to 512, |rfft|^2, the mel matrix, log(max(.,
    floor)), (x - mean) / (2 std), every step in ``dtype``, then one rounding to float32.  Rows from ``valid`` on are the
    normalised zero."""
    dt = np.dtype(dtype)
    cdt = np.complex128 if dt == np.float64 else np.complex64
    x = np.asarray(samples, np.float32).astype(dt)
    window, mel = hann(dt), mel_matrix(n_mels, dt)
    out = np.full((max_length, n_mels), (dt.type(0) - dt.type(mean)) / (dt.type(2) * dt.type(std)), dt)
    for j in range(valid):
        b = x[first + SHIFT * j:first + SHIFT * j + FRAME].copy()
        assert b.size == FRAME
        b = b - b.mean(dtype=dt)
        e = np.empty_like(b)
        e[1:] = b[1:] - dt.type(0.97) * b[:-1]
        e[0] = b[0] * (dt.type(1) - dt.type(0.97))
        buf = np.zeros(NFFT, dt)
        buf[:FRAME] = e * window
        spec = np.fft.rfft(buf).astype(cdt)
        power = (spec.real.astype(dt) ** 2 + spec.imag.astype(dt) ** 2).astype(dt)
        m = (power @ mel).astype(dt)
        out[j] = (np.log(np.maximum(m, dt.type(MEL_FLOOR))) - dt.type(mean)) / (dt.type(2) * dt.type(std))
    return out.astype(np.float32)


def fbank_plan(samples, plan, max_length, n_mels, dtype=np.float64) -> np.ndarray:
    return np.stack([fbank(samples, int(a), int(v), max_length, n_mels, dtype) for a, v in plan])


# ---- patches ------------------------------------------------------------------------------------------------------------------
def patch_rows(spec: np.ndarray, cfg: dict) -> np.ndarray:
    """[B][time][mel] -> [B][f t][256]: patch fi t + ti, element 16 df + dt = spec[tstride ti + dt][fstride fi + df]"""
    f, t = grid(cfg)
    B = spec.shape[0]
    out = np.empty((B, f * t, PATCH * PATCH), spec.dtype)
    for fi in range(f):
        for ti in range(t):
            blk = spec[:, cfg["tstride"] * ti:cfg["tstride"] * ti + PATCH, cfg["fstride"] * fi:cfg["fstride"] * fi + PATCH]  # b dt df
            out[:, fi * t + ti] = blk.transpose(0, 2, 1).reshape(B, -1)
    return out


# ---- weights ------------------------------------------------------------------------------------------------------------------
def random_weights(cfg: dict, seed: int, classifier_gain: float = 8.0) -> dict:
    """Seeded ``state_dict()`` of the exact shapes (torch tensors), in the current ``transformers`` layout."""
    g = torch.Generator().manual_seed(seed)
    d = cfg["hidden"]
    f, t = grid(cfg)
    w = {}

    def lin(name, out, inp, gain=1.0):
        w[name + ".weight"] = gain * torch.randn(out, inp, generator=g) / inp ** 0.5
        w[name + ".bias"] = 0.05 * torch.randn(out, generator=g)

    def lnorm(name):
        w[name + ".weight"] = 1.0 + 0.2 * (torch.rand(d, generator=g) - 0.5)
        w[name + ".bias"] = 0.05 * torch.randn(d, generator=g)

    e = PREFIX + "embeddings."
    w[e + "cls_token"] = 0.2 * torch.randn(1, 1, d, generator=g)
    w[e + "distillation_token"] = 0.2 * torch.randn(1, 1, d, generator=g)
    w[e + "position_embeddings"] = 0.2 * torch.randn(1, f * t + 2, d, generator=g)
    w[e + "patch_embeddings.projection.weight"] = torch.randn(d, 1, PATCH, PATCH, generator=g) / PATCH
    w[e + "patch_embeddings.projection.bias"] = 0.05 * torch.randn(d, generator=g)
    for layer in range(cfg["layers"]):
        p = f"{PREFIX}layers.{layer}."
        for proj in ("q_proj", "k_proj", "v_proj", "o_proj"):
            lin(p + "attention." + proj, d, d)
        lnorm(p + "layernorm_before")
        lnorm(p + "layernorm_after")
        lin(p + "mlp.fc1", cfg["ffn"], d)
        lin(p + "mlp.fc2", d, cfg["ffn"])
    lnorm(PREFIX + "layernorm")
    lnorm("classifier.layernorm")
    lin("classifier.dense", cfg["labels"], d, classifier_gain)
    return w


def old_layout(weights: dict) -> dict:
    """The same tensors under the published checkpoint's older names."""
    ren = (("attention.q_proj.", "attention.attention.query."), ("attention.k_proj.", "attention.attention.key."),
           ("attention.v_proj.", "attention.attention.value."), ("attention.o_proj.", "attention.output.dense."),
           ("mlp.fc1.", "intermediate.dense."), ("mlp.fc2.", "output.dense."))
    out = {}
    for k, v in weights.items():
        if k.startswith(PREFIX + "layers."):
            k = PREFIX + "encoder.layer." + k[len(PREFIX + "layers."):]
            for a, b in ren:
                k = k.replace(a, b)
        out[k] = v
    return out


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
        return F.layer_norm(x, (x.shape[-1],), self.w[name + ".weight"], self.w[name + ".bias"], self.cfg["ln_eps"])

    def _lin(self, x, name):
        return x @ self.w[name + ".weight"].T + self.w[name + ".bias"]

    @torch.no_grad()
    def embed(self, rows: np.ndarray) -> torch.Tensor:
        """(B, P, 256) patch rows -> tokens [B][P + 2][d]: CLS, the distillation token, the patches, each with its position"""
        w, e = self.w, PREFIX + "embeddings."
        x = self.r(torch.from_numpy(np.ascontiguousarray(rows)).float())
        B = x.shape[0]
        tok = x @ w[e + "patch_embeddings.projection.weight"].reshape(-1, PATCH * PATCH).T + w[e + "patch_embeddings.projection.bias"]
        head = torch.cat([w[e + "cls_token"], w[e + "distillation_token"]], 1).expand(B, -1, -1)
        return torch.cat([head, tok], 1) + w[e + "position_embeddings"]

    @torch.no_grad()
    def forward(self, rows: np.ndarray):
        """(B, P, 256) patch rows -> ``(hidden [B][P + 2][d] before the final LayerNorm, logits [B][labels])``"""
        x = self.embed(rows)
        B, n, d = x.shape
        heads = self.cfg["heads"]
        for layer in range(self.cfg["layers"]):
            p = f"{PREFIX}layers.{layer}."
            h = self.r(self._ln(x, p + "layernorm_before"))
            q, k, v = (self.r(self._lin(h, p + "attention." + s)).view(B, n, heads, 64).transpose(1, 2)
                       for s in ("q_proj", "k_proj", "v_proj"))
            s = (q @ k.transpose(-1, -2)) * 0.125
            if self.fp16:
                pr = self.r(torch.exp(s - s.amax(-1, keepdim=True)))
                a = (pr @ v) / pr.sum(-1, keepdim=True)
            else:
                a = torch.softmax(s, dim=-1) @ v
            a = self.r(a.transpose(1, 2).reshape(B, n, d))
            x = x + self._lin(a, p + "attention.o_proj")
            h = self.r(self._ln(x, p + "layernorm_after"))
            mid = self.r(F.gelu(self._lin(h, p + "mlp.fc1")))
            x = x + self._lin(mid, p + "mlp.fc2")
        seq = self._ln(x[:, :2], PREFIX + "layernorm")
        pooled = (seq[:, 0] + seq[:, 1]) / 2
        logits = self._lin(self.r(self._ln(pooled, "classifier.layernorm")), "classifier.dense")
        return x, logits


def sigmoid_topk(logits: np.ndarray, top_k: int):
    """``(scores (n, top_k) float32, ids (n, top_k) int32)``: the ``top_k`` largest logits in a stable descending sort (ties
    to the smaller index) and their sigmoids, taken in float64 and rounded to float32 once."""
    logits = np.asarray(logits, np.float32)
    ids = np.argsort(-logits, axis=-1, kind="stable")[:, :top_k]
    top = np.take_along_axis(logits, ids, -1).astype(np.float64)
    return (1.0 / (1.0 + np.exp(-top))).astype(np.float32), ids.astype(np.int32)


def audio(n_samples: int, seed: int) -> np.ndarray:
    """Synthetic float32 audio: three sines whose pitch and loudness drift, plus seeded noise; amplitude about 0.2."""
    rng = np.random.default_rng(seed)
    t = np.arange(n_samples) / 16000.0
    x = 0.02 * rng.standard_normal(n_samples)
    for f0, amp, wob in ((220.0, 0.08, 0.31), (1330.0, 0.06, 0.57), (4100.0, 0.04, 0.83)):
        x += amp * (1.0 + 0.5 * np.sin(2 * np.pi * wob * t + f0)) * np.sin(2 * np.pi * f0 * t * (1.0 + 0.02 * np.sin(2 * np.pi * wob * t)))
    return x.astype(np.float32)


def steady_audio(seconds: int, seed: int, ramp: float = 0.1) -> np.ndarray:
    """Float32 audio that repeats every second (three modulated sines whose periods divide one second, plus one second of
    seeded noise) under a gain that rises by ``ramp`` over the file: windows a whole number of seconds apart differ only
    slightly, so a model's logits do, too."""
    rng = np.random.default_rng(seed)
    t = np.arange(16000) / 16000.0
    one = 0.02 * rng.standard_normal(16000)
    for f0, amp, wob in ((220.0, 0.08, 1.0), (1330.0, 0.06, 2.0), (4100.0, 0.04, 3.0)):
        one += amp * (1.0 + 0.5 * np.sin(2 * np.pi * wob * t + f0)) * np.sin(2 * np.pi * f0 * t)
    x = np.tile(one, seconds)
    return (x * (1.0 + ramp * np.arange(x.size) / x.size)).astype(np.float32)
