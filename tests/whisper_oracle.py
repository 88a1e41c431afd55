"""CPU oracle for K19 / K20 (Whisper): log-mel, network, logit rules and the greedy loop in plain numpy / torch-CPU.

Two modes.  ``fp16=False`` is the fp32 model.  ``fp16=True`` rounds to fp16 where ``csrc/whisper.hip`` does: the weights of
every linear / conv layer and the token embedding, the mel input, LayerNorm outputs, q / k / v, attention outputs and GELU
outputs; biases, LayerNorm parameters, both position tables, the residual stream, softmax and every accumulation stay
fp32.  Nothing here imports the product or ``transformers``.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

N_FFT, HOP, N_BINS = 400, 160, 201


# ---- configs of the four test models ------------------------------------------------------------------------------------
def model_a_config() -> dict:
    """d 128, 2 heads, 2 + 2 layers, ffn 512, ctx 100 (200-frame windows), 1003 ids with a layout of its own."""
    return {"n_mels": 80, "d_model": 128, "heads": 2, "enc_layers": 2, "dec_layers": 2, "enc_ffn": 512, "dec_ffn": 512,
            "vocab": 1003, "max_source_positions": 100, "max_target_positions": 64,
            "sot": 891, "eot": 890, "lang_ids": [892, 893, 894, 895], "lang_codes": ["en", "de", "fr", "ja"], "translate": 896,
            "transcribe": 897, "no_speech": 900, "no_timestamps": 901, "timestamp_begin": 902,
            "max_initial_timestamp_index": 50, "suppress": [1, 7, 300, 891, 892, 893, 894, 895, 896, 897, 898, 899, 900],
            "begin_suppress": [5, 890]}


def model_b_config() -> dict:
    """The same widths with the real multilingual layout: 51865 ids, ctx 1500."""
    return {"n_mels": 80, "d_model": 128, "heads": 2, "enc_layers": 2, "dec_layers": 2, "enc_ffn": 512, "dec_ffn": 512,
            "vocab": 51865, "max_source_positions": 1500, "max_target_positions": 448,
            "sot": 50258, "eot": 50257, "lang_ids": list(range(50259, 50358)), "lang_codes": [f"l{i}" for i in range(99)],
            "translate": 50358, "transcribe": 50359, "no_speech": 50362, "no_timestamps": 50363, "timestamp_begin": 50364,
            "max_initial_timestamp_index": 50,
            "suppress": [1, 2, 7, 8, 9, 10, 14, 25, 26, 27, 28, 29, 31, 58, 59, 60, 61, 62, 63, 90, 91, 92, 93, 359, 503, 522,
                         50258, 50358, 50359, 50360, 50361, 50362] + list(range(50259, 50358)),
            "begin_suppress": [220, 50257]}


def model_c_config() -> dict:
    """The large-v3 id layout (51866 ids, 100 languages, 128 mel bins, every special id one above model B's) at the narrowest
    real width: d 384 (256 threads take a second, partial trip over it), 6 heads, 2 + 3 layers, ffn 1536 / 768, ctx 200."""
    return {"n_mels": 128, "d_model": 384, "heads": 6, "enc_layers": 2, "dec_layers": 3, "enc_ffn": 1536, "dec_ffn": 768,
            "vocab": 51866, "max_source_positions": 200, "max_target_positions": 448,
            "sot": 50258, "eot": 50257, "lang_ids": list(range(50259, 50359)),
            "lang_codes": ["en"] + [f"l{i}" for i in range(1, 100)],
            "translate": 50359, "transcribe": 50360, "no_speech": 50363, "no_timestamps": 50364, "timestamp_begin": 50365,
            "max_initial_timestamp_index": 50,
            "suppress": [t for t in model_b_config()["suppress"] if t < 50257] + [50258, 50359, 50360, 50361, 50362, 50363]
                        + list(range(50259, 50359)),
            "begin_suppress": [220, 50257]}


def model_d_config() -> dict:
    """Model A's id layout and ctx at large-v3's widths: d 1280, 20 heads, 128 mel bins, 1 + 1 layers, ffn 5120."""
    return {**model_a_config(), "n_mels": 128, "d_model": 1280, "heads": 20, "enc_layers": 1, "dec_layers": 1,
            "enc_ffn": 5120, "dec_ffn": 5120}


# ---- log-mel ------------------------------------------------------------------------------------------------------------
def mel_filters(n_mels: int, sr: int = 16000) -> np.ndarray:
    """Slaney mel filterbank [n_mels][201], float64 (librosa.filters.mel(norm="slaney"), restated)."""
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0

    def hz_to_mel(f):
        f = np.asarray(f, dtype=np.float64)
        return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, f / f_sp)

    def mel_to_hz(m):
        m = np.asarray(m, dtype=np.float64)
        return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)

    fft_freqs = np.linspace(0.0, sr / 2.0, N_BINS)
    hz = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(sr / 2.0), n_mels + 2))
    fdiff = np.diff(hz)
    ramps = hz[:, None] - fft_freqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    return w * (2.0 / (hz[2:n_mels + 2] - hz[:n_mels]))[:, None]


def log_mel(samples: np.ndarray, offset: int, n_frames: int, n_mels: int) -> np.ndarray:
    """One window: [n_mels][n_frames] float32, every stage before the final cast in float64."""
    n = n_frames * HOP
    chunk = np.zeros(n, dtype=np.float64)
    part = np.asarray(samples[offset:offset + n], dtype=np.float64)
    chunk[:len(part)] = part
    padded = np.pad(chunk, N_FFT // 2, mode="reflect")
    window = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)
    idx = np.arange(n_frames)[:, None] * HOP + np.arange(N_FFT)[None, :]
    spec = np.fft.rfft(padded[idx] * window[None, :], axis=1)
    power = spec.real ** 2 + spec.imag ** 2                      # [T][201]
    mel = mel_filters(n_mels) @ power.T                         # [n_mels][T]
    log_spec = np.log10(np.maximum(mel, 1e-10))
    log_spec = np.maximum(log_spec, log_spec.max() - 8.0)
    return ((log_spec + 4.0) / 4.0).astype(np.float32)


# ---- weights --------------------------------------------------------------------------------------------------------------
def sinusoids(length: int, channels: int) -> torch.Tensor:
    inc = math.log(10000.0) / (channels // 2 - 1)
    inv = torch.exp(-inc * torch.arange(channels // 2, dtype=torch.float32))
    t = torch.arange(length, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.cat([t.sin(), t.cos()], dim=1)


def random_weights(cfg: dict, seed: int, boost: dict | None = None, qk_scale: float = 4.0) -> dict:
    """He-scaled linear weights, embeddings std 0.1, q / k projections x 4, LayerNorm gains 1 +- 0.1, biases std 0.1 - the
    recipe under which random weights decode audio-dependent, varied tokens.  ``boost`` {id: amount} raises embedding rows
    along the final LayerNorm's bias direction, which makes those ids (EOT, timestamps) likelier at every step.  ``qk_scale``
    below 4 softens every softmax: rounding errors of q and k are amplified less."""
    g = torch.Generator().manual_seed(seed)
    d = cfg["d_model"]
    w: dict[str, torch.Tensor] = {}

    def lin(name, out, inp, bias=True, scale=1.0):
        w[name + ".weight"] = torch.randn(out, inp, generator=g) * (math.sqrt(2.0 / inp) * scale)
        if bias:
            w[name + ".bias"] = torch.randn(out, generator=g) * 0.1

    def lnorm(name):
        w[name + ".weight"] = 1.0 + (torch.rand(d, generator=g) * 0.2 - 0.1)
        w[name + ".bias"] = torch.randn(d, generator=g) * 0.1

    def attn(p, lnp):
        lin(p + "q_proj", d, d, scale=qk_scale)
        lin(p + "k_proj", d, d, bias=False, scale=qk_scale)
        lin(p + "v_proj", d, d)
        lin(p + "out_proj", d, d)
        lnorm(lnp)

    w["model.encoder.conv1.weight"] = torch.randn(d, cfg["n_mels"], 3, generator=g) * math.sqrt(2.0 / (3 * cfg["n_mels"]))
    w["model.encoder.conv1.bias"] = torch.randn(d, generator=g) * 0.1
    w["model.encoder.conv2.weight"] = torch.randn(d, d, 3, generator=g) * math.sqrt(2.0 / (3 * d))
    w["model.encoder.conv2.bias"] = torch.randn(d, generator=g) * 0.1
    w["model.encoder.embed_positions.weight"] = sinusoids(cfg["max_source_positions"], d)
    for side, n, ffn in (("encoder", cfg["enc_layers"], cfg["enc_ffn"]), ("decoder", cfg["dec_layers"], cfg["dec_ffn"])):
        for i in range(n):
            p = f"model.{side}.layers.{i}."
            attn(p + "self_attn.", p + "self_attn_layer_norm")
            if side == "decoder":
                attn(p + "encoder_attn.", p + "encoder_attn_layer_norm")
            lin(p + "fc1", ffn, d)
            lin(p + "fc2", d, ffn)
            lnorm(p + "final_layer_norm")
        lnorm(f"model.{side}.layer_norm")
    w["model.decoder.embed_tokens.weight"] = torch.randn(cfg["vocab"], d, generator=g) * 0.1
    w["model.decoder.embed_positions.weight"] = torch.randn(cfg["max_target_positions"], d, generator=g) * 0.1
    if boost:
        b = w["model.decoder.layer_norm.bias"]
        direction = b / b.norm()
        for tok, amount in boost.items():
            w["model.decoder.embed_tokens.weight"][tok] += amount * direction
    return w


# ---- the network ----------------------------------------------------------------------------------------------------------
class Oracle:
    def __init__(self, cfg: dict, weights: dict, fp16: bool):
        self.cfg, self.fp16 = cfg, fp16
        self.w = {}
        for k, v in weights.items():
            v = v.detach().float().clone()
            matrix = k.endswith(".weight") and v.dim() >= 2 and "embed_positions" not in k
            self.w[k] = v.half().float() if (fp16 and matrix) else v

    def r(self, t: torch.Tensor) -> torch.Tensor:
        return t.half().float() if self.fp16 else t

    def _ln(self, x, name):
        return self.r(F.layer_norm(x, (x.shape[-1],), self.w[name + ".weight"], self.w[name + ".bias"], 1e-5))

    def _lin(self, x, name):
        b = self.w.get(name + ".bias")
        y = x @ self.w[name + ".weight"].T
        return y + b if b is not None else y

    def _attend(self, q, k, v, causal: bool):
        """q [B][Tq][d], k / v [B][Tk][d] (already rounded) -> rounded [B][Tq][d]"""
        B, Tq, d = q.shape
        h = self.cfg["heads"]
        qh = q.view(B, Tq, h, 64).transpose(1, 2)
        kh = k.view(B, -1, h, 64).transpose(1, 2)
        vh = v.view(B, -1, h, 64).transpose(1, 2)
        s = (qh @ kh.transpose(-1, -2)) * 0.125
        if causal:
            s = s + torch.full((Tq, Tq), float("-inf")).triu(1)
        a = torch.softmax(s, dim=-1) @ vh
        return self.r(a.transpose(1, 2).reshape(B, Tq, d))

    def _block(self, x, p, enc_kv=None, causal=False):
        h = self._ln(x, p + "self_attn_layer_norm")
        q, k, v = (self.r(self._lin(h, p + f"self_attn.{n}_proj")) for n in "qkv")
        x = x + self._lin(self._attend(q, k, v, causal), p + "self_attn.out_proj")
        if enc_kv is not None:
            h = self._ln(x, p + "encoder_attn_layer_norm")
            q = self.r(self._lin(h, p + "encoder_attn.q_proj"))
            x = x + self._lin(self._attend(q, enc_kv[0], enc_kv[1], False), p + "encoder_attn.out_proj")
        h = self._ln(x, p + "final_layer_norm")
        mid = self.r(F.gelu(self._lin(h, p + "fc1")))
        return x + self._lin(mid, p + "fc2")

    @torch.no_grad()
    def encode(self, mel: np.ndarray) -> torch.Tensor:
        """mel [B][n_mels][2 ctx] float32 -> the encoder's final LayerNorm output [B][ctx][d]"""
        x = self.r(torch.from_numpy(np.ascontiguousarray(mel)).float())
        w = self.w
        x = self.r(F.gelu(F.conv1d(x, w["model.encoder.conv1.weight"], w["model.encoder.conv1.bias"], padding=1)))
        x = F.gelu(F.conv1d(x, w["model.encoder.conv2.weight"], w["model.encoder.conv2.bias"], stride=2, padding=1))
        x = x.transpose(1, 2) + w["model.encoder.embed_positions.weight"][None]
        for i in range(self.cfg["enc_layers"]):
            x = self._block(x, f"model.encoder.layers.{i}.")
        return self._ln(x, "model.encoder.layer_norm")

    @torch.no_grad()
    def cross_kv(self, enc: torch.Tensor):
        out = []
        for i in range(self.cfg["dec_layers"]):
            p = f"model.decoder.layers.{i}.encoder_attn."
            out.append((self.r(self._lin(enc, p + "k_proj")), self.r(self._lin(enc, p + "v_proj"))))
        return out

    @torch.no_grad()
    def forced_logits(self, enc: torch.Tensor, ids, kv=None) -> torch.Tensor:
        """Teacher-forced, rule-free logits [B][T][vocab] for ids [B][T]."""
        ids = torch.as_tensor(np.asarray(ids), dtype=torch.long)
        kv = kv if kv is not None else self.cross_kv(enc)
        T = ids.shape[1]
        x = self.w["model.decoder.embed_tokens.weight"][ids] + self.w["model.decoder.embed_positions.weight"][:T][None]
        for i in range(self.cfg["dec_layers"]):
            x = self._block(x, f"model.decoder.layers.{i}.", enc_kv=kv[i], causal=True)
        return self._ln(x, "model.decoder.layer_norm") @ self.w["model.decoder.embed_tokens.weight"].T

    @torch.no_grad()
    def greedy(self, enc: torch.Tensor, prompt: list[int], max_new: int) -> list[dict]:
        """Greedy decode of every window of ``enc``.  Per lane: tokens (EOT-filled to max_new), n (sampled up to and
        including EOT), sum_logprob, no_speech_prob, lang (id), margins (per sampled step, see ``select``), logits (the
        rule-free logits of each sampled step)."""
        cfg = self.cfg
        out = []
        for b in range(enc.shape[0]):
            e = enc[b:b + 1]
            kv = self.cross_kv(e)
            ids, sampled, margins, step_logits = list(prompt), [], [], []
            total, done, nsp, lang, lang_margin = 0.0, False, None, None, None
            for i in range(max_new):
                if done:
                    sampled.append(cfg["eot"])
                    continue
                lg = self.forced_logits(e, [ids], kv)[0].double().numpy()
                if nsp is None:
                    first = lg[0]
                    nsp = float(np.exp(first[cfg["no_speech"]] - _lse(first)))
                    lang = int(cfg["lang_ids"][int(np.argmax(first[cfg["lang_ids"]]))])
                    lang_margin = float(np.diff(np.sort(first[cfg["lang_ids"]])[-2:])[0])
                tok, lp, margin = select(apply_rules(lg[-1], sampled, cfg), cfg)
                step_logits.append(lg[-1])
                margins.append(margin)
                sampled.append(tok)
                ids.append(tok)
                total += lp
                done = tok == cfg["eot"]
            n = sampled.index(cfg["eot"]) + 1 if cfg["eot"] in sampled else len(sampled)
            out.append({"tokens": sampled, "n": n, "sum_logprob": total, "no_speech_prob": nsp, "lang": lang,
                        "lang_margin": lang_margin, "margins": margins, "logits": step_logits})
        return out


# ---- logit rules ----------------------------------------------------------------------------------------------------------
def _lse(v: np.ndarray) -> float:
    v = np.asarray(v, dtype=np.float64)
    m = v.max()
    if not np.isfinite(m):
        return float("-inf")
    return float(m + np.log(np.exp(v - m).sum()))


def apply_rules(logits: np.ndarray, sampled: list[int], cfg: dict) -> np.ndarray:
    """Rules 1-6 of the issue on one lane's logits; ``sampled`` are the tokens sampled so far (the prompt excluded)."""
    z = np.array(logits, dtype=np.float64)
    tb, eot, ninf = cfg["timestamp_begin"], cfg["eot"], float("-inf")
    z[cfg["suppress"]] = ninf                                              # 1
    if len(sampled) == 0:
        z[cfg["begin_suppress"]] = ninf                                    # 2
    z[cfg["no_timestamps"]] = ninf                                         # 3
    last_ts = len(sampled) >= 1 and sampled[-1] >= tb
    pen_ts = len(sampled) < 2 or sampled[-2] >= tb
    if last_ts:                                                            # 5
        if pen_ts:
            z[tb:] = ninf
        else:
            z[:eot] = ninf
    stamps = [t for t in sampled if t >= tb]
    if stamps:                                                             # 6
        limit = stamps[-1] if (last_ts and not pen_ts) else stamps[-1] + 1
        z[tb:limit] = ninf
    if len(sampled) == 0:                                                  # 4
        z[:tb] = ninf
        if cfg["max_initial_timestamp_index"] is not None:
            z[tb + cfg["max_initial_timestamp_index"] + 1:] = ninf
    return z


def text_suppressed(masked: np.ndarray, cfg: dict) -> bool:
    """Rule 7: the probability mass on all timestamps exceeds the largest single text-token probability."""
    tb = cfg["timestamp_begin"]
    return _lse(masked[tb:]) > masked[:tb].max()


def select(masked: np.ndarray, cfg: dict):
    """(token, its log-probability under the final masked distribution, margin).  The margin is the smallest gap a
    perturbation of the logits would have to close to change the token: the gap between the two best remaining candidates
    and, where both sides are finite, the gap of the rule-7 comparison."""
    tb = cfg["timestamp_begin"]
    z = masked.copy()
    lse_ts, max_text = _lse(z[tb:]), z[:tb].max()
    if lse_ts > max_text:
        z[:tb] = float("-inf")
    tok = int(np.argmax(z))  # the first maximum: the lower id wins a tie
    top = np.sort(z[np.isfinite(z)])[-2:]
    margin = float(top[1] - top[0]) if len(top) == 2 else float("inf")
    if np.isfinite(lse_ts) and np.isfinite(max_text):
        margin = min(margin, abs(lse_ts - max_text))
    return tok, float(z[tok] - _lse(z)), margin


# ---- scripted cases shared by the host and GPU rule tests -----------------------------------------------------------------
def scripted_prefixes(cfg: dict) -> dict[str, list[int]]:
    """Sampled-token prefixes that put every rule in force: first position, after one timestamp, after text, after text +
    one timestamp, after a pair, after a pair + text."""
    tb = cfg["timestamp_begin"]
    return {"first": [], "one_timestamp": [tb + 3], "after_text": [tb + 3, 10, 11], "text_then_timestamp": [tb + 3, 10, 11, tb + 20],
            "after_pair": [tb + 3, 10, tb + 20, tb + 20], "pair_then_text": [tb + 3, 10, tb + 20, tb + 20, 12]}


def scripted_logits(cfg: dict, seed: int, timestamp_shift: float) -> np.ndarray:
    """Random logits [vocab] float32; ``timestamp_shift`` moves every timestamp logit, which decides rule 7 either way."""
    z = np.random.default_rng(seed).standard_normal(cfg["vocab"]).astype(np.float32) * 3.0
    z[cfg["timestamp_begin"]:] += np.float32(timestamp_shift)
    return z
