"""CPU oracle for K22 (Silero VAD, 16 kHz branch): the network restated in torch on the CPU, float64 by default.

Built from ``F.pad(mode="reflect")``, ``F.conv1d`` and explicit LSTM-cell arithmetic; it imports nothing from the product.
``dtype=torch.float32`` is the fp32 mode: the same graph in the device's number format, the yardstick for how much of a
device-vs-float64 difference is plain fp32 rounding.  Also here: the seeded weights and the audio the tests share.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

WINDOW, CONTEXT = 512, 64
SHAPES = {"stft.forward_basis_buffer": (258, 1, 256),
          "encoder.0.weight": (128, 129, 3), "encoder.0.bias": (128,), "encoder.1.weight": (64, 128, 3), "encoder.1.bias": (64,),
          "encoder.2.weight": (64, 64, 3), "encoder.2.bias": (64,), "encoder.3.weight": (128, 64, 3), "encoder.3.bias": (128,),
          "decoder.rnn.weight_ih": (512, 128), "decoder.rnn.weight_hh": (512, 128), "decoder.rnn.bias_ih": (512,),
          "decoder.rnn.bias_hh": (512,), "decoder.out.weight": (1, 128, 1), "decoder.out.bias": (1,)}
STRIDES = (1, 2, 2, 1)


def random_weights(seed: int) -> dict[str, np.ndarray]:
    """Seeded fp32 weights in the checkpoint's shapes.  The STFT basis is a Hann-windowed 256-point DFT; the rest is scaled
    so that activations neither die nor saturate on the test audio and the output moves on both sides of 0.5."""
    rng = np.random.default_rng(seed)
    n = np.arange(256, dtype=np.float64)
    ang = 2 * np.pi * np.arange(129, dtype=np.float64)[:, None] * n / 256
    basis = np.concatenate([np.cos(ang), -np.sin(ang)]) * (0.5 - 0.5 * np.cos(2 * np.pi * n / 256))
    out = {"stft.forward_basis_buffer": basis.reshape(258, 1, 256).astype(np.float32)}
    for name, shape in SHAPES.items():
        if name in out:
            continue
        if name == "decoder.out.bias":
            w = -1.0 + 0.1 * rng.standard_normal(shape)       # silence sits well below both thresholds
        elif name.endswith("bias") or "bias_" in name:
            w = 0.1 * rng.standard_normal(shape)
        elif name == "decoder.out.weight":
            w = 0.6 * rng.standard_normal(shape)
        else:
            fan_in = int(np.prod(shape[1:]))
            w = rng.standard_normal(shape) * math.sqrt((2.0 if name.startswith("encoder") else 1.5) / fan_in)
        out[name] = w.astype(np.float32)
    return out


def burst_audio(seed: int, n_samples: int, bursts) -> np.ndarray:
    """Zeros with seeded noise bursts: ``bursts`` = [(first sample, last sample + 1, amplitude)]."""
    rng = np.random.default_rng(seed)
    x = np.zeros(n_samples, dtype=np.float32)
    for a, b, amp in bursts:
        x[a:b] = (amp * rng.standard_normal(b - a)).astype(np.float32)
    return x


class Oracle:
    def __init__(self, weights: dict[str, np.ndarray], dtype=torch.float64):
        self.dtype = dtype
        self.w = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)).reshape(SHAPES[k]).to(dtype) for k, v in weights.items()}

    def features(self, x: torch.Tensor) -> torch.Tensor:
        """x [B][576] (context + chunk) -> LSTM input [B][128]."""
        w = self.w
        xp = F.pad(x.unsqueeze(1), (0, 64), mode="reflect")                      # [B][1][640]
        spec = F.conv1d(xp, w["stft.forward_basis_buffer"], stride=128)           # [B][258][4]
        y = torch.sqrt(spec[:, :129] ** 2 + spec[:, 129:] ** 2)
        for i, s in enumerate(STRIDES):
            y = F.relu(F.conv1d(y, w[f"encoder.{i}.weight"], w[f"encoder.{i}.bias"], stride=s, padding=1))
        assert y.shape[1:] == (128, 1)
        return y[:, :, 0]

    def probs(self, samples: np.ndarray, context: np.ndarray | None = None) -> np.ndarray:
        """One probability per chunk of 512 samples; the tail is padded with ``512 - n % 512`` zeros (a whole chunk of
        zeros when n is a multiple of 512).  ``context``: the 64 samples before the first chunk (None = zeros)."""
        w = self.w
        x = torch.from_numpy(np.asarray(samples, dtype=np.float32)).to(self.dtype)
        x = F.pad(x, (0, WINDOW - x.numel() % WINDOW))
        first = torch.zeros(CONTEXT, dtype=self.dtype) if context is None else torch.from_numpy(np.asarray(context, np.float32)).to(self.dtype)
        x = torch.cat([first, x])
        n = (x.numel() - CONTEXT) // WINDOW
        frames = torch.stack([x[i * WINDOW:i * WINDOW + WINDOW + CONTEXT] for i in range(n)])
        gx = self.features(frames) @ w["decoder.rnn.weight_ih"].T + w["decoder.rnn.bias_ih"] + w["decoder.rnn.bias_hh"]
        h = torch.zeros(128, dtype=self.dtype)
        c = torch.zeros(128, dtype=self.dtype)
        out = []
        for t in range(n):
            g = gx[t] + w["decoder.rnn.weight_hh"] @ h
            i_, f_, g_, o_ = torch.sigmoid(g[:128]), torch.sigmoid(g[128:256]), torch.tanh(g[256:384]), torch.sigmoid(g[384:])
            c = f_ * c + i_ * g_
            h = o_ * torch.tanh(c)
            out.append(torch.sigmoid((w["decoder.out.weight"].reshape(128) * F.relu(h)).sum() + w["decoder.out.bias"][0]))
        return torch.stack(out).to(torch.float64).numpy()
