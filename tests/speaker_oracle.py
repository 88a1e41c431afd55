"""CPU restatement of K24 (speaker labels, csrc/speakers.hip): Kaldi fbank + CMN as WeSpeaker calls it (float64, and an
all-float32 mode whose distance from the float64 one sets the feature test's bar), the WeSpeaker ResNet in torch fp32 with
the masked statistics pooling, the segment mean and the noise reassignment.

[PUBLIC-LIB] restated from the public Kaldi / WeSpeaker sources; nothing here reads eioku_amd.speakers' tables.
"""
from __future__ import annotations

import numpy as np

RATE, FRAME, SHIFT, N_FFT, N_BINS, N_MEL = 16000, 400, 160, 512, 256, 80
WIDTHS = (32, 64, 128, 256)
FLOOR = float(np.finfo(np.float32).eps)   # 1.1920929e-07
BN_EPS = 1e-5


# ---- test signals ---------------------------------------------------------------------------------------------------
def voice(seed: int, f0: float, formants, n: int, noise: float = 0.01) -> np.ndarray:
    """A seeded harmonic 'voice': harmonics of a slowly wandering ``f0`` weighted by resonances at ``formants``, with a
    syllable-rate envelope, plus white noise.  float32, peak about 0.3."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / RATE
    pitch = f0 * (1.0 + 0.04 * np.sin(2 * np.pi * 0.7 * t + rng.uniform(0, 6.28)))
    phase = 2 * np.pi * np.cumsum(pitch) / RATE
    x = np.zeros(n)
    for h in range(1, int(7000 // f0)):
        f = h * f0
        gain = sum(1.0 / (1.0 + ((f - fc) / bw) ** 2) for fc, bw in formants) / h ** 0.5
        x += gain * np.sin(h * phase + rng.uniform(0, 6.28))
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t + rng.uniform(0, 6.28))
    x = 0.3 * x * env / np.abs(x).max()
    return (x + noise * rng.standard_normal(n)).astype(np.float32)


VOICES = ((110.0, ((700, 120), (1200, 150), (2600, 250))), (205.0, ((350, 90), (2100, 200), (3000, 300))),
          (155.0, ((500, 100), (1500, 180), (2500, 220))))


# ---- K24a -----------------------------------------------------------------------------------------------------------
def povey(dtype=np.float64) -> np.ndarray:
    n = np.arange(FRAME, dtype=np.float64)
    return ((0.5 - 0.5 * np.cos(2 * np.pi * n / (FRAME - 1))) ** 0.85).astype(dtype)


def mel_scale(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, np.float64) / 700.0)


def mel_banks(dtype=np.float64) -> np.ndarray:
    """Kaldi MelBanks: 80 triangles between 20 Hz and 8000 Hz over FFT bins 0..255, linear in mel."""
    lo, hi = mel_scale(20.0), mel_scale(8000.0)
    delta = (hi - lo) / (N_MEL + 1)
    out = np.zeros((N_MEL, N_BINS))
    for j in range(N_MEL):
        left, centre, right = lo + j * delta, lo + (j + 1) * delta, lo + (j + 2) * delta
        for i in range(N_BINS):
            m = mel_scale(i * RATE / N_FFT)
            if left < m < right:
                out[j, i] = (m - left) / (centre - left) if m <= centre else (right - m) / (right - centre)
    return out.astype(dtype)


_TABLES = {}


def _tables(dtype):
    if dtype not in _TABLES:
        ang = 2 * np.pi * np.outer(np.arange(N_BINS), np.arange(FRAME)) / N_FFT
        _TABLES[dtype] = (povey(dtype), mel_banks(dtype), np.cos(ang).astype(dtype), np.sin(ang).astype(dtype))
    return _TABLES[dtype]


def fbank_cmn(samples: np.ndarray, first: int, valid: int, dtype=np.float64) -> np.ndarray:
    """One window: ``(80, valid)`` log-mel with CMN; every operation in ``dtype`` (the DFT of the zero-padded frame is a
    matrix product with the cosine / sine tables over its 400 samples)."""
    window, banks, cos_t, sin_t = _tables(dtype)
    idx = first + SHIFT * np.arange(valid)[:, None] + np.arange(FRAME)[None, :]
    x = np.asarray(samples, np.float32)[idx].astype(dtype) * dtype(32768.0)
    x = x - x.mean(axis=1, keepdims=True, dtype=dtype)
    prev = np.concatenate([x[:, :1], x[:, :-1]], axis=1)
    x = (x - dtype(0.97) * prev) * window
    re, im = x @ cos_t.T, x @ sin_t.T
    power = re * re + im * im
    logmel = np.log(np.maximum(power @ banks.T, dtype(FLOOR)))                 # (valid, 80)
    # the mean over the frames, in frame order, as offsets from frame 0: a constant row has mean exactly itself
    acc = np.zeros(N_MEL, dtype)
    for t in range(valid):
        acc = acc + (logmel[t] - logmel[0])
    mean = logmel[0] + acc / dtype(valid)
    return np.ascontiguousarray((logmel - mean).T.astype(dtype))


def features(samples, plan, win: int, dtype=np.float64) -> np.ndarray:
    """``plan`` rows (first sample, valid) -> ``(m, 80, win)``, zero from ``valid`` on."""
    out = np.zeros((len(plan), N_MEL, win), dtype)
    for i, (first, valid) in enumerate(plan):
        out[i, :, :valid] = fbank_cmn(samples, int(first), int(valid), dtype)
    return out


def network_input(feats: np.ndarray) -> np.ndarray:
    """float features ``(m, 80, win)`` -> the device's fp16 NHWC8 input ``(m, 80, win, 8)``."""
    out = np.zeros((*feats.shape, 8), np.float16)
    out[..., 0] = feats.astype(np.float32).astype(np.float16)
    return out


# ---- K24b / K24c ----------------------------------------------------------------------------------------------------
def depths_of(sd: dict) -> tuple:
    out = []
    for li in range(1, 5):
        b = 0
        while f"layer{li}.{b}.conv1.weight" in sd:
            b += 1
        out.append(b)
    return tuple(out)


def resnet(state_dict: dict):
    """torch fp32 WeSpeaker ``ResNet`` (eval mode, base width 32, BasicBlocks) with ``state_dict`` loaded strictly."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F

    class BasicBlock(nn.Module):
        def __init__(self, cin, planes, stride):
            super().__init__()
            self.conv1 = nn.Conv2d(cin, planes, 3, stride, 1, bias=False)
            self.bn1 = nn.BatchNorm2d(planes, eps=BN_EPS)
            self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
            self.bn2 = nn.BatchNorm2d(planes, eps=BN_EPS)
            self.shortcut = nn.Sequential()
            if stride != 1 or cin != planes:
                self.shortcut = nn.Sequential(nn.Conv2d(cin, planes, 1, stride, bias=False), nn.BatchNorm2d(planes, eps=BN_EPS))

        def forward(self, x):
            out = self.bn2(self.conv2(F.relu(self.bn1(self.conv1(x)))))
            return F.relu(out + self.shortcut(x))

    class ResNet(nn.Module):
        def __init__(self, depths):
            super().__init__()
            self.conv1 = nn.Conv2d(1, WIDTHS[0], 3, 1, 1, bias=False)
            self.bn1 = nn.BatchNorm2d(WIDTHS[0], eps=BN_EPS)
            cin = WIDTHS[0]
            for li, (planes, d) in enumerate(zip(WIDTHS, depths), start=1):
                blocks = [BasicBlock(cin if b == 0 else planes, planes, 2 if b == 0 and li > 1 else 1) for b in range(d)]
                setattr(self, f"layer{li}", nn.Sequential(*blocks))
                cin = planes
            self.seg_1 = nn.Linear(2 * WIDTHS[3] * (N_MEL // 8), 256)

        def blocks(self):
            return [b for li in range(1, 5) for b in getattr(self, f"layer{li}")]

        def stem(self, x):
            return F.relu(self.bn1(self.conv1(x)))

    net = ResNet(depths_of(state_dict))
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state_dict.items()}, strict=True)
    return net.eval()


def _twin_blocks(net, x, upto):
    """The network of ``net`` in the device's arithmetic: every BatchNorm folded into the conv before it (folded here, in
    float64, from the modules' own parameters), weights rounded to fp16, fp32 accumulation, and one rounding to fp16 wherever
    the device stores a tensor: relu(conv) of the stem and of conv1, the shortcut conv, and
    ``fp16(relu(fp16(conv2) + shortcut))``."""
    import torch
    import torch.nn.functional as F

    def h(t):
        return t.half().float()

    def conv(c, bn, t):
        s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        w = h((c.weight.double() * s[:, None, None, None]).float())
        return h(F.conv2d(t, w, (bn.bias.double() - bn.running_mean.double() * s).float(), stride=c.stride, padding=c.padding))

    x = h(F.relu(conv(net.conv1, net.bn1, x)))
    peak = float(x.abs().max())
    for i, blk in enumerate(net.blocks()):
        mid = h(F.relu(conv(blk.conv1, blk.bn1, x)))
        res = conv(blk.shortcut[0], blk.shortcut[1], x) if len(blk.shortcut) else x
        x = h(F.relu(conv(blk.conv2, blk.bn2, mid) + res))
        peak = max(peak, float(x.abs().max()))
        if i == upto:
            break
    return x, peak


def forward_blocks(net, x_f16: np.ndarray, upto: int | None = None, fp16: bool = False):
    """fp16 NHWC8 input -> ``(NHWC float64 output of block `upto` (None: the last), largest |activation| on the way)``.
    ``fp16=True``: the twin in the device's arithmetic (:func:`_twin_blocks`) instead of torch fp32."""
    import torch

    x = torch.from_numpy(x_f16[..., 0].astype(np.float32))[:, None]
    if fp16:
        with torch.no_grad():
            x, peak = _twin_blocks(net, x, upto)
        return x.permute(0, 2, 3, 1).numpy().astype(np.float64), peak
    with torch.no_grad():
        x = net.stem(x)
        peak = float(x.abs().max())
        for i, blk in enumerate(net.blocks()):
            x = blk(x)
            peak = max(peak, float(x.abs().max()))
            if i == upto:
                break
    return x.permute(0, 2, 3, 1).numpy().astype(np.float64), peak


def pooled(net, x_f16: np.ndarray, valid):
    """-> ``(statistics (m, 5120) in torch's column order, unnormalised vectors (m, 256), peak activation)``: mean and
    ``sqrt(unbiased variance + 1e-7)`` over each window's first ``ceil(valid / 8)`` columns, then ``seg_1``."""
    import torch

    y, peak = forward_blocks(net, x_f16)
    y = torch.from_numpy(y.astype(np.float32)).permute(0, 3, 1, 2)           # (m, C, F', T')
    stats = []
    for i, v in enumerate(valid):
        t = -(-int(v) // 8)
        z = y[i, :, :, :t].reshape(-1, t)
        stats.append(torch.cat([z.mean(dim=-1), torch.sqrt(z.var(dim=-1) + 1e-7)]))
    stats = torch.stack(stats)
    with torch.no_grad():
        emb = net.seg_1(stats)
    return stats.numpy().astype(np.float64), emb.numpy().astype(np.float64), peak


# ---- K24d -----------------------------------------------------------------------------------------------------------
def segment_vectors(window_vectors, seg_first) -> np.ndarray:
    w = np.asarray(window_vectors, np.float64)
    out = np.stack([w[a:b].mean(axis=0) for a, b in zip(seg_first[:-1], seg_first[1:])])
    return out / np.linalg.norm(out, axis=1, keepdims=True)


def assign(e, labels, assign_max: float):
    """float64: ``(labels with noise rows reassigned, centroids (k, d), per noise row (row, best, second best distance))``."""
    e = np.asarray(e, np.float64)
    labels = np.asarray(labels).astype(np.int64)
    k = int(labels.max()) + 1 if len(labels) and labels.max() >= 0 else 0
    cent = np.zeros((k, e.shape[1]))
    for j in range(k):
        s = e[labels == j].sum(axis=0)
        cent[j] = s / np.linalg.norm(s)
    out, margins = labels.copy(), []
    for i in np.nonzero(labels < 0)[0]:
        if k == 0:
            continue
        d = 1.0 - cent @ e[i]
        j = int(np.argmin(d))
        margins.append((int(i), float(d[j]), float(np.sort(d)[1]) if k > 1 else np.inf))
        if d[j] <= assign_max:
            out[i] = j
    return out.astype(np.int32), cent, margins
