"""K23's definition in numpy: PCM decode, downmix and the polyphase resampler to 16 kHz, one fp32 operation at a time.

Written from the definition alone (no code shared with ``eioku_amd.audio``): the device result has to equal ``resample``
bit for bit, and ``resample`` itself is held against ``scipy.signal.resample_poly`` in tests/test_audio_host.py."""
import math

import numpy as np

WIDTH = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 4}


def geometry(rate):
    g = math.gcd(int(rate), 16000)
    up, down = 16000 // g, int(rate) // g
    m = max(up, down)
    half = 10 * m
    L = 2 * half + 1
    return up, down, m, half, L, -(-L // up)


def taps(rate):
    """float64, scaled by ``up``."""
    up, down, m, half, L, T = geometry(rate)
    k = np.arange(L, dtype=np.float64) - half
    h = (1.0 / m) * np.sinc(k / m) * np.i0(5.0 * np.sqrt(1.0 - (k / half) ** 2)) / np.i0(5.0)
    return h / h.sum() * up


def bank(rate):
    up, down, m, half, L, T = geometry(rate)
    h = taps(rate)
    B = np.zeros((up, T), dtype=np.float32)
    for p in range(up):
        col = h[p::up]
        B[p, :col.size] = col.astype(np.float32)
    return B


def resample(x, rate):
    """``x`` float32 mono at ``rate`` -> float32 at 16 kHz: ``y[n] = sum_q B[p][q] * x[i0 - q]`` accumulated in fp32 from 0 in
    ascending ``q``, multiply and add as two operations.  16000 Hz returns a copy."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    up, down, m, half, L, T = geometry(rate)
    if up == down:
        return x.copy()
    N = x.size
    n_out = -(-N * up // down)
    B = bank(rate)
    t = np.arange(n_out, dtype=np.int64) * down + half
    p = t % up
    i0 = (t - p) // up
    pad = T + 1
    hi = int(i0.max()) + 1 if n_out else 0
    xp = np.zeros(pad + max(hi, N) + 1, dtype=np.float32)
    xp[pad:pad + N] = x
    acc = np.zeros(n_out, dtype=np.float32)
    for q in range(T):
        acc = acc + B[p, q] * xp[i0 - q + pad]
    assert acc.dtype == np.float32
    return acc


def bound(x, rate):
    """``(T + 2) * 2^-24 * max_p sum_q |B[p][q]| * max|x|``: rounding of the taps to fp32, of each product, and of the T
    additions, each at most half an ulp of a partial sum no larger than ``max_p sum_q |B| max|x|``."""
    up, down, m, half, L, T = geometry(rate)
    return (T + 2) * 2.0 ** -24 * float(np.abs(bank(rate)).sum(axis=1).max()) * float(np.abs(x).max())


def decode(raw, fmt, channels):
    """Interleaved PCM bytes -> float32 mono: samples to fp32, summed in channel order in fp32, one fp32 division."""
    raw = np.ascontiguousarray(raw).reshape(-1).view(np.uint8)
    frame = WIDTH[fmt] * channels
    frames = raw.size // frame
    raw = raw[:frames * frame]
    if fmt == "u8":
        v = (raw.astype(np.float32) - np.float32(128)) / np.float32(128)
    elif fmt == "s16":
        v = raw.view("<i2").astype(np.float32) / np.float32(32768)
    elif fmt == "s24":
        b = raw.reshape(-1, 3).astype(np.int32)
        i = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        i = np.where(i >= 1 << 23, i - (1 << 24), i).astype(np.int32)
        v = i.astype(np.float32) / np.float32(8388608)
    elif fmt == "s32":
        v = raw.view("<i4").astype(np.float32) * np.float32(2.0 ** -31)
    elif fmt == "f32":
        v = raw.view("<f4").copy()
    else:
        raise ValueError(fmt)
    v = v.reshape(frames, channels)
    s = v[:, 0].copy()
    for c in range(1, channels):
        s = s + v[:, c]
    return (s / np.float32(channels)).astype(np.float32)


def encode(values, fmt):
    """float64 values in [-1, 1) -> PCM bytes of ``fmt`` (test input: full scale is reached, nothing clips)."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    if fmt == "u8":
        return np.clip(np.round(v * 128 + 128), 0, 255).astype(np.uint8)
    if fmt == "s16":
        return np.clip(np.round(v * 32768), -32768, 32767).astype("<i2").view(np.uint8)
    if fmt == "s24":
        i = np.clip(np.round(v * 8388608), -8388608, 8388607).astype(np.int64) & 0xFFFFFF
        return np.stack([i & 0xFF, (i >> 8) & 0xFF, (i >> 16) & 0xFF], axis=1).astype(np.uint8).reshape(-1)
    if fmt == "s32":
        return np.clip(np.round(v * 2147483648), -2147483648, 2147483647).astype("<i4").view(np.uint8)
    if fmt == "f32":
        return v.astype("<f4").view(np.uint8)
    raise ValueError(fmt)


def make_signal(seed, frames, channels, rate):
    """Full-scale uniform noise over the first half of the frames, a full-scale sweep from 50 Hz to 0.45 * rate over the
    second, every channel with its own noise and sweep phase: float64 ``[frames * channels]`` in [-1, 1)."""
    rng = np.random.default_rng(seed)
    n_noise = -(-frames // 2)
    n_sweep = frames - n_noise
    tt = np.arange(n_sweep, dtype=np.float64) / rate
    dur = max(n_sweep / rate, 1e-9)
    out = np.empty((frames, channels), dtype=np.float64)
    for c in range(channels):
        out[:n_noise, c] = rng.uniform(-1.0, 1.0, n_noise)
        out[n_noise:, c] = np.sin(2 * np.pi * (50.0 * tt + 0.5 * (0.45 * rate - 50.0) / dur * tt * tt) + c)
        if frames:
            out[rng.integers(0, n_noise), c] = -1.0       # full scale is reached
    return np.clip(out, -1.0, 1.0 - 2.0 ** -20).reshape(-1)
