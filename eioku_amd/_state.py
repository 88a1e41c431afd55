"""State-dict helpers shared by the models that fold a PyTorch checkpoint on the host (places, faces, speakers, ocr):
unwrap and strip, fetch with a shape check, BatchNorm scale / shift in float64, the conv + BatchNorm fold, the stage
depths of a ResNet, and the seeded draws of the random state dicts.  The arithmetic and the order of the draws are pinned
bit for bit by ``tests/test_state_fold_host.py``."""
from __future__ import annotations

import numpy as np

BN_EPS = 1e-5


def np_state(state_dict: dict, strip=("module.",)) -> dict:
    """``state_dict`` (or what it holds under ``"state_dict"``) as numpy arrays, torch tensors detached, with the ``strip``
    prefixes taken off the front of each key for as long as one is there.  (``places`` and ``faces`` used to replace
    ``"module."`` anywhere in a key; no key of any of the five architectures has it past the front.)"""
    out = {}
    for k, v in state_dict.get("state_dict", state_dict).items():
        while p := next((p for p in strip if k.startswith(p)), None):
            k = k[len(p):]
        out[k] = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v)
    return out


def tensor(sd: dict, key: str, shape=None) -> np.ndarray:
    """``sd[key]`` in float64: ``KeyError`` when missing, ``ValueError`` when not of ``shape`` (``None``: any)."""
    if key not in sd:
        raise KeyError(f"state dict has no {key}")
    v = sd[key]
    if shape is not None and tuple(v.shape) != tuple(shape):
        raise ValueError(f"{key}: expected shape {tuple(shape)}, got {tuple(v.shape)}")
    return v.astype(np.float64)


def bn_scale_shift(sd: dict, name: str, c=None, eps: float = BN_EPS):
    """BatchNorm ``name`` over ``c`` channels as ``y = scale * x + shift`` (float64)."""
    shape = None if c is None else (c,)
    g, b, mu, var = (tensor(sd, f"{name}.{f}", shape) for f in ("weight", "bias", "running_mean", "running_var"))
    s = g / np.sqrt(var + eps)
    return s, b - mu * s


def fold_conv_bn(sd: dict, conv: str, bn: str, shape=None, eps: float = BN_EPS):
    """Bias-free convolution ``conv`` of weight ``shape`` with the BatchNorm ``bn`` behind it -> fp32 ``(weight, bias)``."""
    w = tensor(sd, conv + ".weight", shape)
    s, t = bn_scale_shift(sd, bn, w.shape[0], eps)
    return (w * s[:, None, None, None]).astype(np.float32), t.astype(np.float32)


def resnet_depths(sd: dict, what: str) -> tuple:
    """Blocks per stage from the ``layer<L>.<b>.conv1.weight`` keys; ``what`` names the architecture in the error."""
    depths = []
    for li in range(1, 5):
        b = 0
        while f"layer{li}.{b}.conv1.weight" in sd:
            b += 1
        if b == 0:
            raise KeyError(f"state dict has no layer{li}.0.conv1.weight (not {what})")
        depths.append(b)
    return tuple(depths)


def rand_conv(rng, sd: dict, name: str, cout: int, cin: int, k: int, gain: float = 1.0) -> None:
    sd[name + ".weight"] = (gain * rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)


def rand_bn(rng, sd: dict, name: str, c: int) -> None:
    sd[name + ".weight"] = rng.uniform(0.7, 1.3, c).astype(np.float32)
    sd[name + ".bias"] = (0.1 * rng.standard_normal(c)).astype(np.float32)
    sd[name + ".running_mean"] = (0.1 * rng.standard_normal(c)).astype(np.float32)
    sd[name + ".running_var"] = rng.uniform(0.6, 1.4, c).astype(np.float32)
    sd[name + ".num_batches_tracked"] = np.array(0, np.int64)
