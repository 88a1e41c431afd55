"""fp32 / float64 reference implementations for face clustering (test infrastructure, imported like ``wellcond``).

- ``IResNet``: insightface arcface_torch's ``iresnet`` written out in torch (fp32, CPU) from its state dict;
- ``crop_u8`` / ``crop_input``: K13a restated in numpy integer arithmetic (bit for bit with the kernel);
  ``crop_float64``: the same crop with exact float64 bilinear weights (what the fixed point approximates);
- ``dbscan``: scikit-learn's DBSCAN labels restated in numpy (cosine distance in float64, the smallest-label border rule).
"""
from __future__ import annotations

import numpy as np

from eioku_amd import faces

BN_EPS = 1e-5


# ---- K13a ------------------------------------------------------------------------------------------------------------
def crop_u8(frames_bgr: np.ndarray, boxes) -> np.ndarray:
    """Integer restatement of k_face_crop: ``(m,112,112,3)`` uint8 RGB crops."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 5)
    n, h, w, _ = frames_bgr.shape
    out = np.zeros((len(boxes), faces.CROP, faces.CROP, 3), np.uint8)
    one = 1 << faces.TAP_BITS
    for i, b in enumerate(boxes):
        f = frames_bgr[int(b[0])].astype(np.int64)
        x0, wx1, y0, wy1 = faces.crop_taps(b[1:], h, w)
        acc = np.full((faces.CROP, faces.CROP, 3), 1 << (2 * faces.TAP_BITS - 1), np.int64)
        for dy in (0, 1):
            yy = y0 + dy
            wy = wy1 if dy else one - wy1
            for dx in (0, 1):
                xx = x0 + dx
                wx = wx1 if dx else one - wx1
                ok = ((yy >= 0) & (yy < h))[:, None] & ((xx >= 0) & (xx < w))[None, :]
                px = f[np.clip(yy, 0, h - 1)][:, np.clip(xx, 0, w - 1)]
                acc += np.where(ok[..., None], (wy[:, None] * wx[None, :])[..., None] * px, 0)
        out[i] = (acc >> (2 * faces.TAP_BITS))[..., ::-1].astype(np.uint8)
    return out


def normalise(u8: np.ndarray) -> np.ndarray:
    """arcface_torch's ``img.div_(255).sub_(0.5).div_(0.5)`` in float32 -> fp16 NHWC8 (R, G, B, 5 zeros)."""
    v = ((u8.astype(np.float32) / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)).astype(np.float16)
    out = np.zeros((*u8.shape[:3], 8), np.float16)
    out[..., :3] = v
    return out


def crop_input(frames_bgr, boxes) -> np.ndarray:
    return normalise(crop_u8(frames_bgr, boxes))


def crop_float64(frame_bgr: np.ndarray, box) -> np.ndarray:
    """Exact float64 bilinear sampling of the crop square at output pixel centres, outside samples 0 -> RGB float64."""
    h, w, _ = frame_bgr.shape
    x1, y1, x2, y2 = (float(np.float32(v)) for v in box)
    side = max(x2 - x1, y2 - y1, 1.0)
    f = frame_bgr.astype(np.float64)

    def axis(lo, hi):
        src = (lo + hi) / 2 - side / 2 + (np.arange(faces.CROP) + 0.5) * side / faces.CROP - 0.5
        i0 = np.floor(src).astype(np.int64)
        return i0, src - i0

    x0, fx = axis(x1, x2)
    y0, fy = axis(y1, y2)
    out = np.zeros((faces.CROP, faces.CROP, 3))
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            yy, xx = y0 + dy, x0 + dx
            ok = ((yy >= 0) & (yy < h))[:, None] & ((xx >= 0) & (xx < w))[None, :]
            px = f[np.clip(yy, 0, h - 1)][:, np.clip(xx, 0, w - 1)]
            out += np.where(ok[..., None], (wy[:, None] * wx[None, :])[..., None] * px, 0)
    return out[..., ::-1]


# ---- K13b ------------------------------------------------------------------------------------------------------------
def _torch_modules():
    import torch
    import torch.nn as nn

    class IBasicBlock(nn.Module):
        def __init__(self, inplanes, planes, stride, down):
            super().__init__()
            self.bn1 = nn.BatchNorm2d(inplanes, eps=BN_EPS)
            self.conv1 = nn.Conv2d(inplanes, planes, 3, 1, 1, bias=False)
            self.bn2 = nn.BatchNorm2d(planes, eps=BN_EPS)
            self.prelu = nn.PReLU(planes)
            self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
            self.bn3 = nn.BatchNorm2d(planes, eps=BN_EPS)
            self.downsample = (nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride, bias=False), nn.BatchNorm2d(planes, eps=BN_EPS))
                               if down else None)

        def forward(self, x):
            out = self.bn3(self.conv2(self.prelu(self.bn2(self.conv1(self.bn1(x))))))
            return out + (self.downsample(x) if self.downsample is not None else x)

    class IResNet(nn.Module):
        def __init__(self, depths):
            super().__init__()
            self.conv1 = nn.Conv2d(3, 64, 3, 1, 1, bias=False)
            self.bn1 = nn.BatchNorm2d(64, eps=BN_EPS)
            self.prelu = nn.PReLU(64)
            inplanes = 64
            for li, (planes, d) in enumerate(zip(faces.WIDTHS, depths), start=1):
                blocks = [IBasicBlock(inplanes, planes, 2, True)] + [IBasicBlock(planes, planes, 1, False) for _ in range(d - 1)]
                setattr(self, f"layer{li}", nn.Sequential(*blocks))
                inplanes = planes
            self.bn2 = nn.BatchNorm2d(512, eps=BN_EPS)
            self.fc = nn.Linear(512 * 49, 512)
            self.features = nn.BatchNorm1d(512, eps=BN_EPS)

        def stem(self, x):
            return self.prelu(self.bn1(self.conv1(x)))

        def forward(self, x):
            x = self.layer4(self.layer3(self.layer2(self.layer1(self.stem(x)))))
            return self.features(self.fc(torch.flatten(self.bn2(x), 1)))

    return IBasicBlock, IResNet


def iresnet(state_dict: dict):
    """torch fp32 ``IResNet`` (eval mode) with ``state_dict`` loaded strictly."""
    import torch

    _, IResNet = _torch_modules()
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in state_dict.items()}
    net = IResNet(faces.depths_from_state(state_dict))
    net.load_state_dict(sd, strict=True)
    return net.eval()


def _bn_scale_shift(sd, name):
    g, b, mu, var = (np.asarray(sd[f"{name}.{k}"], np.float64) for k in ("weight", "bias", "running_mean", "running_var"))
    s = g / np.sqrt(var + BN_EPS)
    return s, b - mu * s


def forward_blocks(state_dict: dict, crops_f16: np.ndarray, upto: int, fp16: bool = False) -> np.ndarray:
    """fp16 NHWC8 crops -> NHWC float64 output of block ``upto`` (0 = layer1.0, counting through the stages).

    ``fp16=False``: the torch fp32 network.  ``fp16=True``: its twin in the device's arithmetic - every BatchNorm that follows
    a conv folded into it (folded here, in float64, not by the package), weights rounded to fp16, fp32 accumulation, and one
    rounding to fp16 wherever the device stores a tensor: each conv's output, the PReLU's, the leading bn1's
    (``fp16(fp16(x) * scale + shift)``) and the shortcut sum ``fp16(fp16(conv2) + shortcut)``."""
    import torch
    import torch.nn.functional as F

    x = torch.from_numpy(crops_f16[..., :3].astype(np.float32)).permute(0, 3, 1, 2)
    depths = faces.depths_from_state(state_dict)
    names = [f"layer{li}.{b}" for li, d in enumerate(depths, start=1) for b in range(d)]
    with torch.no_grad():
        if not fp16:
            net = iresnet(state_dict)
            x = net.stem(x)
            for name in names[:upto + 1]:
                li, b = name[5:].split(".")
                x = getattr(net, f"layer{li}")[int(b)](x)
            return x.permute(0, 2, 3, 1).numpy().astype(np.float64)

        def h(t):
            return t.half().float()

        def conv(c, bn, t, stride):
            s, sh = _bn_scale_shift(state_dict, bn)
            w = np.asarray(state_dict[c + ".weight"], np.float64) * s[:, None, None, None]
            w = h(torch.from_numpy(w.astype(np.float32)))
            return h(F.conv2d(t, w, torch.from_numpy(sh.astype(np.float32)), stride=stride, padding=w.shape[-1] // 2))

        def prelu(name, t):
            return h(torch.where(t > 0, t, t * torch.from_numpy(np.asarray(state_dict[name + ".weight"], np.float32))[None, :, None, None]))

        x = prelu("prelu", conv("conv1", "bn1", x, 1))
        for name in names[:upto + 1]:
            s, sh = (torch.from_numpy(v.astype(np.float32))[None, :, None, None] for v in _bn_scale_shift(state_dict, name + ".bn1"))
            t = h(x * s + sh)
            u = prelu(name + ".prelu", conv(name + ".conv1", name + ".bn2", t, 1))
            down = name + ".downsample.0.weight" in state_dict
            stride = 2 if down else 1
            res = conv(name + ".downsample.0", name + ".downsample.1", x, stride) if down else x
            x = h(conv(name + ".conv2", name + ".bn3", u, stride) + res)
    return x.permute(0, 2, 3, 1).numpy().astype(np.float64)


def embed_fp32(net, crops_f16: np.ndarray) -> np.ndarray:
    """fp16 NHWC8 crops -> unit fp32 embeddings of the torch network (``F.normalize`` of its output)."""
    import torch
    import torch.nn.functional as F

    x = torch.from_numpy(crops_f16[..., :3].astype(np.float32)).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        return F.normalize(net(x), dim=1).numpy()


# ---- K14 -------------------------------------------------------------------------------------------------------------
def cosine_distances(e: np.ndarray) -> np.ndarray:
    e = np.asarray(e, np.float64)
    return 1.0 - e @ e.T


def dbscan(e: np.ndarray, eps: float, min_samples: int) -> np.ndarray:
    """scikit-learn DBSCAN(metric="cosine") labels: neighbours ``d <= eps`` (self included), core iff >= min_samples of
    them, clusters = components of the core-core graph numbered by smallest core index, a border point takes the smallest
    label among its core neighbours."""
    n = len(e)
    if n == 0:
        return np.zeros(0, np.int32)
    adj = cosine_distances(e) <= eps
    np.fill_diagonal(adj, True)
    core = adj.sum(1) >= min_samples
    labels = np.full(n, -1, np.int32)
    nxt = 0
    for i in range(n):
        if not core[i] or labels[i] >= 0:
            continue
        stack = [i]
        labels[i] = nxt
        while stack:
            p = stack.pop()
            for q in np.nonzero(adj[p] & core)[0]:
                if labels[q] < 0:
                    labels[q] = nxt
                    stack.append(q)
        nxt += 1
    for i in np.nonzero(~core)[0]:
        nb = labels[np.nonzero(adj[i] & core)[0]]
        labels[i] = nb.min() if len(nb) else -1
    return labels


def clustered_set(seed: int, n: int, d: int, k: int, spread: float, noise: int = 0) -> np.ndarray:
    """``k`` random unit centres, points at cosine distance ~ ``spread`` around them, ``noise`` isotropic points: unit fp32."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((k, d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    lab = rng.integers(0, k, n - noise)
    x = c[lab] + np.sqrt(2 * spread / d) * rng.standard_normal((n - noise, d))
    x = np.concatenate([x, rng.standard_normal((noise, d))])
    x = x[rng.permutation(n)]
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
