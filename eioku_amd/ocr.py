"""OCR (EasyOCR 1.7.2 ``Reader(['en']).readtext`` with its defaults) on the HIP kernels of ``csrc/ocr.hip``.

Drop-in arithmetic for ``ModelManager.extract_ocr`` (``ml-service/src/services/model_manager.py:469-558``).  Per frame:

- K15 (device): the CRAFT canvas (long side <= 2560 as is, else OpenCV INTER_LINEAR to 2560; padded to multiples of 32,
  then normalised), CRAFT (vgg16_bn + U-Net) -> text / link score maps at half the canvas.
- host (numpy, this module): ``craft_utils.getDetBoxes_core`` (poly=False), ``adjustResultCoordinates``,
  ``utils.group_text_box`` and the ``min_size`` filter -> horizontal boxes and free (tilted) quadrilaterals; grey crops
  (``get_image_list``: slices, or the perspective warp of ``four_point_transform``), ``compute_ratio_and_resize`` to
  height 64, ``AlignCollate`` / ``NormalizePAD`` (Pillow BICUBIC, right pad by the last column).
- K16 (device): english_g2 CRNN (VGG, two BiLSTMs, Linear) -> per step argmax class and probability.
- host: ``CTCLabelConverter.decode_greedy``, ``custom_mean`` confidence, the ``adjust_contrast_grey`` second pass.

``readtext`` runs with ``batch_size=1``, so every box is recognised alone and padded to its own width
(``ceil(max(1, ratio)) * 64``); here all crops of a batch of frames share one recogniser call, each sequence keeping
that width.  English only.  No CPU fallback.
"""
from __future__ import annotations

import json
import math
from pathlib import Path

import numpy as np

from . import _lib
from ._buffers import on_device, ptr
from ._handle import Handle
from ._state import BN_EPS as _BN_EPS, np_state as _np_state, tensor

CANVAS = 2560
MODEL_H = 64
MAX_ROWS = 65536  # sequence steps per recogniser call (its input projection: 512 MiB of fp32 at this size)
TAP_BITS = 11
SUPPORTED_LANGUAGES = ("en",)
# readtext's defaults (easyocr.py, Reader.readtext)
DEFAULTS = dict(min_size=20, text_threshold=0.7, low_text=0.4, link_threshold=0.4, slope_ths=0.1, ycenter_ths=0.5,
                height_ths=0.5, width_ths=0.5, add_margin=0.1, contrast_ths=0.1, adjust_contrast=0.5)


# ---- character set -------------------------------------------------------------------------------------------------
def charset():
    """``(characters, ignore_idx)`` of english_g2 from ``data/easyocr_english_g2.json``: class i + 1 is characters[i]
    (0 is the CTC blank); ignore_idx = classes of characters outside en_char + symbols."""
    d = json.loads((Path(__file__).resolve().parent / "data" / "easyocr_english_g2.json").read_text(encoding="utf-8"))
    chars = d["characters"]
    lang = set(d["en_char"]) | set(d["symbols"])
    return chars, [chars.index(c) + 1 for c in sorted(set(chars) - lang)]


def ignore_renormalise(probs: np.ndarray, ignore_idx) -> np.ndarray:
    """``recognizer_predict``: ``p[..., ignore] = 0; p /= p.sum(-1)`` (float32)."""
    p = np.array(probs, dtype=np.float32)
    p[..., list(ignore_idx)] = 0.0
    return p / np.expand_dims(p.sum(axis=-1), -1)


def decode_greedy(idx, characters: str) -> str:
    """``CTCLabelConverter.decode_greedy`` for one sequence: collapse repeats, drop the blank (0)."""
    out, prev = [], 0
    for i in (int(v) for v in idx):
        if i != 0 and i != prev:
            out.append(characters[i - 1])
        prev = i
    return "".join(out)


def custom_mean(x) -> float:
    """``utils.custom_mean``: ``prod(x) ** (2 / sqrt(len(x)))``."""
    x = np.asarray(x)
    return float(x.prod() ** (2.0 / np.sqrt(len(x))))


def confidence(idx, prob) -> float:
    """Max probabilities of the non-blank steps (``[0]`` when none) -> custom_mean."""
    idx, prob = np.asarray(idx), np.asarray(prob, dtype=np.float32)
    keep = prob[idx != 0]
    return custom_mean(keep if len(keep) else np.array([0], dtype=np.float32))


# ---- weights -------------------------------------------------------------------------------------------------------
def fold_conv(sd: dict, name: str):
    """Conv ``name`` (``<prefix>.<i>``) -> fp32 (weight, bias) with the BatchNorm ``<prefix>.<i + 1>`` folded in when the
    state dict has one (``y = (conv(x) + b - mean) * g / sqrt(var + eps) + beta``); a missing bias is zero."""
    w = tensor(sd, name + ".weight")
    b = sd[name + ".bias"].astype(np.float64) if name + ".bias" in sd else np.zeros(w.shape[0])
    head, _, idx = name.rpartition(".")
    bn = f"{head}.{int(idx) + 1}" if idx.isdigit() else None
    if bn and bn + ".running_mean" in sd:
        s = sd[bn + ".weight"].astype(np.float64) / np.sqrt(sd[bn + ".running_var"].astype(np.float64) + _BN_EPS)
        w = w * s[:, None, None, None]
        b = (b - sd[bn + ".running_mean"]) * s + sd[bn + ".bias"]
    return np.ascontiguousarray(w, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)


def lstm_params(sd: dict, layer: int):
    """``SequenceModeling.<layer>``: (w_ih [2][1024][256], w_hh, b_ih [2][1024], b_hh, w_lin [256][512], b_lin)."""
    p = f"SequenceModeling.{layer}."
    st = lambda n: np.ascontiguousarray(np.stack([sd[p + "rnn." + n + "_l0"], sd[p + "rnn." + n + "_l0_reverse"]]), dtype=np.float32)
    return (st("weight_ih"), st("weight_hh"), st("bias_ih"), st("bias_hh"),
            np.ascontiguousarray(sd[p + "linear.weight"], dtype=np.float32), np.ascontiguousarray(sd[p + "linear.bias"], dtype=np.float32))


CRAFT_CONVS = [  # (name, cout, cin, k, has BN); state dict prefixes of craft.CRAFT
    ("basenet.slice1.0", 64, 3, 3, 1), ("basenet.slice1.3", 64, 64, 3, 1), ("basenet.slice1.7", 128, 64, 3, 1),
    ("basenet.slice1.10", 128, 128, 3, 1), ("basenet.slice2.14", 256, 128, 3, 1), ("basenet.slice2.17", 256, 256, 3, 1),
    ("basenet.slice3.20", 256, 256, 3, 1), ("basenet.slice3.24", 512, 256, 3, 1), ("basenet.slice3.27", 512, 512, 3, 1),
    ("basenet.slice4.30", 512, 512, 3, 1), ("basenet.slice4.34", 512, 512, 3, 1), ("basenet.slice4.37", 512, 512, 3, 1),
    ("basenet.slice5.1", 1024, 512, 3, 0), ("basenet.slice5.2", 1024, 1024, 1, 0), ("upconv1.conv.0", 512, 1536, 1, 1),
    ("upconv1.conv.3", 256, 512, 3, 1), ("upconv2.conv.0", 256, 768, 1, 1), ("upconv2.conv.3", 128, 256, 3, 1),
    ("upconv3.conv.0", 128, 384, 1, 1), ("upconv3.conv.3", 64, 128, 3, 1), ("upconv4.conv.0", 64, 192, 1, 1),
    ("upconv4.conv.3", 32, 64, 3, 1), ("conv_cls.0", 32, 32, 3, 0), ("conv_cls.2", 32, 32, 3, 0), ("conv_cls.4", 16, 32, 3, 0),
    ("conv_cls.6", 16, 16, 1, 0), ("conv_cls.8", 2, 16, 1, 0)]
CRNN_CONVS = [("FeatureExtraction.ConvNet.0", 32, 1, 3, 0, True), ("FeatureExtraction.ConvNet.3", 64, 32, 3, 0, True),
              ("FeatureExtraction.ConvNet.6", 128, 64, 3, 0, True), ("FeatureExtraction.ConvNet.8", 128, 128, 3, 0, True),
              ("FeatureExtraction.ConvNet.11", 256, 128, 3, 1, False), ("FeatureExtraction.ConvNet.14", 256, 256, 3, 1, False),
              ("FeatureExtraction.ConvNet.18", 256, 256, 2, 0, True)]


def _rand_conv(rng, sd, name, cout, cin, k, bn, bias=True):
    sd[name + ".weight"] = (rng.standard_normal((cout, cin, k, k)) * math.sqrt(2.0 / (cin * k * k))).astype(np.float32)
    if bias:
        sd[name + ".bias"] = (0.05 * rng.standard_normal(cout)).astype(np.float32)
    if bn:
        head, _, i = name.rpartition(".")
        b = f"{head}.{int(i) + 1}"
        sd[b + ".weight"] = (1.0 + 0.1 * rng.standard_normal(cout)).astype(np.float32)
        sd[b + ".bias"] = (0.1 * rng.standard_normal(cout)).astype(np.float32)
        sd[b + ".running_mean"] = (0.1 * rng.standard_normal(cout)).astype(np.float32)
        sd[b + ".running_var"] = (1.0 + 0.2 * rng.random(cout)).astype(np.float32)
        sd[b + ".num_batches_tracked"] = np.array(0)


def random_craft_state(seed: int = 5, cls_bias=(0.0, 0.0)) -> dict:
    """Seeded random CRAFT weights of the real shapes (``conv_cls.8`` bias = ``cls_bias``: tests move it so a few percent
    of pixels clear ``low_text``)."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, cout, cin, k, bn in CRAFT_CONVS:
        _rand_conv(rng, sd, name, cout, cin, k, bn)
    sd["conv_cls.8.bias"] = np.asarray(cls_bias, np.float32)
    return sd


def random_crnn_state(seed: int = 6, num_class: int = 97) -> dict:
    rng = np.random.default_rng(seed)
    sd = {}
    for name, cout, cin, k, bn, bias in CRNN_CONVS:
        _rand_conv(rng, sd, name, cout, cin, k, bn, bias)
    u = lambda *s: (rng.random(s) * 2 - 1).astype(np.float32) / 16.0  # nn.LSTM's U(-1/sqrt(256), 1/sqrt(256))
    for l in range(2):
        p = f"SequenceModeling.{l}."
        for suf in ("_l0", "_l0_reverse"):
            sd[p + "rnn.weight_ih" + suf], sd[p + "rnn.weight_hh" + suf] = u(1024, 256), u(1024, 256)
            sd[p + "rnn.bias_ih" + suf], sd[p + "rnn.bias_hh" + suf] = u(1024), u(1024)
        sd[p + "linear.weight"], sd[p + "linear.bias"] = u(256, 512) * 2.0, u(256)
    sd["Prediction.weight"] = (rng.standard_normal((num_class, 256)) * 0.25).astype(np.float32)
    sd["Prediction.bias"] = (0.1 * rng.standard_normal(num_class)).astype(np.float32)
    return sd


def load_checkpoint(path) -> dict:
    import torch

    return _np_state(torch.load(str(path), map_location="cpu", weights_only=True))


# ---- K15 host side: canvas and OpenCV INTER_LINEAR taps ------------------------------------------------------------
def craft_canvas(h: int, w: int, canvas: int = CANVAS):
    """``resize_aspect_ratio(img, canvas, INTER_LINEAR, mag_ratio=1)``: ``(ratio, target_h, target_w, H32, W32)``."""
    target = float(max(h, w))
    if target > canvas:
        target = canvas
    ratio = target / max(h, w)
    th, tw = int(h * ratio), int(w * ratio)
    return ratio, th, tw, th + (-th) % 32, tw + (-tw) % 32


def linear_taps(src: int, dst: int) -> np.ndarray:
    """OpenCV ``resize`` INTER_LINEAR taps of one axis as ``ocr.hip`` linear_taps: int64 (dst, 3) = (first index, w0, w1)
    in 1/2048."""
    out = np.empty((dst, 3), np.int64)
    scale = src / dst
    for d in range(dst):
        fx = np.float32((d + 0.5) * scale - 0.5)
        sx = int(np.floor(fx))
        fx = np.float32(fx - np.float32(sx))
        if sx < 0:
            fx, sx = np.float32(0), 0
        if sx >= src - 1:
            fx, sx = np.float32(0), src - 1
        out[d] = (sx, int(np.rint(np.float32(1 - fx) * np.float32(2048))), int(np.rint(fx * np.float32(2048))))
    return out


def resize_linear_u8(img: np.ndarray, dh: int, dw: int) -> np.ndarray:
    """``cv2.resize(img, (dw, dh), interpolation=INTER_LINEAR)`` on uint8 (H, W[, C]) with 11-bit taps and one rounding
    (``(sum + 2**21) >> 22``), as ``k_craft_prep``.  This is OpenCV's scalar vertical pass; its SIMD pass for u8
    (``VResizeLinearVec_32s8u``: each term shifted by 4, the high half of each product, then rounded by 2) can differ by
    one level, so crops and >2560 canvases are not bit-identical to OpenCV on SIMD builds."""
    h, w = img.shape[:2]
    if (h, w) == (dh, dw):
        return img.copy()
    tx, ty = linear_taps(w, dw), linear_taps(h, dh)
    x0, x1 = tx[:, 0], np.minimum(tx[:, 0] + 1, w - 1)
    y0, y1 = ty[:, 0], np.minimum(ty[:, 0] + 1, h - 1)
    a = img.astype(np.int64)
    ex = (slice(None),) + (None,) * (img.ndim - 2)
    s0 = a[y0][:, x0] * tx[:, 1][ex] + a[y0][:, x1] * tx[:, 2][ex]
    s1 = a[y1][:, x0] * tx[:, 1][ex] + a[y1][:, x1] * tx[:, 2][ex]
    ey = (slice(None), None) + (None,) * (img.ndim - 2)
    v = (ty[:, 1][ey] * s0 + ty[:, 2][ey] * s1 + (1 << 21)) >> 22
    return np.clip(v, 0, 255).astype(np.uint8)


# ---- box post-processing: craft_utils / utils restated -----------------------------------------------------------
def _hull(pts: np.ndarray) -> np.ndarray:
    """Convex hull (Andrew's monotone chain) of integer points, counter-clockwise in (x, y) axes."""
    p = sorted(set(map(tuple, pts.tolist())))
    if len(p) <= 2:
        return np.array(p, np.float64)

    def half(seq):
        out = []
        for q in seq:
            while len(out) >= 2 and (out[-1][0] - out[-2][0]) * (q[1] - out[-2][1]) - (out[-1][1] - out[-2][1]) * (q[0] - out[-2][0]) <= 0:
                out.pop()
            out.append(q)
        return out

    lo, up = half(p), half(p[::-1])
    return np.array(lo[:-1] + up[:-1], np.float64)


def min_area_rect_points(pts: np.ndarray) -> np.ndarray:
    """``cv2.boxPoints(cv2.minAreaRect(pts))`` restated: the minimum-area enclosing rectangle (one side on a hull edge,
    rotating calipers), its corners float32 clockwise on screen (y down)."""
    order = np.lexsort((pts[:, 0], pts[:, 1]))  # the hull's vertices are among each row's two extreme points
    ys = pts[order, 1]
    first = np.r_[True, ys[1:] != ys[:-1]]
    last = np.r_[ys[1:] != ys[:-1], True]
    hull = _hull(pts[order][first | last])
    if len(hull) == 1:
        return np.repeat(hull.astype(np.float32), 4, 0)
    best = None
    for i in range(len(hull)):
        e = hull[(i + 1) % len(hull)] - hull[i]
        n = math.hypot(*e)
        if n == 0:
            continue
        u = e / n
        v = np.array([-u[1], u[0]])
        pu, pv = hull @ u, hull @ v
        area = (pu.max() - pu.min()) * (pv.max() - pv.min())
        if best is None or area < best[0] - 1e-9:
            best = (area, u, v, pu.min(), pu.max(), pv.min(), pv.max())
    _, u, v, a0, a1, b0, b1 = best
    c = np.array([a * u + b * v for a, b in ((a0, b0), (a1, b0), (a1, b1), (a0, b1))])
    ctr = c.mean(0)
    c = c[np.argsort(np.arctan2(c[:, 1] - ctr[1], c[:, 0] - ctr[0]), kind="stable")]  # clockwise on screen
    return c.astype(np.float32)


def det_boxes(textmap: np.ndarray, linkmap: np.ndarray | None, text_threshold=0.7, link_threshold=0.4, low_text=0.4,
              binmap: np.ndarray | None = None) -> list:
    """``craft_utils.getDetBoxes_core`` (poly=False, no character estimate): float32 (4, 2) boxes in score-map pixels.
    ``binmap`` (K15's u8 ``(text > low_text) | (link > link_threshold)``) stands in for the link map: the link-only pixels
    are ``binmap & ~(text > low_text)``."""
    from scipy import ndimage

    img_h, img_w = textmap.shape
    text_score = textmap > low_text
    comb = binmap != 0 if binmap is not None else text_score | (linkmap > link_threshold)
    link_only = comb & ~text_score
    labels, n = ndimage.label(comb, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])  # raster order of first pixels
    if n == 0:
        return []
    sizes = np.bincount(labels.ravel(), minlength=n + 1)
    peaks = ndimage.maximum(textmap, labels, index=np.arange(1, n + 1))
    slices = ndimage.find_objects(labels)
    det = []
    for k in range(1, n + 1):
        size = int(sizes[k])
        if size < 10 or peaks[k - 1] < text_threshold:
            continue
        sl = slices[k - 1]
        y, x = sl[0].start, sl[1].start
        h, w = sl[0].stop - y, sl[1].stop - x
        niter = int(math.sqrt(size * min(w, h) / (w * h)) * 2)
        sx, ex, sy, ey = x - niter, x + w + niter + 1, y - niter, y + h + niter + 1
        sx, sy = max(sx, 0), max(sy, 0)
        ex, ey = min(ex, img_w), min(ey, img_h)
        seg = (labels[sy:ey, sx:ex] == k) & ~link_only[sy:ey, sx:ex]
        # cv2.dilate with a (1 + niter)^2 rectangle, anchor (1 + niter) // 2, inside the ROI only
        # (separable: rows, then columns); out[y, x] = max over i, j in [0, niter] of seg[y + niter - i - a, x + niter - j - a]
        ks, a = 1 + niter, (1 + niter) // 2
        if ks > 1:
            hh, ww = seg.shape
            pad = np.zeros((hh, ww + ks - 1), bool)
            pad[:, a:a + ww] = seg
            row = np.zeros_like(seg)
            for j in range(ks):
                row |= pad[:, ks - 1 - j:ks - 1 - j + ww]
            pad = np.zeros((hh + ks - 1, ww), bool)
            pad[a:a + hh] = row
            seg = np.zeros_like(seg)
            for i in range(ks):
                seg |= pad[ks - 1 - i:ks - 1 - i + hh]
        ys, xs = np.nonzero(seg)
        if len(xs) == 0:
            continue
        pts = np.stack([xs + sx, ys + sy], 1)
        box = min_area_rect_points(pts)
        bw, bh = np.linalg.norm(box[0] - box[1]), np.linalg.norm(box[1] - box[2])
        if abs(1 - max(bw, bh) / (min(bw, bh) + 1e-5)) <= 0.1:  # align diamond-shape
            l, r, t, b = pts[:, 0].min(), pts[:, 0].max(), pts[:, 1].min(), pts[:, 1].max()
            box = np.array([[l, t], [r, t], [r, b], [l, b]], dtype=np.float32)
        start = int(box.sum(axis=1).argmin())
        det.append(np.roll(box, 4 - start, 0))
    return det


def adjust_coordinates(boxes: list, ratio: float) -> list:
    """``adjustResultCoordinates(boxes, 1 / ratio, 1 / ratio)`` then ``np.array(box).astype(np.int32).reshape(-1)``."""
    if not boxes:
        return []
    polys = np.array(boxes)
    r = 1 / ratio
    for k in range(len(polys)):
        polys[k] *= (r * 2, r * 2)
    return [np.array(b).astype(np.int32).reshape(-1) for b in polys]


def group_text_box(polys, slope_ths=0.1, ycenter_ths=0.5, height_ths=0.5, width_ths=0.5, add_margin=0.1):
    """``utils.group_text_box`` (sort_output=True): ``(horizontal [x_min, x_max, y_min, y_max], free [[x, y] x 4])``."""
    horizontal_list, free_list, combined_list, merged_list = [], [], [], []
    for poly in polys:
        slope_up = (poly[3] - poly[1]) / np.maximum(10, (poly[2] - poly[0]))
        slope_down = (poly[5] - poly[7]) / np.maximum(10, (poly[4] - poly[6]))
        if max(abs(slope_up), abs(slope_down)) < slope_ths:
            x_max, x_min = max(poly[0], poly[2], poly[4], poly[6]), min(poly[0], poly[2], poly[4], poly[6])
            y_max, y_min = max(poly[1], poly[3], poly[5], poly[7]), min(poly[1], poly[3], poly[5], poly[7])
            horizontal_list.append([x_min, x_max, y_min, y_max, 0.5 * (y_min + y_max), y_max - y_min])
        else:
            height = np.linalg.norm([poly[6] - poly[0], poly[7] - poly[1]])
            width = np.linalg.norm([poly[2] - poly[0], poly[3] - poly[1]])
            margin = int(1.44 * add_margin * min(width, height))
            theta13 = abs(np.arctan((poly[1] - poly[5]) / np.maximum(10, (poly[0] - poly[4]))))
            theta24 = abs(np.arctan((poly[3] - poly[7]) / np.maximum(10, (poly[2] - poly[6]))))
            x1, y1 = poly[0] - np.cos(theta13) * margin, poly[1] - np.sin(theta13) * margin
            x2, y2 = poly[2] + np.cos(theta24) * margin, poly[3] - np.sin(theta24) * margin
            x3, y3 = poly[4] + np.cos(theta13) * margin, poly[5] + np.sin(theta13) * margin
            x4, y4 = poly[6] - np.cos(theta24) * margin, poly[7] + np.sin(theta24) * margin
            free_list.append([[x1, y1], [x2, y2], [x3, y3], [x4, y4]])
    horizontal_list = sorted(horizontal_list, key=lambda item: item[4])
    new_box = []
    for poly in horizontal_list:
        if len(new_box) == 0:
            b_height, b_ycenter = [poly[5]], [poly[4]]
            new_box.append(poly)
        elif abs(np.mean(b_ycenter) - poly[4]) < ycenter_ths * np.mean(b_height):
            b_height.append(poly[5])
            b_ycenter.append(poly[4])
            new_box.append(poly)
        else:
            b_height, b_ycenter = [poly[5]], [poly[4]]
            combined_list.append(new_box)
            new_box = [poly]
    combined_list.append(new_box)
    for boxes in combined_list:
        if len(boxes) == 1:
            box = boxes[0]
            margin = int(add_margin * min(box[1] - box[0], box[5]))
            merged_list.append([box[0] - margin, box[1] + margin, box[2] - margin, box[3] + margin])
            continue
        boxes = sorted(boxes, key=lambda item: item[0])
        merged_box, new_box = [], []
        for box in boxes:
            if len(new_box) == 0:
                b_height, x_max = [box[5]], box[1]
                new_box.append(box)
            elif abs(np.mean(b_height) - box[5]) < height_ths * np.mean(b_height) and (box[0] - x_max) < width_ths * (box[3] - box[2]):
                b_height.append(box[5])
                x_max = box[1]
                new_box.append(box)
            else:
                b_height, x_max = [box[5]], box[1]
                merged_box.append(new_box)
                new_box = [box]
        if len(new_box) > 0:
            merged_box.append(new_box)
        for mbox in merged_box:
            if len(mbox) != 1:
                x_min, x_max = min(mbox, key=lambda x: x[0])[0], max(mbox, key=lambda x: x[1])[1]
                y_min, y_max = min(mbox, key=lambda x: x[2])[2], max(mbox, key=lambda x: x[3])[3]
                margin = int(add_margin * (min(x_max - x_min, y_max - y_min)))
                merged_list.append([x_min - margin, x_max + margin, y_min - margin, y_max + margin])
            else:
                box = mbox[0]
                margin = int(add_margin * (min(box[1] - box[0], box[3] - box[2])))
                merged_list.append([box[0] - margin, box[1] + margin, box[2] - margin, box[3] + margin])
    return merged_list, free_list


def filter_min_size(horizontal_list, free_list, min_size=20):
    """``Reader.detect``'s ``min_size`` filter."""
    diff = lambda v: max(v) - min(v)
    return ([i for i in horizontal_list if max(i[1] - i[0], i[3] - i[2]) > min_size],
            [i for i in free_list if max(diff([c[0] for c in i]), diff([c[1] for c in i])) > min_size])


def boxes_from_maps(textmap, linkmap, ratio: float, p=DEFAULTS, binmap=None):
    """One frame's score maps (text and link, or text and K15's binary map) -> ``(horizontal_list, free_list)`` as
    ``Reader.detect`` returns them."""
    polys = adjust_coordinates(det_boxes(textmap, linkmap, p["text_threshold"], p["link_threshold"], p["low_text"], binmap), ratio)
    h, f = group_text_box(polys, p["slope_ths"], p["ycenter_ths"], p["height_ths"], p["width_ths"], p["add_margin"])
    return filter_min_size(h, f, p["min_size"])


# ---- crops: utils.get_image_list / AlignCollate restated ---------------------------------------------------------
def bgr_to_gray(bgr: np.ndarray) -> np.ndarray:
    """``cv2.cvtColor(BGR2GRAY)`` on uint8: ``(4899 R + 9617 G + 1868 B + 2**13) >> 14``."""
    a = bgr.astype(np.int32)
    return ((a[..., 2] * 4899 + a[..., 1] * 9617 + a[..., 0] * 1868 + (1 << 13)) >> 14).astype(np.uint8)


def perspective_transform(src: np.ndarray, dst: np.ndarray) -> np.ndarray:
    """``cv2.getPerspectiveTransform``: the 8 x 8 system solved in float64."""
    a, b = np.zeros((8, 8)), np.zeros(8)
    for i in range(4):
        x, y = float(src[i][0]), float(src[i][1])
        u, v = float(dst[i][0]), float(dst[i][1])
        a[i] = [x, y, 1, 0, 0, 0, -x * u, -y * u]
        a[i + 4] = [0, 0, 0, x, y, 1, -x * v, -y * v]
        b[i], b[i + 4] = u, v
    return np.append(np.linalg.solve(a, b), 1.0).reshape(3, 3)


def warp_perspective(img: np.ndarray, M: np.ndarray, w: int, h: int) -> np.ndarray:
    """``cv2.warpPerspective(img, M, (w, h))`` (INTER_LINEAR, BORDER_CONSTANT 0) on a uint8 grey image: inverse map,
    source position rounded to 1/32, 15-bit bilinear weights, ``(sum + 2**14) >> 15``."""
    Mi = np.linalg.inv(M)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    X0 = Mi[0, 0] * xs + Mi[0, 1] * ys + Mi[0, 2]
    Y0 = Mi[1, 0] * xs + Mi[1, 1] * ys + Mi[1, 2]
    W = Mi[2, 0] * xs + Mi[2, 1] * ys + Mi[2, 2]
    W = np.where(W != 0, 32.0 / np.where(W != 0, W, 1), 0.0)
    X = np.rint(np.clip(X0 * W, -2**31, 2**31 - 1)).astype(np.int64)
    Y = np.rint(np.clip(Y0 * W, -2**31, 2**31 - 1)).astype(np.int64)
    sx, sy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
    H_, W_ = img.shape
    a = img.astype(np.int64)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < H_) & (xx >= 0) & (xx < W_)
        return np.where(ok, a[np.clip(yy, 0, H_ - 1), np.clip(xx, 0, W_ - 1)], 0)

    acc = (tap(sy, sx) * (32 - fy) * (32 - fx) + tap(sy, sx + 1) * (32 - fy) * fx + tap(sy + 1, sx) * fy * (32 - fx)
           + tap(sy + 1, sx + 1) * fy * fx) * 32
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


def four_point_transform(image: np.ndarray, rect) -> np.ndarray:
    rect = np.asarray(rect, np.float32)
    tl, tr, br, bl = rect
    max_w = max(int(np.sqrt(((br[0] - bl[0]) ** 2) + ((br[1] - bl[1]) ** 2))), int(np.sqrt(((tr[0] - tl[0]) ** 2) + ((tr[1] - tl[1]) ** 2))))
    max_h = max(int(np.sqrt(((tr[0] - br[0]) ** 2) + ((tr[1] - br[1]) ** 2))), int(np.sqrt(((tl[0] - bl[0]) ** 2) + ((tl[1] - bl[1]) ** 2))))
    dst = np.array([[0, 0], [max_w - 1, 0], [max_w - 1, max_h - 1], [0, max_h - 1]], dtype=np.float32)
    return warp_perspective(image, perspective_transform(rect, dst), max_w, max_h)


def _ratio(width, height):
    r = width / height
    return 1.0 / r if r < 1.0 else r


def compute_ratio_and_resize(img, width, height, model_height=MODEL_H):
    ratio = width / height
    if ratio < 1.0:
        ratio = _ratio(width, height)
        return resize_linear_u8(img, int(model_height * ratio), model_height), ratio
    return resize_linear_u8(img, model_height, int(model_height * ratio)), ratio


def image_list(horizontal_list, free_list, grey: np.ndarray, model_height=MODEL_H):
    """``get_image_list`` for the boxes of one frame as ``recognize`` calls it with ``batch_size=1``: one box at a time
    (horizontal boxes first, then free ones) -> ``[(box, crop u8, padded width)]``."""
    out = []
    max_y, max_x = grey.shape
    for box in free_list:
        t = four_point_transform(grey, box)
        if t.shape[0] == 0 or t.shape[1] == 0 or int(model_height * _ratio(t.shape[1], t.shape[0])) == 0:
            continue
        crop, ratio = compute_ratio_and_resize(t, t.shape[1], t.shape[0], model_height)
        out.append((box, crop, math.ceil(max(ratio, 1)) * model_height))
    hl = []
    for box in horizontal_list:
        x_min, x_max, y_min, y_max = max(0, box[0]), min(box[1], max_x), max(0, box[2]), min(box[3], max_y)
        width, height = x_max - x_min, y_max - y_min
        if width <= 0 or height <= 0 or int(model_height * _ratio(width, height)) == 0:
            continue
        crop, ratio = compute_ratio_and_resize(grey[y_min:y_max, x_min:x_max], width, height, model_height)
        hl.append(([[x_min, y_min], [x_max, y_min], [x_max, y_max], [x_min, y_max]], crop,
                    math.ceil(max(ratio, 1)) * model_height))
    return hl + out


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def _pil_coeffs(in_size: int, out_size: int):
    """Pillow ``precompute_coeffs`` (bicubic, support 2) + ``normalize_coeffs_8bpc``: (xmin, taps int64 (out, ksize))."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    xmins, kk = np.zeros(out_size, np.int64), np.zeros((out_size, ksize), np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = _bicubic((np.arange(xmax) + xmin - center + 0.5) * (1.0 / fs))
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = w / ww
        k = np.where(w < 0, (-0.5 + w * (1 << 22)), (0.5 + w * (1 << 22)))
        kk[xx, :xmax] = np.trunc(k).astype(np.int64)
        xmins[xx] = xmin
    return xmins, kk


def _pil_pass(a: np.ndarray, out_size: int) -> np.ndarray:
    """One Pillow 8bpc resample pass along the last axis."""
    xmins, kk = _pil_coeffs(a.shape[-1], out_size)
    ks = kk.shape[1]
    pad = np.concatenate([a.astype(np.int64), np.zeros(a.shape[:-1] + (ks,), np.int64)], -1)
    idx = xmins[:, None] + np.arange(ks)[None, :]
    ss = (pad[..., idx] * kk).sum(-1) + (1 << 21)
    return np.clip(ss >> 22, 0, 255).astype(np.uint8)


def pil_bicubic(img: np.ndarray, w: int, h: int) -> np.ndarray:
    """``Image.fromarray(img, 'L').resize((w, h), Image.BICUBIC)``: horizontal pass, then vertical."""
    out = img
    if w != img.shape[1]:
        out = _pil_pass(out, w)
    if h != img.shape[0]:
        out = _pil_pass(out.T, h).T
    return np.ascontiguousarray(out)


def adjust_contrast_grey(img: np.ndarray, target: float = 0.4) -> np.ndarray:
    high, low = np.percentile(img, 90), np.percentile(img, 10)
    if (high - low) / np.maximum(10, high + low) < target:
        ratio = 200.0 / np.maximum(10, high - low)
        v = (img.astype(int) - low + 25) * ratio
        return np.maximum(np.full(v.shape, 0), np.minimum(np.full(v.shape, 255), v)).astype(np.uint8)
    return img


def align_collate(crop: np.ndarray, width: int, adjust_contrast: float = 0.0, img_h: int = MODEL_H) -> np.ndarray:
    """``AlignCollate(imgH=64, imgW=width, keep_ratio_with_pad=True, adjust_contrast)`` on one crop -> float32 (64, width)."""
    if adjust_contrast > 0:
        crop = adjust_contrast_grey(crop, target=adjust_contrast)
    h, w = crop.shape
    rw = min(width, math.ceil(img_h * (w / float(h))))
    x = pil_bicubic(crop, rw, img_h).astype(np.float32) / np.float32(255.0)
    x = (x - np.float32(0.5)) / np.float32(0.5)
    out = np.empty((img_h, width), np.float32)
    out[:, :rw] = x
    out[:, rw:] = x[:, rw - 1:rw]
    return out


# ---- the reader ----------------------------------------------------------------------------------------------------
def _set_lstms(crnn: Handle, sd: dict) -> None:
    for l in range(2):
        arrs = lstm_params(sd, l)  # held until the call returns
        _lib.check(crnn.eioku_crnn_set_lstm(l, *(ptr(a) for a in arrs)), "eioku_crnn_set_lstm")


class OcrReader:
    """CRAFT (K15) + english_g2 (K16) from state dicts; ``readtext_batch(frames)`` is ``readtext`` per frame."""

    def __init__(self, craft_state: dict, crnn_state: dict):
        import torch

        self.characters, self.ignore_idx = charset()
        sd_d, sd_r = _np_state(craft_state), _np_state(crnn_state)
        nc = int(tensor(sd_r, "Prediction.weight").shape[0])
        if nc != len(self.characters) + 1:
            raise ValueError(f"Prediction has {nc} classes; english_g2 needs {len(self.characters) + 1}")
        self.num_class = nc
        self._ignore = np.zeros(nc, np.uint8)
        self._ignore[self.ignore_idx] = 1
        device = torch.cuda.current_device() if torch.cuda.is_available() else 0
        self._d = Handle("craft", device=device)
        self._r = self._d.or_close(Handle, "crnn", nc, device=device)
        self._d.or_close(self._r.or_close, self._load, sd_d, sd_r)

    def _load(self, sd_d, sd_r):
        self._d.set_convs(lambda name, *_: fold_conv(sd_d, name))
        self._r.set_convs(lambda name, *_: fold_conv(sd_r, name))
        _set_lstms(self._r, sd_r)

    @classmethod
    def from_cache(cls, cache_dir, seed: int | None = None):
        """Weights from ``<cache>/easyocr/model/{craft_mlt_25k,english_g2}.pth`` (EasyOCR's model_storage_directory
        layout under the model cache).  Nothing is downloaded: a missing file is an error unless ``seed`` asks for seeded
        random weights."""
        d = Path(cache_dir) / "easyocr" / "model"
        pd, pr = d / "craft_mlt_25k.pth", d / "english_g2.pth"
        if pd.exists() and pr.exists():
            return cls(load_checkpoint(pd), load_checkpoint(pr))
        if seed is None:
            raise FileNotFoundError(f"{pd if not pd.exists() else pr} not found (EasyOCR weights are not downloaded here)")
        return cls(random_craft_state(seed), random_crnn_state(seed + 1))

    # -- K15 --
    def score_maps(self, frames_bgr, canvas: int = CANVAS, low_text=0.4, link_threshold=0.4, want_link: bool = True):
        """frames uint8 (n, h, w, 3) BGR (numpy or device tensor) -> CUDA tensors ``(text, link, bin)`` (n, H/2, W/2);
        ``link`` is None unless ``want_link``."""
        import torch

        n, h, w, _ = (int(s) for s in frames_bgr.shape)
        _, _, _, H, W = craft_canvas(h, w, canvas)
        dev = frames_bgr.device if on_device(frames_bgr) else torch.device("cuda", torch.cuda.current_device())
        text = torch.empty((n, H // 2, W // 2), dtype=torch.float32, device=dev)
        link = torch.empty_like(text) if want_link else None
        binm = torch.empty((n, H // 2, W // 2), dtype=torch.uint8, device=dev)
        src = frames_bgr if on_device(frames_bgr) else np.ascontiguousarray(frames_bgr)
        _lib.check(self._d.eioku_craft_forward(ptr(src), n, h, w, canvas, low_text, link_threshold, ptr(text), ptr(link),
                                               ptr(binm), _lib.MEM_DEVICE if on_device(frames_bgr) else _lib.MEM_HOST,
                                               torch.cuda.current_stream(dev).cuda_stream), "eioku_craft_forward")
        return text, link, binm

    def canvas(self, frames_bgr, canvas: int = CANVAS):
        """Stage (``eioku_craft_canvas``): frames as ``score_maps`` takes them -> the network's input alone, CUDA fp16
        (n, H, W, 8)."""
        import torch

        n, h, w, _ = (int(s) for s in frames_bgr.shape)
        _, _, _, H, W = craft_canvas(h, w, canvas)
        dev = frames_bgr.device if on_device(frames_bgr) else torch.device("cuda", torch.cuda.current_device())
        out = torch.empty((n, H, W, 8), dtype=torch.float16, device=dev)
        src = frames_bgr if on_device(frames_bgr) else np.ascontiguousarray(frames_bgr)
        _lib.check(self._d.eioku_craft_canvas(ptr(src), n, h, w, canvas, ptr(out),
                                              _lib.MEM_DEVICE if on_device(frames_bgr) else _lib.MEM_HOST,
                                              torch.cuda.current_stream(dev).cuda_stream), "eioku_craft_canvas")
        return out

    # -- K16 --
    def recognize_raw(self, imgs: list, want_logits: bool = False):
        """Normalised crops float32 (64, width_i) -> per crop ``(idx int32 (T_i,), prob float32 (T_i,)[, logits])``.
        Crops go to the device in calls of at most ``MAX_ROWS`` sequence steps (a crop's steps: width / 4 - 1)."""
        out, chunk, rows = [], [], 0
        for a in imgs:
            t = a.shape[1] // 4 - 1
            if chunk and rows + t > MAX_ROWS:
                out += self._recognize_call(chunk, want_logits)
                chunk, rows = [], 0
            chunk.append(a)
            rows += t
        return out + (self._recognize_call(chunk, want_logits) if chunk else [])

    def _recognize_call(self, imgs: list, want_logits: bool):
        m = len(imgs)
        widths = np.array([a.shape[1] for a in imgs], np.int32)
        packed = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(a, np.float32).ravel() for a in imgs]))
        T = widths // 4 - 1
        rows = int(T.sum())
        idx, prob = np.empty(rows, np.int32), np.empty(rows, np.float32)
        logits = np.empty((rows, self.num_class), np.float32) if want_logits else None
        _lib.check(self._r.eioku_crnn_forward(ptr(packed), ptr(widths), m, ptr(self._ignore), ptr(idx), ptr(prob),
                                              ptr(logits), None), "eioku_crnn_forward")
        out, o = [], 0
        for t in T:
            out.append((idx[o:o + t], prob[o:o + t]) + ((logits[o:o + t],) if want_logits else ()))
            o += t
        return out

    def recognize_crops(self, crops: list, p=DEFAULTS):
        """``get_text`` for ``[(crop u8, padded width)]``: first pass, then the contrast pass on confidences below
        ``contrast_ths``; the higher confidence wins (the first pass on ties) -> ``[(text, confidence)]``."""
        first = self.recognize_raw([align_collate(c, wdt) for c, wdt in crops])
        res = [(decode_greedy(i, self.characters), confidence(i, pr)) for i, pr in first]
        low = [k for k, (_, conf) in enumerate(res) if conf < p["contrast_ths"]]
        if low:
            second = self.recognize_raw([align_collate(crops[k][0], crops[k][1], p["adjust_contrast"]) for k in low])
            for k, (i, pr) in zip(low, second):
                t2, c2 = decode_greedy(i, self.characters), confidence(i, pr)
                if not res[k][1] > c2:
                    res[k] = (t2, c2)
        return res

    def readtext_batch(self, frames, p=DEFAULTS) -> list:
        """frames uint8 (n, h, w, 3) BGR -> per frame ``[(box, text, confidence)]`` in ``readtext``'s order."""
        frames = np.ascontiguousarray(np.asarray(frames))
        n, h, w, _ = frames.shape
        if n == 0:
            return []
        ratio = craft_canvas(h, w)[0]
        # the text map and K15's u8 map are all the box rules need (5 of the 8 bytes per pixel of both maps)
        text, _, binm = self.score_maps(frames, low_text=p["low_text"], link_threshold=p["link_threshold"], want_link=False)
        text, binm = text.cpu().numpy(), binm.cpu().numpy()
        per_frame, crops = [], []
        for f in range(n):
            hl, fl = boxes_from_maps(text[f], None, ratio, p, binmap=binm[f])
            items = image_list(hl, fl, bgr_to_gray(frames[f]))
            per_frame.append([b for b, _, _ in items])
            crops += [(c, wdt) for _, c, wdt in items]
        rec = self.recognize_crops(crops, p)
        out, k = [], 0
        for boxes in per_frame:
            out.append([(b, t, c) for b, (t, c) in zip(boxes, rec[k:k + len(boxes)])])
            k += len(boxes)
        return out

    def last_flops(self) -> tuple:
        return self._d.doubles("last_flops")[0], self._r.doubles("last_flops")[0]

    def close(self):
        self._d.close()
        self._r.close()


# ---- stage entry points (tests hold each stage to a reference of its own) ------------------------------------------
class SequenceTail:
    """K16 from the packed sequences on (``eioku_crnn_tail``): the two BiLSTMs, Prediction and the CTC probabilities of a
    recogniser state dict.  The VGG convolutions get no weights."""

    def __init__(self, crnn_state: dict):
        import torch

        sd = _np_state(crnn_state)
        self.num_class = int(tensor(sd, "Prediction.weight").shape[0])
        self._r = Handle("crnn", self.num_class, device=torch.cuda.current_device() if torch.cuda.is_available() else 0)
        self._r.or_close(self._load, sd)

    def _load(self, sd):
        w, b = (np.ascontiguousarray(sd["Prediction." + k], np.float32) for k in ("weight", "bias"))
        _lib.check(self._r.eioku_crnn_set_conv(self._r.eioku_crnn_num_convs() - 1, ptr(w), ptr(b)), "eioku_crnn_set_conv Prediction")
        _set_lstms(self._r, sd)

    def __call__(self, seqs: list, ignore_idx=()):
        """Sequences float32 (T_i, 256) -> per sequence ``(idx int32 (T_i,), prob float32 (T_i,), logits (T_i, classes))``."""
        lens = np.array([len(s) for s in seqs], np.int32)
        packed = np.ascontiguousarray(np.concatenate([np.asarray(s, np.float32) for s in seqs]))
        rows = int(lens.sum())
        ignore = np.zeros(self.num_class, np.uint8)
        ignore[list(ignore_idx)] = 1
        idx, prob = np.empty(rows, np.int32), np.empty(rows, np.float32)
        logits = np.empty((rows, self.num_class), np.float32)
        _lib.check(self._r.eioku_crnn_tail(ptr(packed), ptr(lens), len(seqs), ptr(ignore), ptr(idx), ptr(prob),
                                           ptr(logits), None), "eioku_crnn_tail")
        o = np.concatenate([[0], np.cumsum(lens)])
        return [(idx[a:b], prob[a:b], logits[a:b]) for a, b in zip(o[:-1], o[1:])]

    def close(self):
        self._r.close()


def ctc_probs(logits, ignore):
    """``eioku_ctc_probs``: CUDA float32 (rows, C) and uint8 (C,) -> CUDA ``(idx int32 (rows,), prob float32 (rows,))``."""
    import torch

    rows, nc = (int(s) for s in logits.shape)
    idx = torch.empty(rows, dtype=torch.int32, device=logits.device)
    prob = torch.empty(rows, dtype=torch.float32, device=logits.device)
    _lib.check(_lib.load().eioku_ctc_probs(ptr(logits), rows, nc, ptr(ignore), ptr(idx), ptr(prob),
                                           torch.cuda.current_stream(logits.device).cuda_stream), "eioku_ctc_probs")
    return idx, prob


def maxpool_f16(x, c_in: tuple, kernel, stride, pad, out, c_out: tuple):
    """``eioku_ocr_maxpool_f16``: channels ``c_in = (offset, count)`` of CUDA fp16 NHWC ``x`` -> channels ``c_out[0]`` on
    of ``out`` (written in place, returned)."""
    import torch

    n, h, w, cs = (int(s) for s in x.shape)
    _lib.check(_lib.load().eioku_ocr_maxpool_f16(ptr(x), cs, c_in[0], n, h, w, c_in[1], *kernel, *stride, *pad, ptr(out),
                                                 int(out.shape[3]), c_out[0], torch.cuda.current_stream(x.device).cuda_stream),
               "eioku_ocr_maxpool_f16")
    return out


def im2col_dil_f16(x, d: int):
    """``eioku_ocr_im2col_dil_f16``: CUDA fp16 (n, h, w, c) -> (n, h, w, 9, c), the taps of a 3x3 / dilation d / pad d conv."""
    import torch

    n, h, w, c = (int(s) for s in x.shape)
    out = torch.empty((n, h, w, 9, c), dtype=torch.float16, device=x.device)
    _lib.check(_lib.load().eioku_ocr_im2col_dil_f16(ptr(x), n, h, w, c, d, ptr(out), torch.cuda.current_stream(x.device).cuda_stream),
               "eioku_ocr_im2col_dil_f16")
    return out


def up2x_f16(x, out, c_off: int = 0):
    """``eioku_ocr_up2x_f16``: CUDA fp16 (n, h, w, c) -> channels ``c_off`` on of ``out`` (n, 2h, 2w, stride), in place."""
    import torch

    n, h, w, c = (int(s) for s in x.shape)
    _lib.check(_lib.load().eioku_ocr_up2x_f16(ptr(x), n, h, w, c, ptr(out), int(out.shape[3]), c_off,
                                              torch.cuda.current_stream(x.device).cuda_stream), "eioku_ocr_up2x_f16")
    return out
