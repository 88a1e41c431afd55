"""fp32 torch restatement of EasyOCR 1.7.2's CRAFT (``craft.CRAFT`` on ``modules.vgg16_bn``) and of its ``english_g2``
recogniser (``model/vgg_model.Model``), reading the same state dicts as ``eioku_amd.ocr``.

Written from the published model definitions (EasyOCR is not installed where this suite runs, so it is not diffed
against EasyOCR itself).  Layers keep the state dict's own modules (BatchNorm unfolded), so the folding in
``eioku_amd.ocr.fold_conv`` is checked too.  The post-processing and decode the GPU tests compare against are the
numpy functions of ``eioku_amd.ocr`` (``det_boxes``: ``craft_utils.getDetBoxes_core``; ``adjust_coordinates``:
``adjustResultCoordinates``; ``group_text_box``: ``utils.group_text_box``; ``decode_greedy``:
``CTCLabelConverter.decode_greedy``; ``confidence``: ``recognizer_predict`` + ``utils.custom_mean``), pinned on the CPU by
``tests/test_ocr_host.py`` with hand-computed cases.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from eioku_amd import ocr

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _t(sd, k):
    return torch.from_numpy(np.asarray(sd[k], np.float32))


def _conv(sd, name, x, pad=1, dil=1):
    b = _t(sd, name + ".bias") if name + ".bias" in sd else None
    return F.conv2d(x, _t(sd, name + ".weight"), b, padding=pad, dilation=dil)


def _bn(sd, name, x):
    return F.batch_norm(x, _t(sd, name + ".running_mean"), _t(sd, name + ".running_var"), _t(sd, name + ".weight"),
                        _t(sd, name + ".bias"), False, 0.0, 1e-5)


def _cbr(sd, conv, bn, x, relu=True, pad=1):
    y = _bn(sd, bn, _conv(sd, conv, x, pad))
    return F.relu(y) if relu else y


def craft_input(frames_bgr: np.ndarray, canvas: int = ocr.CANVAS) -> tuple:
    """``resize_aspect_ratio`` + ``normalizeMeanVariance`` on BGR uint8 (n, h, w, 3) -> (NCHW fp32, ratio)."""
    n, h, w, _ = frames_bgr.shape
    ratio, th, tw, H, W = ocr.craft_canvas(h, w, canvas)
    out = np.zeros((n, H, W, 3), np.float32)
    for i in range(n):
        out[i, :th, :tw] = ocr.resize_linear_u8(frames_bgr[i], th, tw)
    out -= np.array([m * 255.0 for m in MEAN], np.float32)
    out /= np.array([s * 255.0 for s in STD], np.float32)
    return torch.from_numpy(out).permute(0, 3, 1, 2).contiguous(), ratio


def craft(sd: dict, x: torch.Tensor) -> torch.Tensor:
    """CRAFT forward: NCHW canvas -> (n, H/2, W/2, 2) (text, link)."""
    sd = ocr._np_state(sd)
    mp = lambda t: F.max_pool2d(t, 2, 2)
    # vgg16_bn basenet: every slice ends at a BatchNorm output.  Slices 2-4 open with torchvision's ReLU(inplace=True),
    # which also rewrites the tensor CRAFT saved for its skip (h_relu2_2 = h; h = self.slice2(h)): relu2_2, relu3_2 and
    # relu4_3 reach the concats ReLU'd.  slice5 opens with a MaxPool, so relu5_3 keeps its negative values.
    h = _cbr(sd, "basenet.slice1.0", "basenet.slice1.1", x)
    h = mp(_cbr(sd, "basenet.slice1.3", "basenet.slice1.4", h))
    h = _cbr(sd, "basenet.slice1.7", "basenet.slice1.8", h)
    relu2_2 = _cbr(sd, "basenet.slice1.10", "basenet.slice1.11", h)
    h = _cbr(sd, "basenet.slice2.14", "basenet.slice2.15", mp(relu2_2))
    relu3_2 = _cbr(sd, "basenet.slice2.17", "basenet.slice2.18", h)
    h = mp(_cbr(sd, "basenet.slice3.20", "basenet.slice3.21", relu3_2))
    h = _cbr(sd, "basenet.slice3.24", "basenet.slice3.25", h)
    relu4_3 = _cbr(sd, "basenet.slice3.27", "basenet.slice3.28", h)
    h = mp(_cbr(sd, "basenet.slice4.30", "basenet.slice4.31", relu4_3))
    h = _cbr(sd, "basenet.slice4.34", "basenet.slice4.35", h)
    relu5_3 = _cbr(sd, "basenet.slice4.37", "basenet.slice4.38", h, relu=False)
    h = F.max_pool2d(relu5_3, 3, 1, 1)
    h = _conv(sd, "basenet.slice5.1", h, pad=6, dil=6)
    fc7 = _conv(sd, "basenet.slice5.2", h, pad=0)

    def double_conv(p, t):
        t = _cbr(sd, p + ".conv.0", p + ".conv.1", t, pad=0)
        return _cbr(sd, p + ".conv.3", p + ".conv.4", t)

    y = double_conv("upconv1", torch.cat([fc7, relu5_3], 1))
    y = F.interpolate(y, size=relu4_3.shape[2:], mode="bilinear", align_corners=False)
    y = double_conv("upconv2", torch.cat([y, relu4_3], 1))
    y = F.interpolate(y, size=relu3_2.shape[2:], mode="bilinear", align_corners=False)
    y = double_conv("upconv3", torch.cat([y, relu3_2], 1))
    y = F.interpolate(y, size=relu2_2.shape[2:], mode="bilinear", align_corners=False)
    y = double_conv("upconv4", torch.cat([y, relu2_2], 1))
    for i in (0, 2, 4):
        y = F.relu(_conv(sd, f"conv_cls.{i}", y))
    y = F.relu(_conv(sd, "conv_cls.6", y, pad=0))
    y = _conv(sd, "conv_cls.8", y, pad=0)
    return y.permute(0, 2, 3, 1)


def crnn_logits(sd: dict, x: torch.Tensor) -> torch.Tensor:
    """english_g2 ``Model.forward``: (b, 1, 64, W) -> logits (b, W/4 - 1, num_class)."""
    sd = ocr._np_state(sd)
    p = "FeatureExtraction.ConvNet."
    h = F.max_pool2d(F.relu(_conv(sd, p + "0", x)), 2, 2)
    h = F.max_pool2d(F.relu(_conv(sd, p + "3", h)), 2, 2)
    h = F.relu(_conv(sd, p + "8", F.relu(_conv(sd, p + "6", h))))
    h = F.max_pool2d(h, (2, 1), (2, 1))
    h = F.relu(_bn(sd, p + "12", _conv(sd, p + "11", h)))
    h = F.relu(_bn(sd, p + "15", _conv(sd, p + "14", h)))
    h = F.max_pool2d(h, (2, 1), (2, 1))
    h = F.relu(_conv(sd, p + "18", h, pad=0))
    v = F.adaptive_avg_pool2d(h.permute(0, 3, 1, 2), (None, 1)).squeeze(3)  # [b, w, c]
    for l in range(2):
        q = f"SequenceModeling.{l}."
        rnn = torch.nn.LSTM(256, 256, bidirectional=True, batch_first=True)
        rnn.load_state_dict({k[len(q + "rnn."):]: _t(sd, k) for k in sd if k.startswith(q + "rnn.")})
        with torch.no_grad():
            r, _ = rnn(v)
        v = F.linear(r, _t(sd, q + "linear.weight"), _t(sd, q + "linear.bias"))
    return F.linear(v, _t(sd, "Prediction.weight"), _t(sd, "Prediction.bias"))


def crnn_probs(sd: dict, imgs: list, ignore_idx) -> list:
    """``recognizer_predict`` per crop (each alone, as readtext's batch_size=1): float32 (64, W) -> (idx, prob, logits)."""
    out = []
    with torch.no_grad():
        for a in imgs:
            lg = crnn_logits(sd, torch.from_numpy(np.asarray(a, np.float32))[None, None])[0]
            p = ocr.ignore_renormalise(F.softmax(lg, dim=-1).numpy(), ignore_idx)
            out.append((p.argmax(-1).astype(np.int32), p.max(-1), lg.numpy()))
    return out
