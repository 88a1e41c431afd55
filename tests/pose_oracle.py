"""Oracle of the Pose head (the keypoint branch ``cv4`` and K6p): ``oracle.yolo.Net`` with Ultralytics' ``Pose.forward``
on top, and ``Pose.kpts_decode`` + ``ops.scale_coords`` restated in numpy float32.

**Parity unpinned** [PUBLIC-LIB], as ``oracle/yolo.py``: ultralytics is not installed where this suite runs.  Restated
from memory of ultralytics 8.x: ``kpts_decode`` computes ``(r[..., :2] * 2.0 + (anchors - 0.5)) * strides`` and a
sigmoid on the third value; ``scale_coords`` subtracts the unrounded padding ``(img1 - img0 * gain) / 2``, divides by the
gain and clips to the original image (``scale_boxes`` rounds that padding, ``scale_coords`` does not).
"""
from __future__ import annotations

import numpy as np

from oracle import yolo as oy


class PoseNet(oy.Net):
    """``oracle.yolo.Net`` plus ``cv4[l] = Conv -> Conv -> Conv2d`` on the three Detect inputs."""

    def forward_pose(self, x):
        """-> (box[3], cls[3], kpt[3]) float32 NHWC numpy arrays; box and cls are ``Net.forward``'s own."""
        import torch

        feats = []
        conv = self.conv

        def tap(name, t, *a, **k):  # the Detect inputs are what cv2.<l>.0 reads
            if name.startswith("model.22.cv2.") and name.endswith(".0.conv"):
                feats.append(t)
            return conv(name, t, *a, **k)

        self.conv = tap
        try:
            box, cls = self.forward(x)
        finally:
            self.conv = conv
        kpt = []
        with torch.no_grad():
            for l, f in enumerate(feats):
                k = self.conv(f"model.22.cv4.{l}.1.conv", self.conv(f"model.22.cv4.{l}.0.conv", f))
                kpt.append(self.conv(f"model.22.cv4.{l}.2", k, act=False, keep_f32=True).permute(0, 2, 3, 1).contiguous().numpy())
        return box, cls, kpt


def kpt_pad(lb_shape, orig_shape, gain32) -> tuple:
    """``scale_coords``' padding with the float32 gain the device is given, rounded to float32 once."""
    g = float(np.float32(gain32))
    return (np.float32((lb_shape[1] - orig_shape[1] * g) / 2), np.float32((lb_shape[0] - orig_shape[0] * g) / 2))


def kpts_decode(kpt_maps, anchors, image: int, lb_shape, orig_shape, gain) -> np.ndarray:
    """Keypoints ``(len(anchors), K, 3)`` float32 of the listed anchors (indices into P3 | P4 | P5) of one image."""
    f32 = np.float32
    sizes = [m.shape[1] * m.shape[2] for m in kpt_maps]
    px, py = kpt_pad(lb_shape, orig_shape, gain)
    g = f32(gain)
    out = []
    for a in anchors:
        l = 0
        while a >= sizes[l]:
            a -= sizes[l]
            l += 1
        m = kpt_maps[l]
        gy, gx = divmod(int(a), m.shape[2])
        r = m[image, gy, gx].astype(f32).reshape(-1, 3)
        stride = f32(8 << l)
        x = ((r[:, 0] * f32(2) + f32(gx)).astype(f32) * stride).astype(f32)
        y = ((r[:, 1] * f32(2) + f32(gy)).astype(f32) * stride).astype(f32)
        x = np.clip(((x - px).astype(f32) / g).astype(f32), f32(0), f32(orig_shape[1]))
        y = np.clip(((y - py).astype(f32) / g).astype(f32), f32(0), f32(orig_shape[0]))
        with np.errstate(over="ignore"):
            c = (f32(1) / (f32(1) + np.exp(-r[:, 2]).astype(f32))).astype(f32)
        out.append(np.stack([x, y, c], -1))
    return np.asarray(out, f32).reshape(-1, kpt_maps[0].shape[-1] // 3, 3)
