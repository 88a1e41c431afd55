"""Writes tests/golden/actions_preproc.npz: the K25 clip preprocessing as ``transformers`` and Pillow compute it.

For each source size, three seeded BGR frames, the resized and centre-cropped uint8 RGB image from Pillow itself
(``Image.resize(..., BILINEAR)`` of the short edge to 48, the long edge to ``int(48 * long / short)``, crop offsets
``(dim - 48) // 2``), and the normalised float32 values from ``VideoMAEImageProcessorPil`` (mean 0.45, std 0.225).  The
script asserts that the two agree (the processor's output is the normalised Pillow image) before it writes.

    python tests/golden/make_actions_fixture.py
"""
from pathlib import Path

import numpy as np
from PIL import Image
from transformers import VideoMAEImageProcessorPil

TARGET = 48
SOURCES = [(54, 96), (96, 54), (30, 40), (48, 48), (49, 97)]  # (h, w): landscape, portrait, upscale, identity, odd


def main():
    proc = VideoMAEImageProcessorPil(size={"shortest_edge": TARGET}, crop_size={"height": TARGET, "width": TARGET},
                                     image_mean=[0.45] * 3, image_std=[0.225] * 3)
    out = {}
    for i, (h, w) in enumerate(SOURCES):
        rng = np.random.default_rng(100 + i)
        # smooth structure plus noise: flat noise alone would hide a shifted crop
        yy, xx = np.mgrid[0:h, 0:w]
        base = (np.sin(yy / 5.0)[..., None] * 60 + np.cos(xx / 7.0)[..., None] * 60 + 128)
        bgr = np.clip(base + rng.normal(0, 40, (3, h, w, 3)), 0, 255).astype(np.uint8)
        rh, rw = (TARGET, int(TARGET * w / h)) if h <= w else (int(TARGET * h / w), TARGET)
        top, left = (rh - TARGET) // 2, (rw - TARGET) // 2
        u8 = np.stack([np.asarray(Image.fromarray(f[..., ::-1].copy()).resize((rw, rh), Image.BILINEAR))[top:top + TARGET,
                                                                                                        left:left + TARGET]
                       for f in bgr])
        pv = proc([[f[..., ::-1].copy() for f in bgr]], return_tensors="np")["pixel_values"][0]  # (T, 3, S, S)
        norm = np.ascontiguousarray(pv.transpose(0, 2, 3, 1)).astype(np.float32)
        mine = (u8.astype(np.float32) * np.float32(1 / 255) - np.float32(0.45)) / np.float32(0.225)
        assert np.abs(mine - norm).max() < 1e-6, np.abs(mine - norm).max()
        out[f"bgr_{h}x{w}"] = bgr
        out[f"u8_{h}x{w}"] = u8
        out[f"norm_{h}x{w}"] = norm
    path = Path(__file__).resolve().parent / "actions_preproc.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
