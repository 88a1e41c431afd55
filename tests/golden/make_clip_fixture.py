"""Writes tests/golden/clip_preproc.npz: the K26 image preprocessing as Pillow computes it.

For each source size, three seeded BGR frames and the resized and centre-cropped uint8 RGB image from Pillow itself
(``Image.resize(size, BICUBIC)`` of the short edge to 64, the long edge to ``int(64 * long / short)``, crop offsets ``(dim -
64) // 2``), and the normalised float32 values ``(v / 255 - mean) / std`` with OpenAI's CLIP mean and std, computed in
float64 and rounded once.

    python tests/golden/make_clip_fixture.py
"""
from pathlib import Path

import numpy as np
from PIL import Image

TARGET = 64
SOURCES = [(54, 96), (96, 54), (30, 40), (64, 64), (49, 97)]  # (h, w): landscape, portrait, upscale, identity, odd
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)


def main():
    out = {}
    for i, (h, w) in enumerate(SOURCES):
        rng = np.random.default_rng(200 + i)
        # smooth structure plus noise: flat noise alone would hide a shifted crop; hard edges make the bicubic lobes clip
        yy, xx = np.mgrid[0:h, 0:w]
        base = (np.sin(yy / 5.0)[..., None] * 70 + np.cos(xx / 7.0)[..., None] * 70 + 128)
        bgr = np.clip(base + rng.normal(0, 45, (3, h, w, 3)), 0, 255).astype(np.uint8)
        rh, rw = (TARGET, int(TARGET * w / h)) if h <= w else (int(TARGET * h / w), TARGET)
        top, left = (rh - TARGET) // 2, (rw - TARGET) // 2
        u8 = np.stack([np.asarray(Image.fromarray(f[..., ::-1].copy()).resize((rw, rh), Image.BICUBIC))[top:top + TARGET,
                                                                                                       left:left + TARGET]
                       for f in bgr])
        norm = ((u8.astype(np.float64) / 255.0 - np.asarray(MEAN)) / np.asarray(STD)).astype(np.float32)
        out[f"bgr_{h}x{w}"] = bgr
        out[f"u8_{h}x{w}"] = u8
        out[f"norm_{h}x{w}"] = norm
    path = Path(__file__).resolve().parent / "clip_preproc.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
