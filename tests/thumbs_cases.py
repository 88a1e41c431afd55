"""Inputs shared by the thumbnail tests and the golden generator (a helper, not a test): seeded, so that every user
builds the same bytes."""
from __future__ import annotations

import zlib

import numpy as np

# (height, width, quality) with random bytes: block-edge, dummy-block, odd-size, chroma-row-padding (94 vs 95) and
# multi-MCU shapes, the 1 x 1 image and the default thumbnail size
RANDOM_CASES = [(16, 16, 95), (24, 40, 75), (8, 40, 90), (17, 33, 75), (31, 47, 30), (94, 150, 60), (95, 150, 60), (90, 160, 85),
                (180, 320, 85), (9, 9, 75), (1, 1, 75), (64, 64, 75), (64, 64, 95)]
CONTENTS = ("ramp", "checker", "constant")
# every (content, h, w, q) a JPEG test runs
JPEG_CASES = [("random", *c) for c in RANDOM_CASES] + [(c, 64, 64, q) for c in CONTENTS for q in (75, 95)]
# (h, w) -> (th, tw)
RESIZE_CASES = [((37, 53), (16, 23)), ((20, 12), (32, 19)), ((90, 160), (45, 80)), ((270, 480), (180, 320))]
# the five inputs whose Pillow bytes are committed in tests/golden/thumbs_pillow.npz
GOLDEN_JPEG = [("random", 24, 40, 75), ("random", 94, 150, 60), ("random", 1, 1, 75), ("ramp", 64, 64, 95), ("checker", 64, 64, 75)]
GOLDEN_RESIZE = [((37, 53), (16, 23)), ((20, 12), (32, 19))]


def image(content: str, h: int, w: int, variant: int = 0) -> np.ndarray:
    """(h,w,3) uint8 RGB.  ``variant`` picks another image of the same kind (the GPU tests encode three per call)."""
    yy, xx = np.mgrid[0:h, 0:w]
    if content == "random":
        seed = zlib.crc32(f"{h}x{w}/{variant}".encode())
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if content == "ramp":
        # a smooth ramp with a faint ripple at the highest DCT frequency: at quality 95 the (7,7) coefficient survives
        # behind a long run of zeros, so the stream needs ZRL symbols
        base = np.stack([xx * 3 + yy + 5 * variant, 250 - yy * 3 - variant, (xx + yy) * 2], -1).astype(np.float64)
        ripple = np.rint(3 * np.cos(np.pi * (2 * xx + 1) * 7 / 16) * np.cos(np.pi * (2 * yy + 1) * 7 / 16))
        return np.clip(base + ripple[..., None], 0, 255).astype(np.uint8)
    if content == "checker":  # 0 / 255 at pixel pitch: the largest coefficients
        return np.repeat(((((yy + xx + variant) & 1) * 255).astype(np.uint8))[..., None], 3, -1)
    if content == "constant":  # every AC coefficient is zero
        return np.full((h, w, 3), [(10, 200, 90), (255, 255, 255), (0, 0, 0)][variant % 3], np.uint8)
    raise ValueError(content)


def case_id(case) -> str:
    content, h, w, q = case
    return f"{content}-{h}x{w}-q{q}"
