"""Regenerate tests/golden/thumbs_pillow.npz: what Pillow (with libjpeg-turbo) makes of five of the thumbnail tests' inputs.

    python tests/golden/make_thumbs_fixture.py

For each of ``thumbs_cases.GOLDEN_JPEG`` the RGB input and the bytes of ``Image.save(buf, "JPEG", quality=q)``; for each of
``thumbs_cases.GOLDEN_RESIZE`` the input and ``Image.resize((tw, th), Resampling.BICUBIC)``.  It lets a machine without
Pillow (the GPU box) compare the device's files with Pillow's.
"""
import io
import sys
from pathlib import Path

import numpy as np
import PIL
from PIL import Image, features

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import thumbs_cases as tc  # noqa: E402


def main():
    out = {"pillow_version": np.array(PIL.__version__), "libjpeg_version": np.array(str(features.version("jpg")))}
    for i, (content, h, w, q) in enumerate(tc.GOLDEN_JPEG):
        rgb = tc.image(content, h, w)
        buf = io.BytesIO()
        Image.fromarray(rgb).save(buf, "JPEG", quality=q)
        out[f"jpeg{i}_case"] = np.array(tc.case_id((content, h, w, q)))
        out[f"jpeg{i}_rgb"] = rgb
        out[f"jpeg{i}_file"] = np.frombuffer(buf.getvalue(), np.uint8)
    for i, ((h, w), (th, tw)) in enumerate(tc.GOLDEN_RESIZE):
        rgb = tc.image("random", h, w, variant=7)
        out[f"resize{i}_rgb"] = rgb
        out[f"resize{i}_out"] = np.asarray(Image.fromarray(rgb).resize((tw, th), Image.Resampling.BICUBIC))
    path = HERE / "thumbs_pillow.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
