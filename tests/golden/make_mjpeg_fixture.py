"""Writes tests/golden/mjpeg_pillow.npz: the JPEG bytes Pillow (libjpeg-turbo) encodes for every case of tests/mjpeg_cases.py,
and for the cases in ``WITH_PIXELS`` the pixels Pillow decodes from them.  Needs Pillow; the tests do not.

    python tests/golden/make_mjpeg_fixture.py
"""
import io
import sys
from pathlib import Path

import numpy as np
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import mjpeg_cases as mc  # noqa: E402


def main():
    arrays = {}
    for size, content, sampling, variant in mc.ENCODED:
        name = mc.name_of(size, content, sampling, variant)
        buf = io.BytesIO()
        Image.fromarray(mc.image(size, content, sampling)).save(buf, "JPEG", **mc.save_options(sampling, variant))
        arrays["jpeg/" + name] = np.frombuffer(buf.getvalue(), np.uint8)
        if name in mc.WITH_PIXELS:
            arrays["pixels/" + name] = np.asarray(Image.open(io.BytesIO(buf.getvalue())))
    np.savez_compressed(mc.GOLDEN, **arrays)
    print(f"{mc.GOLDEN}: {len(arrays)} arrays, {mc.GOLDEN.stat().st_size} bytes")


if __name__ == "__main__":
    main()
