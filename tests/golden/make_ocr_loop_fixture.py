"""Writes ref_ocr_loop.json: the reference's ``ModelManager.extract_ocr`` (ml-service/src/services/model_manager.py:
469-558) run over a scripted capture, with the stub ``cv2`` of make_reference_fixtures.py and a stub ``easyocr`` module
whose ``Reader.readtext(frame)`` returns scripted ``(box, text, confidence)`` results keyed by the frame number carried
in pixel (0, 0).  It pins the sampling rule, timestamps, the language handling, the detection dict and the result dict;
the OCR arithmetic itself is not pinned by it (tests/test_ocr_gpu.py compares that with tests/ocr_oracle.py).

    python tests/golden/make_ocr_loop_fixture.py      (needs the reference tree)
"""
from __future__ import annotations

import asyncio
import json
import sys
import tempfile
import types
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
from make_reference_fixtures import REF, install_stubs  # noqa: E402


def ocr_results(seed: int, frame_idx: int) -> list:
    """What the stub reader returns for a frame: 0-2 results with int and float box corners."""
    k = (seed * 7 + frame_idx) % 3
    out = []
    for j in range(k):
        x, y = 10 * j + frame_idx % 17, 5 + j
        if j == 0:
            box = [[x, y], [x + 40, y], [x + 40, y + 12], [x, y + 12]]
        else:
            box = [[x + 0.5, y + 0.25], [x + 30.75, y + 3.5], [x + 29.125, y + 15.0], [x - 1.5, y + 11.75]]
        out.append((box, f"w{seed}_{frame_idx}_{j}", 0.5 + 0.0625 * j + frame_idx / 4096))
    return out


def install_easyocr_stub(seed: int) -> list:
    calls = []
    mod = types.ModuleType("easyocr")

    class Reader:
        def __init__(self, langs, gpu=False, verbose=True):
            calls.append({"langs": list(langs)})

        def readtext(self, frame):
            idx = int(frame[0, 0, 0]) | (int(frame[0, 0, 1]) << 8) | (int(frame[0, 0, 2]) << 16)
            calls.append({"frame_index": idx})
            return ocr_results(seed, idx)

    mod.Reader = Reader
    sys.modules["easyocr"] = mod
    return calls


def capture_ocr_loop(ModelManager) -> list:
    specs = [
        (30.0, 200, {}),                                   # defaults: every 2 s, language "en"
        (29.97, 301, {"frame_interval": 1.5, "language": "en"}),
        (23.976, 97, {"frame_interval": 0.5, "languages": ["en"]}),
        (0.0, 70, {"languages": "en"}),                    # fps 0 -> `or 30`; languages as a string
        (60.0, 40, {"frame_interval": 0.001, "languages": []}),  # max(1, int(...)); empty list -> "en"
        (25.0, 0, {}),                                     # empty video
    ]
    cases = []
    for seed, (fps, total, config) in enumerate(specs, start=31):
        install_stubs(fps, total, seed, {})
        calls = install_easyocr_stub(seed)
        with tempfile.TemporaryDirectory() as td:
            result = asyncio.run(ModelManager(cache_dir=td).extract_ocr("/videos/fake.mp4", dict(config)))
        cases.append({"fps": fps, "total_frames": total, "config": config, "seed": seed, "reader_calls": calls, "result": result})
    return cases


def main():
    if not REF.exists():
        sys.exit("needs the reference tree (build container only)")
    sys.path.insert(0, str(REF))
    from src.services.model_manager import ModelManager

    (HERE / "ref_ocr_loop.json").write_text(json.dumps(capture_ocr_loop(ModelManager)) + "\n")
    print("wrote", HERE / "ref_ocr_loop.json")


if __name__ == "__main__":
    main()
