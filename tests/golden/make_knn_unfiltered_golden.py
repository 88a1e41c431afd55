"""Record (D, I) of plain ``IndexFlatL2.search`` calls for tests/test_knn_filtered_gpu.py::test_unfiltered_search_is_
byte_identical_to_the_parent_build.

Run on the GPU against the build of the commit BEFORE row selectors and removal were added (the recorded file
``knn_unfiltered_parent.npz`` came from commit 14bec8a):

    python tests/golden/make_knn_unfiltered_golden.py tests/golden/knn_unfiltered_parent.npz

Shapes: three of test_knn_scan_gpu.py::test_scan_matches_float64_truth (scan path, ``scan_min_rows`` lowered as that
file's ``scan_index`` does) and three of test_knn_gpu.py::test_search_matches_float64_truth (register-tile kernels).
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from eioku_amd import search  # noqa: E402
from oracle import prng  # noqa: E402

# (n, nq, k, d, scan_rt or None = default index, seeds)
CASES = [(20000, 70, 10, 384, 1, 31, 32), (33333, 200, 16, 256, 1, 31, 32), (70001, 257, 10, 384, 2, 31, 32),
         (4096, 16, 10, 384, None, 21, 22), (5000, 70, 10, 384, None, 21, 22), (3000, 5, 32, 384, None, 21, 22)]


def unit_rows(seed, n, d):
    x = prng.approx_normal_f32(seed, n * d).reshape(n, d)
    return (x / np.sqrt((x.astype(np.float64) ** 2).sum(1, keepdims=True))).astype(np.float32)


def run_case(n, nq, k, d, rt, seed_db, seed_q):
    ix = search.IndexFlatL2(d)
    if rt is not None:
        ix.set_param("scan_min_rows", 4096)
        ix.set_param("scan_mode", 1)
        ix.set_param("scan_rt", rt)
    ix.add(unit_rows(seed_db, n, d))
    D, I = ix.search(unit_rows(seed_q, nq, d), k)
    ix.close()
    return D, I


if __name__ == "__main__":
    out = {}
    for c, case in enumerate(CASES):
        out[f"D{c}"], out[f"I{c}"] = run_case(*case)
        out[f"I{c}"] = out[f"I{c}"].astype(np.int32)  # ids < 2^31; the test widens them again
    np.savez_compressed(sys.argv[1], **out)
    print("wrote", sys.argv[1])
