"""GPU: the straight-line epilogue of k_conv3x3_flat against store_frag's generic loop.

The specialised epilogue (fp16 output, whole cout tile inside Cout, SiLU or no activation, no residual or the pre-loaded
vector residual) does store_frag's arithmetic in store_frag's order, so its output must be the same BYTES, canaries
and all, and the launch code must have started the same instantiations.  EIOKU_CONV_EPI is read once per process: the
table of tests/conv_epilogue_cases.py runs once in a fresh child process per setting (two children for the whole file)
and every test below compares what the two wrote.  Which loop ran is read from the launch code's own counter
(``ops.conv_epi_launches``): 1 per flat launch of the common case with the switch on, 0 with it off, and 0 either way for
the k_conv3x3_persist layers, which keep the generic loop (three copies of their tile loop cost them registers and
occupancy) and whose bytes must not move."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import conv_epilogue_cases as cases

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    """{"on" | "off": ({name: bytes of the output buffer}, {name: route log}, {name: straight-line launches})}"""
    out = {}
    tmp = tmp_path_factory.mktemp("conv_epi")
    for name in ("on", "off"):
        env = {k: v for k, v in os.environ.items() if k != "EIOKU_CONV_EPI"}
        if name == "off":
            env["EIOKU_CONV_EPI"] = "0"
        path = tmp / f"{name}.npz"
        r = subprocess.run([sys.executable, str(ROOT / "tests" / "conv_epilogue_cases.py"), str(path)], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        with np.load(path) as z:
            arrays = {k: z[k] for k in z.files}
        log = json.loads(Path(str(path) + ".routes.json").read_text())
        out[name] = (arrays, log["routes"], log["epi"])
    return out


def _same(runs, name):
    (on, ron, _), (off, roff, _) = runs["on"], runs["off"]
    assert ron.get(name) == roff.get(name), (ron.get(name), roff.get(name))
    assert on[name].shape == off[name].shape and on[name].size > 0
    assert np.array_equal(on[name], off[name]), f"{name}: {int((on[name] != off[name]).sum())} bytes differ"
    return on[name], ron.get(name)


@pytest.mark.parametrize("variant", [v[0] for v in cases.VARIANTS])
@pytest.mark.parametrize("layer", cases.LAYERS, ids=[l[0] for l in cases.LAYERS])
def test_specialised_epilogue_writes_the_generic_bytes(runs, layer, variant):
    name, (n, h, w, cin, cout, stride), route = layer
    got, log = _same(runs, f"{name}-{variant}")
    assert len(log) == 1 and next(iter(log)).startswith(route) and set(log.values()) == {1}, log
    # the two runs went through different loops exactly where the specialised one exists
    key = f"{name}-{variant}"
    assert runs["off"][2][key] == 0 and runs["on"][2][key] == (1 if route.startswith("flat<") else 0)
    # the layer did run and left its neighbours alone: channels [4, 4 + cout) written (no 7.0 pattern survives on a whole
    # pixel), the 4 channels before and after still 7.0
    ho, wo = cases.out_dims(h, w, stride)
    buf = got.view(np.float16).reshape(n, ho, wo, cout + 8)
    assert np.all(buf[..., :4] == 7.0) and np.all(buf[..., 4 + cout:] == 7.0)
    body = buf[..., 4:4 + cout]
    assert np.isfinite(body).all() and not np.any(np.all(body == 7.0, axis=-1))


@pytest.mark.parametrize("case", cases.FALLBACK, ids=[c[0] for c in cases.FALLBACK])
def test_layers_outside_the_common_case_keep_the_generic_loop(runs, case):
    name, (n, h, w, cin, cout, stride), act, res, f32 = case
    got, log = _same(runs, name)
    assert "refused" not in log and len(log) == 1, log
    assert runs["on"][2][name] == 0 and runs["off"][2][name] == 0
    ho, wo = cases.out_dims(h, w, stride)
    if f32:
        buf = got.view(np.float32)
        assert buf.size == n * ho * wo * cout + 2 * cases.GUARD
        assert np.all(buf[:cases.GUARD] == 7.0) and np.all(buf[-cases.GUARD:] == 7.0) and np.isfinite(buf).all()
    else:
        cpad = (cout + 3) // 4 * 4
        buf = got.view(np.float16).reshape(n, ho, wo, cpad + 8)
        assert np.all(buf[..., :4] == 7.0) and np.all(buf[..., 4 + cout:] == 7.0) and np.isfinite(buf).all()


def test_workgroups_that_walk_several_tiles_match_the_batch_run_in_halves(runs):
    """From a workgroup's second tile on the residual loads sit in the queue behind the previous prefetch and in front of
    the next one.  The halves run a different number of tiles per workgroup."""
    whole, log = _same(runs, "steady")
    halves, _ = _same(runs, "steady_halves")
    assert list(log.values()) == [3] and next(iter(log)).startswith("persist<NF2,S1,NCH2,"), log
    assert np.array_equal(whole, halves)
    assert np.isfinite(whole.view(np.float16)).all()


def test_yolov8n_detections_are_the_same_bytes(runs):
    (on, ron, eon), (off, roff, eoff) = runs["on"], runs["off"]
    assert ron["yolo"] == roff["yolo"]
    assert eon["yolo"] > 0 and eoff["yolo"] == 0
    assert any(r.startswith("persist<") for r in ron["yolo"]) and any(r.startswith("flat<") for r in ron["yolo"]), ron["yolo"]
    for key in ("yolo_dets", "yolo_counts"):
        assert on[key].shape == off[key].shape and np.array_equal(on[key], off[key]), key
    assert int(on["yolo_counts"].sum()) > 0
