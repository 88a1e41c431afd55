"""The seeded random state dicts and the folded states, pinned bit for bit.

``tests/golden/state_fold_digests.json`` holds a sha256 per array (dtype, shape and bytes), key by key, of what
``random_state_dict`` / ``random_*_state`` draw and of what ``fold_state`` / ``fold_conv`` / ``lstm_params`` make of it,
recorded before the state-dict helpers moved to ``eioku_amd/_state.py``.  The GPU tolerances of the suite were chosen
against exactly these weights, so a refactor of the helpers must not move a bit of them.  Each input is also folded
once wrapped as ``{"state_dict": {"module." + key: value}}`` (speakers: ``"module.resnet."`` too).
"""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from eioku_amd import faces, ocr, places, speakers

FIXTURE = Path(__file__).parent / "golden" / "state_fold_digests.json"


def digest(a) -> str:
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()


def flatten(obj, at="") -> dict:
    """Nested dicts / tuples / lists of arrays -> ``{"a/b/0": digest}``."""
    if isinstance(obj, dict):
        items = obj.items()
    elif isinstance(obj, (tuple, list)) and not all(isinstance(v, (int, np.integer)) for v in obj):
        items = enumerate(obj)
    else:
        return {at: digest(np.asarray(obj))}
    out = {}
    for k, v in items:
        out.update(flatten(v, f"{at}/{k}" if at else str(k)))
    return out


def resnet18_state_dict() -> dict:
    """The torchvision-shaped dict of ``test_places_host.test_fold_state_handles_the_release_checkpoint_layout``."""
    from oracle import places as op

    rng = np.random.default_rng(2)
    sd = {}

    def conv_bn(cname, bname, co, ci, k):
        sd[cname + ".weight"] = rng.standard_normal((co, ci, k, k)).astype(np.float32)
        for nm, v in (("weight", rng.uniform(0.5, 1.5, co)), ("bias", rng.standard_normal(co)),
                      ("running_mean", rng.standard_normal(co)), ("running_var", rng.uniform(0.5, 2, co))):
            sd[f"{bname}.{nm}"] = v.astype(np.float32)
        sd[f"{bname}.num_batches_tracked"] = np.int64(7)

    for name, co, ci, k, _ in op.LAYERS:
        if name == "conv1":
            conv_bn("conv1", "bn1", co, ci, k)
        elif "downsample" in name:
            conv_bn(name, name[:-1] + "1", co, ci, k)
        else:
            conv_bn(name, name.replace("conv", "bn"), co, ci, k)
    sd["fc.weight"] = rng.standard_normal((365, 512)).astype(np.float32)
    sd["fc.bias"] = rng.standard_normal(365).astype(np.float32)
    return sd


def fold_craft(sd):
    sd = ocr._np_state(sd)
    return {name: ocr.fold_conv(sd, name) for name, *_ in ocr.CRAFT_CONVS}


def fold_crnn(sd):
    sd = ocr._np_state(sd)
    out = {name: ocr.fold_conv(sd, name) for name in [n for n, *_ in ocr.CRNN_CONVS] + ["Prediction"]}
    out["lstm"] = [ocr.lstm_params(sd, l) for l in range(2)]
    return out


# model -> (raw state dict, fold, prefixes the wrapped form is taken with)
CASES = {
    "faces": (lambda: faces.random_state_dict(3, (1, 1, 1, 1)), faces.fold_state, ("module.",)),
    "speakers": (lambda: speakers.random_state_dict(3, (1, 1, 1, 1)), speakers.fold_state, ("module.", "module.resnet.")),
    "craft": (lambda: ocr.random_craft_state(5), fold_craft, ("module.",)),
    "crnn": (lambda: ocr.random_crnn_state(6), fold_crnn, ("module.",)),
    "places": (resnet18_state_dict, places.fold_state, ("module.",)),
}


def compute(model: str) -> dict:
    make, fold, prefixes = CASES[model]
    raw = make()
    out = {"raw": flatten(raw), "folded": flatten(fold(raw))}
    for p in prefixes:
        out["folded:" + p] = flatten(fold({"state_dict": {p + k: v for k, v in raw.items()}}))
    return out


@pytest.mark.parametrize("model", sorted(CASES))
def test_random_and_folded_states_are_bit_for_bit_the_recorded_ones(model):
    want = json.loads(FIXTURE.read_text())[model]
    got = compute(model)
    assert sorted(got) == sorted(want)
    for part in want:
        assert sorted(got[part]) == sorted(want[part]), part
        moved = [k for k in want[part] if got[part][k] != want[part][k]]
        assert not moved, f"{model} {part}: {len(moved)} arrays changed, first {moved[:3]}"
    for part in want:
        if part.startswith("folded:"):
            assert got[part] == got["folded"], f"{part} folds differently from the bare keys"
