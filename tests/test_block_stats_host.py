"""Host side of the per-channel and border bars of the block tests (tests/block_stats.py): no GPU.

The bars are 2 x the fp16 twin's own figures against torch fp32, so the twins must be what they claim (close to fp32, not equal
to it), and the seeds the GPU tests use must leave at most 5 % of the channels out of the channel figure as dead.  Prints the
twin's figures at every test point ("ConvNet glue parity")."""
import numpy as np
import pytest
import torch

import block_stats
import face_oracle as fo
import speaker_oracle as so
from eioku_amd import faces, speakers
from oracle import places as op
from test_faces_gpu import BOXES, FP32_MAX, FP32_MEAN, _frames
from test_places_gpu import textured
from test_speakers_gpu import CASES, _audio, _plan


def _twin_is_a_twin(name, twin, want):
    f = block_stats.figures(twin, want)
    rms = np.sqrt((want ** 2).mean())
    err = np.abs(twin - want)
    print(f"{name}: twin worst channel {f['channel']:.3e} (bar {block_stats.FACTOR * f['channel']:.3e}), ring / interior "
          f"{f['ring']:.3f} (bar {block_stats.FACTOR * f['ring']:.3f}), left out {f['left_out']:.3f}; whole tensor mean "
          f"{err.mean() / rms:.2e} max {err.max() / rms:.2e}")
    assert f["left_out"] <= block_stats.MAX_LEFT_OUT, f"{name}: choose another seed"
    assert 0 < err.mean() <= FP32_MEAN * rms and err.max() <= FP32_MAX * rms, "the twin is an fp16 network: inside the device's own bars"
    assert 0 < f["channel"] < 0.05 and 0.2 < f["ring"] < 5


@pytest.mark.parametrize("upto", [0, 1, 2, 7])
def test_face_twin_at_the_block_test_points(upto):
    sd = faces.random_state_dict(11)
    crops = fo.crop_input(_frames(2, 3, 120, 160), BOXES[:6])
    _twin_is_a_twin(f"iresnet block {upto}", fo.forward_blocks(sd, crops, upto, fp16=True), fo.forward_blocks(sd, crops, upto))


@pytest.mark.parametrize("name", list(CASES))
def test_speaker_twin_at_the_block_test_points(name):
    win, depths, valid, seed = CASES[name]
    net = so.resnet(speakers.random_state_dict(seed, depths))
    x16 = so.network_input(so.features(_audio(), _plan(valid), win))
    for upto in (0, depths[0]):
        want, _ = so.forward_blocks(net, x16, upto)
        twin, _ = so.forward_blocks(net, x16, upto, fp16=True)
        _twin_is_a_twin(f"speakers {name} block {upto}", twin, want)


def places_stem_pool(state, x, fp16):
    """oracle/places.py's network up to the max pool: NHWC float64"""
    net = op.ResNet18({"conv1": state["conv1"]}, fp16=fp16)
    with torch.no_grad():
        y = torch.nn.functional.max_pool2d(net.conv("conv1", net._h(x), 2, True), 3, 2, 1)
    return y.permute(0, 2, 3, 1).numpy().astype(np.float64)


def test_places_twin_at_the_stem_and_pool():
    x = op.preprocess(textured(11, 4, 270, 480))
    st = op.random_state(3)
    _twin_is_a_twin("places stem + pool", places_stem_pool(st, x, True), places_stem_pool(st, x, False))


def test_figures_see_one_wrong_channel_and_one_wrong_border_column():
    rng = np.random.default_rng(0)
    want = rng.standard_normal((2, 14, 14, 512))
    twin = want + 1e-3 * rng.standard_normal(want.shape)
    block_stats.check("clean", want + 1e-3 * rng.standard_normal(want.shape), twin, want)
    bad = twin.copy()
    bad[..., 77] += 0.01  # 1 % of one channel's RMS: 2e-5 of the whole tensor's mean error
    with pytest.raises(AssertionError, match="channel 77"):
        block_stats.check("one channel", bad, twin, want)
    bad = twin.copy()
    bad[:, :, 0] += 0.01
    with pytest.raises(AssertionError, match="border"):
        block_stats.check("one border column", bad, twin, want)
    dead = want.copy()
    dead[..., :40] *= 1e-4
    with pytest.raises(AssertionError, match="dead"):
        block_stats.check("dead channels", dead + 1e-3 * rng.standard_normal(dead.shape), dead + 1e-3 * rng.standard_normal(dead.shape), dead)
