"""GPU: the hand-written kernels around the conv family - k_stem7x7, k_maxpool3s2, k_places_head (csrc/resnet.hip), k_chan_ops,
k_face_fc, k_face_norm (csrc/faces.hip), k_spk_pool, k_spk_head (csrc/speakers.hip) - one kernel at a time, against the float64
restatements of tests/convnet_glue_oracle.py.  libeioku_hip_probe.so (csrc/probe/places_probe.hip, faces_probe.hip,
speakers_probe.hip) includes the three model sources unchanged and exports one entry point per kernel with the model's own grid;
the product never loads it.  Handles are created through the probe library, weights go through the product's own fold_state and
set_* calls.

The bars are convnet_glue_oracle's check_* functions, the same ones tests/test_convnet_glue_host.py runs on the emulation and on
sixteen wrong emulations.  Stores: every output buffer is larger than the result and pre-filled with a NaN bit pattern; what the
kernel does not own must still hold it."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import convnet_glue_oracle as o

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "eioku_amd" / "libeioku_hip_probe.so"
pytestmark = pytest.mark.gpu
EINVAL = -1


@pytest.fixture(scope="module")
def probe(gpu):
    from eioku_amd import _lib

    assert LIB.exists(), "build it: make -C eioku_amd/csrc (target all builds the probe library too)"
    lib = C.CDLL(str(LIB))
    for name, (res, args) in _lib.SIGNATURES.items():  # the probe carries its own eioku_resnet18_*, eioku_iresnet_*, eioku_spk_*
        if name.startswith(("eioku_resnet18_", "eioku_iresnet_", "eioku_spk_")):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    p, i, ll = C.c_void_p, C.c_int, C.c_longlong
    lib.eioku_probe_places_stem.argtypes = [p, p, i, p, p]
    lib.eioku_probe_places_maxpool.argtypes = [p, i, i, i, i, p, p]
    lib.eioku_probe_places_head.argtypes = [p, p, i, i, i, p, p, p, p]
    lib.eioku_probe_face_chan_ops.argtypes = [p, ll, i, p, p, p, p, p]
    lib.eioku_probe_face_head.argtypes = [p, p, i, p, p, p]
    lib.eioku_probe_spk_pool.argtypes = [p, p, i, i, p, p]
    lib.eioku_probe_spk_head.argtypes = [p, p, i, p, p]
    lib.eioku_last_error.restype = C.c_char_p
    assert lib.eioku_init(0) == 0, lib.eioku_last_error()  # the probe links its own core.o: its own state
    return lib


@pytest.fixture(scope="module")
def report():
    """name -> largest device error and the bar there; printed once the module is through (pytest -s)"""
    rows = {}
    yield rows
    for name in sorted(rows):
        print(f"\n[convnet glue] {name}: " + ", ".join(f"{k} {v:.3e}" for k, v in rows[name].items()), end="")
    print()


def _handle(probe, prefix, *args):
    from eioku_amd._handle import Handle

    return Handle(prefix, *args, lib=probe)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _sentinel(n, f16):
    return torch.full((n,), o.S16 if f16 else o.S32, dtype=torch.int16 if f16 else torch.int32, device="cuda")


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint16 if a.dtype == np.int16 else np.uint32)


def _err(probe):
    return (probe.eioku_last_error() or b"").decode()


# ---- k_stem7x7 --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stem_handle(probe):
    h = _handle(probe, "resnet18", 365)
    yield h
    h.close()


def _stem(probe, h, x):
    """-> [n][112][112][64] fp16; the buffer has one more image of sentinel"""
    n = x.shape[0]
    per = 112 * 112 * 64
    out = _sentinel((n + 1) * per, True)
    rc = probe.eioku_probe_places_stem(h.ptr, _ptr(_dev(x)), n, _ptr(out), None)
    assert rc == 0, _err(probe)
    b = _bits(out)
    assert (b[n * per:] == o.S16).all(), "k_stem7x7 stored past its last image"
    return b[:n * per].view(np.float16).reshape(n, 112, 112, 64)


@pytest.mark.parametrize("kind", o.STEM_KINDS)
def test_stem_matches_float64(probe, stem_handle, report, kind):
    """One-hot weights (every (channel, tap) of the 147 once: host packing, padded taps, zero border) in bits; random weights and
    the +-1000 ring under the fp16 bar; channel 3 inert; image i of N = 3 equals image i alone."""
    w, b = o.stem_weights(kind)
    assert probe.eioku_resnet18_set_conv(stem_handle.ptr, 0, w.ctypes.data, b.ctypes.data) == 0, _err(probe)
    x = o.stem_input(kind)
    got3 = _stem(probe, stem_handle, x)
    kw = {}
    if kind == "random":
        kw["junk"] = _stem(probe, stem_handle, o.stem_input(kind, True))
    if kind == "ring":
        z = x.copy()
        z[:, :3], z[:, -3:], z[:, :, :3], z[:, :, -3:] = 0, 0, 0, 0
        kw["zero_ring"] = _stem(probe, stem_handle, z)
    o.check_stem(kind, 3, got3, alone=_stem(probe, stem_handle, x[2:3]), report=report, **kw)
    o.check_stem(kind, 1, _stem(probe, stem_handle, x[:1]), report=report)


def test_stem_refuses_what_it_cannot_run(probe, stem_handle):
    buf = _sentinel(16, True)
    assert probe.eioku_probe_places_stem(stem_handle.ptr, None, 1, _ptr(buf), None) == EINVAL
    assert probe.eioku_probe_places_stem(stem_handle.ptr, _ptr(buf), 0, _ptr(buf), None) == EINVAL and "n = 0" in _err(probe)
    fresh = _handle(probe, "resnet18", 365)
    assert probe.eioku_probe_places_stem(fresh.ptr, _ptr(buf), 1, _ptr(buf), None) == EINVAL and "no weights" in _err(probe)
    fresh.close()
    assert (_bits(buf) == o.S16).all()


# ---- k_maxpool3s2 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", o.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_is_exact(probe, shape):
    """Negative inputs (the product never feeds any after its ReLU: only this tells a 0 initialiser from -65504), an all-negative
    map, +-0; H, W of 1, 2, odd, even; the product's 112 x 112 x 64."""
    n, h, w, c = shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = _sentinel(n * ho * wo * c + c, True)
    rc = probe.eioku_probe_places_maxpool(_ptr(_dev(o.pool_input(shape))), n, h, w, c, _ptr(out), None)
    assert rc == 0, _err(probe)
    b = _bits(out)
    assert (b[n * ho * wo * c:] == o.S16).all(), "k_maxpool3s2 stored past its output"
    o.check_pool(shape, b[:n * ho * wo * c].view(np.float16).reshape(n, ho, wo, c))


def test_maxpool_refuses_what_it_cannot_run(probe):
    buf = _sentinel(64, True)
    for shape in ((1, 2, 2, 4), (1, 2, 2, 12), (0, 2, 2, 8), (1, 0, 2, 8)):
        assert probe.eioku_probe_places_maxpool(_ptr(buf), *shape, _ptr(buf), None) == EINVAL and "bad shape" in _err(probe)
    assert probe.eioku_probe_places_maxpool(None, 1, 2, 2, 8, _ptr(buf), None) == EINVAL
    assert (_bits(buf) == o.S16).all()


def test_places_stem_and_pool_block_matches_torch_fp32(probe):
    """The block-level point Places365 lacked: k_stem7x7 then k_maxpool3s2 on the network test's frames and weights, against
    oracle/places.py in fp32 under the network's own bars, and per channel and on the border at most 2 x the oracle's fp16 twin
    (tests/block_stats.py)."""
    import block_stats
    from oracle import places as op
    from test_block_stats_host import places_stem_pool
    from test_places_gpu import FP32_MAX, FP32_MEAN, textured

    st = op.random_state(3)
    x = op.preprocess(textured(11, 4, 270, 480))
    x16 = np.zeros((4, 224, 224, 4), np.float16)
    x16[..., :3] = x.permute(0, 2, 3, 1).numpy().astype(np.float16)
    h = _handle(probe, "resnet18", 365)
    try:
        w, b = (np.ascontiguousarray(a, np.float32) for a in st["conv1"])
        assert probe.eioku_resnet18_set_conv(h.ptr, 0, w.ctypes.data, b.ctypes.data) == 0, _err(probe)
        a112 = _dev(_stem(probe, h, x16))
        out = torch.empty((4, 56, 56, 64), dtype=torch.float16, device="cuda")
        assert probe.eioku_probe_places_maxpool(_ptr(a112), 4, 112, 112, 64, _ptr(out), None) == 0, _err(probe)
    finally:
        h.close()
    got = out.cpu().numpy().astype(np.float64)
    want, twin = places_stem_pool(st, x, False), places_stem_pool(st, x, True)
    rms = float(np.sqrt((want ** 2).mean()))
    err = np.abs(got - want)
    print(f"\nplaces stem + pool: rms {rms:.3f} mean {err.mean() / rms:.2e} max {err.max() / rms:.2e}")
    assert rms > 0.1 and err.mean() <= FP32_MEAN * rms and err.max() <= FP32_MAX * rms
    block_stats.check("places stem + pool", got, twin, want)


# ---- k_places_head ----------------------------------------------------------------------------------------------------------
def _head(probe, h, x, nc, top_k):
    """-> (logits [n][nc], probs [n][top_k], idx [n][top_k]); each buffer has a sentinel tail"""
    n, hw = x.shape[:2]
    logits, probs, idx = _sentinel(n * nc + 8, False), _sentinel(n * top_k + 8, False), _sentinel(n * top_k + 8, False)
    rc = probe.eioku_probe_places_head(h.ptr, _ptr(_dev(x)), n, hw, top_k, _ptr(logits), _ptr(probs), _ptr(idx), None)
    assert rc == 0, _err(probe)
    lb, pb, ib = _bits(logits), _bits(probs), _bits(idx)
    assert (lb[n * nc:] == o.S32).all() and (pb[n * top_k:] == o.S32).all() and (ib[n * top_k:] == o.S32).all(), \
        f"nc {nc} top_k {top_k}: a probability or class slot >= top_k was written"
    return lb[:n * nc].view(np.float32).reshape(n, nc), pb[:n * top_k].view(np.float32).reshape(n, top_k), \
        ib[:n * top_k].view(np.int32).reshape(n, top_k)


@pytest.mark.parametrize("nc", o.HEAD_NC)
def test_places_head_matches_float64(probe, report, nc):
    """nc at 1, 2, around 256 (one thread's two sort slots), the product's 365 and 512 (no padding); exact ties across the
    256 boundary and across bitonic stages; a row whose other probabilities are exactly 0; top_k 1, 10, nc."""
    h = _handle(probe, "resnet18", nc)
    try:
        w, b = o.head_weights(nc)
        assert probe.eioku_resnet18_set_fc(h.ptr, w.ctypes.data, b.ctypes.data) == 0, _err(probe)
        for hw in o.HEAD_HW:
            for n in o.HEAD_N:
                x = o.head_input(nc, hw)[:n]
                full = _head(probe, h, x, nc, nc)
                for top_k in o.head_topk(nc):
                    o.check_head(nc, hw, n, top_k, *_head(probe, h, x, nc, top_k), full=full[1:], report=report)
        # refusals
        buf = _sentinel(4096, False)
        args = (_ptr(buf), _ptr(buf), _ptr(buf), None)
        assert probe.eioku_probe_places_head(h.ptr, _ptr(buf), 1, 1, nc + 1, *args) == EINVAL and "top_k" in _err(probe)
        assert probe.eioku_probe_places_head(h.ptr, _ptr(buf), 1, 1, 0, *args) == EINVAL
        assert probe.eioku_probe_places_head(h.ptr, _ptr(buf), 1, 0, 1, *args) == EINVAL
        assert probe.eioku_probe_places_head(h.ptr, _ptr(buf), 1, 1, 1, None, None, _ptr(buf), None) == EINVAL
        assert (_bits(buf) == o.S32).all()
    finally:
        h.close()


def test_places_head_pooled_mean_is_the_sequential_fp32_sum(probe):
    """nc 512 with fc = I and no bias: the logits are the pooled means, a sequential fp32 sum and one division - equal bits."""
    h = _handle(probe, "resnet18", 512)
    try:
        w, b = o.head_identity()
        assert probe.eioku_resnet18_set_fc(h.ptr, w.ctypes.data, b.ctypes.data) == 0, _err(probe)
        for hw in o.HEAD_HW:
            x = o.head_input(512, hw)
            logits = _head(probe, h, x, 512, 1)[0]
            want = o.head_pool_emulate(x)
            assert np.array_equal(logits, want), f"HW {hw}: {np.abs(logits - want).max()}"  # values: 0 + -0 is +0 in the fc
            assert np.abs(logits - x.astype(np.float64).mean(axis=1)).max() <= 4 * np.abs(want - x.astype(np.float64).mean(axis=1)).max()
    finally:
        h.close()
    fat = C.c_void_p()
    assert probe.eioku_resnet18_create(513, C.byref(fat)) == EINVAL, "more classes than the sort's 512 slots"


# ---- k_chan_ops -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", o.CHAN_MODES)
@pytest.mark.parametrize("c", o.CHAN_C)
@pytest.mark.parametrize("pixels", o.CHAN_PIXELS)
def test_chan_ops_is_the_contract_in_bits(probe, pixels, c, mode):
    """fp16(fp16(prelu in fp32) * scale + shift), two fp32 operations and no FMA, in the four modes run_iresnet uses; every
    channel with its own slope (negative and > 1 too), scale and shift; +-0, +-65504 and inputs that tell the place of the
    first rounding."""
    x, slope, scale, shift = o.chan_case(pixels, c)
    d_slope, d_bn = _dev(slope), _dev(np.concatenate([scale, shift]))
    n = pixels * c
    buf_in, buf_act, buf_bn = _sentinel(n + c, True), _sentinel(n + c, True), _sentinel(n + c, True)
    buf_in[:n] = _dev(o.bits(x).reshape(-1).view(np.int16))
    sl = _ptr(d_slope) if mode != "bn_only" else None
    act = _ptr(buf_in) if mode.startswith("prelu") else None
    bn = _ptr(buf_bn) if mode in ("prelu_bn_aliased", "bn_only") else None
    rc = probe.eioku_probe_face_chan_ops(_ptr(buf_in), pixels, c, sl, act, _ptr(d_bn) if mode != "prelu_in_place" else None, bn, None)
    assert rc == 0, _err(probe)
    o.check_chan(pixels, c, mode, _bits(buf_in), _bits(buf_act), _bits(buf_bn))


def test_chan_ops_refuses_what_it_cannot_run(probe):
    buf = _sentinel(64, True)
    f = _dev(np.ones(32, np.float32))
    for c in (4, 12, 0):
        assert probe.eioku_probe_face_chan_ops(_ptr(buf), 1, c, _ptr(f), _ptr(buf), _ptr(f), _ptr(buf), None) == EINVAL and "c % 8" in _err(probe)
    assert probe.eioku_probe_face_chan_ops(None, 1, 8, _ptr(f), _ptr(buf), _ptr(f), _ptr(buf), None) == EINVAL
    assert probe.eioku_probe_face_chan_ops(_ptr(buf), 1, 8, None, None, None, _ptr(buf), None) == EINVAL
    assert probe.eioku_probe_face_chan_ops(_ptr(buf), 0, 8, _ptr(f), _ptr(buf), _ptr(f), _ptr(buf), None) == 0  # chan_ops: nothing to do
    assert (_bits(buf) == o.S16).all()


# ---- k_face_fc / k_face_norm ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def face_head(probe):
    """the r18 fixture's head through the product's own fold_state and eioku_iresnet_set_head; activations of the RMS the torch
    oracle's last block gives on two of the fixture's crops; the float64 partial sums and the emulation's, once, for m = 33"""
    import face_oracle as fo
    from eioku_amd import faces
    from test_faces_gpu import BOXES, _frames

    sd = faces.random_state_dict(11)
    w, b = faces.fold_state(sd)["head"]
    net = fo.iresnet(sd)
    crops = fo.crop_input(_frames(2, 3, 120, 160), BOXES[:2])
    with torch.no_grad():
        y = net.layer4(net.layer3(net.layer2(net.layer1(net.stem(torch.from_numpy(crops[..., :3].astype(np.float32)).permute(0, 3, 1, 2))))))
    rms = float(f"{float(y.pow(2).mean().sqrt()):.2g}")
    print(f"\n[convnet glue] face head: the torch oracle's last block has RMS {rms:g}")
    h = _handle(probe, "iresnet", (C.c_int * 4)(2, 2, 2, 2))
    assert probe.eioku_iresnet_set_head(h.ptr, w.ctypes.data, b.ctypes.data) == 0, _err(probe)
    x, w16 = o.face_input(rms), o.to_f16(w)
    yield {"h": h, "x": x, "w": w, "w16": w16, "b": b, "ref": o.face_partial_ref(x, w16), "emu": o.face_partial_emulate(x, w16), "emb33": {}}
    h.close()


def _face(probe, h, x):
    m = x.shape[0]
    part = _sentinel((o.FACE_SPLIT * m + o.FACE_TAIL_ROWS) * 512, False)
    emb = _sentinel((m + o.FACE_TAIL_ROWS) * 512, False)
    rc = probe.eioku_probe_face_head(h.ptr, _ptr(_dev(x)), m, _ptr(part), _ptr(emb), None)
    assert rc == 0, _err(probe)
    return _bits(part).reshape(-1, 512), _bits(emb).reshape(-1, 512)


@pytest.mark.parametrize("m", o.FACE_M)
def test_face_head_matches_float64(probe, face_head, report, m):
    """m around the 16-row MFMA group: partials per slice against float64 sums over that slice's own 1568 columns in torch's
    flatten order (the NCHW -> NHWC column permutation of fold_state is under test), the live-row mask, unit norms; face 0 of
    m = 33 equals face 0 alone."""
    f = face_head
    part, emb = _face(probe, f["h"], f["x"][:m])
    if 0 not in f["emb33"]:
        f["emb33"][0] = (emb if m == 33 else _face(probe, f["h"], f["x"])[1])[0].view(np.float32).copy()
    alone = f["emb33"][0] if m == 1 else None
    o.check_face_head(f["x"][:m], f["w16"], f["b"], part, emb, f["ref"][:, :m], f["emu"][:, :m], alone_of=alone, report=report)


def test_face_head_zero_row_returns_zero_not_nan(probe, face_head):
    f = face_head
    zb = np.zeros(512, np.float32)
    assert probe.eioku_iresnet_set_head(f["h"].ptr, f["w"].ctypes.data, zb.ctypes.data) == 0, _err(probe)
    try:
        z = np.zeros_like(f["x"][:2])
        z[1] = f["x"][1]
        part, emb = _face(probe, f["h"], z)
        ref = np.stack([0 * f["ref"][:, 0], f["ref"][:, 1]], axis=1)
        emu = np.stack([0 * f["emu"][:, 0], f["emu"][:, 1]], axis=1)
        o.check_face_head(z, f["w16"], zb, part, emb, ref, emu)
        assert (emb[0] == 0).all(), "a zero row with zero bias: 0 / 1e-12 = 0"
    finally:
        assert probe.eioku_iresnet_set_head(f["h"].ptr, f["w"].ctypes.data, f["b"].ctypes.data) == 0, _err(probe)


def test_face_head_refuses_what_it_cannot_run(probe, face_head):
    buf = _sentinel(64, False)
    h = face_head["h"]
    for m in (0, 257):
        assert probe.eioku_probe_face_head(h.ptr, _ptr(buf), m, _ptr(buf), _ptr(buf), None) == EINVAL and "outside [1, 256]" in _err(probe)
    assert probe.eioku_probe_face_head(h.ptr, _ptr(buf), 1, None, _ptr(buf), None) == EINVAL
    bare = _handle(probe, "iresnet", (C.c_int * 4)(2, 2, 2, 2))
    assert probe.eioku_probe_face_head(bare.ptr, _ptr(buf), 1, _ptr(buf), _ptr(buf), None) == EINVAL and "no weights" in _err(probe)
    bare.close()
    assert (_bits(buf) == o.S32).all()


# ---- k_spk_pool / k_spk_head ------------------------------------------------------------------------------------------------
def _spk_pool(probe, x, valid):
    stats = _sentinel((o.SPK_M + 1) * o.SPK_STAT, False)
    v = np.asarray(valid, np.int32)
    rc = probe.eioku_probe_spk_pool(_ptr(_dev(x)), v.ctypes.data, len(v), x.shape[2], _ptr(stats), None)
    assert rc == 0, _err(probe)
    return _bits(stats).reshape(-1, o.SPK_STAT)


@pytest.mark.parametrize("wf", [5, 25])
def test_speaker_pool_matches_float64(probe, report, wf):
    """T = ceil(valid / 8) in {2, 3, Wf} with valid % 8 in {0, 1, 7}; NaN in the columns >= T (not read: the same bits as with
    zeros there); a constant channel (std sqrt(1e-7)); a channel with mean >> std (two-pass variance)."""
    buf = _spk_pool(probe, o.spk_input(wf), o.SPK_VALID[wf])
    o.check_spk_pool(wf, buf, report=report)
    assert np.array_equal(buf, _spk_pool(probe, o.spk_input(wf, False), o.SPK_VALID[wf])), "the columns >= T were read"


def test_speaker_pool_refuses_a_window_without_statistics(probe):
    x, stats = _dev(o.spk_input(5, False)), _sentinel(o.SPK_STAT * 2, False)
    for valid, word in ((8, "window 0: 8 valid frames"), (0, "window 0: 0 valid"), (41, "window 0: 41 valid")):
        v = np.asarray([valid], np.int32)
        assert probe.eioku_probe_spk_pool(_ptr(x), v.ctypes.data, 1, 5, _ptr(stats), None) == EINVAL and word in _err(probe), _err(probe)
    v = np.asarray([9], np.int32)
    assert probe.eioku_probe_spk_pool(_ptr(x), v.ctypes.data, 65, 5, _ptr(stats), None) == EINVAL
    assert probe.eioku_probe_spk_pool(_ptr(x), None, 1, 5, _ptr(stats), None) == EINVAL
    assert (_bits(stats) == o.S32).all()


@pytest.mark.parametrize("m", [1, 5])
def test_speaker_head_matches_float64(probe, report, m):
    """seg_1 with the weights through the product's fold_state (torch_to_device_columns) and eioku_spk_set_head, against the
    checkpoint's own matrix on the statistics taken back to torch's column order."""
    from eioku_amd import speakers
    from eioku_amd._buffers import ptr

    sd = speakers.random_state_dict(5, speakers.DEPTHS["r18"])
    w_dev, b = speakers.fold_state(sd)["head"]
    window, mel = speakers.povey_window(), np.ascontiguousarray(speakers.kaldi_mel_banks())
    h = _handle(probe, "spk", (C.c_int * 4)(2, 2, 2, 2), 40, ptr(window), ptr(mel))
    try:
        out = _sentinel((m + 1) * 256, False)
        stats = _dev(o.spk_head_stats()[:m])
        assert probe.eioku_probe_spk_head(h.ptr, _ptr(stats), m, _ptr(out), None) == EINVAL and "no weights" in _err(probe)
        assert probe.eioku_spk_set_head(h.ptr, w_dev.ctypes.data, b.ctypes.data) == 0, _err(probe)
        assert probe.eioku_probe_spk_head(h.ptr, _ptr(stats), 65, _ptr(out), None) == EINVAL
        assert (_bits(out) == o.S32).all()
        assert probe.eioku_probe_spk_head(h.ptr, _ptr(stats), m, _ptr(out), None) == 0, _err(probe)
        o.check_spk_head(m, _bits(out).reshape(-1, 256), w_dev, np.asarray(sd["seg_1.weight"], np.float32), b,
                         speakers.device_to_torch_columns, report=report)
    finally:
        h.close()
