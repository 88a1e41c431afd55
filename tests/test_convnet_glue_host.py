"""Host side of the ConvNet glue parity net (tests/convnet_glue_oracle.py, tests/test_convnet_glue_gpu.py): no GPU.

1. The emulation of every kernel passes the checks of the GPU tests on every case of their tables: the inputs and the bars fit
   together, and the oracle's own assumptions hold (the spike's gap, the exact ties, the rounding-order inputs, torch.std of one
   column).
2. Every deliberately wrong emulation fails those checks on at least one case: the GPU tests can fail.
3. Every probe launches its kernel with the grid of the model's own launch line."""
import re
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

import convnet_glue_oracle as o

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "eioku_amd" / "csrc"


def _rejects(check, *args, **kw):
    try:
        check(*args, **kw)
    except AssertionError:
        return 1
    return 0


# ---- the cases, each as (check, emulated outputs under `mutant`) -----------------------------------------------------------
def _stem_runs(mutant):
    """N = 1 is enough on the host: image i of a launch is image i alone in the emulation by construction"""
    for kind in o.STEM_KINDS:
        w, b = o.stem_weights(kind)
        x = o.stem_input(kind)[:1]
        got = o.to_f16(o.stem_emulate32(x, w, b, mutant))
        kw = {}
        if kind == "random":
            kw["junk"] = o.to_f16(o.stem_emulate32(o.stem_input(kind, True)[:1], w, b, mutant))
        if kind == "ring":
            z = x.copy()
            z[:, :3], z[:, -3:], z[:, :, :3], z[:, :, -3:] = 0, 0, 0, 0
            kw["zero_ring"] = o.to_f16(o.stem_emulate32(z, w, b, mutant))
        yield o.check_stem, (kind, 1, got), kw


def _pool_runs(mutant):
    for shape in o.POOL_SHAPES:
        yield o.check_pool, (shape, o.pool_emulate(o.pool_input(shape), mutant)), {}


def _head_runs(mutant):
    for nc in o.HEAD_NC:
        w, b = o.head_weights(nc)
        for hw in o.HEAD_HW:
            for n in o.HEAD_N:
                x = o.head_input(nc, hw)[:n]
                full = o.head_emulate(x, w, b, nc, mutant)[1:]
                for top_k in o.head_topk(nc):
                    yield o.check_head, (nc, hw, n, top_k, *o.head_emulate(x, w, b, top_k, mutant)), {"full": full}


def _chan_runs(mutant):
    for pixels in o.CHAN_PIXELS:
        for c in o.CHAN_C:
            x, slope, scale, shift = o.chan_case(pixels, c)
            for mode in o.CHAN_MODES:
                with np.errstate(over="ignore", invalid="ignore"):
                    act, bn = o.chan_emulate(x, slope if mode.startswith("prelu") else None, scale, shift, mutant)
                tail = np.full(c, o.S16, np.uint16)
                buf_in = np.concatenate([o.bits(act if mode.startswith("prelu") else x).reshape(-1), tail])
                buf_bn = np.concatenate([o.bits(bn).reshape(-1), tail]) if mode in ("prelu_bn_aliased", "bn_only") else \
                    np.full(pixels * c + c, o.S16, np.uint16)
                yield o.check_chan, (pixels, c, mode, buf_in, np.full(pixels * c + c, o.S16, np.uint16), buf_bn), {}


FACE_RMS = 1.0  # the host's stand-in; the GPU test takes the RMS of the torch oracle's last block and prints it


@pytest.fixture(scope="module")
def face_problem():
    rng = np.random.default_rng(5)
    w16 = o.to_f16(rng.standard_normal((512, o.FACE_K)) / np.sqrt(o.FACE_K))
    bias = (0.01 * rng.standard_normal(512)).astype(np.float32)
    x = o.face_input(FACE_RMS)[:17]  # the host walks m in {1, 15, 16, 17}: 33 differs from 17 only in the third group
    return x, w16, bias, o.face_partial_ref(x, w16), o.face_partial_emulate(x, w16)


def _face_runs(mutant, problem):
    x, w16, bias, ref, emu = problem
    for m in (1, 15, 16, 17):
        part, emb = o.face_emulate_buffers(x[:m], w16, bias, emu[:, :m], mutant)
        yield o.check_face_head, (x[:m], w16, bias, part, emb, ref[:, :m], emu[:, :m]), {}
    z = np.zeros_like(x[:2])  # a zero row and a live one, zero bias
    z[1] = x[1]
    zb = np.zeros_like(bias)
    zr, ze = np.stack([0 * ref[:, 0], ref[:, 1]], axis=1), np.stack([0 * emu[:, 0], emu[:, 1]], axis=1)
    part, emb = o.face_emulate_buffers(z, w16, zb, ze, mutant)
    yield o.check_face_head, (z, w16, zb, part, emb, zr, ze), {}


def _spk_runs(mutant):
    for wf in (5, 25):
        buf = np.full((o.SPK_M + 1, o.SPK_STAT), o.S32, np.uint32)
        with np.errstate(invalid="ignore"):
            buf[:o.SPK_M] = o.bits(o.spk_pool_emulate(o.spk_input(wf), o.SPK_VALID[wf], mutant))
        yield o.check_spk_pool, (wf, buf), {}


RUNS = {"stem": (_stem_runs, o.STEM_MUTANTS), "pool": (_pool_runs, o.POOL_MUTANTS), "head": (_head_runs, o.HEAD_MUTANTS),
        "chan": (_chan_runs, o.CHAN_MUTANTS), "spk": (_spk_runs, o.SPK_MUTANTS)}


# ---- 1. the emulation inside the bars ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(RUNS))
def test_emulation_passes_every_check(family):
    n = 0
    for check, args, kw in RUNS[family][0](None):
        check(*args, **kw)
        n += 1
    print(f"{family}: {n} cases")


def test_face_head_emulation_passes_every_check(face_problem):
    for check, args, kw in _face_runs(None, face_problem):
        check(*args, **kw)


def test_face_head_fold_is_torch_flatten_order():
    """fold_state's head (bn2 -> flatten -> fc -> features in one matrix, columns in NHWC order) against the torch modules
    themselves in float64 on an NCHW tensor, and the oracle's own way back to torch's columns."""
    import face_oracle as fo
    from eioku_amd import faces

    sd = faces.random_state_dict(11)
    w, b = faces.fold_state(sd)["head"]
    net = fo.iresnet(sd).double()
    x = np.random.default_rng(3).standard_normal((2, 7, 7, 512))
    with torch.no_grad():
        want = net.features(net.fc(torch.flatten(net.bn2(torch.from_numpy(x).permute(0, 3, 1, 2)), 1))).numpy()
    got = x.reshape(2, -1) @ w.astype(np.float64).T + b
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    cols = np.arange(o.FACE_K, dtype=np.int64)[None]
    assert np.array_equal(o.torch_flatten_columns(faces.nchw_to_nhwc_columns(cols)), cols)
    assert not np.array_equal(faces.nchw_to_nhwc_columns(cols), cols)


def test_speaker_head_emulation_is_within_the_bar():
    """the column order: the device's (f * 256 + c) against torch's flatten (c * 10 + f), by index arithmetic of the test's own"""
    rng = np.random.default_rng(9)
    w_torch = (rng.standard_normal((256, o.SPK_STAT)) / np.sqrt(o.SPK_STAT)).astype(np.float32)
    b = (0.01 * rng.standard_normal(256)).astype(np.float32)

    def to_torch(a):  # [..., 2][10][256] -> [..., 2][256][10]
        return np.ascontiguousarray(a.reshape(*a.shape[:-1], 2, 10, 256).swapaxes(-1, -2).reshape(a.shape))

    def to_device(a):
        return np.ascontiguousarray(a.reshape(*a.shape[:-1], 2, 256, 10).swapaxes(-1, -2).reshape(a.shape))

    from eioku_amd import speakers

    assert np.array_equal(speakers.device_to_torch_columns(o.spk_head_stats()), to_torch(o.spk_head_stats()))
    assert np.array_equal(speakers.torch_to_device_columns(w_torch), to_device(w_torch))
    for m in (1, 5):
        buf = np.full((m + 1, 256), o.S32, np.uint32)
        buf[:m] = o.bits(o.spk_head_emulate(o.spk_head_stats()[:m], to_device(w_torch), b))
        o.check_spk_head(m, buf, to_device(w_torch), w_torch, b, to_torch)
        wrong = buf.copy()  # the weight left in torch's order: the check must notice
        wrong[:m] = o.bits(o.spk_head_emulate(o.spk_head_stats()[:m], w_torch, b))
        assert _rejects(o.check_spk_head, m, wrong, to_device(w_torch), w_torch, b, to_torch)


def test_the_oracles_own_assumptions():
    # the spike: > 150 above every other logit in float64, so that fp32 exp(v - max) is exactly 0 (it is below 2^-149 from -104)
    for nc in o.HEAD_NC:
        w, b = o.head_weights(nc)
        for hw in o.HEAD_HW:
            z = o.head_logits_ref(o.head_input(nc, hw), w, b)
            if nc > 2:
                assert z[2, o.HEAD_SPIKE] - np.delete(z[2], o.HEAD_SPIKE).max() > 200, (nc, hw)
                assert not any(o.HEAD_SPIKE in t for t in o.HEAD_TIES)
            assert np.abs(z[:2]).max() < 30, "the ordinary images stay far from fp32 exp's range"
    # one-hot stem: all 147 (channel, tap) pairs, each once
    ws = np.stack([o.stem_weights(f"onehot{s}")[0].reshape(64, 147) for s in range(3)])
    assert (ws.sum(axis=(0, 1)) == 1).all() and (ws.sum(axis=2) <= 1).all()
    assert (o.stem_input("random") < 0).any() and o.stem_input("ring")[0, 0, 0, 0] in (-1000, 1000)
    assert not o.stem_input("random")[..., 3].any() and o.stem_input("random", True)[..., 3].any()
    # max pool: an all-negative map, zeros of both signs
    for shape in o.POOL_SHAPES:
        x = o.pool_input(shape)
        assert (x[0, ..., :8] < 0).all() and (x < 0).any()
    x = o.pool_input(o.POOL_SHAPES[-1])
    assert ((x == 0) & np.signbit(x)).any() and ((x == 0) & ~np.signbit(x)).any()
    # k_chan_ops: every channel's first pixel separates the two places of the first rounding; the specials are there
    for pixels in o.CHAN_PIXELS:
        for c in o.CHAN_C:
            x, slope, scale, shift = o.chan_case(pixels, c)
            with np.errstate(over="ignore", invalid="ignore"):
                a, m = o.chan_emulate(x[:1], slope, scale, shift)[1], o.chan_emulate(x[:1], slope, scale, shift, "chan_bn_before_rounding")[1]
                ref = o.chan_ref(x, slope, scale, shift)[1]
                bn = o.chan_emulate(x, slope, scale, shift)[1].astype(np.float64)
            assert (o.bits(a) != o.bits(m)).mean() >= 0.75, (pixels, c)  # not all: a slope whose product is exact in fp16 has none
            assert len(set(slope.tolist())) == c and (slope < 0).any() and (slope > 1).any()
            # float64 rounded at the contract's two places: the same bits, but for the rare double rounding through fp32
            with np.errstate(over="ignore", invalid="ignore"):
                act64 = o.chan_ref(x, slope, scale, shift)[0].astype(np.float16)
                bn64 = (act64.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)).astype(np.float16)
            assert ref.shape == bn.shape and (o.bits(bn64) == o.bits(o.chan_emulate(x, slope, scale, shift)[1])).mean() > 0.99
            if pixels > 1:
                assert {0x0000, 0x8000, 0x7BFF, 0xFBFF} <= set(o.bits(x[1:3]).reshape(-1).tolist())
    # speakers: T and valid % 8 as the issue lists them; the offset channel has mean >> std
    for wf, valid in o.SPK_VALID.items():
        assert {(v + 7) // 8 for v in valid} == {2, 3, wf} and {v % 8 for v in valid} == {0, 1, 7} and min(valid) >= 9
        ref = o.spk_pool_ref(o.spk_input(wf), valid).reshape(o.SPK_M, 2, 10, 256)
        assert (ref[:, 0, :, o.SPK_OFFSET] > 200 * ref[:, 1, :, o.SPK_OFFSET]).all()
        assert np.isnan(o.spk_input(wf)[0, 0, 2:].astype(np.float32)).all()


def test_a_window_of_one_column_has_no_standard_deviation():
    """k_spk_pool pools ceil(valid / 8) columns.  Under 9 frames that is one column, and the unbiased deviation of one value
    is 0 / 0: torch agrees that there is nothing to return.  eioku_spk_embed and eioku_spk_forward refuse such a window
    (tests/test_speakers_gpu.py test_bad_windows_are_refused); this pins why."""
    for valid in range(1, 9):
        assert (valid + 7) // 8 == 1
    assert (9 + 7) // 8 == 2
    x = torch.tensor([[0.5], [1.25]], dtype=torch.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # torch says so itself: "degrees of freedom is <= 0"
        assert torch.isnan(torch.std(x, dim=1, unbiased=True)).all()
        assert torch.isnan(torch.sqrt(x.var(dim=-1) + 1e-7)).all()  # speaker_oracle.pooled's own expression
    with np.errstate(invalid="ignore", divide="ignore"):
        emu = o.spk_pool_emulate(np.ones((1, 10, 5, 256), np.float16), [8])
    assert np.isnan(emu[:, o.SPK_STAT // 2:]).all() and (emu[:, :o.SPK_STAT // 2] == 1).all(), "the kernel's arithmetic gives NaN too"
    src = (CSRC / "speakers.hip").read_text()
    for fn in ("eioku_spk_embed", "eioku_spk_forward"):
        body = src[src.index(f"int {fn}("):]
        body = body[:body.index("\n}\n")]
        assert re.search(r">= 9", body), f"{fn} must refuse a window of fewer than 9 frames"
    body = src[src.index("int eioku_spk_features("):]
    assert ">= 9" not in body[:body.index("\n}\n")], "eioku_spk_features still accepts valid >= 1"


# ---- 2. the mutants outside the bars ----------------------------------------------------------------------------------------
def test_every_mutant_is_rejected_by_at_least_one_case(face_problem):
    counts = {}
    for family, (runs, mutants) in RUNS.items():
        for m in mutants:
            counts[m] = sum(_rejects(check, *args, **kw) for check, args, kw in runs(m))
    for m in o.FACE_MUTANTS:
        counts[m] = sum(_rejects(check, *args, **kw) for check, args, kw in _face_runs(m, face_problem))
    for m, n in counts.items():
        print(f"mutant {m}: rejected by {n} cases")
    assert len(counts) == 16
    survivors = [m for m, n in counts.items() if n == 0]
    assert not survivors, f"no case rejects {survivors}: extend the case tables"


# ---- 3. the launch lines ----------------------------------------------------------------------------------------------------
def _launches(path):
    """{kernel: (grid, block)} of every hipLaunchKernelGGL in a source, as written"""
    text = re.sub(r"//[^\n]*", "", path.read_text())
    out = {}
    for m in re.finditer(r"hipLaunchKernelGGL\((\w+),\s*", text):
        args, depth, start = [], 0, m.end()
        for i in range(m.end(), len(text)):
            ch = text[i]
            depth += ch == "("
            depth -= ch == ")"
            if (ch == "," and depth == 0) or depth < 0:
                args.append(" ".join(text[start:i].split()))
                start = i + 1
                if len(args) == 2 or depth < 0:
                    break
        out.setdefault(m.group(1), set()).add(tuple(args))
    return out


PROBED = {"places_probe.hip": ("resnet.hip", ["k_stem7x7", "k_maxpool3s2", "k_places_head"]),
          "faces_probe.hip": ("faces.hip", ["k_face_fc", "k_face_norm"]),
          "speakers_probe.hip": ("speakers.hip", ["k_spk_pool", "k_spk_head"])}


@pytest.mark.parametrize("probe", list(PROBED))
def test_probe_launch_lines_are_the_models(probe):
    model, kernels = PROBED[probe]
    mine, theirs = _launches(CSRC / "probe" / probe), _launches(CSRC / model)
    assert sorted(mine) == sorted(kernels), f"{probe} launches {sorted(mine)}"
    for k in kernels:
        assert len(theirs[k]) == 1 and mine[k] == theirs[k], f"{k}: probe {mine[k]}, {model} {theirs[k]}"
    text = (CSRC / "probe" / probe).read_text()
    assert f'#include "../{model}"' in text


def test_probe_names_behind_the_launch_lines_mean_the_same():
    """the grids are compared as text, so the names in them must mean the same on both sides"""
    places, resnet = (CSRC / "probe" / "places_probe.hip").read_text(), (CSRC / "resnet.hip").read_text()
    assert "const int N = n;" in places
    mine = re.search(r"const long long work = ([^;]*);", places).group(1)
    theirs = re.search(r"const long long work = ([^;]*);", resnet[resnet.index("int run_network("):]).group(1)

    def value(expr, **names):
        return eval(expr.replace("(long long)", "").replace("/", "//"), {}, names)

    for n in (1, 3, 64):
        assert value(mine, N=n, h=112, w=112, c=64) == value(theirs, N=n)
    # faces: k_chan_ops goes through the model's own launch helper
    faces = (CSRC / "probe" / "faces_probe.hip").read_text()
    assert "return chan_ops((const __half*)in, pixels, c, slope, (__half*)out_act, scale_shift, (__half*)out_bn, stream);" in faces
    assert "k_chan_ops" in _launches(CSRC / "faces.hip") and "k_chan_ops" not in _launches(CSRC / "probe" / "faces_probe.hip")
    # speakers: run_pool_head passes win / 8 where the probe takes wf
    assert "s->buf[x].p, d_valid, s->win / 8, s->stats.p" in (CSRC / "speakers.hip").read_text()


def test_model_sources_do_not_know_the_probes():
    for f in ("resnet.hip", "faces.hip", "speakers.hip"):
        assert "probe" not in (CSRC / f).read_text().lower(), f
    header = (ROOT / "include" / "eioku_hip.h").read_text()
    for name in re.findall(r"int (eioku_probe_\w+)\(", "".join((CSRC / "probe" / p).read_text() for p in PROBED)):
        assert name not in header
    assert len(re.findall(r"int (eioku_probe_\w+)\(", "".join((CSRC / "probe" / p).read_text() for p in PROBED))) == 7
