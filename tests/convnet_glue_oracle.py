"""CPU restatements of the hand-written kernels around the conv family in csrc/resnet.hip (k_stem7x7, k_maxpool3s2,
k_places_head), csrc/faces.hip (k_chan_ops, k_face_fc, k_face_norm) and csrc/speakers.hip (k_spk_pool, k_spk_head), for
tests/test_convnet_glue_host.py and tests/test_convnet_glue_gpu.py.

Each operation comes twice, on the exact fp16 / fp32 inputs the device gets:
  * the reference: plain float64 (numpy / torch-CPU), no rounding anywhere;
  * the emulation: the device's arithmetic - fp16 storage, fp32 sums in the kernel's order where the source shows that order
    (the pooled mean, the fc's 8 terms per lane and its xor butterfly, the slice sum and the norm of k_face_norm, k_spk_pool,
    k_spk_head), one k after the other where it does not (the two MFMA kernels).  Its `mutant` argument switches on one
    deliberate error at a time.

The `check_*` functions hold what a kernel returned against the bars.  The GPU test gives them the device's buffers, the host
test the emulation's (which must pass) and each mutant's (which must not): one set of bars, stated once.  They raise
AssertionError with the case in the message.

Bars (the project's own: no new number)
  bits           stages that are one rounding of exact arithmetic (max pool, k_chan_ops, the one-hot stem), and every stage whose
                 summation order the emulation reproduces
  fp32 outputs   max |got - ref64| <= 4 x the emulation's largest error on the same case (K22's rule)
  fp16 outputs   per element, half an fp16 ulp of ref64 more
  softmax        against a float64 softmax of the device's own logits, rtol 2e-6, atol 1e-9 (test_places_gpu.py)
  order          exact given the device's own probabilities: (probability desc, class asc)

Nothing here imports the package's library or needs a GPU."""
from __future__ import annotations

import functools

import numpy as np
import torch

from transformer_core_oracle import half_ulp16, to_f16

S16, S32 = 0x7DDD, 0x7FC0DEAD  # fp16 / fp32 NaN patterns no kernel produces: the pre-fill of every output buffer
F32 = np.float32


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def within_bar(got, ref, bar32, f16):
    """fp32 outputs: max error <= bar32.  fp16 outputs: per element, half an fp16 ulp of the reference more.
    -> (ok, largest error, the bar at that element)"""
    err = np.abs(got.astype(np.float64) - ref)
    bar = bar32 + (half_ulp16(ref) if f16 else 0.0) + np.zeros_like(err)
    if not np.isfinite(err).all():
        return False, float("nan"), float(bar.max())
    i = np.unravel_index(np.argmax(err - bar), err.shape)
    return bool((err <= bar).all()), float(err[i]), float(bar[i])


def bar32_of(emu32, ref):
    return 4 * float(np.abs(emu32.astype(np.float64) - ref).max())


def _note(report, name, **figures):
    if report is not None:
        r = report.setdefault(name, {})
        for k, v in figures.items():
            r[k] = max(r.get(k, 0.0), float(v))


def wave_tree(v):
    """wave_reduce_add as lane 0 sees it (__shfl_down by 32, 16 ... 1): v [..., 64] fp32 -> [...]"""
    v = v.astype(F32)
    for off in (32, 16, 8, 4, 2, 1):
        v = v[..., :off] + v[..., off:2 * off]
    return v[..., 0]


def block_sum_256(v):
    """block_sum_256f / k_face_norm's reduction: four wave trees, then (r0 + r1) + (r2 + r3).  v [..., 256] fp32"""
    r = wave_tree(v.reshape(*v.shape[:-1], 4, 64))
    return (r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])


# ==== k_stem7x7 ==============================================================================================================
STEM_N = (1, 3)
STEM_MUTANTS = ["stem_border_clamped", "stem_taps_transposed", "stem_channel3_weighted"]
STEM_KINDS = ["onehot0", "onehot1", "onehot2", "ring", "random"]


def stem_weights(kind):
    """fp32 [64][3][7][7] and bias [64].  onehot<s>: output channel c carries a single 1.0 at flat (channel, tap) index 64 s + c
    (147 in all: channels 19 .. 63 of set 2 carry none), bias 0.25 c."""
    if kind.startswith("onehot"):
        s = int(kind[-1])
        w = np.zeros((64, 147), F32)
        for c in range(64):
            if 64 * s + c < 147:
                w[c, 64 * s + c] = 1.0
        return w.reshape(64, 3, 7, 7), (0.25 * np.arange(64)).astype(F32)
    rng = np.random.default_rng(41)
    return (1.4 * rng.standard_normal((64, 3, 7, 7)) / np.sqrt(147)).astype(F32), (0.3 * rng.standard_normal(64)).astype(F32)


@functools.lru_cache(maxsize=None)
def stem_input(kind, junk=False):
    """[3][224][224][4] fp16, channel 3 zero (or finite junk).  ring: the outer three rows and columns hold +-1000."""
    rng = np.random.default_rng(43)
    x = rng.standard_normal((3, 224, 224, 4)).astype(np.float16)
    x[0, :4, :4, :3] = [[-2.5, 1.5, 0.75]]  # a corner that is certainly not zero
    if kind == "ring":
        ring = np.ones((224, 224), bool)
        ring[3:-3, 3:-3] = False
        x[:, ring] = np.where(rng.random((3, int(ring.sum()), 4)) < 0.5, -1000, 1000).astype(np.float16)
    x[..., 3] = (100 * rng.standard_normal((3, 224, 224))).astype(np.float16) if junk else 0
    x.setflags(write=False)
    return x


def stem_ref(x, w, b):
    """float64 conv 7x7 / s2 / p3 of the fp16-rounded weights + bias + ReLU: [n][112][112][64]"""
    xt = torch.from_numpy(x[..., :3].astype(np.float64)).permute(0, 3, 1, 2)
    wt = torch.from_numpy(to_f16(w).astype(np.float64))
    y = torch.nn.functional.conv2d(xt, wt, torch.from_numpy(b.astype(np.float64)), stride=2, padding=3)
    return torch.relu(y).permute(0, 2, 3, 1).contiguous().numpy()


def stem_emulate32(x, w, b, mutant=None):
    """fp32: the products (exact) added one (tap, channel) after the other, + bias, ReLU; before the rounding to fp16"""
    n = x.shape[0]
    w16 = to_f16(w).astype(F32)
    if mutant == "stem_taps_transposed":
        w16 = np.ascontiguousarray(w16.transpose(0, 1, 3, 2))
    xp = np.pad(x.astype(F32), ((0, 0), (3, 3), (3, 3), (0, 0)), mode="edge" if mutant == "stem_border_clamped" else "constant")
    acc = np.zeros((n, 112, 112, 64), F32)
    for ty in range(7):
        for tx in range(7):
            for ch in range(4 if mutant == "stem_channel3_weighted" else 3):
                wv = w16[:, ch, ty, tx] if ch < 3 else np.ones(64, F32)
                if wv.any():
                    acc += xp[:, ty:ty + 223:2, tx:tx + 223:2, ch, None] * wv
    return np.maximum(acc + b.astype(F32), F32(0))


@functools.lru_cache(maxsize=None)
def stem_expect(kind):
    """-> (ref64 [3][112][112][64], bar32, emulated fp16 output) on stem_input(kind)"""
    w, b = stem_weights(kind)
    x = stem_input(kind)
    ref, e32 = stem_ref(x, w, b), stem_emulate32(x, w, b)
    return ref, bar32_of(e32, ref), to_f16(e32)


def check_stem(kind, n, got, alone=None, junk=None, zero_ring=None, report=None):
    """got [n][112][112][64] fp16 of images 0 .. n - 1 of stem_input(kind).  alone: image n - 1 in a launch of its own; junk: the
    same launch with finite junk in input channel 3; zero_ring (kind ring): the launch with the ring zeroed instead."""
    case = f"k_stem7x7 {kind} N {n}"
    ref, bar32, emu = stem_expect(kind)
    if kind.startswith("onehot"):  # one exact product + the bias: one fp32 add and one rounding to fp16, in any order of taps
        bad = np.argwhere(bits(got) != bits(emu[:n]))
        assert bad.size == 0, f"{case}: {len(bad)} outputs differ in bits, first (n, y, x, c) {bad[0].tolist()}"
    ok, err, bar = within_bar(got, ref[:n], bar32, True)
    _note(report, "k_stem7x7 " + ("one-hot" if kind.startswith("onehot") else kind), err=err, bar=bar)
    assert ok, f"{case}: error {err:.3e} > bar {bar:.3e} (4 x fp32 emulation {bar32:.3e})"
    if alone is not None:
        assert same_bits(alone[0], got[n - 1]), f"{case}: image {n - 1} differs from the same image alone"
    if junk is not None:
        assert same_bits(junk, got), f"{case}: input channel 3 changed the output"
    if zero_ring is not None:  # output rows and columns 3 .. 108 read no ring pixel
        assert same_bits(zero_ring[:, 3:109, 3:109], got[:, 3:109, 3:109]), f"{case}: the ring leaked into the interior"


# ==== k_maxpool3s2 ===========================================================================================================
POOL_SHAPES = [(1, 1, 1, 8), (2, 2, 3, 8), (1, 5, 4, 16), (2, 7, 7, 64), (1, 112, 112, 64)]
POOL_MUTANTS = ["pool_init_zero", "pool_window_at_2o"]


@functools.lru_cache(maxsize=None)
def pool_input(shape):
    """random fp16 with negative values; image 0's channel group 0 all negative; +0 / -0 sprinkled (and a 2 x 2 patch of each)"""
    rng = np.random.default_rng(7 + sum(shape))
    x = (3 * rng.standard_normal(shape)).astype(np.float16)
    z = rng.random(shape)
    x[z < 0.05] = np.float16(0.0)
    x[z > 0.95] = -np.float16(0.0)
    x[0, ..., :8] = -np.abs(x[0, ..., :8]) - np.float16(0.5)
    if shape[-1] > 8:
        x[-1, :, :, 8] = np.where(rng.random(shape[1:3]) < 0.5, np.float16(0.0), -np.float16(0.0))  # a map of zeros of both signs
    x.setflags(write=False)
    return x


def pool_emulate(x, mutant=None):
    """the kernel's own loop: best = -65504, then the in-bounds taps in (dy, dx) order with a strict > (so the first zero of a run
    of +-0 stays).  Max is exact: bits."""
    n, h, w, c = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    best = np.full((n, ho, wo, c), 0.0 if mutant == "pool_init_zero" else -65504.0, np.float16)
    oy, ox = np.arange(ho)[:, None], np.arange(wo)[None, :]
    first = 0 if mutant == "pool_window_at_2o" else -1
    for dy in range(3):
        for dx in range(3):
            y, xx = 2 * oy + first + dy, 2 * ox + first + dx
            ok = ((y >= 0) & (y < h) & (xx >= 0) & (xx < w))[None, :, :, None]
            v = x[:, np.clip(y, 0, h - 1), np.clip(xx, 0, w - 1)]
            best = np.where(ok & (v > best), v, best)
    return best


def pool_ref(x):
    """float64 max_pool2d(3, 2, 1): torch pads with -inf"""
    t = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)
    return torch.nn.functional.max_pool2d(t, 3, 2, 1).permute(0, 2, 3, 1).numpy()


def check_pool(shape, got):
    case = f"k_maxpool3s2 {shape}"
    x = pool_input(shape)
    assert got.shape == pool_ref(x).shape and np.array_equal(got.astype(np.float64), pool_ref(x)), f"{case}: differs from max_pool2d"
    assert same_bits(got, pool_emulate(x)), f"{case}: differs in bits (the sign of a zero)"


# ==== k_places_head ==========================================================================================================
HEAD_NC = [1, 2, 255, 256, 257, 365, 512]
HEAD_HW = [1, 49]
HEAD_N = [1, 3]
HEAD_TIES = [(0, 1), (255, 256), (3, 364), (100, 511)]  # across the 256 boundary (one thread's two slots) and bitonic stages
HEAD_MUTANTS = ["head_tie_descending", "head_padding_first", "head_softmax_no_max"]
HEAD_SPIKE = 2  # the class of image 2 that lies 200 above the rest (nc > 2)


def head_topk(nc):
    return sorted({1, nc} | ({10} if nc >= 10 else set()))


@functools.lru_cache(maxsize=None)
def head_weights(nc):
    """fc fp32 [nc][512] (already fp16 values) and bias [nc]; each pair of HEAD_TIES below nc shares one row and one bias.
    nc 512 'identity' is head_identity()."""
    rng = np.random.default_rng(500 + nc)
    w = to_f16(4.0 * rng.standard_normal((nc, 512)) / np.sqrt(512)).astype(F32)
    b = (0.1 * rng.standard_normal(nc)).astype(F32)
    for i, j in HEAD_TIES:
        if j < nc:
            w[j], b[j] = w[i], b[i]
    return w, b


@functools.lru_cache(maxsize=None)
def head_input(nc, hw):
    """[3][hw][512] fp16.  Image 2 (nc > 2) is 24 x fc row HEAD_SPIKE on every pixel: that logit is > 200 above the others."""
    rng = np.random.default_rng(600 + nc + hw)
    x = rng.standard_normal((3, hw, 512)).astype(np.float16)
    if nc > 2:
        x[2] = to_f16(24 * head_weights(nc)[0][HEAD_SPIKE])
    x.setflags(write=False)
    return x


def head_logits_ref(x, w, b):
    return x.astype(np.float64).mean(axis=1) @ w.astype(np.float64).T + b.astype(np.float64)


def head_pool_emulate(x):
    """the sequential fp32 sum over the pixels, one division: the kernel's order, so the kernel's bits"""
    s = np.zeros((x.shape[0], 512), F32)
    for p in range(x.shape[1]):
        s = s + x[:, p].astype(F32)
    return s / F32(x.shape[1])


def head_logits_emulate(x, w, b):
    """lane l: channels 8 l .. 8 l + 7 in order; the xor butterfly 32 .. 1 (every lane adds its partner: lane 0's value); + bias.
    The kernel's order: the kernel's bits."""
    pool = head_pool_emulate(x).reshape(-1, 1, 64, 8)
    wl = w.astype(F32).reshape(1, -1, 64, 8)
    s = np.zeros((x.shape[0], w.shape[0], 64), F32)
    for t in range(8):
        s = s + pool[..., t] * wl[..., t]
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lane ^ o]
    return s[..., 0] + b.astype(F32)


def head_emulate(x, w, b, top_k, mutant=None):
    """-> (logits [n][nc] fp32, probs [n][top_k] fp32, classes [n][top_k] int32).  exp and the sum's order are not the device's
    (the softmax bar is relative to a float64 softmax); the sort is by key, as any correct sort."""
    nc = w.shape[0]
    logits = head_logits_emulate(x, w, b)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(logits if mutant == "head_softmax_no_max" else logits - logits.max(axis=1, keepdims=True), dtype=F32)
        p = (e / e.sum(axis=1, keepdims=True, dtype=F32)).astype(F32)
    val = np.full((x.shape[0], 512), 2.0 if mutant == "head_padding_first" else -1.0, F32)
    val[:, :nc] = p
    probs, idx = np.empty((x.shape[0], top_k), F32), np.empty((x.shape[0], top_k), np.int32)
    for n in range(x.shape[0]):
        tie = -1 if mutant == "head_tie_descending" else 1
        order = sorted(range(512), key=lambda j: (-val[n, j] if val[n, j] == val[n, j] else 3.0, tie * j))
        idx[n], probs[n] = order[:top_k], val[n, order[:top_k]]
    return logits, probs, idx


def check_head(nc, hw, n, top_k, logits, probs, idx, full=None, report=None):
    """logits [n][nc], probs / idx [n][top_k] as returned for images 0 .. n - 1.  full: (probs, idx) of the top_k = nc launch."""
    case = f"k_places_head nc {nc} HW {hw} N {n} top_k {top_k}"
    w, b = head_weights(nc)
    x = head_input(nc, hw)[:n]
    ref, emu = head_logits_ref(x, w, b), head_logits_emulate(x, w, b)
    ok, err, bar = within_bar(logits, ref, bar32_of(emu, ref), False)
    _note(report, "k_places_head logits", err=err, bar=bar)
    assert ok, f"{case}: logits error {err:.3e} > bar {bar:.3e}"
    assert same_bits(logits, emu), f"{case}: logits differ in bits from the kernel's own order of sums"
    for i, j in HEAD_TIES:
        if j < nc:
            assert same_bits(logits[:, i], logits[:, j]), f"{case}: classes {i} and {j} share a row and do not tie"
    z = logits.astype(np.float64)
    soft = np.exp(z - z.max(axis=1, keepdims=True))
    soft /= soft.sum(axis=1, keepdims=True)
    assert idx.min() >= 0 and idx.max() < nc, f"{case}: class outside [0, {nc}) (padding sorted ahead of a class?)"
    want = np.take_along_axis(soft, idx.astype(np.int64), axis=1)
    assert np.isfinite(probs).all() and np.allclose(probs, want, rtol=2e-6, atol=1e-9), \
        f"{case}: probabilities differ from the float64 softmax of the device's logits by {np.abs(probs - want).max():.3e}"
    _note(report, "k_places_head softmax", err=np.abs(probs - want).max(), bar=1e-9 + 2e-6 * want.max())
    # the order, given the device's own probabilities: (probability desc, class asc), every class at most once
    for r in range(n):
        keys = [(-float(p), int(c)) for p, c in zip(probs[r], idx[r])]
        assert keys == sorted(keys) and len(set(idx[r].tolist())) == top_k, f"{case} image {r}: not in (probability desc, class asc) order"
    if top_k == nc:
        assert (np.sort(idx, axis=1) == np.arange(nc)).all(), f"{case}: the classes are no permutation"
        if nc > 2 and n == 3:  # the spike: every other probability is exactly 0, and the zeros come in class order
            assert idx[2, 0] == HEAD_SPIKE and probs[2, 0] == 1.0 and (probs[2, 1:] == 0).all(), f"{case}: the spike's row"
            assert idx[2, 1:].tolist() == [c for c in range(nc) if c != HEAD_SPIKE], f"{case}: the zeros are not in class order"
    if full is not None:
        assert same_bits(probs, np.ascontiguousarray(full[0][:, :top_k])) and np.array_equal(idx, full[1][:, :top_k]), \
            f"{case}: not the first {top_k} of the full order"


def head_identity():
    """nc 512, fc = I, bias 0: the logits are the pooled means themselves"""
    return np.eye(512, dtype=F32), np.zeros(512, F32)


# ==== k_chan_ops =============================================================================================================
CHAN_PIXELS = [1, 35, 257]
CHAN_C = [8, 64, 512]
CHAN_MODES = ["prelu_bn_aliased", "prelu_in_place", "bn_only", "no_output"]
CHAN_MUTANTS = ["chan_slope_mod8", "chan_bn_before_rounding"]


@functools.lru_cache(maxsize=None)
def chan_case(pixels, c):
    """-> (x [pixels][c] fp16, slope [c], scale [c], shift [c]).  Every channel has its own parameters (slopes from -0.5 to
    1.6); the first pixel rows carry +-0, +-65504 and negative values picked so that rounding the PReLU to fp16 before the
    BatchNorm changes the BatchNorm's fp16 result."""
    rng = np.random.default_rng(900 + pixels + c)
    slope = np.linspace(-0.5, 1.6, c).astype(F32)[rng.permutation(c)]
    scale = (rng.uniform(0.5, 1.5, c) * np.where(rng.random(c) < 0.2, -1, 1)).astype(F32)
    shift = rng.standard_normal(c).astype(F32)
    x = (4 * rng.standard_normal((pixels, c))).astype(np.float16)
    # per channel: a negative input whose result depends on the place of the first rounding
    cand = -np.abs(8 * rng.standard_normal((256, c))).astype(np.float16)
    with np.errstate(over="ignore"):
        a = chan_emulate(cand, slope, scale, shift)[1]
        m = chan_emulate(cand, slope, scale, shift, "chan_bn_before_rounding")[1]
    pick = np.argmax(bits(a) != bits(m), axis=0)
    x[0] = cand[pick, np.arange(c)]
    special = np.array([0.0, -0.0, 65504.0, -65504.0], np.float16)
    flat = x.reshape(-1)
    at = np.arange(c, min(flat.size, 3 * c)) if pixels > 1 else np.arange(0)  # rows 1, 2: the specials on every channel
    flat[at] = special[(at + at // c) % 4]
    x.setflags(write=False)
    return x, slope, scale, shift


def chan_emulate(x, slope, scale, shift, mutant=None):
    """the contract: act = fp16(x > 0 ? x : x * slope) with the product in fp32; bn = fp16(fp32(act * scale) + shift): two fp32
    operations, no FMA.  slope None: act = x.  -> (act, bn) fp16"""
    c = x.shape[-1]
    v = x.astype(F32)
    act16 = x
    with np.errstate(over="ignore"):  # -65504 x a slope above 1 is -inf in fp16, on the device as here
        if slope is not None:
            s = slope[np.arange(c) % 8] if mutant == "chan_slope_mod8" else slope
            v = np.where(v > 0, v, v * s.astype(F32)).astype(F32)
            act16 = v.astype(np.float16)
        src = v if mutant == "chan_bn_before_rounding" else act16.astype(F32)
        bn = ((src * scale.astype(F32)).astype(F32) + shift.astype(F32)).astype(np.float16)
    return act16, bn


def chan_ref(x, slope, scale, shift):
    """float64, no rounding: (act, bn)"""
    v = x.astype(np.float64)
    act = np.where(v > 0, v, v * slope.astype(np.float64)) if slope is not None else v
    return act, act * scale.astype(np.float64) + shift.astype(np.float64)


def check_chan(pixels, c, mode, in_after, act_buf, bn_buf):
    """The three buffers after the call, as uint16 bits with one sentinel row after the data: the input buffer (it is out_act in
    the aliased modes), a separate out_act buffer (never given to the kernel: must stay sentinel) and out_bn."""
    case = f"k_chan_ops pixels {pixels} C {c} {mode}"
    x, slope, scale, shift = chan_case(pixels, c)
    with np.errstate(over="ignore", invalid="ignore"):
        act, bn = chan_emulate(x, slope if mode.startswith("prelu") else None, scale, shift)
    n = pixels * c
    assert (in_after[n:] == S16).all() and (bn_buf[n:] == S16).all() and (act_buf == S16).all(), f"{case}: a store outside the tensors"
    want_in = act if mode.startswith("prelu") else x
    def where(bad, got, want):
        i = bad[:6]
        return (f"{bad.size} of {n} at {i.tolist()} (channel {bad[0] % c}): input {[hex(v) for v in bits(x).reshape(-1)[i]]}, "
                f"slope {slope[i % c].tolist()}, got {[hex(v) for v in got[i]]}, contract {[hex(v) for v in want[i]]}")

    bad = np.flatnonzero(in_after[:n] != bits(want_in).reshape(-1))
    assert bad.size == 0, f"{case}: the in / out_act buffer differs in bits, {where(bad, in_after, bits(want_in).reshape(-1))}"
    if mode in ("prelu_bn_aliased", "bn_only"):
        bad = np.flatnonzero(bn_buf[:n] != bits(bn).reshape(-1))
        assert bad.size == 0, f"{case}: out_bn differs in bits, {where(bad, bn_buf, bits(bn).reshape(-1))}"
    else:
        assert (bn_buf == S16).all(), f"{case}: out_bn was not requested and was written"


# ==== k_face_fc / k_face_norm ================================================================================================
FACE_M = [1, 15, 16, 17, 33]
FACE_K, FACE_SPLIT, FACE_SLICE = 25088, 16, 1568
FACE_MUTANTS = ["fc_drops_last_slice", "fc_masked_row_stored", "norm_no_floor"]
FACE_TAIL_ROWS = 16  # sentinel rows behind partial [16][m][512] and emb [m][512]: a whole group of masked rows fits


def torch_flatten_columns(w_dev):
    """[..., 25088] in the device's NHWC column order ((y * 7 + x) * 512 + c) -> torch's flatten of NCHW (c * 49 + y * 7 + x),
    by index arithmetic of its own (faces.nchw_to_nhwc_columns is what is under test)"""
    col = np.arange(FACE_K)
    c, p = col // 49, col % 49
    return w_dev[..., p * 512 + c]


@functools.lru_cache(maxsize=None)
def face_input(rms):
    """[33][7][7][512] fp16 activations of the given RMS (the torch oracle's last block: printed by the GPU test)"""
    x = (rms * np.random.default_rng(77).standard_normal((33, 7, 7, 512))).astype(np.float16)
    x.setflags(write=False)
    return x


def face_partial_ref(x, w16_dev):
    """float64 sums over exactly each slice's 1568 columns, in torch's order: the activations flattened as torch flattens NCHW,
    the weights taken back to that order.  A slice is 1568 consecutive device columns = pixels 3.0625 s .. of all channels,
    which is no range of torch columns: the slice's torch columns are gathered.  -> [16][m][512]"""
    m = x.shape[0]
    xt = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2).flatten(1).numpy()  # [m][c * 49 + p]
    wt = torch_flatten_columns(w16_dev.astype(np.float64))
    dev_col = np.arange(FACE_K)
    torch_col = (dev_col % 512) * 49 + dev_col // 512  # the torch column of each device column
    out = np.empty((FACE_SPLIT, m, 512))
    for s in range(FACE_SPLIT):
        cols = torch_col[s * FACE_SLICE:(s + 1) * FACE_SLICE]
        out[s] = xt[:, cols] @ wt[:, cols].T
    return out


def face_partial_emulate(x, w16_dev):
    """fp32, one k after the other within each slice (the MFMA's own order is not visible in the source) -> [16][m][512]"""
    m = x.shape[0]
    xs = x.reshape(m, FACE_SPLIT, FACE_SLICE).astype(F32).transpose(1, 0, 2)
    ws = w16_dev.reshape(512, FACE_SPLIT, FACE_SLICE).astype(F32).transpose(1, 0, 2)
    acc = np.zeros((FACE_SPLIT, m, 512), F32)
    for k in range(FACE_SLICE):
        acc += xs[:, :, k, None] * ws[:, None, :, k]
    return acc


def face_norm_ref(partial64, bias):
    v = partial64.sum(axis=0) + bias.astype(np.float64)
    return v / np.maximum(np.sqrt((v * v).sum(axis=1, keepdims=True)), 1e-12)


def face_norm_emulate(partial, bias, mutant=None):
    """k_face_norm on partial [16][m][512] fp32 in its own order: slices summed in order, + bias; thread t squares outputs t and
    t + 256; the block reduction; sqrtf, the 1e-12 floor, one division.  The kernel's order: the kernel's bits."""
    a = np.zeros(partial.shape[1:], F32)
    for s in range(partial.shape[0]):
        a = a + partial[s]
    v = a + bias.astype(F32)
    ss = (F32(0) + v[:, :256] * v[:, :256]) + v[:, 256:] * v[:, 256:]
    nrm = np.sqrt(block_sum_256(ss))
    if mutant != "norm_no_floor":
        nrm = np.maximum(nrm, F32(1e-12))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (v / nrm[:, None]).astype(F32)


def face_emulate_buffers(x, w16_dev, bias, part_emu, mutant=None):
    """The two output buffers as the (mutated) kernels would leave them, as uint32 bits with FACE_TAIL_ROWS sentinel rows:
    partial [(16 m + tail)][512], emb [(m + tail)][512].  part_emu: face_partial_emulate of these rows."""
    m = x.shape[0]
    part = np.full(((FACE_SPLIT * m + FACE_TAIL_ROWS), 512), S32, np.uint32)
    p = part_emu.copy()
    if mutant == "fc_drops_last_slice":
        p[FACE_SPLIT - 1] = 0
    part[:FACE_SPLIT * m] = bits(p).reshape(-1, 512)
    if mutant == "fc_masked_row_stored":  # the masked rows of the last group carry face 0 and are stored at [s][face]
        for s in range(FACE_SPLIT):
            for face in range(m, (m + 15) // 16 * 16):
                part[s * m + face] = bits(p[s, 0])
    emb = np.full((m + FACE_TAIL_ROWS, 512), S32, np.uint32)
    emb[:m] = bits(face_norm_emulate(part[:FACE_SPLIT * m].view(F32).reshape(FACE_SPLIT, m, 512), bias, mutant))
    return part, emb


def check_face_head(x, w16_dev, bias, part_buf, emb_buf, ref, part_emu, alone_of=None, report=None):
    """part_buf / emb_buf: the buffers after the call (uint32 bits, FACE_TAIL_ROWS sentinel rows).  ref = face_partial_ref and
    part_emu = face_partial_emulate of x's rows.  alone_of: (row i, emb of the m = 33 launch) - face i alone equals it."""
    m = x.shape[0]
    case = f"k_face_fc / k_face_norm m {m}"
    assert (part_buf[FACE_SPLIT * m:] == S32).all(), f"{case}: partial rows >= m were written"
    assert (emb_buf[m:] == S32).all(), f"{case}: embedding rows >= m were written"
    part = part_buf[:FACE_SPLIT * m].view(F32).reshape(FACE_SPLIT, m, 512)
    emb = emb_buf[:m].view(F32)
    for s in range(FACE_SPLIT):  # per slice: a dropped or misplaced slice cannot hide in the sum
        ok, err, bar = within_bar(part[s], ref[s], bar32_of(part_emu[s], ref[s]), False)
        _note(report, "k_face_fc partial", err=err, bar=bar)
        assert ok, f"{case} slice {s}: partial error {err:.3e} > bar {bar:.3e}"
    eref = face_norm_ref(ref, bias)
    ok, err, bar = within_bar(emb, eref, bar32_of(face_norm_emulate(part_emu, bias), eref), False)
    _note(report, "k_face_norm", err=err, bar=bar)
    assert ok, f"{case}: embedding error {err:.3e} > bar {bar:.3e}"
    assert same_bits(emb, face_norm_emulate(part, bias)), f"{case}: k_face_norm differs in bits from its own order on the device's partials"
    live = np.abs(x.reshape(m, -1)).max(axis=1) > 0
    nrm = np.linalg.norm(emb.astype(np.float64), axis=1)
    assert np.abs(nrm[live] - 1).max(initial=0) <= 1e-6, f"{case}: norms {nrm}"
    if not bias.any():
        assert (emb[~live] == 0).all(), f"{case}: a zero row with zero bias must return 0 through the floor, got {emb[~live][:, :4]}"
    if alone_of is not None:
        assert m == 1 and same_bits(emb[0], alone_of), f"{case}: the face alone differs from the same face among 33"


# ==== k_spk_pool / k_spk_head ================================================================================================
SPK_M = 5
SPK_VALID = {5: [9, 16, 23, 40, 33], 25: [15, 17, 24, 200, 193]}  # T = 2, 2, 3, Wf, Wf and 2, 3, 3, Wf, Wf; valid % 8 in {0, 1, 7}
SPK_CONST, SPK_OFFSET = 7, 11  # the constant channel; the channel with mean >> std
SPK_STAT = 5120
SPK_MUTANTS = ["spk_mean_over_wf", "spk_std_biased", "spk_std_one_pass"]


@functools.lru_cache(maxsize=None)
def spk_input(wf, fill_nan=True):
    """[5][10][wf][256] fp16.  Columns >= T = ceil(valid / 8) hold NaN (or 0): they must not be read."""
    x = np.abs(np.random.default_rng(300 + wf).standard_normal((SPK_M, 10, wf, 256))).astype(np.float16)
    x[..., SPK_CONST] = np.float16(0.71875)
    x[..., SPK_OFFSET] = (1000 + 2 * np.random.default_rng(301).standard_normal((SPK_M, 10, wf))).astype(np.float16)
    for b, v in enumerate(SPK_VALID[wf]):
        x[b, :, (v + 7) // 8:] = np.nan if fill_nan else 0
    x.setflags(write=False)
    return x


def spk_pool_ref(x, valid):
    """float64: mean | sqrt(torch.var(unbiased) + 1e-7) over the first T columns, each f * 256 + c -> [m][5120]"""
    out = np.empty((x.shape[0], SPK_STAT))
    for b, v in enumerate(valid):
        t = torch.from_numpy(x[b, :, :(v + 7) // 8].astype(np.float64))
        out[b, :SPK_STAT // 2] = t.mean(dim=1).reshape(-1).numpy()
        out[b, SPK_STAT // 2:] = torch.sqrt(t.var(dim=1, unbiased=True) + 1e-7).reshape(-1).numpy()
    return out


def spk_pool_emulate(x, valid, mutant=None):
    """the kernel's own loops in fp32 (sequential sum, s / T; d = x - mean, q += d * d without FMA; sqrtf(q / (T - 1) + 1e-7f)):
    the kernel's order, the kernel's bits"""
    out = np.empty((x.shape[0], SPK_STAT), F32)
    for b, v in enumerate(valid):
        T = (v + 7) // 8
        cols = x.shape[2] if mutant == "spk_mean_over_wf" else T
        xs = np.nan_to_num(x[b].astype(F32), nan=0.0) if mutant == "spk_mean_over_wf" else x[b].astype(F32)
        s = np.zeros((10, 256), F32)
        for t in range(cols):
            s = s + xs[:, t]
        mean = s / F32(cols)
        q = np.zeros((10, 256), F32)
        if mutant == "spk_std_one_pass":
            for t in range(T):
                q = q + xs[:, t] * xs[:, t]
            q = np.maximum(q - F32(T) * (mean * mean), F32(0))
        else:
            for t in range(T):
                d = xs[:, t] - mean
                q = q + d * d
        den = F32(T if mutant == "spk_std_biased" else T - 1)
        out[b, :SPK_STAT // 2] = mean.reshape(-1)
        out[b, SPK_STAT // 2:] = np.sqrt(q / den + F32(1e-7)).reshape(-1)
    return out


def check_spk_pool(wf, stats_buf, report=None):
    """stats_buf: uint32 bits [(5 + 1)][5120], the last row sentinel, after pooling spk_input(wf)"""
    case = f"k_spk_pool Wf {wf}"
    x, valid = spk_input(wf), SPK_VALID[wf]
    assert (stats_buf[SPK_M:] == S32).all(), f"{case}: a row of another window was written"
    got = stats_buf[:SPK_M].view(F32)
    ref, emu = spk_pool_ref(x, valid), spk_pool_emulate(x, valid)
    for b in range(SPK_M):
        ok, err, bar = within_bar(got[b], ref[b], bar32_of(emu[b], ref[b]), False)
        _note(report, "k_spk_pool", err=err, bar=bar)
        assert ok, f"{case} window {b} (valid {valid[b]}): error {err:.3e} > bar {bar:.3e}"
        assert same_bits(got[b], emu[b]), f"{case} window {b} (valid {valid[b]}): differs in bits from the kernel's own order"
    const = got[:, SPK_STAT // 2:].reshape(SPK_M, 10, 256)[..., SPK_CONST]
    assert (const == np.sqrt(F32(1e-7))).all(), f"{case}: the constant channel's std is not sqrt(1e-7)"


@functools.lru_cache(maxsize=None)
def spk_head_stats():
    """[5][5120] fp32 statistics in the device's column order: what the pool's emulation gives on spk_input(5)"""
    return spk_pool_emulate(spk_input(5), SPK_VALID[5])


def spk_head_ref(stats_torch_order, w_torch, b):
    """float64 seg_1 on torch's column order (means then stds, each c * 10 + f) with the checkpoint's own weight"""
    return stats_torch_order.astype(np.float64) @ w_torch.astype(np.float64).T + b.astype(np.float64)


def spk_head_emulate(stats, w_dev, b):
    """thread t: columns t + 256 j, j = 0 .. 19 in order (no FMA); the block reduction; + bias.  The kernel's bits."""
    m = stats.shape[0]
    s = stats.reshape(m, 1, 20, 256)
    w = w_dev.astype(F32).reshape(1, 256, 20, 256)
    a = np.zeros((m, 256, 256), F32)
    for j in range(20):
        a = a + w[:, :, j] * s[:, :, j]
    return block_sum_256(a) + b.astype(F32)


def check_spk_head(m, out_buf, w_dev, w_torch, b, device_to_torch, report=None):
    """out_buf: uint32 bits [(m + 1)][256], the last row sentinel.  device_to_torch: speakers.device_to_torch_columns."""
    case = f"k_spk_head m {m}"
    stats = spk_head_stats()[:m]
    assert (out_buf[m:] == S32).all(), f"{case}: a row >= m was written"
    got = out_buf[:m].view(F32)
    ref, emu = spk_head_ref(device_to_torch(stats), w_torch, b), spk_head_emulate(stats, w_dev, b)
    ok, err, bar = within_bar(got, ref, bar32_of(emu, ref), False)
    _note(report, "k_spk_head", err=err, bar=bar)
    assert ok, f"{case}: error {err:.3e} > bar {bar:.3e}"
    assert same_bits(got, emu), f"{case}: differs in bits from the kernel's own order"
