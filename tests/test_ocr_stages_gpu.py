"""GPU: OCR stage by stage.  Everything in csrc/ocr.hip that is not a convolution against a float64 reference of its own
(tests/ocr_stage_oracle.py) through the stage entry points - bit for bit where the arithmetic is exact - and the batch
edges of both networks (width groups of more than 64 crops, the MAX_ROWS split, CRAFT's chunks of 8 frames) through
the public API."""
import ctypes as C

import numpy as np
import pytest
import torch

import ocr_oracle
import ocr_stage_oracle as so
from eioku_amd import _lib, ocr
from eioku_amd.synth import ocr_crops as crops, ocr_frames as frames
from test_ocr_gpu import CONF_TOL, MAP_TOL, reader  # noqa: F401  (the module fixture: seeded CRAFT + english_g2)

pytestmark = pytest.mark.gpu

# recogniser tail (fp32 GEMMs on MFMA, BiLSTMs, Linear, Prediction) vs float64 torch: logits drift / max |logit| must stay
# within TAIL_FACTOR x d_ref, d_ref = float32 torch's own drift on the same inputs (summation order, 1-2 ulp expf / tanhf,
# compounding over up to 63 steps in two layers), and TAIL_FACTOR x d_ref itself below TAIL_CEIL
TAIL_FACTOR = 16  # measured on MI355X: drift 6.1e-7 .. 8.2e-7 = 1.3 .. 2.0 x d_ref (d_ref 3.7e-7 .. 5.4e-7) over the seven sets
TAIL_CEIL = 1e-4
# k_ctc_probs vs float64, relative: l - mx rounds by <= 2^-24 x 88; 64-lane partial sums + 6 shuffle steps carry about
# (C / 64 + 6) x 6e-8; three times over (numerator, se, kept), each under 1.5e-5 at C = 4096
CTC_PROB_TOL = 2e-5  # measured on MI355X: worst 2.6e-7 (C = 4096, no mask); 1.5e-7 at C = 97; exactly 1.0f with one class kept


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(got: torch.Tensor, want: np.ndarray):
    g = got.cpu().numpy()
    assert g.shape == want.shape
    bad = np.flatnonzero(g.view(np.uint16).ravel() != want.view(np.uint16).ravel())
    assert bad.size == 0, (bad.size, [(np.unravel_index(i, g.shape), g.ravel()[i], want.ravel()[i]) for i in bad[:4]])


# ---- canvas: k_craft_prep ------------------------------------------------------------------------------------------
CANVAS_CASES = {
    "copy 50x70, padded rows and columns": (50, 70, 2560),
    "copy 64x96, no padding": (64, 96, 2560),
    "copy 1x1": (1, 1, 2560),
    "taps 130x201 to 96": (130, 201, 96),
    "taps 201x130 to 96": (201, 130, 96),
    "taps 97x33 to 32, far-edge clamp": (97, 33, 32),
}


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("case", list(CANVAS_CASES))
def test_canvas_equals_the_oracle_input_bit_for_bit(reader, case, mem):
    h, w, canvas = CANVAS_CASES[case]
    f = so.canvas_frames(h * 1000 + w, 3, h, w)
    want = so.canvas_f16(f, canvas)
    got = reader.canvas(dev(f) if mem == "device" else f, canvas)
    same_bits(got, want)
    _, th, tw, H, W = ocr.craft_canvas(h, w, canvas)
    g = got.cpu().numpy()
    assert g.shape == (3, H, W, 8) and not g[..., 3:].any()
    pad = so.pad_value_f16()
    assert (g[:, th:, :, :3] == pad).all() and (g[:, :, tw:, :3] == pad).all()
    if case.startswith("copy 50x70"):
        assert th < H and tw < W


# ---- max pool ------------------------------------------------------------------------------------------------------
POOL_CASES = {
    "2x2 s2 on 6x10": ((2, 2), (2, 2), (0, 0), 6, 10, False),
    "(2,1) s(2,1) on 4x5": ((2, 1), (2, 1), (0, 0), 4, 5, False),
    "3x3 s1 p1 on 1x1, negative": ((3, 3), (1, 1), (1, 1), 1, 1, True),
    "3x3 s1 p1 on 2x3, negative": ((3, 3), (1, 1), (1, 1), 2, 3, True),
    "3x3 s1 p1 on 5x7, negative": ((3, 3), (1, 1), (1, 1), 5, 7, True),
}


@pytest.mark.parametrize("layout", ["dense", "slices"])
@pytest.mark.parametrize("C", [8, 16])
@pytest.mark.parametrize("case", list(POOL_CASES))
def test_maxpool_equals_float64_max_pool2d(gpu, case, C, layout):
    k, s, p, h, w, neg = POOL_CASES[case]
    if layout == "slices":
        # the input as channels 64.. of a 192-channel tensor, the output as channels 8.. of a 24-channel one
        x = so.f16_values(h * w + C, (2, h, w, 192), neg)
        ci, co = 64, 8
        xin = x[..., ci:ci + C]
    else:
        x = xin = so.f16_values(h * w + C, (2, h, w, C), neg)
        ci, co = 0, 0
    want = so.maxpool(xin, k, s, p)
    if neg:
        assert (want < 0).all()
    full = so.strided(want, 24, co) if layout == "slices" else want
    out = torch.full(full.shape, so.SENTINEL, dtype=torch.float16, device="cuda")
    ocr.maxpool_f16(dev(x), (ci, C), k, s, p, out, (co, C))
    same_bits(out, full)  # the sentinel channels around the slice included


# ---- dilated im2col ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 16])
@pytest.mark.parametrize("h,w", [(4, 4), (7, 7), (6, 13)], ids=["4x4 centre tap only", "7x7 first off-centre tap", "6x13"])
def test_im2col_dilation_6_equals_unfold(gpu, h, w, C):
    x = so.f16_values(h * 100 + w + C, (2, h, w, C))
    x[x == 0] = np.float16(1.0)  # a landed tap is never zero, an out-of-range one always
    want = so.im2col_dil(x, 6)
    landed = (want != 0).any(axis=(0, 1, 2, 4))
    assert landed[4] and landed.sum() == (3 if h >= 7 else 1) * (3 if w >= 7 else 1)
    same_bits(ocr.im2col_dil_f16(dev(x), 6), want)


# ---- 2x bilinear upsample ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 16])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 5), (4, 1), (5, 7)])
def test_up2x_equals_float64_interpolate_rounded_once(gpu, h, w, C):
    x = so.up2x_values(h * 10 + w + C, (2, h, w, C))
    full = so.strided(so.up2x(x), 24, 8)
    out = torch.full(full.shape, so.SENTINEL, dtype=torch.float16, device="cuda")
    ocr.up2x_f16(dev(x), out, 8)
    same_bits(out, full)
    dense = torch.empty((2, 2 * h, 2 * w, C), dtype=torch.float16, device="cuda")
    same_bits(ocr.up2x_f16(dev(x), dense), so.up2x(x))


def test_glue_entry_points_refuse_bad_slices(gpu):
    x = torch.zeros((1, 4, 4, 16), dtype=torch.float16, device="cuda")
    out = torch.zeros((1, 2, 2, 16), dtype=torch.float16, device="cuda")
    with pytest.raises(_lib.EiokuHipError, match="multiple of 8"):
        ocr.maxpool_f16(x, (0, 12), (2, 2), (2, 2), (0, 0), out, (0, 12))
    with pytest.raises(_lib.EiokuHipError, match="8-aligned"):
        ocr.maxpool_f16(x, (4, 8), (2, 2), (2, 2), (0, 0), out, (0, 8))
    with pytest.raises(_lib.EiokuHipError, match="inside the stride"):
        ocr.maxpool_f16(x, (16, 8), (2, 2), (2, 2), (0, 0), out, (0, 8))
    with pytest.raises(_lib.EiokuHipError, match="32-bit"):
        _lib.check(_lib.load().eioku_ocr_im2col_dil_f16(x.data_ptr(), 1 << 14, 1 << 8, 1 << 8, 16, 6, out.data_ptr(), None), "im2col")
    with pytest.raises(_lib.EiokuHipError, match="classes"):
        ocr.ctc_probs(torch.zeros((1, 1), device="cuda"), torch.zeros(1, dtype=torch.uint8, device="cuda"))


# ---- CTC probabilities ---------------------------------------------------------------------------------------------
CTC_C = [2, 63, 64, 65, 97, 4096]
CTC_ROWS = [1, 4, 5, 9]  # one workgroup handles four rows


@pytest.mark.parametrize("mask", so.CTC_MASKS)
@pytest.mark.parametrize("C", CTC_C)
def test_ctc_index_and_probability_against_float64(gpu, C, mask):
    worst = 0.0
    for rows in CTC_ROWS:
        l, ignore = so.ctc_case(C, rows, mask)
        ridx, rprob, margin = so.ctc(l, ignore)
        assert (margin > so.CTC_MARGIN).all()
        idx, prob = (t.cpu().numpy() for t in ocr.ctc_probs(dev(l), dev(ignore)))
        assert np.array_equal(idx, ridx), (C, rows, mask)
        assert not ignore[idx].any()
        if mask == "top":
            assert ignore[l.argmax(-1)].all()  # the raw top class of every row is masked
        if mask == "all_but_one" or C - int(ignore.sum()) == 1:
            assert (prob == np.float32(1.0)).all(), (C, rows, prob)
        rel = float((np.abs(prob - rprob) / rprob).max())
        worst = max(worst, rel)
        assert rel <= CTC_PROB_TOL, (C, rows, mask, rel)
    print(f"\nk_ctc_probs C={C} mask={mask}: prob rel err vs float64 {worst:.2e}")


@pytest.mark.parametrize("C", CTC_C)
def test_ctc_exact_ties_resolve_to_the_lower_kept_class(gpu, C):
    l, names, lo, hi = so.ctc_tie_cases(C)
    none = np.zeros(C, np.uint8)
    idx, _ = ocr.ctc_probs(dev(l), dev(none))
    for name, got, want in zip(names, idx.cpu().numpy(), lo):
        assert got == want, f"C={C}, tie on {name}: class {got}, the lower is {want}"
    if C == 2:
        return  # masking the lower class of two leaves no tie to decide (all_but_one covers it)
    for r, name in enumerate(names):  # the lower class of the tie ignored: the upper must win
        ign = none.copy()
        ign[lo[r]] = 1
        got = int(ocr.ctc_probs(dev(l[r:r + 1]), dev(ign))[0].cpu().numpy()[0])
        assert got == hi[r], f"C={C}, tie on {name} with the lower class ignored: class {got}, expected {hi[r]}"


# ---- the recogniser's tail -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tail(gpu):
    t = ocr.SequenceTail(so.tail_state())  # BiLSTM + Prediction weights only: the VGG convolutions have none
    yield t
    t.close()


@pytest.mark.parametrize("name", list(so.TAIL_SETS))
def test_crnn_tail_against_float64_torch(tail, name):
    seqs, l64, d_ref, ridx, rprob, margin = so.tail_reference(name)
    got = tail(seqs, so.TAIL_IGNORE)
    assert [len(g[0]) for g in got] == list(so.TAIL_SETS[name])
    idx, prob, logits = (np.concatenate([g[k] for g in got]) for k in range(3))
    scale = float(np.abs(l64).max())
    drift = float(np.abs(logits - l64).max()) / scale
    worst_seq = int(np.argmax([np.abs(g[2] - l64[o:o + len(g[2])]).max() for g, o in
                               zip(got, np.concatenate([[0], np.cumsum(so.TAIL_SETS[name])[:-1]]))]))
    print(f"\nCRNN tail {name}: logits drift / max|logit| GPU {drift:.2e}, float32 torch (d_ref) {d_ref:.2e}, "
          f"ratio {drift / d_ref:.2f}; worst sequence {worst_seq}")
    assert TAIL_FACTOR * d_ref < TAIL_CEIL
    assert drift <= TAIL_FACTOR * d_ref, (name, drift, d_ref, worst_seq)
    stable = margin > 4 * drift * scale
    assert stable.mean() >= 0.9
    assert np.array_equal(idx[stable], ridx[stable])
    assert not np.isin(idx, so.TAIL_IGNORE).any()
    rel = float((np.abs(prob - rprob) / rprob)[stable].max())
    print(f"CRNN tail {name}: {int(stable.sum())} of {len(stable)} steps margin-stable, prob rel err {rel:.2e}")
    # the probability carries the logits' drift (d softmax <= 2 x max |d logit|) on top of k_ctc_probs' own error
    assert rel <= 2 * TAIL_FACTOR * d_ref * scale + CTC_PROB_TOL


def test_crnn_tail_needs_no_vgg_weights_but_needs_its_own(gpu):
    lib, r = _lib.load(), C.c_void_p()
    _lib.check(lib.eioku_crnn_create(97, C.byref(r)), "eioku_crnn_create")
    seq, ln, ign = np.zeros((1, 256), np.float32), np.ones(1, np.int32), np.zeros(97, np.uint8)
    idx, prob = np.zeros(1, np.int32), np.zeros(1, np.float32)
    rc = lib.eioku_crnn_tail(r, seq.ctypes.data, ln.ctypes.data, 1, ign.ctypes.data, idx.ctypes.data, prob.ctypes.data, None, None)
    lib.eioku_crnn_destroy(r)
    assert rc == -1 and "no weights" in _lib.last_error()


# ---- recogniser batching -------------------------------------------------------------------------------------------
def assert_each_crop_as_alone(reader, imgs, alone_of):
    got = reader.recognize_raw(imgs, want_logits=True)
    assert len(got) == len(imgs)
    for k, (a, g) in enumerate(zip(imgs, got)):
        for what, x, y in zip(("idx", "prob", "logits"), g, alone_of(k, a)):
            assert np.array_equal(x, y), f"crop {k} (width {a.shape[1]}) of {len(imgs)}: {what} differs from the crop alone"


def test_width_group_split_at_64_with_interleaved_widths(reader):
    widths = [64] * 70
    for pos, wdt in ((3, 128), (17, 192), (30, 128), (44, 128), (74, 192)):  # the last crop is a wide one
        widths.insert(pos, wdt)
    assert widths.count(64) == 70 and widths.count(128) == 3 and widths.count(192) == 2
    imgs = crops(21, widths)
    assert_each_crop_as_alone(reader, imgs, lambda k, a: reader.recognize_raw([a], want_logits=True)[0])


@pytest.mark.parametrize("m", [64, 65])
def test_one_width_at_exactly_the_group_size_and_one_more(reader, m):
    imgs = crops(22, [64] * m)
    assert_each_crop_as_alone(reader, imgs, lambda k, a: reader.recognize_raw([a], want_logits=True)[0])


def test_max_rows_split_gives_the_same_arrays(reader, monkeypatch):
    imgs = crops(23, [64, 128, 64, 192, 64, 64, 128, 64, 256, 64, 64, 128])
    whole = reader.recognize_raw(imgs, want_logits=True)
    calls = []
    call = reader._recognize_call
    monkeypatch.setattr(reader, "_recognize_call", lambda chunk, wl: calls.append(len(chunk)) or call(chunk, wl))
    monkeypatch.setattr(ocr, "MAX_ROWS", 40)
    split = reader.recognize_raw(imgs, want_logits=True)
    assert len(calls) > 2 and sum(calls) == len(imgs)
    for k, (a, b) in enumerate(zip(whole, split)):
        for x, y in zip(a, b):
            assert np.array_equal(x, y), f"crop {k}"


def test_widths_the_pipeline_never_produces(reader):
    widths = [8, 12, 68, 100]
    imgs = crops(24, widths)
    got = reader.recognize_raw(imgs, want_logits=True)
    ref = ocr_oracle.crnn_probs(ocr.random_crnn_state(6), imgs, reader.ignore_idx)
    for (gi, gp, gl), (ri, rp, rl), wdt in zip(got, ref, widths):
        T = wdt // 4 - 1
        assert len(gi) == len(gp) == T and gl.shape == rl.shape == (T, reader.num_class)
        err = float(np.abs(gl - rl).max())
        print(f"\nCRNN width {wdt} (T = {T}): logits drift / max|logit| {err / float(np.abs(rl).max()):.2e}")
        assert err <= 1e-2 * float(np.abs(rl).max()), wdt
        srt = np.sort(rl, -1)
        if (srt[:, -1] - srt[:, -2]).min() > 4 * err:  # margin-stable, as test_ocr_gpu.py
            assert np.array_equal(gi, ri), wdt
            cg, cr = ocr.confidence(gi, gp), ocr.confidence(ri, rp)
            assert abs(cg - cr) <= CONF_TOL * max(cr, 1e-30), (wdt, cg, cr)


# ---- CRAFT chunks --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nine(reader):
    f = frames(31, 9, 64, 96)
    return f, tuple(t.cpu().numpy() for t in reader.score_maps(f))


def test_second_chunk_equals_the_frame_alone(reader, nine):
    f, (text, link, binm) = nine
    assert text.shape == link.shape == binm.shape == (9, 32, 48)
    for name, got, alone in zip(("text", "link", "bin"), (text, link, binm), reader.score_maps(f[8:9])):
        assert np.array_equal(got[8], alone.cpu().numpy()[0]), f"{name} map of frame 8 (second chunk)"


def test_device_frames_equal_host_frames(reader, nine):
    f, maps = nine
    for name, want, got in zip(("text", "link", "bin"), maps, reader.score_maps(dev(f))):
        assert np.array_equal(got.cpu().numpy(), want), name


def test_without_the_link_map_text_and_bin_are_unchanged(reader, nine):
    f, (text, _, binm) = nine
    t, l, b = reader.score_maps(f, want_link=False)
    assert l is None
    assert np.array_equal(t.cpu().numpy(), text) and np.array_equal(b.cpu().numpy(), binm)


def test_first_chunk_meets_the_map_bar(reader, nine):
    f, (text, link, _) = nine
    x, _ = ocr_oracle.craft_input(f[:8])
    with torch.no_grad():
        ref = ocr_oracle.craft(ocr.random_craft_state(5, reader.cls_bias), x).numpy()
    for name, got, r in (("text", text[:8], ref[..., 0]), ("link", link[:8], ref[..., 1])):
        for k in range(8):
            rng_ = float(r[k].max() - r[k].min())
            err = float(np.abs(got[k] - r[k]).max())
            assert err <= MAP_TOL * rng_, (name, k, err, rng_)
