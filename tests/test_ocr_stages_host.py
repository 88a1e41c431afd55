"""CPU: the float64 references of tests/ocr_stage_oracle.py pinned to torch / hand arithmetic, and the conditions its input
recipes promise to tests/test_ocr_stages_gpu.py (exact fp32 upsampling, decided CTC rows, the tail's margin-stable
share)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ocr_oracle
import ocr_stage_oracle as so
from eioku_amd import ocr


# ---- references ----------------------------------------------------------------------------------------------------
def test_canvas_reference_is_the_oracle_input_in_eight_channels():
    f = so.canvas_frames(1, 2, 50, 70)
    c = so.canvas_f16(f, 2560)
    assert c.shape == (2, 64, 96, 8) and c.dtype == np.float16 and not c[..., 3:].any()
    x, _ = ocr_oracle.craft_input(f, 2560)
    assert np.array_equal(c[..., :3], x.permute(0, 2, 3, 1).numpy().astype(np.float16))
    pad = so.pad_value_f16()
    assert (c[:, 50:, :, :3] == pad).all() and (c[:, :, 70:, :3] == pad).all()
    want = [np.float16(np.float32(-m * 255.0) / np.float32(s * 255.0)) for m, s in zip(ocr_oracle.MEAN, ocr_oracle.STD)]
    assert pad.tolist() == want
    # the resize path: the taps' restatement, on a canvas smaller than the frame
    c = so.canvas_f16(so.canvas_frames(2, 1, 97, 33), 32)
    assert c.shape == (1, 32, 32, 8) and ocr.craft_canvas(97, 33, 32)[1:3] == (32, 10)
    assert ocr.linear_taps(97, 32)[-1, 0] + 1 <= 96 and ocr.linear_taps(33, 10)[:, 0].max() <= 32


@pytest.mark.parametrize("k,s,p,h,w", [((2, 2), (2, 2), (0, 0), 6, 10), ((2, 1), (2, 1), (0, 0), 4, 5), ((3, 3), (1, 1), (1, 1), 1, 1),
                                       ((3, 3), (1, 1), (1, 1), 5, 7)])
def test_maxpool_reference_against_plain_loops(k, s, p, h, w):
    x = so.f16_values(3, (2, h, w, 8), negative=True)
    got = so.maxpool(x, k, s, p)
    ho, wo = (h + 2 * p[0] - k[0]) // s[0] + 1, (w + 2 * p[1] - k[1]) // s[1] + 1
    assert got.shape == (2, ho, wo, 8)
    for y in range(ho):
        for xo in range(wo):
            ys = [y * s[0] - p[0] + d for d in range(k[0]) if 0 <= y * s[0] - p[0] + d < h]
            xs = [xo * s[1] - p[1] + d for d in range(k[1]) if 0 <= xo * s[1] - p[1] + d < w]
            assert np.array_equal(got[:, y, xo], x[:, ys][:, :, xs].max(axis=(1, 2)))


def test_im2col_reference_is_tap_major_as_fc6_reads_it():
    """conv2d(3x3, dilation 6, padding 6) == the im2col times the weights laid out [o][(ky * 3 + kx) * C + c]."""
    x = so.f16_values(4, (2, 7, 9, 8))
    col = so.im2col_dil(x, 6).astype(np.float64)
    assert col.shape == (2, 7, 9, 9, 8)
    w = np.random.default_rng(5).standard_normal((4, 8, 3, 3))
    ref = F.conv2d(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), torch.from_numpy(w), padding=6, dilation=6)
    got = col.reshape(2, 7, 9, 72) @ w.transpose(0, 2, 3, 1).reshape(4, 72).T
    assert np.allclose(got, ref.permute(0, 2, 3, 1).numpy(), atol=1e-12)
    assert np.array_equal(col[:, :, :, 4], x.astype(np.float64))  # the centre tap is the input


def test_up2x_reference_against_the_quarter_weights():
    x = so.up2x_values(6, (1, 3, 4, 8))
    y = so.up2x(x).astype(np.float64)
    a = x.astype(np.float64)
    assert np.array_equal(y[0, 0, 0], a[0, 0, 0])  # clamped corner
    # output (3, 2): rows 0.25 x in[1] + 0.75 x in[2]... odd row 3 -> 0.75 in[1] + 0.25 in[2]; even column 2 -> 0.25 in[0] + 0.75 in[1]
    want = 0.75 * (0.25 * a[0, 1, 0] + 0.75 * a[0, 1, 1]) + 0.25 * (0.25 * a[0, 2, 0] + 0.75 * a[0, 2, 1])
    assert np.array_equal(y[0, 3, 2], want.astype(np.float16).astype(np.float64))


def test_ctc_reference_is_softmax_then_ignore_renormalise():
    l, ignore = so.ctc_case(97, 9, "top")
    idx, prob, margin = so.ctc(l, ignore)
    p = ocr.ignore_renormalise(F.softmax(torch.from_numpy(l.astype(np.float64)), -1).numpy(), np.flatnonzero(ignore))
    # ignore_renormalise works in float32; rows with a spread of 60 keep little mass on the kept classes
    assert np.array_equal(idx, p.argmax(-1)) and np.allclose(prob, p.max(-1), rtol=1e-5)
    assert not ignore[idx].any() and (prob > 0).all() and (prob <= 1).all()


def test_tail_reference_against_explicit_lstm_cells():
    sd = so.tail_state()
    seq = so.tail_inputs((5,))[0]
    got = so.tail_logits(sd, [seq], torch.float64)[0]
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    v = seq.astype(np.float64)
    for l in range(2):
        p = f"SequenceModeling.{l}.rnn."
        outs = []
        for suf, order in (("_l0", range(5)), ("_l0_reverse", range(4, -1, -1))):
            wi, wh, bi, bh = (sd[p + n + suf].astype(np.float64) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
            h, c, hs = np.zeros(256), np.zeros(256), np.zeros((5, 256))
            for t in order:
                i, f, g, o = np.split(wi @ v[t] + bi + wh @ h + bh, 4)  # PyTorch gate order
                c = sig(f) * c + sig(i) * np.tanh(g)
                h = sig(o) * np.tanh(c)
                hs[t] = h
            outs.append(hs)
        q = f"SequenceModeling.{l}.linear."
        v = np.concatenate(outs, 1) @ sd[q + "weight"].astype(np.float64).T + sd[q + "bias"]
    want = v @ sd["Prediction.weight"].astype(np.float64).T + sd["Prediction.bias"]
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


# ---- recipes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (1, 5), (4, 1), (5, 7)])
def test_up2x_recipe_makes_fp32_exact(h, w):
    x = so.up2x_values(h * 10 + w + 8, (2, h, w, 16))
    assert (np.abs(x) < 4).all() and (np.abs(x) >= 2.0 ** -6).all()
    t = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)
    y64 = F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)
    y32 = F.interpolate(t.float(), scale_factor=2, mode="bilinear", align_corners=False)
    assert torch.equal(y32.double(), y64)
    assert np.array_equal(so.up2x(x, torch.float32), so.up2x(x))


@pytest.mark.parametrize("C", [2, 63, 64, 65, 97, 4096])
def test_ctc_recipes_decide_every_row(C):
    for mask in so.CTC_MASKS:
        for rows in (1, 4, 5, 9):
            l, ignore = so.ctc_case(C, rows, mask)
            assert l.shape == (rows, C) and l.dtype == np.float32 and 0 < (ignore == 0).sum()
            _, prob, margin = so.ctc(l, ignore)
            assert (margin > so.CTC_MARGIN).all() and (prob > 0).all()
            if rows > 1 and mask == "none":
                assert abs(float(l[1].max() - l[1].min()) - 60.0) < 2.0  # the wide rows (before the winner was raised)
            if mask == "top":
                assert ignore[l.argmax(-1)].all()
            if mask == "all_but_one":
                assert (ignore == 0).sum() == 1 and np.allclose(prob, 1.0, rtol=0, atol=1e-15)
    l, names, lo, hi = so.ctc_tie_cases(C)
    assert len(names) == (1 if C < 64 else 2 if C == 64 else 3)
    for r in range(len(names)):
        assert lo[r] < hi[r] < C and l[r, lo[r]] == l[r, hi[r]]
        assert np.sort(l[r])[-3] <= l[r, lo[r]] - 1.0 if C > 2 else True
    by_name = dict(zip(names, zip(lo, hi)))
    if C > 64:
        a, b = by_name["one lane (c, c + 64)"]
        assert b == a + 64
    if C >= 64:
        a, b = by_name["lanes 0 and 63"]
        assert a % 64 == 0 and b % 64 == 63
    a, b = by_name["neighbouring lanes"]
    assert b == a + 1


@pytest.mark.parametrize("name", list(so.TAIL_SETS))
def test_tail_recipe_leaves_the_reference_decided(name):
    """float32 torch's own drift leaves 16 x d_ref under 1e-4, and at least 90 % of the steps keep a float64 top-2 margin
    above 4 x that bar (the GPU test uses its measured drift, which the bar bounds)."""
    seqs, l64, d_ref, idx, prob, margin = so.tail_reference(name)
    assert [len(s) for s in seqs] == list(so.TAIL_SETS[name])
    assert 0 < 16 * d_ref < 1e-4, d_ref
    scale = float(np.abs(l64).max())
    assert (margin > 4 * 16 * d_ref * scale).mean() >= 0.9
    assert not np.isin(idx, so.TAIL_IGNORE).any()
    # standard normal features keep the gates out of saturation: pre-activations O(1)
    sd = so.tail_state()
    pre = np.concatenate(seqs) @ sd["SequenceModeling.0.rnn.weight_ih_l0"].T
    assert 0.3 < pre.std() < 1.0


def test_tail_sets_cover_the_row_tails():
    rows = {n: sum(v) for n, v in so.TAIL_SETS.items()}
    assert rows["15 rows"] == 15 and rows["17 rows"] == 17
    assert len(so.TAIL_SETS["five sequences, partial last tile"]) % 4 == 1 and max(so.TAIL_SETS["five sequences, partial last tile"]) == 63
