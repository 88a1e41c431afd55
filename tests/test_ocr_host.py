"""CPU: the OCR host side - loaders, CTC decode and confidence, CRAFT box post-processing on planted score maps with
hand-computed boxes, crops, and the extract_ocr / process_ml_task wiring against the reference loop's capture
(tests/golden/ref_ocr_loop.json, made by make_ocr_loop_fixture.py)."""
import asyncio
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from eioku_amd import ocr, task_handler
from eioku_amd.model_manager import ModelManager
from test_host_boundary import ScriptedSource

CASES = json.loads((GOLDEN / "ref_ocr_loop.json").read_text())


# ---- loaders -------------------------------------------------------------------------------------------------------
def test_fold_conv_strips_module_prefix_and_folds_bn():
    sd = ocr.random_craft_state(3)
    wrapped = {"module." + k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    st = ocr._np_state(wrapped)
    assert set(st) == set(sd)
    w, b = ocr.fold_conv(st, "basenet.slice1.3")
    x = torch.randn(1, 64, 9, 9, dtype=torch.float64)
    t = lambda k: torch.from_numpy(np.asarray(sd[k], np.float64))
    ref = F.batch_norm(F.conv2d(x, t("basenet.slice1.3.weight"), t("basenet.slice1.3.bias"), padding=1), t("basenet.slice1.4.running_mean"),
                       t("basenet.slice1.4.running_var"), t("basenet.slice1.4.weight"), t("basenet.slice1.4.bias"), False, 0.0, 1e-5)
    got = F.conv2d(x, torch.from_numpy(w.astype(np.float64)), torch.from_numpy(b.astype(np.float64)), padding=1)
    assert torch.allclose(got, ref, atol=1e-5, rtol=1e-5)
    # no BatchNorm after fc6, no bias in the recogniser's BN convs
    w6, b6 = ocr.fold_conv(st, "basenet.slice5.1")
    assert np.array_equal(w6, sd["basenet.slice5.1.weight"]) and np.array_equal(b6, sd["basenet.slice5.1.bias"])
    rs = ocr.random_crnn_state(4)
    assert "FeatureExtraction.ConvNet.11.bias" not in rs
    w11, b11 = ocr.fold_conv(rs, "FeatureExtraction.ConvNet.11")
    s = rs["FeatureExtraction.ConvNet.12.weight"] / np.sqrt(rs["FeatureExtraction.ConvNet.12.running_var"] + 1e-5)
    assert np.allclose(b11, rs["FeatureExtraction.ConvNet.12.bias"] - rs["FeatureExtraction.ConvNet.12.running_mean"] * s, atol=1e-6)


def test_charset_and_class_count():
    chars, ignore = ocr.charset()
    assert len(chars) == 96 and chars[0] == "0" and chars.endswith("xyz") and "€" in chars
    # english_g2's `symbols` include the euro sign, so readtext's ignore set for ['en'] is empty
    assert ignore == []


# ---- decode ----------------------------------------------------------------------------------------------------------
def test_ignore_renormalise():
    p = np.array([[0.1, 0.2, 0.3, 0.4], [0.5, 0.25, 0.125, 0.125]], np.float32)
    q = ocr.ignore_renormalise(p, [3])
    assert np.allclose(q, [[1 / 6, 2 / 6, 3 / 6, 0], [0.5 / 0.875, 0.25 / 0.875, 0.125 / 0.875, 0]], atol=1e-7)
    assert q.dtype == np.float32 and np.array_equal(ocr.ignore_renormalise(p, []), p)


def test_decode_greedy_and_custom_mean():
    chars = "abc"
    assert ocr.decode_greedy([0, 1, 1, 0, 1, 2, 2, 3, 0, 0], chars) == "aabc"
    assert ocr.decode_greedy([0, 0], chars) == ""
    idx = np.array([0, 1, 1, 0, 2])
    prob = np.array([0.9, 0.5, 0.8, 0.99, 0.25], np.float32)
    assert ocr.confidence(idx, prob) == pytest.approx((0.5 * 0.8 * 0.25) ** (2 / math.sqrt(3)), rel=1e-6)
    assert ocr.confidence([0, 0, 0], [0.9, 0.9, 0.9]) == 0.0  # no non-blank step: custom_mean([0])


# ---- box post-processing on planted maps -------------------------------------------------------------------------
def planted(h=60, w=170):
    return np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)


def test_two_words_on_one_line_merge():
    text, link = planted()
    text[10:20, 10:40] = 0.9
    text[10:20, 45:75] = 0.9
    boxes = ocr.det_boxes(text, link)
    # niter = int(sqrt(300 * 10 / 300) * 2) = 6: a 7 x 7 dilation, 3 pixels each way
    assert [b.tolist() for b in boxes] == [[[7, 7], [42, 7], [42, 22], [7, 22]], [[42, 7], [77, 7], [77, 22], [42, 22]]]
    polys = ocr.adjust_coordinates(boxes, 1.0)
    assert [p.tolist() for p in polys] == [[14, 14, 84, 14, 84, 44, 14, 44], [84, 14, 154, 14, 154, 44, 84, 44]]
    hl, fl = ocr.group_text_box(polys)
    assert hl == [[11, 157, 11, 47]] and fl == []  # margin int(0.1 * min(140, 30)) = 3
    assert ocr.boxes_from_maps(text, link, 1.0) == ([[11, 157, 11, 47]], [])


def test_link_only_pixels_are_removed_and_weak_components_dropped():
    text, link = planted()
    text[10:20, 10:40] = 0.9
    link[25:40, 10:40] = 0.9   # a link-only component: peak text score 0 < 0.7
    text[45:55, 100:130] = 0.6  # clears low_text but not text_threshold
    text[30:32, 150:154] = 0.95  # size 8 < 10
    assert len(ocr.det_boxes(text, link)) == 1


def test_min_size_drop():
    text, link = planted()
    text[10:14, 10:14] = 0.9  # niter 4: an 8 x 8 box, 14 px after the 2x map scale, 16 with the margin
    hl, fl = ocr.boxes_from_maps(text, link, 1.0)
    assert hl == [] and fl == []
    polys = ocr.adjust_coordinates(ocr.det_boxes(text, link), 1.0)
    assert [p.tolist() for p in polys] == [[16, 16, 30, 16, 30, 30, 16, 30]]


def test_diamond_rule():
    text, link = planted(80, 80)
    yy, xx = np.mgrid[0:80, 0:80]
    text[np.abs(yy - 30) + np.abs(xx - 30) <= 6] = 0.9  # 85 pixels, niter 5: a 6 x 6 dilation, anchor 3 -> [-2, +3]
    boxes = ocr.det_boxes(text, link)
    assert [b.tolist() for b in boxes] == [[[22, 22], [39, 22], [39, 39], [22, 39]]]
    # without the rule the box would be the tilted minimum-area rectangle of the dilated diamond
    seg = np.zeros_like(text, bool)
    m = text > 0.4
    for dy in range(-2, 4):
        for dx in range(-2, 4):
            seg |= np.roll(np.roll(m, dy, 0), dx, 1)
    ys, xs = np.nonzero(seg)
    r = ocr.min_area_rect_points(np.stack([xs, ys], 1))
    assert not np.allclose(r[0, 1], r[1, 1])


def test_tilted_box_takes_the_free_list_path():
    text, link = planted(100, 120)
    for x in range(10, 90):
        y0 = int(20 + 0.4 * (x - 10))
        text[y0:y0 + 10, x] = 0.9
    hl, fl = ocr.boxes_from_maps(text, link, 1.0)
    assert hl == [] and len(fl) == 1
    q = np.array(fl[0])
    slope = (q[1][1] - q[0][1]) / (q[1][0] - q[0][0])
    assert 0.3 < slope < 0.5
    grey = (np.arange(200 * 240) % 251).astype(np.uint8).reshape(200, 240)
    items = ocr.image_list(hl, fl, grey)
    assert len(items) == 1 and items[0][1].shape[0] == 64 and items[0][2] % 64 == 0


def test_ratio_scaling_of_a_frame_above_the_canvas():
    ratio, th, tw, H, W = ocr.craft_canvas(2160, 3840)
    assert (th, tw, H, W) == (1440, 2560, 1440, 2560) and ratio == 2560 / 3840
    assert ocr.craft_canvas(1080, 1920) == (1.0, 1080, 1920, 1088, 1920)
    assert ocr.craft_canvas(481, 641)[3:] == (512, 672)
    box = np.array([[7, 7], [42, 7], [42, 22], [7, 22]], np.float32)
    polys = ocr.adjust_coordinates([box], ratio)
    assert polys[0].tolist() == [21, 21, 126, 21, 126, 66, 21, 66]  # x 1 / ratio x 2 = 3


# ---- crops -----------------------------------------------------------------------------------------------------------
def test_gray_and_linear_resize():
    bgr = np.array([[[10, 200, 30], [255, 255, 255], [0, 0, 0]]], np.uint8)
    assert ocr.bgr_to_gray(bgr).tolist() == [[(10 * 1868 + 200 * 9617 + 30 * 4899 + 8192) >> 14, 255, 0]]
    img = np.arange(48, dtype=np.uint8).reshape(6, 8)
    assert np.array_equal(ocr.resize_linear_u8(img, 6, 8), img)
    up = ocr.resize_linear_u8(img, 12, 16)
    assert up[0, 0] == 0 and up[-1, -1] == 47 and up.shape == (12, 16)
    half = ocr.resize_linear_u8(img, 3, 4)  # exact 1/2: taps (1/2, 1/2) at odd centres
    assert half.tolist() == [[(img[2 * i, 2 * j] + img[2 * i, 2 * j + 1] + img[2 * i + 1, 2 * j] + img[2 * i + 1, 2 * j + 1] + 2) // 4
                              for j in range(4)] for i in range(3)]


def test_pillow_bicubic_matches_pillow():
    from PIL import Image

    rng = np.random.default_rng(0)
    for h, w, nw, nh in ((64, 150, 300, 64), (64, 37, 20, 64), (90, 64, 43, 64), (20, 33, 64, 64)):
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(img, "L").resize((nw, nh), Image.BICUBIC))
        assert np.array_equal(ocr.pil_bicubic(img, nw, nh), ref), (h, w, nw, nh)


def test_align_collate_pads_with_the_last_column():
    crop = np.tile(np.arange(0, 200, 2, dtype=np.uint8), (64, 1))  # 64 x 100
    x = ocr.align_collate(crop, 192)
    assert x.shape == (64, 192) and x.dtype == np.float32
    assert np.array_equal(x[:, 100:], np.repeat(x[:, 99:100], 92, 1))
    dull = np.full((64, 64), 60, np.uint8)
    dull[:, 32:] = 160  # contrast 100 / 220 < 0.5: stretched by 200 / 100 around low - 25 before the resize
    y = ocr.align_collate(dull, 64, adjust_contrast=0.5)
    assert y[0, 0] == pytest.approx((50 / 255 - 0.5) / 0.5) and y[0, -1] == pytest.approx((250 / 255 - 0.5) / 0.5)
    assert ocr.align_collate(dull, 64)[0, -1] == pytest.approx((160 / 255 - 0.5) / 0.5)


# ---- extract_ocr / process_ml_task against the reference loop -------------------------------------------------------
class ScriptedReader:
    def __init__(self, seed):
        from make_ocr_loop_fixture import ocr_results

        self.seed, self.frames, self.batches, self.closed = seed, [], [], False
        self._results = ocr_results

    def readtext_batch(self, frames):
        self.batches.append(len(frames))
        out = []
        for f in frames:
            i = int(f[0, 0, 0]) | (int(f[0, 0, 1]) << 8) | (int(f[0, 0, 2]) << 16)
            self.frames.append(i)
            out.append(self._results(self.seed, i))
        return out

    def close(self):
        self.closed = True


@pytest.fixture(autouse=True)
def _golden_on_path(monkeypatch):
    monkeypatch.syspath_prepend(str(GOLDEN))


@pytest.mark.parametrize("case", CASES, ids=[f"{c['fps']}-{c['total_frames']}" for c in CASES])
@pytest.mark.parametrize("batch", [1, 5, 64])
def test_extract_ocr_equals_reference_capture(case, batch, tmp_path):
    made = []

    def factory(cache_dir):
        made.append(ScriptedReader(case["seed"]))
        return made[-1]

    mm = ModelManager(cache_dir=str(tmp_path), frame_source=lambda p: ScriptedSource(case["fps"], case["total_frames"]),
                      ocr_reader_factory=factory, batch_size=batch)
    got = asyncio.run(mm.extract_ocr("/videos/fake.mp4", dict(case["config"])))
    assert got == case["result"]
    assert json.dumps(got) == json.dumps(case["result"])
    assert made[0].frames == [c["frame_index"] for c in case["reader_calls"] if "frame_index" in c]
    assert made[0].closed and all(b <= batch for b in made[0].batches)


def test_extract_ocr_refuses_other_languages(tmp_path):
    mm = ModelManager(cache_dir=str(tmp_path), frame_source=lambda p: ScriptedSource(30, 10),
                      ocr_reader_factory=lambda cd: ScriptedReader(1))
    with pytest.raises(ValueError, match="supported"):
        asyncio.run(mm.extract_ocr("/v.mp4", {"language": "ch_sim"}))
    with pytest.raises(ValueError, match="supported"):
        asyncio.run(mm.extract_ocr("/v.mp4", {"languages": ["en", "ja"]}))


def test_missing_weights_raise_without_a_seed(tmp_path):
    with pytest.raises(FileNotFoundError, match="craft_mlt_25k"):
        ocr.OcrReader.from_cache(tmp_path)


def test_ocr_task_is_opt_in(tmp_path, monkeypatch):
    case = CASES[1]
    monkeypatch.setenv("MODEL_CACHE_DIR", str(tmp_path))
    sink = []
    ctx = {"artifact_sink": sink.extend,
           "model_manager_factory": lambda cache_dir: ModelManager(
               cache_dir=cache_dir, frame_source=lambda p: ScriptedSource(case["fps"], case["total_frames"]),
               ocr_reader_factory=lambda cd: ScriptedReader(case["seed"]))}
    with pytest.raises(RuntimeError, match="outside the MI355X hot path"):
        asyncio.run(task_handler.process_ml_task(ctx, "t1", "ocr", "vid", "/videos/fake.mp4", dict(case["config"])))
    ctx["gpu_ocr"] = True
    out = asyncio.run(task_handler.process_ml_task(ctx, "t2", "ocr", "vid", "/videos/fake.mp4", dict(case["config"])))
    dets = case["result"]["detections"]
    assert out == {"task_id": "t2", "status": "completed", "artifact_count": len(dets)}
    assert [e.artifact_type for e in sink] == ["ocr.text"] * len(dets)
    for e, d in zip(sink, dets):
        assert e.span_start_ms == e.span_end_ms == d["timestamp_ms"] and json.loads(e.payload_json) == d


# ---- the oracle's CRAFT against EasyOCR's module structure ----------------------------------------------------------
def _easyocr_craft():
    """craft.CRAFT as EasyOCR builds it: torchvision's vgg16_bn ``features`` ([Conv, BN, ReLU(inplace=True)] per conv,
    MaxPool per 'M'), sliced at 12 / 19 / 29 / 39 and kept under their original indices, slice5, the U-Net and conv_cls.
    The in-place ReLUs that open slices 2-4 rewrite the tensors CRAFT saved for its skips."""
    nn = torch.nn
    feats, cin = [], 3
    for v in [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]:
        if v == "M":
            feats.append(nn.MaxPool2d(2, 2))
        else:
            feats += [nn.Conv2d(cin, v, 3, padding=1), nn.BatchNorm2d(v), nn.ReLU(inplace=True)]
            cin = v

    def sl(a, b):
        s = nn.Sequential()
        for i in range(a, b):
            s.add_module(str(i), feats[i])
        return s

    class double_conv(nn.Module):
        def __init__(self, i, m, o):
            super().__init__()
            self.conv = nn.Sequential(nn.Conv2d(i + m, m, 1), nn.BatchNorm2d(m), nn.ReLU(inplace=True),
                                      nn.Conv2d(m, o, 3, padding=1), nn.BatchNorm2d(o), nn.ReLU(inplace=True))

        def forward(self, x):
            return self.conv(x)

    class Basenet(nn.Module):
        def __init__(self):
            super().__init__()
            self.slice1, self.slice2, self.slice3, self.slice4 = sl(0, 12), sl(12, 19), sl(19, 29), sl(29, 39)
            self.slice5 = nn.Sequential(nn.MaxPool2d(3, 1, 1), nn.Conv2d(512, 1024, 3, padding=6, dilation=6), nn.Conv2d(1024, 1024, 1))

        def forward(self, x):
            h = self.slice1(x)
            h_relu2_2 = h
            h = self.slice2(h)
            h_relu3_2 = h
            h = self.slice3(h)
            h_relu4_3 = h
            h = self.slice4(h)
            h_relu5_3 = h
            h = self.slice5(h)
            return h, h_relu5_3, h_relu4_3, h_relu3_2, h_relu2_2

    class Craft(nn.Module):
        def __init__(self):
            super().__init__()
            self.basenet = Basenet()
            self.upconv1, self.upconv2 = double_conv(1024, 512, 256), double_conv(512, 256, 128)
            self.upconv3, self.upconv4 = double_conv(256, 128, 64), double_conv(128, 64, 32)
            self.conv_cls = nn.Sequential(nn.Conv2d(32, 32, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(32, 32, 3, padding=1),
                                          nn.ReLU(inplace=True), nn.Conv2d(32, 16, 3, padding=1), nn.ReLU(inplace=True),
                                          nn.Conv2d(16, 16, 1), nn.ReLU(inplace=True), nn.Conv2d(16, 2, 1))

        def forward(self, x):
            s = self.basenet(x)
            y = self.upconv1(torch.cat([s[0], s[1]], 1))
            y = F.interpolate(y, size=s[2].size()[2:], mode="bilinear", align_corners=False)
            y = self.upconv2(torch.cat([y, s[2]], 1))
            y = F.interpolate(y, size=s[3].size()[2:], mode="bilinear", align_corners=False)
            y = self.upconv3(torch.cat([y, s[3]], 1))
            y = F.interpolate(y, size=s[4].size()[2:], mode="bilinear", align_corners=False)
            y = self.upconv4(torch.cat([y, s[4]], 1))
            return self.conv_cls(y).permute(0, 2, 3, 1)

    return Craft()


def test_oracle_craft_equals_easyocr_module_structure():
    import ocr_oracle

    sd = ocr.random_craft_state(5)
    net = _easyocr_craft().eval()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((1, 3, 64, 96)).astype(np.float32))
    with torch.no_grad():
        ref = net(x.clone())
        got = ocr_oracle.craft(sd, x)
    assert got.shape == ref.shape == (1, 32, 48, 2)
    assert torch.allclose(got, ref, atol=1e-4, rtol=1e-4)


def test_det_boxes_from_the_binary_map_equal_the_link_map_route():
    text, link = planted()
    text[10:20, 10:40] = 0.9
    link[15:25, 38:50] = 0.9  # a link bridge: link-only pixels removed before the box fit
    text[10:20, 48:70] = 0.8
    binm = ((text > 0.4) | (link > 0.4)).astype(np.uint8)
    a = [b.tolist() for b in ocr.det_boxes(text, link)]
    assert a == [b.tolist() for b in ocr.det_boxes(text, None, binmap=binm)] and len(a) == 1
