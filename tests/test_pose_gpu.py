"""The detector's Pose head on the device: the keypoint branch's maps against the fp16 oracle network, K6p against its
numpy restatement on identical maps, and ``detect(with_kpts=True)`` against ``detect()``."""
import numpy as np
import pytest

import pose_oracle as po
import wellcond
from eioku_amd import detect as D, weights as W
from oracle import yolo as oy
from test_yolo_gpu import BOX_RTOL, _check_heads, _dev, _random_heads, _stable

pytestmark = pytest.mark.gpu


# (the last case is not one the issue lists: K = 6 makes c4 = 18, which the library pads to 24 channels with zero weights)
@pytest.mark.parametrize("variant,nk,n,h,w", [("n", 15, 1, 64, 96), ("n", 15, 2, 96, 160), ("s", 15, 1, 64, 64), ("n", 18, 1, 64, 64)])
def test_keypoint_maps_match_fp16_oracle_and_leave_box_and_class_maps_alone(gpu, variant, nk, n, h, w):
    import torch

    state = W.random_state(variant, 1, seed=7, nk=nk)
    det = D.Yolov8Detector(variant, 1, state)
    assert det.nk == nk and det.kpt_shape == (nk // 3, 3)
    rng = np.random.default_rng(3)
    x = np.zeros((n, h, w, 8), dtype=np.float16)
    x[..., :3] = rng.random((n, h, w, 3)).astype(np.float16)
    box, cls, kpt = det.forward_raw_pose(_dev(x, gpu))
    net = po.PoseNet(state, *W.YOLO_VARIANTS[variant], 1)
    rbox, rcls, rkpt = net.forward_pose(torch.from_numpy(x[..., :3].astype(np.float32)).permute(0, 3, 1, 2))
    assert [tuple(k.shape) for k in kpt] == [(n, h // s, w // s, nk) for s in (8, 16, 32)]
    _check_heads(kpt, rkpt, (variant, "kpt"))
    _check_heads(box, rbox, (variant, "box"))
    _check_heads(cls, rcls, (variant, "cls"))
    # the same weights without the branch: the other six maps are the same bytes, from either entry point
    plain = D.Yolov8Detector(variant, 1, {k: v for k, v in state.items() if ".cv4." not in k})
    assert plain.nk == 0 and plain.kpt_shape is None
    pbox, pcls = plain.forward_raw(_dev(x, gpu))
    box2, cls2 = det.forward_raw(_dev(x, gpu))
    for a, b, c in zip(box + cls, pbox + pcls, box2 + cls2):
        assert torch.equal(a, b) and torch.equal(a, c)
    with pytest.raises(ValueError):
        plain.forward_raw_pose(_dev(x, gpu))
    with pytest.raises(ValueError):
        plain.detect(np.zeros((1, 64, 64, 3), np.uint8), with_kpts=True)
    det.close()
    plain.close()


# 96 x 160 letterboxes by an exact factor of 4 without padding (LetterBox scales small frames up: it is not a copy), 333 x
# 517 by a fractional gain with padding, 470 x 640 is the copy mode (gain 1) with padding
@pytest.mark.parametrize("h,w,seed,mode", [(96, 160, 11, 1), (333, 517, 12, 1), (470, 640, 13, 0)],
                         ids=["gain_4_no_padding", "padded_bilinear", "padded_copy"])
def test_keypoint_decode_on_identical_maps(gpu, h, w, seed, mode):
    """K6 + K7 + K6p through the stand-alone entry on random maps: kept anchors exact, keypoints within the box bars."""
    n, nk, conf = 2, 15, 0.5
    plan = D.letterbox_plan(h, w)
    assert plan.mode == mode
    hl, wl = [plan.out_h // s for s in (8, 16, 32)], [plan.out_w // s for s in (8, 16, 32)]
    for attempt in range(8):
        box, cls = _random_heads(seed + 1000 * attempt, n, hl, wl, 1, -1.0, 1.5)
        boxes, scores = oy.decode(box, cls)
        ref = oy.non_max_suppression(boxes, scores, conf, 0.7, 300)
        if _stable(boxes, scores, conf, 0.7, 300, ref):
            break
    else:
        pytest.fail("no well-conditioned draw in 8 seeds")
    rng = np.random.default_rng(seed)
    kpt = [(2.0 * rng.standard_normal((n, a, b, nk))).astype(np.float32) for a, b in zip(hl, wl)]
    dets, counts, kpts = D.postprocess_pose([_dev(b, gpu) for b in box], [_dev(c, gpu) for c in cls], [_dev(k, gpu) for k in kpt],
                                            plan, conf, 0.7, 300)
    assert kpts.shape == (n, 300, 5, 3)
    lo = hi_x = hi_y = 0
    for i in range(n):
        k = int(counts[i])
        anchors = [a for a, *_ in ref[i]]
        assert k == len(anchors) and k > 0 and list(dets["anchor"][i, :k]) == anchors
        want = po.kpts_decode(kpt, anchors, i, (plan.out_h, plan.out_w), (h, w), np.float32(plan.gain))
        print(f"{h}x{w} image {i}: {k} detections, max |dx| {np.abs(kpts[i, :k, :, :2] - want[..., :2]).max():.3g}, "
              f"max |dconf| {np.abs(kpts[i, :k, :, 2] - want[..., 2]).max():.3g}")
        assert np.allclose(kpts[i, :k, :, :2], want[..., :2], rtol=BOX_RTOL, atol=2e-3)
        assert np.allclose(kpts[i, :k, :, 2], want[..., 2], rtol=BOX_RTOL, atol=0)
        assert not kpts[i, k:].any()
        lo += int((want[..., :2] == 0).sum())
        hi_x += int((want[..., 0] == w).sum())
        hi_y += int((want[..., 1] == h).sum())
    assert lo and hi_x and hi_y  # coordinates clamped at both edges of the frame are among the inputs
    pad = D.kpt_pad(plan)
    assert pad == tuple(float(v) for v in po.kpt_pad((plan.out_h, plan.out_w), (h, w), np.float32(plan.gain)))
    if (h, w) == (333, 517):
        assert pad[1] != plan.pad_y and 0 < abs(pad[1] - plan.pad_y) < 1  # unrounded, where scale_boxes rounds


def test_detect_with_keypoints_leaves_detections_byte_identical(gpu):
    import torch

    frames = wellcond.blob_frames(5, 3, 96, 160)
    state = wellcond.calibrated_state(frames[:1], "n", 1, seed=8, frac=0.03, conf=0.3)
    pose = W.random_state("n", 1, 8, nk=15)
    state.update({k: v for k, v in pose.items() if ".cv4." in k})
    det = D.Yolov8Detector("n", 1, state)
    for src in (frames, torch.from_numpy(frames).to(gpu)):
        d0, c0 = det.detect(src, conf=0.3)
        d1, c1, kp = det.detect(src, conf=0.3, with_kpts=True)
        assert c0.sum() > 0 and np.array_equal(c0, c1) and d0.tobytes() == d1.tobytes()
        assert kp.shape == (3, 300, 5, 3) and kp.dtype == np.float32
        for i, c in enumerate(c1):
            assert not kp[i, int(c):].any()
            assert np.all((kp[i, :int(c), :, 0] >= 0) & (kp[i, :int(c), :, 0] <= 160) & (kp[i, :int(c), :, 1] >= 0) & (kp[i, :int(c), :, 1] <= 96))
            assert np.all((kp[i, :int(c), :, 2] >= 0) & (kp[i, :int(c), :, 2] <= 1))  # (a sigmoid in fp32: it saturates)
    # ... and the keypoints are K6p of the raw maps at the kept anchors (frames this small are scaled up by K3 as its own
    # pass in detect() too, so the maps are the ones detect() saw)
    x, plan = D.letterbox_f16(torch.from_numpy(frames).to(gpu))
    _, _, kmaps = det.forward_raw_pose(x)
    kmaps = [k.cpu().numpy() for k in kmaps]
    for i, c in enumerate(c1):
        want = po.kpts_decode(kmaps, list(d1["anchor"][i, :int(c)]), i, (plan.out_h, plan.out_w), (96, 160), np.float32(plan.gain))
        assert np.allclose(kp[i, :int(c)], want, rtol=BOX_RTOL, atol=2e-3)
    pipe = D.PipelinedDetector(det, depth=2)
    pipe.submit(frames, conf=0.3, with_kpts=True)
    pipe.submit(frames, conf=0.3)
    d2, c2, f2, k2 = pipe.result_with_frames_and_kpts()
    assert np.array_equal(c2, c1) and np.array_equal(k2, kp)
    assert all(d2[i, :int(c)].tobytes() == d1[i, :int(c)].tobytes() for i, c in enumerate(c1))  # (the lanes leave unused rows as they are)
    assert tuple(f2.shape) == (3, 96, 160, 3)
    with pytest.raises(ValueError):
        pipe.result_with_kpts()
    d3, c3 = pipe.result()
    assert np.array_equal(c3, c1)
    pipe.close()
