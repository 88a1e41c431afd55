"""GPU: K28 (csrc/mjpeg.hip) against the decode oracle and against Pillow's committed pixels, with no tolerance: the
coefficient stage, BGR / RGB / LUMA output, the synchronisation rounds, the independence of the result from the
subsequence size and from the sub-batch split; then Motion-JPEG in AVI through ModelManager's wired frame loops."""
import asyncio
import json

import numpy as np
import pytest

import jpeg_decode_oracle as jd
import mjpeg_cases as mc
from eioku_amd import mjpeg as M
from eioku_amd._buffers import on_device
from eioku_amd._lib import EiokuHipError

pytestmark = pytest.mark.gpu


def _names(size, sampling):
    """Every case of one geometry: 8 encoded files, the DHT-stripped one, and the restart-per-row one where it exists."""
    out = [mc.name_of(size, c, sampling, v) for c in mc.CONTENTS for v in ("q75", "q100", "q20opt", "q90rst")]
    out.append(mc.name_of(size, "noise", sampling, "q75", stripped=True))
    if (size, "noise", sampling, "q75rows") in mc.ENCODED:
        out.append(mc.name_of(size, "noise", sampling, "q75rows"))
    return out


def test_the_geometries_cover_every_case():
    assert sorted(n for size in mc.SIZES for s in mc.SAMPLINGS for n in _names(size, s)) == sorted(mc.NAMES)


@pytest.mark.parametrize("sampling", mc.SAMPLINGS)
@pytest.mark.parametrize("size", mc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_case_equals_the_oracle(gpu, size, sampling):
    """Three frames per call, each with its own quality and tables: coefficients, BGR, RGB and LUMA, bit for bit."""
    names = _names(size, sampling)
    names += names[:-len(names) % 3]
    dec = M.MjpegDecoder()
    try:
        for lo in range(0, len(names), 3):
            trio = names[lo:lo + 3]
            files = [mc.files()[n] for n in trio]
            want = [mc.oracle(n) for n in trio]
            assert np.array_equal(dec.coefficients(files), np.stack([o["coef"] for o in want])), trio
            rgb = dec.decode(files, "rgb").cpu().numpy()
            assert np.array_equal(rgb, np.stack([o["rgb"] for o in want])), trio
            assert np.array_equal(dec.decode(files, "bgr").cpu().numpy(), rgb[..., ::-1]), trio
            assert np.array_equal(dec.decode(files, "luma").cpu().numpy(), np.stack([o["luma"] for o in want])), trio
    finally:
        dec.close()


def test_output_equals_the_committed_pillow_pixels(gpu):
    for name, ref in mc.pillow_pixels().items():
        dec = M.MjpegDecoder()
        got = dec.decode([mc.files()[name]], "rgb" if ref.ndim == 3 else "luma").cpu().numpy()[0]
        dec.close()
        assert np.array_equal(got, ref), name


TRIO = ["40x56-noise-444-q75", "40x56-noise-444-q100", "40x56-noise-444-q20opt"]


def test_subsequence_size_does_not_change_a_byte_and_the_rounds_are_the_oracles(gpu):
    files = [mc.files()[n] for n in TRIO]
    dec = M.MjpegDecoder()
    try:
        default = dec.decode(files, "bgr").cpu().numpy()
        coef = dec.coefficients(files)
        rounds_default = dec.last()["rounds"]
        for bits in (32, 256, 4096):
            dec.set_subseq_bits(bits)
            assert np.array_equal(dec.decode(files, "bgr").cpu().numpy(), default), bits
            assert np.array_equal(dec.coefficients(files), coef), bits
            assert dec.last()["rounds"] == jd.sync_rounds(files, bits), bits
            if bits == 32:
                assert dec.last()["rounds"] >= 2, "the fixed-point loop ran"
        assert rounds_default == jd.sync_rounds(files, M.DEFAULT_SUBSEQ_BITS)
        for bits in (0, 16, 48, 8192):
            with pytest.raises(EiokuHipError, match="multiple of 32"):
                dec.set_subseq_bits(bits)
        assert np.array_equal(dec.decode(files, "bgr").cpu().numpy(), default)  # the handle is still usable
    finally:
        dec.close()


def test_large_frame_many_subsequences_and_workgroups(gpu):
    """94x95 at quality 100 is the largest stream of the case list: at S = 32 it spans several workgroups per frame."""
    names = ["94x95-noise-420-q100", "94x95-noise-420-q75rows", "94x95-noise-420-q90rst"]
    files = [mc.files()[n] for n in names]
    dec = M.MjpegDecoder(subseq_bits=32)
    try:
        assert np.array_equal(dec.decode(files, "rgb").cpu().numpy(), np.stack([mc.oracle(n)["rgb"] for n in names]))
        assert dec.last()["rounds"] == jd.sync_rounds(files, 32)
    finally:
        dec.close()


@pytest.mark.parametrize("sampling", mc.SAMPLINGS)
def test_restart_and_restartless_variants_agree(gpu, sampling):
    for size in ((33, 47), (94, 95)):
        a, b = (mc.files()[mc.name_of(size, "noise", sampling, v)] for v in ("q75", "q75rows"))
        assert b"\xff\xdd" in b and b"\xff\xdd" not in a
        dec = M.MjpegDecoder()
        out = dec.decode([a, b], "bgr").cpu().numpy()
        dec.close()
        assert np.array_equal(out[0], out[1])


def test_sub_batch_split_does_not_change_the_output(gpu):
    names = _names((33, 47), "420")[:7]
    files = [mc.files()[n] for n in names]
    dec = M.MjpegDecoder()
    try:
        whole = dec.decode(files, "bgr").cpu().numpy()
        coef = dec.coefficients(files)
        for per in (1, 3):
            dec.set_batch_frames(per)
            assert np.array_equal(dec.decode(files, "bgr").cpu().numpy(), whole), per
            assert np.array_equal(dec.coefficients(files), coef), per
        assert np.array_equal(whole, np.stack([mc.oracle(n)["rgb"][..., ::-1] for n in names]))
    finally:
        dec.close()


def test_limits_are_refused_before_the_device_and_geometry_is_fixed(gpu):
    files = [mc.files()[n] for n in TRIO]
    dec = M.MjpegDecoder()
    try:
        entropy, seg, qtab, huff, comp = M.pack([M.parse_jpeg(f) for f in files])
        status = np.zeros(3, np.int32)
        bad_seg = seg.copy()
        bad_seg[1, 4] = 8 * entropy.size  # a bit length that leaves the buffer
        import torch

        from eioku_amd._buffers import ptr

        out = torch.zeros(3 * 64 * 64 * 3, dtype=torch.uint8, device=gpu)  # room for every geometry below that is no limit error
        for args, message in (((entropy, seg, 3, 56, 9000, 3, 1, 1), "outside"), ((entropy, seg, 3, 56, 40, 3, 1, 2), "sampling"),
                              ((entropy, seg, 3, 56, 48, 3, 1, 1), "MCUs"), ((entropy, bad_seg, 3, 56, 40, 3, 1, 1), "bits at byte")):
            e, s, n, h, w, nc, hs, vs = args
            rc = dec._h.eioku_mjpeg_decode(ptr(e), e.size, ptr(s), len(s), ptr(qtab), ptr(huff), ptr(comp), n, h, w, nc, hs, vs, 0, ptr(out),
                                           ptr(status), None)
            assert rc == -1, message
            with pytest.raises(EiokuHipError, match=message):
                dec._h.check(rc, "eioku_mjpeg_decode")
        want = np.stack([mc.oracle(n)["rgb"] for n in TRIO])
        assert np.array_equal(dec.decode(files, "rgb").cpu().numpy(), want)
        with pytest.raises(RuntimeError, match="departs from the source"):
            dec.decode([mc.files()["33x47-noise-444-q75"]])
    finally:
        dec.close()


# ---- end to end ------------------------------------------------------------------------------------------------------
def _clip():
    """12 frames of 64 x 96 (h x w) with a cut after frame 5, as BGR."""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:64, 0:96]
    a = np.stack([xx * 2, yy * 3, (xx + yy)], -1)
    b = np.stack([255 - yy * 3, 200 - xx, 255 - (xx + yy)], -1)
    return np.stack([np.clip((a if i < 6 else b) + 3 * i + rng.integers(-4, 5, (64, 96, 3)), 0, 255).astype(np.uint8) for i in range(12)])


@pytest.fixture(scope="module")
def clips(gpu, tmp_path_factory):
    """The clip as a Motion-JPEG AVI (frames coded by K18, the project's own encoder) and as an .npy clip of the
    oracle-decoded frames."""
    from eioku_amd.thumbs import ThumbnailEncoder

    d = tmp_path_factory.mktemp("mjpeg")
    enc = ThumbnailEncoder((320, 180), 85)  # 96 x 64 fits the box: the frames keep their size
    jpegs = enc.encode(_clip())
    enc.close()
    (d / "clip.avi").write_bytes(mc.avi_bytes(jpegs, 25, 1, 96, 64, awkward=True))
    decoded = np.stack([jd.decode(j, "bgr") for j in jpegs])
    assert decoded.shape == (12, 64, 96, 3)
    np.save(d / "clip.npy", decoded)
    (d / "clip.npy.json").write_text(json.dumps({"fps": 25.0, "time_base": [1, 25], "duration": 12 / 25}))
    return str(d / "clip.avi"), str(d / "clip.npy"), jpegs, decoded


def test_read_and_luma_planes_of_the_avi(gpu, clips):
    avi, _, jpegs, decoded = clips
    from eioku_amd.frames import open_video

    src = open_video(avi)
    assert isinstance(src, M.MjpegSource) and src.total_frames == 12 and src.fps == 25.0
    assert src.grab() and src.grab()
    ok, frame = src.read()
    assert ok and isinstance(frame, np.ndarray) and np.array_equal(frame, decoded[2])
    assert np.array_equal(src.luma_planes(3, 5), np.stack([jd.decode(j, "luma") for j in jpegs[3:8]]))
    src.release()


def test_detection_and_scenes_on_the_avi_equal_the_npy_clip(gpu, clips, tmp_path):
    from eioku_amd.model_manager import ModelManager

    avi, npy, _, _ = clips
    mm = ModelManager(cache_dir=str(tmp_path / "m"), random_init_seed=7, batch_size=4)
    cfg = {"frame_interval": 0.08, "confidence_threshold": 0.05}
    a, b = (asyncio.run(mm.detect_objects(p, cfg)) for p in (avi, npy))
    assert a == b and {d["frame_index"] for d in a["detections"]} <= set(range(0, 12, 2))
    content = {"detector": "content", "min_scene_len": 2}
    a, b = (asyncio.run(mm.detect_scenes(p, content)) for p in (avi, npy))
    assert a == b and len(a["scenes"]) == 2
    a, b = (asyncio.run(mm.detect_scenes(p, {"threshold": 0.2})) for p in (avi, npy))
    assert a == b and a["scenes"][-1]["scene_index"] == 1 and a["scenes"][-1]["start_ms"] == 240  # one cut, at frame 6
    both = asyncio.run(mm.analyze_video(avi, {"object_detection": cfg, "scene_detection": content}))
    assert both == asyncio.run(mm.analyze_video(npy, {"object_detection": cfg, "scene_detection": content}))


def test_wired_loops_decode_once_per_batch_and_hand_over_device_tensors(gpu, clips, tmp_path, monkeypatch):
    from eioku_amd.model_manager import ModelManager

    avi = clips[0]
    calls, seen = [], []
    decode = M.MjpegDecoder.decode

    def counting(self, frames, fmt="bgr", device=None):
        calls.append((len(frames), fmt))
        return decode(self, frames, fmt, device)

    monkeypatch.setattr(M.MjpegDecoder, "decode", counting)

    class Detector:
        names = {0: "thing"}

        def detect(self, frames, conf):
            seen.append((on_device(frames), tuple(frames.shape)))
            return [[] for _ in range(len(frames))], [0] * len(frames)

    mm = ModelManager(cache_dir=str(tmp_path / "m"), detector_factory=lambda name, cache: Detector(), batch_size=4)
    asyncio.run(mm.detect_objects(avi, {"frame_interval": 0.08}))  # every 2nd frame: 6 frames in batches of 4 and 2
    assert calls == [(4, "bgr"), (2, "bgr")] and seen == [(True, (4, 64, 96, 3)), (True, (2, 64, 96, 3))]
    calls.clear()
    asyncio.run(mm.detect_scenes(avi, {"detector": "content"}))
    assert calls == [(12, "bgr")]
    calls.clear()
    asyncio.run(mm.detect_scenes(avi, {}))
    assert calls == [(12, "luma")]
