"""Host side of the thumbnail path (no GPU): the numpy oracle against Pillow byte for byte, the product's tables, size rule,
frame choice and segment assignment against the oracle / brute force, the task-handler mapping, and the committed golden
file against what the generator would write today."""
import asyncio
import io
import json

import numpy as np
import pytest

import jpeg_oracle as jo
import thumbs_cases as tc
from conftest import GOLDEN
from eioku_amd import task_handler, thumbs


def pil_jpeg(rgb, q):
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=q)
    return buf.getvalue()


@pytest.mark.parametrize("case", tc.JPEG_CASES, ids=tc.case_id)
def test_oracle_file_is_pillows(case):
    content, h, w, q = case
    rgb = tc.image(content, h, w)
    enc = jo.encode(rgb, q)
    assert enc["coef"].shape == (-(-h // 16) * -(-w // 16), 6, 64)
    assert len(enc["stream"]) == (enc["nbits"] + 7) // 8
    assert jo.bitstream_slow(enc["coef"]) == (enc["stream"], enc["nbits"], enc["zrl"])  # the vectorised coder is the literal one
    assert enc["file"] == pil_jpeg(rgb, q)
    if content == "constant":  # a single colour: every AC coefficient is zero
        assert not enc["coef"][..., 1:].any()


def test_ramp_at_q95_needs_zrl_and_others_cover_the_rest():
    assert jo.encode(tc.image("ramp", 64, 64), 95)["zrl"]
    assert not jo.encode(tc.image("constant", 64, 64), 75)["zrl"]
    # the pixel-pitch checkerboard puts its energy into the last zigzag coefficient of every luma block, far beyond
    # what random bytes leave there
    last = np.abs(jo.encode(tc.image("checker", 64, 64), 95)["coef"][:, :4, 63].astype(np.int64))
    assert last.min() > np.abs(jo.encode(tc.image("random", 64, 64), 95)["coef"][..., 63].astype(np.int64)).max()


@pytest.mark.parametrize("src,dst", tc.RESIZE_CASES)
def test_oracle_resize_is_pillows(src, dst):
    Image = pytest.importorskip("PIL.Image")
    rgb = tc.image("random", *src, variant=7)
    want = np.asarray(Image.fromarray(rgb).resize((dst[1], dst[0]), Image.Resampling.BICUBIC))
    assert np.array_equal(jo.resize_bicubic(rgb, (dst[1], dst[0])), want)


@pytest.mark.parametrize("a,b", [(53, 23), (37, 16), (12, 19), (20, 32), (160, 80), (480, 320), (1920, 320), (1080, 180), (7, 7), (5, 1),
                                 (1, 5), (1000, 3)])
def test_product_tables_equal_the_oracles(a, b):
    gb, gk, gs = thumbs.bicubic_tables(a, b)
    wb, wk, ws = jo.bicubic_tables(a, b)
    assert gs == ws and np.array_equal(gb, wb) and np.array_equal(gk, wk)
    assert gb.dtype == np.int32 and gk.dtype == np.int32
    assert (gb[:, 0] >= 0).all() and (gb[:, 0] + gb[:, 1] <= a).all() and (gb[:, 1] <= gs).all()  # what the kernel relies on


def test_bilinear_sibling_equals_places_tables():
    from eioku_amd import places

    for a, b in [(1920, 224), (97, 224), (224, 224)]:
        for got, want in zip(thumbs.resample_tables(a, b, "bilinear"), places.resize_tables(a, b)):
            assert np.array_equal(got, want)


def test_product_jpeg_tables_and_file_equal_the_oracles():
    for q in (1, 30, 49, 50, 60, 75, 85, 90, 95, 100):
        tab = thumbs.jpeg_tables(q)
        assert tab.dtype == np.uint16 and tab.shape == (2, 64)
        assert np.array_equal(tab[0], jo.quant_tables(q)[0]) and np.array_equal(tab[1], jo.quant_tables(q)[1])
    for content, h, w, q in tc.GOLDEN_JPEG:
        enc = jo.encode(tc.image(content, h, w), q)
        assert thumbs.jpeg_file(enc["stream"], enc["nbits"], w, h, q) == enc["file"]
    with pytest.raises(ValueError):
        thumbs.jpeg_file(b"\x00", 17, 8, 8, 75)


SIZE_GRID = [(w, h, box) for w in (1, 2, 3, 16, 319, 320, 321, 1000, 1920, 5000) for h in (1, 5, 179, 180, 181, 1080, 4001)
             for box in ((320, 180), (64, 48), (1, 1))]


def test_thumbnail_size_is_pillows():
    Image = pytest.importorskip("PIL.Image")
    assert len(SIZE_GRID) >= 200
    for w, h, box in SIZE_GRID:
        im = Image.new("RGB", (w, h))
        im.thumbnail(box, reducing_gap=None)
        assert thumbs.thumbnail_size(w, h, box) == im.size == jo.thumbnail_size(w, h, box), (w, h, box)


def test_thumbnail_size_without_pillow():
    for w, h, box in SIZE_GRID:
        assert thumbs.thumbnail_size(w, h, box) == jo.thumbnail_size(w, h, box)
    assert thumbs.thumbnail_size(1920, 1080) == (320, 180) and thumbs.thumbnail_size(96, 128, (64, 48)) == (36, 48)
    assert thumbs.thumbnail_size(100, 50) == (100, 50)


@pytest.mark.parametrize("fps", [30.0, 29.97, 25.0])
def test_scene_frame_index(fps):
    total = 200
    stamp = [int((i / fps) * 1000) for i in range(total)]
    # the reference's scene list for cuts at 1000, 2500, 4000 ms of a 5000 ms video: no scene before the first cut and
    # the last scene's index is the number of cuts
    scenes = [{"scene_index": 0, "start_ms": 1000, "end_ms": 2500}, {"scene_index": 1, "start_ms": 2500, "end_ms": 4000},
              {"scene_index": 3, "start_ms": 4000, "end_ms": 5000}, {"scene_index": 0, "start_ms": 0, "end_ms": 5000},
              {"scene_index": 7, "start_ms": 1001, "end_ms": 1034}, {"scene_index": 8, "start_ms": 33, "end_ms": 34}]
    for sc in scenes:
        for position, target in (("start", sc["start_ms"]), ("middle", (sc["start_ms"] + sc["end_ms"]) // 2)):
            want = next(i for i, t in enumerate(stamp) if t >= target)
            assert thumbs.scene_frame_index(sc, fps, total, position) == want
    assert thumbs.scene_frame_index(scenes[0], fps, total) == thumbs.scene_frame_index(scenes[0], fps, total, "start")
    # clamp: a scene that starts at or after the last frame's timestamp
    late = {"scene_index": 4, "start_ms": 9000, "end_ms": 12000}
    assert thumbs.scene_frame_index(late, fps, total) == total - 1 == thumbs.scene_frame_index(late, fps, total, "middle")
    assert thumbs.scene_frame_index(scenes[2], fps, 100, "start") == 99
    with pytest.raises(ValueError):
        thumbs.scene_frame_index(scenes[0], fps, total, "end")


def test_assign_thumbnails():
    rows = [{"scene_index": 0, "start_ms": 1000, "end_ms": 2500, "thumbnail_path": "/t/scene_0000.jpg"},
            {"scene_index": 3, "start_ms": 4000, "end_ms": 5000, "thumbnail_path": "/t/scene_0003.jpg"},
            {"scene_index": 1, "start_ms": 2500, "end_ms": 3000, "thumbnail_path": "/t/scene_0001.jpg"}]
    segs = [{"text": "before every scene", "start_ms": 0, "end_ms": 900},
            {"text": "inside the first", "start_ms": 1000, "end_ms": 1200},
            {"text": "on a boundary", "start_ms": 2500, "end_ms": 2600},
            {"text": "in the gap", "start_ms": 3500, "end_ms": 3900},
            {"text": "seconds form", "start": 4.2, "end": 4.9},
            {"text": "after the end", "start_ms": 7000, "end_ms": 7100, "thumbnail_path": "old"}]
    out = thumbs.assign_thumbnails(segs, rows)
    assert [s["thumbnail_path"] for s in out] == ["/t/scene_0000.jpg", "/t/scene_0000.jpg", "/t/scene_0001.jpg", "/t/scene_0001.jpg",
                                                  "/t/scene_0003.jpg", "/t/scene_0003.jpg"]
    assert "thumbnail_path" not in segs[0] and segs[5]["thumbnail_path"] == "old"  # new dicts
    assert [{k: v for k, v in s.items() if k != "thumbnail_path"} for s in out[:5]] == segs[:5]
    assert thumbs.assign_thumbnails(segs[:1], []) == segs[:1]


class FakeManager:
    def __init__(self, cache_dir="/models"):
        self.calls = []

    async def generate_thumbnails(self, path, config):
        self.calls.append((path, config))
        return {"thumbnails": [{"scene_index": i, "start_ms": a, "end_ms": b, "timestamp_ms": a + 1, "frame_index": a // 40,
                                "width": 64, "height": 36, "thumbnail_path": f"/t/scene_{i:04d}.jpg", "bytes": 900 + i}
                               for i, (a, b) in ((0, (1000, 2500)), (1, (2500, 4000)), (3, (4000, 5000)))]}


def test_task_handler_maps_thumbnail_generation():
    assert task_handler.TASK_TO_ARTIFACT_TYPE["thumbnail_generation"] == "scene.thumbnail"
    assert task_handler.TASK_TO_RESULT_KEY["thumbnail_generation"] == "thumbnails"
    assert "thumbnail_generation" in task_handler.KNOWN_TASK_TYPES
    sink, made = [], []

    def factory(cache_dir):
        made.append(FakeManager(cache_dir))
        return made[-1]

    cfg = {"output_dir": "/t", "position": "middle"}
    out = asyncio.run(task_handler.process_ml_task({"artifact_sink": sink.extend, "model_manager_factory": factory}, "t1",
                                                   "thumbnail_generation", "vid9", "/v.mp4", cfg))
    assert out == {"task_id": "t1", "status": "completed", "artifact_count": 3}
    assert made[0].calls == [("/v.mp4", cfg)]
    assert [e.artifact_type for e in sink] == ["scene.thumbnail"] * 3
    assert [(e.span_start_ms, e.span_end_ms) for e in sink] == [(1000, 2500), (2500, 4000), (4000, 5000)]
    payloads = [json.loads(e.payload_json) for e in sink]
    assert [p["thumbnail_path"] for p in payloads] == ["/t/scene_0000.jpg", "/t/scene_0001.jpg", "/t/scene_0003.jpg"]
    assert set(payloads[0]) == {"scene_index", "start_ms", "end_ms", "timestamp_ms", "frame_index", "width", "height", "thumbnail_path",
                                "bytes"}


def test_generate_thumbnails_needs_an_output_dir(tmp_path):
    from eioku_amd.model_manager import ModelManager

    mm = ModelManager(cache_dir=str(tmp_path))
    with pytest.raises(ValueError, match="output_dir"):
        asyncio.run(mm.generate_thumbnails("/nowhere.npy", {"scenes": []}))


def test_golden_file_is_what_pillow_writes_today():
    """The committed Pillow bytes (what the GPU tests compare with) are the oracle's, and Pillow still writes them."""
    gold = np.load(GOLDEN / "thumbs_pillow.npz")
    for i, (content, h, w, q) in enumerate(tc.GOLDEN_JPEG):
        rgb = tc.image(content, h, w)
        assert str(gold[f"jpeg{i}_case"]) == tc.case_id((content, h, w, q))
        assert np.array_equal(gold[f"jpeg{i}_rgb"], rgb)
        assert gold[f"jpeg{i}_file"].tobytes() == jo.encode(rgb, q)["file"]
    for i, ((h, w), (th, tw)) in enumerate(tc.GOLDEN_RESIZE):
        rgb = tc.image("random", h, w, variant=7)
        assert np.array_equal(gold[f"resize{i}_rgb"], rgb)
        assert np.array_equal(gold[f"resize{i}_out"], jo.resize_bicubic(rgb, (tw, th)))
    Image = pytest.importorskip("PIL.Image")
    for i, (content, h, w, q) in enumerate(tc.GOLDEN_JPEG):
        assert gold[f"jpeg{i}_file"].tobytes() == pil_jpeg(tc.image(content, h, w), q)
    for i, ((h, w), (th, tw)) in enumerate(tc.GOLDEN_RESIZE):
        want = np.asarray(Image.fromarray(tc.image("random", h, w, variant=7)).resize((tw, th), Image.Resampling.BICUBIC))
        assert np.array_equal(gold[f"resize{i}_out"], want)
