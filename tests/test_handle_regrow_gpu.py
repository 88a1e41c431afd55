"""Grow-on-demand of the handles' device buffers: one handle run at a small size, then a larger one (every buffer
regrows), then the small size again (nothing regrows, the larger buffers are reused) must give, each time, the bits of a
fresh handle that only ever saw that size.  Random-weight fixtures and helpers of each model's own GPU test; no failure
is provoked."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bits(x):
    """A result as nested tuples of bytes: tensors, arrays, structured arrays, lists of them."""
    if isinstance(x, (list, tuple)):
        return tuple(_bits(v) for v in x)
    if isinstance(x, (bytes, int, type(None))):
        return x
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    x = np.ascontiguousarray(x)
    return (x.dtype.str, x.shape, x.tobytes())


def _check_regrow(make, run, small, large):
    """make() -> handle with close(); run(handle, size) -> result."""
    fresh = {}
    for name, size in (("small", small), ("large", large)):
        h = make()
        try:
            fresh[name] = _bits(run(h, size))
        finally:
            h.close()
    assert fresh["small"] != fresh["large"]
    h = make()
    try:
        for name, size in (("small", small), ("large", large), ("small", small)):
            assert _bits(run(h, size)) == fresh[name], f"{name} run on the regrown handle differs from a fresh handle"
    finally:
        h.close()


def test_resnet18_classify(gpu):
    from oracle import places as op
    from eioku_amd import places
    from test_places_gpu import textured

    st = op.random_state(3)
    frames = textured(12, 3, 48, 64)
    _check_regrow(lambda: places.Places365Classifier(st), lambda clf, n: clf.classify(frames[:n], top_k=5, with_logits=True), 1, 3)


def test_iresnet_embed(gpu):
    from eioku_amd import faces
    from test_faces_gpu import _frames

    state = faces.fold_state(faces.random_state_dict(11, (1, 1, 1, 1)))
    frame = _frames(3, 1, 64, 64)
    boxes = [(0, 4.0, 6.0, 40.0, 50.0), (0, -10.0, -5.0, 30.0, 28.0), (0, 20.5, 10.25, 63.0, 61.5)]
    _check_regrow(lambda: faces.FaceEmbedder(state), lambda emb, m: emb.embed(frame, boxes[:m]), 1, 3)


def test_wespeaker_embed(gpu):
    import speaker_oracle as so
    from eioku_amd import speakers

    state = speakers.fold_state(speakers.random_state_dict(3, (1, 1, 1, 1)))
    f0, formants = so.VOICES[0]
    audio = so.voice(10, f0, formants, so.RATE)
    plan = [(1000, 16), (4000, 12), (9000, 9)]
    _check_regrow(lambda: speakers.SpeakerLabeller(state, win_frames=16), lambda lab, m: lab.embed_windows(audio, plan[:m]), 1, 3)


@pytest.fixture(scope="module")
def ocr_states():
    from eioku_amd import ocr

    return ocr.random_craft_state(5), ocr.random_crnn_state(6)


def test_craft_score_maps(gpu, ocr_states):
    from eioku_amd import ocr
    from eioku_amd.synth import ocr_frames

    frames = ocr_frames(11, 2, 480, 640)  # tests/test_ocr_gpu.py's smallest canvas
    _check_regrow(lambda: ocr.OcrReader(*ocr_states), lambda r, n: r.score_maps(frames[:n]), 1, 2)


def test_crnn_recognize(gpu, ocr_states):
    from eioku_amd import ocr
    from eioku_amd.synth import ocr_crops

    imgs = {1: ocr_crops(1, [128]), 3: ocr_crops(2, [64, 192, 128])}
    _check_regrow(lambda: ocr.OcrReader(*ocr_states), lambda r, m: r.recognize_raw(imgs[m], want_logits=True), 1, 3)


def test_yolo_forward_and_detect(gpu):
    import torch

    from eioku_amd import detect as D, weights as W

    state = W.random_state("n", 80, seed=1)
    rng = np.random.default_rng(4)
    frames = {(n, s): rng.integers(0, 256, (n, s, s, 3), dtype=np.uint8) for n, s in ((1, 32), (2, 64))}
    x8 = {k: torch.from_numpy(np.concatenate([f, np.zeros(f.shape[:3] + (5,), np.uint8)], -1).astype(np.float16) / 255).to(gpu)
          for k, f in frames.items()}

    def run(det, size):
        box, cls = det.forward_raw(x8[size])
        dets, counts = det.detect(frames[size], conf=0.001, imgsz=size[1])  # a low bar: random heads still give candidates
        return box, cls, dets.view(np.uint8), counts

    _check_regrow(lambda: D.Yolov8Detector("n", 80, state), run, (1, 32), (2, 64))


def test_thumbnails(gpu):
    import thumbs_cases as tc
    from eioku_amd import thumbs

    frames = {1: np.stack([tc.image("random", 120, 160, 0)]), 2: np.stack([tc.image("random", 360, 640, v) for v in range(2)])}
    _check_regrow(thumbs.ThumbnailEncoder, lambda enc, n: enc.encode(frames[n]), 1, 2)


def test_flat_index_add_and_search(gpu):
    """Rows, norms and the search workspace grow; a handle that grew answers like one that received its rows at once.
    d = 64: the smallest dimension eioku_index_flat_create accepts."""
    from eioku_amd import search
    from test_knn_gpu import unit_rows

    d = 64
    xb = unit_rows(5, 64 + 4096, d)
    q = {64: xb[[3, 40, 63]] + np.float32(0.01), 64 + 4096: unit_rows(6, 40, d)}
    fresh = {}
    for n in q:
        ix = search.IndexFlatL2(d)
        ix.add(xb[:n])
        fresh[n] = _bits(ix.search(q[n], 5))
        ix.close()
    ix = search.IndexFlatL2(d)
    ix.add(xb[:64])
    assert _bits(ix.search(q[64], 5)) == fresh[64]
    ix.add(xb[64:])  # 4160 rows: past the first allocation of 1024, the old rows are carried over
    assert ix.ntotal == 64 + 4096
    assert _bits(ix.search(q[64 + 4096], 5)) == fresh[64 + 4096]
    ix.close()


def test_bert_encode(gpu):
    from eioku_amd import embed
    from test_bert_gpu import _inputs

    cfg = dict(embed.MINILM_L6_V2, vocab=3000)
    state = embed.random_state(cfg, 3)
    inputs = {(B, S): _inputs(cfg["vocab"], B, S, B * 100 + S) for B, S in ((1, 8), (3, 16))}
    _check_regrow(lambda: embed.MiniLMEncoder(state, cfg), lambda enc, bs: enc.encode_ids(*inputs[bs]), (1, 8), (3, 16))
