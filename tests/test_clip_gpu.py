"""K26 on the device against tests/clip_oracle.py (the CPU oracle; transformers is not needed here).

Configurations, the smallest at which each kernel can still go wrong:
  VS   image 64, patch 32 (5 tokens: below one MFMA tile), hidden 128 (2 heads), 2 layers, ffn 256, projection 64, quick_gelu,
       3 images
  V14  image 56, patch 14 (K 588 padded to 608; 17 tokens: one past a 16-query tile), 1 layer, gelu
  VW   the base width: image 224, patch 16 (197 tokens: two LDS stages, a multiple of neither 16 nor 64), hidden 768, 12
       heads, ffn 3072, 2 layers, projection 512, 1 image
  TS   vocab 300, hidden 128, 2 layers, 77 positions, projection 64; 4 texts whose EOT sits at positions 2, 16, 64 and 76
       (lengths 3, 17, 65, 77: either side of the 16- and 64-query edges)
  TW   vocab 49408, hidden 512, 8 heads, ffn 2048, 2 layers, projection 512; lengths 9 and 77
"""
import asyncio
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import clip_oracle as co

pytestmark = pytest.mark.gpu

SOURCES = [(54, 96), (96, 54), (30, 40), (64, 64), (49, 97)]
EOTS = (2, 16, 64, 76)


def _device(cfg, weights):
    from eioku_amd.visual import ClipModel

    return ClipModel({k: v.numpy() for k, v in weights.items()}, co.hf_config(cfg))


def _rows16(cfg, n, seed):
    """seeded uint8 images -> fp16 patch rows (n, 1 + P, Kp), as the preprocessor would write them"""
    v = cfg["vision"]
    u8 = np.random.default_rng(seed).integers(0, 256, (n, v["image"], v["image"], 3), dtype=np.uint8)
    return co.patch_rows(co.normalise(u8), v["patch"]).astype(np.float16)


def _ids(cfg, eots, seed):
    """(len(eots), positions) ids: BOS, random ids below the EOT id, EOT at the given position, random ids after it"""
    t, eos = cfg["text"], cfg["eos_token_id"]
    ids = np.random.default_rng(seed).integers(3, eos - 1, (len(eots), t["positions"])).astype(np.int32)
    ids[:, 0] = 0
    for b, p in enumerate(eots):
        ids[b, p] = eos
    return ids


class Vision:
    """One vision test model: the device model, both oracles, and the three results on one seeded input."""

    def __init__(self, cfg, n, seed):
        self.cfg, self.weights = cfg, co.random_weights(cfg, seed)
        self.dev = _device(cfg, self.weights)
        self.o32, self.o16 = co.Oracle(cfg, self.weights, False), co.Oracle(cfg, self.weights, True)
        self.rows = _rows16(cfg, n, seed + 1)
        f32 = self.rows.astype(np.float32)
        self.h32, self.u32 = (t.numpy() for t in self.o32.vision(f32))
        self.h16, self.u16 = (t.numpy() for t in self.o16.vision(f32))
        self.unit, self.hidden = self.run(self.rows)

    def run(self, rows):
        unit, hidden = self.dev.encode_patches(torch.from_numpy(rows).cuda(), with_hidden=True)
        return unit.cpu().numpy(), hidden.cpu().numpy()


class Text:
    def __init__(self, cfg, eots, seed):
        self.cfg, self.weights = cfg, co.random_weights(cfg, seed)
        self.dev = _device(cfg, self.weights)
        self.o32, self.o16 = co.Oracle(cfg, self.weights, False), co.Oracle(cfg, self.weights, True)
        self.ids = _ids(cfg, eots, seed + 1)
        n = max(eots) + 1
        self.h32, self.u32 = (t.numpy() for t in self.o32.text(self.ids, n))
        self.h16, self.u16 = (t.numpy() for t in self.o16.text(self.ids, n))
        self.unit, self.hidden = self.dev.encode_ids(self.ids, with_hidden=True)


@pytest.fixture(scope="module")
def model_vs(gpu):
    m = Vision(co.config_vs(), 3, 11)
    yield m
    m.dev.close()


@pytest.fixture(scope="module")
def model_vw(gpu):
    m = Vision(co.config_vw(), 1, 17)
    yield m
    m.dev.close()


@pytest.fixture(scope="module")
def model_ts(gpu):
    m = Text(co.config_ts(), EOTS, 13)
    yield m
    m.dev.close()


def _drift(got, ref):
    """(mean, max) of |got - ref| as fractions of the reference RMS"""
    rms = float(np.sqrt(np.mean(np.square(ref, dtype=np.float64))))
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    return float(d.mean()) / rms, float(d.max()) / rms


def _check_drift(name, got, ref32, ref16):
    """The project's rule (tests/test_actions_gpu.py): the device may drift from the fp32 oracle by at most twice what the
    oracle's own fp16 mode does on the same input."""
    assert got.shape == ref32.shape and np.isfinite(got).all()
    bar_mean, bar_max = (2 * v for v in _drift(ref16, ref32))
    mean, mx = _drift(got, ref32)
    print(f"{name}: device drift mean {mean:.3e} max {mx:.3e} of the rms; bar (2 x CPU fp16 drift) mean {bar_mean:.3e} max {bar_max:.3e}")
    assert mean <= bar_mean and mx <= bar_max


def _check_unit(name, got, ref32, ref16):
    _check_drift(name, got, ref32, ref16)
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max() <= 1e-6


# ---- 1. preprocessing --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("patch", [32, 16])
def test_preprocess_equals_pillow_from_host_and_device(gpu, patch):
    cfg = co.config_vs()
    cfg = {**cfg, "vision": {**cfg["vision"], "patch": patch, "layers": 0}}
    dev = _device(cfg, co.random_weights(cfg, 1))
    g = np.load(Path(__file__).resolve().parent / "golden" / "clip_preproc.npz")
    try:
        for h, w in SOURCES:
            bgr, want = g[f"bgr_{h}x{w}"], g[f"u8_{h}x{w}"]
            rows_want = co.patch_rows(co.normalise(want), patch).astype(np.float16)
            for src in (bgr, torch.from_numpy(bgr).cuda()):
                rows, u8 = dev.preprocess(src)
                assert np.array_equal(u8.cpu().numpy(), want), (h, w)
                assert np.array_equal(rows.cpu().numpy().view(np.uint16), rows_want.view(np.uint16)), (h, w)
    finally:
        dev.close()


# ---- 2. drift ----------------------------------------------------------------------------------------------------------------
def test_hidden_and_vector_drift_vs(model_vs):
    """B = 2 (the model's third image is for the batch test below).  Measured values: DESIGN.md "K26"."""
    unit, hidden = model_vs.run(model_vs.rows[:2])
    _check_drift("VS hidden", hidden, model_vs.h32[:2], model_vs.h16[:2])
    _check_unit("VS unit", unit, model_vs.u32[:2], model_vs.u16[:2])


def test_hidden_and_vector_drift_v14(gpu):
    m = Vision(co.config_v14(), 2, 23)
    try:
        assert m.rows.shape == (2, 17, 608)
        _check_drift("V14 hidden", m.hidden, m.h32, m.h16)
        _check_unit("V14 unit", m.unit, m.u32, m.u16)
    finally:
        m.dev.close()


def test_hidden_and_vector_drift_vw(model_vw):
    _check_drift("VW hidden", model_vw.hidden, model_vw.h32, model_vw.h16)
    _check_unit("VW unit", model_vw.unit, model_vw.u32, model_vw.u16)


def test_hidden_and_vector_drift_ts(model_ts):
    assert model_ts.hidden.shape == (4, 77, 128)
    _check_drift("TS hidden", model_ts.hidden, model_ts.h32, model_ts.h16)
    _check_unit("TS unit", model_ts.unit, model_ts.u32, model_ts.u16)


def test_hidden_and_vector_drift_tw(gpu):
    m = Text(co.config_tw(), (8, 76), 29)
    try:
        _check_drift("TW hidden", m.hidden, m.h32, m.h16)
        _check_unit("TW unit", m.unit, m.u32, m.u16)
    finally:
        m.dev.close()


# ---- 3. the embedding alone ----------------------------------------------------------------------------------------------------
def test_embedding_alone_vw_and_ts(gpu, model_vw, model_ts):
    """Zero-layer handles with VW's and TS's embedding weights: hidden_out is the embedding (after pre_layrnorm for the
    image), so a token-order or position error shows on its own."""
    cfg = co.config_vw(layers=0)
    weights = {k: v for k, v in model_vw.weights.items() if "vision_model.encoder.layers." not in k}
    dev = _device(cfg, weights)
    try:
        unit, hidden = dev.encode_patches(torch.from_numpy(model_vw.rows).cuda(), with_hidden=True)
        f32 = model_vw.rows.astype(np.float32)
        h32, u32 = (t.numpy() for t in co.Oracle(cfg, weights, False).vision(f32))
        h16, u16 = (t.numpy() for t in co.Oracle(cfg, weights, True).vision(f32))
        _check_drift("VW embedding", hidden.cpu().numpy(), h32, h16)
        _check_unit("VW embedding unit", unit.cpu().numpy(), u32, u16)
    finally:
        dev.close()
    cfg = co.config_ts(layers=0)
    weights = {k: v for k, v in model_ts.weights.items() if "text_model.encoder.layers." not in k}
    dev = _device(cfg, weights)
    try:
        unit, hidden = dev.encode_ids(model_ts.ids, with_hidden=True)
        h32, u32 = (t.numpy() for t in co.Oracle(cfg, weights, False).text(model_ts.ids))
        # the embedding is a sum of two fp32 table rows: exact on the device and in both oracle modes
        assert np.array_equal(hidden.view(np.uint32), h32.view(np.uint32))
        h16, u16 = (t.numpy() for t in co.Oracle(cfg, weights, True).text(model_ts.ids))
        _check_unit("TS embedding unit", unit, u32, u16)
    finally:
        dev.close()


# ---- 4. causality and padding ------------------------------------------------------------------------------------------------
def test_ids_after_eot_do_not_matter(model_ts):
    ids = model_ts.ids.copy()
    rng = np.random.default_rng(5)
    for b, p in enumerate(EOTS):
        ids[b, p + 1:] = rng.integers(3, 290, 76 - p)
    unit, hidden = model_ts.dev.encode_ids(ids, with_hidden=True)
    assert not np.array_equal(ids, model_ts.ids)
    assert np.array_equal(unit.view(np.uint32), model_ts.unit.view(np.uint32))
    for b, p in enumerate(EOTS):
        assert np.array_equal(hidden[b, :p + 1].view(np.uint32), model_ts.hidden[b, :p + 1].view(np.uint32))


def test_a_text_alone_at_its_own_n_equals_the_mixed_batch(model_ts):
    for b, p in enumerate(EOTS):
        unit, hidden = model_ts.dev.encode_ids(model_ts.ids[b:b + 1], with_hidden=True)
        assert hidden.shape == (1, p + 1, 128)  # only eot + 1 positions were run
        assert np.array_equal(unit[0].view(np.uint32), model_ts.unit[b].view(np.uint32))
        assert np.array_equal(hidden[0].view(np.uint32), model_ts.hidden[b, :p + 1].view(np.uint32))


def test_an_image_does_not_depend_on_its_batch(model_vs):
    for i in range(3):
        unit, hidden = model_vs.run(model_vs.rows[i:i + 1])
        assert np.array_equal(unit[0].view(np.uint32), model_vs.unit[i].view(np.uint32))
        assert np.array_equal(hidden[0].view(np.uint32), model_vs.hidden[i].view(np.uint32))


# ---- 5. both EOT rules ---------------------------------------------------------------------------------------------------------
def test_both_eot_rules_on_the_device(gpu, model_ts):
    """eos_token_id == 2: the pooled row is the largest id's, here at a non-final position with EOT-looking ids after it; the
    general rule: the first position holding eos_token_id, with a second one later.  Each against the oracle."""
    cfg = co.config_ts(eos_token_id=2)
    ids = np.random.default_rng(3).integers(3, 290, (3, 77)).astype(np.int32)
    ids[:, 0] = 0
    for b, p in enumerate((5, 40, 70)):
        ids[b, p] = 298
    ids[:, 72] = 2  # the id 2 itself is not what the legacy rule looks for
    m = _device(cfg, model_ts.weights)
    try:
        assert co.eot_positions(ids, 2).tolist() == [5, 40, 70]
        unit, hidden = m.encode_ids(ids, with_hidden=True)
        assert hidden.shape == (3, 71, 128)
        o32, o16 = co.Oracle(cfg, model_ts.weights, False), co.Oracle(cfg, model_ts.weights, True)
        _check_unit("TS legacy EOT unit", unit, o32.text(ids, 71)[1].numpy(), o16.text(ids, 71)[1].numpy())
    finally:
        m.close()
    ids = model_ts.ids[:2].copy()
    ids[0, 30] = ids[1, 50] = 299  # a second EOT after the first
    unit = model_ts.dev.encode_ids(ids)
    assert co.eot_positions(ids, 299).tolist() == [2, 16]
    _check_unit("TS first-EOT unit", unit, model_ts.o32.text(ids, 17)[1].numpy(), model_ts.o16.text(ids, 17)[1].numpy())
    assert np.array_equal(unit.view(np.uint32), model_ts.dev.encode_ids(model_ts.ids[:2]).view(np.uint32))


# ---- 6. retrieval end to end ---------------------------------------------------------------------------------------------------
RETRIEVAL_SEED = 6  # chosen on the CPU: gap 5.7e-3 against an fp16-oracle drift of 1.8e-4
QUERY = "a red car by the lake"


def _retrieval_cache(root):
    """``<cache>/clip/tiny``: VS's vision and TS's text tower, and a vocabulary of lower-case letters (with and without
    ``</w>``), a few merges, BOS and EOT; no weights (they are seeded)."""
    letters = [chr(c) for c in range(ord("a"), ord("z") + 1)]
    merges = [("t", "h"), ("th", "e</w>"), ("c", "a"), ("ca", "r</w>"), ("r", "e"), ("re", "d</w>"), ("l", "a"), ("la", "k"),
              ("lak", "e</w>"), ("b", "y</w>")]
    tokens = letters + [c + "</w>" for c in letters] + [a + b for a, b in merges] + ["<|startoftext|>", "<|endoftext|>"]
    vocab = {t: i for i, t in enumerate(tokens)}
    cfg = co.config_vs_ts()
    cfg["eos_token_id"] = vocab["<|endoftext|>"]
    d = root / "clip" / "tiny"
    d.mkdir(parents=True)
    (d / "config.json").write_text(json.dumps(co.hf_config(cfg)))
    (d / "preprocessor_config.json").write_text(json.dumps({"size": {"shortest_edge": 64}, "crop_size": {"height": 64, "width": 64},
                                                           "resample": 3}))
    (d / "vocab.json").write_text(json.dumps(vocab))
    (d / "merges.txt").write_text("#version: 0.2\n" + "\n".join(f"{a} {b}" for a, b in merges) + "\n")
    return cfg


def _retrieval_frames(seed=RETRIEVAL_SEED):
    """40 frames of 48 x 64: a coarse random colour layout each (so that the frames differ in what they show) plus noise"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 256, (40, 3, 4, 3)).astype(np.float64)
    frames = np.kron(coarse, np.ones((1, 16, 16, 1))) + rng.normal(0, 20, (40, 48, 64, 3))
    return np.clip(frames, 0, 255).astype(np.uint8)


def test_retrieval_end_to_end(gpu, tmp_path):
    """Frames through ``embed_frames`` and the ``frame_embedding`` task into the store, then queries by image and in words.
    The text ranking is only meaningful while the oracle's six best cosines are further apart than the device may drift, so
    that condition is asserted, not assumed (the seed was chosen on the CPU so that it holds)."""
    from eioku_amd import task_handler, visual
    from eioku_amd.frames import NpyFrameSource
    from eioku_amd.model_manager import ModelManager
    from eioku_amd.semantic import VectorStore

    cfg = _retrieval_cache(tmp_path / "cache")
    frames = _retrieval_frames()
    np.save(tmp_path / "clip.npy", frames)
    np.save(tmp_path / "other.npy", frames[::-1][:10])
    mm = ModelManager(cache_dir=str(tmp_path / "cache"), frame_source=NpyFrameSource, batch_size=16, random_init_seed=RETRIEVAL_SEED)
    config = {"model_name": "tiny", "frame_interval": 0.01}  # 30 fps: every frame
    out = asyncio.run(mm.embed_frames(str(tmp_path / "clip.npy"), config))
    emb = np.asarray([e["embedding"] for e in out["embeddings"]], np.float32)
    assert [e["frame_index"] for e in out["embeddings"]] == list(range(40)) and emb.shape == (40, 64)
    assert out["embeddings"][7]["timestamp_ms"] == int(7 / 30.0 * 1000)
    # the oracle on its own preprocessing and on the product's token ids (pinned against transformers on the host)
    state = visual.random_state(co.hf_config(cfg), RETRIEVAL_SEED)
    o32 = co.Oracle(cfg, state, False)
    rows = co.patch_rows(co.preprocess(frames, 64, 64)[1], 32).astype(np.float16).astype(np.float32)
    frames32 = o32.vision(rows)[1].numpy()
    clip = visual.ClipModel.from_cache(tmp_path / "cache", "tiny", seed=RETRIEVAL_SEED)
    try:
        engine = visual.VisualSearchEngine(clip, VectorStore(d=clip.projection_dim))
        ctx = {"model_manager_factory": lambda cache_dir: mm, "visual_search_engine": engine}
        for video, path in (("v1", "clip.npy"), ("v2", "other.npy"), ("v1", "clip.npy")):  # v1 twice: rows are replaced
            res = asyncio.run(task_handler.process_ml_task(ctx, "t", "frame_embedding", video, str(tmp_path / path), config))
            assert res["artifact_count"] == (40 if video == "v1" else 10)
        assert len(engine.store) == 50
        assert np.array_equal(engine.store.matrix()[10:], emb)  # the task indexed what embed_frames returns
        # by image: an indexed frame comes back first
        hit = engine.search_by_image(frames[23], filters={"video_id": "v1"}, top_k=3)
        assert hit[0]["frame_index"] == 23 and hit[0]["video_id"] == "v1" and abs(hit[0]["relevance_score"] - 1.0) <= 1e-3
        assert hit[0]["timestamp_ms"] == int(23 / 30.0 * 1000) and hit[1]["relevance_score"] < 0.999
        # in words
        ids, lengths = clip.tokenizer.encode([QUERY])
        assert lengths[0] == 8 and ids[0, 7] == cfg["eos_token_id"]  # BOS a red car by the lake EOT
        cos32 = frames32 @ o32.text(ids)[1].numpy()[0]
        got = engine.search(QUERY, filters={"video_id": "v1"}, top_k=40)
        assert len(got) == 40 and all(r["video_id"] == "v1" for r in got)
        cos_dev = np.empty(40)
        for r in got:
            cos_dev[r["frame_index"]] = r["relevance_score"]
        drift = float(np.abs(cos_dev - cos32).max())
        top6 = np.sort(cos32)[::-1][:6]
        gap = float(np.min(top6[:-1] - top6[1:]))
        print(f"retrieval: max cosine drift {drift:.3e}, smallest gap among the oracle's six best cosines {gap:.3e}; "
              f"device ms {clip.last_ms()}")
        assert gap > 4 * drift
        assert [r["frame_index"] for r in got[:5]] == np.argsort(-cos32, kind="stable")[:5].tolist()
        # both videos hold these frames; the filter keeps one
        both = engine.search(QUERY, top_k=50)
        assert len(both) == 50 and {r["video_id"] for r in both} == {"v1", "v2"}
        only = engine.search(QUERY, filters={"video_id": "v2"}, top_k=50)
        assert len(only) == 10 and all(r["video_id"] == "v2" for r in only)
    finally:
        clip.close()


# ---- 7. limits -----------------------------------------------------------------------------------------------------------------
def test_limits_and_handle_lifecycle(gpu):
    from eioku_amd._handle import Handle
    from eioku_amd._lib import EiokuHipError

    def create(image=64, patch=32, vh=128, vl=1, vheads=2, vffn=256, vocab=300, positions=77, th=128, tl=1, theads=2, tffn=256, proj=64,
               eps=1e-5, act=0):
        return Handle("clip", image, patch, vh, vl, vheads, vffn, vocab, positions, th, tl, theads, tffn, proj, eps, act)

    for kw, match in [({"vheads": 4}, "vision head_dim must be 64"), ({"theads": 1}, "text head_dim must be 64"),
                      ({"image": 60}, "must be a multiple of patch_size"), ({"image": 480, "patch": 32}, r"image_size must be in \[1, 448\]"),
                      ({"positions": 78}, r"max_position_embeddings must be in \[1, 77\]"), ({"act": 2}, "bad config")]:
        with pytest.raises(EiokuHipError, match=match):
            create(**kw)
    h = create()
    names = [n for n, _, _ in h.tensors()]
    assert names == list(co.random_weights({**co.config_vs_ts(), "vision": {**co.config_vs()["vision"], "layers": 1},
                                            "text": {**co.config_ts()["text"], "layers": 1}}, 0))
    assert names[0] == "text_model.embeddings.token_embedding.weight" and names[-1] == "text_projection.weight"
    assert len(names) == 2 + 16 + 2 + 5 + 16 + 2 + 2
    shapes = dict((n, (r, c)) for n, r, c in h.tensors())
    assert shapes["vision_model.embeddings.patch_embedding.weight"] == (128, 3072)
    assert shapes["text_model.encoder.layers.0.self_attn.q_proj.weight"] == (128, 128)
    rows = torch.zeros((1, 5, 3072), dtype=torch.float16, device="cuda")
    out = torch.empty((1, 64), dtype=torch.float32, device="cuda")
    rc = h.eioku_clip_encode_patches(rows.data_ptr(), 1, out.data_ptr(), None, None)
    assert rc != 0 and b"has no weights" in h.lib.eioku_last_error()
    ids, eot, vec = np.zeros((1, 77), np.int32), np.array([3], np.int32), np.empty((1, 64), np.float32)
    rc = h.eioku_clip_encode_text(ids.ctypes.data, eot.ctypes.data, 1, 4, vec.ctypes.data, None, 0, None)
    assert rc != 0 and b"has no weights" in h.lib.eioku_last_error()
    for bad_ids, bad_eot, n, match in [(np.full((1, 77), 300, np.int32), eot, 4, b"outside the vocabulary"), (ids, np.array([4], np.int32), 4, b"eot position"),
                                       (ids, eot, 78, b"n must be in")]:
        rc = h.eioku_clip_encode_text(bad_ids.ctypes.data, bad_eot.ctypes.data, 1, n, vec.ctypes.data, None, 0, None)
        assert rc != 0 and match in h.lib.eioku_last_error()
    h.close()
    h.close()  # idempotent
    with pytest.raises(EiokuHipError, match="closed"):
        h.eioku_clip_num_tensors()
    m = _device(co.config_vs(), co.random_weights(co.config_vs(), 1))
    m.close()
    m.close()
    with pytest.raises(EiokuHipError, match="closed"):
        m.encode_ids(np.zeros((1, 77), np.int32))
