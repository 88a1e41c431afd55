"""K26 on the host: the oracle against ``transformers.CLIPModel``, the preprocessing restatement against real Pillow, the
tokenizer against ``transformers.CLIPTokenizer``, the product's tables and config checks, and the task plumbing.  No GPU."""
import asyncio
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import clip_oracle as co
from eioku_amd import task_handler, visual
from eioku_amd.model_manager import ModelManager
from eioku_amd.semantic import VectorStore

SOURCES = [(54, 96), (96, 54), (30, 40), (64, 64), (49, 97)]


# ---- the oracle ----------------------------------------------------------------------------------------------------------
def _features(out):
    """``get_*_features`` returns the projected vectors, as a tensor or (this ``transformers``) inside an output object"""
    return out if torch.is_tensor(out) else out.pooler_output


@pytest.mark.parametrize("act,eos", [("quick_gelu", 299), ("gelu", 2)])
def test_fp32_oracle_equals_transformers(act, eos):
    """Both towers, both activations, both EOT rules (eos 299: the first position holding it, with a second one later in the
    row; eos 2: the legacy argmax rule, the largest id at a non-final position).  The bar is the 5e-5 of
    ``test_actions_host.py``: a few fp32 roundings on values of a few units, nothing a wrong token order, mask, activation or
    pooled row could meet.  Measured here: hidden <= 9e-6, unit vectors <= 5e-7."""
    tr = pytest.importorskip("transformers")
    cfg = {**co.config_vs_ts(), "act": act, "eos_token_id": eos}
    w = co.random_weights(cfg, 3)
    model = tr.CLIPModel(tr.CLIPConfig(**co.hf_config(cfg))).eval()
    res = model.load_state_dict(w, strict=False)
    assert not res.unexpected_keys and all(k == "logit_scale" or k.endswith("position_ids") for k in res.missing_keys)
    rng = np.random.default_rng(1)
    rows = co.patch_rows(rng.standard_normal((3, 64, 64, 3)).astype(np.float32), 32)
    ids = rng.integers(3, 290, (4, 77))
    ids[:, 0] = 0
    if eos == 2:
        for b, p in enumerate((2, 16, 64, 76)):
            ids[b, p] = 298  # the largest id marks the pooled row; what follows is smaller
    else:
        for b, p in enumerate((2, 16, 64, 76)):
            ids[b, p] = eos
        ids[0, 40] = eos  # a second EOT: the first one counts
    pix = torch.from_numpy(co.pixel_values(rows, 64, 32))
    tid = torch.from_numpy(ids.astype(np.int64))
    with torch.no_grad():
        vh = model.vision_model(pixel_values=pix).last_hidden_state
        vu = _features(model.get_image_features(pixel_values=pix))
        th = model.text_model(input_ids=tid).last_hidden_state
        tu = _features(model.get_text_features(input_ids=tid))
    vu, tu = vu / vu.norm(dim=-1, keepdim=True), tu / tu.norm(dim=-1, keepdim=True)
    o = co.Oracle(cfg, w, fp16=False)
    h, u = o.vision(rows)
    ht, ut = o.text(ids)
    assert co.eot_positions(ids, eos).tolist() == [2, 16, 64, 76]
    d = [(vh - h).abs().max().item(), (vu - u).abs().max().item(), (th - o.text_final(ht)).abs().max().item(),
         (tu - ut).abs().max().item()]
    print(f"{act} / eos {eos}: oracle vs transformers: vision hidden {d[0]:.3e} unit {d[1]:.3e}, text hidden {d[2]:.3e} unit {d[3]:.3e}")
    assert vh.shape == h.shape == (3, 5, 128) and th.shape == (4, 77, 128) and u.shape == (3, 64) and ut.shape == (4, 64)
    assert max(d) <= 5e-5


def test_patch_row_relayout_round_trips():
    x = np.random.default_rng(0).standard_normal((2, 56, 56, 3)).astype(np.float32)
    rows = co.patch_rows(x, 14)
    assert rows.shape == (2, 17, 608) and not rows[:, 0].any() and not rows[:, :, 588:].any()
    # patch 5 (row 1, column 1), channel 1, ky 5, kx 7
    assert rows[1, 1 + 5, 196 + 5 * 14 + 7] == x[1, 14 + 5, 14 + 7, 1]
    assert np.array_equal(co.pixel_values(rows, 56, 14), x.transpose(0, 3, 1, 2))


# ---- preprocessing ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(Path(__file__).resolve().parent / "golden" / "clip_preproc.npz")


@pytest.mark.parametrize("h,w", SOURCES)
def test_preprocessing_restatement_equals_pillow(golden, h, w):
    u8, norm = co.preprocess(golden[f"bgr_{h}x{w}"], 64, 64)
    assert np.array_equal(u8, golden[f"u8_{h}x{w}"])
    assert np.abs(norm - golden[f"norm_{h}x{w}"]).max() <= 1e-6


@pytest.mark.parametrize("h,w", SOURCES + [(1080, 1920)])
def test_image_tables_are_the_cropped_rows_of_the_full_tables(h, w):
    """The product's vectorised tables equal the oracle's scalar ones on the rows the crop keeps, and stay inside the frame."""
    crop = 64 if h < 1000 else 224
    xb, xk, kx, yb, yk, ky = visual.image_tables(h, w, crop, crop)
    assert xb.shape == yb.shape == (crop, 2) and xk.shape == (crop, kx) and yk.shape == (crop, ky)
    assert (xb[:, 0] >= 0).all() and (xb.sum(1) <= w).all() and (yb[:, 0] >= 0).all() and (yb.sum(1) <= h).all()
    rh, rw = co.resized_size(h, w, crop)
    for (b, k), size, out, off in ((((xb, xk)), w, rw, (rw - crop) // 2), ((yb, yk), h, rh, (rh - crop) // 2)):
        fb, fk = co.bicubic_coeffs(size, out)
        assert np.array_equal(b, fb[off:off + crop]) and np.array_equal(k, fk[off:off + crop])
    assert (h, w) == (64, 64) or ((xk < 0).any() and (yk < 0).any())  # bicubic: negative lobes, except at the identity


def test_image_tables_refuse_a_frame_smaller_than_the_crop_after_resize():
    assert visual.image_tables(10, 10, 64, 64)[0].shape == (64, 2)  # upscaling is fine
    with pytest.raises(ValueError, match="smaller than the 64 crop"):
        visual.image_tables(100, 100, 32, 64)


# ---- the tokenizer ---------------------------------------------------------------------------------------------------------
def _byte_chars():
    bs = list(range(33, 127)) + list(range(161, 173)) + list(range(174, 256))
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {b: chr(c) for b, c in zip(bs, cs)}


def _write_vocab(root, positions):
    """A synthetic vocabulary: every byte character with and without ``</w>``, a few merges (none produces a bare ``</w>``),
    BOS, and EOT as the last id."""
    chars = _byte_chars()
    e, smile = [chars[b] for b in "é".encode()], [chars[b] for b in "😀".encode()]
    merges = [("d", "o"), ("do", "g</w>"), ("c", "a"), ("ca", "t</w>"), ("t", "h"), ("th", "e</w>"), ("'", "s</w>"), ("c", "a"),
              ("ca", "f"), (e[0], e[1] + "</w>"), ("caf", e[0] + e[1] + "</w>"), ("!", "!</w>"), (smile[0], smile[1]),
              (smile[2], smile[3] + "</w>"), ("w", "o"), ("wo", "r"), ("wor", "d</w>"), ("o", "n</w>"), ("2", "0")]
    merges = list(dict.fromkeys(merges))
    tokens = [c for c in chars.values()] + [c + "</w>" for c in chars.values()] + [a + b for a, b in merges]
    tokens = list(dict.fromkeys(tokens)) + [visual.BOS, visual.EOT]
    vocab = {t: i for i, t in enumerate(tokens)}
    (root / "vocab.json").write_text(json.dumps(vocab), encoding="utf-8")
    (root / "merges.txt").write_text("#version: 0.2\n" + "\n".join(f"{a} {b}" for a, b in merges) + "\n", encoding="utf-8")
    (root / "tokenizer_config.json").write_text(json.dumps({"model_max_length": positions, "tokenizer_class": "CLIPTokenizer"}))
    return vocab


STRINGS = ["the dog on the cat", "the  dog\ton \t the   cat ", "The DOG On THE Cat", "DOG's café!", "in 2024 the dog", "a 😀 dog!!",
           "", " ".join(["word", "dog", "the", "cat"] * 25)]


@pytest.mark.parametrize("positions", [77, 16])
def test_tokenizer_equals_transformers(tmp_path, positions):
    tr = pytest.importorskip("transformers")
    vocab = _write_vocab(tmp_path, positions)
    assert max(vocab.values()) == vocab[visual.EOT]
    ref = tr.CLIPTokenizer.from_pretrained(str(tmp_path))
    mine = visual.ClipTokenizer(tmp_path / "vocab.json", tmp_path / "merges.txt", positions)
    want = ref(STRINGS, padding="max_length", truncation=True, max_length=positions, return_tensors="np")
    ids, lengths = mine.encode(STRINGS)
    assert ids.dtype == np.int32 and ids.shape == (len(STRINGS), positions)
    for s, a, b in zip(STRINGS, ids, want["input_ids"]):
        assert a.tolist() == b.tolist(), s
    assert lengths.tolist() == want["attention_mask"].sum(1).tolist()
    assert lengths[6] == 2 and lengths[7] == (positions if positions == 16 else 77)  # empty: BOS EOT; 100 words: truncated
    assert ids[7, -1] == vocab[visual.EOT] and ids[3].tolist() != ids[0].tolist()
    assert mine.tokens("DOG's") == [vocab["dog</w>"], vocab["'s</w>"]] and len(mine.tokens("2024")) == 4


def test_piece_pattern():
    assert visual.clip_pieces("dog's café!! 2024 x9y <|endoftext|>'ll") == ["dog", "'s", "café", "!!", "2", "0", "2", "4", "x", "9", "y",
                                                                              "<|endoftext|>", "'ll"]
    assert visual.clip_pieces("!!'s a'b") == ["!!'", "s", "a", "'", "b"]  # a run of symbols takes the apostrophe with it


# ---- configuration ---------------------------------------------------------------------------------------------------------
def test_dims_defaults_limits_and_tensor_names():
    d = visual.clip_dims({})
    assert d["vision"] == {"hidden": 768, "layers": 12, "heads": 12, "ffn": 3072, "image": 224, "patch": 32}
    assert d["text"] == {"hidden": 512, "layers": 12, "heads": 8, "ffn": 2048, "vocab": 49408, "positions": 77}
    assert (d["projection"], d["act"], d["eos_token_id"], d["ln_eps"]) == (512, "quick_gelu", 49407, 1e-5)
    hf = co.hf_config(co.config_v14())
    assert visual.clip_dims(hf)["act"] == "gelu"
    for edit, match in [({"vision_config": {**hf["vision_config"], "num_attention_heads": 4}}, "vision head dimension must be 64"),
                        ({"vision_config": {**hf["vision_config"], "image_size": 60}}, "multiple of patch_size"),
                        ({"vision_config": {**hf["vision_config"], "image_size": 462}}, "at most 448"),
                        ({"text_config": {**hf["text_config"], "max_position_embeddings": 78}}, r"in \[1, 77\]"),
                        ({"text_config": {**hf["text_config"], "hidden_act": "quick_gelu"}}, "must share hidden_act"),
                        ({"vision_config": {**hf["vision_config"], "hidden_act": "relu"},
                          "text_config": {**hf["text_config"], "hidden_act": "relu"}}, "is not built")]:
        with pytest.raises(ValueError, match=match):
            visual.clip_dims({**hf, **edit})
    tr = pytest.importorskip("transformers")
    cfg = co.config_vs_ts()
    sd = tr.CLIPModel(tr.CLIPConfig(**co.hf_config(cfg))).state_dict()
    names = [k for k in sd if k != "logit_scale" and not k.endswith("position_ids")]
    shapes = visual.tensor_shapes(visual.clip_dims(co.hf_config(cfg)))
    assert [n for n, _ in shapes] == names == list(co.random_weights(cfg, 0))
    assert all(tuple(sd[n].shape) == s for n, s in shapes)
    state = visual.random_state(co.hf_config(cfg), 5)
    assert list(state) == names and all(state[n].shape == s and state[n].dtype == np.float32 for n, s in shapes)
    with pytest.raises(ValueError, match="bicubic"):
        visual.preprocessing(co.hf_config(cfg), {"resample": 2})
    assert visual.preprocessing(co.hf_config(cfg), {"size": {"shortest_edge": 64}, "crop_size": {"height": 64, "width": 64}}) == {
        "shortest_edge": 64, "crop": 64, "mean": visual.CLIP_MEAN, "std": visual.CLIP_STD}


def test_eot_rules():
    ids = np.array([[0, 5, 9, 7, 9, 1], [0, 9, 1, 1, 1, 1]])
    assert visual.eot_positions(ids, 9).tolist() == [2, 1] and co.eot_positions(ids, 9).tolist() == [2, 1]
    assert visual.eot_positions(ids, 2).tolist() == [2, 1] and visual.eot_positions(np.array([[0, 3, 8, 4]]), 2).tolist() == [2]


# ---- plumbing ----------------------------------------------------------------------------------------------------------------
def test_task_tables_name_the_new_type():
    assert task_handler.TASK_TO_ARTIFACT_TYPE["frame_embedding"] == "frame.embedding"
    assert task_handler.TASK_TO_RESULT_KEY["frame_embedding"] == "embeddings"
    assert "frame_embedding" in task_handler.KNOWN_TASK_TYPES


class _Frames:
    def __init__(self, n, fps=10.0):
        self.n, self.fps, self.total_frames, self.pos, self.released = n, fps, n, 0, False

    def read(self):
        if self.pos >= self.n:
            return False, None
        self.pos += 1
        return True, np.full((4, 6, 3), self.pos - 1, np.uint8)

    def grab(self):
        if self.pos >= self.n:
            return False
        self.pos += 1
        return True

    def release(self):
        self.released = True


class _Clip:
    """A stand-in with no GPU: the vector of a frame is the unit vector along axis (frame value mod 8)."""
    projection_dim = 8

    def __init__(self):
        self.batches, self.closed = [], False

    def encode_images(self, frames):
        assert isinstance(frames, np.ndarray) and frames.shape[1:] == (4, 6, 3) and frames.dtype == np.uint8
        self.batches.append(len(frames))
        return np.eye(8, dtype=np.float32)[frames[:, 0, 0, 0] % 8]

    def encode_text(self, texts):
        return np.eye(8, dtype=np.float32)[[int(t) for t in texts]]

    def close(self):
        self.closed = True


def _manager(n_frames, batch_size=4):
    clip, src = _Clip(), _Frames(n_frames)
    seen = []
    mm = ModelManager(cache_dir="/tmp/eioku-test-cache", frame_source=lambda p: src, batch_size=batch_size,
                      clip_factory=lambda cache, name: (seen.append(name), clip)[1])
    return mm, clip, src, seen


def test_embed_frames_result_shape():
    mm, clip, src, seen = _manager(19)
    out = asyncio.run(mm.embed_frames("video.mp4", {"frame_interval": 0.2}))  # fps 10: every 2nd frame, 10 sampled
    assert clip.closed and src.released and seen == ["clip-vit-base-patch32"] and clip.batches == [4, 4, 2]
    assert sorted(out) == ["embeddings"] and len(out["embeddings"]) == 10
    for i, e in enumerate(out["embeddings"]):
        assert sorted(e) == ["embedding", "frame_index", "timestamp_ms"]
        assert e["frame_index"] == 2 * i and e["timestamp_ms"] == 200 * i and type(e["frame_index"]) is int
        assert len(e["embedding"]) == 8 and all(type(v) is float for v in e["embedding"]) and e["embedding"][(2 * i) % 8] == 1.0
    # frame_interval defaults to 1.0 s: every 10th frame
    mm, *_ = _manager(19)
    assert [e["frame_index"] for e in asyncio.run(mm.embed_frames("video.mp4", {}))["embeddings"]] == [0, 10]
    with pytest.raises(ValueError, match="model_name"):
        asyncio.run(_manager(1)[0].embed_frames("video.mp4", {"model_name": "a/b"}))


class _Index:
    """A host stand-in for IndexFlatL2 (the store's ``index_factory`` seam)."""

    def __init__(self, d):
        self.x, self.dead = np.zeros((0, d), np.float32), set()

    @property
    def ntotal(self):
        return len(self.x)

    def add(self, x):
        self.x = np.concatenate([self.x, x])

    def remove_ids(self, ids):
        self.dead.update(int(i) for i in ids)

    def search_many(self, q, k, sel=None):
        d = ((self.x - q[0]) ** 2).sum(1)
        ok = np.ones(len(d), bool) if sel is None else sel.to_mask()[:len(d)].copy()
        ok[list(self.dead)] = False
        order = [i for i in np.argsort(d, kind="stable") if ok[i]][:k]
        return d[order][None], np.asarray(order, np.int64)[None]

    def close(self):
        pass


def test_index_frames_replaces_a_videos_rows_and_filters_select_them():
    eng = visual.VisualSearchEngine(_Clip(), VectorStore(8, index_factory=_Index))
    eye = np.eye(8, dtype=np.float32)
    meta = [{"frame_index": 10 * i, "timestamp_ms": 1000 * i, "thumbnail_path": f"/t/{i}.jpg", "video_duration": 9.0} for i in range(4)]
    assert eng.index_frames("a", meta, eye[:4]) == 4 and eng.index_frames("b", meta[:2], eye[[2, 5]]) == 2
    hit = eng.search("2")
    assert [(r["video_id"], r["frame_index"]) for r in hit[:2]] == [("a", 20), ("b", 0)] and hit[0]["relevance_score"] == 1.0
    assert sorted(hit[0]) == ["frame_index", "relevance_score", "thumbnail_path", "timestamp_ms", "video_id"]
    assert hit[0]["timestamp_ms"] == 2000 and hit[0]["thumbnail_path"] == "/t/2.jpg" and hit[2]["relevance_score"] == 0.0
    assert [r["frame_index"] for r in eng.search("5", filters={"video_id": "b"})] == [10, 0]
    assert [r["video_id"] for r in eng.search("2", filters={"video_id": "a", "min_duration": 5})] == ["a"] * 4
    m = eng.store._meta[0]
    assert m["segment_id"] == "a_frame0" and m["start_time"] == m["end_time"] == 0.0 and eng.store._meta[3]["start_time"] == 3.0
    # a re-run replaces the video's rows
    assert eng.index_frames("a", meta[:3], eye[[7, 6, 5]]) == 3 and len(eng.store) == 5
    assert [(r["video_id"], r["frame_index"]) for r in eng.search("7", top_k=1)] == [("a", 0)]
    by_image = eng.search_by_image(np.full((4, 6, 3), 6, np.uint8), top_k=1)
    assert [(r["video_id"], r["frame_index"], r["relevance_score"]) for r in by_image] == [("a", 10, 1.0)]


def test_process_ml_task_emits_frame_envelopes_and_indexes_them():
    eng = visual.VisualSearchEngine(_Clip(), VectorStore(8, index_factory=_Index))
    mm, clip, *_ = _manager(30)
    got = []
    ctx = {"model_manager_factory": lambda cache_dir: mm, "artifact_sink": got.extend, "visual_search_engine": eng}
    for _ in range(2):  # the second run replaces the first one's rows
        clip.closed, mm._frame_source = False, (lambda p: _Frames(30))
        res = asyncio.run(task_handler.process_ml_task(ctx, "t1", "frame_embedding", "vid", "/x.mp4", {"video_duration": 3.0}))
        assert res == {"task_id": "t1", "status": "completed", "artifact_count": 3}
    assert [e.artifact_type for e in got] == ["frame.embedding"] * 6
    assert [(e.span_start_ms, e.span_end_ms) for e in got[:3]] == [(0, 0), (1000, 1000), (2000, 2000)]
    assert len(json.loads(got[1].payload_json)["embedding"]) == 8 and len(eng.store) == 3
    assert [m["segment_id"] for m in eng.store._meta] == ["vid_frame0", "vid_frame10", "vid_frame20"]
    assert all(m["video_duration"] == 3.0 for m in eng.store._meta)
    with pytest.raises(RuntimeError, match="Unknown task type: frame_embeddings"):
        asyncio.run(task_handler.process_ml_task(ctx, "t2", "frame_embeddings", "vid", "/x.mp4", {}))
