"""Row selectors on the host and the search filters of semantic.VectorStore.

No-GPU part: RowSelector packing against a bit-by-bit loop; filter -> eligible rows for every key; the store's device-row
map and compaction policy over a fake index.  GPU part: filtered searches against a brute-force numpy ranking of the
matching rows, and the number of rows each store operation uploads."""
import logging

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from eioku_amd import search, semantic

RTOL = 1e-4


# ---- RowSelector --------------------------------------------------------------------------------------
def pack_by_hand(mask):
    words = [0] * ((len(mask) + 31) // 32)
    for r, bit in enumerate(mask):
        if bit:
            words[r // 32] |= 1 << (r % 32)
    return np.array(words, dtype=np.uint32)


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 4097])
def test_row_selector_packs_bit_r_mod_32_of_word_r_div_32(n):
    rng = np.random.default_rng(n)
    for density in (0.0, 0.03, 0.5, 1.0):
        mask = rng.random(n) < density if density < 1.0 else np.ones(n, bool)
        sel = search.RowSelector.from_mask(mask)
        assert sel.words.dtype == np.uint32 and sel.words.shape == ((n + 31) // 32,) and sel.n == n
        assert np.array_equal(sel.words, pack_by_hand(mask))
        assert np.array_equal(sel.to_mask(), mask) and sel.count() == int(mask.sum())
        ids = np.flatnonzero(mask)
        assert np.array_equal(search.RowSelector.from_ids(ids, n).words, sel.words)


@settings(max_examples=60, deadline=None)
@given(st.integers(0, 300).flatmap(lambda n: st.tuples(st.just(n), st.lists(st.booleans(), min_size=n, max_size=n))))
def test_row_selector_matches_the_loop_for_any_mask(case):
    n, bits = case
    assert np.array_equal(search.RowSelector.from_mask(np.array(bits, dtype=bool)).words, pack_by_hand(bits))


def test_row_selector_from_ids_and_ranges_clip_and_ignore():
    n = 100
    sel = search.RowSelector.from_ids([5, 5, 99, -1, 100, 12345], n)
    assert np.flatnonzero(sel.to_mask()).tolist() == [5, 99]
    sel = search.RowSelector.from_ranges([(-10, 3), (30, 34), (98, 500), (50, 50)], n)
    assert np.flatnonzero(sel.to_mask()).tolist() == [0, 1, 2, 30, 31, 32, 33, 98, 99]
    with pytest.raises(ValueError):
        search.RowSelector(np.zeros(3, np.uint32), n)  # 100 rows are 4 words


# ---- a host stand-in for IndexFlatL2 ---------------------------------------------------------------------
class FakeIndex:
    """Brute force with the surface VectorStore uses; counts what is uploaded."""

    instances = []

    def __init__(self, d):
        self.d, self.x, self.live, self.add_calls, self.closed = d, np.zeros((0, d), np.float32), np.zeros(0, bool), [], False
        FakeIndex.instances.append(self)

    @property
    def ntotal(self):
        return len(self.x)

    @property
    def nlive(self):
        return int(self.live.sum())

    def add(self, x):
        self.add_calls.append(len(x))
        self.x = np.concatenate([self.x, np.asarray(x, np.float32)])
        self.live = np.concatenate([self.live, np.ones(len(x), bool)])

    def remove_ids(self, ids):
        before = self.nlive
        self.live[np.asarray(ids, np.int64)] = False
        return before - self.nlive

    def search_many(self, q, k, sel=None):
        ok = self.live.copy()
        if sel is not None:
            assert isinstance(sel, search.RowSelector) and sel.n == self.ntotal
            ok &= sel.to_mask()
        ids = np.flatnonzero(ok)
        dist = ((self.x[ids].astype(np.float64) - np.asarray(q, np.float64)) ** 2).sum(1)
        order = np.lexsort((ids, dist))[:k]
        D = np.full((1, k), np.finfo(np.float32).max, np.float32)
        I = np.full((1, k), -1, np.int64)
        D[0, :len(order)], I[0, :len(order)] = dist[order], ids[order]
        return D, I

    def close(self):
        self.closed = True


def library(n_videos=8, per_video=5, d=16, seed=0, factory=FakeIndex):
    """Videos v0..: created on 2024-03-(1 + i), durations 60 (i + 1) s; v3 has no date, v5 no duration."""
    rng = np.random.default_rng(seed)
    store = semantic.VectorStore(d, index_factory=factory)
    x = rng.standard_normal((n_videos * per_video, d)).astype(np.float32)
    for v in range(n_videos):
        for s in range(per_video):
            meta = {"video_id": f"v{v}", "start_time": 10.0 * s, "end_time": 10.0 * s + 8.0, "text": f"v{v}s{s}", "row": v * per_video + s}
            if v != 3:
                meta["file_created_at"] = f"2024-03-{1 + v:02d}T12:00:00" + ("Z" if v % 2 else "")
            if v != 5:
                meta["video_duration"] = 60.0 * (v + 1)
            store.index_segment(f"v{v}_seg{s}", x[v * per_video + s], meta)
    return store, x


def videos_of(store, filters):
    ok = store.eligible_rows(filters)
    return sorted({m["video_id"] for m, keep in zip(store._meta, ok) if keep})


def test_each_filter_key_selects_its_rows():
    store, _ = library()
    assert store.eligible_rows(None) is None and store.eligible_rows({}) is None and store.eligible_rows({"video_id": None}) is None
    assert videos_of(store, {"video_id": "v2"}) == ["v2"]
    assert videos_of(store, {"video_id": ["v2", "v7", "nope"]}) == ["v2", "v7"]
    assert videos_of(store, {"video_id": "nope"}) == []
    # dates: inclusive at both ends; a date without a time covers its whole day; v3 has no date and never matches
    assert videos_of(store, {"created_from": "2024-03-06"}) == ["v5", "v6", "v7"]
    assert videos_of(store, {"created_from": "2024-03-06T12:00:00"}) == ["v5", "v6", "v7"]
    assert videos_of(store, {"created_from": "2024-03-06T12:00:01"}) == ["v6", "v7"]
    assert videos_of(store, {"created_to": "2024-03-02"}) == ["v0", "v1"]
    assert videos_of(store, {"created_to": "2024-03-02T12:00:00Z"}) == ["v0", "v1"]
    assert videos_of(store, {"created_to": "2024-03-02T11:59:59"}) == ["v0"]
    assert videos_of(store, {"created_from": "2024-03-01", "created_to": "2024-03-31"}) == ["v0", "v1", "v2", "v4", "v5", "v6", "v7"]
    assert videos_of(store, {"created_from": "2024-03-03T14:00:00+02:00"}) == ["v2", "v4", "v5", "v6", "v7"]  # = 12:00 UTC
    # durations: inclusive; v5 has none and never matches
    assert videos_of(store, {"min_duration": 360}) == ["v6", "v7"]
    assert videos_of(store, {"max_duration": 120}) == ["v0", "v1"]
    assert videos_of(store, {"min_duration": 120.0, "max_duration": 240}) == ["v1", "v2", "v3"]
    # the segment's own span overlaps [start_time, end_time]
    ok = store.eligible_rows({"video_id": "v0", "start_time": 18.0, "end_time": 30.0})
    assert [m["text"] for m, keep in zip(store._meta, ok) if keep] == ["v0s1", "v0s2", "v0s3"]
    # AND
    assert videos_of(store, {"video_id": ["v1", "v2", "v6"], "created_from": "2024-03-03", "max_duration": 180}) == ["v2"]
    assert videos_of(store, {"min_duration": 60, "created_to": "2024-03-04"}) == ["v0", "v1", "v2"]


def test_unknown_filter_key_is_ignored_with_one_warning(caplog):
    store, x = library()
    with caplog.at_level(logging.WARNING, logger="eioku_amd.semantic"):
        got = store.search(x[7], top_k=3, filters={"video_id": "v1", "colour": "red"})
    assert [m["video_id"] for _, m in got] == ["v1"] * 3 and got[0][1]["row"] == 7
    warned = [r for r in caplog.records if "colour" in r.getMessage()]
    assert len(warned) == 1 and warned[0].levelno == logging.WARNING
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="eioku_amd.semantic"):
        assert store.search(x[7], top_k=3, filters={"colour": "red"}) == store.search(x[7], top_k=3)
        assert store.search(x[7], top_k=3, filters={"video_id": "v1"})[0][1]["row"] == 7
    assert len([r for r in caplog.records if "colour" in r.getMessage()]) == 1


def brute(store, x_of_row, q, filters, top_k):
    ok = store.eligible_rows(filters)
    rows = [i for i in range(len(store)) if ok is None or ok[i]]
    dist = [float(((x_of_row[store._meta[i]["row"]].astype(np.float64) - q) ** 2).sum()) for i in rows]
    order = sorted(range(len(rows)), key=lambda j: (dist[j], rows[j]))[:top_k]
    return [store._meta[rows[j]]["row"] for j in order]


def test_store_keeps_a_bijection_between_live_device_rows_and_host_rows(tmp_path):
    FakeIndex.instances.clear()
    store, x = library(n_videos=8, per_video=5)
    q = x[11].astype(np.float64)
    assert FakeIndex.instances == []  # nothing touches a device before the first search
    assert [m["row"] for _, m in store.search(q, 4)] == brute(store, x, q, None, 4)
    fake = FakeIndex.instances[0]
    assert fake.add_calls == [40]
    rng = np.random.default_rng(1)
    extra = rng.standard_normal((9, 16)).astype(np.float32)
    x = np.concatenate([x, extra])

    def consistent():
        assert len(store) == len(store._meta) == len(store.matrix()) == len(store._dev_row)
        d2h = store.device_to_host_rows()
        assert len(d2h) == store._index.ntotal and store._index.nlive == len(store)
        live = np.flatnonzero(d2h >= 0)
        assert sorted(d2h[live].tolist()) == list(range(len(store)))  # onto the live host rows, one to one
        assert np.array_equal(live, np.flatnonzero(store._index.live))
        for dev, host in zip(live, d2h[live]):
            assert np.array_equal(store._index.x[dev], store._rows[host])
        for filters in (None, {"video_id": ["v1", "v6", "new"]}, {"min_duration": 200}):
            assert [m["row"] for _, m in store.search(q, 7, filters)] == brute(store, x, q, filters, 7)

    consistent()
    assert store.delete_by_video_id("v2") and not store.delete_by_video_id("v2")
    consistent()
    for j in range(4):
        store.index_segment(f"new_seg{j}", extra[j], {"video_id": "new", "row": 40 + j, "video_duration": 250.0})
    consistent()
    assert store.delete_by_video_id("v0")
    store.index_segments([f"new_seg{j}" for j in range(4, 9)], extra[4:], [{"video_id": "new", "row": 40 + j} for j in range(4, 9)])
    consistent()
    assert store.delete_by_video_id("new") and store.delete_by_video_id("v5")
    consistent()
    assert store._index is fake and fake.add_calls == [40, 1, 1, 1, 1, 5]  # appended, never rebuilt: 24 dead <= 25 live
    # removed (24 + 5) > live (20): the device index is dropped once and rebuilt compactly by the next search
    assert store.delete_by_video_id("v7")
    assert store._index is None and fake.closed and len(store) == 20
    assert [m["row"] for _, m in store.search(q, 5)] == brute(store, x, q, None, 5)
    assert len(FakeIndex.instances) == 2 and FakeIndex.instances[1].add_calls == [20] and FakeIndex.instances[1].ntotal == 20
    consistent()
    # the .index file holds the compact store
    store.save(tmp_path / "lib.index")
    back = semantic.VectorStore.load(tmp_path / "lib.index")
    assert back._meta == store._meta and np.array_equal(back.matrix(), store.matrix()) and len(back) == 20
    assert videos_of(back, {"min_duration": 200}) == videos_of(store, {"min_duration": 200}) == ["v3", "v4", "v6"]
    assert videos_of(back, {"created_to": "2024-03-05"}) == ["v1", "v4"]


def test_job_config_and_segment_dicts_carry_date_and_duration():
    from eioku_amd import task_handler

    class Gen:
        def generate_batch_embeddings(self, texts):
            return np.eye(len(texts), 8, dtype=np.float32)

    engine = semantic.SemanticSearchEngine(Gen(), semantic.VectorStore(8, index_factory=FakeIndex))
    segs = [{"text": "a", "start": 0.0, "end": 1.0}, {"text": "b", "start": 1.0, "end": 2.0, "video_duration": 7.0}]
    task_handler.embed_segments(engine, "vidA", segs, {"file_created_at": "2023-12-24", "video_duration": 99.0})
    assert [m.get("video_duration") for m in engine.store._meta] == [99.0, 7.0]
    assert [m.get("file_created_at") for m in engine.store._meta] == ["2023-12-24"] * 2
    task_handler.embed_segments(engine, "vidB", segs[:1])
    assert "file_created_at" not in engine.store._meta[2] and "video_duration" not in engine.store._meta[2]
    engine.index_transcript("vidC", [dict(segs[0], file_created_at="2024-01-05T08:00:00", video_duration=12.5)])
    assert videos_of(engine.store, {"created_from": "2024-01-01"}) == ["vidC"]
    assert videos_of(engine.store, {"max_duration": 10}) == ["vidA"]


# ---- GPU ---------------------------------------------------------------------------------------------------
def ranking(x, q, rows, top_k):
    """(rows in the float64 order, their distances, which ranks are separated from both neighbours by > 4 RTOL)."""
    rows = np.asarray(rows, np.int64)
    dist = ((x[rows].astype(np.float64) - q.astype(np.float64)) ** 2).sum(1)
    order = np.lexsort((rows, dist))
    rows, dist = rows[order], dist[order]
    gap = np.diff(dist, append=dist[-1:] + 1)
    sure = np.ones(len(rows), bool)
    sure[:-1] &= gap[:-1] > 4 * RTOL * dist[:-1]
    sure[1:] &= gap[:-1] > 4 * RTOL * dist[1:]
    return rows[:top_k], dist[:top_k], sure[:top_k]


def assert_ranked(got, x, q, rows, top_k):
    want, dist, sure = ranking(x, q, rows, top_k)
    assert len(got) == len(want)
    got_rows = np.array([m["row"] for _, m in got], np.int64)
    assert set(got_rows.tolist()) <= set(np.asarray(rows).tolist()) and len(set(got_rows.tolist())) == len(got_rows)
    assert np.allclose([d for d, _ in got], dist, rtol=RTOL, atol=1e-6)
    assert np.array_equal(got_rows[sure], want[sure])
    true = ((x[got_rows].astype(np.float64) - q.astype(np.float64)) ** 2).sum(1)
    assert np.all(np.abs(true - dist) <= RTOL * np.maximum(dist, 1e-6) + 1e-6)


@pytest.mark.gpu
def test_filtered_store_search_equals_brute_force_ranking(gpu):
    rng = np.random.default_rng(11)
    n, n_videos, d = 2000, 40, 384
    x = rng.standard_normal((n, d)) * (1.0 / (1.0 + np.arange(d) / 4.0))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    store = semantic.VectorStore(d)
    metas = []
    for i in range(n):
        v = i % n_videos
        m = {"video_id": f"v{v}", "row": i, "start_time": float(i // n_videos), "end_time": float(i // n_videos) + 1.0, "text": str(i)}
        if v % 10 != 9:
            m["file_created_at"] = f"2024-{1 + v // 4:02d}-{1 + 3 * (v % 4):02d}T09:30:00"
        if v % 7 != 6:
            m["video_duration"] = 30.0 + 15.0 * v
        metas.append(m)
    store.index_segments([f"s{i}" for i in range(n)], x, metas)
    q = x[123] + 0.05 * rng.standard_normal(d).astype(np.float32)
    cases = [{"video_id": "v17"}, {"video_id": ["v1", "v2", "v39"]}, {"created_from": "2024-03-04", "created_to": "2024-06-07"},
             {"created_to": "2024-02-01T09:30:00"}, {"min_duration": 300}, {"max_duration": 100.0}, {"min_duration": 90, "max_duration": 420},
             {"start_time": 10.0, "end_time": 12.5},
             {"video_id": [f"v{v}" for v in range(0, 40, 3)], "created_from": "2024-02-01", "max_duration": 500},
             {"created_from": "2024-05-01", "min_duration": 400, "start_time": 5.0, "end_time": 30.0}]
    for filters in cases:
        ok = store.eligible_rows(filters)
        rows = [metas[i]["row"] for i in np.flatnonzero(ok)]
        assert 0 < len(rows) < n, filters
        for top_k in (10, 45):
            assert_ranked(store.search(q, top_k, filters), x, q, rows, top_k)
    assert_ranked(store.search(q, 100), x, q, list(range(n)), 100)
    assert store.search(q, 5, {"video_id": "nobody"}) == []


@pytest.mark.gpu
def test_narrow_filter_in_a_large_library_and_uploads_per_operation(gpu, monkeypatch):
    """The far video owns 60 of 20 000 rows, none of them among the global nearest: one selector search returns them.
    Deleting and re-adding a video uploads only the new rows; the device index is rebuilt exactly when the removed rows
    outnumber the live ones."""
    rng = np.random.default_rng(5)
    n, d = 20000, 384
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = x[0] + 0.01 * rng.standard_normal(d).astype(np.float32)
    order = np.argsort(((x.astype(np.float64) - q) ** 2).sum(1), kind="stable")
    far = set(order[-60:].tolist())
    uploads, searches = [], []
    real_add, real_many = search.IndexFlatL2.add, search.IndexFlatL2.search_many
    monkeypatch.setattr(search.IndexFlatL2, "add", lambda self, rows: (uploads.append(int(rows.shape[0])), real_add(self, rows))[1])
    monkeypatch.setattr(search.IndexFlatL2, "search_many",
                        lambda self, qq, k, sel=None: (searches.append(k), real_many(self, qq, k, sel))[1])
    store = semantic.VectorStore(d)
    vid = lambda i: "far" if i in far else f"near{i % 4}"  # noqa: E731
    store.index_segments([f"s{i}" for i in range(n)], x, [{"video_id": vid(i), "row": i} for i in range(n)])
    assert uploads == []
    assert_ranked(store.search(q, top_k=100), x, q, list(range(n)), 100)
    assert uploads == [n]
    searches.clear()
    assert_ranked(store.search(q, top_k=40, filters={"video_id": "far"}), x, q, sorted(far), 40)
    assert len(store.search(q, top_k=500, filters={"video_id": ["far"]})) == 60  # all the video has
    assert searches == [40, 60]  # one search_many per call: no over-fetch loop
    with pytest.raises(ValueError):
        store.search(q, top_k=0)
    # delete a video, search, re-add it, search
    near1 = [i for i in range(n) if vid(i) == "near1"]
    assert store.delete_by_video_id("near1") and len(store) == n - len(near1)
    rest = [i for i in range(n) if vid(i) != "near1"]
    assert_ranked(store.search(q, top_k=50), x, q, rest, 50)
    assert_ranked(store.search(q, top_k=20, filters={"video_id": ["near2", "far"]}), x, q, [i for i in rest if vid(i) in ("near2", "far")], 20)
    store.index_segments([f"s{i}" for i in near1], x[near1], [{"video_id": "near1", "row": i} for i in near1])
    assert uploads == [n, len(near1)] and store._index.ntotal == n + len(near1) and store._index.nlive == n
    assert_ranked(store.search(q, top_k=50), x, q, list(range(n)), 50)
    assert_ranked(store.search(q, top_k=33, filters={"video_id": "near1"}), x, q, near1, 33)
    # compaction policy: rebuilt exactly when removed > live
    first = store._index
    store.delete_by_video_id("near0")
    assert store._index is first  # removed ~ n/2 <= live ~ 3n/4
    store.delete_by_video_id("near1")  # removed: |near1| (old copy) + |near0| + |near1| ~ 3/4 n; live ~ n/2
    assert store._index is None and uploads == [n, len(near1)]
    live = [i for i in range(n) if vid(i) not in ("near0", "near1")]
    assert_ranked(store.search(q, top_k=50), x, q, live, 50)
    assert uploads == [n, len(near1), len(live)] and store._index is not first and store._index.ntotal == len(live)
    store.delete_by_video_id("far")  # 60 removed <= live: the index stays
    assert store._index is not None and store._index.nlive == len(live) - 60
    assert store.search(q, 5, {"video_id": "far"}) == []
