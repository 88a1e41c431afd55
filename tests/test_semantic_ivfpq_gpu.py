"""GPU: ``VectorStore`` over an IVF-PQ index (``ivfpq.store_index_factory``): the product's filter keys and
delete-by-video on the index built for libraries that cannot be flat."""
import numpy as np
import pytest

from eioku_amd import ivfpq
from eioku_amd.search import RowSelector
from eioku_amd.semantic import VectorStore

pytestmark = pytest.mark.gpu

D_, NVID, PER = 64, 20, 300


def clustered(seed, n, d, ncl=40, spread=0.15):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((ncl, d)).astype(np.float32)
    x = c[rng.integers(0, ncl, n)] + spread * rng.standard_normal((n, d)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def video_of(meta):
    return int(meta["video_id"][1:])


def test_store_filters_and_deletes_on_ivfpq(gpu):
    n = NVID * PER
    x = clustered(1, n, D_)
    store = VectorStore(D_, index_factory=ivfpq.store_index_factory(nlist=16, m=8, nprobe=16))
    meta = [{"video_id": f"v{i // PER}", "start_time": float(i % PER), "end_time": float(i % PER + 1),
             "file_created_at": f"2024-01-{i // PER + 1:02d}", "video_duration": 60.0 + 10.0 * (i // PER)} for i in range(n)]
    assert store.index_segments([f"s{i}" for i in range(n)], x, meta) == n
    q = clustered(2, 1, D_)[0]

    # one video: nprobe = nlist, so every eligible row is reachable and 10 results come back
    got = store.search(q, 10, filters={"video_id": "v7"})
    assert len(got) == 10 and all(m["video_id"] == "v7" for _, m in got)
    index = store._index
    assert isinstance(index, ivfpq.IndexIVFPQ) and index.is_trained and index.ntotal == n
    D, I = index.search_many(q.reshape(1, -1), 10, sel=RowSelector.from_ranges([(7 * PER, 8 * PER)], n))
    assert isinstance(D, np.ndarray)
    assert [m["segment_id"] for _, m in got] == [f"s{i}" for i in I[0]]
    assert [d for d, _ in got] == [float(d) for d in D[0]]

    # a date range and a duration range
    got = store.search(q, 32, filters={"created_from": "2024-01-03", "created_to": "2024-01-05"})
    assert len(got) == 32 and all(2 <= video_of(m) <= 4 for _, m in got)
    got = store.search(q, 32, filters={"min_duration": 100, "max_duration": 120})
    assert len(got) == 32 and all(4 <= video_of(m) <= 6 for _, m in got)

    # delete-by-video takes the rows out of the same index: nothing is rebuilt
    assert store.delete_by_video_id("v7")
    assert store._index is index and index.ntotal == n and index.nlive == n - PER
    got = store.search(q, 32)
    assert len(got) == 32 and all(m["video_id"] != "v7" for _, m in got)
    assert store.search(q, 10, filters={"video_id": "v7"}) == []
    got = store.search(q, 10, filters={"video_id": ["v7", "v8"]})
    assert len(got) == 10 and all(m["video_id"] == "v8" for _, m in got)
    assert store._index is index

    with pytest.raises(ValueError, match="32"):
        store.search(q, top_k=40)
    index.close()
