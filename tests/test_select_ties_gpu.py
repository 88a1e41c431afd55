"""The order every search route shares: the k best by (distance, id) ascending, ties to the smaller id, ``(FLT_MAX, -1)``
padding.  Each case is the smallest shape at which one of the selection kernels meets equal distances - rows that are
copies of a few vectors, lists that share distances - and the expected answer is exact: known from the structure of
the data, or ``numpy.lexsort`` on (distance, id) of the very distances the device returned.  No tolerances."""
import numpy as np
import pytest

from eioku_amd import _lib, ivfpq, search
from eioku_amd._buffers import current_stream, ptr

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max


def copies(seed, n, d, nbase):
    """n rows, row i = base[i % nbase]: the copies of base[b] are the ids b, b + nbase, b + 2 nbase, ..."""
    base = np.random.default_rng(seed).standard_normal((nbase, d)).astype(np.float32)
    return base, np.ascontiguousarray(base[np.arange(n) % nbase])


def assert_lexsorted(D, I):
    """Every row of (D, I) ascends by (distance, id); padding is (FLT_MAX, -1) and comes last."""
    D, I = np.asarray(D), np.asarray(I)
    for q in range(D.shape[0]):
        have = int((I[q] >= 0).sum())
        assert (I[q, have:] == -1).all() and (D[q, have:] == FLT_MAX).all(), (q, D[q], I[q])
        order = np.lexsort((I[q, :have], D[q, :have]))
        assert (order == np.arange(have)).all(), (q, D[q], I[q])


# ---- 1: register-tile kernels + partial merge -------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 33])
@pytest.mark.parametrize("k", [10, 32])
def test_register_tile_route_orders_copies_by_id(gpu, nq, k):
    base, xb = copies(1, 300, 64, 5)
    ix = search.IndexFlatL2(64)
    ix.add(xb)
    D, I = ix.search(np.ascontiguousarray(np.repeat(base[2:3], nq, 0)), k)
    ix.close()
    for q in range(nq):
        assert list(I[q]) == [2 + 5 * j for j in range(k)], (q, I[q])   # k <= 60 copies: all of the answer is one tie group
        assert (D[q].view(np.uint32) == D[q, :1].view(np.uint32)).all(), (q, D[q])


# ---- 2: scan route (bin + select), and its gated fallback --------------------------------------------------------------
@pytest.mark.parametrize("rt", [1, 2])
def test_scan_route_orders_copies_by_id_and_so_does_its_fallback(gpu, rt):
    d, n, nq, k = 128, 4128, 65, 10
    base, xb = copies(2, n, d, 5)
    xq = np.ascontiguousarray(base[np.arange(nq) % 5])
    want = np.array([[q % 5 + 5 * j for j in range(k)] for q in range(nq)], dtype=np.int64)
    ix = search.IndexFlatL2(d)
    for name, v in (("scan_min_rows", 4096), ("scan_mode", 1), ("scan_min_nq", 1), ("scan_rt", rt)):
        ix.set_param(name, v)
    ix.add(xb)
    D, I = ix.search(xq, k)
    assert (I == want).all(), I
    assert (D == 0).all(), D                       # the re-rank sums (q - x)^2: a copy scores exactly 0
    ix.set_param("scan_cap", 16)                   # 826 copies per query overflow 16 slots: the register-tile kernels answer
    D, I = ix.search(xq, k)
    assert (I == want).all(), I
    assert_lexsorted(D, I)
    ix.close()


# ---- 3: the merge of sorted lists, directly ----------------------------------------------------------------------------
def sorted_lists(seed, nlists, nq, k_in, short_query):
    """[nlists][nq][k_in] lists ascending by (distance, id): distances from six values, so they repeat within and across
    lists; ids unique per query; lists of any length 0 .. k_in, (FLT_MAX, -1) padding; ``short_query`` holds 5 entries."""
    rng = np.random.default_rng(seed)
    dl = np.full((nlists, nq, k_in), FLT_MAX, np.float32)
    il = np.full((nlists, nq, k_in), -1, np.int64)
    for q in range(nq):
        ids = rng.permutation(nlists * k_in).astype(np.int64) + (1 << 33) * (q % 2)   # ids beyond 32 bits too
        for l in range(nlists):
            c = int(rng.integers(0, k_in + 1)) if l % 3 else k_in
            if q == short_query:
                c = 2 if l == 0 else (3 if l == nlists - 1 else 0)
            v = rng.integers(0, 6, c).astype(np.float32) * 0.25
            i = ids[l * k_in:l * k_in + c]
            o = np.lexsort((i, v))
            dl[l, q, :c], il[l, q, :c] = v[o], i[o]
    return dl, il


@pytest.mark.parametrize("nlists", [3, 70])
@pytest.mark.parametrize("k_in,k", [(10, 10), (32, 32), (32, 10)])
def test_topk_merge_is_lexsort_of_the_union(gpu, nlists, k_in, k):
    import torch

    nq, short = 4, 1
    dl, il = sorted_lists(3, nlists, nq, k_in, short)
    d_dev, i_dev = torch.from_numpy(dl).to(gpu), torch.from_numpy(il).to(gpu)
    D = torch.empty((nq, k), dtype=torch.float32, device=gpu)
    I = torch.empty((nq, k), dtype=torch.int64, device=gpu)
    _lib.check(_lib.load().eioku_topk_merge_ex(ptr(d_dev), ptr(i_dev), nlists, nq, k_in, k, ptr(D), ptr(I),
                                               current_stream(d_dev)), "eioku_topk_merge_ex")
    D, I = D.cpu().numpy(), I.cpu().numpy()
    for q in range(nq):
        v, i = dl[:, q].reshape(-1), il[:, q].reshape(-1)
        v, i = v[i >= 0], i[i >= 0]
        o = np.lexsort((i, v))[:k]
        wd, wi = np.full(k, FLT_MAX, np.float32), np.full(k, -1, np.int64)
        wd[:len(o)], wi[:len(o)] = v[o], i[o]
        assert (I[q] == wi).all() and (D[q].view(np.uint32) == wd.view(np.uint32)).all(), (q, D[q], I[q], wd, wi)
    assert int((I[short] >= 0).sum()) == 5


# ---- 4: IVF-PQ, list-major re-rank, its chunk carry and the probe merge of the fallback --------------------------------
def ivfpq_index(gpu, xb):
    d, m, nlist = 64, 8, 4
    rng = np.random.default_rng(4)
    ix = ivfpq.IndexIVFPQ(d, nlist, m)
    ix.set_codebooks(rng.standard_normal((nlist, d)).astype(np.float32),
                     (0.5 * rng.standard_normal((m, 256, d // m))).astype(np.float32))
    ix.add(xb)
    ix.nprobe = 4
    return ix


def both_modes(ix, q, k):
    out = {}
    for mode in ("queries", "lists"):
        ix.scan_mode = mode
        D, I = ix.search(q, k)
        out[mode] = (D.cpu().numpy(), I.cpu().numpy())
    return out["queries"], out["lists"]


def assert_same_bits(a, b):
    assert (a[1] == b[1]).all(), (a[1], b[1])
    assert (a[0].view(np.uint32) == b[0].view(np.uint32)).all(), (a[0], b[0])


@pytest.mark.parametrize("k", [10, 32])
def test_ivfpq_copies_order_by_id_in_both_scan_modes(gpu, k):
    base, xb = copies(5, 300, 64, 3)
    xq = np.concatenate([base, np.random.default_rng(6).standard_normal((2, 64)).astype(np.float32)])
    ix = ivfpq_index(gpu, xb)
    (Dq, Iq), (Dl, Il) = both_modes(ix, xq, k)
    assert int(ix.last_stats[0]) == 0
    ix.close()
    assert_same_bits((Dq, Iq), (Dl, Il))
    assert_lexsorted(Dl, Il)
    for q in range(xq.shape[0]):  # equal rows have equal codes: the 100 copies of the best vector are the whole answer
        assert list(Il[q]) == [Il[q, 0] % 3 + 3 * j for j in range(k)], (q, Il[q])
        assert (Dl[q].view(np.uint32) == Dl[q, :1].view(np.uint32)).all(), (q, Dl[q])


@pytest.mark.parametrize("k", [10, 32])
def test_ivfpq_rerank_carries_ties_across_chunks(gpu, k):
    """6000 copies of one row: one list, and 6000 equal candidates per query - three chunks of the re-rank."""
    base, xb = copies(7, 6000, 64, 1)
    xq = np.concatenate([base, -base])
    ix = ivfpq_index(gpu, xb)
    (Dq, Iq), (Dl, Il) = both_modes(ix, xq, k)
    stats = ix.last_stats.cpu().tolist()
    ix.close()
    assert stats[0] == 0 and stats[2] == 6000, stats
    assert_same_bits((Dq, Iq), (Dl, Il))
    for q in range(2):
        assert list(Il[q]) == list(range(k)), (q, Il[q])
        assert (Dl[q].view(np.uint32) == Dl[q, :1].view(np.uint32)).all(), (q, Dl[q])


def test_ivfpq_overflow_fallback_orders_copies_by_id(gpu):
    """16 candidate slots cannot hold 100 equal rows: the query-major scan and the probe merge answer."""
    k = 10
    base, xb = copies(5, 300, 64, 3)
    xq = np.concatenate([base, np.random.default_rng(6).standard_normal((2, 64)).astype(np.float32)])
    ix = ivfpq_index(gpu, xb)
    ix.cand_cap = 16
    (Dq, Iq), (Dl, Il) = both_modes(ix, xq, k)
    stats = ix.last_stats.cpu().tolist()
    ix.close()
    assert stats[0] & 1, stats
    assert_same_bits((Dq, Iq), (Dl, Il))
    assert_lexsorted(Dl, Il)
    for q in range(xq.shape[0]):
        assert list(Il[q]) == [Il[q, 0] % 3 + 3 * j for j in range(k)], (q, Il[q])
