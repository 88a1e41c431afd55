"""GPU: row selectors and removal in IVF-PQ (K10f, ``eioku_ivfpq_select_view``).

A filtered search scans a compact view of the probed lists that holds only the eligible rows, with the scans of the
unfiltered search.  Checked three ways: against the numpy oracle restricted to the selected rows (the bars of
``test_encode_and_scan_match_oracle_given_codebooks``), bit for bit against the unfiltered search (the answers under S and
under its complement merge into it, so no tolerance is involved), and the view's bytes against numpy."""
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import ivfpq as oivf
from eioku_amd import ivfpq
from eioku_amd.search import RowSelector

pytestmark = pytest.mark.gpu

D_, NLIST, M, N = 64, 16, 8, 6001  # 6001 rows: the last selector word is ragged
SELECTORS = ("video", "scatter", "even", "five", "none", "no_biggest_list")


def clustered(seed, n, d, ncl=40, spread=0.15):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((ncl, d)).astype(np.float32)
    x = c[rng.integers(0, ncl, n)] + spread * rng.standard_normal((n, d)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def host_pack(ix):
    return tuple(t.cpu().numpy() for t in ix._pack())


def build_index(o, x):
    ix = ivfpq.IndexIVFPQ(D_, NLIST, M)
    ix.set_codebooks(o.coarse, o.pq)
    ix.add(x[:2500])
    ix.add(x[2500:])  # two batches: ids keep counting
    return ix


def make_masks(n, pack):
    offsets, sizes, _, list_ids = pack
    masks = {name: np.zeros(n, dtype=bool) for name in SELECTORS}
    masks["video"][2000:2300] = True
    masks["scatter"] = np.random.default_rng(3).random(n) < 0.01
    masks["even"][0::2] = True
    masks["five"][[7, 31, 32, 4095, 6000]] = True
    big = int(np.argmax(sizes))
    masks["no_biggest_list"][:] = True
    masks["no_biggest_list"][list_ids[offsets[big]:offsets[big] + sizes[big]]] = False
    return masks


@pytest.fixture(scope="module")
def env(gpu):
    x = clustered(1, N, D_)
    o = oivf.IVFPQ(D_, NLIST, M)
    o.train(x[:3000])
    ix = build_index(o, x)
    assert ix.ntotal == N
    pack = host_pack(ix)
    offsets, sizes, list_codes, list_ids = pack
    # the oracle runs on the GPU's own lists and codes (identical inputs)
    lst, codes = np.empty(N, np.int64), np.empty((N, M), np.uint8)
    for l in range(NLIST):
        ids = list_ids[offsets[l]:offsets[l] + sizes[l]]
        lst[ids], codes[ids] = l, list_codes[offsets[l]:offsets[l] + sizes[l]]
    e = SimpleNamespace(x=x, o=o, ix=ix, pack=pack, lst=lst, codes=codes, q=clustered(2, 40, D_), masks=make_masks(N, pack),
                        oracle={})
    assert int(e.masks["scatter"].sum()) == 75
    yield e
    ix.close()


def oracle_answer(e, name, nprobe, k):
    """The oracle restricted to the selected rows: rows outside the mask sit in no list.  Its answer neither depends on the
    form of the look-up tables nor (beyond a prefix) on k: computed once per (selector, nprobe) at k = 32."""
    if (name, nprobe) not in e.oracle:
        e.o.lst, e.o.codes, e.o.nprobe = e.lst.copy(), e.codes, nprobe
        e.o.lst[~e.masks[name]] = -1
        e.oracle[(name, nprobe)] = e.o.search(e.q, 32)
    Do, Io = e.oracle[(name, nprobe)]
    return Do[:, :k], Io[:, :k]


def set_mode(ix, mode="lists", pre=True, nprobe=4):
    ix.scan_mode, ix.use_precomputed_table, ix.nprobe = mode, pre, nprobe


@pytest.mark.parametrize("nprobe", (1, 4, 16))
@pytest.mark.parametrize("pre,rtol,atol", ((False, 1e-5, 1e-6), (True, 1e-4, 1e-5)))
def test_filtered_search_matches_the_oracle_on_the_selected_rows(env, pre, rtol, atol, nprobe):
    set_mode(env.ix, "lists", pre, nprobe)
    seen = set()
    for name in SELECTORS:
        mask = env.masks[name]
        sel = RowSelector.from_mask(mask)
        for k in (1, 10, 32):
            D, I = env.ix.search(env.q, k, sel=sel)
            D, I = D.cpu().numpy(), I.cpu().numpy()
            Do, Io = oracle_answer(env, name, nprobe, k)
            found = I >= 0
            assert mask[I[found]].all(), (name, k)
            assert np.allclose(D, Do, rtol=rtol, atol=atol), (name, k, float(np.abs(D - Do).max()))
            agree = (I == Io).mean()
            assert agree > 0.97, (name, k, agree)
            per_query = found.sum(1)
            seen |= {"empty"} if (per_query == 0).any() else set()
            seen |= {"short"} if ((per_query > 0) & (per_query < k)).any() else set()
            seen |= {"full"} if (per_query == k).any() else set()
    assert seen == {"empty", "short", "full"}  # the selectors were chosen to produce all three


def merged(Da, Ia, Db, Ib, k):
    """Per query the k best of two answers by (D, id), -1 last."""
    Dc, Ic = np.concatenate([Da, Db], 1), np.concatenate([Ia, Ib], 1)
    key = np.where(Ic < 0, np.iinfo(np.int64).max, Ic)
    D, I = np.empty((len(Dc), k), np.float32), np.empty((len(Dc), k), np.int64)
    for r in range(len(Dc)):
        o = np.lexsort((key[r], Dc[r]))[:k]
        D[r], I[r] = Dc[r, o], Ic[r, o]
    return D, I


def bits(D):
    return np.ascontiguousarray(D).view(np.uint32)


@pytest.mark.parametrize("mode", ("lists", "queries"))
def test_selector_and_complement_merge_into_the_unfiltered_search_bit_for_bit(env, gpu, mode):
    import torch

    ix = env.ix
    set_mode(ix, mode, True, 4)
    ones = np.full((N + 31) // 32, 0xFFFFFFFF, dtype=np.uint32)
    for k in (1, 10, 32):
        D0, I0 = ix.search(env.q, k)
        assert ix.last_view is None
        D1, I1 = ix.search(env.q, k, sel=ones)  # packed host words
        assert ix.last_view is not None
        assert torch.equal(D0, D1) and torch.equal(I0, I1)
        D0, I0 = D0.cpu().numpy(), I0.cpu().numpy()
        for name in SELECTORS:
            mask = env.masks[name]
            Da, Ia = ix.search(env.q, k, sel=RowSelector.from_mask(mask))
            # the complement as a device selector
            words = torch.from_numpy(RowSelector.from_mask(~mask).words.view(np.int32)).to(gpu)
            Db, Ib = ix.search(env.q, k, sel=words)
            Ia, Ib = Ia.cpu().numpy(), Ib.cpu().numpy()
            assert mask[Ia[Ia >= 0]].all() and not mask[Ib[Ib >= 0]].any()
            Dm, Im = merged(Da.cpu().numpy(), Ia, Db.cpu().numpy(), Ib, k)
            assert np.array_equal(Im, I0), (name, k)
            assert np.array_equal(bits(Dm), bits(D0)), (name, k)


@pytest.mark.parametrize("d,m,nlist,n,nq,nprobe,k", [
    (64, 8, 16, 6000, 40, 4, 10),
    (384, 48, 64, 12000, 33, 8, 10),
    (256, 32, 40, 9000, 5, 40, 1),
])
def test_filtered_scan_modes_return_identical_bits(gpu, d, m, nlist, n, nq, nprobe, k):
    import torch

    x = clustered(7, n, d, ncl=max(8, nlist // 2), spread=0.2)
    ix = ivfpq.IndexIVFPQ(d, nlist, m)
    ix.train(x[: max(nlist * 40, 3000)])
    ix.add(x[: n // 3])
    ix.add(x[n // 3:])
    ix.nprobe = nprobe
    rng = np.random.default_rng(8)
    q = clustered(9, nq, d, ncl=max(8, nlist // 2), spread=0.2)
    q[: nq // 3] = x[rng.integers(0, n, nq // 3)]
    q[-1] = -q[-1]
    contiguous = np.zeros(n, dtype=bool)
    contiguous[n // 2:n // 2 + 300] = True
    for mask in (np.random.default_rng(3).random(n) < 0.03, contiguous):
        sel = RowSelector.from_mask(mask)
        ix.scan_mode = "queries"
        Dq, Iq = ix.search(q, k, sel=sel)
        ix.scan_mode = "lists"
        Dl, Il = ix.search(q, k, sel=sel)
        assert int(ix.last_stats[0]) == 0, "candidate lists overflowed on ordinary data"
        assert torch.equal(Iq, Il)
        assert torch.equal(Dq, Dl)
        got = Iq.cpu().numpy()
        assert (got >= 0).any() and mask[got[got >= 0]].all()
    ix.close()


def probed_lists(ix, q, gpu):
    import torch

    _, probes = ix._quantizer.search_many(torch.from_numpy(q).to(gpu), ix.nprobe)
    return set(int(l) for l in probes.cpu().numpy().reshape(-1) if l >= 0)


@pytest.mark.parametrize("mode", ("lists", "queries"))
@pytest.mark.parametrize("name", ("even", "scatter", "none"))
def test_the_view_is_what_numpy_says(env, gpu, mode, name):
    ix = env.ix
    set_mode(ix, mode, True, 4)
    q = env.q[:3]  # 3 queries x 4 probes: most of the 16 lists stay unprobed
    ix.search(q, 10)
    assert ix.last_view is None
    mask = env.masks[name]
    ix.search(q, 10, sel=RowSelector.from_mask(mask))
    v_offsets, v_sizes, v_codes, v_ids = (t.cpu().numpy() for t in ix.last_view)
    offsets, sizes, list_codes, list_ids = env.pack
    probed = probed_lists(ix, q, gpu)
    assert 0 < len(probed) < NLIST
    at = 0
    for l in range(NLIST):
        if l not in probed:
            assert v_sizes[l] == 0
            continue
        ids = list_ids[offsets[l]:offsets[l] + sizes[l]]
        keep = mask[ids]
        assert v_sizes[l] == keep.sum() and v_offsets[l] == at
        assert np.array_equal(v_ids[at:at + v_sizes[l]], ids[keep])
        assert np.array_equal(v_codes[at:at + v_sizes[l]], list_codes[offsets[l]:offsets[l] + sizes[l]][keep])
        at += int(v_sizes[l])


def test_a_view_that_does_not_fit_comes_out_empty_and_says_so(env, gpu, built_lib):
    """The eligible rows are known on the device only: a capacity that turns out too small must not be written past."""
    import torch
    from eioku_amd import _lib
    from eioku_amd._buffers import ptr

    ix = env.ix
    set_mode(ix, "queries", True, 4)
    offsets, sizes, list_codes, list_ids = ix._pack()
    q = torch.from_numpy(env.q[:3]).to(gpu)
    _, probes = ix._quantizer.search_many(q, 4)
    probes = probes.contiguous()
    keep = torch.full(((N + 31) // 32,), -1, dtype=torch.int32, device=gpu)
    eligible = int(sum(env.pack[1][l] for l in probed_lists(ix, env.q[:3], gpu)))
    cap = 8
    assert eligible > cap
    v_offsets = torch.full((NLIST,), -7, dtype=torch.int32, device=gpu)
    v_sizes = torch.full((NLIST,), -7, dtype=torch.int32, device=gpu)
    v_codes = torch.full((cap + 64, M), 0xAB, dtype=torch.uint8, device=gpu)
    v_ids = torch.full((cap + 64,), -7, dtype=torch.int64, device=gpu)
    status = torch.zeros((2,), dtype=torch.int32, device=gpu)
    _lib.check(built_lib.eioku_ivfpq_select_view(ptr(probes), 3, 4, NLIST, M, N, ptr(offsets), ptr(sizes), ptr(list_codes),
                                                 ptr(list_ids), None, ptr(keep), cap, ptr(v_offsets), ptr(v_sizes), ptr(v_codes),
                                                 ptr(v_ids), None, ptr(status), None), "eioku_ivfpq_select_view")
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [1, eligible]
    assert not v_sizes.cpu().numpy().any()
    assert (v_ids.cpu().numpy() == -7).all() and (v_codes.cpu().numpy() == 0xAB).all()
    # NULL keep is an error: the unfiltered path never makes this call
    assert built_lib.eioku_ivfpq_select_view(ptr(probes), 3, 4, NLIST, M, N, ptr(offsets), ptr(sizes), ptr(list_codes),
                                             ptr(list_ids), None, None, cap, ptr(v_offsets), ptr(v_sizes), ptr(v_codes),
                                             ptr(v_ids), None, ptr(status), None) == -1


def test_removed_rows_never_come_back(env, gpu):
    import torch

    ix = build_index(env.o, env.x)
    set_mode(ix, "lists", True, 16)
    q = env.q
    R = np.arange(2000, 2300)
    not_r = np.ones(N, dtype=bool)
    not_r[R] = False
    D_before, I_before = ix.search(q, 10, sel=RowSelector.from_mask(not_r))
    assert ix.remove_ids(np.concatenate([R, [N + 5], R[:3]])) == 300  # + an unknown id + repeats
    assert ix.nlive == ix.ntotal - 300 and ix.ntotal == N
    for mode in ("lists", "queries"):
        ix.scan_mode = mode
        D, I = ix.search(q, 10)
        assert ix.last_view is not None
        assert torch.equal(D, D_before) and torch.equal(I, I_before)
    for k in (1, 32):
        for sel in (None, RowSelector.from_mask(env.masks["even"]), RowSelector.from_mask(env.masks["video"])):
            _, I = ix.search(q, k, sel=sel)
            assert not np.isin(I.cpu().numpy(), R).any()
    _, I = ix.search(q, 10, sel=RowSelector.from_mask(env.masks["video"]))  # every selected row is gone
    assert (I.cpu().numpy() == -1).all()
    assert ix.remove_ids(torch.from_numpy(R).to(gpu)) == 0
    assert ix.nlive == N - 300
    # add() after removal: fresh ids, live, found
    rng = np.random.default_rng(11)
    fresh = rng.standard_normal((100, D_)).astype(np.float32)
    fresh /= np.linalg.norm(fresh, axis=1, keepdims=True)
    ix.add(fresh)
    assert ix.ntotal == N + 100 and ix.nlive == N - 200
    with pytest.raises(ValueError):
        ix.search(q, 10, sel=RowSelector.from_mask(not_r))  # a selector of the old length
    only_fresh = np.zeros(N + 100, dtype=bool)
    only_fresh[N:] = True
    _, I = ix.search(fresh, 1, sel=RowSelector.from_mask(only_fresh))  # nprobe = nlist: every list is scanned
    I = I.cpu().numpy()
    assert ((I >= N) & (I < N + 100)).all()
    for j in (0, 57, 99):  # a selector of one row finds exactly that row
        _, I = ix.search(fresh[j:j + 1], 10, sel=RowSelector.from_ids([N + j], N + 100))
        assert I.cpu().numpy()[0].tolist() == [N + j] + [-1] * 9
    _, I = ix.search(q, 32)
    assert not np.isin(I.cpu().numpy(), R).any()  # the bitmap survived the re-pack
    ix.close()
    ix.close()  # idempotent


def test_argument_checks(env, gpu):
    import torch

    ix = env.ix
    set_mode(ix, "lists", True, 4)
    nwords = (N + 31) // 32
    with pytest.raises(ValueError, match="words"):
        ix.search(env.q, 10, sel=np.zeros(nwords + 1, dtype=np.uint32))
    with pytest.raises(ValueError, match="words"):
        ix.search(env.q, 10, sel=torch.zeros(nwords - 1, dtype=torch.int32, device=gpu))
    with pytest.raises(ValueError, match="uint32"):
        ix.search(env.q, 10, sel=np.zeros(nwords, dtype=np.int64))
    with pytest.raises(ValueError, match="int32"):
        ix.search(env.q, 10, sel=torch.zeros(nwords, dtype=torch.int64, device=gpu))
    with pytest.raises(ValueError, match="rows"):
        ix.search(env.q, 10, sel=RowSelector.from_mask(np.ones(N - 1, dtype=bool)))
    with pytest.raises(ValueError, match="32"):
        ix.search_many(env.q, 33)
    # search_many: numpy in -> numpy out, CUDA in -> CUDA out, the same bits as search
    sel = RowSelector.from_mask(env.masks["even"])
    D, I = ix.search(env.q, 32, sel=sel)
    Dn, In = ix.search_many(env.q, 32, sel=sel)
    assert isinstance(Dn, np.ndarray) and isinstance(In, np.ndarray)
    assert np.array_equal(bits(Dn), bits(D.cpu().numpy())) and np.array_equal(In, I.cpu().numpy())
    Dc, Ic = ix.search_many(torch.from_numpy(env.q).to(gpu), 32, sel=sel)
    assert torch.equal(Dc, D) and torch.equal(Ic, I)
