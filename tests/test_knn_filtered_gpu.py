"""GPU parity of K9f: flat kNN under a row selector and after remove_ids, against the float64 brute force.

Bar: the project's own (test_knn_gpu.check, RTOL = 1e-4): distances within 1e-4 relative of float64, every returned id's
true distance within that of the truth at its rank, ids identical where the truth is separated by more than 4 RTOL; plus
every returned id is eligible and -1 stands exactly where the truth has -1.  The truth of a selector is the oracle on
``xb[eligible]`` with ids mapped back (row order, hence the smaller-id tie rule, is preserved).

Inputs have a decaying spectrum (dimension j scaled by 1 / (1 + j/4)): isotropic unit rows concentrate every distance
near 2.0 and leave 14-46 % of the (query, rank) entries inside the 4 RTOL near-tie band.  Every test computes that
excluded share from the float64 truth BEFORE it looks at the GPU result and asserts it <= 0.10 (k <= 16) / 0.16 (k = 32);
excluded entries are excluded from the id-equality assertion only.

Routes: a selector search runs on the exact-fp32 register-tile kernels, either walking every slab with the mask applied
("masked", sel_list_ppm 0) or walking the compacted list of non-empty tiles ("list", sel_list_ppm 1000000), chosen on
the device by density in between ("auto").  Selector searches never take the scan path, so the "scan" configurations
below (scan_min_rows lowered as test_knn_scan_gpu.scan_index does) check that a selector is honoured when the index
would otherwise scan; removal IS exercised on the scan kernels (an unfiltered search after remove_ids takes them)."""
import numpy as np
import pytest

from oracle import knn as oknn, prng
from eioku_amd import search
from test_knn_gpu import RTOL, check

pytestmark = pytest.mark.gpu
FLT_MAX = np.finfo(np.float32).max

ROUTES = {
    "masked": dict(scan_mode=0, sel_list_ppm=0),
    "list": dict(scan_mode=0, sel_list_ppm=1000000),
    "auto": dict(scan_mode=0),
    "scan_rt1": dict(scan_mode=1, scan_min_rows=4096, scan_rt=1),
    "scan_rt2": dict(scan_mode=1, scan_min_rows=4096, scan_rt=2),
}


def spectrum_rows(seed, n, d):
    x = prng.approx_normal_f32(seed, n * d).reshape(n, d).astype(np.float64)
    x *= 1.0 / (1.0 + np.arange(d) / 4.0)
    return (x / np.sqrt((x ** 2).sum(1, keepdims=True))).astype(np.float32)


def make_index(d, xb=None, **params):
    ix = search.IndexFlatL2(d)
    for k, v in params.items():
        ix.set_param(k, v)
    if xb is not None:
        ix.add(xb)
    return ix


def set_route(ix, route):
    ix.set_param("sel_list_ppm", 32000)  # the default
    for k, v in ROUTES[route].items():
        ix.set_param(k, v)


def selectors(n):
    rng = np.random.default_rng(1234 + n)
    run = np.zeros(n, bool)
    run[n // 2 + 5:n // 2 + 305] = True  # one "video": contiguous, not tile-aligned
    return {"half": rng.random(n) < 0.5, "one_percent": rng.random(n) < 0.01, "run300": run}


def masked_truth(xb, xq, k, mask):
    ids = np.flatnonzero(mask)
    Dt, It = oknn.search(xb[ids], xq, k)
    return Dt, np.where(It >= 0, ids[np.clip(It, 0, max(len(ids) - 1, 0))] if len(ids) else -1, -1)


def excluded_share(Dt, It):
    """Share of the truth's finite (query, rank) entries inside the 4 RTOL near-tie band: test_knn_gpu.check's rule."""
    finite = It >= 0
    with np.errstate(invalid="ignore"):
        gap = np.diff(Dt, axis=1, append=Dt[:, -1:] + 1)
        sure = np.ones_like(It, dtype=bool)
        sure[:, :-1] &= gap[:, :-1] > 4 * RTOL * Dt[:, :-1]
        sure[:, 1:] &= gap[:, :-1] > 4 * RTOL * Dt[:, 1:]
    return float((finite & ~sure).sum()) / max(int(finite.sum()), 1)


def truth_with_cap(xb, xq, k, mask, what=""):
    Dt, It = masked_truth(xb, xq, k, mask)
    share = excluded_share(Dt, It)
    print(f"excluded share {what}: {share:.3f}")
    assert share <= (0.10 if k <= 16 else 0.16), (what, share)
    return Dt, It


def check_filtered(D, I, Dt, It, xb, xq, mask):
    D, I = np.asarray(D), np.asarray(I)
    got = I[I >= 0]
    assert np.all(mask[got]), "an ineligible row was returned"
    assert np.array_equal(I == -1, It == -1)
    assert np.all(D[I == -1] == FLT_MAX)
    for q in range(I.shape[0]):
        assert len(set(I[q][I[q] >= 0].tolist())) == int((I[q] >= 0).sum()), "duplicate id"
    check(D, I, Dt, It, xb, xq)


@pytest.mark.parametrize("n,nq,k,d", [(20000, 70, 10, 384), (50001, 300, 10, 384), (33333, 200, 16, 256), (40000, 129, 10, 128),
                                      (5000, 16, 10, 384), (300000, 64, 10, 384), (30000, 100, 32, 384), (3000, 5, 32, 384)])
def test_selector_search_matches_float64_truth_on_every_route(gpu, n, nq, k, d):
    import torch

    xb, xq = spectrum_rows(71, n, d), spectrum_rows(72, nq, d)
    truth_with_cap(xb, xq, k, np.ones(n, bool), "all rows")
    sels = selectors(n)
    truths = {name: truth_with_cap(xb, xq, k, mask, name) for name, mask in sels.items()}
    ix = make_index(d, xb)
    for name, mask in sels.items():
        Dt, It = truths[name]
        sel = search.RowSelector.from_mask(mask)
        for route in ROUTES:
            set_route(ix, route)
            D, I = ix.search(xq, k, sel=sel)
            check_filtered(D, I, Dt, It, xb, xq, mask)
            # the packed words on the device, and the words as a bare array: the same bytes back
            Dd, Id = ix.search(xq, k, sel=torch.from_numpy(sel.words.view(np.int32)).to(gpu))
            assert np.array_equal(Dd, D) and np.array_equal(Id, I), (name, route)
            Dw, Iw = ix.search(xq, k, sel=sel.words)
            assert np.array_equal(Dw, D) and np.array_equal(Iw, I)
    ix.close()


def bound_trap():
    n, nq, k, d = 20000, 70, 10, 384
    xb, xq = spectrum_rows(81, n, d), spectrum_rows(82, nq, d)
    noise = prng.approx_normal_f32(83, 6000 * d).reshape(6000, d)
    bad = 3 * np.arange(6000) + 1
    near = xq[np.arange(6000) % nq].astype(np.float64) + 0.01 * noise
    xb[bad] = (near / np.sqrt((near ** 2).sum(1, keepdims=True))).astype(np.float32)
    mask = np.ones(n, bool)
    mask[bad] = False
    return xb, xq, k, d, mask


@pytest.mark.parametrize("params", [
    dict(scan_mode=1, scan_min_rows=4096, scan_prescan=0), dict(scan_mode=1, scan_min_rows=4096, scan_prescan=4),
    dict(scan_mode=1, scan_min_rows=4096, scan_prescan=0, scan_cap=16), dict(scan_mode=1, scan_min_rows=4096, scan_prescan=4, scan_cap=16),
    dict(scan_mode=0, sel_list_ppm=0), dict(scan_mode=0, sel_list_ppm=1000000)])
def test_a_bound_over_ineligible_rows_never_hides_eligible_neighbours(gpu, params):
    """The ineligible rows (3i + 1, i < 6000: scattered, never tile-aligned) are tight copies of the queries: every
    unfiltered top-10 lies inside that cluster (k-th distance <= 0.036) while the nearest ELIGIBLE row of any query is
    >= 0.276 away.  A search that bounds its scan with ineligible rows rejects every eligible row and returns -1s.  Here
    a selector search leaves the scan path alone; the same rows REMOVED instead run on the scan kernels, whose sample
    search and pre-scan then see +inf norms for them.

    The removal half runs where an unfiltered 70-query search stays on the scan kernels.  With scan_mode 0, or when
    scan_cap 16 overflows into the fallback, such a search is the split-bf16 register-tile kernel, as it was before
    removal existed, and on these strongly correlated rows (q.x ~ 0.7) its dropped lo.lo products bias the distances:
    measured max relative error 1.62e-4 against float64 on a FRESH compact index of the eligible rows, the same figure
    after remove_ids - outside this file's 1e-4 bar with or without removal.  Selector searches never run that kernel;
    test_removal_leaves_the_split_bf16_kernel_bit_exact covers removal on it."""
    xb, xq, k, d, mask = bound_trap()
    Du, _ = oknn.search(xb, xq, k)
    assert Du[:, -1].max() <= 0.036
    Dt, It = truth_with_cap(xb, xq, k, mask, "bound trap")
    assert Dt[:, 0].min() >= 0.275  # 0.2759
    ix = make_index(d, xb, **params)
    D, I = ix.search(xq, k, sel=search.RowSelector.from_mask(mask))
    check_filtered(D, I, Dt, It, xb, xq, mask)
    if params["scan_mode"] == 1 and params.get("scan_cap") != 16:
        assert ix.remove_ids(np.flatnonzero(~mask)) == 6000
        D, I = ix.search(xq, k)  # unfiltered: the scan path when the parameters ask for it
        check_filtered(D, I, Dt, It, xb, xq, mask)
    ix.close()


@pytest.mark.parametrize("route", ["masked", "list", "auto"])
def test_few_eligible_rows_empty_and_full_selectors_and_bits_beyond_n(gpu, route):
    n, nq, d = 5003, 16, 384  # 5003 = 156 * 32 + 11: the last word has 21 bits beyond n
    xb, xq = spectrum_rows(71, n, d), spectrum_rows(72, nq, d)
    ix = make_index(d, xb)
    set_route(ix, route)
    seven = np.zeros(n, bool)
    seven[[3, 64, 65, 1000, 4095, 4992, 5002]] = True
    for k in (10, 32):
        Dt, It = masked_truth(xb, xq, k, seven)
        D, I = ix.search(xq, k, sel=search.RowSelector.from_mask(seven))
        assert np.all(I[:, 7:] == -1) and np.all(D[:, 7:] == FLT_MAX) and np.array_equal(I[:, :7], It[:, :7])
        assert np.allclose(D[:, :7], Dt[:, :7], rtol=RTOL, atol=1e-6)
        D, I = ix.search(xq, k, sel=search.RowSelector.from_mask(np.zeros(n, bool)))
        assert np.all(I == -1) and np.all(D == FLT_MAX)
    # all ones == no selector, bit for bit (16 queries over 5003 rows: the plain search runs the same exact-fp32
    # register-tile kernel; wider plain searches use split-bf16 products or the scan path's re-rank, whose distances
    # differ from the exact-fp32 ones in their last bits)
    D0, I0 = ix.search(xq, 10)
    ones = search.RowSelector.from_mask(np.ones(n, bool))
    D1, I1 = ix.search(xq, 10, sel=ones)
    assert np.array_equal(D1, D0) and np.array_equal(I1, I0)
    beyond = ones.words.copy()
    beyond[-1] = 0xFFFFFFFF  # bits of rows that do not exist
    D2, I2 = ix.search(xq, 10, sel=beyond)
    assert np.array_equal(D2, D0) and np.array_equal(I2, I0)
    seven_beyond = search.RowSelector.from_mask(seven).words.copy()
    seven_beyond[-1] |= 0xFFFFF800
    D3, I3 = ix.search(xq, 10, sel=seven_beyond)
    assert np.all(I3[:, 7:] == -1) and np.all((I3[:, :7] >= 0) & (I3[:, :7] < n))
    with pytest.raises(ValueError):
        ix.search(xq, 10, sel=ones.words[:-1])
    with pytest.raises(ValueError):
        ix.search(xq, 10, sel=search.RowSelector.from_mask(np.ones(n + 40, bool)))
    ix.close()


@pytest.mark.parametrize("route", ["masked", "list"])
def test_search_many_under_a_selector(gpu, route):
    n, nq, d = 50001, 5, 384
    xb, xq = spectrum_rows(71, n, d), spectrum_rows(72, nq, d)
    ix = make_index(d, xb)
    set_route(ix, route)
    mask = selectors(n)["run300"]
    Dt, It = masked_truth(xb, xq, 300, mask)
    D, I = ix.search_many(xq, 100, sel=search.RowSelector.from_mask(mask))
    assert D.shape == (nq, 100) and np.all(np.diff(D, axis=1) >= 0)
    for q in range(nq):
        assert len(set(I[q].tolist())) == 100 and np.all(mask[I[q]])
    check(D, I, Dt[:, :100], It[:, :100], xb, xq)
    sixty = np.zeros(n, bool)
    sixty[np.random.default_rng(3).choice(n, 60, replace=False)] = True
    D, I = ix.search_many(xq, 500, sel=search.RowSelector.from_mask(sixty))
    assert D.shape == (nq, 500) and np.all(I[:, 60:] == -1) and np.all(D[:, 60:] == FLT_MAX)
    for q in range(nq):
        assert sorted(I[q, :60].tolist()) == np.flatnonzero(sixty).tolist()
    ix.close()


@pytest.mark.parametrize("family", ["register_tile", "scan_rt1", "scan_rt2"])
def test_remove_ids_keeps_ids_stable_and_composes_with_selectors_and_add(gpu, family):
    # register_tile: 64 queries = two narrow passes of the exact-fp32 kernel (a wider unfiltered search is the split-bf16
    # kernel, whose own error on these rows exceeds the 1e-4 bar, see test_removal_leaves_the_split_bf16_kernel_bit_exact)
    n, nq, k, d = 20000, 64 if family == "register_tile" else 70, 10, 384
    xb_all, xq = spectrum_rows(71, n + 5000, d), spectrum_rows(72, nq, d)
    xb = xb_all[:n]
    params = dict(scan_mode=0) if family == "register_tile" else dict(ROUTES[family])
    ix = make_index(d, xb, **params)
    D, I = ix.search(xq, k)  # the scan family builds its planes here, before anything is removed
    live = np.ones(n, bool)
    # a whole contiguous "video", a scattered 1 %, ids that do not exist, one id twice
    video = np.arange(7001, 7641)
    scattered = np.flatnonzero(np.random.default_rng(9).random(n) < 0.01)
    assert ix.remove_ids(video) == len(video)
    live[video] = False
    assert ix.remove_ids(np.concatenate([scattered, [-5, n, n + 123456, scattered[0]]])) == int(live[scattered].sum())
    live[scattered] = False
    assert ix.remove_ids(video[:10]) == 0  # twice is harmless
    assert ix.ntotal == n and ix.nlive == int(live.sum())
    Dt, It = truth_with_cap(xb, xq, k, live, "after removal")
    D, I = ix.search(xq, k)
    check_filtered(D, I, Dt, It, xb, xq, live)
    # remove AND selector
    half = selectors(n)["half"]
    Dt, It = truth_with_cap(xb, xq, k, live & half, "removal and selector")
    for ppm in (0, 1000000):
        ix.set_param("sel_list_ppm", ppm)
        D, I = ix.search(xq, k, sel=search.RowSelector.from_mask(half))
        check_filtered(D, I, Dt, It, xb, xq, live & half)
    # add() after removal: fresh ids, the removed ones stay gone (the planes are extended, not rebuilt)
    ix.add(xb_all[n:])
    live2 = np.concatenate([live, np.ones(5000, bool)])
    assert ix.ntotal == n + 5000 and ix.nlive == int(live2.sum())
    Dt, It = truth_with_cap(xb_all, xq, k, live2, "add after removal")
    D, I = ix.search(xq, k)
    check_filtered(D, I, Dt, It, xb_all, xq, live2)
    assert (I >= n).any()
    assert ix.remove_ids([n + 7, 3]) == 2  # a new row and an old one
    live2[[n + 7, 3]] = False
    Dt, It = masked_truth(xb_all, xq, k, live2)
    D, I = ix.search(xq, k)
    check_filtered(D, I, Dt, It, xb_all, xq, live2)
    # reset() then add() starts clean
    ix.reset()
    assert ix.ntotal == 0 and ix.nlive == 0
    ix.add(xb[:6000])
    assert ix.nlive == 6000
    Dt, It = oknn.search(xb[:6000], xq, k)
    D, I = ix.search(xq, k)
    check(D, I, Dt, It, xb, xq)
    ix.close()


def test_removal_leaves_the_split_bf16_kernel_bit_exact(gpu):
    """Unfiltered searches of more than 64 queries with k <= 16 run k_flat_l2_bf.  Its distances carry the bias of the
    dropped lo.lo products (up to 1.6e-4 relative on rows as correlated as these, so the float64 bar is not this test's
    yardstick); what removal must guarantee is that the kernel computes, for the rows that remain, exactly what it
    computes for an index that never held the others: same bits in D, same rows in I (ids mapped; the mapping is
    monotone, so ties keep their order)."""
    n, nq, k, d = 20000, 70, 10, 384
    xb, xq = spectrum_rows(71, n, d), spectrum_rows(72, nq, d)
    live = np.random.default_rng(4).random(n) < 0.7
    live[6400:7040] = False  # whole tiles as well
    ix = make_index(d, xb, scan_mode=0)
    assert ix.remove_ids(np.flatnonzero(~live)) == int((~live).sum())
    D, I = ix.search(xq, k)
    compact = make_index(d, xb[live], scan_mode=0)
    Dc, Ic = compact.search(xq, k)
    assert D.tobytes() == Dc.tobytes() and np.array_equal(I, np.flatnonzero(live)[Ic])
    Dt, It = masked_truth(xb, xq, k, live)
    assert np.allclose(D, Dt, rtol=4 * RTOL, atol=1e-6) and (I == It).mean() > 0.9  # sanity only: the bar above is exact
    ix.close()
    compact.close()


def test_remove_ids_on_an_attached_tensor(gpu):
    import torch

    n, nq, k, d = 20000, 20, 10, 384
    xb, xq = spectrum_rows(71, n, d), spectrum_rows(72, nq, d)
    t = torch.from_numpy(xb).to(gpu)
    before = t.clone()
    ix = search.IndexFlatL2(d)
    ix.set_param("scan_mode", 0)
    ix.attach(t)
    gone = torch.arange(100, 9000, 7, device=gpu)
    assert ix.remove_ids(gone) == int(gone.numel()) and ix.nlive == n - int(gone.numel())
    live = np.ones(n, bool)
    live[gone.cpu().numpy()] = False
    Dt, It = masked_truth(xb, xq, k, live)
    D, I = ix.search(torch.from_numpy(xq).to(gpu), k)
    check_filtered(D.cpu().numpy(), I.cpu().numpy(), Dt, It, xb, xq, live)
    assert torch.equal(t, before)  # the caller's buffer is not written
    ix.attach(t)  # attaching again forgets the removals
    assert ix.nlive == n
    ix.close()


def test_unfiltered_search_is_byte_identical_to_the_parent_build(gpu):
    """(D, I) of plain searches equal tests/golden/knn_unfiltered_parent.npz, recorded on the GPU from the build of the
    commit before selectors and removal existed with

        python tests/golden/make_knn_unfiltered_golden.py tests/golden/knn_unfiltered_parent.npz

    (three shapes of test_scan_matches_float64_truth on the scan path, three of test_search_matches_float64_truth on the
    register-tile kernels)."""
    import importlib.util

    from conftest import GOLDEN

    spec = importlib.util.spec_from_file_location("make_knn_unfiltered_golden", GOLDEN / "make_knn_unfiltered_golden.py")
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    g = np.load(GOLDEN / "knn_unfiltered_parent.npz")
    for c, case in enumerate(mk.CASES):
        D, I = mk.run_case(*case)
        assert D.tobytes() == g[f"D{c}"].tobytes(), case
        assert np.array_equal(I, g[f"I{c}"].astype(np.int64)), case


@pytest.mark.parametrize("route", ["masked", "list"])
def test_selector_words_are_addressed_exactly(gpu, route):
    """The device selector is a view into the middle of a larger tensor whose neighbouring words hold the complement
    pattern (and ones beyond n in the last word): an off-by-one in the word index is a wrong answer, not an over-read
    nobody sees."""
    import torch

    n, nq, k, d = 40011, 33, 10, 128
    xb, xq = spectrum_rows(71, n, d), spectrum_rows(72, nq, d)
    ix = make_index(d, xb)
    set_route(ix, route)
    for name, mask in selectors(n).items():
        words = search.RowSelector.from_mask(mask).words
        nw = len(words)
        inside = words.copy()
        inside[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)  # ones beyond n in the view's last word
        big = np.concatenate([~words, inside, ~words])
        dev = torch.from_numpy(big.view(np.int32)).to(gpu)
        own = torch.from_numpy(words.view(np.int32)).to(gpu)
        D0, I0 = ix.search(xq, k, sel=own)
        D1, I1 = ix.search(xq, k, sel=dev[nw:2 * nw])
        assert np.array_equal(D1, D0) and np.array_equal(I1, I0), name
        Dt, It = masked_truth(xb, xq, k, mask)
        check_filtered(D0, I0, Dt, It, xb, xq, mask)
    ix.close()
