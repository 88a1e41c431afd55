"""GPU: IVF-PQ (K10) - kernels vs the numpy oracle step by step, then recall against exact search.

k-means centroids come from 64-bit fixed-point sums on the GPU and float64 means in the oracle, and
assignments from fp32 MFMA vs float64, so trained codebooks agree to ~1e-6 but not bit for bit;
downstream stages are therefore compared GIVEN IDENTICAL CODEBOOKS (installed with set_codebooks),
where codes must match exactly up to argmin near-ties and ADC distances to 1e-5."""
import numpy as np
import pytest

from oracle import ivfpq as oivf, knn as oknn, prng
from eioku_amd import ivfpq, search

pytestmark = pytest.mark.gpu


def clustered(seed, n, d, ncl=40, spread=0.15):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((ncl, d)).astype(np.float32)
    x = c[rng.integers(0, ncl, n)] + spread * rng.standard_normal((n, d)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def test_kmeans_update_is_exact_mean_and_reproducible(gpu, built_lib):
    import torch
    from eioku_amd import _lib
    from eioku_amd._buffers import ptr

    rng = np.random.default_rng(0)
    x = rng.standard_normal((5000, 64)).astype(np.float32)
    a = rng.integers(0, 37, 5000).astype(np.int64)
    a[a == 5] = 6  # cluster 5 empty -> keeps its previous centroid
    cent0 = rng.standard_normal((37, 64)).astype(np.float32)
    outs = []
    for _ in range(2):
        xd, ad, cd = (torch.from_numpy(v).to(gpu) for v in (x, a, cent0.copy()))
        _lib.check(built_lib.eioku_kmeans_update(ptr(xd), 5000, 64, ptr(ad), 37, ptr(cd), None, None), "kmeans_update")
        outs.append(cd.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])  # integer atomics: bit reproducible
    want = cent0.copy()
    for c in range(37):
        if (a == c).any():
            want[c] = x[a == c].astype(np.float64).mean(0).astype(np.float32)
    assert np.allclose(outs[0], want, rtol=0, atol=2e-7)
    assert np.array_equal(outs[0][5], cent0[5])


def test_encode_and_scan_match_oracle_given_codebooks(gpu):
    d, nlist, m = 64, 16, 8
    x = clustered(1, 6000, d)
    o = oivf.IVFPQ(d, nlist, m)
    o.train(x[:3000])
    ix = ivfpq.IndexIVFPQ(d, nlist, m)
    ix.set_codebooks(o.coarse, o.pq)
    ix.add(x[:2500])
    ix.add(x[2500:])  # two batches: ids keep counting
    assert ix.ntotal == 6000
    o.add(x)
    offsets, sizes, list_codes, list_ids = (t.cpu().numpy() for t in ix._pack())
    assert sizes.sum() == 6000 and np.array_equal(np.sort(list_ids), np.arange(6000))
    # every stored (list, code) equals the oracle's, up to argmin near-ties
    got_list = np.empty(6000, np.int64)
    got_codes = np.empty((6000, m), np.uint8)
    for l in range(nlist):
        ids = list_ids[offsets[l]:offsets[l] + sizes[l]]
        got_list[ids] = l
        got_codes[ids] = list_codes[offsets[l]:offsets[l] + sizes[l]]
    assert (got_list == o.lst).mean() > 0.999
    same_list = got_list == o.lst
    assert (got_codes[same_list] == o.codes[same_list]).mean() > 0.999
    # search: compare against the oracle run on the GPU's own lists/codes (identical inputs -> ADC within 1e-5)
    o.lst, o.codes = got_list, got_codes
    q = clustered(2, 40, d)
    # both forms of the look-up table: built from the codebook per (query, list) - the oracle's own arithmetic, 1e-5 -
    # and FAISS' precomputed-table decomposition (the default): ||q-c||^2 + (||p||^2 + 2 c.p) + (-2 q.p), whose fp32
    # rounding differs from the direct sum of squares; bar = BASELINE's 1e-4 relative for kNN distances
    for pre, rtol, atol in ((False, 1e-5, 1e-6), (True, 1e-4, 1e-5)):
        ix.use_precomputed_table = pre
        for nprobe in (1, 4, 16):
            ix.nprobe = o.nprobe = nprobe
            D, I = ix.search(q, 10)
            Do, Io = o.search(q, 10)
            D, I = D.cpu().numpy(), I.cpu().numpy()
            assert np.allclose(D, Do, rtol=rtol, atol=atol), (pre, float(np.abs(D - Do).max()))
            agree = (I == Io).mean()
            assert agree > 0.97, (pre, agree)  # equal ADC distances (same code) may order by id differently only on fp ties
    ix._quantizer.close()


def test_trained_on_gpu_recall_vs_exact(gpu):
    """Train + add + search entirely on the HIP path; recall@10 against exact L2 must match what the
    oracle's own training reaches on the same data (same algorithm, different rounding)."""
    d, nlist, m = 64, 32, 16
    x = clustered(3, 20000, d)
    q = clustered(4, 64, d)
    _, It = oknn.search(x, q, 10)
    ix = ivfpq.IndexIVFPQ(d, nlist, m)
    ix.train(x)
    assert ix.is_trained and tuple(ix.coarse.shape) == (nlist, d) and tuple(ix.pq.shape) == (m, 256, d // m)
    ix.add(x)
    o = oivf.IVFPQ(d, nlist, m)
    o.train(x)
    o.add(x)
    # coarse codebooks agree closely (same init, same iterations)
    assert np.abs(ix.coarse.cpu().numpy() - o.coarse).max() < 1e-3
    rec = {}
    for name, idx in (("hip", ix), ("oracle", o)):
        idx.nprobe = 8
        _, I = idx.search(q, 10)
        I = I.cpu().numpy() if hasattr(I, "cpu") else I
        rec[name] = np.mean([len(set(I[i]) & set(It[i])) / 10 for i in range(len(q))])
    assert rec["hip"] > 0.3 and abs(rec["hip"] - rec["oracle"]) < 0.05, rec  # tight clusters: PQ cannot rank within one
    # more probes never lower recall much; nprobe = nlist scans everything
    ix.nprobe = nlist
    _, I = ix.search(q, 10)
    full = np.mean([len(set(I.cpu().numpy()[i]) & set(It[i])) / 10 for i in range(len(q))])
    assert full >= rec["hip"] - 0.02
    ix._quantizer.close()


def test_384d_m48_shapes_and_sharded_merge(gpu):
    """BASELINE cfg5 geometry (d 384, m 48 -> 8-dim sub-vectors) at a small N; two row shards with shared
    codebooks + merge == one index."""
    import torch

    d, nlist, m = 384, 64, 48
    rng = np.random.default_rng(5)
    A = rng.standard_normal((12, d)).astype(np.float32)  # 12-dim latent structure + a little noise

    def latent(n):
        z = rng.standard_normal((n, 12)).astype(np.float32) @ A + 0.3 * rng.standard_normal((n, d)).astype(np.float32)
        return (z / np.linalg.norm(z, axis=1, keepdims=True)).astype(np.float32)

    x, q = latent(12000), latent(16)
    whole = ivfpq.IndexIVFPQ(d, nlist, m)
    whole.train(x[:8000])
    whole.add(x)
    whole.nprobe = 8
    Dw, Iw = whole.search(q, 10)
    dl, il = [], []
    for r in range(2):
        lo, hi = search.shard_bounds(len(x), 2, r)
        s = ivfpq.IndexIVFPQ(d, nlist, m)
        s.set_codebooks(whole.coarse, whole.pq)
        s.add(x[lo:hi])
        s.nprobe = 8
        D, I = s.search(q, 10)
        dl.append(D)
        il.append(torch.where(I >= 0, I + lo, I))
    D, I = search.merge_topk(torch.stack(dl), torch.stack(il), 10)
    assert torch.equal(I, Iw) and torch.allclose(D, Dw)
    _, It = oknn.search(x, q, 10)
    rec = np.mean([len(set(Iw.cpu().numpy()[i]) & set(It[i])) / 10 for i in range(len(q))])
    assert rec > 0.1, rec  # chance level is 10/12000


def test_nprobe_above_32_matches_the_oracle_scan(gpu):
    """nprobe > 32 used to fail (probe selection is an IndexFlatL2 search, k <= 32 per call); rounds of 32
    chained with eioku_index_search_after now serve any nprobe.  nlist 96 / nprobe 64: same codebooks as the oracle ->
    same probed lists, ADC distances to 1e-5, and probing every list equals probing 64 when the rest hold no winner."""
    d, nlist, m = 64, 96, 8
    x = clustered(3, 9000, d, ncl=96)
    o = oivf.IVFPQ(d, nlist, m)
    o.train(x[:6000])
    o.add(x)
    ix = ivfpq.IndexIVFPQ(d, nlist, m)
    ix.set_codebooks(o.coarse, o.pq)
    ix.add(x)
    q = clustered(4, 50, d, ncl=96)
    for nprobe in (33, 64, 96):
        ix.nprobe = o.nprobe = nprobe
        D, I = (t.cpu().numpy() for t in ix.search(q, 10))
        Do, Io = o.search(q, 10)
        assert (I == Io).mean() > 0.97, nprobe
        assert np.allclose(D, Do, rtol=1e-4, atol=1e-5) or (np.abs(D - Do) < 1e-4).mean() > 0.97
    Dt, It = oknn.search(x, q, 10)
    recall = np.mean([len(set(I[i]) & set(It[i])) / 10 for i in range(len(q))])
    assert recall > 0.25  # every list probed: only the (coarse, m = 8) PQ quantisation separates it from the exact answer


def test_cfg5_geometry_nlist4096_m48_and_sharded_wrapper(gpu):
    """BASELINE cfg5's geometry on one GPU's worth of a small shard: d 384, nlist 4096, m 48 (8-dim sub-vectors), nprobe 32,
    trained by the product loop (one integer reduction per k-means iteration; `group=None` here), searched through the
    same ShardedFlatL2 wrapper the 8-GPU run uses (world 1: no collective).  Clustered unit vectors: recall against the
    exact index is the quality bar, planted exact copies must come back first."""
    import torch

    d, nlist, m, n, nq = 384, 4096, 48, 200_000, 256
    rng = np.random.default_rng(11)
    centers = rng.standard_normal((2000, d)).astype(np.float32)
    x = centers[rng.integers(0, 2000, n)] + 0.25 * rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = x[rng.integers(0, n, nq)] + 0.02 * rng.standard_normal((nq, d)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[:16] = x[1000:1016]
    xd, qd = torch.from_numpy(x).to(gpu), torch.from_numpy(q).to(gpu)
    ix = ivfpq.IndexIVFPQ(d, nlist, m)
    ix.train(xd)
    assert ix.allreduce_calls == 0 and tuple(ix.coarse.shape) == (nlist, d) and tuple(ix.pq.shape) == (m, 256, 8)
    ix.add(xd[:120_000])
    ix.add(xd[120_000:])
    ix.nprobe = 32
    sh = search.ShardedFlatL2(ix, id_base=0)
    D, I = sh.search(qd, 10)
    I = I.cpu().numpy()
    assert list(I[:16, 0]) == list(range(1000, 1016))
    flat = search.IndexFlatL2(d)
    flat.attach(xd)
    _, It = flat.search(qd, 10)
    It = It.cpu().numpy()
    recall = np.mean([len(set(I[i]) & set(It[i])) / 10 for i in range(nq)])
    r1 = np.mean([It[i, 0] in I[i] for i in range(nq)])
    assert recall > 0.45 and r1 > 0.9, (recall, r1)  # measured 0.57 / 1.0: 48 x 8-bit codes on 0.25-sigma clusters
    # the two halves of the k-means update are the whole update (what the sharded build relies on)
    from eioku_amd import _lib
    from eioku_amd._buffers import ptr

    ops = ivfpq.HipTrainOps(gpu)
    a = ops.assign(xd[:5000].contiguous(), ix.coarse)
    c1 = ix.coarse.clone()
    _lib.check(_lib.load().eioku_kmeans_update(ptr(xd[:5000].contiguous()), 5000, d, ptr(a), nlist, ptr(c1), None, None), "kmeans_update")
    c2 = ops.finalize(ops.accumulate(xd[:5000].contiguous(), a, nlist), ix.coarse.clone())
    assert torch.equal(c1, c2)


def _both_modes(ix, q, k):
    ix.scan_mode = "queries"
    Dq, Iq = ix.search(q, k)
    ix.scan_mode = "lists"
    Dl, Il = ix.search(q, k)
    return Dq, Iq, Dl, Il


@pytest.mark.parametrize("d,m,nlist,n,nq,nprobe,k", [
    (64, 8, 16, 6000, 40, 4, 10),
    (128, 16, 50, 30000, 100, 8, 10),
    (384, 48, 64, 12000, 33, 8, 10),
    (384, 48, 300, 60000, 257, 32, 20),   # k > 16: the 32-wide partial lists; ragged query tiles
    (256, 32, 40, 9000, 5, 40, 1),        # every list probed, k = 1
])
def test_list_major_scan_is_bit_identical_to_query_major(gpu, d, m, nlist, n, nq, nprobe, k):
    """Round 3: the list-major scan filters with bf16 MFMA products and re-ranks the survivors with
    the query-major kernel's fp32 arithmetic, so distances AND ids must be the query-major scan's, bit for bit - on
    unbalanced lists (clustered rows), lists without rows, queries that are database rows (distance ~ 0 candidates)
    and far-away queries alike."""
    import torch

    x = clustered(7, n, d, ncl=max(8, nlist // 2), spread=0.2)
    ix = ivfpq.IndexIVFPQ(d, nlist, m)
    ix.train(x[: max(nlist * 40, 3000)])
    ix.add(x[: n // 3])
    ix.add(x[n // 3:])
    ix.nprobe = nprobe
    rng = np.random.default_rng(8)
    q = clustered(9, nq, d, ncl=max(8, nlist // 2), spread=0.2)
    q[: nq // 3] = x[rng.integers(0, n, nq // 3)]           # exact copies of rows
    q[-1] = -q[-1]                                           # far from everything
    Dq, Iq, Dl, Il = _both_modes(ix, q, k)
    assert int(ix.last_stats[0]) == 0, "candidate lists overflowed on ordinary data"
    assert torch.equal(Iq, Il)
    assert torch.equal(Dq, Dl)
    assert int((Iq >= 0).sum()) > 0
    ix._quantizer.close()


def test_list_major_results_do_not_depend_on_its_launch_knobs(gpu, tmp_path):
    """EIOKU_LSCAN_TAU_ROWS (rows of the bound pass) is read once per process: each value in its own process, same
    index, same queries - distances and ids must be the default's bytes."""
    import os
    import subprocess
    import sys

    code = (
        "import sys, numpy as np, torch\n"
        "sys.path.insert(0, %r)\n"
        "from eioku_amd import ivfpq\n"
        "from oracle import prng\n"
        "rng = np.random.default_rng(5)\n"
        "c = rng.standard_normal((40, 128)).astype(np.float32)\n"
        "x = (c[rng.integers(0, 40, 40000)] + 0.2 * rng.standard_normal((40000, 128))).astype(np.float32)\n"
        "ix = ivfpq.IndexIVFPQ(128, 64, 16)\n"
        "ix.train(x[:6000]); ix.add(x); ix.nprobe = 8\n"
        "q = x[rng.integers(0, 40000, 150)] + 0.05 * rng.standard_normal((150, 128)).astype(np.float32)\n"
        "D, I = ix.search(q.astype(np.float32), 10)\n"
        "assert int(ix.last_stats[0]) == 0\n"
        "np.savez(sys.argv[1], D=D.cpu().numpy(), I=I.cpu().numpy())\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),)
    outs = {}
    for name, env in {"default": {}, "tau128": {"EIOKU_LSCAN_TAU_ROWS": "128"},
                      "tau8192": {"EIOKU_LSCAN_TAU_ROWS": "8192"}}.items():
        path = tmp_path / f"{name}.npz"
        subprocess.run([sys.executable, "-c", code, str(path)], check=True, env=dict(os.environ, **env), timeout=300)
        with np.load(path) as z:
            outs[name] = (z["D"], z["I"])
    assert (outs["default"][1] >= 0).all()
    for name, (D, I) in outs.items():
        assert np.array_equal(I, outs["default"][1]) and np.array_equal(D, outs["default"][0]), name


def test_list_major_overflow_falls_back_to_the_query_major_scan(gpu):
    """A candidate capacity of 8 per query (and per workgroup list) cannot hold the survivors: the overflow flag must be
    raised and the gated query-major launches must deliver the same (D, I)."""
    import torch

    d, m, nlist = 64, 8, 16
    x = clustered(1, 8000, d)
    ix = ivfpq.IndexIVFPQ(d, nlist, m)
    ix.train(x[:4000])
    ix.add(x)
    ix.nprobe = 8
    q = clustered(2, 50, d)
    ix.scan_mode = "queries"
    Dq, Iq = ix.search(q, 10)
    ix.scan_mode = "lists"
    ix.cand_cap = 8
    Dl, Il = ix.search(q, 10)
    assert int(ix.last_stats[0]) & 1                      # the workgroup lists (capacity 8 too) overflowed: every query redone
    assert torch.equal(Iq, Il) and torch.equal(Dq, Dl)
    ix.cand_cap = 64                                      # only SOME queries overflow: those are redone, the rest stand
    Dl, Il = ix.search(q, 10)
    st = ix.last_stats.cpu().tolist()
    assert st[0] == 2 and st[2] > 64, st
    assert torch.equal(Iq, Il) and torch.equal(Dq, Dl)
    ix.cand_cap = 2048
    Dl, Il = ix.search(q, 10)
    assert int(ix.last_stats[0]) == 0
    assert torch.equal(Iq, Il) and torch.equal(Dq, Dl)
    # an index none of whose lists holds k rows has no bound: everything is a candidate, still identical (fewer than k results)
    tiny = ivfpq.IndexIVFPQ(d, nlist, m)
    tiny.set_codebooks(ix.coarse, ix.pq)
    tiny.add(x[:20])
    tiny.nprobe = 16
    Dq, Iq, Dl, Il = _both_modes(tiny, q, 10)
    assert torch.equal(Iq, Il) and torch.equal(Dq, Dl)
    Dq, Iq, Dl, Il = _both_modes(tiny, q, 32)
    assert torch.equal(Iq, Il) and torch.equal(Dq, Dl) and int((Il < 0).sum()) > 0
    ix._quantizer.close()
    tiny._quantizer.close()


def test_cfg5_shard_size_12_5M_rows(gpu):
    """BASELINE cfg5 at ONE GPU's share of the 100 M x 384 index (12.5 M rows, nlist 4096, m 48, nprobe 32; VERDICT r2
    missing #3).  Rows are generated on the device (20 000 clusters: uniform 384-d vectors have no neighbourhoods for an
    IVF to find); queries = rows + a small perturbation, so each has a planted true neighbour.  Checked: the planted row
    comes back first, the list-major scan's (D, I) are the query-major scan's bit for bit, recall against the exact flat
    index on a 64-query strip, the ShardedFlatL2 wrapper (world 1) returns the index's own answer, codes cross HBM once."""
    import torch

    from eioku_amd import synth

    n, d, nlist, m, nprobe, nq, k = 12_500_000, 384, 4096, 48, 32, 1024, 10
    ncl, sigma = 20000, 0.02
    centres = synth.normal_f32(5, ncl, d, gpu, l2_normalise=True)
    assign = torch.randint(0, ncl, (n,), device=gpu, generator=torch.Generator(device=gpu).manual_seed(6))
    xb = torch.empty((n, d), dtype=torch.float32, device=gpu)
    step = 2_500_000
    for lo in range(0, n, step):
        xb[lo:lo + step] = centres[assign[lo:lo + step]] + sigma * synth.normal_f32(100 + lo // step, step, d, gpu)
    qa = torch.randint(0, n, (nq,), device=gpu, generator=torch.Generator(device=gpu).manual_seed(7))
    q = xb[qa] + 0.1 * sigma * synth.normal_f32(9, nq, d, gpu)
    ix = ivfpq.IndexIVFPQ(d, nlist, m, device=gpu)
    ix.train(xb)
    for lo in range(0, n, step):
        ix.add(xb[lo:lo + step])
    assert ix.ntotal == n
    ix.nprobe = nprobe
    D, I = ix.search(q, k)                      # list-major (default)
    stats = ix.last_stats.cpu().tolist()
    assert stats[0] == 0, stats                 # no candidate list overflowed
    offsets, sizes, list_codes, _ = ix._pack()
    assert int(sizes.sum()) == n and list_codes.shape == (n, m)
    assert stats[1] <= n // 512 + nlist         # work items: every code of a probed list is decoded at most once
    assert torch.equal(I[:, 0], qa), "a planted neighbour did not come back first"
    # bit-identity with the query-major scan (the round-2 kernel) on a strip and on the whole batch
    ix.scan_mode = "queries"
    Dq, Iq = ix.search(q, k)
    assert torch.equal(Iq, I) and torch.equal(Dq, D)
    Dq, Iq = ix.search(q[100:164], k)
    ix.scan_mode = "lists"
    Dl, Il = ix.search(q[100:164], k)
    assert torch.equal(Iq, Il) and torch.equal(Dq, Dl) and torch.equal(Il, I[100:164])
    # the 8-GPU search wrapper on a world of one: the index's own answer
    sh = search.ShardedFlatL2(ix, id_base=0)
    Ds, Is = sh.search(q[:256], k)
    assert torch.equal(Is, I[:256]) and torch.equal(Ds, D[:256])
    # recall against the exact index on a 64-query strip (inside one cluster the rows are near-equidistant in 384-d, so
    # beyond the planted neighbour an unplanted top-10 is arbitrary for ANY 48-byte code: the bar is the measured level)
    flat = search.IndexFlatL2(d)
    flat.attach(xb)
    _, It = flat.search(q[:64], k)
    assert torch.equal(It[:, 0], qa[:64])
    hit = (I[:64].unsqueeze(2) == It.unsqueeze(1)).any(dim=2).float().mean().item()
    assert hit > 0.15, hit                      # measured 0.21 at 10 M
    flat.close()
    ix._quantizer.close()
