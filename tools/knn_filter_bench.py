"""Filtered kNN over N x 384 on one GPU (K9f): every selector route against selector density, the over-fetch loop that
VectorStore.search ran before selectors existed, and the unfiltered search for an old-vs-new comparison.

    python tools/knn_filter_bench.py sweep [N] [out.json]        # routes x densities x nq, forced through sel_list_ppm
    python tools/knn_filter_bench.py overfetch [N] [out.json]    # the host over-fetch loop on plain search_many
    python tools/knn_filter_bench.py selector [N] [out.json]     # the same selectors through search(q, k, sel=...)
    python tools/knn_filter_bench.py unfiltered [N] [out.json]   # search(q, 10), nq 1024, no selector
    python tools/knn_filter_bench.py trace <route> [N]           # one filtered search per call (for rocprofv3)

``overfetch`` and ``unfiltered`` use nothing but ``attach`` / ``search`` / ``search_many``, so they also run against a
checkout of an older commit: set EIOKU_BENCH_PACKAGE_ROOT to its root to import that tree's eioku_amd instead.
Synthetic unit rows are generated on the device; HIP events bracket every timed search; every point is warmed up first;
20 timed searches per point (5 where one search takes over 200 ms), median / min / max reported in ms."""
import json
import os
import sys

sys.path.insert(0, os.environ.get("EIOKU_BENCH_PACKAGE_ROOT") or os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from eioku_amd import _lib, search, synth

D = 384
K = 10
OVERFETCH_CALL_CAP = 2000  # search_after calls (one full pass over the rows each) before the loop is reported as "> cap"


def pack(mask):
    """bool [n] on the device -> int32 words [ceil(n/32)] (bit r % 32 of word r // 32)."""
    n = mask.numel()
    pad = (-n) % 32
    if pad:
        mask = torch.cat([mask, torch.zeros(pad, dtype=torch.bool, device=mask.device)])
    bits = mask.view(-1, 32).to(torch.int64)
    w = (bits << torch.arange(32, device=mask.device, dtype=torch.int64)).sum(1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).contiguous()


def selector_masks(n, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    out = []
    run = torch.zeros(n, dtype=torch.bool, device=dev)
    run[n // 2 + 5:n // 2 + 305] = True
    out.append(("video300", "contiguous", run))
    for p in (1e-4, 1e-3, 1e-2, 0.1, 0.5, 1.0):
        out.append((f"{p:g}", "scattered", torch.rand(n, device=dev, generator=g) < p if p < 1.0 else torch.ones(n, dtype=torch.bool, device=dev)))
        if p < 1.0:
            c = torch.zeros(n, dtype=torch.bool, device=dev)
            c[n // 3 + 5:n // 3 + 5 + int(p * n)] = True
            out.append((f"{p:g}", "contiguous", c))
    return out


def timed(fn, reps=20):
    fn()  # warm-up: workspaces, planes
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    first = a.elapsed_time(b)
    ms = []
    for _ in range(5 if first > 200 else reps):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "reps": len(ms)}


def setup(n):
    _lib.init()
    dev = torch.device("cuda:0")
    xb = synth.normal_f32(21, n, D, dev, l2_normalise=True)
    ix = search.IndexFlatL2(D)
    ix.attach(xb)
    return dev, xb, ix


def sweep(n, out):
    dev, xb, ix = setup(n)
    points = []
    masks = selector_masks(n, dev)
    for nq in (1, 64, 1024):
        q = synth.normal_f32(22, nq, D, dev, l2_normalise=True)
        for name, layout, mask in masks:
            words = pack(mask)
            tiles = int((words != 0).sum())
            ref = None
            for route, ppm in (("masked", 0), ("list", 1000000)):
                ix.set_param("sel_list_ppm", ppm)
                t = timed(lambda: ix.search(q, K, sel=words))
                I = ix.search(q, K, sel=words)[1]
                ref = I if ref is None else ref
                p = dict(n=n, nq=nq, k=K, selector=name, layout=layout, eligible_rows=int(mask.sum()), nonempty_tiles=tiles,
                         tile_density=tiles / words.numel(), route=route, ids_equal_other_route=bool(torch.equal(I, ref)), **t)
                points.append(p)
                print(json.dumps(p), flush=True)
    json.dump({"sweep": points}, open(out, "w"), indent=1)


def overfetch_search(ix, q, allowed, n, top_k):
    """semantic.VectorStore.search as it was before selectors: over-fetch global neighbours, filter, quadruple."""
    fetch = min(n, max(32, 4 * top_k))
    calls = 0
    while True:
        calls += (fetch + 31) // 32 if fetch > 32 else 1
        if calls > OVERFETCH_CALL_CAP:
            return None, calls
        Dd, I = ix.search_many(q, fetch)
        ids = I[0]
        ids = ids[ids >= 0]
        hit = ids[allowed[ids]][:top_k]
        if hit.numel() == top_k or fetch >= n:
            return hit, calls
        fetch = min(n, fetch * 4)


def overfetch(n, out, use_selector):
    dev, xb, ix = setup(n)
    q = synth.normal_f32(22, 1, D, dev, l2_normalise=True)
    points = []
    for name, layout, mask in selector_masks(n, dev):
        if use_selector:
            words = pack(mask)
            t = timed(lambda: ix.search_many(q, K, sel=words))
            p = dict(method="selector", n=n, nq=1, k=K, selector=name, layout=layout, **t)
        else:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            hit, calls = overfetch_search(ix, q, mask, n, K)  # warm-up, and whether the loop ends under the cap at all
            if hit is None:
                p = dict(method="overfetch", n=n, nq=1, k=K, selector=name, layout=layout, median_ms=None,
                         note=f"> cap: more than {OVERFETCH_CALL_CAP} full passes over the rows", search_after_calls=calls)
            else:
                ms = []
                for _ in range(20 if calls < 50 else 3):
                    torch.cuda.synchronize()
                    a.record()
                    overfetch_search(ix, q, mask, n, K)
                    b.record()
                    torch.cuda.synchronize()
                    ms.append(a.elapsed_time(b))
                ms.sort()
                p = dict(method="overfetch", n=n, nq=1, k=K, selector=name, layout=layout, median_ms=round(ms[len(ms) // 2], 4),
                         min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), reps=len(ms), search_after_calls=calls)
        points.append(p)
        print(json.dumps(p), flush=True)
    json.dump({"points": points}, open(out, "w"), indent=1)


def unfiltered(n, out):
    dev, xb, ix = setup(n)
    q = synth.normal_f32(22, 1024, D, dev, l2_normalise=True)
    p = dict(method="unfiltered", n=n, nq=1024, k=K, **timed(lambda: ix.search(q, K)))
    print(json.dumps(p), flush=True)
    json.dump(p, open(out, "w"))


def trace(route, n):
    dev, xb, ix = setup(n)
    ix.set_param("sel_list_ppm", 0 if route == "masked" else 1000000)
    name, layout, mask = selector_masks(n, dev)[5 if route == "masked" else 0]  # masked: 1 % scattered; list: one video
    q = synth.normal_f32(22, 64, D, dev, l2_normalise=True)
    words = pack(mask)
    for _ in range(3):
        ix.search(q, K, sel=words)
    torch.cuda.synchronize()
    print("traced", route, name, layout)


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "trace":
        trace(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000)
    else:
        n = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
        out = sys.argv[3] if len(sys.argv) > 3 else "/dev/null"
        {"sweep": sweep, "unfiltered": unfiltered, "overfetch": lambda n, o: overfetch(n, o, False),
         "selector": lambda n, o: overfetch(n, o, True)}[mode](n, out)
