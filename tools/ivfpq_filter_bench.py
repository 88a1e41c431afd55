"""Filtered IVF-PQ search over N x 384 on one GPU (K10f): the selected view + scan against selector density, beside the
unfiltered search on the same build and the only thing an index without selectors can do (over-fetch 32, filter on the host).

    python tools/ivfpq_filter_bench.py [N=10_000_000] [out=profiles/ivfpq_filtered.json]
    python tools/ivfpq_filter_bench.py trace [N]        # three filtered searches (1 % scattered, nq 64) for rocprofv3

Geometry and data of tools/ivfpq_bench.py (nlist 4096, m 48, nprobe 32, k 10; clustered rows, queries with a planted
neighbour), the selector ladder of tools/knn_filter_bench.py.  HIP events bracket every timed call; every point is warmed
up first; median / min / max of 20 calls in ms.  The view pre-pass (eioku_ivfpq_select_view) is also timed alone."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from eioku_amd import _lib, ivfpq, synth

D, NLIST, M, NPROBE, K = 384, 4096, 48, 32, 10
OVERFETCH = 32  # the most one IVF-PQ search returns


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
    fn()  # warm-up: workspaces, view arrays
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def setup(n):
    _lib.init(0)
    dev = torch.device("cuda:0")
    ncl, sigma, step = 20000, 0.02, 2_000_000
    centres = synth.normal_f32(5, ncl, D, dev, l2_normalise=True)
    assign = torch.randint(0, ncl, (n,), device=dev, generator=torch.Generator(device=dev).manual_seed(6))
    xb = torch.empty((n, D), dtype=torch.float32, device=dev)
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        xb[lo:hi] = centres[assign[lo:hi]] + sigma * synth.normal_f32(100 + lo // step, hi - lo, D, dev)
    ix = ivfpq.IndexIVFPQ(D, NLIST, M, device=dev)
    ix.train(xb)
    for lo in range(0, n, step):
        ix.add(xb[lo:min(n, lo + step)])
    ix._pack()
    ix.nprobe = NPROBE
    queries = {}
    for nq in (1, 64, 1024):
        qa = torch.randint(0, n, (nq,), device=dev, generator=torch.Generator(device=dev).manual_seed(7))
        queries[nq] = (xb[qa] + 0.1 * sigma * synth.normal_f32(9, nq, D, dev)).contiguous()
    del xb
    torch.cuda.synchronize()
    return dev, ix, queries


def view_only(ix, q, words):
    """The pre-pass alone, as search() calls it (list-major scan: hx travels with the view)."""
    keep, cap = ix._keep(words)
    packed = ix._pack()
    _, probes = ix._quantizer.search_many(q, NPROBE)
    probes = probes.contiguous()
    hx = ix._lists_aux(q, *packed[:3])[1]
    return lambda: ix._select_view(q, probes, NPROBE, packed, keep, cap, hx)


def sweep(n, out):
    dev, ix, queries = setup(n)
    masks = selector_masks(n, dev)
    points = []
    for nq, q in queries.items():
        base = timed(lambda: ix.search(q, K))
        over = timed(lambda: ix.search(q, OVERFETCH))
        _, I32 = ix.search(q, OVERFETCH)
        p = dict(point="unfiltered", n=n, nq=nq, k=K, **base, overfetch32_median_ms=over["median_ms"])
        points.append(p)
        print(json.dumps(p), flush=True)
        for name, layout, mask in masks:
            words = pack(mask)
            total = timed(lambda: ix.search(q, K, sel=words))
            _, I = ix.search(q, K, sel=words)
            in_view = int(ix._view[6][1])
            view = timed(view_only(ix, q, words))
            # what an index without selectors delivers: the eligible ones among its 32 global neighbours, of 10 wanted
            ok = (I32 >= 0) & mask[I32.clamp(min=0)]
            delivered = ok.sum(1).clamp(max=K).float()
            found = (I >= 0).sum(1).float()
            p = dict(point="filtered", n=n, nq=nq, k=K, selector=name, layout=layout, eligible_rows=int(mask.sum()),
                     rows_in_view=in_view, **total, view_median_ms=view["median_ms"],
                     scan_median_ms=round(total["median_ms"] - view["median_ms"], 4),
                     vs_unfiltered=round(total["median_ms"] / base["median_ms"], 3),
                     results_per_query=round(float(found.mean()), 3),
                     overfetch32_results_per_query=round(float(delivered.mean()), 3),
                     overfetch32_queries_with_all_10=round(float((delivered >= K).float().mean()), 4),
                     ids_all_eligible=bool(mask[I[I >= 0]].all()), overflow_flag=int(ix.last_stats[0]))
            points.append(p)
            print(json.dumps(p), flush=True)
    meta = dict(device=_lib.device_info()["name"], n=n, d=D, nlist=NLIST, m=M, nprobe=NPROBE, k=K, reps=20, scan_mode=ix.scan_mode)
    json.dump({"meta": meta, "points": points}, open(out, "w"), indent=1)


def trace(n):
    dev, ix, queries = setup(n)
    words = pack(selector_masks(n, dev)[5][2])  # 1 % scattered
    for _ in range(3):
        ix.search(queries[64], K, sel=words)
    torch.cuda.synchronize()
    print("traced")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        trace(int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000)
    else:
        sweep(int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000,
              sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "ivfpq_filtered.json"))
