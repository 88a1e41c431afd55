"""Approximate kNN: ``IndexIVFPQ`` (FAISS semantics: L2, residual encoding, 8-bit codes) on the HIP kernels.

BASELINE.json cfg5 (IVF-PQ over 100M x 384, nlist 4096).  The reference itself holds intent only for
vector search (``.kiro/specs/semantic-video-search/design.md:35-40``).  Host orchestration - the
k-means / PQ training loops and the inverted-list bookkeeping - is Python here, as the north star
asks; every data-parallel step is a kernel of ``libeioku_hip``: coarse assignment and probe
selection = K9 (``k=1`` / ``k=nprobe``), centroid update = fixed-point atomics (bit-reproducible),
PQ assignment / encoding, counting-sort into lists, ADC scan with LUT in LDS, top-k merge.

Deviations from FAISS defaults, all deterministic: k-means initialises from
``default_rng(seed).permutation(n)[:k]``, an empty cluster keeps its previous centroid (FAISS splits
the largest), 25 iterations, at most 256 training points per centroid.

Multi-GPU build (BASELINE cfg5: 100M x 384 over 8 GPUs): ``train(x, group=...)`` trains the
quantisers on the union of every rank's rows with one integer all-reduce per k-means iteration; ``add`` /
``search`` stay local to the rank's row shard, and ``search.ShardedFlatL2(local=this index, id_base=...)`` merges
the per-rank results with the single all-gather of the flat index.

Row selectors and removal (K10f): ``search(q, k, sel=...)``, ``search_many``, ``remove_ids`` / ``nlive`` and ``close()`` have
the semantics of ``search.IndexFlatL2``; a filtered search scans a compact view of the probed lists that holds only the
eligible rows (``eioku_ivfpq_select_view``) with the scans of the unfiltered one.  ``store_index_factory`` puts the index
behind ``semantic.VectorStore``.
"""

from __future__ import annotations

import numpy as np

from . import _lib
from ._buffers import current_stream, ptr
from .search import IndexFlatL2, RowSelector, empty_results, selector_words

NITER = 25
MAX_K = 32  # results per query of one search (the partial lists of the scans are 16 or 32 wide)
_POP8 = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int64)  # bits set per byte
MAX_POINTS_PER_CENTROID = 256


def _sample(n: int, want: int, seed: int) -> np.ndarray:
    perm = np.random.default_rng(seed).permutation(n)
    return np.sort(perm[:want]) if want < n else np.arange(n)


class HipTrainOps:
    """The data-parallel steps of training on this rank's rows, on the HIP kernels.  (A seam: the world-size-2 gloo
    test drives :meth:`IndexIVFPQ.train` on CPU ranks with a numpy stand-in of the same integer arithmetic.)"""

    def __init__(self, device):
        self._lib = _lib.load()
        self.device = device

    def to_device(self, a):
        import torch

        return torch.as_tensor(a, dtype=torch.float32).to(self.device).contiguous()

    def take(self, x, idx):
        import torch

        return x[torch.from_numpy(np.asarray(idx)).to(x.device)].contiguous()

    def assign(self, x, cent):
        """nearest centroid of every row (int64): K9 with k = 1"""
        flat = IndexFlatL2(int(cent.shape[1]))
        flat.attach(cent)
        _, a = flat.search(x, 1)
        a = a.reshape(-1).contiguous()
        flat.close()
        return a

    def accumulate(self, x, assign, k):
        """int64 (k, d + 1): per-centroid sums of the assigned rows in 2^-32 fixed point, and the count in column d"""
        import torch

        n, d = (int(v) for v in x.shape)
        sums = torch.zeros((k, d), dtype=torch.int64, device=x.device)
        counts = torch.zeros((k,), dtype=torch.int32, device=x.device)
        _lib.check(self._lib.eioku_kmeans_accumulate(ptr(x), n, d, ptr(assign), k, ptr(sums), ptr(counts), current_stream(x)),
                   "eioku_kmeans_accumulate")
        return torch.cat([sums, counts.to(torch.int64)[:, None]], 1).contiguous()

    def finalize(self, packed, cent):
        """centroids <- sums / counts (a centroid without rows keeps its value); in place"""
        import torch

        k, d = (int(v) for v in cent.shape)
        sums = packed[:, :d].contiguous()
        counts = packed[:, d].to(torch.int32).contiguous()
        _lib.check(self._lib.eioku_kmeans_finalize(ptr(sums), ptr(counts), k, d, ptr(cent), current_stream(cent)),
                   "eioku_kmeans_finalize")
        return cent

    def residuals(self, x, coarse, lst, m):
        import torch

        resid = torch.empty_like(x)
        dummy = torch.zeros((m, 256, x.shape[1] // m), dtype=torch.float32, device=x.device)
        _lib.check(self._lib.eioku_pq_assign(ptr(x), x.shape[0], x.shape[1], m, ptr(coarse), ptr(lst), ptr(dummy), None, ptr(resid),
                                             current_stream(x)), "eioku_pq_assign(residual)")
        return resid

    def pq_codes(self, resid, pq):
        import torch

        n, d = (int(v) for v in resid.shape)
        codes = torch.empty((n, pq.shape[0]), dtype=torch.uint8, device=resid.device)
        _lib.check(self._lib.eioku_pq_assign(ptr(resid), n, d, int(pq.shape[0]), None, None, ptr(pq), ptr(codes), None,
                                             current_stream(resid)), "eioku_pq_assign(train)")
        return codes

    def column(self, x, lo, hi):
        return x[:, lo:hi].contiguous()

    def codes_column(self, codes, j):
        import torch

        return codes[:, j].to(torch.int64).contiguous()


class IndexIVFPQ:
    def __init__(self, d: int, nlist: int, m: int, nbits: int = 8, device=None, seed: int = 1234, train_ops=None):
        import torch

        if nbits != 8:
            raise ValueError("only 8-bit PQ codes are supported")
        if d % m or d // m not in (4, 8, 16):
            raise ValueError("d/m must be 4, 8 or 16")
        self.d, self.nlist, self.m, self.dsub, self.seed = d, nlist, m, d // m, seed
        self.nprobe = 1
        if train_ops is None:
            self._lib = _lib.load()
            _lib.init()
            self.device = device or torch.device("cuda", torch.cuda.current_device())
            train_ops = HipTrainOps(self.device)
        else:
            self._lib = None
            self.device = device
        self._ops = train_ops
        self.is_trained = False
        self.coarse = None          # (nlist, d) float32 cuda
        self.pq = None              # (m, 256, dsub) float32 cuda
        self._quantizer = None      # IndexFlatL2 over the coarse centroids
        self._pending = []          # (list int64, codes uint8, id_base) per add() batch
        self.ntotal = 0
        self._packed = None
        self.use_precomputed_table = True   # FAISS' IndexIVFPQ.use_precomputed_table; False = tables from the codebook per (query, list)
        self._list_tables = None
        # "lists": the list-major scan (codes cross HBM once per search, MFMA filter + exact re-rank; same (D, I) bits as
        # "queries"); "queries": one workgroup per (query, probe).  "lists" needs d/m = 8, d in {64, 128, 256, 384} and the
        # precomputed tables; other geometries always take "queries".
        self.scan_mode = "lists"
        self.cand_cap = 8192                # per-query candidate capacity of the list-major filter (overflow -> query-major redo)
        self._aux = None                    # (pqh, hx, pmax2) of the current pack
        self._ws = None
        self.last_stats = None              # device int32[6] after a list-major search: overflow bits, work items, largest candidate list, candidates in all, its query, its size
        self.allreduce_calls = 0
        # row selectors and removal (K10f): see search()
        self._live = None                   # device int32 words by id, bit set = not removed; None until remove_ids()
        self._nremoved = 0
        self._view = None                   # (capacity in rows, v_offsets, v_sizes, v_codes, v_ids, v_hx, status): kept and grown like _ws
        self.last_view = None               # (v_offsets, v_sizes, v_codes, v_ids) of the last filtered search, None after an unfiltered one

    # ---- training ------------------------------------------------------------------------------
    def _allreduce(self, packed, group):
        """Sum the integer (sums | counts) table over the ranks of ``group`` (RCCL on GPUs): exact and order
        independent, so every rank - and a single-GPU run over the same rows - finalises the same centroids."""
        if group is None:
            return packed
        import torch.distributed as dist

        dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=group)
        self.allreduce_calls += 1
        return packed

    def _bcast(self, t, group):
        if group is not None:
            import torch.distributed as dist

            dist.broadcast(t, src=dist.get_global_rank(group, 0) if hasattr(dist, "get_global_rank") else 0, group=group)
        return t

    def _kmeans(self, x, k: int, seed: int, group=None):
        """Lloyd iterations on this rank's (n,d) rows -> (k,d) centroids shared by every rank of ``group``:
        assignment on the MFMA flat kernel, one all-reduce of k x (d + 1) int64 per iteration."""
        ops = self._ops
        n = int(x.shape[0])
        init = np.sort(np.random.default_rng(seed).permutation(n)[:k])
        cent = self._bcast(ops.take(x, init).clone(), group)  # rank 0's picks seed every rank
        for _ in range(NITER):
            packed = self._allreduce(ops.accumulate(x, ops.assign(x, cent), k), group)
            cent = ops.finalize(packed, cent)
        return cent

    def train(self, x, group=None) -> None:
        """``x``: float32 (n,d) rows of THIS rank (numpy array or CUDA tensor).  ``group``: a ``torch.distributed``
        group (RCCL on GPUs) whose ranks each hold a shard of the training rows: the quantisers are trained on the
        union - per k-means iteration ONE all-reduce of ``nlist x (d + 1)`` (coarse) / ``m x 256 x (dsub + 1)`` (PQ)
        integers - and come out identical on every rank."""
        ops = self._ops
        x = ops.to_device(x)
        n = int(x.shape[0])
        if n < max(self.nlist, 256):
            raise ValueError(f"need at least max(nlist={self.nlist}, 256) training vectors on every rank (the k-means seeds), got {n}")
        xs = ops.take(x, _sample(n, MAX_POINTS_PER_CENTROID * self.nlist, self.seed))
        self.coarse = self._kmeans(xs, self.nlist, self.seed + 1, group)
        # PQ on residuals of (at most 65536 per rank) training vectors
        xp = ops.take(x, _sample(n, MAX_POINTS_PER_CENTROID * 256, self.seed + 2))
        lst = ops.assign(xp, self.coarse)
        resid = ops.residuals(xp, self.coarse, lst, self.m)
        npq = int(resid.shape[0])
        init = np.sort(np.random.default_rng(self.seed + 3).permutation(npq)[:256])
        pq = self._bcast(ops.take(resid, init).reshape(256, self.m, self.dsub).permute(1, 0, 2).contiguous(), group)
        import torch

        for _ in range(NITER):
            codes = ops.pq_codes(resid, pq)
            packed = torch.stack([ops.accumulate(ops.column(resid, j * self.dsub, (j + 1) * self.dsub),
                                                 ops.codes_column(codes, j), 256) for j in range(self.m)])
            packed = self._allreduce(packed.contiguous(), group)  # (m, 256, dsub + 1): one collective for all sub-quantisers
            pq = torch.stack([ops.finalize(packed[j], pq[j].contiguous()) for j in range(self.m)]).contiguous()
        self.pq = pq
        self._codebooks_changed()

    def set_codebooks(self, coarse, pq) -> None:
        """Install trained quantisers (e.g. broadcast from rank 0): coarse (nlist,d), pq (m,256,dsub)."""
        import torch

        self.coarse = torch.as_tensor(coarse, dtype=torch.float32).to(self.device).contiguous()
        self.pq = torch.as_tensor(pq, dtype=torch.float32).to(self.device).contiguous()
        self._codebooks_changed()

    def _invalidate(self, tables: bool) -> None:
        """New rows outdate the pack, new codebooks (``tables``) the per-list tables; both outdate the pack's aux planes."""
        self._aux = None
        if tables:
            self._list_tables = None
        else:
            self._packed = None

    def _codebooks_changed(self) -> None:
        self._invalidate(tables=True)
        if self._lib is not None:  # the coarse quantiser: a flat index over the new centroids (HIP ops only)
            self.close()
            self._quantizer = IndexFlatL2(self.d)
            self._quantizer.attach(self.coarse)
        self.is_trained = True

    # ---- add / search --------------------------------------------------------------------------------
    def add(self, x) -> None:
        import torch

        if not self.is_trained:
            raise RuntimeError("train() or set_codebooks() first")
        x = torch.as_tensor(x, dtype=torch.float32).to(self.device).contiguous()
        n = x.shape[0]
        if n == 0:
            return
        _, lst = self._quantizer.search(x, 1)
        lst = lst.reshape(-1).contiguous()
        codes = torch.empty((n, self.m), dtype=torch.uint8, device=self.device)
        _lib.check(self._lib.eioku_pq_assign(ptr(x), n, self.d, self.m, ptr(self.coarse), ptr(lst), ptr(self.pq), ptr(codes),
                                             None, current_stream(x)), "eioku_pq_assign(encode)")
        self._pending.append((lst, codes, self.ntotal))
        self.ntotal += n
        self._invalidate(tables=False)
        if self._live is not None:  # fresh ids are live; the bits beyond ntotal in the last word are kept set
            grow = (self.ntotal + 31) // 32 - int(self._live.numel())
            if grow > 0:
                self._live = torch.cat([self._live, torch.full((grow,), -1, dtype=torch.int32, device=self.device)])

    def _pack(self):
        """Counting sort of everything added so far into contiguous inverted lists."""
        import torch

        if self._packed is not None:
            return self._packed
        counts = torch.zeros((self.nlist,), dtype=torch.int32, device=self.device)
        tmp = torch.empty_like(counts)
        for lst, _, _ in self._pending:
            _lib.check(self._lib.eioku_ivf_histogram(ptr(lst), lst.numel(), self.nlist, ptr(tmp), current_stream(lst)),
                       "eioku_ivf_histogram")
            counts += tmp
        offsets = (torch.cumsum(counts, 0) - counts).to(torch.int32).contiguous()
        cursor = offsets.clone()
        list_codes = torch.empty((max(self.ntotal, 1), self.m), dtype=torch.uint8, device=self.device)
        list_ids = torch.empty((max(self.ntotal, 1),), dtype=torch.int64, device=self.device)
        for lst, codes, base in self._pending:
            _lib.check(self._lib.eioku_ivf_scatter(ptr(lst), lst.numel(), self.m, ptr(codes), base, ptr(cursor),
                                                   ptr(list_codes), ptr(list_ids), current_stream(lst)), "eioku_ivf_scatter")
        self._packed = (offsets, counts.contiguous(), list_codes, list_ids)
        return self._packed

    # ---- row selectors and removal (K10f) ---------------------------------------------------------------
    @property
    def nlive(self) -> int:
        """Rows a search can return: ``ntotal`` minus the rows taken out by :meth:`remove_ids`."""
        return self.ntotal - self._nremoved

    def remove_ids(self, ids) -> int:
        """Take rows out of every later search; returns how many were live until now (as ``IndexFlatL2.remove_ids``).

        Ids never shift: ``ntotal`` stays, later ``add()`` calls continue with fresh ids.  Unknown and repeated ids are
        ignored.  Removal is a bitmap by id on the device: nothing is re-encoded or re-packed, and a later ``add()``
        (which re-packs the lists) leaves it as it is.  ``ids``: int64 numpy array / sequence, or a CUDA int64 tensor."""
        import torch

        if not torch.is_tensor(ids):
            ids = torch.from_numpy(np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1)))
        ids = ids.to(self.device, torch.int64).reshape(-1)
        ids = torch.unique(ids[(ids >= 0) & (ids < self.ntotal)])
        if ids.numel() == 0:
            return 0
        nwords = (self.ntotal + 31) // 32
        if self._live is None:
            self._live = torch.full((nwords,), -1, dtype=torch.int32, device=self.device)
        word, bit = ids >> 5, ids & 31
        gone = int(((self._live[word].to(torch.int64) >> bit) & 1).sum())
        # distinct bits of one word add up without carries: the sum IS their OR
        clear = torch.zeros((nwords,), dtype=torch.int64, device=self.device).index_add_(0, word, torch.ones_like(bit) << bit)
        clear = torch.where(clear >= 2 ** 31, clear - 2 ** 32, clear).to(torch.int32)
        self._live = self._live & ~clear
        self._nremoved += gone
        return gone

    def _keep(self, sel):
        """-> (device int32 words ``selector AND NOT removed`` by id, capacity in rows of the view), or ``(None, 0)``
        when every row is eligible.  The capacity is what the host knows without asking the device: the bits set in a host
        selector, else ``ntotal``."""
        import torch

        words, _, mem = selector_words(sel, self.ntotal)  # the selector forms and the ValueError texts of the flat index
        if words is None or self.ntotal == 0:
            return (self._live, self.ntotal) if self._live is not None and self.ntotal else (None, 0)
        cap = self.ntotal
        if mem == _lib.MEM_HOST:
            cap = min(cap, int(_POP8[words.view(np.uint8)].sum()))
            words = torch.from_numpy(words.view(np.int32)).to(self.device)
        elif words.dtype != torch.int32:
            words = words.view(torch.int32)
        return (words if self._live is None else words & self._live), cap

    def _select_view(self, q, probes, nprobe, pack, keep, cap, hx):
        """``eioku_ivfpq_select_view``: the eligible rows of the probed lists as a compact pack (+ their ``hx``)."""
        import torch

        if self._view is None or self._view[0] < cap or self._view[3].shape[1] != self.m or self._view[1].numel() != self.nlist:
            rows = max(cap, 1)
            self._view = (cap, torch.empty((self.nlist,), dtype=torch.int32, device=self.device),
                          torch.empty((self.nlist,), dtype=torch.int32, device=self.device),
                          torch.empty((rows, self.m), dtype=torch.uint8, device=self.device),
                          torch.empty((rows,), dtype=torch.int64, device=self.device),
                          torch.empty((rows,), dtype=torch.float32, device=self.device),
                          torch.zeros((2,), dtype=torch.int32, device=self.device))
        _, v_offsets, v_sizes, v_codes, v_ids, v_hx, status = self._view
        offsets, sizes, list_codes, list_ids = pack
        _lib.check(self._lib.eioku_ivfpq_select_view(ptr(probes), int(q.shape[0]), nprobe, self.nlist, self.m, self.ntotal,
                                                     ptr(offsets), ptr(sizes), ptr(list_codes), ptr(list_ids),
                                                     None if hx is None else ptr(hx), ptr(keep), cap, ptr(v_offsets),
                                                     ptr(v_sizes), ptr(v_codes), ptr(v_ids), None if hx is None else ptr(v_hx),
                                                     ptr(status), current_stream(q)), "eioku_ivfpq_select_view")
        self.last_view = (v_offsets, v_sizes, v_codes, v_ids)
        return (v_offsets, v_sizes, v_codes, v_ids), (None if hx is None else v_hx)

    def search(self, q, k: int, sel=None):
        """(D, I) CUDA tensors: approximate squared L2 (ADC) ascending, int64 ids (-1 = fewer than k found).

        ``sel``: optional :class:`eioku_amd.search.RowSelector`, packed ``uint32`` host words or a contiguous CUDA int32 /
        uint32 tensor over ``ntotal`` rows (what ``IndexFlatL2.search`` accepts; one selector serves all queries).  The
        probes are chosen as without it; the answer is the k best by (distance, id) among the rows of the probed lists
        whose bit is set and which were not removed, ``(FLT_MAX, -1)`` padding.  A row's distance bits do not depend on
        the selector.  With a selector or after :meth:`remove_ids` the scan of the current ``scan_mode`` runs on the
        selected view of the probed lists (``last_view``); otherwise on the lists as they are (``last_view`` is None)."""
        import torch

        q = torch.as_tensor(q, dtype=torch.float32).to(self.device).contiguous()
        nq = q.shape[0]
        nprobe = min(self.nprobe, self.nlist)
        keep, cap = self._keep(sel)
        pack = self._pack()
        _, probes = self._quantizer.search_many(q, nprobe)  # nprobe > 32: chained rounds of 32 (search_after)
        probes = probes.contiguous()
        lists = (self.scan_mode == "lists" and self.use_precomputed_table and self.dsub == 8
                 and self.d in (64, 128, 256, 384) and self.ntotal > 0)
        if self.use_precomputed_table:
            # FAISS' decomposition: the per-list half of every look-up table is part of the index (nlist x m x 1 KB, built
            # on the first search after the codebooks change), the per-query half is built once per search
            if self._list_tables is None:
                self._list_tables = torch.empty((self.nlist, self.m, 256), dtype=torch.float32, device=self.device)
                _lib.check(self._lib.eioku_ivfpq_tables(ptr(self.coarse), self.nlist, self.d, self.m, ptr(self.pq), 1.0, 2.0,
                                                        ptr(self._list_tables), current_stream(q)), "eioku_ivfpq_tables")
            qt = torch.empty((nq, self.m, 256), dtype=torch.float32, device=self.device)
            _lib.check(self._lib.eioku_ivfpq_tables(ptr(q), nq, self.d, self.m, ptr(self.pq), 0.0, -2.0, ptr(qt),
                                                    current_stream(q)), "eioku_ivfpq_tables")
        hx = None
        if keep is None:
            self.last_view = None
        else:  # the scans below run unchanged on the eligible rows of the probed lists
            if lists:
                hx = self._lists_aux(q, *pack[:3])[1]
            pack, hx = self._select_view(q, probes, nprobe, pack, keep, cap, hx)
        head, tail = self._scan_args(q, probes, nprobe, pack)
        if lists:
            return self._search_lists(q, k, nprobe, head, tail, pack, qt, hx)
        K = 16 if k <= 16 else 32
        pd = torch.empty((nprobe, nq, K), dtype=torch.float32, device=self.device)
        pi = torch.empty((nprobe, nq, K), dtype=torch.int64, device=self.device)
        if self.use_precomputed_table:
            _lib.check(self._lib.eioku_ivfpq_scan_tables(*head, *tail, ptr(self._list_tables), ptr(qt), k, ptr(pd), ptr(pi),
                                                         current_stream(q)), "eioku_ivfpq_scan_tables")
        else:
            _lib.check(self._lib.eioku_ivfpq_scan(*head, *tail, k, ptr(pd), ptr(pi), current_stream(q)), "eioku_ivfpq_scan")
        D, I = empty_results(q, nq, k)
        _lib.check(self._lib.eioku_topk_merge_ex(ptr(pd), ptr(pi), nprobe, nq, K, k, ptr(D), ptr(I), current_stream(q)),
                   "eioku_topk_merge_ex")
        return D, I

    def _scan_args(self, q, probes, nprobe, pack):
        """The arguments every scan entry point takes, in their order: (q, nq, d, m, probes, nprobe) and (coarse, pq, the
        four tensors of the pack); ``eioku_ivfpq_search_lists`` puts nlist and ntotal between the two."""
        return ((ptr(q), int(q.shape[0]), self.d, self.m, ptr(probes), nprobe),
                (ptr(self.coarse), ptr(self.pq), *(ptr(t) for t in pack)))

    def search_many(self, q, k: int, sel=None):
        """:meth:`search` behind the protocol ``VectorStore`` speaks (``IndexFlatL2.search_many``): numpy queries give
        numpy results and the call is synchronous, CUDA queries give CUDA results.  ``k`` is at most 32: chained rounds
        are not built for IVF-PQ."""
        if k > MAX_K:
            raise ValueError(f"IndexIVFPQ returns at most {MAX_K} results per query (k <= {MAX_K}), got k = {k}")
        import torch

        host = not torch.is_tensor(q)
        D, I = self.search(q, k, sel)
        if not host:
            return D, I
        D, I = D.cpu().numpy(), I.cpu().numpy()
        if self.last_view is not None and int(self._view[6][0]) != 0:
            raise _lib.EiokuHipError(f"eioku_ivfpq_select_view: {int(self._view[6][1])} eligible rows do not fit the "
                                     f"view's {self._view[0]}")
        return D, I

    def close(self) -> None:
        """Release the coarse quantiser's handle; idempotent."""
        if self._quantizer is not None:
            self._quantizer.close()
            self._quantizer = None

    def _lists_aux(self, q, offsets, sizes, list_codes):
        """(pqh, hx, pmax2) of the current pack (``eioku_ivfpq_lists_aux``), built once per pack / codebook change."""
        import torch

        if self._aux is None:
            pqh = torch.empty((self.m * 256, 4), dtype=torch.int32, device=self.device)
            hx = torch.empty((max(self.ntotal, 1),), dtype=torch.float32, device=self.device)
            pmax2 = torch.empty((self.nlist,), dtype=torch.float32, device=self.device)
            _lib.check(self._lib.eioku_ivfpq_lists_aux(ptr(list_codes), ptr(offsets), ptr(sizes), self.nlist, self.d, self.m,
                                                       ptr(self._list_tables), ptr(self.pq), ptr(pqh), ptr(hx), ptr(pmax2),
                                                       current_stream(q)), "eioku_ivfpq_lists_aux")
            self._aux = (pqh, hx, pmax2)
        return self._aux

    def _search_lists(self, q, k, nprobe, head, tail, pack, qt, view_hx=None):
        """The list-major scan (``eioku_ivfpq_search_lists``): one C call enqueues the whole search.  ``view_hx``: the
        lists are a selected view and this is its ``hx`` (``pqh`` and ``pmax2`` stay the pack's)."""
        import torch

        nq = int(q.shape[0])
        if view_hx is None:
            pqh, hx, pmax2 = self._lists_aux(q, *pack[:3])
        else:
            pqh, _, pmax2 = self._aux
            hx = view_hx
        need = int(self._lib.eioku_ivfpq_lists_workspace(nq, self.d, nprobe, self.nlist, self.ntotal, k, self.cand_cap))
        if need < 0:
            raise _lib.EiokuHipError("eioku_ivfpq_lists_workspace: bad argument")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty((need,), dtype=torch.uint8, device=self.device)
        D, I = empty_results(q, nq, k)
        stats = torch.zeros((6,), dtype=torch.int32, device=self.device)
        _lib.check(self._lib.eioku_ivfpq_search_lists(*head, self.nlist, self.ntotal, *tail, ptr(self._list_tables), ptr(qt),
                                                      ptr(pqh), ptr(hx), ptr(pmax2), k, self.cand_cap, ptr(self._ws),
                                                      self._ws.numel(), ptr(D), ptr(I), ptr(stats), current_stream(q)),
                   "eioku_ivfpq_search_lists")
        self.last_stats = stats
        return D, I


class _StoreIVFPQ(IndexIVFPQ):
    """What :func:`store_index_factory` builds: an :class:`IndexIVFPQ` that trains on the rows of its first ``add``."""

    def add(self, x) -> None:
        if not self.is_trained:
            self.train(x)  # ValueError when there are fewer than max(nlist, 256) rows
        super().add(x)


def store_index_factory(nlist: int, m: int, nprobe: int, seed: int = 1234):
    """``d -> index`` for ``VectorStore(index_factory=...)``: an IVF-PQ index (``nlist`` inverted lists, ``m`` 8-bit
    sub-quantisers, ``nprobe`` lists scanned per query) behind the protocol the store speaks - ``add(numpy)``, ``ntotal``,
    ``remove_ids``, ``search_many(numpy q, k, sel=RowSelector)`` (k <= 32) and ``close()``.

    The index is untrained when the store builds it and trains on the rows of its first ``add`` - the store adds its
    whole matrix first, so that is the library; fewer than ``max(nlist, 256)`` rows raise ``train``'s ``ValueError``.
    When the store rebuilds its device index (removed rows outnumber the live ones) the new index trains again."""
    for name, v in (("nlist", nlist), ("m", m), ("nprobe", nprobe)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"{name} must be a positive integer, got {v!r}")
    if nprobe > nlist:
        raise ValueError(f"nprobe = {nprobe} exceeds nlist = {nlist}")
    nlist, m, nprobe, seed = int(nlist), int(m), int(nprobe), int(seed)

    def build(d: int):
        if d % m or d // m not in (4, 8, 16):
            raise ValueError(f"d/m must be 4, 8 or 16 (d = {d}, m = {m})")
        ix = _StoreIVFPQ(int(d), nlist, m, seed=seed)
        ix.nprobe = nprobe
        return ix

    return build
