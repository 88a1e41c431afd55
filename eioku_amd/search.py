"""Semantic-search stage: exact kNN over segment embeddings (FAISS ``IndexFlatL2`` surface).

The reference never built this stage (``.kiro/specs/semantic-video-search/tasks.md:304-313`` is
unchecked; the design names a FAISS index over 384-d all-MiniLM-L6-v2 vectors,
``design.md:35-40,1105-1113``), so the interface mirrored here is the FAISS one BASELINE.json's
north_star names: ``add(x)``, ``search(q, k) -> (D, I)`` with squared-L2 distances ascending, int64
ids, ``-1`` padding, ``ntotal``, ``reset()``.

Multi-GPU: rows are sharded across ranks, every rank searches its shard with the
same replicated queries, ONE all-gather (RCCL over xGMI) moves ``nq*k*(4+8)`` bytes per rank and
every rank merges the ``world*k`` candidates locally (``eioku_topk_merge``).
"""

from __future__ import annotations

import numpy as np

from . import _lib
from ._buffers import current_stream, mem_flag, on_device, ptr
from ._handle import Handle


class RowSelector:
    """Which rows a search may return: ``ceil(n/32)`` little-endian 32-bit words, bit ``r % 32`` of word ``r // 32`` set =
    row ``r`` eligible (one word = one 32-row MFMA tile of the kNN kernels).  Packed on the host with numpy; one
    selector serves all queries of a call (FAISS ``SearchParameters.sel``)."""

    def __init__(self, words: np.ndarray, n: int):
        words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        if words.shape[0] != (int(n) + 31) // 32:
            raise ValueError(f"a selector over {n} rows has {(int(n) + 31) // 32} words, got {words.shape[0]}")
        self.words, self.n = words, int(n)

    @classmethod
    def from_mask(cls, mask) -> "RowSelector":
        mask = np.asarray(mask, dtype=bool).reshape(-1)
        n = mask.shape[0]
        padded = np.zeros(((n + 31) // 32) * 32, dtype=bool)
        padded[:n] = mask
        return cls(np.packbits(padded, bitorder="little").view(np.uint32), n)

    @classmethod
    def from_ids(cls, ids, n: int) -> "RowSelector":
        """Ids outside ``[0, n)`` are ignored; repeats are harmless."""
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        mask = np.zeros(int(n), dtype=bool)
        mask[ids[(ids >= 0) & (ids < n)]] = True
        return cls.from_mask(mask)

    @classmethod
    def from_ranges(cls, ranges, n: int) -> "RowSelector":
        """Half-open row ranges ``[(lo, hi), ...]``, clipped to ``[0, n)``."""
        mask = np.zeros(int(n), dtype=bool)
        for lo, hi in ranges:
            mask[max(0, int(lo)):max(0, min(int(n), int(hi)))] = True
        return cls.from_mask(mask)

    def to_mask(self) -> np.ndarray:
        return np.unpackbits(self.words.view(np.uint8), bitorder="little")[:self.n].astype(bool)

    def count(self) -> int:
        return int(self.to_mask().sum())


def selector_words(sel, ntotal: int):
    """-> (keep-alive object, pointer, mem flag) of a selector argument, length-checked against ``ntotal`` rows."""
    if sel is None:
        return None, None, _lib.MEM_HOST
    nwords = (ntotal + 31) // 32
    if isinstance(sel, RowSelector):
        if sel.n != ntotal:
            raise ValueError(f"selector covers {sel.n} rows, the index holds {ntotal}")
        sel = sel.words
    if on_device(sel):
        import torch

        if sel.dtype not in (torch.int32, torch.uint32) or sel.dim() != 1 or not sel.is_contiguous():
            raise ValueError("a device selector is a contiguous 1-d int32 / uint32 tensor of packed words")
        if int(sel.numel()) != nwords:
            raise ValueError(f"a selector over {ntotal} rows has {nwords} words, got {int(sel.numel())}")
        return sel, ptr(sel), _lib.MEM_DEVICE
    sel = np.asarray(sel)
    if sel.dtype != np.uint32 or sel.ndim != 1:
        raise ValueError("a host selector is a 1-d uint32 array of packed words (see RowSelector)")
    if sel.shape[0] != nwords:
        raise ValueError(f"a selector over {ntotal} rows has {nwords} words, got {sel.shape[0]}")
    sel = np.ascontiguousarray(sel)
    if nwords == 0:
        return None, None, _lib.MEM_HOST
    return sel, ptr(sel), _lib.MEM_HOST


def empty_results(q, nq: int, k: int):
    """Uninitialised ``(D, I)``, float32 and int64 ``(nq, k)``, on the side of PCIe that ``q`` is on."""
    if on_device(q):
        import torch

        return (torch.empty((nq, k), dtype=torch.float32, device=q.device),
                torch.empty((nq, k), dtype=torch.int64, device=q.device))
    return np.empty((nq, k), dtype=np.float32), np.empty((nq, k), dtype=np.int64)


class IndexFlatL2:
    """Exact squared-L2 index resident in HBM (d in {64,128,256,384,512}, k <= 32)."""

    def __init__(self, d: int):
        self.d = int(d)
        self._h = Handle("index", self.d, create="eioku_index_flat_create")
        self._attached = None  # keeps an attached tensor alive

    @property
    def ntotal(self) -> int:
        return int(self._h.eioku_index_ntotal())

    @property
    def nlive(self) -> int:
        """Rows a search can return: ``ntotal`` minus the rows taken out by :meth:`remove_ids`."""
        return int(self._h.eioku_index_nlive())

    def remove_ids(self, ids) -> int:
        """Take rows out of every later search without rebuilding anything; returns how many were live until now.

        Ids never shift (unlike FAISS ``remove_ids``): ``ntotal`` stays, later ``add()`` calls continue with fresh ids.
        Unknown and repeated ids are ignored.  ``ids``: int64 numpy array / sequence, or a CUDA int64 tensor."""
        before = self.nlive
        if on_device(ids):
            import torch

            ids = ids.to(torch.int64).contiguous().view(-1)
            n_ids, mem = int(ids.numel()), _lib.MEM_DEVICE
        else:
            ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
            n_ids, mem = int(ids.shape[0]), _lib.MEM_HOST
        if n_ids:
            _lib.check(self._h.eioku_index_remove_ids(ptr(ids), n_ids, mem, current_stream(ids)),
                       "eioku_index_remove_ids")
        return before - self.nlive

    def add(self, x) -> None:
        """Append vectors: float32 ``(n,d)`` numpy (staged over PCIe) or CUDA tensor (device copy)."""
        n, d = (int(s) for s in x.shape)
        if d != self.d:
            raise ValueError(f"expected dimension {self.d}, got {d}")
        if not on_device(x):
            x = np.ascontiguousarray(x, dtype=np.float32)
        _lib.check(self._h.eioku_index_add(ptr(x), n, _lib.MEM_DEVICE if on_device(x) else _lib.MEM_HOST,
                                           current_stream(x)), "eioku_index_add")

    def attach(self, x_cuda) -> None:
        """Search an existing CUDA float32 ``(n,d)`` tensor in place (no copy; the tensor must outlive the index)."""
        n, d = (int(s) for s in x_cuda.shape)
        if d != self.d or not on_device(x_cuda):
            raise ValueError("attach() needs a CUDA tensor of shape (n, d)")
        _lib.check(self._h.eioku_index_attach(ptr(x_cuda), n, current_stream(x_cuda)), "eioku_index_attach")
        self._attached = x_cuda

    def reset(self) -> None:
        _lib.check(self._h.eioku_index_reset(), "eioku_index_reset")
        self._attached = None

    def search(self, q, k: int, sel=None):
        """``(D, I)``: float32 ``(nq,k)`` squared distances ascending, int64 ``(nq,k)`` ids (-1 = none).

        numpy queries -> numpy results (synchronous); CUDA queries -> CUDA results (asynchronous).
        ``sel``: optional :class:`RowSelector` or packed ``uint32`` words (numpy, or a CUDA int32 / uint32 tensor): only
        live rows whose bit is set are candidates.
        """
        nq, d = (int(s) for s in q.shape)
        if d != self.d:
            raise ValueError(f"expected dimension {self.d}, got {d}")
        if sel is not None:
            return self._search_sel(q, k, sel, None, None)
        if not on_device(q):
            q = np.ascontiguousarray(q, dtype=np.float32)
        D, I = empty_results(q, nq, k)
        _lib.check(self._h.eioku_index_search(ptr(q), nq, int(k), ptr(D), ptr(I), mem_flag(q), current_stream(q)),
                   "eioku_index_search")
        return D, I

    def _search_sel(self, q, k: int, sel, after_D, after_I):
        """``eioku_index_search_sel``: selector and (optional) ``search_after`` bound in one call."""
        nq = int(q.shape[0])
        keep, sel_ptr, sel_mem = selector_words(sel, self.ntotal)
        if on_device(q):
            import torch

            if after_D is not None:
                after_D = after_D.to(torch.float32).contiguous()
                after_I = after_I.to(torch.int64).contiguous()
            mem = _lib.MEM_DEVICE
        else:
            q = np.ascontiguousarray(q, dtype=np.float32)
            if after_D is not None:
                after_D = np.ascontiguousarray(after_D, dtype=np.float32)
                after_I = np.ascontiguousarray(after_I, dtype=np.int64)
            mem = _lib.MEM_HOST
        D, I = empty_results(q, nq, k)
        _lib.check(self._h.eioku_index_search_sel(ptr(q), nq, int(k), sel_ptr, sel_mem,
                                                  None if after_D is None else ptr(after_D),
                                                  None if after_I is None else ptr(after_I), ptr(D), ptr(I), mem,
                                                  current_stream(q)), "eioku_index_search_sel")
        del keep
        return D, I

    def search_after(self, q, k: int, after_D, after_I, sel=None):
        """The next ``k`` results after a previous answer: rows with ``(distance, id) > (after_D[q], after_I[q])``
        in the result order (``after_*``: shape ``(nq,)``, same side of PCIe as ``q``); ``sel`` as in :meth:`search`."""
        nq, d = (int(s) for s in q.shape)
        if d != self.d:
            raise ValueError(f"expected dimension {self.d}, got {d}")
        if sel is not None:
            return self._search_sel(q, k, sel, after_D, after_I)
        if on_device(q):
            import torch

            after_D = after_D.to(torch.float32).contiguous()
            after_I = after_I.to(torch.int64).contiguous()
            mem = _lib.MEM_DEVICE
        else:
            q = np.ascontiguousarray(q, dtype=np.float32)
            after_D = np.ascontiguousarray(after_D, dtype=np.float32)
            after_I = np.ascontiguousarray(after_I, dtype=np.int64)
            mem = _lib.MEM_HOST
        D, I = empty_results(q, nq, k)
        _lib.check(self._h.eioku_index_search_after(ptr(q), nq, int(k), ptr(after_D), ptr(after_I), ptr(D),
                                                    ptr(I), mem, current_stream(q)), "eioku_index_search_after")
        return D, I

    def search_many(self, q, k: int, sel=None):
        """``search`` for any ``k``: rounds of at most 32 results chained with :meth:`search_after`."""
        if k <= 32:
            return self.search(q, k, sel)
        parts_d, parts_i = [], []
        got = 0
        while got < k:
            kk = min(32, k - got)
            if not parts_d:
                D, I = self.search_after(q, kk, *self._before_everything(q), sel=sel)
            else:
                D, I = self.search_after(q, kk, parts_d[-1][:, -1], parts_i[-1][:, -1], sel=sel)
            parts_d.append(D)
            parts_i.append(I)
            got += kk
        if on_device(q):
            import torch

            return torch.cat(parts_d, 1), torch.cat(parts_i, 1)
        return np.concatenate(parts_d, 1), np.concatenate(parts_i, 1)

    @staticmethod
    def _before_everything(q):
        nq = int(q.shape[0])
        if on_device(q):
            import torch

            return (torch.full((nq,), -1.0, dtype=torch.float32, device=q.device),
                    torch.full((nq,), -1, dtype=torch.int64, device=q.device))
        return np.full((nq,), -1.0, np.float32), np.full((nq,), -1, np.int64)

    def set_param(self, name: str, value: int) -> None:
        """Knobs of the search paths (``eioku_index_set_param``): scan_mode, scan_cap, scan_min_rows, ..., sel_list_ppm."""
        _lib.check(self._h.eioku_index_set_param(name.encode(), int(value)), f"eioku_index_set_param({name})")

    def close(self):
        self._h.close()


def merge_topk(d_lists, i_lists, k: int):
    """HIP merge of per-shard results: CUDA ``(L,nq,k)`` float32 / int64 (global ids) -> ``(nq,k)``."""
    if not on_device(d_lists):
        raise _lib.EiokuHipError("merge_topk runs on the GPU (eioku_topk_merge); got host tensors")
    lib = _lib.load()
    _lib.init()
    L, nq, kk = (int(s) for s in d_lists.shape)
    assert kk == k and tuple(i_lists.shape) == (L, nq, k)
    D, I = empty_results(d_lists, nq, k)
    _lib.check(lib.eioku_topk_merge(ptr(d_lists.contiguous()), ptr(i_lists.contiguous()), L, nq, k, ptr(D), ptr(I),
                                    current_stream(d_lists)), "eioku_topk_merge")
    return D, I


def shard_bounds(n_total: int, world: int, rank: int) -> tuple[int, int]:
    """Rows ``[lo, hi)`` of rank ``rank``: contiguous, sizes differ by at most one."""
    base, rem = divmod(n_total, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


class ShardedFlatL2:
    """Row-sharded exact index: local shard search + one all-gather + local merge.

    ``local`` is this rank's shard (anything with ``search(q, k) -> (D, I)`` of torch tensors and local
    ids); ``id_base`` the global id of its first row.  ``group`` is a ``torch.distributed`` group whose
    backend is RCCL ("nccl") on GPUs; ``merge`` defaults to the HIP merge kernel.
    """

    def __init__(self, local, id_base: int, group=None, merge=merge_topk):
        self.local, self.id_base, self.group, self.merge = local, int(id_base), group, merge

    def search(self, q, k: int):
        import torch
        import torch.distributed as dist

        D, I = self.local.search(q, k)
        I = torch.where(I >= 0, I + self.id_base, I)
        if not dist.is_initialized() or dist.get_world_size(self.group) == 1:
            return D, I
        world = dist.get_world_size(self.group)
        # one collective of 12 bytes per (distance, id): an int32 payload [nq][3k] = the float bits | the id's two halves
        payload = torch.cat([D.contiguous().view(torch.int32), I.contiguous().view(torch.int32)], dim=1).contiguous()
        nq = payload.shape[0]
        flat = torch.empty((world * nq, 3 * k), dtype=torch.int32, device=payload.device)
        dist.all_gather_into_tensor(flat, payload, group=self.group)  # rank-major concatenation
        gathered = flat.view(world, nq, 3 * k)
        dl = gathered[:, :, :k].contiguous().view(torch.float32)
        il = gathered[:, :, k:].contiguous().view(torch.int64)
        return self.merge(dl, il, k)


class RcclComm:
    """The library's own RCCL communicator (``eioku_comm_*``): for hosts that hold no ``torch.distributed`` process
    group.  Rank 0 calls :meth:`unique_id` and ships the 128 bytes to its peers by whatever channel the service has;
    every rank (one process per GPU) then constructs ``RcclComm(id, rank, world)`` -- a collective call."""

    ID_BYTES = 128

    def __init__(self, unique_id: bytes, rank: int, world: int):
        if len(unique_id) != self.ID_BYTES:
            raise ValueError(f"unique id must be {self.ID_BYTES} bytes, got {len(unique_id)}")
        uid = np.frombuffer(bytes(unique_id), np.uint8)  # held until the create call returns
        self._h = Handle("comm", ptr(uid), int(rank), int(world))
        self.rank, self.world = int(rank), int(world)

    @staticmethod
    def unique_id() -> bytes:
        buf = np.zeros(RcclComm.ID_BYTES, np.uint8)
        _lib.check(_lib.load().eioku_comm_unique_id(ptr(buf)), "eioku_comm_unique_id")
        return buf.tobytes()

    def close(self):
        self._h.close()


class CommShardedFlatL2:
    """:class:`ShardedFlatL2` with the collective inside the C ABI (``eioku_index_search_sharded``): local shard
    search, one RCCL all-gather of the packed answers, local merge.  ``local`` is this rank's :class:`IndexFlatL2`."""

    def __init__(self, local: "IndexFlatL2", id_base: int, comm: RcclComm):
        self.local, self.id_base, self.comm = local, int(id_base), comm

    def search(self, q, k: int):
        if not on_device(q):
            raise _lib.EiokuHipError("eioku_index_search_sharded takes device queries")
        nq, d = (int(s) for s in q.shape)
        if d != self.local.d:
            raise ValueError(f"expected dimension {self.local.d}, got {d}")
        q = q.contiguous()
        D, I = empty_results(q, nq, k)
        _lib.check(self.local._h.eioku_index_search_sharded(self.comm._h.ptr, self.id_base, ptr(q), nq, int(k),
                                                            ptr(D), ptr(I), current_stream(q)), "eioku_index_search_sharded")
        return D, I
