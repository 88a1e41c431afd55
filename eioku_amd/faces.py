"""Face clustering: ArcFace embeddings (insightface ``arcface_torch`` IResNet) and cosine DBSCAN on the HIP kernels of
``csrc/faces.hip``; HDBSCAN, the clustering without an ``eps`` (``face_cluster_method="hdbscan"``), is ``hdbscan.py``.

Fills the ``cluster_id`` that ``ModelManager.detect_faces`` returns (``cluster_faces`` config key).  Per face the device
produces a 112 x 112 crop, normalises it as arcface_torch's inference does (``(v / 255 - 0.5) / 0.5``) and runs the IResNet
(K13b) to a unit 512-vector; once per video the vectors are clustered by DBSCAN on cosine distance with scikit-learn's
labels (K14).  The crop is the aligned one ArcFace networks are trained on when the detector is a Pose checkpoint with
five landmarks: their similarity transform onto insightface's template (``align_matrices``, Umeyama on the host) and
``cv2.warpAffine`` in OpenCV's fixed point on the device (K13c).  Without landmarks, or for a face whose landmarks give no
usable transform, it is a square of side ``max(w, h, 1)`` centred on the detector's box, resampled bilinearly (K13a).
No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from functools import partial
from pathlib import Path

import numpy as np

from . import _lib
from ._buffers import current_stream, on_device, ptr
from ._handle import Handle
from ._state import bn_scale_shift, fold_conv_bn, np_state, rand_bn, rand_conv, resnet_depths, tensor

CROP = 112
FEAT = 512
TAP_BITS = 11
WIDTHS = (64, 128, 256, 512)
DEPTHS = {"r18": (2, 2, 2, 2), "r34": (3, 4, 6, 3), "r50": (3, 4, 14, 3), "r100": (3, 13, 30, 3)}


# ---- host side of K13a ---------------------------------------------------------------------------------------------
def axis_taps(lo: float, hi: float, side: float, size: int):
    """One axis of a crop (float64, as ``faces.hip`` axis_taps): ``(first source index int64 (112,), weight of the second
    tap in 1/2048 int64 (112,))`` for output pixel centres over ``[centre - side / 2, centre + side / 2]``; the index is
    clamped to ``[-2, size]`` (taps outside the frame read 0 either way)."""
    left = (lo + hi) * 0.5 - side * 0.5
    step = side / CROP
    src = left + (np.arange(CROP, dtype=np.float64) + 0.5) * step - 0.5
    f = np.floor(src)
    w1 = np.floor((src - f) * (1 << TAP_BITS) + 0.5).astype(np.int64)
    x0 = f.astype(np.int64)
    carry = w1 == (1 << TAP_BITS)
    x0 = np.where(carry, x0 + 1, x0)
    w1 = np.where(carry, 0, w1)
    return np.clip(x0, -2, size), w1


def crop_taps(box, h: int, w: int):
    """``box = (x1, y1, x2, y2)`` -> ``(x0, wx1, y0, wy1)``: the square of side ``max(w, h, 1)`` centred on the box."""
    x1, y1, x2, y2 = (float(np.float32(v)) for v in box)
    side = max(max(x2 - x1, y2 - y1), 1.0)
    return (*axis_taps(x1, x2, side, w), *axis_taps(y1, y2, side, h))


# ---- host side of K13c: landmarks -> similarity transform ---------------------------------------------------------------
# insightface face_align.arcface_dst: left eye, right eye, nose, left and right mouth corner in the 112 x 112 crop
ARCFACE_DST = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]],
                       dtype=np.float64)


def align_matrices(landmarks_xy):
    """``landmarks_xy`` ``(m, 5, 2)`` (frame pixels, ``ARCFACE_DST``'s order) -> ``(M, fallback)``: ``M`` float64 ``(m, 2, 3)``,
    the matrix ``cv2.warpAffine`` takes (frame -> crop), and ``fallback`` bool ``(m,)``, set where ``M`` is not usable (a
    non-finite entry or a scale <= 0: all five landmarks coincide) and the face keeps its box crop.

    ``M`` is scikit-image's ``SimilarityTransform.estimate(landmarks, ARCFACE_DST)`` (insightface's ``estimate_norm``):
    Umeyama's least-squares similarity with scale, here for all faces at once on stacked ``np.linalg.svd``, with its
    reflection rule (``det(A) < 0`` flips the last singular direction) and its rank-1 rule (collinear landmarks)."""
    src = np.asarray(landmarks_xy, dtype=np.float64).reshape(-1, 5, 2)
    m = src.shape[0]
    if m == 0:
        return np.zeros((0, 2, 3)), np.zeros(0, bool)
    dst_mean = ARCFACE_DST.mean(axis=0)
    dst_d = ARCFACE_DST - dst_mean
    src_mean = src.mean(axis=1)
    src_d = src - src_mean[:, None, :]
    with np.errstate(all="ignore"):
        A = np.matmul(dst_d.T, src_d) / 5  # (m, 2, 2)
        d = np.ones((m, 2))
        d[np.linalg.det(A) < 0, 1] = -1
        U, S, Vt = np.linalg.svd(A)
        rank = (S > S.max(axis=1, keepdims=True) * (2 * np.finfo(np.float64).eps)).sum(axis=1)  # np.linalg.matrix_rank
        dr = d.copy()
        # rank 1: the sign comes from det(U) det(V) instead of det(A) (which is 0 up to rounding there)
        one = rank == 1
        dr[one, 1] = np.where(np.linalg.det(U[one]) * np.linalg.det(Vt[one]) > 0, 1.0, -1.0)
        R = np.matmul(U * dr[:, None, :], Vt)
        scale = 1.0 / src_d.var(axis=1).sum(axis=1) * (S * d).sum(axis=1)
        t = dst_mean - scale[:, None] * np.matmul(R, src_mean[:, :, None])[:, :, 0]
        M = np.concatenate([R * scale[:, None, None], t[:, :, None]], axis=2)
        M[rank == 0] = np.nan
        fallback = ~np.isfinite(M).all(axis=(1, 2)) | ~(scale > 0)
    return M, fallback


# ---- arcface_torch state dict -> folded parameters -------------------------------------------------------------------
def depths_from_state(sd: dict) -> tuple:
    """Blocks per stage from the ``layer<L>.<b>.conv1.weight`` keys (r18 [2,2,2,2], r50 [3,4,14,3], r100 [3,13,30,3])."""
    return resnet_depths(sd, "an arcface_torch iresnet")


def fold_state(state_dict: dict) -> dict:
    """arcface_torch ``iresnet`` state dict (optionally under ``"state_dict"`` / with ``module.`` prefixes) ->
    ``{"depths", "convs": {name: (w, b)}, "prelu": [stem, block 0, ...], "bn": [(scale, shift) per block], "head": (w, b)}``
    with every BatchNorm that follows a conv folded into it, and ``bn2 -> fc -> features`` folded into one fc whose
    columns are permuted from torch's NCHW flatten (``c * 49 + y * 7 + x``) to the device's NHWC (``(y * 7 + x) * 512 + c``).
    A missing or misshapen tensor raises."""
    sd = np_state(state_dict)
    depths = depths_from_state(sd)
    convs, prelu, bns = {}, [], []

    def fold(conv, bn, cout, cin, k):
        return fold_conv_bn(sd, conv, bn, (cout, cin, k, k))

    convs["conv1"] = fold("conv1", "bn1", 64, 3, 3)
    prelu.append(tensor(sd, "prelu.weight", (64,)).astype(np.float32))
    inplanes = 64
    for li, (planes, depth) in enumerate(zip(WIDTHS, depths), start=1):
        for b in range(depth):
            p = f"layer{li}.{b}"
            cin = inplanes if b == 0 else planes
            s, t = bn_scale_shift(sd, p + ".bn1", cin)
            bns.append((s.astype(np.float32), t.astype(np.float32)))
            convs[p + ".conv1"] = fold(p + ".conv1", p + ".bn2", planes, cin, 3)
            prelu.append(tensor(sd, p + ".prelu.weight", (planes,)).astype(np.float32))
            convs[p + ".conv2"] = fold(p + ".conv2", p + ".bn3", planes, planes, 3)
            if b == 0:
                convs[p + ".downsample.0"] = fold(p + ".downsample.0", p + ".downsample.1", planes, cin, 1)
        inplanes = planes
    # fc(bn2(x)) = W (s2 * x + t2) + b, then features: a * (z - mu) + beta  (all exact: no padding is involved)
    s2, t2 = bn_scale_shift(sd, "bn2", 512)
    W = tensor(sd, "fc.weight", (FEAT, 512 * 49))
    fb = tensor(sd, "fc.bias", (FEAT,))
    sf, tf = bn_scale_shift(sd, "features", FEAT)
    s2x = np.repeat(s2, 49)  # NCHW flatten: channel c covers columns c * 49 .. c * 49 + 48
    t2x = np.repeat(t2, 49)
    Wf = sf[:, None] * (W * s2x[None, :])
    bf = sf * (W @ t2x + fb) + tf
    return {"depths": depths, "convs": convs, "prelu": prelu, "bn": bns,
            "head": (nchw_to_nhwc_columns(Wf).astype(np.float32), bf.astype(np.float32))}


def nchw_to_nhwc_columns(w: np.ndarray) -> np.ndarray:
    """fc weight ``[out][c * 49 + y * 7 + x]`` -> ``[out][(y * 7 + x) * 512 + c]`` (the device's NHWC activations)."""
    return np.ascontiguousarray(w.reshape(w.shape[0], 512, 49).transpose(0, 2, 1).reshape(w.shape[0], 512 * 49))


def random_state_dict(seed: int = 3, depths=DEPTHS["r18"]) -> dict:
    """Seeded random arcface_torch-shaped state dict (float32 numpy), BatchNorm running statistics randomised too:
    benchmarks and tests (no checkpoint is reachable offline)."""
    rng = np.random.default_rng(seed)
    sd = {}
    conv, bn = partial(rand_conv, rng, sd), partial(rand_bn, rng, sd)

    def prelu(name, c):
        sd[name + ".weight"] = rng.uniform(0.15, 0.35, c).astype(np.float32)

    conv("conv1", 64, 3, 3, 1.4)
    bn("bn1", 64)
    prelu("prelu", 64)
    inplanes = 64
    for li, (planes, depth) in enumerate(zip(WIDTHS, depths), start=1):
        for b in range(depth):
            p = f"layer{li}.{b}"
            cin = inplanes if b == 0 else planes
            bn(p + ".bn1", cin)
            conv(p + ".conv1", planes, cin, 3, 1.4)
            bn(p + ".bn2", planes)
            prelu(p + ".prelu", planes)
            conv(p + ".conv2", planes, planes, 3, 0.5)
            bn(p + ".bn3", planes)
            if b == 0:
                conv(p + ".downsample.0", planes, cin, 1)
                bn(p + ".downsample.1", planes)
        inplanes = planes
    bn("bn2", 512)
    sd["fc.weight"] = (rng.standard_normal((FEAT, 512 * 49)) / np.sqrt(512 * 49)).astype(np.float32)
    sd["fc.bias"] = (0.01 * rng.standard_normal(FEAT)).astype(np.float32)
    bn("features", FEAT)
    sd["features.weight"] = np.ones(FEAT, np.float32)  # arcface_torch: constant 1, not trained
    return sd


def load_checkpoint(path) -> dict:
    """``backbone.pth`` (arcface_torch's released state dict) -> folded state (torch's restricted unpickler: tensors only)."""
    import torch

    return fold_state(torch.load(str(path), map_location="cpu", weights_only=True))


# ---- K14 ---------------------------------------------------------------------------------------------------------
def dbscan_cosine(embeddings, eps: float, min_samples: int):
    """scikit-learn ``DBSCAN(eps, min_samples=min_samples, metric="cosine").fit(embeddings).labels_`` on unit-norm rows,
    on the device: float32 ``(n, d)`` (numpy or CUDA tensor; d % 32 == 0, n <= 65536, eps in [0, 2]) -> int32 ``(n,)``
    labels on the same side (-1 = noise)."""
    lib = _lib.load()
    _lib.init()
    dev = on_device(embeddings)
    if dev:
        e = embeddings.contiguous()
        import torch

        labels = torch.empty((int(e.shape[0]),), dtype=torch.int32, device=e.device)
    else:
        e = np.ascontiguousarray(embeddings, dtype=np.float32)
        labels = np.empty(int(e.shape[0]), np.int32)
    if len(e.shape) != 2:
        raise ValueError("expected (n, d) embeddings")
    n, d = int(e.shape[0]), int(e.shape[1])
    _lib.check(lib.eioku_dbscan_cosine(ptr(e) if n else None, n, d, float(eps), int(min_samples), ptr(labels) if n else None,
                                       _lib.MEM_DEVICE if dev else _lib.MEM_HOST, current_stream(e) if dev else None),
               "eioku_dbscan_cosine")
    return labels


def cluster_ids(labels) -> list:
    """DBSCAN labels -> the artifact's ``cluster_id`` strings: ``face_cluster_001`` for label 0, ``None`` for noise."""
    return [None if int(v) < 0 else f"face_cluster_{int(v) + 1:03d}" for v in labels]


class FaceEmbedder:
    """arcface_torch ``iresnet`` (``backbone.pth``) + the crop / normalisation of its inference script, on the device."""

    def __init__(self, state: dict):
        self.depths = tuple(int(v) for v in state["depths"])
        self._h = Handle("iresnet", (C.c_int * 4)(*self.depths))
        self._h.or_close(self._load, state)

    def _load(self, state: dict) -> None:
        h = self._h
        h.set_convs(state["convs"])
        nb = h.eioku_iresnet_num_blocks()
        if len(state["prelu"]) != nb + 1 or len(state["bn"]) != nb:
            raise ValueError(f"state has {len(state['prelu'])} PReLUs / {len(state['bn'])} bn1s for {nb} blocks")
        for u, a in enumerate(state["prelu"]):
            a = np.ascontiguousarray(a, dtype=np.float32)
            _lib.check(h.eioku_iresnet_set_prelu(u, ptr(a)), "eioku_iresnet_set_prelu")
        for b, (s, t) in enumerate(state["bn"]):
            s, t = np.ascontiguousarray(s, dtype=np.float32), np.ascontiguousarray(t, dtype=np.float32)
            _lib.check(h.eioku_iresnet_set_bn(b, ptr(s), ptr(t)), "eioku_iresnet_set_bn")
        w, b = (np.ascontiguousarray(a, dtype=np.float32) for a in state["head"])
        if w.shape != (FEAT, 512 * 49) or b.shape != (FEAT,):
            raise ValueError(f"head: expected weight {(FEAT, 512 * 49)}, got {w.shape}")
        _lib.check(h.eioku_iresnet_set_head(ptr(w), ptr(b)), "eioku_iresnet_set_head")

    @classmethod
    def from_cache(cls, cache_dir, model_name: str = "arcface_r18.pth", seed: int | None = None):
        """Weights from ``<cache>/insightface/<model_name>`` (an arcface_torch ``backbone.pth`` state dict).  A missing file
        is an error unless a ``seed`` asks for seeded random r18 weights (the ``Places365Classifier.from_cache`` rule)."""
        path = Path(cache_dir) / "insightface" / model_name
        if path.exists():
            return cls(load_checkpoint(path))
        if seed is None:
            raise FileNotFoundError(f"{path} not found (no weights to embed faces with)")
        return cls(fold_state(random_state_dict(seed)))

    @staticmethod
    def _boxes(boxes):
        b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 5)
        return b

    def crop(self, frames_bgr, boxes):
        """K13a alone: BGR uint8 ``(n,h,w,3)`` + float32 ``(m,5)`` (slot, x1, y1, x2, y2) -> fp16 ``(m,112,112,8)`` CUDA."""
        import torch

        n, h, w, _ = (int(s) for s in frames_bgr.shape)
        b = self._boxes(boxes)
        dev = frames_bgr.device if on_device(frames_bgr) else torch.device("cuda", torch.cuda.current_device())
        out = torch.empty((len(b), CROP, CROP, 8), dtype=torch.float16, device=dev)
        src = frames_bgr if on_device(frames_bgr) else np.ascontiguousarray(frames_bgr, dtype=np.uint8)
        _lib.check(self._h.eioku_iresnet_crop(ptr(src), n, h, w, ptr(b), len(b), ptr(out),
                                              _lib.MEM_DEVICE if on_device(src) else _lib.MEM_HOST, current_stream(out)),
                   "eioku_iresnet_crop")
        return out

    def crop_aligned(self, frames_bgr, slots, M):
        """K13c alone: BGR uint8 ``(n,h,w,3)`` + frame slots ``(m,)`` + matrices float64 ``(m,2,3)`` (frame -> crop, as
        ``cv2.warpAffine`` takes them) -> fp16 ``(m,112,112,8)`` CUDA."""
        import torch

        n, h, w, _ = (int(s) for s in frames_bgr.shape)
        sl = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        mats = np.ascontiguousarray(M, dtype=np.float64).reshape(-1, 6)
        if len(sl) != len(mats):
            raise ValueError("one frame slot per matrix")
        dev = frames_bgr.device if on_device(frames_bgr) else torch.device("cuda", torch.cuda.current_device())
        out = torch.empty((len(sl), CROP, CROP, 8), dtype=torch.float16, device=dev)
        src = frames_bgr if on_device(frames_bgr) else np.ascontiguousarray(frames_bgr, dtype=np.uint8)
        _lib.check(self._h.eioku_iresnet_crop_aligned(ptr(src), n, h, w, ptr(sl), ptr(mats), len(sl), ptr(out),
                                                      _lib.MEM_DEVICE if on_device(src) else _lib.MEM_HOST, current_stream(out)),
                   "eioku_iresnet_crop_aligned")
        return out

    def forward_raw(self, crops, upto_block: int = -1):
        """fp16 ``(m,112,112,8)`` CUDA crops (m <= 256) -> float32 ``(m,512)`` embeddings, or (``upto_block >= 0``) that
        block's NHWC fp16 output (CUDA)."""
        import torch

        m = int(crops.shape[0])
        crops = crops.contiguous()
        if upto_block >= 0:
            hw, c = CROP, 64
            k = 0
            for li, d in enumerate(self.depths):
                hw //= 2
                c = WIDTHS[li]
                if upto_block < k + d:
                    break
                k += d
            out = torch.empty((m, hw, hw, c), dtype=torch.float16, device=crops.device)
            _lib.check(self._h.eioku_iresnet_forward(ptr(crops), m, int(upto_block), ptr(out), None, current_stream(crops)),
                       "eioku_iresnet_forward")
            return out
        out = torch.empty((m, FEAT), dtype=torch.float32, device=crops.device)
        _lib.check(self._h.eioku_iresnet_forward(ptr(crops), m, -1, None, ptr(out), current_stream(crops)),
                   "eioku_iresnet_forward")
        return out

    def embed(self, frames_bgr, boxes) -> np.ndarray:
        """BGR uint8 ``(n,h,w,3)`` frames (numpy: staged once; CUDA tensor: read in place) + ``boxes`` float32 ``(m,5)``
        rows ``(frame slot, x1, y1, x2, y2)`` -> float32 ``(m,512)`` unit embeddings (numpy)."""
        return self._embed(frames_bgr, boxes, None)

    def embed_aligned(self, frames_bgr, boxes, landmarks) -> np.ndarray:
        """``embed`` on aligned crops: ``landmarks`` ``(m,5,2)`` (or ``(m,5,3)`` with a confidence that is not used), frame
        pixels in ``ARCFACE_DST``'s order.  A face whose landmarks give no usable transform (``align_matrices``' mask)
        is embedded from its box crop, exactly as ``embed`` does."""
        lm = np.asarray(landmarks, dtype=np.float64)
        if lm.ndim != 3 or lm.shape[1] != 5 or lm.shape[2] not in (2, 3):
            raise ValueError(f"expected (m,5,2) landmarks, got {lm.shape}")
        return self._embed(frames_bgr, boxes, align_matrices(lm[:, :, :2]))

    def _embed(self, frames_bgr, boxes, aligned) -> np.ndarray:
        n, h, w, c = (int(s) for s in frames_bgr.shape)
        if c != 3:
            raise ValueError("expected (n,h,w,3) BGR frames")
        b = self._boxes(boxes)
        out = np.empty((len(b), FEAT), np.float32)
        if aligned is not None and len(aligned[0]) != len(b):
            raise ValueError("one landmark set per box")
        if len(b) == 0:
            return out
        src = frames_bgr if on_device(frames_bgr) else np.ascontiguousarray(frames_bgr, dtype=np.uint8)
        dev = on_device(src)
        if dev:
            import torch

            dst = torch.empty((len(b), FEAT), dtype=torch.float32, device=src.device)
        else:
            dst = out
        mem, stream = (_lib.MEM_DEVICE, current_stream(src)) if dev else (_lib.MEM_HOST, None)
        if aligned is None:
            _lib.check(self._h.eioku_iresnet_embed(ptr(src), n, h, w, ptr(b), len(b), ptr(dst), mem, stream),
                       "eioku_iresnet_embed")
        else:
            M, fallback = aligned
            mats = np.ascontiguousarray(np.where(fallback[:, None, None], 0.0, M), dtype=np.float64).reshape(-1, 6)
            flags = np.ascontiguousarray(fallback, dtype=np.int32)
            _lib.check(self._h.eioku_iresnet_embed_aligned(ptr(src), n, h, w, ptr(b), ptr(mats), ptr(flags), len(b), ptr(dst),
                                                           mem, stream), "eioku_iresnet_embed_aligned")
        return dst.cpu().numpy() if dev else out

    def cluster(self, embeddings, eps: float, min_samples: int):
        """DBSCAN on cosine distance (``dbscan_cosine``) -> int32 labels, numpy."""
        labels = dbscan_cosine(embeddings, eps, min_samples)
        return labels.cpu().numpy() if on_device(labels) else labels

    def cluster_hdbscan(self, embeddings, min_cluster_size: int, min_samples: int, selection_epsilon: float = 0.0):
        """HDBSCAN on cosine distance (``hdbscan.hdbscan_cosine``, K14h) -> ``(int32 labels, float64 probabilities)``,
        numpy: no ``eps`` to choose, and a membership strength per face."""
        from .hdbscan import hdbscan_cosine

        return hdbscan_cosine(embeddings, min_cluster_size=min_cluster_size, min_samples=min_samples,
                              cluster_selection_epsilon=selection_epsilon)

    def last_flops(self) -> float:
        return self._h.doubles("last_flops")[0]

    def close(self):
        self._h.close()


CLUSTER_METHODS = ("dbscan", "hdbscan")


class FaceClusterer:
    """Per-video collector shared by ``detect_faces`` and ``analyze_video``: embeddings of the faces that pass the face
    path's confidence filter, batch by batch, then one clustering at the end that fills each face's ``cluster_id``:
    DBSCAN (``method="dbscan"``: ``eps``, ``min_samples``) or HDBSCAN (``"hdbscan"``: ``min_cluster_size``, ``min_samples``
    and, only if given, ``eps`` as its ``cluster_selection_epsilon``), which also fills ``cluster_probability``."""

    def __init__(self, embedder, eps, min_samples: int, method: str = "dbscan", min_cluster_size: int = 5):
        if method not in CLUSTER_METHODS:
            raise ValueError(f"face_cluster_method must be one of {CLUSTER_METHODS}, got {method!r}")
        self.embedder = embedder
        self.method = method
        self.eps = None if eps is None else float(eps)
        self.min_samples = int(min_samples)
        self.min_cluster_size = int(min_cluster_size)
        self._dets: list[dict] = []
        self._emb: list[np.ndarray] = []

    def add(self, frames_bgr, boxes, dets: list, landmarks=None) -> None:
        """``frames_bgr`` the batch the detector saw (device copy or host), ``boxes`` ``(slot, x1, y1, x2, y2)`` rows for
        ``dets`` (the detection dicts, in emission order).  ``landmarks`` ``(m,5,2)``: the faces' five landmarks, embedded
        from aligned crops (``embed_aligned``); without them the box crops, through ``embed`` as ever."""
        if not dets:
            return
        b = np.asarray(boxes, np.float32).reshape(-1, 5)
        if landmarks is None or not hasattr(self.embedder, "embed_aligned"):  # (an embedder fake may have ``embed`` only)
            emb = self.embedder.embed(frames_bgr, b)
        else:
            emb = self.embedder.embed_aligned(frames_bgr, b, landmarks)
        self._emb.append(np.asarray(emb, np.float32))
        self._dets.extend(dets)

    def embeddings(self) -> np.ndarray:
        return np.concatenate(self._emb) if self._emb else np.zeros((0, FEAT), np.float32)

    def finish(self) -> None:
        if not self._dets:
            return
        if self.method == "hdbscan":
            labels, prob = self.embedder.cluster_hdbscan(self.embeddings(), self.min_cluster_size, self.min_samples,
                                                         0.0 if self.eps is None else self.eps)
            for det, cid, p in zip(self._dets, cluster_ids(labels), prob):
                det["cluster_id"] = cid
                det["cluster_probability"] = float(p) if cid is not None else 0.0
            return
        labels = self.embedder.cluster(self.embeddings(), self.eps, self.min_samples)
        for det, cid in zip(self._dets, cluster_ids(labels)):
            det["cluster_id"] = cid
