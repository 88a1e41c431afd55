"""Speaker labels for transcript segments (K24): WeSpeaker ResNet speaker embeddings and cosine DBSCAN on the HIP kernels
of ``csrc/speakers.hip``.

Fills the ``speaker`` key that ``transcribe_video`` adds under ``speaker_labels``.  Per transcript segment the host plans up
to :data:`MAX_WINDOWS` windows of :data:`WIN` frames (:func:`plan_windows`); per window the device computes the 80-bin Kaldi
fbank with CMN (K24a), runs the BasicBlock ResNet of base width 32 (K24b), pools mean and standard deviation over the
window's valid columns and applies ``seg_1`` (K24c); a segment's vector is the normalised mean of its windows' vectors, the
video's segment vectors are clustered by K14 (``faces.dbscan_cosine``) and noise rows are reassigned to the nearest
centroid (K24d).  No CPU fallback.

[PUBLIC-LIB] The front end (Kaldi ``fbank`` as WeSpeaker calls it), the network (WeSpeaker's ``ResNet34``, the embedding
model of ``pyannote/speaker-diarization-3.1``) and its tensor names are restated from the public sources; neither package
nor a checkpoint is a dependency, and none could be read when this was written.
"""
from __future__ import annotations

import ctypes as C
import math
from functools import partial
from pathlib import Path

import numpy as np

from . import _lib
from ._buffers import current_stream, on_device, ptr
from ._handle import Handle
from ._state import fold_conv_bn, np_state, rand_bn, rand_conv, resnet_depths, tensor

SAMPLE_RATE = 16000
FRAME = 400            # 25 ms
SHIFT = 160            # 10 ms
N_FFT = 512
N_BINS = 256           # Kaldi's mel banks cover FFT bins 0 .. 255 (no Nyquist bin)
N_MEL = 80
WIN = 200              # frames per window (the handle's ``win_frames``)
HOP = 100              # nominal hop between a segment's windows: half a window
MAX_WINDOWS = 8
MIN_FRAMES = 40
FEAT = 256
WIDTHS = (32, 64, 128, 256)
N_STAT = 2 * WIDTHS[3] * (N_MEL // 8)   # 5120
PASS = 64              # windows per network pass
MAX_SEGMENTS = 65536   # K14's limit
DEPTHS = {"r18": (2, 2, 2, 2), "r34": (3, 4, 6, 3)}
_STRIP = ("module.", "resnet.")
# picked, not tuned: no checkpoint was available to validate them against
DEFAULT_EPS = 0.25
DEFAULT_MIN_SAMPLES = 2
DEFAULT_ASSIGN_MAX = 0.5


# ---- K24 window plan (host, integers) ---------------------------------------------------------------------------------
def num_frames(n: int) -> int:
    """Kaldi frames (``snip_edges``) of ``n`` samples."""
    return 0 if n < FRAME else 1 + (n - FRAME) // SHIFT


def plan_windows(start_ms: int, end_ms: int, n_samples: int, win_frames: int = WIN) -> list[tuple[int, int]]:
    """Windows of the segment ``[start_ms, end_ms)`` over ``n_samples`` of 16 kHz audio: ``[(first sample, valid frames)]``.
    Fewer than :data:`MIN_FRAMES` frames: none.  Up to ``win_frames``: one window of every frame.  Otherwise
    ``k = min(MAX_WINDOWS, 1 + ceil(span / hop))`` full windows (``span = frames - win_frames``, ``hop = win_frames // 2``)
    with window ``j`` at frame ``j * span // (k - 1)``: the first starts and the last ends with the segment."""
    s0 = int(start_ms) * (SAMPLE_RATE // 1000)
    s1 = min(int(end_ms) * (SAMPLE_RATE // 1000), int(n_samples))
    nf = num_frames(s1 - s0) if s0 >= 0 else 0
    if nf < MIN_FRAMES:
        return []
    if nf <= win_frames:
        return [(s0, nf)]
    span, hop = nf - win_frames, win_frames // 2
    k = min(MAX_WINDOWS, 1 + -(-span // hop))
    return [(s0 + SHIFT * ((j * span) // (k - 1)), win_frames) for j in range(k)]


# ---- K24a tables (host, float64) --------------------------------------------------------------------------------------
def povey_window() -> np.ndarray:
    n = np.arange(FRAME, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / (FRAME - 1))) ** 0.85


def kaldi_mel_banks(low: float = 20.0, high: float = SAMPLE_RATE / 2) -> np.ndarray:
    """Kaldi's ``MelBanks`` (no VTLN): ``(80, 256)`` triangles, linear in the mel scale ``1127 ln(1 + f / 700)``."""
    def mel(f):
        return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)

    lo, hi = float(mel(low)), float(mel(high))
    delta = (hi - lo) / (N_MEL + 1)
    m = mel(np.arange(N_BINS, dtype=np.float64) * (SAMPLE_RATE / N_FFT))
    banks = np.zeros((N_MEL, N_BINS), np.float64)
    for j in range(N_MEL):
        left, centre, right = lo + j * delta, lo + (j + 1) * delta, lo + (j + 2) * delta
        inside = (m > left) & (m < right)
        up = (m - left) / (centre - left)
        down = (right - m) / (right - centre)
        banks[j] = np.where(inside, np.where(m <= centre, up, down), 0.0)
    return banks


# ---- WeSpeaker state dict -> folded parameters --------------------------------------------------------------------------
def depths_from_state(sd: dict) -> tuple:
    """Blocks per stage from the ``layer<L>.<b>.conv1.weight`` keys (r18 (2,2,2,2), r34 (3,4,6,3)); prefixes are stripped."""
    return resnet_depths(np_state(sd, _STRIP), "a WeSpeaker ResNet")


def torch_to_device_columns(w: np.ndarray) -> np.ndarray:
    """``[..., 5120]`` in torch's flatten of ``(C, F')`` (means then stds, each ``c * 10 + f``) -> the device's NHWC order
    (each ``f * 256 + c``)."""
    w = np.asarray(w)
    return np.ascontiguousarray(w.reshape(*w.shape[:-1], 2, WIDTHS[3], N_MEL // 8).swapaxes(-1, -2).reshape(w.shape))


def device_to_torch_columns(w: np.ndarray) -> np.ndarray:
    """The inverse of :func:`torch_to_device_columns`."""
    w = np.asarray(w)
    return np.ascontiguousarray(w.reshape(*w.shape[:-1], 2, N_MEL // 8, WIDTHS[3]).swapaxes(-1, -2).reshape(w.shape))


def fold_state(state_dict: dict) -> dict:
    """WeSpeaker ``ResNet`` state dict (optionally under ``"state_dict"`` / with ``module.`` / ``resnet.`` prefixes) ->
    ``{"depths", "convs": {name: (w, b)}, "head": (w, b)}``: every BatchNorm folded into the conv before it, ``seg_1``'s
    columns permuted to the device's order.  A missing or misshapen tensor raises."""
    sd = np_state(state_dict, _STRIP)
    depths = depths_from_state(sd)
    convs = {}

    def fold(conv, bn, cout, cin, k):
        return fold_conv_bn(sd, conv, bn, (cout, cin, k, k))

    convs["conv1"] = fold("conv1", "bn1", WIDTHS[0], 1, 3)
    inplanes = WIDTHS[0]
    for li, (planes, depth) in enumerate(zip(WIDTHS, depths), start=1):
        for b in range(depth):
            p = f"layer{li}.{b}"
            cin = inplanes if b == 0 else planes
            convs[p + ".conv1"] = fold(p + ".conv1", p + ".bn1", planes, cin, 3)
            convs[p + ".conv2"] = fold(p + ".conv2", p + ".bn2", planes, planes, 3)
            if b == 0 and li > 1:
                convs[p + ".shortcut.0"] = fold(p + ".shortcut.0", p + ".shortcut.1", planes, cin, 1)
        inplanes = planes
    w = tensor(sd, "seg_1.weight", (FEAT, N_STAT))
    b = tensor(sd, "seg_1.bias", (FEAT,))
    return {"depths": depths, "convs": convs, "head": (torch_to_device_columns(w).astype(np.float32), b.astype(np.float32))}


def random_state_dict(seed: int = 3, depths=DEPTHS["r34"]) -> dict:
    """Seeded random WeSpeaker-shaped state dict (float32 numpy), BatchNorm running statistics randomised too: benchmarks
    and tests.  The gains are ``faces.random_state_dict``'s (1.4 on conv1, 0.5 on conv2, 1.0 on shortcuts): they keep the
    activations of an r34 far inside fp16, which plain He initialisation does not."""
    rng = np.random.default_rng(seed)
    sd = {}
    conv, bn = partial(rand_conv, rng, sd), partial(rand_bn, rng, sd)
    conv("conv1", WIDTHS[0], 1, 3, 1.4)
    bn("bn1", WIDTHS[0])
    inplanes = WIDTHS[0]
    for li, (planes, depth) in enumerate(zip(WIDTHS, depths), start=1):
        for b in range(depth):
            p = f"layer{li}.{b}"
            cin = inplanes if b == 0 else planes
            conv(p + ".conv1", planes, cin, 3, 1.4)
            bn(p + ".bn1", planes)
            conv(p + ".conv2", planes, planes, 3, 0.5)
            bn(p + ".bn2", planes)
            if b == 0 and li > 1:
                conv(p + ".shortcut.0", planes, cin, 1)
                bn(p + ".shortcut.1", planes)
        inplanes = planes
    sd["seg_1.weight"] = (rng.standard_normal((FEAT, N_STAT)) / np.sqrt(N_STAT)).astype(np.float32)
    sd["seg_1.bias"] = (0.01 * rng.standard_normal(FEAT)).astype(np.float32)
    return sd


def load_checkpoint(path) -> dict:
    """WeSpeaker's ``avg_model.pt`` -> folded state (torch's restricted unpickler: tensors only)."""
    import torch

    return fold_state(torch.load(str(path), map_location="cpu", weights_only=True))


# ---- options and labels -------------------------------------------------------------------------------------------------
def _is_real(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v)


def check_speaker_options(speaker_eps=DEFAULT_EPS, speaker_min_samples=DEFAULT_MIN_SAMPLES,
                          speaker_assign_max=DEFAULT_ASSIGN_MAX) -> dict:
    """The three clustering options, normalised, or ``ValueError``: ``speaker_eps`` in (0, 2), ``speaker_min_samples`` an
    integer >= 1, ``speaker_assign_max`` in [0, 2]."""
    if not _is_real(speaker_eps) or not 0.0 < speaker_eps < 2.0:
        raise ValueError(f"speaker_eps must be a number in (0, 2), got {speaker_eps!r}")
    if not _is_real(speaker_min_samples) or int(speaker_min_samples) != speaker_min_samples or speaker_min_samples < 1:
        raise ValueError(f"speaker_min_samples must be an integer >= 1, got {speaker_min_samples!r}")
    if not _is_real(speaker_assign_max) or not 0.0 <= speaker_assign_max <= 2.0:
        raise ValueError(f"speaker_assign_max must be a number in [0, 2], got {speaker_assign_max!r}")
    return {"eps": float(speaker_eps), "min_samples": int(speaker_min_samples), "assign_max": float(speaker_assign_max)}


SPEAKER_KEYS = ("speaker_eps", "speaker_min_samples", "speaker_assign_max")


def speaker_ids(labels, starts_ms=None) -> list:
    """Cluster labels -> ``speaker_001`` ... numbered by first appearance in time (``starts_ms``; list order without it);
    negative labels and ``None`` -> ``None``."""
    labels = [None if v is None or int(v) < 0 else int(v) for v in labels]
    order = range(len(labels)) if starts_ms is None else sorted(range(len(labels)), key=lambda i: (starts_ms[i], i))
    number = {}
    for i in order:
        if labels[i] is not None and labels[i] not in number:
            number[labels[i]] = len(number) + 1
    return [None if v is None else f"speaker_{number[v]:03d}" for v in labels]


def assign_noise(embeddings, labels, assign_max: float, return_centroids: bool = False):
    """K24d on the device: float32 ``(n, 256)`` unit rows and int32 DBSCAN labels (CUDA tensors) -> int32 labels (CUDA)
    with every noise row given the label of the nearest centroid when ``1 - cos <= assign_max``."""
    import torch

    lib = _lib.load()
    _lib.init()
    e, lab = embeddings.contiguous(), labels.contiguous()
    n = int(e.shape[0])
    if tuple(e.shape) != (n, FEAT) or e.dtype != torch.float32 or lab.dtype != torch.int32 or tuple(lab.shape) != (n,):
        raise ValueError(f"expected float32 (n, {FEAT}) embeddings and int32 (n,) labels")
    out = torch.empty_like(lab)
    cent = torch.zeros((n, FEAT), dtype=torch.float32, device=e.device) if return_centroids else None
    k = C.c_int(0)
    _lib.check(lib.eioku_spk_assign(ptr(e) if n else None, n, ptr(lab) if n else None, float(assign_max), ptr(out) if n else None,
                                    ptr(cent) if n and cent is not None else None, C.byref(k), current_stream(e)),
               "eioku_spk_assign")
    return (out, cent[:k.value]) if return_centroids else out


class SpeakerLabeller:
    """WeSpeaker ResNet (``avg_model.pt``) with its Kaldi fbank front end and the per-video clustering, on the device."""

    def __init__(self, state: dict, win_frames: int = WIN):
        self.depths = tuple(int(v) for v in state["depths"])
        self.win = int(win_frames)
        if self.win < 16 or self.win % 8:
            raise ValueError(f"win_frames must be a multiple of 8, at least 16, got {win_frames!r}")
        window, mel = povey_window(), np.ascontiguousarray(kaldi_mel_banks())
        self._h = Handle("spk", (C.c_int * 4)(*self.depths), self.win, ptr(window), ptr(mel))
        self._h.or_close(self._load, state)

    def _load(self, state: dict) -> None:
        self._h.set_convs(state["convs"])
        w, b = (np.ascontiguousarray(a, dtype=np.float32) for a in state["head"])
        if w.shape != (FEAT, N_STAT) or b.shape != (FEAT,):
            raise ValueError(f"head: expected weight {(FEAT, N_STAT)}, got {w.shape}")
        _lib.check(self._h.eioku_spk_set_head(ptr(w), ptr(b)), "eioku_spk_set_head")

    @classmethod
    def from_cache(cls, cache_dir, model_name: str = "voxceleb_resnet34_LM", seed: int | None = None, **kw):
        """Weights from ``<cache>/wespeaker/<model_name>/avg_model.pt``.  A missing file is an error unless a ``seed`` asks
        for seeded random r34 weights (the ``FaceEmbedder.from_cache`` rule)."""
        path = Path(cache_dir) / "wespeaker" / model_name / "avg_model.pt"
        if path.exists():
            return cls(load_checkpoint(path), **kw)
        if seed is None:
            raise FileNotFoundError(f"{path} not found (no weights to embed speakers with)")
        return cls(fold_state(random_state_dict(seed)), **kw)

    # ---- stages -----------------------------------------------------------------------------------------------------
    @staticmethod
    def _device():
        import torch

        return torch.device("cuda", torch.cuda.current_device())

    def set_audio(self, samples) -> None:
        """The video's 16 kHz mono float32 samples (numpy: uploaded once; CUDA tensor: copied on the device)."""
        if on_device(samples):
            import torch

            s = samples.reshape(-1).to(torch.float32).contiguous()
        else:
            s = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
        n = int(s.shape[0])
        _lib.check(self._h.eioku_spk_set_audio(ptr(s) if n else None, n, _lib.MEM_DEVICE if on_device(s) else _lib.MEM_HOST,
                                               current_stream(s)), "eioku_spk_set_audio")

    @staticmethod
    def _plan(plan) -> np.ndarray:
        return np.ascontiguousarray(plan, dtype=np.int32).reshape(-1, 2)

    def features(self, samples, plan):
        """K24a alone: ``plan`` rows ``(first sample, valid frames)`` (at most 64) -> ``(fp16 (m, 80, win, 8), float32
        (m, 80, win))`` CUDA tensors: the network's input and the same values before the rounding to fp16."""
        import torch

        self.set_audio(samples)
        p = self._plan(plan)
        dev = self._device()
        f16 = torch.empty((len(p), N_MEL, self.win, 8), dtype=torch.float16, device=dev)
        f32 = torch.empty((len(p), N_MEL, self.win), dtype=torch.float32, device=dev)
        _lib.check(self._h.eioku_spk_features(ptr(p), len(p), ptr(f16), ptr(f32), current_stream(f16)), "eioku_spk_features")
        return f16, f32

    def block_shape(self, upto_block: int) -> tuple:
        """``(H, W, C)`` of block ``upto_block``'s output."""
        hh, ww, k = N_MEL, self.win, 0
        for li, d in enumerate(self.depths):
            if li:
                hh, ww = (hh + 1) // 2, (ww + 1) // 2
            if upto_block < k + d:
                return hh, ww, WIDTHS[li]
            k += d
        raise ValueError(f"block {upto_block} outside [0, {k})")

    def forward_raw(self, feats, valid=None, upto_block: int = -1, stats: bool = False):
        """fp16 ``(m, 80, win, 8)`` CUDA features (m <= 64) -> float32 ``(m, 256)`` unnormalised vectors pooled over the
        first ``ceil(valid / 8)`` columns (with ``stats``: ``(vectors, (m, 5120) statistics in the device's column
        order)``), or (``upto_block >= 0``) that block's NHWC fp16 output.  CUDA tensors."""
        import torch

        m = int(feats.shape[0])
        feats = feats.contiguous()
        if tuple(feats.shape) != (m, N_MEL, self.win, 8) or feats.dtype != torch.float16:
            raise ValueError(f"expected fp16 (m, {N_MEL}, {self.win}, 8) features")
        if upto_block >= 0:
            out = torch.empty((m, *self.block_shape(upto_block)), dtype=torch.float16, device=feats.device)
            _lib.check(self._h.eioku_spk_forward(ptr(feats), None, m, int(upto_block), ptr(out), None, None,
                                                 current_stream(feats)), "eioku_spk_forward")
            return out
        v = np.ascontiguousarray(valid, dtype=np.int32).reshape(-1)
        if len(v) != m:
            raise ValueError(f"{m} windows but {len(v)} valid counts")
        out = torch.empty((m, FEAT), dtype=torch.float32, device=feats.device)
        st = torch.empty((m, N_STAT), dtype=torch.float32, device=feats.device) if stats else None
        _lib.check(self._h.eioku_spk_forward(ptr(feats), ptr(v), m, -1, None, ptr(st), ptr(out), current_stream(feats)),
                   "eioku_spk_forward")
        return (out, st) if stats else out

    def embed_windows(self, samples, plan):
        """``plan`` rows ``(first sample, valid frames)`` over ``samples`` (numpy or CUDA) -> float32 ``(m, 256)``
        unnormalised window vectors (CUDA), in passes of 64."""
        import torch

        self.set_audio(samples)
        p = self._plan(plan)
        out = torch.empty((len(p), FEAT), dtype=torch.float32, device=self._device())
        _lib.check(self._h.eioku_spk_embed(ptr(p) if len(p) else None, len(p), ptr(out) if len(p) else None,
                                           current_stream(out)), "eioku_spk_embed")
        return out

    def segment_vectors(self, window_vectors, seg_first):
        """Window vectors ``(rows, 256)`` (CUDA) and ``seg_first`` (n_seg + 1 ascending row offsets) -> float32
        ``(n_seg, 256)`` unit vectors (CUDA): the normalised mean of each segment's rows."""
        import torch

        first = np.ascontiguousarray(seg_first, dtype=np.int32).reshape(-1)
        n = len(first) - 1
        wv = window_vectors.contiguous()
        if n < 0 or (n and int(first[-1]) != int(wv.shape[0])):
            raise ValueError("seg_first does not cover the window vectors")
        out = torch.empty((max(n, 0), FEAT), dtype=torch.float32, device=wv.device)
        if n > 0:
            _lib.check(self._h.lib.eioku_spk_segments(ptr(wv), ptr(first), n, ptr(out), current_stream(wv)), "eioku_spk_segments")
        return out

    def embed_segments(self, samples, segments):
        """Segments (dicts with ``start_ms`` / ``end_ms`` in file time) over the file's 16 kHz ``samples`` ->
        ``(float32 (n, 256) unit vectors (CUDA), indices of the n segments long enough to embed)``."""
        n_samples = int(np.prod(samples.shape))
        plan, first, index = [], [0], []
        for i, seg in enumerate(segments):
            w = plan_windows(seg["start_ms"], seg["end_ms"], n_samples, self.win)
            if w:
                plan.extend(w)
                first.append(len(plan))
                index.append(i)
        if len(index) > MAX_SEGMENTS:
            raise ValueError(f"{len(index)} segments to cluster, more than {MAX_SEGMENTS}")
        wv = self.embed_windows(samples, np.asarray(plan, np.int32).reshape(-1, 2))
        return self.segment_vectors(wv, first), index

    def label(self, samples, segments, eps: float = DEFAULT_EPS, min_samples: int = DEFAULT_MIN_SAMPLES,
              assign_max: float = DEFAULT_ASSIGN_MAX) -> list:
        """One ``speaker_NNN`` (or ``None``: too short, or noise no centroid is near) per segment."""
        from .faces import dbscan_cosine

        vectors, index = self.embed_segments(samples, segments)
        out = [None] * len(segments)
        if not index:
            return out
        labels = assign_noise(vectors, dbscan_cosine(vectors, eps, min_samples), assign_max).cpu().numpy()
        ids = speaker_ids(labels, [int(segments[i]["start_ms"]) for i in index])
        for i, s in zip(index, ids):
            out[i] = s
        return out

    def last_ms(self) -> tuple[float, float, float]:
        """Device milliseconds of the last ``embed_windows``: (features, network, pooling + seg_1)."""
        return self._h.doubles("last_ms", 3)

    def close(self):
        self._h.close()
