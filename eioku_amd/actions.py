"""Action recognition (TimeSformer, divided space-time attention) on the HIP kernels of ``csrc/actions.hip``.

The reference's design names an "Action Detector" (``.kiro/specs/semantic-video-search/design.md`` §1.8: X3D, SlowFast or
TimeSformer on Kinetics-400, ``detectActions(videoPath, stride, window) -> [{frame, timestamp, labels[top-5], scores[]}]``)
and never builds it.  The model here is Hugging Face ``TimesformerForVideoClassification``: its ``state_dict()`` names, its
``config.json`` keys, and the arithmetic of ``VideoMAEImageProcessor`` (Pillow's antialiased bilinear resize of the short
edge, centre crop, ``x / 255``, normalise).  The host computes Pillow's coefficient tables for the rows and columns the
crop keeps; everything else runs on the device behind ``eioku_timesformer_classify``.  No CPU fallback.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

from . import _lib
from ._buffers import current_stream, on_device, ptr
from ._handle import Handle
from ._state import np_state
from .places import resize_tables

PATCH = 16
MAX_IMAGE = 448
MAX_FRAMES = 96
DEFAULT_MODEL = "timesformer-base-finetuned-k400"
DEFAULT_MEAN = (0.45, 0.45, 0.45)
DEFAULT_STD = (0.225, 0.225, 0.225)


def timesformer_dims(config: dict) -> dict:
    """The dimensions the library needs from a ``config.json``; what the kernels do not build is a ``ValueError``."""
    c = config
    attention = c.get("attention_type", "divided_space_time")
    if attention != "divided_space_time":
        raise ValueError(f"timesformer: attention_type {attention!r} is not built (only 'divided_space_time')")
    hidden, heads = int(c.get("hidden_size", 768)), int(c.get("num_attention_heads", 12))
    if heads <= 0 or hidden != heads * 64:
        raise ValueError(f"timesformer: head dimension must be 64 (hidden_size {hidden} / num_attention_heads {heads})")
    patch = c.get("patch_size", 16)
    if patch != PATCH:
        raise ValueError(f"timesformer: patch_size must be {PATCH}, got {patch!r}")
    image = c.get("image_size", 224)
    if isinstance(image, bool) or not isinstance(image, int) or image <= 0 or image % PATCH or image > MAX_IMAGE:
        raise ValueError(f"timesformer: image_size must be a multiple of {PATCH}, at most {MAX_IMAGE}, got {image!r}")
    frames = int(c.get("num_frames", 8))
    if not 1 <= frames <= MAX_FRAMES:
        raise ValueError(f"timesformer: num_frames must be in [1, {MAX_FRAMES}], got {frames}")
    if int(c.get("num_channels", 3)) != 3:
        raise ValueError("timesformer: num_channels must be 3")
    if c.get("hidden_act", "gelu") != "gelu":
        raise ValueError(f"timesformer: hidden_act {c.get('hidden_act')!r} is not built (only 'gelu')")
    ffn = int(c.get("intermediate_size", 3072))
    if ffn <= 0 or ffn % 32:
        raise ValueError(f"timesformer: intermediate_size must be a multiple of 32, got {ffn}")
    id2label = c.get("id2label") or {}
    labels = int(c.get("num_labels", len(id2label) or 400))
    if id2label and len(id2label) != labels:
        raise ValueError(f"timesformer: id2label has {len(id2label)} entries for {labels} labels")
    return {"image": image, "patch": PATCH, "frames": frames, "hidden": hidden, "layers": int(c.get("num_hidden_layers", 12)),
            "heads": heads, "ffn": ffn, "labels": labels, "ln_eps": float(c.get("layer_norm_eps", 1e-6)),
            "qkv_bias": bool(c.get("qkv_bias", True))}


def config_labels(config: dict, n: int) -> list[str]:
    """``id2label`` of a ``config.json`` (keys may be strings), else ``action_<i>``."""
    id2label = config.get("id2label") or {}
    lookup = {int(k): v for k, v in id2label.items()}
    return [str(lookup.get(i, f"action_{i}")) for i in range(n)]


def tensor_shapes(dims: dict) -> list:
    """``[(name, shape)]`` of the model's ``state_dict()`` in the library's order."""
    d, P, T = dims["hidden"], (dims["image"] // PATCH) ** 2, dims["frames"]
    out = [("timesformer.embeddings.cls_token", (1, 1, d)), ("timesformer.embeddings.position_embeddings", (1, 1 + P, d)),
           ("timesformer.embeddings.time_embeddings", (1, T, d)),
           ("timesformer.embeddings.patch_embeddings.projection.weight", (d, 3, PATCH, PATCH)),
           ("timesformer.embeddings.patch_embeddings.projection.bias", (d,))]

    def lin(name, rows, cols):
        out.extend([(name + ".weight", (rows, cols)), (name + ".bias", (rows,))])

    def lnorm(name):
        out.extend([(name + ".weight", (d,)), (name + ".bias", (d,))])

    for layer in range(dims["layers"]):
        p = f"timesformer.encoder.layer.{layer}."
        lnorm(p + "temporal_layernorm")
        lin(p + "temporal_attention.attention.qkv", 3 * d, d)
        lin(p + "temporal_attention.output.dense", d, d)
        lin(p + "temporal_dense", d, d)
        lnorm(p + "layernorm_before")
        lin(p + "attention.attention.qkv", 3 * d, d)
        lin(p + "attention.output.dense", d, d)
        lnorm(p + "layernorm_after")
        lin(p + "intermediate.dense", dims["ffn"], d)
        lin(p + "output.dense", d, dims["ffn"])
    lnorm("timesformer.layernorm")
    lin("classifier", dims["labels"], d)
    return out


def random_state(config: dict, seed: int = 5, classifier_gain: float = 8.0) -> dict:
    """Seeded weights of the exact shapes (benchmarks, tests: no checkpoint is reachable offline).  Linear layers draw
    N(0, 1 / fan_in), LayerNorm weights sit around 1, the embedding tables are small; the classifier is ``classifier_gain``
    times larger, which spreads the logits of the (unit-variance) final LayerNorm output over about +-3 gain, so that the
    five largest are well separated (tests/test_actions_gpu.py asserts the gap it relies on)."""
    dims = timesformer_dims(config)
    rng = np.random.default_rng(seed)
    sd = {}
    for name, shape in tensor_shapes(dims):
        if name.endswith("layernorm.weight") or name.endswith("layernorm_before.weight") or name.endswith("layernorm_after.weight"):
            v = rng.uniform(0.8, 1.2, shape)
        elif name.endswith(".bias"):
            v = 0.05 * rng.standard_normal(shape)
        elif "embeddings." in name and not name.endswith("projection.weight"):
            v = 0.2 * rng.standard_normal(shape)
        else:
            fan_in = int(np.prod(shape[1:]))
            gain = classifier_gain if name == "classifier.weight" else 1.0
            v = gain * rng.standard_normal(shape) / np.sqrt(fan_in)
        sd[name] = v.astype(np.float32)
    return sd


def read_state(root: Path) -> dict:
    """``model.safetensors`` (the reader of ``transcribe.py``) or ``pytorch_model.bin`` (torch's restricted unpickler)."""
    if (root / "model.safetensors").exists():
        from .transcribe import read_safetensors

        return read_safetensors(root / "model.safetensors")
    if (root / "pytorch_model.bin").exists():
        import torch

        return np_state(torch.load(str(root / "pytorch_model.bin"), map_location="cpu", weights_only=True))
    raise FileNotFoundError(f"{root} has neither model.safetensors nor pytorch_model.bin")


def preprocessing(config: dict, preprocessor_config: dict | None = None) -> dict:
    """``{"shortest_edge", "crop", "mean", "std"}``: shortest edge = crop = ``image_size``, mean 0.45, std 0.225 unless a
    ``preprocessor_config.json`` says otherwise.  The crop must be the model's ``image_size`` (no embedding
    interpolation)."""
    image = timesformer_dims(config)["image"]
    pc = preprocessor_config or {}
    size, crop = pc.get("size", {}), pc.get("crop_size", {})
    edge = size.get("shortest_edge", image) if isinstance(size, dict) else size
    ch, cw = (crop.get("height", image), crop.get("width", image)) if isinstance(crop, dict) else (crop, crop)
    if pc.get("do_center_crop", True) is False or pc.get("do_resize", True) is False:
        raise ValueError("timesformer: preprocessing without resize or centre crop is not built")
    if ch != image or cw != image:
        raise ValueError(f"timesformer: crop_size {ch} x {cw} must equal image_size {image} (embedding interpolation is not built)")
    if isinstance(edge, bool) or not isinstance(edge, int) or edge < image:
        raise ValueError(f"timesformer: shortest_edge must be an integer >= image_size {image}, got {edge!r}")

    def triple(v, default):
        v = default if v is None else v
        v = [float(v)] * 3 if isinstance(v, (int, float)) else [float(x) for x in v]
        if len(v) != 3:
            raise ValueError("timesformer: image_mean / image_std must have three entries")
        return tuple(v)

    return {"shortest_edge": int(edge), "crop": image, "mean": triple(pc.get("image_mean"), DEFAULT_MEAN),
            "std": triple(pc.get("image_std"), DEFAULT_STD)}


def clip_tables(h: int, w: int, shortest_edge: int, crop: int):
    """Pillow's tables for ``h x w`` frames, resized so that the short edge is ``shortest_edge`` (the long one
    ``int(edge * long / short)``) and centre-cropped to ``crop`` (offsets ``(dim - crop) // 2``): the ``crop`` rows of each
    axis's table that survive, ``(xbounds, xk, kx, ybounds, yk, ky)``."""
    if h <= w:
        rh, rw = shortest_edge, int(shortest_edge * w / h)
    else:
        rh, rw = int(shortest_edge * h / w), shortest_edge
    if rh < crop or rw < crop:
        raise ValueError(f"timesformer: {h} x {w} frames resize to {rh} x {rw}, smaller than the {crop} crop")
    top, left = (rh - crop) // 2, (rw - crop) // 2
    xb, xk, kx = resize_tables(w, rw)
    yb, yk, ky = resize_tables(h, rh)
    cut = lambda a, o: np.ascontiguousarray(a[o:o + crop])  # noqa: E731
    return cut(xb, left), cut(xk, left), kx, cut(yb, top), cut(yk, top), ky


class ActionRecognizer:
    """``TimesformerForVideoClassification(config).load_state_dict(state)`` + the image processor + softmax / top-k."""

    def __init__(self, state: dict, config: dict, labels: list[str] | None = None, preprocessor_config: dict | None = None):
        self.config = dict(config)
        self.dims = d = timesformer_dims(config)
        self.pre = preprocessing(config, preprocessor_config)
        self.labels = list(labels) if labels is not None else config_labels(config, d["labels"])
        if len(self.labels) != d["labels"]:
            raise ValueError(f"timesformer: {len(self.labels)} label names for {d['labels']} labels")
        self.frames, self.image, self.num_labels = d["frames"], d["image"], d["labels"]
        self.patches = (d["image"] // PATCH) ** 2
        self._tables = {}
        self._h = Handle("timesformer", d["image"], d["patch"], d["frames"], d["hidden"], d["layers"], d["heads"], d["ffn"],
                         d["labels"], d["ln_eps"])
        self._h.or_close(self._load, state)

    def _load(self, state: dict) -> None:
        sd = np_state(state)
        if not self.dims["qkv_bias"]:  # the checkpoint has no qkv biases: zeros
            for name, shape in tensor_shapes(self.dims):
                if name.endswith("qkv.bias"):
                    sd.setdefault(name, np.zeros(shape, np.float32))
        for name, shape in tensor_shapes(self.dims):
            if name in sd and tuple(sd[name].shape) != shape:
                raise ValueError(f"{name}: expected shape {shape}, got {tuple(sd[name].shape)} "
                                 "(position / time embedding interpolation is not built: the checkpoint must match the config)")
        self._h.set_tensors(sd)
        mean, std = (np.asarray(self.pre[k], np.float32) for k in ("mean", "std"))
        _lib.check(self._h.eioku_timesformer_set_norm(ptr(mean), ptr(std)), "eioku_timesformer_set_norm")

    @classmethod
    def from_cache(cls, cache_dir, model_name: str = DEFAULT_MODEL, seed: int | None = None):
        """``<cache>/timesformer/<model_name>/{config.json, model.safetensors | pytorch_model.bin[,
        preprocessor_config.json]}``.  A missing directory is a ``FileNotFoundError`` unless ``seed`` asks for
        ``random_state`` of the base configuration (or of the directory's ``config.json`` when only the weights are
        missing)."""
        root = Path(cache_dir) / "timesformer" / model_name
        cfg_path = root / "config.json"
        if not cfg_path.exists():
            if seed is None:
                raise FileNotFoundError(f"{cfg_path} not found (no weights to detect actions with)")
            return cls(random_state({}, seed), {})
        config = json.loads(cfg_path.read_text())
        pc_path = root / "preprocessor_config.json"
        pc = json.loads(pc_path.read_text()) if pc_path.exists() else None
        try:
            state = read_state(root)
        except FileNotFoundError:
            if seed is None:
                raise
            state = random_state(config, seed)
        return cls(state, config, config_labels(config, timesformer_dims(config)["labels"]), pc)

    def _tab(self, h: int, w: int):
        key = (h, w)
        if key not in self._tables:
            self._tables[key] = clip_tables(h, w, self.pre["shortest_edge"], self.pre["crop"])
        return self._tables[key]

    def _shape(self, clips_bgr):
        if len(clips_bgr.shape) != 5 or int(clips_bgr.shape[1]) != self.frames or int(clips_bgr.shape[4]) != 3:
            raise ValueError(f"expected (n, {self.frames}, h, w, 3) BGR clips, got {tuple(clips_bgr.shape)}")
        n, _, h, w, _ = (int(s) for s in clips_bgr.shape)
        return n, h, w

    def _input(self, clips_bgr):
        if on_device(clips_bgr):
            import torch

            if clips_bgr.dtype != torch.uint8:
                raise ValueError("expected uint8 frames")
            return clips_bgr.contiguous()
        return np.ascontiguousarray(clips_bgr, dtype=np.uint8)

    @staticmethod
    def upload(frames_bgr: np.ndarray):
        """Host uint8 frames -> a CUDA tensor (the one copy ``detect_actions`` makes of a batch)."""
        import torch

        return torch.from_numpy(np.ascontiguousarray(frames_bgr, dtype=np.uint8)).cuda()

    def preprocess(self, clips_bgr):
        """-> ``(fp16 (n, P, T, 768) patch rows, uint8 (n, T, S, S, 3) resized and cropped RGB)`` CUDA tensors."""
        import torch

        n, h, w = self._shape(clips_bgr)
        clips_bgr = self._input(clips_bgr)
        xb, xk, kx, yb, yk, ky = self._tab(h, w)
        dev = clips_bgr.device if on_device(clips_bgr) else torch.device("cuda", torch.cuda.current_device())
        x = torch.empty((n, self.patches, self.frames, 3 * PATCH * PATCH), dtype=torch.float16, device=dev)
        u8 = torch.empty((n, self.frames, self.image, self.image, 3), dtype=torch.uint8, device=dev)
        _lib.check(self._h.eioku_timesformer_preprocess(ptr(clips_bgr), n, h, w, ptr(xb), ptr(xk), kx, ptr(yb), ptr(yk), ky, ptr(x),
                                                        ptr(u8), _lib.MEM_DEVICE if on_device(clips_bgr) else _lib.MEM_HOST,
                                                        current_stream(x)), "eioku_timesformer_preprocess")
        return x, u8

    def forward_raw(self, patches, with_hidden: bool = False):
        """fp16 (n, P, T, 768) CUDA tensor -> float32 (n, labels) logits (CUDA) [, float32 (n, 1 + P T, hidden) residual
        stream before the final LayerNorm, in the model's token order]."""
        import torch

        n = int(patches.shape[0])
        if tuple(patches.shape[1:]) != (self.patches, self.frames, 3 * PATCH * PATCH) or patches.dtype != torch.float16:
            raise ValueError(f"expected fp16 (n, {self.patches}, {self.frames}, {3 * PATCH * PATCH}) patch rows")
        logits = torch.empty((n, self.num_labels), dtype=torch.float32, device=patches.device)
        hidden = (torch.empty((n, 1 + self.patches * self.frames, self.dims["hidden"]), dtype=torch.float32, device=patches.device)
                  if with_hidden else None)
        _lib.check(self._h.eioku_timesformer_forward(ptr(patches.contiguous()), n, ptr(logits), ptr(hidden), current_stream(patches)),
                   "eioku_timesformer_forward")
        return (logits, hidden) if with_hidden else logits

    def topk(self, logits, top_k: int = 5):
        """float32 (n, labels) CUDA logits -> ``(probs float32 (n, top_k), ids int32 (n, top_k))`` CUDA tensors."""
        import torch

        n = int(logits.shape[0])
        probs = torch.empty((n, top_k), dtype=torch.float32, device=logits.device)
        ids = torch.empty((n, top_k), dtype=torch.int32, device=logits.device)
        _lib.check(self._h.eioku_timesformer_topk(ptr(logits.contiguous()), n, int(top_k), ptr(probs), ptr(ids), current_stream(logits)),
                   "eioku_timesformer_topk")
        return probs, ids

    def classify(self, clips_bgr, top_k: int = 5, with_logits: bool = False):
        """BGR uint8 ``(n, T, h, w, 3)`` (numpy: staged; CUDA tensor: zero copy) -> ``(probs float32 (n, top_k), ids int32
        (n, top_k))`` numpy arrays in descending probability order (+ logits (n, labels) when asked)."""
        n, h, w = self._shape(clips_bgr)
        clips_bgr = self._input(clips_bgr)
        top_k = max(1, min(int(top_k), self.num_labels))
        xb, xk, kx, yb, yk, ky = self._tab(h, w)
        dev = on_device(clips_bgr)
        if dev:
            import torch

            probs = torch.empty((n, top_k), dtype=torch.float32, device=clips_bgr.device)
            ids = torch.empty((n, top_k), dtype=torch.int32, device=clips_bgr.device)
            logits = torch.empty((n, self.num_labels), dtype=torch.float32, device=clips_bgr.device) if with_logits else None
        else:
            probs = np.empty((n, top_k), np.float32)
            ids = np.empty((n, top_k), np.int32)
            logits = np.empty((n, self.num_labels), np.float32) if with_logits else None
        _lib.check(self._h.eioku_timesformer_classify(ptr(clips_bgr), n, h, w, ptr(xb), ptr(xk), kx, ptr(yb), ptr(yk), ky, top_k,
                                                      ptr(probs), ptr(ids), ptr(logits), _lib.MEM_DEVICE if dev else _lib.MEM_HOST,
                                                      current_stream(clips_bgr)), "eioku_timesformer_classify")
        if dev:
            probs, ids = probs.cpu().numpy(), ids.cpu().numpy()
            logits = logits.cpu().numpy() if with_logits else None
        return (probs, ids, logits) if with_logits else (probs, ids)

    def last_flops(self) -> float:
        return self._h.doubles("last_flops")[0]

    def last_ms(self) -> dict:
        pre, enc, head = self._h.doubles("last_ms", 3)
        return {"preprocess": pre, "encoder": enc, "head": head}

    def close(self):
        self._h.close()


# ---- the window rule of ModelManager.detect_actions ---------------------------------------------------------------------
def action_settings(config: dict, frames: int | None = None, labels: int | None = None) -> dict:
    """``model_name``, ``frame_interval``, ``clip_stride`` (default: the checkpoint's frame count) and ``top_k`` (clamped to
    ``[1, labels]``) of an ``action_detection`` task; bad values are a ``ValueError``."""
    def integer(key, default, lo):
        v = config.get(key, default)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
            raise ValueError(f"action_detection: {key} must be an integer >= {lo}, got {v!r}")
        return int(v)

    name = config.get("model_name", DEFAULT_MODEL)
    if not isinstance(name, str) or not name or "/" in name or name in (".", ".."):
        raise ValueError(f"action_detection: model_name must be a directory name, got {name!r}")
    seconds = config.get("frame_interval", 1)
    if isinstance(seconds, bool) or not isinstance(seconds, (int, float, np.integer, np.floating)) or not seconds >= 0:
        raise ValueError(f"action_detection: frame_interval must be a number >= 0, got {seconds!r}")
    top_k = integer("top_k", 5, 1)
    out = {"model_name": name, "frame_interval": seconds, "top_k": top_k if labels is None else min(top_k, labels)}
    out["clip_stride"] = integer("clip_stride", frames, 1) if (frames is not None or "clip_stride" in config) else None
    return out


def clip_windows(n_sampled: int, frames: int, stride: int) -> list:
    """Clips over ``n_sampled`` sampled frames: clip c is sampled frames ``[c stride, c stride + frames)``, a trailing
    partial window is dropped; a video with no full window is one clip padded with its last frame.  ``[(first, last
    real)]`` as indices into the sampled sequence."""
    if n_sampled <= 0:
        return []
    if n_sampled < frames:
        return [(0, n_sampled - 1)]
    return [(s, s + frames - 1) for s in range(0, n_sampled - frames + 1, stride)]
