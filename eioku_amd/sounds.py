"""Sound tagging (Audio Spectrogram Transformer on AudioSet labels) on the HIP kernels of ``csrc/sounds.hip``.

Music, applause, laughter, engines, sirens, barking: the sounds a transcript does not hold.  The model is Hugging Face
``ASTForAudioClassification`` (``MIT/ast-finetuned-audioset-10-10-0.4593``, 527 labels): its ``state_dict()`` names (both the
current ``layers.N.attention.q_proj`` layout and the published file's older ``encoder.layer.N.attention.attention.query``
one), its ``config.json`` keys, and the arithmetic of ``ASTFeatureExtractor``'s numpy path (``audio_utils.spectrogram``: the
waveform in [-1, 1], Hann window, Kaldi-scale mel triangles).  The host builds the window and the mel matrix and plans the
windows over the file; everything else runs on the device behind ``eioku_ast_classify``.  No CPU fallback.

Scores are sigmoids of the logits: AudioSet is multi-label and the model was trained with binary cross-entropy (the
``audio-classification`` pipeline of ``transformers`` applies a softmax instead).
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

from . import _lib
from ._buffers import current_stream, on_device, ptr
from ._handle import Handle
from ._state import np_state

SAMPLE_RATE = 16000
FRAME, SHIFT, FFT_BINS = 400, 160, 257
PATCH = 16
MAX_MEL = 128
MAX_TOKENS = 4094
MAX_WINDOWS = 64  # per device call
DEFAULT_MODEL = "ast-finetuned-audioset-10-10-0.4593"
DEFAULT_MEAN, DEFAULT_STD = -4.2677393, 4.5689974
_PREFIX = "audio_spectrogram_transformer."


def ast_dims(config: dict) -> dict:
    """The dimensions the library needs from a ``config.json``; what the kernels do not build is a ``ValueError``."""
    c = config
    hidden, heads = int(c.get("hidden_size", 768)), int(c.get("num_attention_heads", 12))
    if heads <= 0 or hidden != heads * 64:
        raise ValueError(f"ast: head dimension must be 64 (hidden_size {hidden} / num_attention_heads {heads})")
    if c.get("patch_size", PATCH) != PATCH:
        raise ValueError(f"ast: patch_size must be {PATCH}, got {c.get('patch_size')!r}")
    mel, length = int(c.get("num_mel_bins", 128)), int(c.get("max_length", 1024))
    if not PATCH <= mel <= MAX_MEL:
        raise ValueError(f"ast: num_mel_bins must be in [{PATCH}, {MAX_MEL}], got {mel}")
    fs, ts = int(c.get("frequency_stride", 10)), int(c.get("time_stride", 10))
    if not 1 <= fs <= PATCH or not 1 <= ts <= PATCH:
        raise ValueError(f"ast: frequency_stride and time_stride must be in [1, {PATCH}], got {fs} and {ts}")
    if length < PATCH:
        raise ValueError(f"ast: max_length must be at least {PATCH}, got {length}")
    f, t = (mel - PATCH) // fs + 1, (length - PATCH) // ts + 1
    if f * t + 2 > MAX_TOKENS:
        raise ValueError(f"ast: at most {MAX_TOKENS} tokens, max_length {length} and the strides give {f * t + 2}")
    if c.get("hidden_act", "gelu") != "gelu":
        raise ValueError(f"ast: hidden_act {c.get('hidden_act')!r} is not built (only 'gelu')")
    if c.get("qkv_bias", True) is not True:
        raise ValueError("ast: qkv_bias must be true")
    ffn = int(c.get("intermediate_size", 3072))
    if ffn <= 0 or ffn % 32:
        raise ValueError(f"ast: intermediate_size must be a multiple of 32, got {ffn}")
    id2label = c.get("id2label") or {}
    labels = int(c.get("num_labels", len(id2label) or 527))
    if id2label and len(id2label) != labels:
        raise ValueError(f"ast: id2label has {len(id2label)} entries for {labels} labels")
    if labels < 1:
        raise ValueError(f"ast: num_labels must be at least 1, got {labels}")
    return {"mel": mel, "max_length": length, "fstride": fs, "tstride": ts, "f": f, "t": t, "patches": f * t, "tokens": f * t + 2,
            "hidden": hidden, "layers": int(c.get("num_hidden_layers", 12)), "heads": heads, "ffn": ffn, "labels": labels,
            "ln_eps": float(c.get("layer_norm_eps", 1e-12))}


def config_labels(config: dict, n: int) -> list[str]:
    """``id2label`` of a ``config.json`` (keys may be strings), else ``sound_<i>``."""
    lookup = {int(k): v for k, v in (config.get("id2label") or {}).items()}
    return [str(lookup.get(i, f"sound_{i}")) for i in range(n)]


def preprocessing(config: dict, preprocessor_config: dict | None = None) -> dict:
    """``{"mean", "std"}`` of the normalisation ``(x - mean) / (2 std)``: AudioSet's unless a ``preprocessor_config.json`` says
    otherwise.  Its ``max_length`` and ``num_mel_bins`` must be the model's (no position-embedding interpolation)."""
    d = ast_dims(config)
    pc = preprocessor_config or {}
    for key, have in (("max_length", d["max_length"]), ("num_mel_bins", d["mel"])):
        if key in pc and pc[key] != have:
            raise ValueError(f"ast: preprocessor_config {key} {pc[key]!r} differs from config.json's {have}")
    if pc.get("sampling_rate", SAMPLE_RATE) != SAMPLE_RATE:
        raise ValueError(f"ast: sampling_rate must be {SAMPLE_RATE}, got {pc.get('sampling_rate')!r}")
    if pc.get("do_normalize", True) is not True:
        raise ValueError("ast: preprocessing without normalisation is not built")
    mean, std = float(pc.get("mean", DEFAULT_MEAN)), float(pc.get("std", DEFAULT_STD))
    if not std > 0:
        raise ValueError(f"ast: std must be positive, got {std}")
    return {"mean": mean, "std": std}


def ast_tables(num_mel_bins: int = 128):
    """``(window float64 (400,), mel float64 (257, num_mel_bins))``: the symmetric Hann window, and the triangular filters
    of ``num_mel_bins`` bands between 20 Hz and 8000 Hz, equally spaced and triangular on Kaldi's mel scale ``1127 ln(1 + f /
    700)``, no area normalisation, at the 257 bin frequencies ``31.25 i`` Hz of a 512-point FFT at 16 kHz."""
    i = np.arange(FRAME, dtype=np.float64)
    window = 0.5 - 0.5 * np.cos(2.0 * np.pi * i / (FRAME - 1))
    mel_of = lambda f: 1127.0 * np.log(1.0 + f / 700.0)  # noqa: E731
    edges = np.linspace(mel_of(20.0), mel_of(SAMPLE_RATE // 2), num_mel_bins + 2)
    bins = mel_of(SAMPLE_RATE / ((FFT_BINS - 1) * 2) * np.arange(FFT_BINS))
    width = np.diff(edges)
    slopes = edges[None, :] - bins[:, None]
    down, up = -slopes[:, :-2] / width[:-1], slopes[:, 2:] / width[1:]
    return window, np.maximum(0.0, np.minimum(down, up))


def tensor_shapes(dims: dict) -> list:
    """``[(name, shape)]`` of the model's ``state_dict()`` in the library's order (the current ``transformers`` layout)."""
    d = dims["hidden"]
    e = _PREFIX + "embeddings."
    out = [(e + "cls_token", (1, 1, d)), (e + "distillation_token", (1, 1, d)), (e + "position_embeddings", (1, dims["tokens"], d)),
           (e + "patch_embeddings.projection.weight", (d, 1, PATCH, PATCH)), (e + "patch_embeddings.projection.bias", (d,))]

    def lin(name, rows, cols):
        out.extend([(name + ".weight", (rows, cols)), (name + ".bias", (rows,))])

    def lnorm(name):
        out.extend([(name + ".weight", (d,)), (name + ".bias", (d,))])

    for layer in range(dims["layers"]):
        p = f"{_PREFIX}layers.{layer}."
        for proj in ("q_proj", "k_proj", "v_proj", "o_proj"):
            lin(p + "attention." + proj, d, d)
        lnorm(p + "layernorm_before")
        lnorm(p + "layernorm_after")
        lin(p + "mlp.fc1", dims["ffn"], d)
        lin(p + "mlp.fc2", d, dims["ffn"])
    lnorm(_PREFIX + "layernorm")
    lnorm("classifier.layernorm")
    lin("classifier.dense", dims["labels"], d)
    return out


_OLD_TO_NEW = (("attention.attention.query.", "attention.q_proj."), ("attention.attention.key.", "attention.k_proj."),
               ("attention.attention.value.", "attention.v_proj."), ("attention.output.dense.", "attention.o_proj."),
               ("intermediate.dense.", "mlp.fc1."), ("output.dense.", "mlp.fc2."))


def canonical_state(state: dict) -> dict:
    """A ``state_dict()`` in either layout -> the current one: the published checkpoint's ``encoder.layer.N.attention.attention.
    {query, key, value}``, ``attention.output.dense``, ``intermediate.dense`` and ``output.dense`` become ``layers.N.attention.
    {q, k, v, o}_proj`` and ``mlp.fc1 / fc2``; every other name is kept."""
    old = _PREFIX + "encoder.layer."
    out = {}
    for name, value in state.items():
        if name.startswith(old):
            name = _PREFIX + "layers." + name[len(old):]
            for a, b in _OLD_TO_NEW:
                if a in name:
                    name = name.replace(a, b)
                    break
        out[name] = value
    return out


def random_state(config: dict, seed: int = 5, classifier_gain: float = 2.0) -> dict:
    """Seeded weights of the exact shapes (benchmarks, tests: no checkpoint is reachable offline).  Linear layers draw
    N(0, 1 / fan_in), LayerNorm weights sit around 1, the tokens and the position table are small; ``classifier.dense`` is
    ``classifier_gain`` times larger, which spreads the logits of the (unit-variance) LayerNorm output over about +-3 gain:
    at 2 the largest sigmoids stay apart in fp32 (tests/test_sounds_gpu.py asserts the logit gap it relies on)."""
    dims = ast_dims(config)
    rng = np.random.default_rng(seed)
    sd = {}
    for name, shape in tensor_shapes(dims):
        if "layernorm" in name and name.endswith(".weight"):
            v = rng.uniform(0.8, 1.2, shape)
        elif name.endswith(".bias"):
            v = 0.05 * rng.standard_normal(shape)
        elif "embeddings." in name and not name.endswith("projection.weight"):
            v = 0.2 * rng.standard_normal(shape)
        else:
            fan_in = int(np.prod(shape[1:]))
            gain = classifier_gain if name == "classifier.dense.weight" else 1.0
            v = gain * rng.standard_normal(shape) / np.sqrt(fan_in)
        sd[name] = v.astype(np.float32)
    return sd


def window_samples(max_length: int) -> int:
    return FRAME + SHIFT * (max_length - 1)


def plan_windows(n_samples: int, max_length: int, stride_samples: int) -> list:
    """Windows of ``400 + 160 (max_length - 1)`` samples over a file: window w starts at ``w stride_samples``; it exists iff at
    least 400 samples remain there and, for w > 0, it holds a sample no earlier window covers.  ``[(first sample, valid
    frames)]`` with ``valid = min(max_length, 1 + (remaining - 400) // 160)``."""
    if stride_samples < 1:
        raise ValueError(f"stride_samples must be at least 1, got {stride_samples}")
    span = window_samples(max_length)
    plan = []
    w = 0
    while True:
        first = w * stride_samples
        remaining = n_samples - first
        if remaining < FRAME or (w > 0 and not remaining > span - stride_samples):
            return plan
        plan.append((first, min(max_length, 1 + (remaining - FRAME) // SHIFT)))
        w += 1


def sound_settings(config: dict, labels: int | None = None) -> dict:
    """``model_name``, ``window_stride`` (seconds), ``top_k``, ``min_score`` and ``batch_windows`` of a ``sound_detection`` task;
    bad values are a ``ValueError``."""
    def number(key, default, lo, hi):
        v = config.get(key, default)
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not lo <= v <= hi:
            raise ValueError(f"sound_detection: {key} must be a number in [{lo}, {hi}], got {v!r}")
        return float(v)

    def integer(key, default, lo, hi):
        v = config.get(key, default)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"sound_detection: {key} must be an integer in [{lo}, {hi}], got {v!r}")
        return int(v)

    name = config.get("model_name", DEFAULT_MODEL)
    if not isinstance(name, str) or not name or "/" in name or name in (".", ".."):
        raise ValueError(f"sound_detection: model_name must be a directory name, got {name!r}")
    top = 5 if labels is None else min(5, labels)
    return {"model_name": name, "window_stride": number("window_stride", 10.0, 0.01, float("inf")),
            "top_k": integer("top_k", top, 1, labels if labels is not None else 2 ** 31 - 1),
            "min_score": number("min_score", 0.0, 0.0, 1.0), "batch_windows": integer("batch_windows", 32, 1, MAX_WINDOWS)}


def sound_events(sounds: list, threshold: float) -> list:
    """Jump-navigation events from ``detect_sounds``' windows (host only): every run of consecutive windows in which a label
    scores at least ``threshold`` becomes ``{label, start_ms, end_ms, score}``: the run's first start, its last end, its
    largest score.  Ordered by start, then label."""
    events, running = [], {}
    for item in list(sounds) + [None]:
        present = {} if item is None else {l: s for l, s in zip(item["labels"], item["scores"]) if s >= threshold}
        for label in [l for l in running if l not in present]:
            events.append(running.pop(label))
        for label, score in present.items():
            if label in running:
                ev = running[label]
                ev["end_ms"], ev["score"] = item["end_ms"], max(ev["score"], score)
            else:
                running[label] = {"label": label, "start_ms": item["start_ms"], "end_ms": item["end_ms"], "score": score}
    return sorted(events, key=lambda e: (e["start_ms"], e["label"]))


class SoundTagger:
    """``ASTForAudioClassification(config).load_state_dict(state)`` + the feature extractor + sigmoid / top-k."""

    def __init__(self, state: dict, config: dict, labels: list[str] | None = None, preprocessor_config: dict | None = None):
        self.config = dict(config)
        self.dims = d = ast_dims(config)
        self.pre = preprocessing(config, preprocessor_config)
        self.labels = list(labels) if labels is not None else config_labels(config, d["labels"])
        if len(self.labels) != d["labels"]:
            raise ValueError(f"ast: {len(self.labels)} label names for {d['labels']} labels")
        self.max_length, self.mel, self.patches, self.num_labels = d["max_length"], d["mel"], d["patches"], d["labels"]
        self.window_samples = window_samples(d["max_length"])
        self._ms, self._flops = {"features": 0.0, "encoder": 0.0, "head": 0.0}, 0.0
        window, mel = ast_tables(d["mel"])
        mel = np.ascontiguousarray(mel, dtype=np.float64)
        self._h = Handle("ast", d["mel"], d["max_length"], d["fstride"], d["tstride"], d["hidden"], d["layers"], d["heads"], d["ffn"],
                         d["labels"], d["ln_eps"], ptr(window), ptr(mel), self.pre["mean"], self.pre["std"])
        self._h.or_close(self._load, state)

    def _load(self, state: dict) -> None:
        sd = canonical_state(np_state(state))
        for name, shape in tensor_shapes(self.dims):
            if name in sd and tuple(sd[name].shape) != shape:
                raise ValueError(f"{name}: expected shape {shape}, got {tuple(sd[name].shape)} "
                                 "(position-embedding interpolation is not built: the checkpoint must match the config)")
        self._h.set_tensors(sd)

    @classmethod
    def from_cache(cls, cache_dir, model_name: str = DEFAULT_MODEL, seed: int | None = None):
        """``<cache>/ast/<model_name>/{config.json, model.safetensors[, preprocessor_config.json]}``.  A missing directory
        is a ``FileNotFoundError`` unless ``seed`` asks for ``random_state`` of the published configuration (or of the
        directory's ``config.json`` when only the weights are missing)."""
        root = Path(cache_dir) / "ast" / model_name
        cfg_path = root / "config.json"
        if not cfg_path.exists():
            if seed is None:
                raise FileNotFoundError(f"{cfg_path} not found (no weights to tag sounds with)")
            return cls(random_state({}, seed), {})
        config = json.loads(cfg_path.read_text())
        pc_path = root / "preprocessor_config.json"
        pc = json.loads(pc_path.read_text()) if pc_path.exists() else None
        if (root / "model.safetensors").exists():
            from .transcribe import read_safetensors

            state = read_safetensors(root / "model.safetensors")
        elif seed is None:
            raise FileNotFoundError(f"{root} has no model.safetensors")
        else:
            state = random_state(config, seed)
        return cls(state, config, config_labels(config, ast_dims(config)["labels"]), pc)

    @staticmethod
    def _device():
        import torch

        return torch.device("cuda", torch.cuda.current_device())

    def set_audio(self, samples) -> None:
        """The file's 16 kHz mono float32 samples in [-1, 1] (numpy: uploaded once; CUDA tensor: copied on the device)."""
        if on_device(samples):
            import torch

            s = samples.reshape(-1).to(torch.float32).contiguous()
        else:
            s = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
        n = int(s.shape[0])
        _lib.check(self._h.eioku_ast_set_audio(ptr(s) if n else None, n, _lib.MEM_DEVICE if on_device(s) else _lib.MEM_HOST,
                                               current_stream(s)), "eioku_ast_set_audio")

    @staticmethod
    def _plan(plan) -> np.ndarray:
        return np.ascontiguousarray(plan, dtype=np.int32).reshape(-1, 2)

    def features(self, samples, plan):
        """K29a and K29b alone: ``plan`` rows ``(first sample, valid frames)`` (at most 64) -> ``(float32 (m, max_length, mel)
        normalised log-mel spectrogram, fp16 (m, P, 256) patch rows)`` CUDA tensors."""
        import torch

        self.set_audio(samples)
        p = self._plan(plan)
        dev = self._device()
        spec = torch.empty((len(p), self.max_length, self.mel), dtype=torch.float32, device=dev)
        rows = torch.empty((len(p), self.patches, PATCH * PATCH), dtype=torch.float16, device=dev)
        _lib.check(self._h.eioku_ast_features(ptr(p), len(p), ptr(spec), ptr(rows), current_stream(spec)), "eioku_ast_features")
        return spec, rows

    def forward_raw(self, patches, with_hidden: bool = False):
        """fp16 (m, P, 256) CUDA tensor -> float32 (m, labels) logits (CUDA) [, float32 (m, P + 2, hidden) residual stream
        before the final LayerNorm: CLS, the distillation token, then the patches]."""
        import torch

        m = int(patches.shape[0])
        if tuple(patches.shape[1:]) != (self.patches, PATCH * PATCH) or patches.dtype != torch.float16:
            raise ValueError(f"expected fp16 (m, {self.patches}, {PATCH * PATCH}) patch rows")
        logits = torch.empty((m, self.num_labels), dtype=torch.float32, device=patches.device)
        hidden = (torch.empty((m, self.dims["tokens"], self.dims["hidden"]), dtype=torch.float32, device=patches.device)
                  if with_hidden else None)
        _lib.check(self._h.eioku_ast_forward(ptr(patches.contiguous()), m, ptr(logits), ptr(hidden), current_stream(patches)),
                   "eioku_ast_forward")
        return (logits, hidden) if with_hidden else logits

    def topk(self, logits, top_k: int = 5):
        """float32 (m, labels) CUDA logits -> ``(scores float32 (m, top_k), ids int32 (m, top_k))`` CUDA tensors."""
        import torch

        m = int(logits.shape[0])
        scores = torch.empty((m, top_k), dtype=torch.float32, device=logits.device)
        ids = torch.empty((m, top_k), dtype=torch.int32, device=logits.device)
        _lib.check(self._h.eioku_ast_topk(ptr(logits.contiguous()), m, int(top_k), ptr(scores), ptr(ids), current_stream(logits)),
                   "eioku_ast_topk")
        return scores, ids

    def classify(self, samples, plan, top_k: int = 5, batch_windows: int = 32, with_logits: bool = False, with_hidden: bool = False):
        """Samples (numpy or CUDA tensor; ``None``: the audio of the last ``set_audio``) and ``plan`` rows ``(first sample,
        valid frames)`` -> ``(scores float32 (m, top_k), ids int32 (m, top_k))`` numpy arrays in descending score order (+
        logits (m, labels), + hidden (m, P + 2, hidden) when asked), ``batch_windows`` (at most 64) windows per device call."""
        if not 1 <= int(batch_windows) <= MAX_WINDOWS:
            raise ValueError(f"batch_windows must be in [1, {MAX_WINDOWS}], got {batch_windows}")
        if not 1 <= int(top_k) <= self.num_labels:
            raise ValueError(f"top_k must be in [1, {self.num_labels}], got {top_k}")
        if samples is not None:
            self.set_audio(samples)
        p = self._plan(plan)
        m, top_k = len(p), int(top_k)
        scores, ids = np.empty((m, top_k), np.float32), np.empty((m, top_k), np.int32)
        logits = np.empty((m, self.num_labels), np.float32) if with_logits else None
        hidden = np.empty((m, self.dims["tokens"], self.dims["hidden"]), np.float32) if with_hidden else None
        self._ms, self._flops = {"features": 0.0, "encoder": 0.0, "head": 0.0}, 0.0
        for a in range(0, m, int(batch_windows)):
            b = min(m, a + int(batch_windows))
            part = np.ascontiguousarray(p[a:b])
            _lib.check(self._h.eioku_ast_classify(ptr(part), b - a, top_k, ptr(scores[a:b]), ptr(ids[a:b]),
                                                  ptr(logits[a:b]) if with_logits else None,
                                                  ptr(hidden[a:b]) if with_hidden else None, _lib.MEM_HOST, None),
                       "eioku_ast_classify")
            for key, v in zip(("features", "encoder", "head"), self._h.doubles("last_ms", 3)):
                self._ms[key] += v
            self._flops += self._h.doubles("last_flops")[0]
        out = (scores, ids)
        if with_logits:
            out += (logits,)
        if with_hidden:
            out += (hidden,)
        return out

    def last_flops(self) -> float:
        """GEMM, attention and head FLOPs of the last ``classify`` (all its device calls)."""
        return self._flops

    def last_ms(self) -> dict:
        """Device milliseconds of the last ``classify`` per stage, summed over its device calls."""
        return dict(self._ms)

    def close(self):
        self._h.close()
