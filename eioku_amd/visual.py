"""Search videos by what they show: CLIP frame and text embeddings on the HIP kernels of ``csrc/clip.hip`` (K26).

The model is Hugging Face ``CLIPModel``: its ``state_dict()`` names, its ``config.json`` keys (``text_config`` /
``vision_config``), the arithmetic of ``CLIPImageProcessor`` (Pillow's bicubic resize of the short edge, centre crop, ``x /
255``, normalise) and of ``CLIPTokenizer`` (NFC, whitespace, lower case, CLIP's piece pattern, byte-level BPE with ``</w>``).
The host computes Pillow's coefficient tables for the rows and columns the crop keeps and tokenises the queries; everything
else runs on the device behind ``eioku_clip_encode_images`` / ``eioku_clip_encode_text``.  No CPU fallback.

``VisualSearchEngine`` puts the frame vectors into the ``VectorStore`` the transcript search already uses (flat index,
filters, deletes), so a video with no speech can be found, and a frame can be asked for in words or by another frame.
"""
from __future__ import annotations

import json
import re
import unicodedata
from pathlib import Path

import numpy as np

from . import _lib
from ._buffers import current_stream, on_device, ptr
from ._handle import Handle
from ._state import np_state
from .actions import read_state

MAX_IMAGE = 448
MAX_POSITIONS = 77
PRECISION_BITS = 22
DEFAULT_MODEL = "clip-vit-base-patch32"
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
BOS, EOT = "<|startoftext|>", "<|endoftext|>"
_ACTS = {"quick_gelu": 0, "gelu": 1}


# ---- configuration ----------------------------------------------------------------------------------------------------------
def clip_dims(config: dict) -> dict:
    """The dimensions the library needs from a ``config.json`` (defaults: ``CLIPConfig``'s, i.e. ViT-B/32); what the kernels
    do not build is a ``ValueError``."""
    tc, vc = config.get("text_config") or {}, config.get("vision_config") or {}

    def tower(c, what, hidden, heads, ffn):
        hidden, heads = int(c.get("hidden_size", hidden)), int(c.get("num_attention_heads", heads))
        if heads <= 0 or hidden != heads * 64:
            raise ValueError(f"clip: {what} head dimension must be 64 (hidden_size {hidden} / num_attention_heads {heads})")
        ffn = int(c.get("intermediate_size", ffn))
        if ffn <= 0 or ffn % 32:
            raise ValueError(f"clip: {what} intermediate_size must be a multiple of 32, got {ffn}")
        return {"hidden": hidden, "layers": int(c.get("num_hidden_layers", 12)), "heads": heads, "ffn": ffn}

    vision, text = tower(vc, "vision", 768, 12, 3072), tower(tc, "text", 512, 8, 2048)
    image, patch = vc.get("image_size", 224), vc.get("patch_size", 32)
    for key, v in (("image_size", image), ("patch_size", patch)):
        if isinstance(v, bool) or not isinstance(v, int) or v <= 0:
            raise ValueError(f"clip: {key} must be a positive integer, got {v!r}")
    if image % patch or image > MAX_IMAGE:
        raise ValueError(f"clip: image_size must be a multiple of patch_size {patch}, at most {MAX_IMAGE}, got {image}")
    if int(vc.get("num_channels", 3)) != 3:
        raise ValueError("clip: num_channels must be 3")
    positions = int(tc.get("max_position_embeddings", 77))
    if not 1 <= positions <= MAX_POSITIONS:
        raise ValueError(f"clip: max_position_embeddings must be in [1, {MAX_POSITIONS}], got {positions}")
    acts = {tc.get("hidden_act", "quick_gelu"), vc.get("hidden_act", "quick_gelu")}
    eps = {float(tc.get("layer_norm_eps", 1e-5)), float(vc.get("layer_norm_eps", 1e-5))}
    if len(acts) != 1 or len(eps) != 1:
        raise ValueError(f"clip: the towers must share hidden_act and layer_norm_eps (got {sorted(acts)}, {sorted(eps)})")
    act = acts.pop()
    if act not in _ACTS:
        raise ValueError(f"clip: hidden_act {act!r} is not built (only {sorted(_ACTS)})")
    vision.update(image=image, patch=patch)
    text.update(vocab=int(tc.get("vocab_size", 49408)), positions=positions)
    return {"vision": vision, "text": text, "projection": int(config.get("projection_dim", 512)), "ln_eps": eps.pop(), "act": act,
            "eos_token_id": int(tc.get("eos_token_id", 49407))}


def tensor_shapes(dims: dict) -> list:
    """``[(name, shape)]`` of ``CLIPModel.state_dict()`` in the library's order (no ``logit_scale``, no ``position_ids``)."""
    out = []

    def lin(name, rows, cols):
        out.extend([(name + ".weight", (rows, cols)), (name + ".bias", (rows,))])

    def lnorm(name, d):
        out.extend([(name + ".weight", (d,)), (name + ".bias", (d,))])

    def layers(model, t):
        d = t["hidden"]
        for layer in range(t["layers"]):
            p = f"{model}.encoder.layers.{layer}."
            for proj in ("k_proj", "v_proj", "q_proj", "out_proj"):
                lin(p + "self_attn." + proj, d, d)
            lnorm(p + "layer_norm1", d)
            lin(p + "mlp.fc1", t["ffn"], d)
            lin(p + "mlp.fc2", d, t["ffn"])
            lnorm(p + "layer_norm2", d)

    t, v = dims["text"], dims["vision"]
    out.append(("text_model.embeddings.token_embedding.weight", (t["vocab"], t["hidden"])))
    out.append(("text_model.embeddings.position_embedding.weight", (t["positions"], t["hidden"])))
    layers("text_model", t)
    lnorm("text_model.final_layer_norm", t["hidden"])
    out.append(("vision_model.embeddings.class_embedding", (v["hidden"],)))
    out.append(("vision_model.embeddings.patch_embedding.weight", (v["hidden"], 3, v["patch"], v["patch"])))
    out.append(("vision_model.embeddings.position_embedding.weight", (1 + (v["image"] // v["patch"]) ** 2, v["hidden"])))
    lnorm("vision_model.pre_layrnorm", v["hidden"])
    layers("vision_model", v)
    lnorm("vision_model.post_layernorm", v["hidden"])
    out.append(("visual_projection.weight", (dims["projection"], v["hidden"])))
    out.append(("text_projection.weight", (dims["projection"], t["hidden"])))
    return out


def random_state(config: dict, seed: int = 5) -> dict:
    """Seeded weights of the exact shapes (benchmarks, tests: no checkpoint is reachable offline).  Linear layers draw
    N(0, 1 / fan_in), LayerNorm weights sit around 1, the embedding tables are small."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, shape in tensor_shapes(clip_dims(config)):
        if "norm" in name and name.endswith(".weight"):
            v = rng.uniform(0.8, 1.2, shape)
        elif name.endswith(".bias"):
            v = 0.05 * rng.standard_normal(shape)
        elif name.endswith(("class_embedding", "token_embedding.weight")):
            v = 0.5 * rng.standard_normal(shape)
        elif name.endswith("position_embedding.weight"):
            v = 0.2 * rng.standard_normal(shape)
        else:
            v = rng.standard_normal(shape) / np.sqrt(int(np.prod(shape[1:])))
        sd[name] = v.astype(np.float32)
    return sd


def preprocessing(config: dict, preprocessor_config: dict | None = None) -> dict:
    """``{"shortest_edge", "crop", "mean", "std"}``: shortest edge = crop = ``image_size`` and OpenAI's mean / std unless a
    ``preprocessor_config.json`` says otherwise.  The crop must be the model's ``image_size`` (no embedding interpolation)
    and the resample Pillow's bicubic (3)."""
    image = clip_dims(config)["vision"]["image"]
    pc = preprocessor_config or {}
    size, crop = pc.get("size", image), pc.get("crop_size", image)
    edge = size.get("shortest_edge", image) if isinstance(size, dict) else size
    ch, cw = (crop.get("height", image), crop.get("width", image)) if isinstance(crop, dict) else (crop, crop)
    if pc.get("do_center_crop", True) is False or pc.get("do_resize", True) is False:
        raise ValueError("clip: preprocessing without resize or centre crop is not built")
    if pc.get("resample", 3) != 3:
        raise ValueError(f"clip: resample {pc.get('resample')!r} is not built (only 3, bicubic)")
    if ch != image or cw != image:
        raise ValueError(f"clip: crop_size {ch} x {cw} must equal image_size {image} (embedding interpolation is not built)")
    if isinstance(edge, bool) or not isinstance(edge, int) or edge < image:
        raise ValueError(f"clip: shortest_edge must be an integer >= image_size {image}, got {edge!r}")

    def triple(v, default):
        v = [float(x) for x in (default if v is None else v)]
        if len(v) != 3:
            raise ValueError("clip: image_mean / image_std must have three entries")
        return tuple(v)

    return {"shortest_edge": int(edge), "crop": image, "mean": triple(pc.get("image_mean"), CLIP_MEAN),
            "std": triple(pc.get("image_std"), CLIP_STD)}


# ---- Pillow's bicubic tables ------------------------------------------------------------------------------------------------
def bicubic_tables(in_size: int, out_size: int):
    """Pillow ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for the bicubic filter (support 2, a = -0.5), whole axis
    ``in_size`` -> ``out_size``: ``(bounds int32 (out, 2) = first input index | taps, k int32 (out, ksize) taps x 2**22,
    ksize)``."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    xx = np.arange(out_size, dtype=np.float64)
    center = (xx + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)  # C (int) cast: values below zero are > -1 only when clamped
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.float64)[None, :]
    arg = np.abs((x + xmin[:, None] - center[:, None] + 0.5) * (1.0 / filterscale))
    a = -0.5
    near = ((a + 2.0) * arg - (a + 3.0)) * arg * arg + 1
    far = (((arg - 5) * arg + 8) * arg - 4) * a
    w = np.where(arg < 1.0, near, np.where(arg < 2.0, far, 0.0))
    w[x >= xmax[:, None]] = 0.0
    ww = np.zeros(out_size, np.float64)
    for t in range(ksize):  # Pillow sums the taps in index order
        ww = ww + w[:, t]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    scaled = w * (1 << PRECISION_BITS)
    k = np.where(w < 0, -0.5 + scaled, 0.5 + scaled).astype(np.int64)  # the C cast truncates toward zero
    k[x.repeat(out_size, 0) >= xmax[:, None]] = 0
    bounds = np.stack([xmin, xmax], 1).astype(np.int32)
    return np.ascontiguousarray(bounds), np.ascontiguousarray(k.astype(np.int32)), ksize


def image_tables(h: int, w: int, shortest_edge: int, crop: int):
    """Pillow's bicubic tables for ``h x w`` frames, resized so that the short edge is ``shortest_edge`` (the long one
    ``int(edge * long / short)``) and centre-cropped to ``crop`` (offsets ``(dim - crop) // 2``): the ``crop`` rows of each
    axis's table that survive, ``(xbounds, xk, kx, ybounds, yk, ky)``."""
    if h <= w:
        rh, rw = shortest_edge, int(shortest_edge * w / h)
    else:
        rh, rw = int(shortest_edge * h / w), shortest_edge
    if rh < crop or rw < crop:
        raise ValueError(f"clip: {h} x {w} frames resize to {rh} x {rw}, smaller than the {crop} crop")
    top, left = (rh - crop) // 2, (rw - crop) // 2
    xb, xk, kx = bicubic_tables(w, rw)
    yb, yk, ky = bicubic_tables(h, rh)
    cut = lambda a, o: np.ascontiguousarray(a[o:o + crop])  # noqa: E731
    return cut(xb, left), cut(xk, left), kx, cut(yb, top), cut(yk, top), ky


# ---- the tokenizer ----------------------------------------------------------------------------------------------------------
def _bytes_to_unicode() -> dict:
    """The byte -> printable character table of byte-level BPE (GPT-2's)."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, map(chr, cs)))


_CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")


def clip_pieces(text: str) -> list[str]:
    """CLIP's piece pattern ``<|startoftext|>|<|endoftext|>|'s|'t|'re|'ve|'m|'ll|'d|[\\p{L}]+|[\\p{N}]|[^\\s\\p{L}\\p{N}]+``
    as a scanner over ``unicodedata`` categories: at each position the alternatives in that order, each greedy."""
    def kind(ch):
        c = unicodedata.category(ch)
        return "L" if c[0] == "L" else "N" if c[0] == "N" else "S" if ch.isspace() else "O"

    out, i, n = [], 0, len(text)
    while i < n:
        hit = next((s for s in (BOS, EOT) + _CONTRACTIONS if text.startswith(s, i)), None)
        if hit:
            out.append(hit)
            i += len(hit)
            continue
        k = kind(text[i])
        if k == "S":
            i += 1
            continue
        j = i + 1
        if k != "N":  # a digit is a piece of its own
            while j < n and kind(text[j]) == k:
                j += 1
        out.append(text[i:j])
        i = j
    return out


class ClipTokenizer:
    """``CLIPTokenizer`` from ``vocab.json`` and ``merges.txt``: ids with BOS and EOT around them, truncated to
    ``positions`` (the first ``positions - 1`` ids, then EOT) and padded with the pad id.  Text is not repaired first
    (``transformers`` without ``ftfy`` does not either)."""

    def __init__(self, vocab_path, merges_path, positions: int = 77, pad_token: str = EOT):
        self.vocab = json.loads(Path(vocab_path).read_text(encoding="utf-8"))
        lines = Path(merges_path).read_text(encoding="utf-8").split("\n")
        if lines and lines[0].startswith("#version"):
            lines = lines[1:]
        pairs = [tuple(line.split()) for line in lines if line.strip()]
        self.ranks = {p: i for i, p in enumerate(pairs) if len(p) == 2}
        self.positions = int(positions)
        self.bos_id, self.eot_id = self.vocab[BOS], self.vocab[EOT]
        self.unk_id = self.eot_id
        self.pad_id = self.vocab[pad_token]
        self._byte = _bytes_to_unicode()
        self._cache: dict = {}

    @staticmethod
    def normalise(text: str) -> str:
        return re.sub(r"\s+", " ", unicodedata.normalize("NFC", text)).strip().lower()

    def _bpe(self, piece: str) -> list[str]:
        if piece in self._cache:
            return self._cache[piece]
        word = [self._byte[b] for b in piece.encode("utf-8")]
        word[-1] += "</w>"
        while len(word) > 1:
            rank, at = min((self.ranks.get((a, b), len(self.ranks)), i) for i, (a, b) in enumerate(zip(word, word[1:])))
            if rank == len(self.ranks):
                break
            a, b = word[at], word[at + 1]
            merged, i = [], 0
            while i < len(word):  # every occurrence of the best pair, left to right
                if i + 1 < len(word) and word[i] == a and word[i + 1] == b:
                    merged.append(a + b)
                    i += 2
                else:
                    merged.append(word[i])
                    i += 1
            word = merged
        self._cache[piece] = word
        return word

    def tokens(self, text: str) -> list[int]:
        """The ids of ``text`` alone: no BOS, EOT, truncation or padding."""
        ids = []
        for piece in clip_pieces(self.normalise(text)):
            if piece in (BOS, EOT):
                ids.append(self.vocab[piece])
            else:
                ids.extend(self.vocab.get(t, self.unk_id) for t in self._bpe(piece))
        return ids

    def encode(self, texts: list[str]):
        """-> ``(ids int32 (n, positions), lengths (n,))``; a length counts BOS and EOT."""
        ids = np.full((len(texts), self.positions), self.pad_id, np.int32)
        lengths = np.zeros(len(texts), np.int32)
        for row, text in enumerate(texts):
            seq = [self.bos_id] + self.tokens(text)[:self.positions - 2] + [self.eot_id]
            ids[row, :len(seq)] = seq
            lengths[row] = len(seq)
        return ids, lengths


def eot_positions(ids: np.ndarray, eos_token_id: int) -> np.ndarray:
    """Hugging Face's pooling rule: the first position holding ``eos_token_id``; for the legacy configurations whose
    ``eos_token_id`` is 2, the position of the largest id."""
    ids = np.asarray(ids)
    if eos_token_id == 2:
        return ids.argmax(-1).astype(np.int32)
    return (ids == eos_token_id).argmax(-1).astype(np.int32)


# ---- the model ----------------------------------------------------------------------------------------------------------------
class ClipModel:
    """``CLIPModel(config).load_state_dict(state)`` + the image processor + the tokenizer: frames and texts -> unit vectors of
    one space."""

    def __init__(self, state: dict, config: dict, preprocessor_config: dict | None = None, tokenizer: ClipTokenizer | None = None):
        self.config = dict(config)
        self.dims = d = clip_dims(config)
        self.pre = preprocessing(config, preprocessor_config)
        self.tokenizer = tokenizer
        v, t = d["vision"], d["text"]
        self.image, self.patch, self.projection_dim = v["image"], v["patch"], d["projection"]
        self.tokens = 1 + (v["image"] // v["patch"]) ** 2
        self.row_len = (3 * v["patch"] ** 2 + 31) // 32 * 32
        self.positions, self.eos_token_id = t["positions"], d["eos_token_id"]
        self._tables = {}
        self._h = Handle("clip", v["image"], v["patch"], v["hidden"], v["layers"], v["heads"], v["ffn"], t["vocab"], t["positions"],
                         t["hidden"], t["layers"], t["heads"], t["ffn"], d["projection"], d["ln_eps"], _ACTS[d["act"]])
        self._h.or_close(self._load, state)

    def _load(self, state: dict) -> None:
        sd = np_state(state)
        for name, shape in tensor_shapes(self.dims):
            if name in sd and tuple(sd[name].shape) != shape:
                raise ValueError(f"{name}: expected shape {shape}, got {tuple(sd[name].shape)} "
                                 "(position embedding interpolation is not built: the checkpoint must match the config)")
        self._h.set_tensors(sd)
        mean, std = (np.asarray(self.pre[k], np.float32) for k in ("mean", "std"))
        _lib.check(self._h.eioku_clip_set_norm(ptr(mean), ptr(std)), "eioku_clip_set_norm")

    @classmethod
    def from_cache(cls, cache_dir, model_name: str = DEFAULT_MODEL, seed: int | None = None):
        """``<cache>/clip/<model_name>/{config.json, preprocessor_config.json, model.safetensors | pytorch_model.bin,
        vocab.json, merges.txt}``.  A missing directory is a ``FileNotFoundError`` unless ``seed`` asks for
        ``random_state`` of the base configuration (or of the directory's ``config.json`` when only the weights are
        missing).  Without ``vocab.json`` / ``merges.txt`` the model has no tokenizer: ``encode_text`` then raises,
        ``encode_ids`` works."""
        root = Path(cache_dir) / "clip" / model_name
        cfg_path = root / "config.json"
        if not cfg_path.exists():
            if seed is None:
                raise FileNotFoundError(f"{cfg_path} not found (no weights to embed frames with)")
            return cls(random_state({}, seed), {})
        config = json.loads(cfg_path.read_text())
        pc_path = root / "preprocessor_config.json"
        pc = json.loads(pc_path.read_text()) if pc_path.exists() else None
        tok = None
        if (root / "vocab.json").exists() and (root / "merges.txt").exists():
            tok = ClipTokenizer(root / "vocab.json", root / "merges.txt", clip_dims(config)["text"]["positions"])
        try:
            state = read_state(root)
        except FileNotFoundError:
            if seed is None:
                raise
            state = random_state(config, seed)
        return cls(state, config, pc, tok)

    # ---- images -------------------------------------------------------------------------------------------------------------
    def _tab(self, h: int, w: int):
        key = (h, w)
        if key not in self._tables:
            self._tables[key] = image_tables(h, w, self.pre["shortest_edge"], self.pre["crop"])
        return self._tables[key]

    @staticmethod
    def _frames(frames_bgr):
        if len(frames_bgr.shape) != 4 or int(frames_bgr.shape[3]) != 3:
            raise ValueError(f"expected (n, h, w, 3) BGR frames, got {tuple(frames_bgr.shape)}")
        if on_device(frames_bgr):
            import torch

            if frames_bgr.dtype != torch.uint8:
                raise ValueError("expected uint8 frames")
            return frames_bgr.contiguous()
        return np.ascontiguousarray(frames_bgr, dtype=np.uint8)

    @staticmethod
    def upload(frames_bgr: np.ndarray):
        """Host uint8 frames -> a CUDA tensor (the one copy ``embed_frames`` makes of a batch)."""
        import torch

        return torch.from_numpy(np.ascontiguousarray(frames_bgr, dtype=np.uint8)).cuda()

    def preprocess(self, frames_bgr):
        """-> ``(fp16 (n, 1 + P, Kp) patch rows, uint8 (n, S, S, 3) resized and cropped RGB)`` CUDA tensors."""
        import torch

        frames_bgr = self._frames(frames_bgr)
        n, h, w, _ = (int(s) for s in frames_bgr.shape)
        xb, xk, kx, yb, yk, ky = self._tab(h, w)
        dev = frames_bgr.device if on_device(frames_bgr) else torch.device("cuda", torch.cuda.current_device())
        x = torch.empty((n, self.tokens, self.row_len), dtype=torch.float16, device=dev)
        u8 = torch.empty((n, self.image, self.image, 3), dtype=torch.uint8, device=dev)
        _lib.check(self._h.eioku_clip_preprocess(ptr(frames_bgr), n, h, w, ptr(xb), ptr(xk), kx, ptr(yb), ptr(yk), ky, ptr(x), ptr(u8),
                                                 _lib.MEM_DEVICE if on_device(frames_bgr) else _lib.MEM_HOST, current_stream(x)),
                   "eioku_clip_preprocess")
        return x, u8

    def encode_patches(self, rows, with_hidden: bool = False):
        """fp16 (n, 1 + P, Kp) CUDA patch rows -> float32 (n, projection_dim) unit vectors (CUDA) [, float32 (n, 1 + P,
        hidden) residual stream before ``post_layernorm``]."""
        import torch

        n = int(rows.shape[0])
        if tuple(rows.shape[1:]) != (self.tokens, self.row_len) or rows.dtype != torch.float16:
            raise ValueError(f"expected fp16 (n, {self.tokens}, {self.row_len}) patch rows")
        out = torch.empty((n, self.projection_dim), dtype=torch.float32, device=rows.device)
        hidden = (torch.empty((n, self.tokens, self.dims["vision"]["hidden"]), dtype=torch.float32, device=rows.device)
                  if with_hidden else None)
        _lib.check(self._h.eioku_clip_encode_patches(ptr(rows.contiguous()), n, ptr(out), ptr(hidden), current_stream(rows)),
                   "eioku_clip_encode_patches")
        return (out, hidden) if with_hidden else out

    def encode_images(self, frames_bgr):
        """BGR uint8 ``(n, h, w, 3)`` -> float32 ``(n, projection_dim)`` unit vectors: a numpy array for numpy frames (staged),
        a CUDA tensor for CUDA frames (zero copy; it can go to ``IndexFlatL2.add`` as it is)."""
        frames_bgr = self._frames(frames_bgr)
        n, h, w, _ = (int(s) for s in frames_bgr.shape)
        xb, xk, kx, yb, yk, ky = self._tab(h, w)
        dev = on_device(frames_bgr)
        if dev:
            import torch

            out = torch.empty((n, self.projection_dim), dtype=torch.float32, device=frames_bgr.device)
        else:
            out = np.empty((n, self.projection_dim), np.float32)
        _lib.check(self._h.eioku_clip_encode_images(ptr(frames_bgr), n, h, w, ptr(xb), ptr(xk), kx, ptr(yb), ptr(yk), ky, ptr(out),
                                                    _lib.MEM_DEVICE if dev else _lib.MEM_HOST, current_stream(frames_bgr)),
                   "eioku_clip_encode_images")
        return out

    # ---- text ---------------------------------------------------------------------------------------------------------------
    def encode_ids(self, ids, with_hidden: bool = False):
        """int ``(n_texts, positions)`` ids -> float32 ``(n_texts, projection_dim)`` unit vectors (numpy) [, the residual
        stream before ``final_layer_norm``, ``(n_texts, n, hidden)``].  n positions are run: the largest ``eot + 1`` of the
        batch."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        if ids.ndim != 2 or ids.shape[1] != self.positions:
            raise ValueError(f"expected (n, {self.positions}) token ids, got {ids.shape}")
        eot = np.ascontiguousarray(eot_positions(ids, self.eos_token_id), dtype=np.int32)
        n = int(eot.max()) + 1 if len(ids) else 1
        out = np.empty((len(ids), self.projection_dim), np.float32)
        hidden = np.empty((len(ids), n, self.dims["text"]["hidden"]), np.float32) if with_hidden else None
        _lib.check(self._h.eioku_clip_encode_text(ptr(ids), ptr(eot), len(ids), n, ptr(out), ptr(hidden), _lib.MEM_HOST, None),
                   "eioku_clip_encode_text")
        return (out, hidden) if with_hidden else out

    def encode_text(self, texts: list[str]) -> np.ndarray:
        if self.tokenizer is None:
            raise ValueError("this ClipModel has no tokenizer (vocab.json and merges.txt were not found)")
        return self.encode_ids(self.tokenizer.encode(list(texts))[0])

    def last_flops(self) -> float:
        return self._h.doubles("last_flops")[0]

    def last_ms(self) -> dict:
        pre, enc, head = self._h.doubles("last_ms", 3)
        return {"preprocess": pre, "encoder": enc, "head": head}

    def close(self):
        self._h.close()


# ---- the index ----------------------------------------------------------------------------------------------------------------
def embedding_settings(config: dict) -> dict:
    """``model_name`` and ``frame_interval`` of a ``frame_embedding`` task; bad values are a ``ValueError``."""
    name = config.get("model_name", DEFAULT_MODEL)
    if not isinstance(name, str) or not name or "/" in name or name in (".", ".."):
        raise ValueError(f"frame_embedding: model_name must be a directory name, got {name!r}")
    seconds = config.get("frame_interval", 1.0)
    if isinstance(seconds, bool) or not isinstance(seconds, (int, float, np.integer, np.floating)) or not seconds >= 0:
        raise ValueError(f"frame_embedding: frame_interval must be a number >= 0, got {seconds!r}")
    return {"model_name": name, "frame_interval": seconds}


class VisualSearchEngine:
    """Frame vectors in a ``VectorStore(d=projection_dim)``; queries in words (``search``) or by a frame
    (``search_by_image``).  Results are ``{video_id, frame_index, timestamp_ms, relevance_score, thumbnail_path}`` with
    ``relevance_score = 1 - D / 2``, the cosine of two unit vectors at squared distance D."""

    def __init__(self, clip, store):
        self.clip, self.store = clip, store

    def index_frames(self, video_id: str, frames_meta: list[dict], embeddings) -> int:
        """``frames_meta``: ``{frame_index, timestamp_ms[, thumbnail_path, file_created_at, video_duration]}`` per row of
        ``embeddings``.  The video's earlier rows go first: a re-run replaces, it does not duplicate."""
        self.store.delete_by_video_id(video_id)
        meta = []
        for f in frames_meta:
            t = int(f["timestamp_ms"]) / 1000.0
            meta.append({"video_id": video_id, "start_time": t, "end_time": t, "frame_index": int(f["frame_index"]),
                         "timestamp_ms": int(f["timestamp_ms"]), "thumbnail_path": f.get("thumbnail_path")})
            for key in ("file_created_at", "video_duration"):
                if f.get(key) is not None:
                    meta[-1][key] = f[key]
        ids = [f"{video_id}_frame{m['frame_index']}" for m in meta]
        return self.store.index_segments(ids, np.asarray(embeddings, dtype=np.float32).reshape(len(ids), -1), meta)

    def _results(self, vector, filters, top_k) -> list[dict]:
        return [{"video_id": m["video_id"], "frame_index": m["frame_index"], "timestamp_ms": m["timestamp_ms"],
                 "relevance_score": 1.0 - dist / 2.0, "thumbnail_path": m.get("thumbnail_path")}
                for dist, m in self.store.search(vector, top_k, filters)]

    def search(self, query: str, filters: dict | None = None, top_k: int = 10) -> list[dict]:
        return self._results(self.clip.encode_text([query])[0], filters, top_k)

    def search_by_image(self, frame_bgr, filters: dict | None = None, top_k: int = 10) -> list[dict]:
        """``frame_bgr``: a BGR frame (host array or device tensor), or a baseline JPEG as ``bytes`` or as a ``str`` / ``Path``
        naming the file; the JPEG is decoded on the device (K28, ``eioku_amd.mjpeg``)."""
        if isinstance(frame_bgr, (str, bytes, bytearray)) or hasattr(frame_bgr, "__fspath__"):
            from pathlib import Path

            from .mjpeg import MjpegDecoder

            data = bytes(frame_bgr) if isinstance(frame_bgr, (bytes, bytearray)) else Path(frame_bgr).read_bytes()
            decoder = MjpegDecoder()
            try:
                frame_bgr = decoder.decode([data], "bgr")
            finally:
                decoder.close()
        vec =self.clip.encode_images(frame_bgr[None] if len(frame_bgr.shape) == 3 else frame_bgr)
        vec = vec.cpu().numpy() if on_device(vec) else vec
        return self._results(vec[0], filters, top_k)


def index_frame_embeddings(engine: VisualSearchEngine, video_id: str, rows: list[dict], config: dict | None = None) -> int:
    """The ``frame_embedding`` task's indexing half: the rows ``ModelManager.embed_frames`` returned into the engine's store;
    ``thumbnail_path`` of a row, and ``file_created_at`` / ``video_duration`` of a row or else of the job config, travel
    into the metadata."""
    meta = []
    for r in rows:
        meta.append({"frame_index": r["frame_index"], "timestamp_ms": r["timestamp_ms"], "thumbnail_path": r.get("thumbnail_path")})
        for key in ("file_created_at", "video_duration"):
            value = r.get(key, (config or {}).get(key))
            if value is not None:
                meta[-1][key] = value
    emb = np.asarray([r["embedding"] for r in rows], dtype=np.float32).reshape(len(rows), engine.store.d)
    return engine.index_frames(video_id, meta, emb)
