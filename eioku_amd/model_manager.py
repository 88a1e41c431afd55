"""Drop-in ``ModelManager`` for the ml-service worker: same methods, arguments, result dicts and
error behaviour as ``/root/reference/ml-service/src/services/model_manager.py`` for the three task
types on the hot path, with the arithmetic on the MI355X HIP library instead of
ffmpeg / OpenCV / Ultralytics on the CPU.

    detect_objects(video_path, config) -> {"detections": [{frame_index, timestamp_ms, label,
                                           confidence, bbox{x,y,width,height}}]}       (ref :215-306)
    detect_faces(video_path, config)   -> same + "cluster_id", label "face"            (ref :308-407)
                                          (None, or with config["cluster_faces"] the face's DBSCAN
                                          cluster of ArcFace embeddings: "face_cluster_001", ...)
    detect_scenes(video_path, config)  -> {"scenes": [{scene_index, start_ms, end_ms,
                                           duration_ms}]}                              (ref :715-835)
    extract_ocr(video_path, config)    -> {"detections": [{frame_index, timestamp_ms, text, confidence,
                                           language, polygon}], "language"}           (ref :469-558)
    generate_thumbnails(video_path, config) -> {"thumbnails": [{scene_index, start_ms, end_ms, timestamp_ms,
                                           frame_index, width, height, thumbnail_path, bytes}]}   (design only)
    detect_actions(video_path, config) -> {"actions": [{frame_index, timestamp_ms, start_ms, end_ms,
                                           labels[top_k], scores[top_k]}]}             (design only)
    embed_frames(video_path, config)   -> {"embeddings": [{frame_index, timestamp_ms,
                                           embedding[projection_dim]}]}                (design only)
    detect_sounds(video_path, config)  -> {"sounds": [{start_ms, end_ms, timestamp_ms, labels[<= top_k],
                                           scores[<= top_k]}]}                         (not in the reference)

What changes underneath (and nothing else): sampled frames are detected in batches instead of one
``model(frame)`` call each, and the scene score is computed by K1/K2 instead of an ffmpeg child
process.  Sampling rule, timestamps, label lookup, float widening and the scene-list quirks are the
reference's (pinned by ``tests/golden/ref_detect_loop.json`` / ``ref_scenes.json``).

There is no CPU fallback: without the HIP library / a gfx950 device the calls raise.
"""

from __future__ import annotations

import logging
from pathlib import Path

import numpy as np

logger = logging.getLogger(__name__)

OUT_OF_SCOPE = "is outside the MI355X hot path (SURVEY.md §8): delegate to the reference ModelManager"

# detection task -> (model_name, confidence_threshold, frame_interval seconds, face): the reference's defaults (:230-232,
# :324-326), read by detect_objects / detect_faces and analyze_video alike
_DETECT_DEFAULTS = {"object_detection": ("yolov8n.pt", 0.5, 1, False),
                    "face_detection": ("yolov8n-face.pt", 0.7, 3, True)}


def _detect_settings(task: str, config: dict):
    model_name, conf, seconds, face = _DETECT_DEFAULTS[task]
    return (config.get("model_name", model_name), config.get("confidence_threshold", conf),
            config.get("frame_interval", seconds), face)


def _frame_interval(fps, seconds) -> int:
    """The sampling rule of every frame loop (ref :243 / :337): every ``max(1, int(fps * seconds))``-th frame."""
    return max(1, int(fps * seconds))


def _timestamp_ms(frame_idx: int, fps) -> int:
    return int((frame_idx / fps) * 1000)


def _sampled_batches(cap, fps, interval: int, batch_size: int, device_decode: bool = False):
    """The reference's frame loop, batched: ``read()`` the sampled frames, ``grab()`` the others, stop at the first
    failure.  Yields ``(meta, frames)`` with ``meta`` the ``(frame_index, timestamp_ms)`` of each frame, a full batch
    before the next frame is read, then the rest.

    ``device_decode``: on a source that hands out its frames undecoded (``read_encoded`` / ``decode``: Motion-JPEG) the
    sampled frames are gathered as file bytes and ``frames`` is ONE device tensor ``(n, h, w, 3)`` from one decode call per
    batch; no pixel crosses PCIe.  Every other source yields the list of host frames as before."""
    encoded = device_decode and hasattr(cap, "read_encoded")
    read = cap.read_encoded if encoded else cap.read
    meta, frames = [], []
    frame_idx = 0
    while True:
        if frame_idx % interval == 0:
            ret, frame = read()
            if not ret:
                break
            frames.append(frame)
            meta.append((frame_idx, _timestamp_ms(frame_idx, fps)))
            if len(frames) >= batch_size:
                yield meta, (cap.decode(frames) if encoded else frames)
                meta, frames = [], []
        elif not cap.grab():
            break
        frame_idx += 1
    if frames:
        yield meta, (cap.decode(frames) if encoded else frames)


def _stack_rows(rows):
    """Device frame rows of the uploaded chunks -> one contiguous batch (a single row: a view, no copy)."""
    import torch

    return (torch.stack(rows) if len(rows) > 1 else rows[0][None]).contiguous()


def _stack_frames(items):
    """Frames or clips of one kind (host arrays, or device tensors) -> one batch along a new first axis."""
    if isinstance(items[0], np.ndarray):
        return np.stack(items)
    import torch

    return torch.stack(list(items))


class _DetectionLane:
    """One detection task's output, shared by ``detect_objects`` / ``detect_faces`` and ``analyze_video``: batches go in
    through ``submit``, detection dicts (the reference's float widening, the face path's confidence filter,
    ``cluster_id``) come out in ``out``.  With a ``PipelinedDetector`` two batches are in flight and results are taken in
    submission order, so the list is the one the synchronous ``detector.detect`` path produces."""

    def __init__(self, detector, face: bool, conf: float, pipe=None, cluster=None, alignment="auto"):
        """``alignment`` (the ``face_alignment`` config key): ``"auto"`` embeds aligned crops when the detector has exactly
        five keypoints, ``False`` keeps the box crops, ``True`` insists (``ValueError`` without five keypoints)."""
        self.detector, self.pipe = detector, pipe
        self.face, self.conf, self.names = face, conf, detector.names
        self.cluster = cluster  # FaceClusterer or None
        nk = int(getattr(detector, "nk", 0) or 0)
        self.kpts = face and nk > 0  # a Pose checkpoint: every face carries "landmarks"
        if alignment not in ("auto", True, False):
            raise ValueError(f"face_alignment must be \"auto\", True or False, not {alignment!r}")
        if alignment is True and not (face and nk == 15):
            raise ValueError(f"face_alignment needs a face detector with 5 keypoints; this one has {nk // 3}")
        self.align = self.kpts and nk == 15 and alignment is not False
        self.metas: list[list[tuple[int, int]]] = []  # the batches in flight, oldest first
        self.out: list[dict] = []

    def submit(self, meta, frames) -> None:
        """``frames``: the stacked batch (host ndarray or device tensor), ``meta``: its ``(frame_index, timestamp_ms)``."""
        if self.pipe is None:
            if self.kpts:
                dets, counts, kpts = self.detector.detect(frames, conf=self.conf, with_kpts=True)
                self._emit(meta, dets, counts, frames, kpts)
            else:
                self._emit(meta, *self.detector.detect(frames, conf=self.conf), frames)
            return
        if self.kpts:
            self.pipe.submit(frames, conf=self.conf, with_kpts=True)
        else:
            self.pipe.submit(frames, conf=self.conf)
        self.metas.append(meta)
        self._drain(self.pipe.depth - 1)

    def finish(self) -> list[dict]:
        """Drain every batch in flight, cluster the faces; the detection list."""
        if self.pipe is not None:
            self._drain(0)
        if self.cluster is not None:
            self.cluster.finish()
        return self.out

    def close(self) -> None:
        close = self.pipe.close if self.pipe is not None else getattr(self.detector, "close", None)
        if close:
            close()
        close = getattr(self.cluster.embedder, "close", None) if self.cluster is not None else None
        if close:
            close()

    def _drain(self, keep: int) -> None:
        while self.pipe.in_flight() > keep:  # the clusterer crops the faces from the batch's device copy
            if self.kpts:
                result = self.pipe.result_with_frames_and_kpts()
            else:
                result = self.pipe.result_with_frames() if self.cluster is not None else self.pipe.result()
            self._emit(self.metas.pop(0), *result)

    def _emit(self, meta, dets, counts, frames=None, kpts=None) -> None:
        boxes, batch, marks = [], [], []
        for slot, ((frame_idx, timestamp_ms), row, cnt) in enumerate(zip(meta, dets, counts)):
            for i, d in enumerate(row[: int(cnt)]):
                x1, y1, x2, y2 = (np.float32(d[k]) for k in ("x1", "y1", "x2", "y2"))
                confidence = float(np.float32(d["conf"]))  # float32 -> Python float, as float(tensor)
                if self.face and confidence < self.conf:
                    continue  # the face path's extra safety filter (ref :375-377)
                det = {"frame_index": frame_idx, "timestamp_ms": timestamp_ms,
                       "label": "face" if self.face else self.names[int(d["cls"])], "confidence": confidence,
                       "bbox": {"x": float(x1), "y": float(y1),
                                "width": float(np.float32(x2 - x1)), "height": float(np.float32(y2 - y1))}}
                if self.face:
                    det["cluster_id"] = None
                    if kpts is not None:  # original-image pixels, in the checkpoint's keypoint order
                        det["landmarks"] = [{"x": float(x), "y": float(y), "confidence": float(c)} for x, y, c in kpts[slot][i]]
                    if self.cluster is not None:
                        boxes.append((slot, x1, y1, x2, y2))
                        batch.append(det)
                        if self.align:
                            marks.append(np.asarray(kpts[slot][i], np.float64)[:, :2])
                self.out.append(det)
        if self.cluster is not None:
            if self.align:
                self.cluster.add(frames, boxes, batch, landmarks=np.asarray(marks, np.float64).reshape(-1, 5, 2))
            else:
                self.cluster.add(frames, boxes, batch)


class ModelManager:
    """Manages model lifecycle and inference for the hot-path task types."""

    def __init__(self, cache_dir: str = "/models", *, frame_source=None, detector_factory=None, batch_size: int = 64,
                 random_init_seed: int | None = None, place_classifier_factory=None, face_embedder_factory=None,
                 ocr_reader_factory=None, gpu_transcription: bool = False, audio_source=None, transcriber_factory=None,
                 gpu_vad: bool = False, vad_factory=None, gpu_audio: bool = False, audio_frontend_factory=None,
                 gpu_speakers: bool = False, speaker_factory=None, action_recognizer_factory=None, clip_factory=None,
                 sound_tagger_factory=None):
        """``cache_dir`` as in the reference (:12-21).  Keyword-only extras are seams for tests and bench:
        ``frame_source(path) -> FrameSource``, ``detector_factory(model_name, cache_dir) -> detector`` with
        ``detect(frames, conf=...) -> (dets, counts)`` and ``names``; ``random_init_seed`` builds random
        weights of the right shapes when no checkpoint can exist (offline benchmarks);
        ``face_embedder_factory(cache_dir, model_name) -> embedder`` with ``embed(frames, boxes)`` and
        ``cluster(embeddings, eps, min_samples)`` (``cluster_faces``); ``ocr_reader_factory(cache_dir) -> reader`` with
        ``readtext_batch(frames) -> per frame [(box, text, confidence)]``.  ``gpu_transcription=True`` enables
        ``transcribe_video`` on the HIP path (Whisper, ``eioku_amd.transcribe``); ``audio_source(path) -> (float32 mono
        samples, sample_rate)`` and ``transcriber_factory(cache_dir, model_name) -> object with transcribe(samples, language,
        window_mode=, batch_windows=)`` are its seams (``beam_size=`` / ``patience=`` follow only when the task's config sets
        them).  ``gpu_vad=True`` runs Silero VAD (``eioku_amd.vad``) in front of the transcription when the task's
        ``vad_filter`` is on (the reference's default); ``vad_factory(cache_dir) -> object with speech_probs(samples)`` is
        its seam.  ``gpu_audio=True`` (with ``gpu_transcription``) reads PCM WAV of any sample rate, width and channel count
        and resamples it to 16 kHz on the device (``eioku_amd.audio``); ``audio_frontend_factory() -> object with load(path)
        and resample_float(samples, rate)`` is its seam.  Without it audio that is not 16 kHz raises, as before.
        ``gpu_speakers=True`` (with ``gpu_transcription``) labels the segments' speakers (``eioku_amd.speakers``) when the
        task's ``speaker_labels`` is true; ``speaker_factory(cache_dir, model_name) -> object with label(samples, segments,
        eps=, min_samples=, assign_max=)`` is its seam (``speaker_model`` in the task's config names the checkpoint).
        ``clip_factory(cache_dir, model_name) -> object with encode_images(frames)`` and optionally ``upload(frames)`` and
        ``close()`` is the seam of ``embed_frames``; ``sound_tagger_factory(cache_dir, model_name) -> object with
        classify(samples, plan, top_k, batch_windows=)``, ``labels``, ``max_length`` and ``window_samples`` that of
        ``detect_sounds``."""
        self.cache_dir = Path(cache_dir)
        self.cache_dir.mkdir(parents=True, exist_ok=True)
        self.models = {}
        self._gpu_available = None  # Lazy initialization
        self._frame_source = frame_source
        self._detector_factory = detector_factory
        self._place_classifier_factory = place_classifier_factory  # (cache_dir) -> object with classify(frames, top_k), labels
        self._face_embedder_factory = face_embedder_factory
        self._ocr_reader_factory = ocr_reader_factory
        self._gpu_transcription = bool(gpu_transcription)
        self._audio_source = audio_source
        self._transcriber_factory = transcriber_factory
        self._gpu_vad = bool(gpu_vad)
        self._vad_factory = vad_factory
        self._gpu_audio = bool(gpu_audio)
        self._audio_frontend_factory = audio_frontend_factory
        self._gpu_speakers = bool(gpu_speakers)
        self._speaker_factory = speaker_factory
        # (cache_dir, model_name) -> object with classify(clips, top_k), labels, frames and optionally upload(frames)
        self._action_recognizer_factory = action_recognizer_factory
        self._clip_factory = clip_factory
        self._sound_tagger_factory = sound_tagger_factory
        self._batch_size = int(batch_size)
        self._lane_streams = {}  # task -> the two HIP streams its detector lanes run on (created once per manager)
        self._seed = random_init_seed

    # ---- GPU probe: identical surface to the reference (:23-42, 168-213) -------------------------
    @property
    def gpu_available(self) -> bool:
        if self._gpu_available is None:
            try:
                import torch

                self._gpu_available = torch.cuda.is_available()
            except Exception as e:  # noqa: BLE001 - same tolerance as the reference
                logger.warning(f"Could not check GPU availability: {e}")
                self._gpu_available = False
        return self._gpu_available

    def _get_device(self) -> str:
        return "cuda" if self.gpu_available else "cpu"  # ROCm torch reports through torch.cuda

    def get_gpu_info(self) -> dict:
        if not self.gpu_available:
            return {"gpu_available": False, "gpu_device_name": None, "gpu_memory_total_mb": None,
                    "gpu_memory_used_mb": None}
        import torch

        return {"gpu_available": True, "gpu_device_name": torch.cuda.get_device_name(0),
                "gpu_memory_total_mb": int(torch.cuda.get_device_properties(0).total_memory / 1e6),
                "gpu_memory_used_mb": int(torch.cuda.memory_allocated(0) / 1e6)}

    def detect_gpu(self) -> bool:
        return self.gpu_available

    def log_gpu_info(self):
        if self.gpu_available:
            info = self.get_gpu_info()
            logger.info(f"GPU device: {info['gpu_device_name']}")
            logger.info(f"GPU memory: {info['gpu_memory_total_mb'] / 1e3:.2f} GB")
        else:
            logger.warning("GPU not available - the HIP hot path cannot run")

    # ---- out-of-scope members: fail loudly, never silently diverge ----------------------------------
    async def download_model(self, model_name: str, model_type: str):
        raise NotImplementedError(f"download_model {OUT_OF_SCOPE} (needs network)")

    async def verify_model(self, model_name: str, model_type: str) -> bool:
        raise NotImplementedError(f"verify_model {OUT_OF_SCOPE}")

    async def transcribe_video(self, video_path: str, config: dict) -> dict:
        """Whisper on the HIP path when the manager was built with ``gpu_transcription=True`` (reference: :406-467, which
        calls faster-whisper on the CPU); otherwise refused as before.  Result: ``{"segments": [{start_ms, end_ms, text,
        language, confidence: None, words: None}]}``.  Greedy decoding by default; config ``beam_size`` (1..8; 5 is the
        reference's call) and ``patience`` switch to beam search, ``temperature`` (a list) with ``best_of`` and the two
        thresholds adds the temperature fallback, ``condition_on_previous_text`` the previous-text prompts
        (``transcribe.REFERENCE_CALL`` is the reference's call); values outside their ranges raise ``ValueError``.  A manager
        built with ``gpu_vad=True`` applies ``vad_filter`` (default on) and ``vad_parameters`` through Silero VAD first; one
        built with ``gpu_audio=True`` takes PCM WAV of any rate, width and channel count and resamples it on the device; one
        built with ``gpu_speakers=True`` adds a ``speaker`` key to every segment when ``speaker_labels`` is true.  The
        deviations from the reference's call are listed in INTEGRATION.md §3."""
        if not self._gpu_transcription:
            raise NotImplementedError(f"transcribe_video {OUT_OF_SCOPE}")
        try:
            from .transcribe import WhisperTranscriber, transcribe_video

            config = config or {}
            model_name = config.get("model_name", "base")
            logger.info(f"Transcription: {video_path} with whisper {model_name} (GPU: {self.gpu_available})")
            if self._transcriber_factory is not None:
                transcriber = self._transcriber_factory(self.cache_dir, model_name)
            else:
                transcriber = WhisperTranscriber.from_cache(self.cache_dir, model_name, seed=self._seed)
            vad = frontend = speakers = None
            try:
                extra = {}
                if self._gpu_audio:
                    if self._audio_frontend_factory is not None:
                        frontend = self._audio_frontend_factory()
                    else:
                        from .audio import AudioFrontEnd

                        frontend = AudioFrontEnd()
                    extra["audio_frontend"] = frontend
                if self._gpu_vad and config.get("vad_filter", True):
                    if self._vad_factory is not None:
                        vad = self._vad_factory(self.cache_dir)
                    else:
                        from .vad import SileroVad

                        vad = SileroVad.from_cache(self.cache_dir, seed=self._seed)
                if self._gpu_speakers and config.get("speaker_labels") is True:
                    speaker_model = config.get("speaker_model", "voxceleb_resnet34_LM")
                    if self._speaker_factory is not None:
                        speakers = self._speaker_factory(self.cache_dir, speaker_model)
                    else:
                        from .speakers import SpeakerLabeller

                        speakers = SpeakerLabeller.from_cache(self.cache_dir, speaker_model, seed=self._seed)
                    extra["speakers"] = speakers
                result = transcribe_video(video_path, config, transcriber=transcriber, audio_source=self._audio_source, vad=vad,
                                          **extra)
            finally:
                for model in (frontend, vad, speakers, transcriber):
                    close = getattr(model, "close", None)
                    if close:
                        close()
            logger.info(f"✅ Transcription complete: {len(result['segments'])} segments")
            return result
        except Exception as e:
            logger.error(f"Transcription failed: {e}", exc_info=True)
            raise

    async def extract_ocr(self, video_path: str, config: dict) -> dict:
        """On-screen text with EasyOCR's CRAFT + english_g2 on the HIP path (reference: :469-558): every
        ``max(1, int(fps * frame_interval))``-th frame -> ``readtext`` detections ``{frame_index, timestamp_ms, text,
        confidence, language, polygon: [{x, y}]}``.  English only: another language raises ``ValueError``."""
        try:
            logger.info(f"OCR: {video_path} (GPU: {self.gpu_available})")
            # 'language' (singular) first, then the legacy 'languages' list (ref :489-499)
            language = config.get("language")
            if language:
                languages = [language]
            else:
                languages = config.get("languages", ["en"])
                if isinstance(languages, str):
                    languages = [languages]
                language = languages[0] if languages else "en"
            from .ocr import SUPPORTED_LANGUAGES

            unsupported = [lang for lang in languages if lang not in SUPPORTED_LANGUAGES]
            if unsupported:
                raise ValueError(f"OCR languages {unsupported} are not supported (supported: {list(SUPPORTED_LANGUAGES)})")
            frame_interval_seconds = config.get("frame_interval", 2)
            reader = self._load_ocr_reader()
            cap = self._open(video_path)
            fps = cap.fps or 30
            total_frames = int(cap.total_frames)
            frame_interval = _frame_interval(fps, frame_interval_seconds)
            frames_to_process = (total_frames + frame_interval - 1) // frame_interval
            logger.info(f"Video FPS: {fps}, Total frames: {total_frames}, Processing every {frame_interval} frames "
                        f"(every {frame_interval_seconds}s, ~{frames_to_process} frames to process)")
            detections: list[dict] = []
            try:
                for meta, frames in _sampled_batches(cap, fps, frame_interval, self._batch_size):
                    for (frame_idx, timestamp_ms), results in zip(meta, reader.readtext_batch(np.stack(frames))):
                        for bbox, text, confidence in results:
                            detections.append({"frame_index": frame_idx, "timestamp_ms": timestamp_ms, "text": text,
                                               "confidence": confidence, "language": language,
                                               "polygon": [{"x": float(p[0]), "y": float(p[1])} for p in bbox]})
            finally:
                cap.release()
                close = getattr(reader, "close", None)
                if close:
                    close()
            logger.info(f"✅ OCR complete: {len(detections)} detections")
            return {"detections": detections, "language": language}
        except Exception as e:
            logger.error(f"OCR failed: {e}", exc_info=True)
            raise

    def _load_ocr_reader(self):
        """``easyocr.Reader(languages)`` (ref :507) from ``<cache>/easyocr/model``, per job like the reference."""
        if self._ocr_reader_factory is not None:
            return self._ocr_reader_factory(self.cache_dir)
        from .ocr import OcrReader

        return OcrReader.from_cache(self.cache_dir, seed=self._seed)

    async def extract_metadata(self, video_path: str, config: dict) -> dict:
        raise NotImplementedError(f"extract_metadata {OUT_OF_SCOPE}")

    # ---- seams ----------------------------------------------------------------------------------------
    def _open(self, video_path: str):
        if self._frame_source is not None:
            return self._frame_source(video_path)
        from .frames import open_video

        return open_video(video_path)

    def _load_detector(self, model_name: str, keypoints: int = 0):
        """``YOLO(cache_dir/ultralytics/model_name); model.to(device)`` (ref :252-254): per job, like the reference.
        ``keypoints`` (the face task's config key of that name) shapes seeded weights only: a checkpoint has its own head."""
        if self._detector_factory is not None:
            return self._detector_factory(model_name, self.cache_dir)
        from .detect import Yolov8Detector

        path = self.cache_dir / "ultralytics" / model_name
        if self._seed is not None and not path.exists():
            return Yolov8Detector.from_model_name(model_name, seed=self._seed, keypoints=keypoints)
        return Yolov8Detector.from_model_name(model_name, path=path)

    def _lanes(self, task: str, depth: int = 2):
        """The detector lanes' streams of a task, created on first use and kept: the model is loaded per job like the
        reference's, the streams are not - a HIP stream's hardware queue is fixed when it is created, and a worker that
        made new ones for every job would see its lanes land on whichever queues the earlier jobs left (measured in
        bench.py: the same pipeline at 41 k instead of 58 k frames/s behind three earlier runs)."""
        import torch

        if task not in self._lane_streams:
            self._lane_streams[task] = [torch.cuda.Stream(priority=-1) for _ in range(depth)]
        return self._lane_streams[task]

    # ---- face clustering (opt-in: config["cluster_faces"]) ---------------------------------------------
    CLUSTER_EPS = 0.5         # cosine distance (1 - similarity) of two unit ArcFace embeddings; INTEGRATION.md
    CLUSTER_MIN_SAMPLES = 3   # faces (the point itself included) that make a core point
    CLUSTER_MIN_SIZE = 5      # face_cluster_method "hdbscan": the fewest faces that make a person

    def _face_clusterer(self, config: dict):
        """The per-video ``FaceClusterer`` of a face-detection config, or None without ``cluster_faces`` (then no
        embedder is loaded and every ``cluster_id`` stays None, as in the reference)."""
        if not config.get("cluster_faces", False):
            return None
        from .faces import CLUSTER_METHODS, FaceClusterer

        method = config.get("face_cluster_method", "dbscan")
        if method not in CLUSTER_METHODS:
            raise ValueError(f"face_cluster_method must be one of {CLUSTER_METHODS}, got {method!r}")
        model_name = config.get("face_embedding_model", "arcface_r18.pth")
        if self._face_embedder_factory is not None:
            embedder = self._face_embedder_factory(self.cache_dir, model_name)
        else:
            from .faces import FaceEmbedder

            embedder = FaceEmbedder.from_cache(self.cache_dir, model_name, seed=self._seed)
        min_samples = config.get("cluster_min_samples", self.CLUSTER_MIN_SAMPLES)
        if method == "hdbscan":  # no density threshold: cluster_eps, only if given, is its cluster_selection_epsilon
            return FaceClusterer(embedder, config.get("cluster_eps"), min_samples, method,
                                 config.get("cluster_min_size", self.CLUSTER_MIN_SIZE))
        return FaceClusterer(embedder, config.get("cluster_eps", self.CLUSTER_EPS), min_samples)

    # ---- objects / faces: one skeleton, as in the reference --------------------------------------------
    def _detect_loop(self, task: str, video_path: str, config: dict) -> dict:
        what = "Face detection" if task == "face_detection" else "Object detection"
        try:
            model_name, confidence_threshold, frame_interval_seconds, face = _detect_settings(task, config)
            logger.info(f"{what}: {video_path} (device: {self._get_device()})")
            cluster = self._face_clusterer(config) if face else None
            cap = self._open(video_path)
            fps = cap.fps or 30
            total_frames = int(cap.total_frames)
            logger.info(f"Video FPS: {fps}, Total frames: {total_frames}")
            frame_interval = _frame_interval(fps, frame_interval_seconds)
            frames_to_process = (total_frames + frame_interval - 1) // frame_interval
            logger.info(f"Processing every {frame_interval} frames (every {frame_interval_seconds}s at {fps} FPS, "
                        f"~{frames_to_process} frames to process)")
            detector = self._load_detector(model_name, int(config.get("keypoints", 0)) if face else 0)

            # Two batches in flight on the HIP path (PipelinedDetector: second handle + stream); test stubs run synchronously
            from .detect import PipelinedDetector, Yolov8Detector

            pipe = (PipelinedDetector(detector, depth=2, streams=self._lanes(task))
                    if isinstance(detector, Yolov8Detector) else None)
            lane = _DetectionLane(detector, face, confidence_threshold, pipe, cluster, config.get("face_alignment", "auto"))
            try:
                for meta, frames in _sampled_batches(cap, fps, frame_interval, self._batch_size, device_decode=True):
                    lane.submit(meta, np.stack(frames) if isinstance(frames, list) else frames)
                detections = lane.finish()
            finally:
                cap.release()
                lane.close()
            logger.info(f"✅ {what} complete: {len(detections)} detections")
            return {"detections": detections}
        except Exception as e:
            logger.error(f"{what} failed: {e}", exc_info=True)
            raise

    # ---- places: Places365 ResNet18 (reference :560-713) ---------------------------------------------------
    def _load_place_classifier(self):
        """``models.resnet18`` + 365-way fc + ``<cache>/places365/resnet18_places365.pth.tar`` and the label file
        (ref :579-624), per job like the reference."""
        if self._place_classifier_factory is not None:
            return self._place_classifier_factory(self.cache_dir)
        from .places import Places365Classifier

        return Places365Classifier.from_cache(self.cache_dir, seed=self._seed)

    async def classify_places(self, video_path: str, config: dict) -> dict:
        """Classify places in video frames using Places365 on the HIP path (reference: :560-713): every
        ``max(1, int(fps * frame_interval))``-th frame -> softmax top_k ``{"label", "confidence"}`` lists."""
        try:
            logger.info(f"Place detection: {video_path} (device: {self._get_device()})")
            classifier = self._load_place_classifier()
            classes = classifier.labels
            cap = self._open(video_path)
            fps = cap.fps or 30
            total_frames = int(cap.total_frames)
            frame_interval_seconds = config.get("frame_interval", 1)
            top_k = config.get("top_k", 5)
            frame_interval = _frame_interval(fps, frame_interval_seconds)
            frames_to_process = (total_frames + frame_interval - 1) // frame_interval
            logger.info(f"Video FPS: {fps}, Total frames: {total_frames}, Processing every {frame_interval} frames "
                        f"(every {frame_interval_seconds}s, ~{frames_to_process} frames to process)")
            classifications: list[dict] = []
            try:
                for meta, frames in _sampled_batches(cap, fps, frame_interval, self._batch_size):
                    probs, idx = classifier.classify(np.stack(frames), top_k)
                    for (frame_idx, timestamp_ms), p, i in zip(meta, probs, idx):
                        # `for j, i in enumerate(idx[:top_k])`: float(probs[j]) widens the float32 (ref :677-683)
                        classifications.append({"frame_index": frame_idx, "timestamp_ms": timestamp_ms,
                                                "predictions": [{"label": classes[int(c)], "confidence": float(np.float32(v))}
                                                                for v, c in zip(p, i)]})
            finally:
                cap.release()
                close = getattr(classifier, "close", None)
                if close:
                    close()
            logger.info(f"✅ Place detection complete: {len(classifications)} classifications")
            return {"classifications": classifications}
        except Exception as e:
            logger.error(f"Place detection failed: {e}", exc_info=True)
            raise

    # ---- actions: TimeSformer on windows of the sampled frames (design.md §1.8; the reference never builds it) ----
    def _load_action_recognizer(self, model_name: str):
        """``<cache>/timesformer/<model_name>/`` (``eioku_amd.actions``), per job like the other stages."""
        if self._action_recognizer_factory is not None:
            return self._action_recognizer_factory(self.cache_dir, model_name)
        from .actions import ActionRecognizer

        return ActionRecognizer.from_cache(self.cache_dir, model_name, seed=self._seed)

    async def detect_actions(self, video_path: str, config: dict) -> dict:
        """Recognise actions on the HIP path: every ``max(1, int(fps * frame_interval))``-th frame is sampled, clip c is
        sampled frames ``[c * clip_stride, c * clip_stride + T)`` (T from the checkpoint, ``clip_stride`` defaults to T), a
        trailing partial window is dropped, and a video with no full window is one clip padded with its last frame.
        -> ``{"actions": [{frame_index, timestamp_ms, start_ms, end_ms, labels, scores}]}``: the clip's first sampled
        frame, the span up to its last real sampled frame, and the ``top_k`` labels in descending probability."""
        from .actions import action_settings

        try:
            logger.info(f"Action detection: {video_path} (device: {self._get_device()})")
            recognizer = self._load_action_recognizer(action_settings(config)["model_name"])
            actions: list[dict] = []
            try:
                T, names = int(recognizer.frames), recognizer.labels
                settings = action_settings(config, T, len(names))
                stride, top_k = settings["clip_stride"], settings["top_k"]
                cap = self._open(video_path)
                try:
                    fps = cap.fps or 30
                    interval = _frame_interval(fps, settings["frame_interval"])
                    upload = getattr(recognizer, "upload", None)
                    held, first, seen, start = [], 0, 0, 0  # held[i]: (meta, batch, row) of sampled frame first + i

                    def run(windows):
                        """``[(first, last real)]`` windows over the held frames -> their action dicts"""
                        if not windows:
                            return
                        clips = []
                        for a, b in windows:
                            rows = [held[min(i, b) - first] for i in range(a, a + T)]  # past the last real frame: repeat it
                            batch, lo = rows[0][1], rows[0][2]
                            if all(r[1] is batch and r[2] == lo + j for j, r in enumerate(rows)):
                                clips.append(batch[lo:lo + T])  # one batch, consecutive rows: a view
                            else:
                                clips.append(_stack_frames([r[1][r[2]] for r in rows]))
                        probs, ids = recognizer.classify(_stack_frames(clips), top_k)
                        for (a, b), p, i in zip(windows, probs, ids):
                            (frame_idx, ts), (_, end_ts) = held[a - first][0], held[b - first][0]
                            actions.append({"frame_index": frame_idx, "timestamp_ms": ts, "start_ms": ts, "end_ms": end_ts,
                                            "labels": [names[int(c)] for c in i], "scores": [float(np.float32(v)) for v in p]})

                    for meta, frames in _sampled_batches(cap, fps, interval, self._batch_size):
                        batch = np.stack(frames)
                        batch = upload(batch) if upload else batch  # the one upload of these frames
                        held.extend((m, batch, j) for j, m in enumerate(meta))
                        seen += len(meta)
                        windows = []
                        while start + T <= seen:
                            windows.append((start, start + T - 1))
                            start += stride
                        run(windows)
                        drop = min(start, seen) - first  # frames no later window reads
                        if drop > 0:
                            del held[:drop]
                            first += drop
                    if 0 < seen < T:  # no full window at all: one clip, padded with the last frame
                        run([(0, seen - 1)])
                finally:
                    cap.release()
            finally:
                close = getattr(recognizer, "close", None)
                if close:
                    close()
            logger.info(f"✅ Action detection complete: {len(actions)} clips")
            return {"actions": actions}
        except Exception as e:
            logger.error(f"Action detection failed: {e}", exc_info=True)
            raise

    # ---- sounds: the Audio Spectrogram Transformer on windows of the audio track (eioku_amd.sounds) ----
    def _load_sound_tagger(self, model_name: str):
        """``<cache>/ast/<model_name>/`` (``eioku_amd.sounds``), per job like the other stages."""
        if self._sound_tagger_factory is not None:
            return self._sound_tagger_factory(self.cache_dir, model_name)
        from .sounds import SoundTagger

        return SoundTagger.from_cache(self.cache_dir, model_name, seed=self._seed)

    async def detect_sounds(self, video_path: str, config: dict) -> dict:
        """Tag non-speech sounds (music, applause, barking, ...) on the HIP path: windows of the checkpoint's length (10.24 s)
        every ``window_stride`` seconds (default 10.0) over the 16 kHz audio, which is found as ``transcribe_video`` finds it
        (the manager's ``audio_source``, else the path or its sibling ``.wav``; with ``gpu_audio=True`` any PCM WAV, resampled
        on the device; otherwise another rate raises ``ValueError``).  -> ``{"sounds": [{start_ms, end_ms, timestamp_ms,
        labels, scores}]}``, one item per window: the ``top_k`` (default 5) labels in descending score, the sigmoid scores,
        entries below ``min_score`` dropped.  A file shorter than one frame (400 samples) has no windows."""
        from .sounds import SAMPLE_RATE, plan_windows, sound_settings
        from .transcribe import check_rate, default_audio_source

        try:
            config = config or {}
            logger.info(f"Sound detection: {video_path} (device: {self._get_device()})")
            tagger = self._load_sound_tagger(sound_settings(config)["model_name"])
            frontend = None
            sounds: list[dict] = []
            try:
                names = tagger.labels
                settings = sound_settings(config, len(names))
                if self._gpu_audio:
                    if self._audio_frontend_factory is not None:
                        frontend = self._audio_frontend_factory()
                    else:
                        from .audio import AudioFrontEnd

                        frontend = AudioFrontEnd()
                if frontend is not None and self._audio_source is None:
                    samples, rate = frontend.load(video_path)
                else:
                    samples, rate = (self._audio_source or default_audio_source)(video_path)
                    if frontend is not None and int(rate) != SAMPLE_RATE:
                        samples, rate = frontend.resample_float(samples, rate), SAMPLE_RATE
                check_rate(rate)
                samples = np.asarray(samples, dtype=np.float32).reshape(-1)
                n = int(samples.shape[0])
                span = int(tagger.window_samples)
                stride = max(1, int(round(settings["window_stride"] * SAMPLE_RATE)))
                plan = plan_windows(n, int(tagger.max_length), stride)
                if plan:
                    scores, ids = tagger.classify(samples, plan, settings["top_k"], batch_windows=settings["batch_windows"])[:2]
                    for (first, _), sc, idx in zip(plan, scores, ids):
                        start_ms = first * 1000 // SAMPLE_RATE
                        keep = [(names[int(c)], float(np.float32(v))) for c, v in zip(idx, sc) if float(v) >= settings["min_score"]]
                        sounds.append({"start_ms": start_ms, "end_ms": min(n, first + span) * 1000 // SAMPLE_RATE,
                                       "timestamp_ms": start_ms, "labels": [str(k) for k, _ in keep],
                                       "scores": [v for _, v in keep]})
            finally:
                for model in (frontend, tagger):
                    close = getattr(model, "close", None)
                    if close:
                        close()
            logger.info(f"✅ Sound detection complete: {len(sounds)} windows")
            return {"sounds": sounds}
        except Exception as e:
            logger.error(f"Sound detection failed: {e}", exc_info=True)
            raise

    # ---- frame embeddings: CLIP's image tower on the sampled frames (eioku_amd.visual) ----
    def _load_clip(self, model_name: str):
        """``<cache>/clip/<model_name>/`` (``eioku_amd.visual``), per job like the other stages."""
        if self._clip_factory is not None:
            return self._clip_factory(self.cache_dir, model_name)
        from .visual import ClipModel

        return ClipModel.from_cache(self.cache_dir, model_name, seed=self._seed)

    async def embed_frames(self, video_path: str, config: dict) -> dict:
        """Embed frames on the HIP path: every ``max(1, int(fps * frame_interval))``-th frame (``frame_interval`` defaults
        to 1.0 s) goes through CLIP's image tower (``model_name`` defaults to ``clip-vit-base-patch32``), each batch uploaded
        once -> ``{"embeddings": [{frame_index, timestamp_ms, embedding: [float] * projection_dim}]}``, unit vectors."""
        from .visual import embedding_settings

        try:
            logger.info(f"Frame embedding: {video_path} (device: {self._get_device()})")
            settings = embedding_settings(config)
            clip = self._load_clip(settings["model_name"])
            embeddings: list[dict] = []
            try:
                cap = self._open(video_path)
                try:
                    fps = cap.fps or 30
                    interval = _frame_interval(fps, settings["frame_interval"])
                    upload = getattr(clip, "upload", None)
                    for meta, frames in _sampled_batches(cap, fps, interval, self._batch_size):
                        batch = np.stack(frames)
                        vectors = clip.encode_images(upload(batch) if upload else batch)  # the one upload of these frames
                        vectors = vectors if isinstance(vectors, np.ndarray) else vectors.cpu().numpy()
                        for (frame_idx, timestamp_ms), v in zip(meta, vectors):
                            embeddings.append({"frame_index": frame_idx, "timestamp_ms": timestamp_ms,
                                               "embedding": [float(x) for x in v]})
                finally:
                    cap.release()
            finally:
                close = getattr(clip, "close", None)
                if close:
                    close()
            logger.info(f"✅ Frame embedding complete: {len(embeddings)} frames")
            return {"embeddings": embeddings}
        except Exception as e:
            logger.error(f"Frame embedding failed: {e}", exc_info=True)
            raise

    async def detect_objects(self, video_path: str, config: dict) -> dict:
        """Detect objects in video using YOLOv8 on the HIP path (reference: :215-306)."""
        return self._detect_loop("object_detection", video_path, config)

    async def detect_faces(self, video_path: str, config: dict) -> dict:
        """Detect faces in video using YOLOv8-face on the HIP path (reference: :308-407).  With
        ``config["cluster_faces"]`` every face that passes the confidence filter is embedded (ArcFace IResNet,
        ``face_embedding_model`` under ``<cache>/insightface/``) and the video's faces are clustered once by cosine DBSCAN
        (``cluster_eps``, ``cluster_min_samples``): ``cluster_id`` = ``face_cluster_001``, ... or None for noise.
        ``face_cluster_method="hdbscan"`` clusters by HDBSCAN instead (``cluster_min_size``, ``cluster_min_samples``; no
        ``eps``) and adds ``cluster_probability`` to every clustered face's record (0.0 for noise).
        A Pose checkpoint (the community ``yolov8n-face.pt``: five landmarks) adds ``"landmarks": [{"x", "y", "confidence"}]``
        to every face, and the embeddings then come from crops aligned on them unless ``face_alignment`` is False
        (INTEGRATION.md section 3)."""
        return self._detect_loop("face_detection", video_path, config)

    # ---- single pass: one decode, one upload, three stages ------------------------------
    async def analyze_video(self, video_path: str, configs: dict) -> dict:
        """Scenes + objects + faces from ONE read of the file.

        The reference opens and decodes the file once per task (``cv2.VideoCapture`` at :237 and :331, an ffmpeg child at
        :750-755): three decodes of every frame, and the detection loops decode even the frames they skip (``grab()``, :294).
        Here every frame is read once, goes through pinned host memory into HBM once (chunks of ``batch_size`` frames), and
        all three stages read that copy: K1 (``eioku_scene_sad_luma_bgr``: the luma OpenCV derives from these BGR frames)
        on every frame, the two detectors on the frames their own sampling rule picks (``max(1, int(fps * seconds))``,
        :243 / :337).  ``configs``: ``{"scene_detection": {...}, "object_detection": {...}, "face_detection": {...}}`` -
        the per-task config dicts the backend would have put into three jobs; a task type that is absent is not run.

        Returns ``{task_type: result}`` with, per task, exactly the dict the separate call returns on a BGR source
        (``.npy`` clips and cv2 captures whose backend hands back BGR: tests/test_single_pass_gpu.py).  On a capture
        that can expose the decoder's own Y plane the separate ``detect_scenes`` scores THAT plane (bit-exact with
        ffmpeg); this entry scores the BGR-derived luma, which differs by the YUV -> BGR -> Y round trip.
        """
        import torch

        from . import scene
        from .detect import PipelinedDetector
        from .frames import bgr_to_luma_bt601

        unknown = set(configs) - {"scene_detection", "object_detection", "face_detection", "decode"}
        if unknown:
            raise NotImplementedError(f"analyze_video covers the hot-path task types only, got {sorted(unknown)}")
        logger.info(f"Single-pass analysis ({', '.join(sorted(configs))}): {video_path} (device: {self._get_device()})")
        src = self._open(video_path)
        fps = src.fps or 30
        total_frames = int(src.total_frames)
        dev = torch.device("cuda", torch.cuda.current_device())
        chunk_n = max(1, self._batch_size)
        # Decoder planes when the source can hand them over (a .y4m clip, a cv2 capture that honours CONVERT_RGB = 0):
        # 1.5 bytes per pixel cross PCIe instead of 3, the scene score is taken on the decoder's own Y plane (what ffmpeg's
        # select filter scores: bit-exact with the separate detect_scenes), and the BGR frames the detectors / the
        # ContentDetector read are produced on the device with OpenCV's integer BT.601 (eioku_yuv420_to_bgr) - the
        # conversion cap.read() would have run on the CPU
        if getattr(src, "yuv_layout", None) is None and hasattr(src, "try_yuv") and configs.get("decode", {}).get("planes", True):
            src.try_yuv()
        yuv = getattr(src, "yuv_layout", None)
        lanes = {}  # task -> (lane, sampling interval, meta and device frame rows of the batch being gathered)
        for task in _DETECT_DEFAULTS:
            if task not in configs:
                continue
            cfg = configs[task] or {}
            model_name, conf, seconds, face = _detect_settings(task, cfg)
            detector = self._load_detector(model_name, int(cfg.get("keypoints", 0)) if face else 0)
            interval = _frame_interval(fps, seconds)
            pipe = PipelinedDetector(detector, depth=2, streams=self._lanes(task))
            lanes[task] = (_DetectionLane(detector, face, conf, pipe, self._face_clusterer(cfg) if face else None,
                                          cfg.get("face_alignment", "auto")), interval, [], [])
        want_scenes = "scene_detection" in configs
        scfg = configs.get("scene_detection") or {}
        content = scfg.get("detector", "ffmpeg") == "content"
        sums, prev_dev, npx = [], None, 1
        pinned = [None, None]
        copied = [None, None]  # events: the chunk's upload has left the pinned buffer
        frame_idx, slot = 0, 0
        try:
            done = False
            while not done:
                host = []
                encoded = yuv is None and hasattr(src, "read_encoded")  # Motion-JPEG: file bytes in, decoded on the device
                read = src.read_yuv if yuv else (src.read_encoded if encoded else src.read)
                while len(host) < chunk_n:
                    ret, frame = read()
                    if not ret:
                        done = True
                        break
                    host.append(frame)
                if not host:
                    break
                n = len(host)
                if encoded:
                    host = src.decode(host)  # one decode call per chunk; the chunk is born in HBM
                h, w = host[0].shape[:2]
                fshape = (h, w) if yuv else (h, w, 3)
                if yuv:
                    h = h * 2 // 3
                npx = h * w
                if encoded:
                    chunk = host
                else:
                    if pinned[slot] is None or tuple(pinned[slot].shape[1:]) != fshape:
                        pinned = [torch.empty((chunk_n, *fshape), dtype=torch.uint8).pin_memory() for _ in range(2)]
                        copied = [None, None]
                    if copied[slot] is not None:
                        copied[slot].synchronize()  # the upload that last used this pinned buffer has finished
                    buf = pinned[slot][:n]
                    view = buf.numpy()  # the pinned buffer as an ndarray: frames are copied in without wrapping (possibly
                    for i, f in enumerate(host):  # read-only, memory-mapped) source arrays as tensors
                        view[i] = f
                    chunk = buf.to(dev, non_blocking=True)  # the one trip over PCIe
                    ev = torch.cuda.Event()
                    ev.record()
                    copied[slot] = ev
                    slot ^= 1
                planes = None
                if yuv:
                    planes = chunk
                    chunk = scene.yuv420_to_bgr(planes, h, w, yuv) if (lanes or (want_scenes and content)) else None
                if want_scenes and planes is not None and not content:
                    # K1 straight on the Y planes of the uploaded frames: rows 0 .. h-1 of every (3h/2, w) frame
                    sums.append(scene.luma_sad(planes, prev_dev, shape=(n, h, w), row_stride=w, frame_stride=h * 3 // 2 * w,
                                               keep_on_device=True))
                    prev_dev = planes[n - 1]
                elif want_scenes:
                    if content:
                        sums.append(scene.hsv_sums(chunk, prev_dev, keep_on_device=True))
                    elif npx % 4 == 0:
                        sums.append(scene.luma_sad_bgr(chunk, prev_dev, keep_on_device=True))
                    else:  # odd pixel counts: luma plane on the device, then K1
                        y = bgr_to_luma_bt601(chunk)
                        py = bgr_to_luma_bt601(prev_dev) if prev_dev is not None else None
                        sums.append(scene.luma_sad(y.contiguous(), py.contiguous() if py is not None else None, keep_on_device=True))
                    prev_dev = chunk[n - 1]
                for lane, interval, meta, rows in lanes.values():
                    for i in range(n):
                        idx = frame_idx + i
                        if idx % interval == 0:
                            rows.append(chunk[i])
                            meta.append((idx, _timestamp_ms(idx, fps)))
                            if len(rows) >= self._batch_size:
                                lane.submit(list(meta), _stack_rows(rows))
                                meta.clear()
                                rows.clear()
                frame_idx += n
            for lane, _, meta, rows in lanes.values():
                if rows:
                    lane.submit(meta, _stack_rows(rows))
                lane.finish()
        finally:
            src.release()
            for lane, *_ in lanes.values():
                lane.close()
        out = {task: {"detections": lane.out} for task, (lane, *_) in lanes.items()}
        if want_scenes:
            s_all = torch.cat(sums).cpu().numpy() if sums else np.zeros((0, 3) if content else (0,), np.uint64)
            scene_list = scene.content_scene_list if content else scene.ffmpeg_scene_list
            out["scene_detection"] = {"scenes": scene_list(s_all, npx, scfg, src.time_base, src.duration_s)}
        logger.info(f"✅ Single-pass analysis complete: {frame_idx} frames (header: {total_frames}), "
                    + ", ".join(f"{k}: {len(v.get('detections', v.get('scenes', [])))}" for k, v in out.items()))
        return out

    # ---- scenes ----------------------------------------------------------------------------------------
    async def detect_scenes(self, video_path: str, config: dict) -> dict:
        """Scene boundaries.  Default = what the reference observes from
        ``ffmpeg -vf select='gt(scene\\,T)',showinfo`` (:736-828): luma SAD score (K1), ``pts_time`` with
        six significant digits, the scene list with its index quirk.  ``config["detector"] = "content"``
        selects the PySceneDetect ContentDetector of BASELINE.json's north_star (K2) instead."""
        try:
            from . import scene

            logger.info(f"Scene detection: {video_path}")
            src = self._open(video_path)
            try:
                n = int(src.total_frames)
                chunk = 64
                if config.get("detector", "ffmpeg") == "content":
                    sums = []
                    prev = None
                    for lo in range(0, n, chunk):
                        frames = self._bgr_chunk(src, lo, min(chunk, n - lo))
                        sums.append(scene.hsv_sums(frames, prev))
                        prev = frames[-1]
                    sums = np.concatenate(sums) if sums else np.zeros((0, 3), np.uint64)
                    h, w = (frames.shape[1], frames.shape[2]) if n else (1, 1)
                    return {"scenes": scene.content_scene_list(sums, h * w, config, src.time_base, src.duration_s)}
                from .frames import EndOfStream

                sad = []
                prev = None
                y = None
                lo = 0
                while lo < n:
                    want = min(chunk, n - lo)
                    try:
                        if hasattr(src, "luma_planes_device"):  # Motion-JPEG: the Y planes are decoded into HBM and stay there
                            y = src.luma_planes_device(lo, want)
                        else:
                            y = np.ascontiguousarray(src.luma_planes(lo, want))
                    except EndOfStream:
                        break  # the header's frame count was an estimate: the stream ended early
                    sad.append(scene.luma_sad(y, prev))
                    prev = y[-1]
                    lo += len(y)
                    if len(y) < want:
                        break
                sad = np.concatenate(sad) if sad else np.zeros(0, np.uint64)
                count = int(y.shape[1] * y.shape[2]) if y is not None else 1
                scenes = scene.ffmpeg_scene_list(sad, count, config, src.time_base, src.duration_s)
                if scenes[-1]["scene_index"] == 0:  # the last scene's index is the number of cuts
                    logger.info(f"No scene cuts detected. Created single scene for entire video ({scenes[0]['end_ms']}ms)")
                logger.info(f"✅ Scene detection complete: {len(scenes)} scenes")
                return {"scenes": scenes}
            finally:
                src.release()
        except Exception as e:
            logger.error(f"Scene detection failed: {e}", exc_info=True)
            raise

    # ---- thumbnails: one JPEG per scene (K18) -----------------------------------------------------------------
    async def generate_thumbnails(self, video_path: str, config: dict) -> dict:
        """One thumbnail per scene, resized and JPEG-encoded on the HIP path (``eioku_amd.thumbs``): the stage the
        reference's design schedules behind scene detection.  ``config``: ``scenes`` (the list ``detect_scenes`` returned;
        absent: ``detect_scenes`` is called with ``config["scene_detection"]``), ``size`` (bounding box, default
        ``(320, 180)``), ``quality`` (75), ``position`` (``"start"`` / ``"middle"``: which frame of the scene) and
        ``output_dir`` (required).  One sequential pass over the file uploads only the wanted frames; the files are
        ``<output_dir>/scene_<scene_index:04d>.jpg``."""
        try:
            from . import scene as scene_mod
            from .thumbs import MAX_BATCH, ThumbnailEncoder, scene_frame_index, thumbnail_size

            if not config.get("output_dir"):
                raise ValueError("generate_thumbnails needs config['output_dir']")
            out_dir = Path(config["output_dir"])
            position = config.get("position", "start")
            scenes = config.get("scenes")
            if scenes is None:
                scenes = (await self.detect_scenes(video_path, config.get("scene_detection", {})))["scenes"]
            logger.info(f"Thumbnail generation: {video_path} ({len(scenes)} scenes, device: {self._get_device()})")
            src = self._open(video_path)
            fps = src.fps or 30
            total_frames = int(src.total_frames)
            wanted: dict[int, list[dict]] = {}  # frame index -> the scenes it illustrates
            for sc in scenes:
                wanted.setdefault(scene_frame_index(sc, fps, total_frames, position), []).append(sc)
            if getattr(src, "yuv_layout", None) is None and hasattr(src, "try_yuv"):
                src.try_yuv()
            yuv = getattr(src, "yuv_layout", None)
            encoder = ThumbnailEncoder(config.get("size", (320, 180)), config.get("quality", 75))
            out_dir.mkdir(parents=True, exist_ok=True)
            rows: list[dict] = []
            batch = max(1, min(self._batch_size, MAX_BATCH))

            def flush(indices, frames):
                host = np.stack(frames)
                if yuv:  # decoder planes: 1.5 bytes per pixel cross PCIe, BGR is made on the device
                    import torch

                    h = host.shape[1] * 2 // 3
                    host = scene_mod.yuv420_to_bgr(torch.from_numpy(host).to(torch.device("cuda", torch.cuda.current_device())),
                                                   h, host.shape[2], yuv)
                h, w = int(host.shape[1]), int(host.shape[2])
                tw, th = thumbnail_size(w, h, encoder.size)
                for idx, data in zip(indices, encoder.encode(host)):
                    for sc in wanted[idx]:
                        path = out_dir / f"scene_{int(sc['scene_index']):04d}.jpg"
                        path.write_bytes(data)
                        rows.append({"scene_index": int(sc["scene_index"]), "start_ms": int(sc["start_ms"]),
                                     "end_ms": int(sc["end_ms"]), "timestamp_ms": _timestamp_ms(idx, fps), "frame_index": idx,
                                     "width": tw, "height": th, "thumbnail_path": str(path), "bytes": len(data)})

            try:
                indices, frames = [], []
                last = max(wanted) if wanted else -1
                for frame_idx in range(last + 1):
                    if frame_idx in wanted:
                        ret, frame = src.read_yuv() if yuv else src.read()
                        if not ret:
                            break
                        indices.append(frame_idx)
                        frames.append(frame)
                        if len(frames) >= batch:
                            flush(indices, frames)
                            indices, frames = [], []
                    elif not src.grab():
                        break
                if frames:
                    flush(indices, frames)
            finally:
                src.release()
                encoder.close()
            by_scene = {r["scene_index"]: r for r in rows}  # rows in the order of the scene list (a stream that ended
            rows = [by_scene[int(sc["scene_index"])] for sc in scenes if int(sc["scene_index"]) in by_scene]  # early: fewer)
            logger.info(f"✅ Thumbnail generation complete: {len(rows)} thumbnails")
            return {"thumbnails": rows}
        except Exception as e:
            logger.error(f"Thumbnail generation failed: {e}", exc_info=True)
            raise

    @staticmethod
    def _bgr_chunk(src, lo, count):
        frames = getattr(src, "frames", None)
        if frames is not None:
            return np.ascontiguousarray(frames[lo:lo + count])
        if hasattr(src, "read_encoded"):  # Motion-JPEG: one decode call per chunk, a device tensor
            out = [src.read_encoded()[1] for _ in range(count)]
            return src.decode([f for f in out if f is not None])
        out = []
        for _ in range(count):
            ok, f = src.read()
            if not ok:
                break
            out.append(f)
        return np.stack(out)
