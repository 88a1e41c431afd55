"""Every owner of a library handle, at the smallest configuration the library accepts: ``close()`` twice is accepted, the
handle is false afterwards, and a method called afterwards is refused in Python with ``EiokuHipError``; a constructor
whose loading fails has destroyed the handle or handles it created before the exception reaches the caller.

Destroys are observed through a wrapper on the library's destroy functions, not through device memory.  No closed or
stale handle reaches the library and no failure is provoked on the device: every refusal asserted here is raised by
Python."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DESTROYS = ("yolo", "resnet18", "iresnet", "spk", "craft", "crnn", "thumbs", "vad", "index")


@pytest.fixture
def destroyed(gpu, monkeypatch):
    """The prefixes of the handles destroyed so far, in order."""
    from eioku_amd import _lib

    lib, seen = _lib.load(), []
    for prefix in DESTROYS:
        real = getattr(lib, f"eioku_{prefix}_destroy")

        def destroy(h, prefix=prefix, real=real):
            seen.append(prefix)
            real(h)

        monkeypatch.setattr(lib, f"eioku_{prefix}_destroy", destroy)
    return seen


@pytest.fixture(scope="module")
def states():
    from eioku_amd import faces, ocr, places, speakers, weights

    return {"faces": faces.fold_state(faces.random_state_dict(3, (1, 1, 1, 1))),
            "speakers": speakers.fold_state(speakers.random_state_dict(3, (1, 1, 1, 1))),
            "yolo": weights.random_state("n", 80, seed=1),
            "craft": ocr.random_craft_state(5), "crnn": ocr.random_crnn_state(6),
            "places": places.random_state(3)}


def _owners(states):
    """name -> (build, a call to make on the closed owner, the destroys a close makes)."""
    from eioku_amd import detect, faces, ocr, places, search, speakers, thumbs, vad

    return {
        "FaceEmbedder": (lambda: faces.FaceEmbedder(states["faces"]), lambda o: o.last_flops(), ["iresnet"]),
        "SpeakerLabeller": (lambda: speakers.SpeakerLabeller(states["speakers"], win_frames=40), lambda o: o.last_ms(), ["spk"]),
        "SileroVad": (lambda: vad.SileroVad(vad.seeded_weights(2), slab_chunks=8), lambda o: o.speech_probs(np.zeros(2048, np.float32)),
                      ["vad"]),
        "IndexFlatL2": (lambda: search.IndexFlatL2(64), lambda o: o.ntotal, ["index"]),
        "Yolov8Detector": (lambda: detect.Yolov8Detector("n", 80, states["yolo"]),
                           lambda o: o.detect(np.zeros((1, 32, 32, 3), np.uint8), imgsz=32), ["yolo"]),
        "ThumbnailEncoder": (thumbs.ThumbnailEncoder, lambda o: o.encode(np.zeros((1, 24, 32, 3), np.uint8)), ["thumbs"]),
        "Places365Classifier": (lambda: places.Places365Classifier(states["places"]),
                                lambda o: o.classify(np.zeros((1, 24, 32, 3), np.uint8)), ["resnet18"]),
        "OcrReader": (lambda: ocr.OcrReader(states["craft"], states["crnn"]), lambda o: o.last_flops(), ["craft", "crnn"]),
    }


@pytest.mark.parametrize("name", ["FaceEmbedder", "SpeakerLabeller", "SileroVad", "IndexFlatL2", "Yolov8Detector",
                                  "ThumbnailEncoder", "Places365Classifier", "OcrReader"])
def test_close_is_idempotent_and_a_closed_owner_is_refused_in_python(name, states, destroyed):
    from eioku_amd._lib import EiokuHipError

    build, use, prefixes = _owners(states)[name]
    owner = build()
    handles = [owner._d, owner._r] if name == "OcrReader" else [owner._h]
    assert all(handles) and destroyed == []
    owner.close()
    assert destroyed == prefixes and not any(handles)
    owner.close()
    assert destroyed == prefixes
    with pytest.raises(EiokuHipError, match="handle is closed"):
        use(owner)
    del owner, handles
    assert destroyed == prefixes


def _without(d: dict, key: str) -> dict:
    return {k: v for k, v in d.items() if k != key}


def _narrower(pair):
    """(weight, bias) with one input channel less."""
    return pair[0][:, :-1], pair[1]


def _failing(states):
    """id -> (constructor, the exception it documents, the destroys it must have made)."""
    from eioku_amd import detect, faces, ocr, speakers

    f, s, y, craft, crnn = (states[k] for k in ("faces", "speakers", "yolo", "craft", "crnn"))
    conv = "layer2.0.conv1"
    narrow_craft = dict(craft, **{"basenet.slice1.3.weight": craft["basenet.slice1.3.weight"][:, :-1]})
    return {
        "faces-missing": (lambda: faces.FaceEmbedder(dict(f, convs=_without(f["convs"], conv))), KeyError, ["iresnet"]),
        "faces-shape": (lambda: faces.FaceEmbedder(dict(f, convs=dict(f["convs"], **{conv: _narrower(f["convs"][conv])}))),
                        ValueError, ["iresnet"]),
        "speakers-missing": (lambda: speakers.SpeakerLabeller(dict(s, convs=_without(s["convs"], conv)), win_frames=40), KeyError, ["spk"]),
        "speakers-shape": (lambda: speakers.SpeakerLabeller(dict(s, convs=dict(s["convs"], **{conv: _narrower(s["convs"][conv])})),
                                                            win_frames=40), ValueError, ["spk"]),
        "yolo-missing": (lambda: detect.Yolov8Detector("n", 80, _without(y, "model.1.conv")), KeyError, ["yolo"]),
        "yolo-shape": (lambda: detect.Yolov8Detector("n", 80, dict(y, **{"model.1.conv": _narrower(y["model.1.conv"])})),
                       ValueError, ["yolo"]),
        # the reader's second handle is destroyed first, then the first
        "ocr-missing": (lambda: ocr.OcrReader(_without(craft, "basenet.slice1.0.weight"), crnn), KeyError, ["crnn", "craft"]),
        "ocr-shape": (lambda: ocr.OcrReader(narrow_craft, crnn), ValueError, ["crnn", "craft"]),
        # the class count is read from Prediction.weight before either handle exists
        "ocr-no-prediction": (lambda: ocr.OcrReader(craft, _without(crnn, "Prediction.weight")), KeyError, []),
    }


@pytest.mark.parametrize("case", ["faces-missing", "faces-shape", "speakers-missing", "speakers-shape", "yolo-missing",
                                  "yolo-shape", "ocr-missing", "ocr-shape", "ocr-no-prediction"])
def test_a_constructor_that_fails_to_load_has_destroyed_its_handles(case, states, destroyed):
    build, error, prefixes = _failing(states)[case]
    with pytest.raises(error):
        build()
    assert destroyed == prefixes
