"""Closes the loop from the models to tests/test_conv_gpu.py: every conv-family instantiation a model forward launches
(read from the launch code's own route log) either has a single-layer parity case there or is a fused route whose bytes a
named test compares with the unfused launches.  A retune that moves a model layer onto an instantiation nothing compares
fails here with the route's name."""
import pytest

from eioku_amd import detect as D, faces, ocr, ops, places, weights as W
from eioku_amd.synth import ocr_crops, ocr_frames
from oracle import prng
from test_conv_gpu import ROUTE_CASES

# fused route -> the byte-identity test (tests/test_yolo_gpu.py) that vouches for it: that test asserts that its fused
# process launched the route and that the result equals the unfused launches bit for bit
PAIRS = "test_fused_3x3_1x1_pairs_are_bit_identical_to_separate_launches"
SWITCHES = "test_detect_fusion_switches_leave_the_detections_byte_identical"
STEM = "test_fused_stem_equals_letterbox_then_network"
LAZY = "test_lazy_and_dense_box_branch_give_identical_detections"
FUSED_ROUTES = {
    "persist<NF2,S2,NCH1,DB0,POST1,NWV4>": PAIRS,
    "persist<NF4,S2,NCH1,DB0,POST1,NWV4>": PAIRS,
    "chain<NF1,DB0,CAT1,NFCAT2>": PAIRS,
    "chain<NF2,DB0,CAT0,NFCAT2>": PAIRS,
    "chain<NF2,DB0,CAT2,NFCAT4>": PAIRS,
    "chain<NF2,DB0,CAT3,NFCAT4>": PAIRS,
    "1x1<NF4,UP1,NWV4,CLSMAX0>": PAIRS,
    "1x1<NF6,UP1,NWV4,CLSMAX0>": PAIRS,
    "1x1<NF5,UP0,NWV4,CLSMAX1>": SWITCHES,
    "gather": LAZY,
    "stem_chain<MODE0>": STEM,
    "stem_chain<MODE1>": STEM,
    "stem_chain<MODE2>": STEM,
    "c8<NF1,S2,SRC1>": STEM,
    "c8<NF1,S2,SRC2>": STEM,
    "c8<NF1,S2,SRC3>": SWITCHES,
}


def test_fused_routes_name_tests_that_exist():
    import test_yolo_gpu

    assert not set(FUSED_ROUTES) & set(ROUTE_CASES)
    for route, test in FUSED_ROUTES.items():
        assert callable(getattr(test_yolo_gpu, test, None)), (route, test)


def _yolo(variant, nc, sizes):
    def run(gpu):
        import torch

        det = D.Yolov8Detector(variant, nc, W.random_state(variant, nc, 7))
        for (h, w) in sizes:
            x = torch.zeros((1, h, w, 8), dtype=torch.float16, device=gpu)
            x[..., :3] = 0.5
            det.forward_raw(x)
        det.close()
    return run


def _detect(gpu):
    import torch

    det = D.Yolov8Detector("n", 80, W.random_state("n", 80, 7))
    for (h, w) in ((480, 640), (1080, 1920)):  # a 640-wide copy-mode source and a 1080p one
        f = torch.from_numpy(prng.synth_frames_bgr(5, 2, h, w)).to(gpu)
        det.calibrate_random_head(f, frac=0.01)
        for _ in range(2):  # the second call may evaluate the box branch lazily
            det.detect(f, conf=0.25)
            torch.cuda.synchronize()
    det.close()


def _places(gpu):
    clf = places.Places365Classifier(places.random_state(3))
    clf.classify(prng.synth_frames_bgr(6, 2, 120, 160), 5)
    clf.close()


def _arcface(gpu):
    emb = faces.FaceEmbedder(faces.fold_state(faces.random_state_dict(11)))
    emb.embed(prng.synth_frames_bgr(6, 2, 120, 160), [(0, 10.0, 20.0, 60.0, 90.0), (1, 0.0, 0.0, 160.0, 120.0)])
    emb.close()


def _ocr(gpu):
    r = ocr.OcrReader(ocr.random_craft_state(5), ocr.random_crnn_state(6))
    r.score_maps(ocr_frames(11, 1, 480, 640))
    r.recognize_raw(ocr_crops(1, [64, 192, 320]))
    r.close()


MODELS = {
    "yolov8n": _yolo("n", 80, ((96, 160), (384, 640), (640, 640))),
    "yolov8s": _yolo("s", 80, ((96, 160), (384, 640))),
    "yolov8m": _yolo("m", 80, ((96, 160), (384, 640), (640, 640))),
    "yolov8n-face": _yolo("n", 1, ((96, 160), (384, 640))),
    "detect": _detect,
    "places365-resnet18": _places,
    "arcface-r18": _arcface,
    "craft-and-crnn": _ocr,
}


@pytest.mark.gpu
@pytest.mark.parametrize("model", list(MODELS))
def test_every_route_a_model_takes_is_compared_somewhere(gpu, model):
    ops.conv_routes(reset=True)
    MODELS[model](gpu)
    log = ops.conv_routes(reset=True)
    assert log, "the model launched nothing of the conv family"
    orphans = sorted(r for r in log if r not in ROUTE_CASES and r not in FUSED_ROUTES)
    assert not orphans, (f"{model} runs on instantiations with no single-layer parity case (tests/test_conv_gpu.py ROUTE_CASES) "
                         f"and no byte-identity test (FUSED_ROUTES): {orphans}")
    print(model, len(log), "routes")
