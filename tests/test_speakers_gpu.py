"""GPU parity of K24 (speaker labels, csrc/speakers.hip) against tests/speaker_oracle.py: features, blocks, pooled
statistics and window vectors, masking and batching, segment vectors, noise reassignment, and ModelManager end to end."""
import asyncio
import json

import numpy as np
import pytest

import block_stats
import face_oracle as fo
import speaker_oracle as so
from eioku_amd import faces, speakers

pytestmark = pytest.mark.gpu

FP32_MEAN, FP32_MAX = 1e-2, 5e-2   # of the activations' RMS: the fp16-network bound of tests/test_faces_gpu.py
COS_FLOOR = 0.99
SEPARATION = 5 * FP32_MEAN         # the oracle's windows must lie this far apart (of the RMS) for "nearest is its own"
FP16_HEADROOM = 65504 / 8          # 8188

# name -> (win_frames, depths, valid frames per window, weight seed)
CASES = {"win40": (40, (1, 1, 1, 1), [40, 40, 33, 17, 16], 3),
         "win40_r34": (40, (3, 4, 6, 3), [40, 40, 33, 17, 16], 5),
         "win200": (200, (1, 1, 1, 1), [200, 120, 56], 11)}
SECONDS = 3


def _audio():
    """Three voices, three seconds each."""
    return np.concatenate([so.voice(10 + i, f0, formants, SECONDS * so.RATE) for i, (f0, formants) in enumerate(so.VOICES)])


def _plan(valid):
    """Windows spread over the three voices (window i starts in voice i % 3)."""
    starts = [(i % 3) * SECONDS * so.RATE + 1000 + 2317 * i for i in range(len(valid))]
    return [(s, v) for s, v in zip(starts, valid)]


_CACHE = {}


@pytest.fixture(scope="module")
def audio():
    return _audio()


@pytest.fixture(scope="module", params=list(CASES))
def case(request, gpu, audio):
    """The labeller and the oracle's side of one shape, computed once."""
    win, depths, valid, seed = CASES[request.param]
    if request.param not in _CACHE:
        sd = speakers.random_state_dict(seed, depths)
        plan = _plan(valid)
        f64 = so.features(audio, plan, win)
        x16 = so.network_input(f64)
        net = so.resnet(sd)
        stats, emb, peak = so.pooled(net, x16, valid)
        _CACHE[request.param] = dict(sd=sd, plan=plan, f64=f64, x16=x16, net=net, stats=stats, emb=emb, peak=peak)
    c = dict(_CACHE[request.param], win=win, depths=depths, valid=valid)
    c["lab"] = speakers.SpeakerLabeller(speakers.fold_state(c["sd"]), win_frames=win)
    yield c
    c["lab"].close()


@pytest.fixture(scope="module")
def small(gpu):
    lab = speakers.SpeakerLabeller(speakers.fold_state(speakers.random_state_dict(3, (1, 1, 1, 1))), win_frames=40)
    yield lab
    lab.close()


def _rel(got, want):
    rms = float(np.sqrt((want ** 2).mean()))
    err = np.abs(got - want)
    return rms, float(err.mean() / rms), float(err.max() / rms)


# ---- 1. features ----------------------------------------------------------------------------------------------------------
def test_features_match_the_float64_oracle(case, audio):
    """Bar: 4 x the oracle's own float32-against-float64 difference on these windows (K22's rule)."""
    f16, f32 = (t.cpu().numpy() for t in case["lab"].features(audio, case["plan"]))
    want = case["f64"]
    bar = 4 * float(np.abs(so.features(audio, case["plan"], case["win"], np.float32).astype(np.float64) - want).max())
    err = float(np.abs(f32.astype(np.float64) - want).max())
    print(f"features win={case['win']}: device - float64 oracle {err:.3e}, bar (4 x float32 oracle) {bar:.3e}")
    assert np.abs(want).max() > 1 and err <= bar
    assert np.array_equal(f16[..., 0].view(np.uint16), f32.astype(np.float16).view(np.uint16))
    assert not f16[..., 1:].any()
    for i, v in enumerate(case["valid"]):
        assert not f32[i, :, v:].any() and not f16[i, :, v:].any() and f32[i, :, :v].any()


def test_digital_silence_and_dc_give_exactly_zero(small):
    n = 400 + 160 * 39
    for x in (np.zeros(n, np.float32), np.full(n, -0.5, np.float32)):
        f16, f32 = small.features(x, [(0, 40), (160, 17)])
        assert not f32.cpu().numpy().any() and not f16.cpu().numpy().any()


# ---- 2. blocks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["layer1.0", "layer2.0"])
def test_blocks_match_torch_fp32(case, gpu, which):
    """Stem + layer1.0, and through layer2.0 (the stride-2 block with its 1x1 shortcut), on the oracle's fp16 input."""
    import torch

    upto = 0 if which == "layer1.0" else case["depths"][0]
    got = case["lab"].forward_raw(torch.from_numpy(case["x16"]).to(gpu), upto_block=upto).cpu().numpy().astype(np.float64)
    want, _ = so.forward_blocks(case["net"], case["x16"], upto)
    assert got.shape == want.shape == (len(case["valid"]), *case["lab"].block_shape(upto))
    rms, mean, mx = _rel(got, want)
    print(f"{which} win={case['win']} depths={case['depths']}: rms {rms:.3f} mean {mean:.2e} max {mx:.2e}")
    assert rms > 0.1 and mean <= FP32_MEAN and mx <= FP32_MAX
    # every channel against its own RMS and the border against the interior: at most 2 x the oracle's fp16 twin at this point
    twin, _ = so.forward_blocks(case["net"], case["x16"], upto, fp16=True)
    block_stats.check(f"speakers {which} win={case['win']} depths={case['depths']}", got, twin, want)


# ---- 3. statistics and embeddings ----------------------------------------------------------------------------------------------
def test_statistics_and_window_vectors_match_torch_fp32(case, gpu, audio):
    import torch

    want_s, want_e, peak = case["stats"], case["emb"], case["peak"]
    m = len(case["valid"])
    # the oracle alone: the windows are far enough apart for "nearest is its own" to mean something, and fp16 has headroom
    rms_s = float(np.sqrt((want_s ** 2).mean()))
    pair = np.sqrt(((want_s[:, None] - want_s[None]) ** 2).mean(-1)) + np.eye(m) * 1e9
    print(f"oracle win={case['win']} depths={case['depths']}: peak activation {peak:.1f}, smallest pairwise distance "
          f"{pair.min() / rms_s:.3f} of the RMS")
    assert pair.min() >= SEPARATION * rms_s and peak < FP16_HEADROOM
    emb, st = case["lab"].forward_raw(torch.from_numpy(case["x16"]).to(gpu), case["valid"], stats=True)
    got_s = speakers.device_to_torch_columns(st.cpu().numpy()).astype(np.float64)
    got_e = emb.cpu().numpy().astype(np.float64)
    for name, got, want in (("statistics", got_s, want_s), ("vectors", got_e, want_e)):
        rms, mean, mx = _rel(got, want)
        print(f"{name}: rms {rms:.3f} mean {mean:.2e} max {mx:.2e}")
        assert rms > 0.1 and mean <= FP32_MEAN and mx <= FP32_MAX
    cos = (got_e * want_e).sum(1) / np.linalg.norm(got_e, axis=1) / np.linalg.norm(want_e, axis=1)
    assert cos.min() >= COS_FLOOR, cos
    nearest = np.sqrt(((got_s[:, None] - want_s[None]) ** 2).mean(-1)).argmin(1)
    assert np.array_equal(nearest, np.arange(m)), nearest
    # features + network in one call (embed_windows) on the device's own features: the same route, close to the oracle too
    own = case["lab"].embed_windows(audio, case["plan"]).cpu().numpy().astype(np.float64)
    rms, mean, mx = _rel(own, want_e)
    assert mean <= FP32_MEAN and mx <= FP32_MAX


# ---- 4. masking and batching -------------------------------------------------------------------------------------------------
def test_samples_past_a_short_window_do_not_matter(small, audio):
    first, valid = 5000, 17
    end = first + 400 + 160 * (valid - 1)
    base = audio[:end + 8000].copy()
    zeros, noise = base.copy(), base.copy()
    zeros[end:] = 0
    noise[end:] = np.random.default_rng(1).standard_normal(len(noise) - end).astype(np.float32)
    a, b = (small.embed_windows(x, [(first, valid)]).cpu().numpy() for x in (zeros, noise))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.abs(a).max() > 0
    fa, fb = (small.features(x, [(first, valid)])[1].cpu().numpy() for x in (zeros, noise))
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32))


def test_more_windows_than_one_pass_and_device_audio_give_the_same_bits(small, audio, gpu):
    import torch

    base = _plan(CASES["win40"][2])
    few = small.embed_windows(audio, base).cpu().numpy()
    many_plan = [base[i % len(base)] for i in range(speakers.PASS + 1)]
    many = small.embed_windows(audio, many_plan).cpu().numpy()
    assert many.shape == (speakers.PASS + 1, 256)
    for i in range(len(many_plan)):
        assert np.array_equal(many[i].view(np.uint32), few[i % len(base)].view(np.uint32)), i
    dev = small.embed_windows(torch.from_numpy(audio).to(gpu), base).cpu().numpy()
    assert np.array_equal(dev.view(np.uint32), few.view(np.uint32))


def test_bad_windows_are_refused(small, audio):
    from eioku_amd._lib import EiokuHipError

    for plan in ([(len(audio) - 400 - 160 * 39 + 1, 40)], [(-1, 40)], [(0, 41)], [(0, 0)], [(0, 8)]):
        with pytest.raises(EiokuHipError):
            small.embed_windows(audio, plan)
    # Under 9 frames the pooling has one column and no standard deviation (tests/test_convnet_glue_host.py pins the NaN): both
    # pooling paths refuse every such window and name it; the features alone still accept a single frame.
    import torch

    x16 = torch.zeros((3, 80, 40, 8), dtype=torch.float16, device="cuda")
    for valid in range(1, 9):
        with pytest.raises(EiokuHipError, match=rf"window 1: {valid} valid frames"):
            small.embed_windows(audio, [(0, 40), (0, valid), (0, 9)])
        with pytest.raises(EiokuHipError, match=rf"window 1: {valid} valid frames"):
            small.forward_raw(x16, [40, valid, 9])
        f16, f32 = small.features(audio, [(0, valid)])
        assert np.isfinite(f32.cpu().numpy()).all() and not f32.cpu().numpy()[0, :, valid:].any()
    assert small.forward_raw(x16, [40, 1, 9], upto_block=0).shape[0] == 3  # a block output pools nothing: any valid goes
    emb = small.embed_windows(audio, [(0, 9)]).cpu().numpy()
    assert emb.shape == (1, 256) and np.isfinite(emb).all()


# ---- 5. segments -------------------------------------------------------------------------------------------------------------
def test_segment_vectors_are_the_normalised_mean_of_their_windows(small, audio):
    n = len(audio)
    segments = [{"start_ms": 100, "end_ms": 2900}, {"start_ms": 3000, "end_ms": 3300}, {"start_ms": 3100, "end_ms": 3700},
                {"start_ms": 6200, "end_ms": 9900}, {"start_ms": 8000, "end_ms": 8420}]
    plans = [speakers.plan_windows(s["start_ms"], s["end_ms"], n, 40) for s in segments]
    # 2.8 s: capped; 300 ms: 28 frames, none; 600 ms: 58 frames, two windows; cut by the end of the audio; 420 ms: 40 frames
    assert [len(p) for p in plans] == [8, 0, 2, 8, 1] and plans[3][-1][0] + 400 + 160 * 39 <= n
    vec, index = small.embed_segments(audio, segments)
    assert index == [0, 2, 3, 4]
    flat = [w for p in plans for w in p]
    wv = small.embed_windows(audio, flat).cpu().numpy()
    first = np.cumsum([0] + [len(p) for p in plans if p])
    want = so.segment_vectors(wv, first)
    got = vec.cpu().numpy()
    assert np.allclose(np.linalg.norm(got.astype(np.float64), axis=1), 1.0, rtol=0, atol=1e-5)
    assert np.abs(got - want).max() <= 1e-6


# ---- 6. assignment -----------------------------------------------------------------------------------------------------------
def _assign_case(e, eps, ms, assign_max, gpu):
    import torch

    te = torch.from_numpy(e).to(gpu)
    labels = faces.dbscan_cosine(te, eps, ms)
    got, cent = speakers.assign_noise(te, labels, assign_max, return_centroids=True)
    want, want_c, margins = so.assign(e, labels.cpu().numpy(), assign_max)
    for _, best, second in margins:                          # the oracle's decisions are not close calls
        assert abs(best - assign_max) >= 1e-4 and second - best >= 1e-4
    assert np.array_equal(got.cpu().numpy(), want)
    assert cent.shape == want_c.shape and (len(want_c) == 0 or np.abs(cent.cpu().numpy() - want_c).max() <= 1e-6)
    return labels.cpu().numpy(), want


def test_noise_rows_take_the_nearest_centroid(gpu):
    e = fo.clustered_set(4, 300, 256, 5, 0.02, noise=30)
    # some rows between two others: too far from either for eps, near enough to a centroid for assign_max
    for i in range(0, 40, 4):
        v = e[i] + 0.55 * e[200 + i // 4]
        e[i] = v / np.linalg.norm(v)
    before, after = _assign_case(e, 0.08, 4, 0.6, gpu)
    assert (before < 0).sum() > 5 and (after < 0).sum() < (before < 0).sum() and (after < 0).sum() > 0
    assert np.array_equal(after[before >= 0], before[before >= 0])


def test_assignment_edge_cases(gpu):
    import torch

    e = fo.clustered_set(7, 120, 256, 3, 0.02, noise=12)
    one = e[:1]
    before, after = _assign_case(one, 0.1, 2, 0.5, gpu)                 # n = 1, noise: no centroid to go to
    assert before.tolist() == [-1] and after.tolist() == [-1]
    before, after = _assign_case(one, 0.1, 1, 0.5, gpu)                 # n = 1, its own cluster
    assert after.tolist() == [0]
    before, after = _assign_case(e, 1e-4, 3, 2.0, gpu)                  # all rows noise
    assert (before < 0).all() and (after < 0).all()
    before, after = _assign_case(e, 0.08, 1, 0.5, gpu)                  # min_samples 1: no noise
    assert (before >= 0).all() and np.array_equal(before, after)
    before, after = _assign_case(e, 0.08, 4, 0.0, gpu)                  # assign_max 0: noise stays
    assert (before < 0).any() and np.array_equal(before, after)
    before, after = _assign_case(e, 0.08, 4, 2.0, gpu)                  # assign_max 2: every noise row is claimed
    assert (before < 0).any() and (after >= 0).all()
    empty = speakers.assign_noise(torch.zeros((0, 256), device=gpu), torch.zeros((0,), dtype=torch.int32, device=gpu), 0.5)
    assert tuple(empty.shape) == (0,)


# ---- 7. end to end -------------------------------------------------------------------------------------------------------------
SPANS = [(0, 1400), (1500, 2900), (3000, 3250), (3100, 4600), (4700, 5900), (6100, 7500), (7600, 8900), (200, 2400), (6500, 8700)]


class FixedTranscriber:
    def transcribe(self, samples, language, **kw):
        return {"segments": [{"start_ms": a, "end_ms": b, "text": f" segment {i}", "language": "en", "confidence": None, "words": None}
                             for i, (a, b) in enumerate(SPANS)], "language": "en"}


def test_model_manager_labels_speakers_like_the_oracle_pipeline(gpu, audio, tmp_path):
    from eioku_amd.model_manager import ModelManager

    path = tmp_path / "talk.npy"
    np.save(path, audio)
    mm = ModelManager(cache_dir=str(tmp_path / "cache"), gpu_transcription=True, gpu_speakers=True, random_init_seed=7,
                      transcriber_factory=lambda c, m: FixedTranscriber())
    plain = asyncio.run(mm.transcribe_video(str(path), {"vad_filter": False}))
    assert asyncio.run(mm.transcribe_video(str(path), {"vad_filter": False, "speaker_labels": False})) == plain
    assert all("speaker" not in s for s in plain["segments"]) and len(plain["segments"]) == len(SPANS)

    # the device's own segment vectors -> eps in the middle of the largest gap of their pairwise distances
    lab = speakers.SpeakerLabeller.from_cache(tmp_path / "cache", seed=7)
    vec, index = lab.embed_segments(audio, plain["segments"])
    lab.close()
    vec = vec.cpu().numpy()
    assert index == [i for i in range(len(SPANS)) if i != 2]             # 250 ms: too short to embed
    d = np.sort(fo.cosine_distances(vec)[np.triu_indices(len(vec), 1)])
    gaps = np.diff(d)
    g = int(np.argmax(gaps))
    print(f"pairwise distances {d[0]:.2e} .. {d[-1]:.2e}, largest gap {gaps[g]:.2e} after {d[g]:.2e}")
    assert gaps[g] >= 2e-4
    eps, assign_max = float(d[g] + gaps[g] / 2), 0.5
    labels, _, margins = so.assign(vec, fo.dbscan(vec, eps, 2), assign_max)
    for _, best, second in margins:
        assert abs(best - assign_max) >= 1e-4 and second - best >= 1e-4
    want = [None] * len(SPANS)
    for i, s in zip(index, speakers.speaker_ids(labels, [SPANS[i][0] for i in index])):
        want[i] = s

    config = {"vad_filter": False, "speaker_labels": True, "speaker_eps": eps, "speaker_min_samples": 2, "speaker_assign_max": assign_max}
    got = asyncio.run(mm.transcribe_video(str(path), config))
    assert [s["speaker"] for s in got["segments"]] == want and any(w is not None for w in want)
    assert [{k: v for k, v in s.items() if k != "speaker"} for s in got["segments"]] == plain["segments"]
    assert asyncio.run(mm.transcribe_video(str(path), config)) == got    # a second run: identical labels
    assert json.loads(json.dumps(got)) == got
