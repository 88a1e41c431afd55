"""The layers tests/test_conv_epilogue_gpu.py compares between the straight-line epilogue of k_conv3x3_flat (the default)
and store_frag's generic loop (EIOKU_CONV_EPI=0); the k_conv3x3_persist layers keep the generic loop under both settings
and must not change either.  The switch is read once per process, so
this file is also a program: ``python conv_epilogue_cases.py OUT.npz`` runs every case in the process it is started in
and writes the raw output buffers and the route log of each; tools/bounds_probe.py launches the same table through the
bounds-check build."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

# (name, (n, h, w, cin, cout, stride), route prefix the layer must run on)
LAYERS = [
    ("p_nf2_nch2", (2, 40, 40, 64, 64, 1), "persist<NF2,S1,NCH2,"),
    ("p_db1", (2, 20, 20, 32, 32, 1), "persist<NF2,S1,NCH1,DB1,"),
    ("p_nwv8_ragged", (2, 17, 33, 72, 80, 1), "persist<NF3,S1,NCH3,DB0,POST0,NWV8>"),  # second cout tile: 32 of 48 couts
    ("p_s2", (1, 50, 52, 64, 64, 2), "persist<NF4,S2,NCH2,"),
    ("f_mt2", (3, 20, 20, 128, 128, 1), "flat<NF4,S1,MT2,"),
    ("f_mt1_s2", (1, 20, 20, 256, 256, 2), "flat<NF4,S2,MT1,"),
]
# (suffix, act code of the C ABI, residual)
VARIANTS = [("silu", 1, False), ("none", 0, False), ("silu_res", 1, True)]
# what stays on the generic loop: a cout that is no multiple of 4, and the fp32 output
FALLBACK = [
    ("fb_cout81", (1, 9, 17, 72, 81, 1), 1, False, False),
    ("fb_f32", (1, 9, 17, 72, 16, 1), 1, False, True),
]
# several tiles per workgroup (1080 tiles of 8 x 16 on at most 4 workgroups per CU): the order of the residual loads and
# the next tile's prefetch only matters from a workgroup's second tile on
STEADY = ("steady", (72, 40, 40, 64, 64, 1), 1, True)
GUARD = 64


def out_dims(h, w, stride):
    return (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1


def launch(gpu, shape, act, res, f32=False, seed=11):
    """One 3x3 layer on seeded operands.  The input is channels [8, 8 + cin) of a buffer that is NaN elsewhere, the fp16
    output channels [4, 4 + cout) of a buffer of 7.0 (fp32: dense between 7.0 guards), the residual channels
    [4, 4 + cout) of a buffer that is NaN elsewhere.  Returns the whole output buffer (device), refused or not."""
    import torch
    from eioku_amd import ops
    from eioku_amd._lib import EiokuHipError

    n, h, w, cin, cout, stride = shape
    ho, wo = out_dims(h, w, stride)
    rng = np.random.default_rng(seed + cin * 1000 + cout + stride)
    x = rng.standard_normal((n, h, w, cin)).astype(np.float16)
    wgt = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32)
    b = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    xbuf = np.full((n, h, w, cin + 16), np.nan, np.float16)
    xbuf[..., 8:8 + cin] = x
    cpad = (cout + 3) // 4 * 4
    kw = dict(stride=stride, act=act, in_coff=8, cin=cin)
    if res:
        rbuf = np.full((n, ho, wo, cpad + 8), np.nan, np.float16)
        rbuf[..., 4:4 + cout] = rng.standard_normal((n, ho, wo, cout)).astype(np.float16)
        kw.update(residual=torch.from_numpy(rbuf).to(gpu), res_coff=4)
    if f32:
        out = torch.full((GUARD + n * ho * wo * cout + GUARD,), 7.0, dtype=torch.float32, device=gpu)
        kw.update(out_f32=out[GUARD:out.numel() - GUARD].view(n, ho, wo, cout))
    else:
        out = torch.full((n, ho, wo, cpad + 8), 7.0, dtype=torch.float16, device=gpu)
        kw.update(out=out, out_coff=4)
    try:
        ops.conv2d_f16(torch.from_numpy(xbuf).to(gpu), wgt, b, **kw)
    except EiokuHipError:
        return out, True
    return out, False


def launch_steady(gpu, seed=13):
    """STEADY as one batch and as two halves; operands generated on the device (14.7 MB of input)."""
    import torch
    from eioku_amd import ops

    _, (n, h, w, cin, cout, stride), act, _ = STEADY
    gen = torch.Generator(device=gpu).manual_seed(seed)
    x = torch.randn((n, h, w, cin), generator=gen, device=gpu, dtype=torch.float32).half()
    r = torch.randn((n, h, w, cout), generator=gen, device=gpu, dtype=torch.float32).half()
    rng = np.random.default_rng(seed)
    wgt = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32)
    b = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    whole = ops.conv2d_f16(x, wgt, b, stride=stride, act=act, residual=r)
    halves = torch.cat([ops.conv2d_f16(x[i:i + n // 2].contiguous(), wgt, b, stride=stride, act=act,
                                       residual=r[i:i + n // 2].contiguous()) for i in (0, n // 2)])
    return whole, halves


def all_cases():
    """(name, shape, act, residual, fp32 output) of every single-layer case"""
    for name, shape, _ in LAYERS:
        for suffix, act, res in VARIANTS:
            yield f"{name}-{suffix}", shape, act, res, False
    yield from FALLBACK


def main(path):
    import torch
    from eioku_amd import _lib, detect as D, ops, weights as W
    from oracle import prng

    _lib.init(0)
    gpu = torch.device("cuda:0")
    arrays, routes, epi = {}, {}, {}
    for name, shape, act, res, f32 in all_cases():
        ops.conv_routes(reset=True)
        out, refused = launch(gpu, shape, act, res, f32)
        torch.cuda.synchronize()
        routes[name] = {"refused": True} if refused else ops.conv_routes(reset=True)
        epi[name] = ops.conv_epi_launches(reset=True)
        arrays[name] = out.cpu().numpy().view(np.uint8)
    ops.conv_routes(reset=True)
    whole, halves = launch_steady(gpu)
    torch.cuda.synchronize()
    routes["steady"] = ops.conv_routes(reset=True)
    epi["steady"] = ops.conv_epi_launches(reset=True)
    arrays["steady"] = whole.cpu().numpy().view(np.uint8)
    arrays["steady_halves"] = halves.cpu().numpy().view(np.uint8)
    # end to end: every 3x3 layer of YOLOv8n, the decode and the NMS behind them
    frames = torch.from_numpy(prng.synth_frames_bgr(43, 2, 96, 160)).to(gpu)
    det = D.Yolov8Detector("n", 80, W.random_state("n", 80, seed=7))
    det.calibrate_random_head(frames, frac=0.02)
    ops.conv_routes(reset=True)
    ops.conv_epi_launches(reset=True)
    dets, counts = det.detect(frames, conf=0.25)
    torch.cuda.synchronize()
    routes["yolo"] = ops.conv_routes(reset=True)
    epi["yolo"] = ops.conv_epi_launches(reset=True)
    arrays["yolo_dets"] = np.ascontiguousarray(dets).view(np.uint8)
    arrays["yolo_counts"] = np.ascontiguousarray(counts)
    det.close()
    np.savez(path, **arrays)
    Path(str(path) + ".routes.json").write_text(json.dumps({"routes": routes, "epi": epi}))


if __name__ == "__main__":
    main(sys.argv[1])
