"""GPU parity: K4 implicit-GEMM conv (fp16 operands, fp32 accumulate) vs torch-CPU conv2d in float64 on the
same fp16-rounded operands.  Tolerance: the fp32 accumulation order differs (MFMA vs CPU), and the
result is rounded to fp16 once, so outputs agree to 1 fp16 ulp (rel 2**-10) + tiny absolute slack.

Which ``__global__`` instantiation a shape runs on is decided on the host (pick_nf and plan_conv of csrc/conv_plan.h;
tests/test_conv_plan_host.py holds the plan to this file's table without a GPU).  Every case here names the
instantiation ("route") it is there for, and the test reads the route back from
the launch code's own log (``ops.conv_routes``): a retune that moves a shape elsewhere fails with both names instead
of leaving an instantiation untested."""
import numpy as np
import pytest

from eioku_amd import ops

pytestmark = pytest.mark.gpu

RTOL = 2.0 ** -9   # 2 fp16 ulps
ATOL = 2e-3


def ref_conv(x_nhwc16, w, b, stride, silu, residual16=None, out_f32=False, act=None):
    """float64 conv2d on the fp16-rounded operands, then the kernel's rounding order: fp16 once, the residual add, fp16
    again.  ``act``: the C ABI's code (0 none, 1 SiLU, 2 ReLU, 3 ReLU after the residual sum); default from ``silu``."""
    import torch
    import torch.nn.functional as F

    act = int(bool(silu)) if act is None else act
    x = torch.from_numpy(x_nhwc16.astype(np.float64)).permute(0, 3, 1, 2)
    w16 = torch.from_numpy(w.astype(np.float16).astype(np.float64))
    k = w.shape[-1]
    y = F.conv2d(x, w16, None if b is None else torch.from_numpy(b.astype(np.float64)), stride=stride, padding=k // 2)
    if act == 1:
        y = y * torch.sigmoid(y)
    elif act == 2:
        y = torch.relu(y)
    y = y.permute(0, 2, 3, 1).contiguous()
    if out_f32:
        return y.float().numpy()
    y = y.half()
    if residual16 is not None:
        y = y.double() + torch.from_numpy(residual16.astype(np.float64))
        y = (torch.relu(y) if act == 3 else y).half()
    elif act == 3:
        y = torch.relu(y)
    return y.numpy()


def bar_fraction(got, want):
    """worst |got - want| as a fraction of this file's fp16 bar (<= 1 passes)"""
    got = got.astype(np.float64)
    want = want.astype(np.float64)
    if got.size == 0:
        return 0.0
    return float((np.abs(got - want) / (ATOL + RTOL * np.abs(want))).max())


def close(a, b):
    return bar_fraction(a, b) <= 1.0


def out_dims(h, w, k, stride):
    return (h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1


# route -> (n, h, w, cin, cout, k, stride) cases that must run on it.  Per family: the smallest shapes that land on each
# instantiation, maps of 1x1 and 1x5 pixels, 2x2 at stride 2, output widths on either side of the 24- and 48-pixel cuts,
# Ho on either side of the 8-wave threshold, cin that is no multiple of 32, tiles that cross frame borders (flat).
ROUTE_CASES = {
    "igemm<NF1,K3,S1>": [(1, 50, 50, 128, 1, 3, 1), (1, 3, 25, 104, 1, 3, 1)],
    "igemm<NF1,K3,S2>": [(1, 100, 100, 128, 1, 3, 2), (1, 17, 16, 104, 1, 3, 2)],
    "igemm<NF2,K3,S1>": [(1, 9, 49, 104, 32, 3, 1), (1, 3, 49, 104, 32, 3, 1)],
    "igemm<NF2,K3,S2>": [(1, 98, 66, 72, 32, 3, 2), (1, 5, 160, 72, 32, 3, 2)],
    "igemm<NF3,K3,S1>": [(1, 9, 49, 104, 48, 3, 1), (1, 3, 49, 104, 48, 3, 1)],
    "igemm<NF3,K3,S2>": [(1, 5, 160, 72, 48, 3, 2), (1, 5, 50, 72, 48, 3, 2)],
    "igemm<NF4,K3,S1>": [(1, 49, 51, 104, 64, 3, 1), (1, 9, 49, 128, 64, 3, 1), (1, 17, 49, 128, 64, 3, 1)],
    "igemm<NF4,K3,S2>": [(2, 2, 2, 128, 64, 3, 2), (1, 15, 50, 72, 64, 3, 2), (1, 9, 95, 128, 64, 3, 2), (1, 9, 97, 128, 64, 3, 2)],
    "igemm<NF5,K3,S1>": [(1, 9, 49, 104, 80, 3, 1), (1, 3, 49, 104, 80, 3, 1)],
    "igemm<NF5,K3,S2>": [(1, 56, 56, 144, 80, 3, 2), (2, 2, 2, 144, 80, 3, 2), (1, 9, 95, 144, 80, 3, 2), (1, 9, 97, 144, 80, 3, 2)],
    "igemm<NF6,K3,S1>": [(1, 52, 84, 192, 96, 3, 1), (1, 3, 49, 144, 192, 3, 1)],
    "igemm<NF6,K3,S2>": [(1, 50, 50, 96, 192, 3, 2), (1, 5, 160, 40, 96, 3, 2)],
    "flat<NF2,S1,MT1,NS8>": [(1, 1, 1, 40, 32, 3, 1), (2, 1, 1, 40, 32, 3, 1)],
    "flat<NF2,S1,MT2,NS4>": [(5, 5, 7, 128, 32, 3, 1), (2, 3, 8, 40, 64, 3, 1)],
    "flat<NF2,S1,MT2,NS8>": [(2, 24, 24, 40, 32, 3, 1), (1, 3, 24, 144, 32, 3, 1)],
    "flat<NF2,S2,MT1,NS8>": [(1, 9, 11, 40, 32, 3, 2), (2, 1, 1, 40, 32, 3, 2), (2, 1, 5, 40, 32, 3, 2), (1, 9, 24, 40, 32, 3, 2), (1, 9, 25, 40, 32, 3, 2), (1, 9, 48, 40, 32, 3, 2), (1, 17, 48, 40, 32, 3, 2)],
    "flat<NF3,S1,MT1,NS8>": [(2, 1, 1, 72, 80, 3, 1), (1, 1, 1, 72, 80, 3, 1)],
    "flat<NF3,S1,MT2,NS4>": [(1, 9, 9, 144, 144, 3, 1), (1, 3, 8, 72, 80, 3, 1)],
    "flat<NF3,S1,MT2,NS8>": [(2, 24, 24, 48, 48, 3, 1), (2, 1, 5, 72, 80, 3, 1), (2, 2, 2, 72, 80, 3, 1), (1, 9, 24, 72, 80, 3, 1)],
    "flat<NF3,S2,MT1,NS8>": [(3, 7, 5, 160, 48, 3, 2), (1, 5, 16, 144, 48, 3, 2)],
    "flat<NF4,S1,MT1,NS8>": [(2, 1, 1, 128, 64, 3, 1), (1, 1, 1, 128, 64, 3, 1)],
    "flat<NF4,S1,MT2,NS4>": [(3, 20, 20, 128, 128, 3, 1), (1, 9, 8, 104, 64, 3, 1)],
    "flat<NF4,S1,MT2,NS8>": [(2, 24, 24, 104, 64, 3, 1), (2, 1, 5, 128, 64, 3, 1), (2, 2, 2, 128, 64, 3, 1), (1, 9, 24, 128, 64, 3, 1), (1, 9, 25, 128, 64, 3, 1), (1, 9, 48, 128, 64, 3, 1), (1, 17, 48, 128, 64, 3, 1)],
    "flat<NF4,S2,MT1,NS8>": [(1, 20, 20, 256, 256, 3, 2), (3, 40, 40, 128, 256, 3, 2), (2, 21, 19, 136, 64, 3, 2), (2, 1, 1, 128, 64, 3, 2), (2, 1, 5, 128, 64, 3, 2), (1, 9, 24, 128, 64, 3, 2), (1, 9, 25, 128, 64, 3, 2), (1, 9, 48, 128, 64, 3, 2), (1, 9, 49, 128, 64, 3, 2), (1, 17, 48, 128, 64, 3, 2), (1, 17, 49, 128, 64, 3, 2)],
    "flat<NF5,S1,MT1,NS8>": [(1, 1, 1, 144, 80, 3, 1), (2, 1, 1, 144, 80, 3, 1)],
    "flat<NF5,S1,MT2,NS4>": [(1, 7, 9, 104, 80, 3, 1), (1, 9, 8, 144, 80, 3, 1)],
    "flat<NF5,S1,MT2,NS8>": [(2, 40, 40, 128, 80, 3, 1), (1, 8, 24, 104, 80, 3, 1)],
    "flat<NF5,S2,MT1,NS8>": [(1, 15, 17, 40, 80, 3, 2), (2, 1, 1, 144, 80, 3, 2), (2, 1, 5, 144, 80, 3, 2), (1, 9, 24, 144, 80, 3, 2), (1, 9, 25, 144, 80, 3, 2), (1, 9, 48, 144, 80, 3, 2), (1, 9, 49, 144, 80, 3, 2), (1, 17, 48, 144, 80, 3, 2), (1, 17, 49, 144, 80, 3, 2)],
    "flat<NF6,S1,MT1,NS8>": [(2, 1, 1, 104, 96, 3, 1), (1, 1, 1, 104, 96, 3, 1)],
    "flat<NF6,S1,MT2,NS4>": [(1, 7, 9, 104, 96, 3, 1), (1, 9, 8, 104, 96, 3, 1)],
    "flat<NF6,S1,MT2,NS8>": [(2, 24, 24, 104, 96, 3, 1), (1, 3, 25, 104, 192, 3, 1)],
    "flat<NF6,S2,MT1,NS8>": [(1, 15, 17, 40, 96, 3, 2), (1, 40, 40, 384, 576, 3, 2)],
    "persist<NF1,S1,NCH1,DB1,POST0,NWV4>": [(1, 8, 16, 8, 16, 3, 1), (2, 1, 1, 16, 16, 3, 1), (2, 1, 5, 16, 16, 3, 1), (2, 2, 2, 16, 16, 3, 1), (1, 9, 24, 16, 16, 3, 1), (1, 9, 25, 16, 16, 3, 1), (1, 9, 48, 16, 16, 3, 1), (1, 9, 49, 16, 16, 3, 1), (1, 17, 48, 16, 16, 3, 1), (1, 17, 49, 16, 16, 3, 1)],
    "persist<NF1,S1,NCH2,DB1,POST0,NWV4>": [(2, 9, 17, 40, 1, 3, 1), (1, 17, 8, 40, 1, 3, 1)],
    "persist<NF1,S1,NCH3,DB0,POST0,NWV4>": [(1, 9, 17, 72, 16, 3, 1), (1, 17, 8, 72, 1, 3, 1)],
    "persist<NF1,S2,NCH1,DB0,POST0,NWV4>": [(1, 19, 35, 16, 16, 3, 2), (2, 1, 1, 16, 16, 3, 2), (2, 1, 5, 16, 16, 3, 2), (2, 2, 2, 16, 16, 3, 2), (1, 9, 24, 16, 16, 3, 2), (1, 9, 25, 16, 16, 3, 2), (1, 9, 48, 16, 16, 3, 2), (1, 9, 49, 16, 16, 3, 2), (1, 17, 48, 16, 16, 3, 2), (1, 17, 49, 16, 16, 3, 2)],
    "persist<NF1,S2,NCH2,DB0,POST0,NWV4>": [(1, 19, 35, 40, 16, 3, 2), (1, 5, 96, 40, 1, 3, 2)],
    "persist<NF1,S2,NCH3,DB0,POST0,NWV4>": [(1, 19, 35, 72, 16, 3, 2), (2, 5, 48, 72, 1, 3, 2)],
    "persist<NF2,S1,NCH1,DB1,POST0,NWV4>": [(2, 20, 20, 32, 32, 3, 1), (2, 3, 8, 16, 32, 3, 1)],
    "persist<NF2,S1,NCH2,DB0,POST0,NWV4>": [(2, 40, 40, 64, 64, 3, 1), (1, 3, 80, 40, 32, 3, 1)],
    "persist<NF2,S2,NCH1,DB0,POST0,NWV4>": [(1, 33, 47, 16, 32, 3, 2), (2, 5, 48, 16, 32, 3, 2)],
    "persist<NF2,S2,NCH2,DB0,POST0,NWV4>": [(2, 50, 50, 40, 32, 3, 2), (2, 2, 2, 40, 32, 3, 2), (1, 9, 49, 40, 32, 3, 2), (1, 17, 49, 40, 32, 3, 2), (1, 9, 95, 40, 32, 3, 2), (1, 9, 97, 40, 32, 3, 2)],
    "persist<NF3,S1,NCH1,DB1,POST0,NWV4>": [(1, 11, 19, 16, 48, 3, 1), (1, 3, 24, 8, 48, 3, 1)],
    "persist<NF3,S1,NCH2,DB0,POST0,NWV4>": [(1, 24, 40, 48, 80, 3, 1), (1, 3, 25, 40, 128, 3, 1)],
    "persist<NF3,S1,NCH3,DB0,POST0,NWV4>": [(2, 8, 33, 72, 80, 3, 1), (1, 3, 49, 72, 96, 3, 1)],
    "persist<NF3,S1,NCH3,DB0,POST0,NWV8>": [(2, 17, 33, 72, 80, 3, 1), (2, 9, 33, 72, 80, 3, 1), (2, 16, 33, 72, 80, 3, 1), (1, 9, 25, 72, 80, 3, 1), (1, 9, 48, 72, 80, 3, 1), (1, 9, 49, 72, 80, 3, 1), (1, 17, 48, 72, 80, 3, 1), (1, 17, 49, 72, 80, 3, 1)],
    "persist<NF3,S2,NCH1,DB0,POST0,NWV4>": [(1, 19, 35, 16, 48, 3, 2), (2, 5, 16, 16, 80, 3, 2)],
    "persist<NF3,S2,NCH2,DB0,POST0,NWV4>": [(1, 50, 52, 64, 48, 3, 2), (2, 5, 96, 40, 48, 3, 2)],
    "persist<NF4,S1,NCH1,DB1,POST0,NWV4>": [(1, 11, 19, 32, 64, 3, 1), (1, 9, 8, 8, 64, 3, 1)],
    "persist<NF4,S2,NCH1,DB0,POST0,NWV4>": [(1, 19, 35, 32, 64, 3, 2), (1, 17, 16, 16, 64, 3, 2)],
    "persist<NF4,S2,NCH2,DB0,POST0,NWV4>": [(1, 50, 52, 64, 64, 3, 2), (1, 17, 50, 40, 64, 3, 2)],
    "1x1<NF1,UP0,NWV4,CLSMAX0>": [(1, 16, 16, 64, 1, 1, 1), (2, 17, 80, 16, 16, 1, 1)],
    "1x1<NF2,UP0,NWV4,CLSMAX0>": [(1, 7, 9, 24, 32, 1, 1), (2, 1, 1, 24, 32, 1, 1), (2, 1, 5, 24, 32, 1, 1), (2, 2, 2, 24, 32, 1, 1), (1, 9, 24, 24, 32, 1, 1), (1, 9, 25, 24, 32, 1, 1), (1, 9, 48, 24, 32, 1, 1), (1, 9, 49, 24, 32, 1, 1), (1, 17, 48, 24, 32, 1, 1), (1, 17, 49, 24, 32, 1, 1)],
    "1x1<NF3,UP0,NWV4,CLSMAX0>": [(1, 7, 9, 40, 48, 1, 1), (1, 7, 9, 1152, 576, 1, 1)],
    "1x1<NF4,UP0,NWV4,CLSMAX0>": [(3, 12, 20, 128, 64, 1, 1), (1, 12, 20, 384, 128, 1, 1), (2, 20, 20, 512, 256, 1, 1), (2, 5, 3, 160, 64, 1, 1), (2, 1, 1, 136, 64, 1, 1), (2, 1, 5, 136, 64, 1, 1), (2, 2, 2, 136, 64, 1, 1), (1, 9, 24, 136, 64, 1, 1), (1, 9, 25, 136, 64, 1, 1), (1, 9, 48, 136, 64, 1, 1), (1, 9, 49, 136, 64, 1, 1), (1, 17, 48, 136, 64, 1, 1), (1, 17, 49, 136, 64, 1, 1)],
    "1x1<NF5,UP0,NWV4,CLSMAX0>": [(1, 16, 16, 80, 80, 1, 1), (1, 9, 7, 136, 80, 1, 1)],
    "1x1<NF6,UP0,NWV4,CLSMAX0>": [(1, 7, 9, 40, 96, 1, 1), (2, 17, 80, 16, 192, 1, 1)],
    "1x1<NF8,UP0,NWV4,CLSMAX0>": [(1, 10, 10, 256, 128, 1, 1), (2, 17, 80, 16, 128, 1, 1)],
    "c8<NF1,S2,SRC0>": [(2, 64, 64, 8, 16, 3, 2), (2, 1, 1, 8, 16, 3, 2), (2, 1, 5, 8, 16, 3, 2), (2, 2, 2, 8, 16, 3, 2), (1, 9, 24, 8, 16, 3, 2), (1, 9, 25, 8, 16, 3, 2), (1, 9, 48, 8, 16, 3, 2), (1, 9, 49, 8, 16, 3, 2), (1, 17, 48, 8, 16, 3, 2), (1, 17, 49, 8, 16, 3, 2)],
    "c8<NF2,S2,SRC0>": [(1, 19, 35, 8, 32, 3, 2), (1, 5, 96, 8, 32, 3, 2)],
    "c8<NF3,S2,SRC0>": [(1, 19, 35, 8, 48, 3, 2), (2, 5, 16, 8, 80, 3, 2)],
    "c8<NF4,S2,SRC0>": [(1, 19, 35, 8, 64, 3, 2), (1, 17, 16, 8, 64, 3, 2)],
}
CASES = [c for cases in ROUTE_CASES.values() for c in cases]
ROUTE_OF = {c: r for r, cases in ROUTE_CASES.items() for c in cases}
assert len(ROUTE_OF) == len(CASES)


def operands(case, seed):
    n, h, w, cin, cout, k, stride = case
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h, w, cin)).astype(np.float16)
    wgt = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
    b = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    return x, wgt, b


@pytest.mark.parametrize("n,h,w,cin,cout,k,stride", CASES)
def test_conv_matches_torch_cpu(gpu, n, h, w, cin, cout, k, stride):
    import torch

    case = (n, h, w, cin, cout, k, stride)
    x, wgt, b = operands(case, cin * 1000 + cout + k + stride)
    ops.conv_routes(reset=True)
    got = ops.conv2d_f16(torch.from_numpy(x).to(gpu), wgt, b, stride=stride, silu=True).cpu().numpy()
    assert ops.conv_routes(reset=True) == {ROUTE_OF[case]: 1}
    want = ref_conv(x, wgt, b, stride, True)
    assert got.shape == want.shape
    frac = bar_fraction(got, want)
    print(f"{ROUTE_OF[case]} {case}: worst error {frac:.3f} of the bar")
    assert frac <= 1.0, float(np.abs(got.astype(np.float32) - want.astype(np.float32)).max())


# ---- one instantiation whose LDS size varies at run time: below the 64 KB default, above it, below it again --------------
# (route, small layer, large layer).  The launch code lifts a kernel's dynamic-LDS ceiling once per larger request and keeps
# it; the sizes come from the plan (ops.conv_plan), so the cases stay on either side of 64 KB or fail saying so.  1x1: 6 KB
# and 108 KB of weights.  flat: no smaller pair exists on one instantiation -- the large layer's three 1 x 48 frames make
# the 9-row patch of a tile that crosses two frame borders, 192 bytes above 64 KB.
LDS_STEPS = [
    ("1x1<NF3,UP0,NWV4,CLSMAX0>", (1, 7, 9, 40, 48, 1, 1), (1, 7, 9, 1152, 576, 1, 1)),
    ("flat<NF4,S1,MT2,NS8>", (2, 24, 24, 104, 64, 3, 1), (3, 1, 48, 104, 64, 3, 1)),
]


@pytest.mark.parametrize("route,small,large", LDS_STEPS, ids=[s[0] for s in LDS_STEPS])
def test_lds_ceiling_follows_small_large_small_launches(gpu, route, small, large):
    import torch

    assert ops.conv_plan(*small)[0] == route and ops.conv_plan(*small)[1] <= 64 * 1024
    assert ops.conv_plan(*large)[0] == route and ops.conv_plan(*large)[1] > 64 * 1024
    want = {}
    for case in (small, large, small):
        stride = case[6]
        x, wgt, b = operands(case, 77)
        if case not in want:
            want[case] = ref_conv(x, wgt, b, stride, True)
        ops.conv_routes(reset=True)
        got = ops.conv2d_f16(torch.from_numpy(x).to(gpu), wgt, b, stride=stride, silu=True).cpu().numpy()
        assert ops.conv_routes(reset=True) == {route: 1}
        frac = bar_fraction(got, want[case])
        print(f"{route} {case} ({ops.conv_plan(*case)[1]} B of LDS): worst error {frac:.3f} of the bar")
        assert got.shape == want[case].shape and frac <= 1.0


# ---- epilogues, slices and canaries ----------------------------------------------------------------------------------
# ((n, h, w, cin, cout, k, stride), act, residual, fp32 output, route).  The input is channels [8, 8 + cin) of a buffer 16
# channels wider that is NaN elsewhere; an fp16 output goes to channels [4, 4 + cout) of a wider buffer pre-filled with
# 7.0 (an fp32 output is dense: the 7.0 guard is before and after it); a residual is channels [4, 4 + cout) of a buffer
# that is NaN elsewhere.
def _ragged(case):
    """the same layer with a cout that is no multiple of 16 but has as many 16-wide fragments: the same route"""
    n, h, w, cin, cout, k, stride = case
    return (n, h, w, cin, cout - 4 if cout > 4 else cout, k, stride)


# every route: a ragged cout tile next to live neighbours
EPILOGUE_CASES = [(_ragged(cases[0]), 1, False, False, route) for route, cases in ROUTE_CASES.items()]
# residual slices with the activation before (1) and after (3) the sum, one route per family and the 8-wave kernel
EPILOGUE_CASES += [(_ragged(c), act, True, False, ROUTE_OF[c]) for act in (1, 3) for c in (
    (1, 49, 51, 104, 64, 3, 1), (3, 20, 20, 128, 128, 3, 1), (2, 21, 19, 136, 64, 3, 2), (2, 20, 20, 32, 32, 3, 1),
    (2, 17, 33, 72, 80, 3, 1), (3, 12, 20, 128, 64, 1, 1))]
# cout a custom model can ask for (nc is a loader parameter), fp16 and fp32 output: within the bar, or refused with the
# neighbours intact
ODD_COUTS = (2, 3, 5, 81)
EPILOGUE_CASES += [((2, 9, 17, 40, cout, k, 1), 1, False, f32, route) for f32 in (False, True) for (k, cout, route) in (
    (3, 2, "persist<NF1,S1,NCH2,DB1,POST0,NWV4>"), (3, 3, "persist<NF1,S1,NCH2,DB1,POST0,NWV4>"),
    (3, 5, "persist<NF1,S1,NCH2,DB1,POST0,NWV4>"), (3, 81, "flat<NF3,S1,MT2,NS4>"),
    (1, 2, "1x1<NF1,UP0,NWV4,CLSMAX0>"), (1, 3, "1x1<NF1,UP0,NWV4,CLSMAX0>"), (1, 5, "1x1<NF1,UP0,NWV4,CLSMAX0>"),
    (1, 81, "1x1<NF6,UP0,NWV4,CLSMAX0>"))]
GUARD = 64  # fp32 elements of 7.0 on either side of a dense fp32 output


def launch_epilogue(gpu, item, seed=5):
    """Runs one EPILOGUE_CASES item; returns (refused, output buffer on the device, numpy operands) -- tools/bounds_probe.py
    launches the same table through the bounds-check build."""
    import torch
    from eioku_amd._lib import EiokuHipError

    case, act, res, f32, _ = item
    n, h, w, cin, cout, k, stride = case
    ho, wo = out_dims(h, w, k, stride)
    x, wgt, b = operands(case, seed + cin * 1000 + cout + k + stride)
    rng = np.random.default_rng(seed)
    xbuf = np.full((n, h, w, cin + 16), np.nan, np.float16)
    xbuf[..., 8:8 + cin] = x
    cpad = (cout + 3) // 4 * 4
    rbuf = None
    if res:
        rbuf = np.full((n, ho, wo, cpad + 8), np.nan, np.float16)
        rbuf[..., 4:4 + cout] = rng.standard_normal((n, ho, wo, cout)).astype(np.float16)
    kw = dict(stride=stride, act=act, in_coff=8, cin=cin)
    if res:
        kw.update(residual=torch.from_numpy(rbuf).to(gpu), res_coff=4)
    if f32:
        out = torch.full((GUARD + n * ho * wo * cout + GUARD,), 7.0, dtype=torch.float32, device=gpu)
        kw.update(out_f32=out[GUARD:out.numel() - GUARD].view(n, ho, wo, cout))
    else:
        out = torch.full((n, ho, wo, cpad + 8), 7.0, dtype=torch.float16, device=gpu)
        kw.update(out=out, out_coff=4)
    try:
        ops.conv2d_f16(torch.from_numpy(xbuf).to(gpu), wgt, b, **kw)
        refused = False
    except EiokuHipError:
        refused = True
    return refused, out, (x, wgt, b, None if rbuf is None else rbuf[..., 4:4 + cout])


def _epilogue_id(item):
    case, act, res, f32, route = item
    return "-".join(map(str, case)) + f"-act{act}" + ("-res" if res else "") + ("-f32" if f32 else "")


@pytest.mark.parametrize("item", EPILOGUE_CASES, ids=_epilogue_id)
def test_conv_epilogue_writes_its_slice_and_nothing_else(gpu, item):
    case, act, res, f32, route = item
    n, h, w, cin, cout, k, stride = case
    ops.conv_routes(reset=True)
    refused, out, (x, wgt, b, r) = launch_epilogue(gpu, item)
    log = ops.conv_routes(reset=True)
    got = out.cpu().numpy()
    if refused:  # loudly, before any launch, and only a cout no model of the project has
        assert cout in ODD_COUTS and log == {} and np.all(got == 7.0)
        return
    assert log == {route: 1}
    if f32:
        want = ref_conv(x, wgt, b, stride, None, out_f32=True, act=act).reshape(-1)
        body = got[GUARD:got.size - GUARD]
        frac = float((np.abs(body.astype(np.float64) - want) / (1e-4 + 1e-4 * np.abs(want))).max())
        assert np.all(got[:GUARD] == 7.0) and np.all(got[got.size - GUARD:] == 7.0)
    else:
        want = ref_conv(x, wgt, b, stride, None, residual16=r, act=act)
        frac = bar_fraction(got[..., 4:4 + cout], want)
        assert np.all(got[..., :4] == 7.0) and np.all(got[..., 4 + cout:] == 7.0)  # neighbours untouched, bit for bit
    print(f"{route} {_epilogue_id(item)}: worst error {frac:.3f} of the bar")
    assert frac <= 1.0


# ---- steady state of the persistent kernels ----------------------------------------------------------------------------
# (h, w, cin, cout, k, stride, route, tiles per frame, cout tiles, workgroups per CU the launcher starts at most).  n makes
# every workgroup of the largest grid walk >= 3 tiles: the double-buffered prefetch fills, reaches its steady state and
# drains.
STEADY = [
    (8, 16, 40, 1, 3, 1, "persist<NF1,S1,NCH2,DB1,POST0,NWV4>", 1, 1, 4),
    (8, 16, 72, 16, 3, 1, "persist<NF1,S1,NCH3,DB0,POST0,NWV4>", 1, 1, 4),
    (9, 32, 72, 80, 3, 1, "persist<NF3,S1,NCH3,DB0,POST0,NWV8>", 2, 2, 4),  # 16 x 16 tiles
    (16, 32, 8, 16, 3, 2, "c8<NF1,S2,SRC0>", 1, 1, 6),
    (8, 16, 24, 32, 1, 1, "1x1<NF2,UP0,NWV4,CLSMAX0>", 1, 1, 4),  # a "tile": the 4 x 32 pixels of one workgroup step
]


@pytest.mark.parametrize("h,w,cin,cout,k,stride,route,frame_tiles,ntiles,per_cu", STEADY, ids=[s[6] for s in STEADY])
def test_persistent_workgroups_walk_three_tiles_and_more(gpu, h, w, cin, cout, k, stride, route, frame_tiles, ntiles, per_cu):
    import torch
    import torch.nn.functional as F

    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    n = -(-3 * (per_cu * cus // ntiles) // frame_tiles)
    n += n % 2
    gen = torch.Generator(device=gpu).manual_seed(cin + cout)
    x = torch.randn((n, h, w, cin), generator=gen, device=gpu, dtype=torch.float32).half()
    rng = np.random.default_rng(cin)
    wgt = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
    b = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    ops.conv_routes(reset=True)
    got = ops.conv2d_f16(x, wgt, b, stride=stride, silu=True)
    assert ops.conv_routes(reset=True) == {route: 1}
    halves = torch.cat([ops.conv2d_f16(x[i:i + n // 2].contiguous(), wgt, b, stride=stride, silu=True) for i in (0, n // 2)])
    assert torch.equal(got.view(torch.int16), halves.view(torch.int16))
    # fp32 on the CPU (float64 is too slow at this size): its own rounding, ~1e-6 relative, is far inside the bar
    y = F.conv2d(x.cpu().float().permute(0, 3, 1, 2), torch.from_numpy(wgt.astype(np.float16).astype(np.float32)),
                 torch.from_numpy(b), stride=stride, padding=k // 2)
    want = (y * torch.sigmoid(y)).permute(0, 2, 3, 1).half().numpy()
    frac = bar_fraction(got.cpu().numpy(), want)
    print(f"{route} n={n}: worst error {frac:.3f} of the bar")
    assert frac <= 1.0


# ---- the sweep: nothing reachable is left without a parity case -------------------------------------------------------
SWEEP_CIN = (8, 16, 40, 72, 104, 144, 1152)
SWEEP_COUT = (1, 16, 32, 48, 64, 80, 96, 128, 192)
SWEEP_KS = ((1, 1), (3, 1), (3, 2))
SWEEP_HO_WO = [(ho, wo) for ho in (8, 9) for wo in (8, 24, 25, 48, 49, 80)] + [(1, 1)]


def sweep_routes(gpu):
    """route -> layers, of a grid of tiny zero-weight layers (no reference: only where they run)"""
    import torch

    seen = {}
    for cin in SWEEP_CIN:
        for cout in SWEEP_COUT:
            for (k, stride) in SWEEP_KS:
                wgt = np.zeros((cout, cin, k, k), np.float32)
                for (ho, wo) in SWEEP_HO_WO:
                    h, w = (ho, wo) if stride == 1 else (2 * ho - 1, 2 * wo)
                    x = torch.zeros((2, h, w, cin), dtype=torch.float16, device=gpu)
                    ops.conv_routes(reset=True)
                    ops.conv2d_f16(x, wgt, None, stride=stride, silu=False)
                    log = ops.conv_routes(reset=True)
                    assert len(log) == 1 and set(log.values()) == {1}, log
                    seen.setdefault(next(iter(log)), []).append((2, h, w, cin, cout, k, stride))
    return seen


def test_every_route_the_sweep_reaches_has_a_parity_case(gpu):
    seen = sweep_routes(gpu)
    missing = {r: v[0] for r, v in seen.items() if r not in ROUTE_CASES}
    assert not missing, f"instantiations with no single-layer parity case (route: first layer that reached it): {missing}"
    # and the table names nothing the sweep cannot reach: the two sets are the same ("Conv routes and what
    # tests them", gives the number)
    assert set(ROUTE_CASES) == set(seen), sorted(set(ROUTE_CASES) - set(seen))
    print(f"{len(seen)} routes over {sum(len(v) for v in seen.values())} layers")


def test_conv_slices_residual_and_fp32_out(gpu):
    """Concat-slice addressing: read channels [16,48) of a 64-wide buffer, write at offset 8 of a
    48-wide buffer with a residual taken from channels [32,64) of a third buffer."""
    import torch

    rng = np.random.default_rng(11)
    n, h, w = 2, 17, 23
    xbuf = rng.standard_normal((n, h, w, 64)).astype(np.float16)
    rbuf = rng.standard_normal((n, h, w, 64)).astype(np.float16)
    wgt = (rng.standard_normal((32, 32, 3, 3)) / 17.0).astype(np.float32)
    b = (0.1 * rng.standard_normal(32)).astype(np.float32)
    out = torch.full((n, h, w, 48), 7.0, dtype=torch.float16, device=gpu)
    ops.conv2d_f16(torch.from_numpy(xbuf).to(gpu), wgt, b, in_coff=16, cin=32, residual=torch.from_numpy(rbuf).to(gpu),
                   res_coff=32, out=out, out_coff=8)
    got = out.cpu().numpy()
    want = ref_conv(xbuf[..., 16:48], wgt, b, 1, True, residual16=rbuf[..., 32:64])
    assert close(got[..., 8:40], want)
    assert np.all(got[..., :8] == 7.0) and np.all(got[..., 40:] == 7.0)  # neighbours untouched
    # fp32 output, no activation (Detect's last 1x1)
    w1 = (rng.standard_normal((80, 64, 1, 1)) / 8.0).astype(np.float32)
    got32 = ops.conv2d_f16(torch.from_numpy(xbuf).to(gpu), w1, None, silu=False, out_f32=True).cpu().numpy()
    want32 = ref_conv(xbuf, w1, None, 1, False, out_f32=True)
    assert np.allclose(got32, want32, rtol=1e-4, atol=1e-4)


def test_conv_ignores_nan_outside_slice(gpu):
    """Channels outside the input slice (and the zero-padded chunk tail) must never leak in."""
    import torch

    rng = np.random.default_rng(12)
    x = rng.standard_normal((1, 8, 16, 24)).astype(np.float16)
    x[..., 16:] = np.nan
    wgt = (rng.standard_normal((16, 16, 3, 3)) / 12.0).astype(np.float32)
    got = ops.conv2d_f16(torch.from_numpy(x).to(gpu), wgt, None, cin=16).cpu().numpy()
    assert np.isfinite(got).all()
    assert close(got, ref_conv(x[..., :16], wgt, None, 1, True))


def test_conv_rejects_bad_shapes(gpu):
    import torch
    from eioku_amd._lib import EiokuHipError

    x = torch.zeros((1, 8, 8, 12), dtype=torch.float16, device=gpu)
    with pytest.raises(EiokuHipError):
        ops.conv2d_f16(x, np.zeros((16, 12, 3, 3), np.float32), None)  # cin % 8 != 0
    x = torch.zeros((1, 8, 8, 16), dtype=torch.float16, device=gpu)
    with pytest.raises(EiokuHipError):
        ops.conv2d_f16(x, np.zeros((16, 16, 5, 5), np.float32), None)  # k=5
