"""The conv family's plan -- which kernel instantiation a layer runs on, decided on the host before anything is launched
(csrc/conv_plan.h, read through ``ops.conv_plan``) -- names, for every single-layer case of tests/test_conv_gpu.py, the
route that file's table gives.  The table is what the launch code's own log reports on the GPU, so this proves without a
device that no shape moved to another instantiation.  (No GPU.)"""
import pytest

from eioku_amd import ops
from eioku_amd._lib import EiokuHipError
from test_conv_gpu import EPILOGUE_CASES, LDS_STEPS, ROUTE_CASES, ROUTE_OF


def test_the_plan_names_the_route_of_every_parity_case(built_lib):
    moved = {case: (ops.conv_plan(*case)[0], route) for case, route in ROUTE_OF.items() if ops.conv_plan(*case)[0] != route}
    assert not moved, f"(planned, expected) per layer: {moved}"
    assert len(ROUTE_OF) == sum(len(v) for v in ROUTE_CASES.values())


def test_the_plan_names_the_route_of_every_epilogue_case(built_lib):
    """residuals, fp32 outputs and ragged couts: the flags the plan sees beside the shape"""
    for case, act, res, f32, route in EPILOGUE_CASES:
        assert ops.conv_plan(*case, residual=res, out_f32=f32)[0] == route, (case, res, f32)


def test_lds_bytes_are_the_layouts(built_lib):
    """spot values worked out by hand from the kernels' carve-ups (16-byte units)"""
    # 1x1: the whole weight tile, nchunks x 16 nf rows x 4 units
    assert ops.conv_plan(1, 7, 9, 40, 48, 1, 1) == ("1x1<NF3,UP0,NWV4,CLSMAX0>", 2 * 48 * 4 * 16)
    assert ops.conv_plan(1, 7, 9, 1152, 576, 1, 1) == ("1x1<NF3,UP0,NWV4,CLSMAX0>", 36 * 48 * 4 * 16)
    # persist, 8 waves: 3 chunks of 9 x 48 x 4 weights, one 18 x 18 patch per chunk, one spare unit
    assert ops.conv_plan(2, 17, 33, 72, 80, 3, 1) == ("persist<NF3,S1,NCH3,DB0,POST0,NWV8>", (3 * 1728 + 3 * 18 * 18 * 4 + 1) * 16)
    # igemm at stride 2: a 17 x 33 patch in rows of 2 x 17 pixels, 4 spare units, one chunk of 9 x 64 x 4 weights
    assert ops.conv_plan(2, 2, 2, 128, 64, 3, 2) == ("igemm<NF4,K3,S2>", (17 * 34 * 4 + 4 + 2304) * 16)
    # c8: 3 k-steps of 16 x 4 weights, two buffers of 17 x 34 + 1 one-unit pixels
    assert ops.conv_plan(2, 64, 64, 8, 16, 3, 2) == ("c8<NF1,S2,SRC0>", (3 * 64 + 2 * (17 * 34 + 1)) * 16)
    for route, small, large in LDS_STEPS:
        assert ops.conv_plan(*small)[1] <= 64 * 1024 < ops.conv_plan(*large)[1]


@pytest.mark.parametrize("args,what", [
    ((1, 8, 8, 16, 16, 5, 1), "kernel size 5"),       # no 5x5 kernel
    ((1, 8, 8, 16, 16, 1, 2), "stride 2 with k=1"),   # a strided 1x1 runs as a centre-tap 3x3, never as a 1x1
    ((1, 8, 8, 12, 16, 3, 1), "cin 12"),              # channels in 16-byte units
    ((1 << 15, 256, 256, 8, 16, 3, 2), "32-bit"),     # a tensor past the kernels' 32-bit element offsets
])
def test_a_shape_no_kernel_runs_is_an_error_not_a_route(built_lib, args, what):
    with pytest.raises(EiokuHipError, match=what):
        ops.conv_plan(*args)
