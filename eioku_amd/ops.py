"""Thin wrappers over single-kernel C-ABI entry points (building blocks; used by the parity tests)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._buffers import current_stream, ptr


def conv2d_f16(x_nhwc, weight_oihw: np.ndarray, bias: np.ndarray | None, *, stride: int = 1, silu: bool = True,
               in_coff: int = 0, cin: int | None = None, residual=None, res_coff: int = 0,
               out=None, out_coff: int = 0, out_f32=False, act: int | None = None):
    """K4: one NHWC fp16 convolution (k in {1,3}, pad k//2) with fused bias/SiLU/residual.

    ``x_nhwc``: CUDA fp16 tensor (n,h,w,C); the conv reads channels [in_coff, in_coff+cin).
    ``out``: optional preallocated CUDA fp16 tensor (n,ho,wo,C_out_total) written at ``out_coff``.
    ``out_f32``: True, or a preallocated dense CUDA fp32 tensor (n,ho,wo,cout), for the fp32 output.
    ``act``: the C ABI's activation code (0 none, 1 SiLU, 2 ReLU, 3 ReLU after the residual sum); default: ``silu``.
    """
    import torch

    lib = _lib.load()
    _lib.init()
    n, h, w, ctot = (int(s) for s in x_nhwc.shape)
    cout, cin_w, k, _ = weight_oihw.shape
    cin = cin_w if cin is None else cin
    assert cin == cin_w
    w32 = np.ascontiguousarray(weight_oihw, dtype=np.float32)
    b32 = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    ho = (h + 2 * (k // 2) - k) // stride + 1
    wo = (w + 2 * (k // 2) - k) // stride + 1
    o32 = None
    if out_f32 is True:
        o32 = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=x_nhwc.device)
    elif out_f32 is not False:
        o32 = out_f32
        assert o32.dtype == torch.float32 and tuple(o32.shape) == (n, ho, wo, cout) and o32.is_contiguous()
    elif out is None:
        out = torch.empty((n, ho, wo, cout), dtype=torch.float16, device=x_nhwc.device)
    _lib.check(lib.eioku_conv2d_f16(ptr(x_nhwc), n, h, w, ctot, in_coff, cin, ptr(w32), ptr(b32), cout, k, stride,
                                    int(silu) if act is None else int(act), ptr(residual), 0 if residual is None else int(residual.shape[-1]),
                                    res_coff, ptr(out), 0 if out is None else int(out.shape[-1]), out_coff,
                                    ptr(o32), current_stream(x_nhwc)), "eioku_conv2d_f16")
    return o32 if o32 is not None else out


def conv_routes(reset: bool = False) -> dict[str, int]:
    """Route log of the conv family: {instantiation name: launches} in this process since the last reset, as counted
    by the launch code itself (``eioku_debug_conv_routes``), e.g. ``{"persist<NF3,S1,NCH3,DB0,POST0,NWV8>": 4}``."""
    buf = C.create_string_buffer(1 << 16)
    _lib.check(_lib.load().eioku_debug_conv_routes(buf, len(buf), int(reset)), "eioku_debug_conv_routes")
    routes = {}
    for line in buf.value.decode().splitlines():
        name, count = line.rsplit(" ", 1)
        routes[name] = int(count)
    return routes


def conv_plan(n: int, h: int, w: int, cin: int, cout: int, k: int, stride: int, *, residual: bool = False,
              out_f32: bool = False) -> tuple[str, int]:
    """(route, dynamic LDS bytes) ``conv2d_f16`` would launch for a dense layer of this shape, decided on the host
    (``eioku_debug_conv_plan``): no launch, no device.  Raises ``EiokuHipError`` where ``conv2d_f16`` would."""
    buf = C.create_string_buffer(160)
    lds = C.c_size_t(0)
    _lib.check(_lib.load().eioku_debug_conv_plan(n, h, w, cin, cout, k, stride, int(residual), int(out_f32), buf, len(buf),
                                                 C.byref(lds)), "eioku_debug_conv_plan")
    return buf.value.decode(), lds.value


def conv_epi_launches(reset: bool = False) -> int:
    """Launches of k_conv3x3_flat in this process since the last reset that took the straight-line epilogue on at least
    their first cout tile (``eioku_debug_conv_epi``); 0 with ``EIOKU_CONV_EPI=0``."""
    n = C.c_int(0)
    _lib.check(_lib.load().eioku_debug_conv_epi(C.byref(n), int(reset)), "eioku_debug_conv_epi")
    return n.value
