"""CPU-side checks of the frame loop's flags (FLX_FRAME_FXAA / FLX_FRAME_TAA / FLX_FRAME_RASTERIZER, OR'ed into flx_frame_begin's format): the
header declares them with their values, the ctypes binding exposes the same values and builds the format from its keywords, the boundary gained
no function — and the RGBA8 word k_raster stores equals k_quantize of the float frame for every byte value, which is what lets the byte variant
stand in for the float frame and the quantize pass."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "flexlight_hip.h")


def macros():
    text = open(HEADER).read()
    return {m.group(1): int(m.group(2), 0) for m in re.finditer(r"^#define\s+(FLX_FRAME_[A-Z0-9_]+)\s+(0x[0-9a-fA-F]+|\d+)\b", text, flags=re.M)}


def test_header_declares_the_flags():
    m = macros()
    assert m["FLX_FRAME_FLOAT"] == 0 and m["FLX_FRAME_RGBA8"] == 1 and m["FLX_FRAME_DEVICE"] == 2
    assert m["FLX_FRAME_FXAA"] == 0x10 and m["FLX_FRAME_TAA"] == 0x20 and m["FLX_FRAME_RASTERIZER"] == 0x100
    for flag in ("FLX_FRAME_FXAA", "FLX_FRAME_TAA", "FLX_FRAME_RASTERIZER"):       # flags stay clear of the format values and of each other
        assert m[flag] & 0x0f == 0 and bin(m[flag]).count("1") == 1


def test_capi_exposes_the_flags():
    from flexlight_hip import capi
    m = macros()
    assert (capi.FRAME_FXAA, capi.FRAME_TAA, capi.FRAME_RASTERIZER) == (m["FLX_FRAME_FXAA"], m["FLX_FRAME_TAA"], m["FLX_FRAME_RASTERIZER"])


def test_the_boundary_gained_no_function():
    from test_capi_cpu import declared_functions
    assert len(declared_functions(headers=("flexlight_hip.h",))) == 80


def test_capi_frame_begin_builds_the_format():
    """the keywords -> the format word handed to flx_frame_begin (the library itself is not called: a stand-in records the word)"""
    from flexlight_hip import capi

    class Rec:
        def __init__(self):
            self.fmt = []

        def flx_frame_begin(self, h, p, fmt):
            self.fmt.append(fmt)
            return 0

    ctx = capi.Context.__new__(capi.Context)
    ctx._h, ctx._pending = None, []
    ctx.tile_row_count = lambda p: 1
    rec, lib = Rec(), capi.LIB
    capi.LIB = rec
    try:
        p = capi.FrameParams()
        p.width = 1
        ctx.frame_begin(p)
        ctx.frame_begin(p, rgba8=True, antialiasing="fxaa")
        ctx.frame_begin(p, device=True, rasterizer=True, antialiasing="taa")
        ctx.frame_begin(p, rasterizer=True)
        with pytest.raises(ValueError):
            ctx.frame_begin(p, antialiasing="msaa")
    finally:
        capi.LIB = lib
    assert rec.fmt == [0, 1 | 0x10, 2 | 0x100 | 0x20, 0x100]


def quant_unorm8(x):
    """flx_kernel_util.h quant_unorm8 in float32: floor(clamp(x, 0, 1) * 255 + 0.5), NaN -> 0 (IEEE single rounding at every step)"""
    x = np.float32(x)
    if not (x > np.float32(0)):
        return 0
    if x >= np.float32(1):
        return 255
    return int(np.float32(np.float32(x * np.float32(255)) + np.float32(0.5)))


def test_every_byte_survives_the_quantize_of_its_float():
    """k_raster keeps each channel as Q(x) = k / 255 in float32 (rasterQ); the byte variant stores pack_rgba8 of that value.  That is k itself — and
    so what k_quantize stores for the float frame — for all 256 k"""
    for k in range(256):
        v = np.float32(np.float32(k) / np.float32(255))
        assert quant_unorm8(v) == k, k
