"""Helpers of the ray-planes tests (test_rays_planes_cpu.py, test_rays_planes_gpu.py, test_rays_planes_js_gpu.py): the CPU reference built once per session and its
planes computed once per key, the oracle's denoise chain over float planes, and the comparison of planes.  The rays are rays_trace_util's."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "rays_planes_ref"))
import flx_rays_planes_ref  # noqa: E402
from flx_rays_planes_ref import quant  # noqa: E402,F401

PLANES = ("color", "color_ip", "original_color", "id", "original_id")      # flx_render_planes_device's order

_ref = []
_want = {}
_chain = {}


def reference(tmp_path_factory):
    """the CPU reference, built once per session"""
    if not _ref:
        _ref.append(flx_rays_planes_ref.build(str(tmp_path_factory.mktemp("rays_planes_ref"))))
    return _ref[0]


def wanted(ref, key, sc, t, rays):
    """the reference's (float planes [5, n, 4], hit [n]), computed once per key and left unchanged"""
    if key not in _want:
        planes, hit = ref.planes(sc, t, rays)
        planes.setflags(write=False)
        hit.setflags(write=False)
        _want[key] = (planes, hit)
    return _want[key]


def oracle_chain(oracle, planes32, width, height, hdr, key=None):
    """flx_oracle_filter (the oracle library's own chain, which stores its inputs as RGBA8 itself) over float planes [5, width * height, 4] -> float32 [height, width, 4]"""
    if key is not None and (key, hdr) in _chain:
        return _chain[(key, hdr)]
    from flexlight_hip.scene_io import FrameParams, GBuffers
    p = FrameParams()
    p.width, p.height, p.samples, p.max_reflections, p.use_filter, p.hdr, p.texture_width = width, height, 1, 1, 1, int(hdr), 1
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    fl = [np.ascontiguousarray(planes32[k], np.float32).reshape(height, width, 4) for k in range(5)]
    gb = GBuffers(fp(fl[0]), fp(fl[1]), fp(fl[2]), fp(fl[3]), fp(fl[4]), None)
    out = np.zeros((height, width, 4), np.float32)
    assert oracle.lib().flx_oracle_filter(C.byref(p), C.byref(gb), fp(out), 0) == 0
    if key is not None:
        out.setflags(write=False)
        _chain[(key, hdr)] = out
    return out


def same_floats(got, want):
    """bool, elementwise: float32 against float32 bit for bit, a NaN equal to a NaN"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))


def assert_floats(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(~same_floats(got, want))
    assert bad.size == 0, "%s: %d of %d floats differ, first at %s: got %r want %r" % (what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def assert_texels(got, want, what=""):
    got, want = np.asarray(got).view(np.uint32), np.asarray(want).view(np.uint32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d of %d texels differ, first at %s: got %08x want %08x" % (what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
