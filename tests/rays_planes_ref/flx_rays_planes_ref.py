"""ctypes loader of flx_rays_planes' CPU reference (tests/rays_planes_ref/flx_rays_planes_ref.c).  TEST INFRASTRUCTURE ONLY.

build(out_dir) compiles it with gcc and the oracle Makefile's flags into out_dir (outside git).  The file includes oracle/flx_oracle.c and is linked with
oracle/flx_oracle_filter.c, so it needs no libflx_oracle.so; -Wl,-Bsymbolic keeps its copy of the oracle's exported names to itself where both are loaded."""
import ctypes as C
import os
import subprocess

import numpy as np

from flexlight_hip.scene_io import FrameParams, SceneView

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ORACLE = os.path.join(ROOT, "oracle")
CFLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-comment"]


def build(out_dir):
    """-> a RaysPlanesRef over the library built in out_dir"""
    so = os.path.join(out_dir, "libflx_rays_planes_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-I", os.path.join(ROOT, "include"), "-I", ORACLE, "-shared", "-Wl,-Bsymbolic", "-o", so,
                                              os.path.join(HERE, "flx_rays_planes_ref.c"), os.path.join(ORACLE, "flx_oracle_filter.c")])
    return RaysPlanesRef(so)


def frame_params_of(trace_params):
    """a FrameParams that holds a TraceParams' fields (the reference reads no other)"""
    p = FrameParams()
    p.width = p.height = 1
    p.samples, p.max_reflections, p.min_importancy = trace_params.samples, trace_params.max_reflections, trace_params.min_importancy
    p.ambient[:] = trace_params.ambient[:]
    p.random_seed, p.texture_width = trace_params.random_seed, trace_params.texture_width
    return p


def quant(planes):
    """float32 [..., 4] -> uint32 [...]: the RGBA8 texel a render target stores of each value, the oracle's `quant` per channel in float32 arithmetic — NaN and
    values <= 0 give 0, values >= 1 give 255, otherwise (uint8)(x * 255 + 0.5f) — r in the low byte"""
    x = np.ascontiguousarray(planes, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        inside = (x > np.float32(0.0)) & (x < np.float32(1.0))
        product = (np.where(inside, x, np.float32(0.0)) * np.float32(255.0)).astype(np.float32)
        q = (product + np.float32(0.5)).astype(np.float32).astype(np.uint32)
        q = np.where(x >= np.float32(1.0), np.uint32(255), np.where(inside, q, np.uint32(0))).astype(np.uint32)
    return q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | (q[..., 3] << 24)


class RaysPlanesRef:
    def __init__(self, so):
        lib = C.CDLL(so)
        lib.flx_rays_planes_ref.argtypes = [C.POINTER(SceneView), C.POINTER(FrameParams), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.c_uint32,
                                            C.c_int]
        lib.flx_rays_planes_ref.restype = C.c_int
        self.lib = lib

    def planes(self, scene, trace_params, rays, threads=0):
        """scene: a scene_io.Scene or a SceneView; trace_params: capi.TraceParams; rays [n, 8] float32 -> (the five float planes float32 [5, n, 4] in
        flx_render_planes_device's order, hit bool [n])"""
        view = scene.view() if hasattr(scene, "view") else scene
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n = rays.shape[0]
        out = np.zeros((5, n, 4), np.float32)
        hit = np.zeros(n, np.uint8)
        fp = frame_params_of(trace_params)
        rc = self.lib.flx_rays_planes_ref(C.byref(view), C.byref(fp), rays.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)),
                                          hit.ctypes.data_as(C.POINTER(C.c_uint8)), n, threads)
        if rc != 0:
            raise RuntimeError("flx_rays_planes_ref failed: %d" % rc)
        return out, hit.astype(bool)
