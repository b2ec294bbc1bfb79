"""ctypes loader of flx_rays_trace's CPU reference (tests/rays_trace_ref/flx_rays_trace_ref.c).  TEST INFRASTRUCTURE ONLY.

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
    """-> a RaysTraceRef over the library built in out_dir"""
    so = os.path.join(out_dir, "libflx_rays_trace_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-I", os.path.join(ROOT, "include"), "-I", ORACLE, "-shared", "-Wl,-Bsymbolic", "-o", so,
                                              os.path.join(HERE, "flx_rays_trace_ref.c"), os.path.join(ORACLE, "flx_oracle_filter.c")])
    return RaysTraceRef(so)


def frame_params_of(trace_params):
    """a FrameParams that holds a TraceParams' fields (the reference reads no other)"""
    p = FrameParams()
    p.width = p.height = 1
    p.samples, p.max_reflections, p.min_importancy = trace_params.samples, trace_params.max_reflections, trace_params.min_importancy
    p.ambient[:] = trace_params.ambient[:]
    p.random_seed, p.texture_width = trace_params.random_seed, trace_params.texture_width
    return p


class RaysTraceRef:
    def __init__(self, so):
        lib = C.CDLL(so)
        lib.flx_rays_trace_ref.argtypes = [C.POINTER(SceneView), C.POINTER(FrameParams), C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_uint32, C.c_int]
        lib.flx_rays_trace_ref.restype = C.c_int
        self.lib = lib

    def trace(self, scene, trace_params, rays, threads=0):
        """scene: a scene_io.Scene or a SceneView; trace_params: capi.TraceParams; rays [n, 8] float32 -> radiance rows as words, uint32 [n, 8]"""
        view = scene.view() if hasattr(scene, "view") else scene
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros((rays.shape[0], 8), np.uint32)
        fp = frame_params_of(trace_params)
        rc = self.lib.flx_rays_trace_ref(C.byref(view), C.byref(fp), rays.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_uint32)),
                                         rays.shape[0], threads)
        if rc != 0:
            raise RuntimeError("flx_rays_trace_ref failed: %d" % rc)
        return out
