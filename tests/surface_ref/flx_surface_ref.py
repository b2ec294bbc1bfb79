"""ctypes loader of the surface rows' CPU reference (tests/surface_ref/flx_surface_ref.c).  TEST INFRASTRUCTURE ONLY.

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
PLANES = 8


def build(out_dir):
    """-> a SurfaceRef over the library built in out_dir"""
    so = os.path.join(out_dir, "libflx_surface_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-I", os.path.join(ROOT, "include"), "-I", ORACLE, "-shared", "-Wl,-Bsymbolic", "-o", so,
                                              os.path.join(HERE, "flx_surface_ref.c"), os.path.join(ORACLE, "flx_oracle_filter.c")])
    return SurfaceRef(so)


class SurfaceRef:
    def __init__(self, so):
        lib = C.CDLL(so)
        lib.flx_surface_ref_rays.argtypes = [C.POINTER(SceneView), C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32]
        lib.flx_surface_ref_rays.restype = C.c_int
        lib.flx_surface_ref_frame.argtypes = [C.POINTER(SceneView), C.POINTER(FrameParams), C.POINTER(C.c_float)]
        lib.flx_surface_ref_frame.restype = C.c_int
        self.lib = lib

    def rays(self, scene, rays, texture_width):
        """scene: a scene_io.Scene or a SceneView; rays [n, 8] float32 -> all eight planes as words, uint32 [8, n, 4]"""
        view = scene.view() if hasattr(scene, "view") else scene
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros((PLANES, rays.shape[0], 4), np.float32)
        rc = self.lib.flx_surface_ref_rays(C.byref(view), int(texture_width), rays.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)),
                                           rays.shape[0])
        if rc != 0:
            raise RuntimeError("flx_surface_ref_rays failed: %d" % rc)
        return out.view(np.uint32)

    def frame(self, scene, params):
        """the frame of params -> all eight planes as words, uint32 [8, width * height, 4], row k = pixel k with row 0 on top"""
        view = scene.view() if hasattr(scene, "view") else scene
        out = np.zeros((PLANES, params.width * params.height, 4), np.float32)
        rc = self.lib.flx_surface_ref_frame(C.byref(view), C.byref(params), out.ctypes.data_as(C.POINTER(C.c_float)))
        if rc != 0:
            raise RuntimeError("flx_surface_ref_frame failed: %d" % rc)
        return out.view(np.uint32)
