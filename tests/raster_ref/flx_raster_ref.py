"""ctypes loader of the rasterizer's CPU reference (tests/raster_ref/flx_raster_ref.c).  TEST INFRASTRUCTURE ONLY.

build(out_dir) compiles it with gcc and the oracle's flags into out_dir and links it to oracle/libflx_oracle.so, whose exported
routines (shadowTest, forwardTrace, rayCuboid, pow) it calls; the oracle must be built first (the `oracle` fixture does that)."""
import ctypes as C
import os
import subprocess

import numpy as np

from flexlight_hip.scene_io import Counters, FrameParams, SceneView

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ORACLE = os.path.join(ROOT, "oracle")
CFLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-comment"]


def build(out_dir):
    """-> a RasterRef over the library built in out_dir"""
    so = os.path.join(out_dir, "libflx_raster_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-I", os.path.join(ROOT, "include"), "-I", ORACLE, "-shared", "-o", so,
                                              os.path.join(HERE, "flx_raster_ref.c"), "-L", ORACLE, "-lflx_oracle",
                                              "-Wl,-rpath," + ORACLE])
    return RasterRef(so)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class RasterRef:
    def __init__(self, so):
        lib = C.CDLL(so)
        fp = C.POINTER(C.c_float)
        lib.flx_raster_ref_render.argtypes = [C.POINTER(SceneView), C.POINTER(FrameParams), fp, C.POINTER(Counters), C.c_int]
        lib.flx_raster_ref_render.restype = C.c_int
        lib.flx_raster_ref_fragment.argtypes = [C.POINTER(SceneView), C.POINTER(FrameParams), C.c_int, C.c_int, fp, fp, C.POINTER(Counters)]
        lib.flx_raster_ref_fragment.restype = None
        lib.flx_raster_ref_blend.argtypes = [fp, fp]
        lib.flx_raster_ref_blend.restype = None
        lib.flx_raster_ref_fragments.argtypes = [C.POINTER(SceneView), C.POINTER(FrameParams), C.c_uint32, C.c_uint32, fp,
                                                 C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
        lib.flx_raster_ref_fragments.restype = C.c_int
        lib.flx_raster_ref_visits.argtypes = [C.POINTER(SceneView), C.POINTER(FrameParams), C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.c_int]
        lib.flx_raster_ref_visits.restype = C.c_int
        self.lib = lib

    def render(self, scene, params, threads=0):
        """scene: a scene_io.Scene or a SceneView -> (rgba [rows, W, 4] float32, counters dict)"""
        view = scene.view() if hasattr(scene, "view") else scene
        tr, tc, ti = params.tile_rows, params.tile_count, params.tile_index
        rows = params.height if (tr == 0 or tc <= 1) else sum(1 for y in range(params.height) if (y // tr) % tc == ti)
        out = np.zeros((rows, params.width, 4), np.float32)
        cnt = Counters()
        rc = self.lib.flx_raster_ref_render(C.byref(view), C.byref(params), _fp(out), C.byref(cnt), threads)
        if rc != 0:
            raise RuntimeError("flx_raster_ref_render failed: %d" % rc)
        return out, cnt.as_dict()

    def fragment(self, view, params, transform2, tri, suv):
        """main() of one fragment -> (renderColor float32[4], counters dict)"""
        out = np.zeros(4, np.float32)
        s = np.ascontiguousarray(suv, np.float32)
        cnt = Counters()
        self.lib.flx_raster_ref_fragment(C.byref(view), C.byref(params), int(transform2), int(tri), _fp(s), _fp(out), C.byref(cnt))
        return out, cnt.as_dict()

    def blend(self, src, dst):
        """one blend of renderColor src over the RGBA8 buffer's dst -> the new dst"""
        s = np.ascontiguousarray(src, np.float32)
        d = np.array(dst, np.float32)
        self.lib.flx_raster_ref_blend(_fp(s), _fp(d))
        return d

    def fragments(self, view, params, px, py_gl, cap=4096):
        """the fragments of a pixel that pass the depth test, in draw order: [(suv float32[3], 2 x transform, entry)]"""
        suv = np.zeros(3 * cap, np.float32)
        ti = (C.c_int * cap)()
        tri = (C.c_int * cap)()
        n = self.lib.flx_raster_ref_fragments(C.byref(view), C.byref(params), px, py_gl, _fp(suv), ti, tri, cap)
        return [(suv[3 * k:3 * k + 3].copy(), ti[k], tri[k]) for k in range(min(n, cap))]

    def visits(self, view, params, px, py_gl, cap=4096):
        """the entry indices that the pixel's walk fetches, in order, the terminator included"""
        out = (C.c_int * cap)()
        n = self.lib.flx_raster_ref_visits(C.byref(view), C.byref(params), px, py_gl, out, cap)
        assert n <= cap, n
        return list(out[:n])
