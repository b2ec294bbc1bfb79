"""ctypes loader of flx_rays_planes_gather's CPU reference (tests/rays_planes_gather_ref/flx_rays_planes_gather_ref.c).  TEST INFRASTRUCTURE ONLY.

build(out_dir) compiles it with gcc and the oracle Makefile's flags into out_dir (outside git), as its siblings are built: the file includes
tests/rays_gather_ref/flx_rays_gather_ref.c, which includes oracle/flx_oracle.c and include/flx_gather.h, and is linked with oracle/flx_oracle_filter.c;
-Wl,-Bsymbolic keeps its copy of their exported names to itself."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from flexlight_hip.scene_io import FrameParams, SceneView

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ORACLE = os.path.join(ROOT, "oracle")
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "rays_planes_ref"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "rays_gather_ref"))
from flx_rays_gather_ref import RefVolume  # noqa: E402
from flx_rays_planes_ref import CFLAGS, frame_params_of, quant  # noqa: E402,F401

LIT, CONSTANT, NO_POINT = 1, 2, 3          # a sample's class: A = E * gain; a last point but W not > 0; the sample shaded nothing
PLANES, TEMPORAL_CANVAS, TEMPORAL_FILTER = 0, 1, 2


def build(out_dir):
    """-> a RaysPlanesGatherRef over the library built in out_dir"""
    so = os.path.join(out_dir, "libflx_rays_planes_gather_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-I", os.path.join(ROOT, "include"), "-I", ORACLE, "-shared", "-Wl,-Bsymbolic", "-o", so,
                                              os.path.join(HERE, "flx_rays_planes_gather_ref.c"), os.path.join(ORACLE, "flx_oracle_filter.c")])
    return RaysPlanesGatherRef(so)


class RaysPlanesGatherRef:
    def __init__(self, so):
        lib = C.CDLL(so)
        fp, u8 = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        lib.flx_rays_planes_gather_ref.argtypes = [C.POINTER(SceneView), C.POINTER(FrameParams), C.POINTER(RefVolume), fp, fp, u8, fp, u8, C.c_uint32, C.c_int, C.c_int]
        lib.flx_rays_planes_gather_ref.restype = C.c_int
        self.lib = lib

    def planes(self, scene, trace_params, rays, grid, sh, gain, vmap=None, maps=None, offsets=None, mode=PLANES, details=False, threads=0):
        """scene: a scene_io.Scene or a SceneView; trace_params: capi.TraceParams; rays [n, 8] float32; grid: VolumeGrid; sh float32 [probes, 36]; vmap and maps float32
        [probes * bins, 4] or neither; offsets float32 [probes, 4] or None -> (float planes float32 [5, n, 4] in flx_render_planes_device's order — [6, n, 4] with the
        location id in a temporal mode —, hit bool [n]); with details=True also (c before fract float32 [n, 3], the class of every sample uint8 [n, samples])"""
        view = scene.view() if hasattr(scene, "view") else scene
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n, samples = rays.shape[0], int(trace_params.samples)
        fp, u8 = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        sh = np.ascontiguousarray(sh, np.float32).reshape(-1, 36)
        assert sh.shape[0] == grid.probes and (vmap is None) == (maps is None)
        v = RefVolume()
        v.grid, v.sh, v.gain = C.pointer(grid), sh.ctypes.data_as(fp), gain
        if vmap is not None:
            maps = np.ascontiguousarray(maps, np.float32).reshape(-1, 4)
            assert maps.shape[0] == grid.probes * vmap.bins
            v.map, v.maps = C.pointer(vmap), maps.ctypes.data_as(fp)
        if offsets is not None:
            offsets = np.ascontiguousarray(offsets, np.float32).reshape(-1, 4)
            assert offsets.shape[0] == grid.probes
            v.offsets = offsets.ctypes.data_as(fp)
        out = np.zeros((6 if mode else 5, n, 4), np.float32)
        hit = np.zeros(n, np.uint8)
        colour = np.zeros((n, 3), np.float32)
        classes = np.zeros((n, samples), np.uint8)
        params = frame_params_of(trace_params)
        rc = self.lib.flx_rays_planes_gather_ref(C.byref(view), C.byref(params), C.byref(v), rays.ctypes.data_as(fp), out.ctypes.data_as(fp), hit.ctypes.data_as(u8),
                                                 colour.ctypes.data_as(fp), classes.ctypes.data_as(u8), n, int(mode), threads)
        if rc != 0:
            raise RuntimeError("flx_rays_planes_gather_ref failed: %d" % rc)
        return (out, hit.astype(bool), colour, classes) if details else (out, hit.astype(bool))
