"""ctypes loader of flx_rays_trace_gather's CPU reference (tests/rays_gather_ref/flx_rays_gather_ref.c).  TEST INFRASTRUCTURE ONLY.

build(out_dir) compiles it with gcc and the oracle Makefile's flags into out_dir (outside git), as tests/rays_trace_ref is built: the file includes
oracle/flx_oracle.c and include/flx_gather.h and is linked with oracle/flx_oracle_filter.c; -Wl,-Bsymbolic keeps its copy of the oracle's exported names to itself."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from flexlight_hip.capi import VolumeGrid, VolumeMap
from flexlight_hip.scene_io import FrameParams, SceneView

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ORACLE = os.path.join(ROOT, "oracle")
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "rays_trace_ref"))
from flx_rays_trace_ref import CFLAGS, frame_params_of  # noqa: E402


class RefVolume(C.Structure):
    """flx_gather_ref_volume of the reference: the grid, the SH rows, the map and its rows (or NULL), the offset rows (or NULL), the gain"""
    _fields_ = [("grid", C.POINTER(VolumeGrid)), ("sh", C.POINTER(C.c_float)), ("map", C.POINTER(VolumeMap)), ("maps", C.POINTER(C.c_float)),
                ("offsets", C.POINTER(C.c_float)), ("gain", C.c_float)]


def build(out_dir):
    """-> a RaysGatherRef over the library built in out_dir"""
    so = os.path.join(out_dir, "libflx_rays_gather_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-I", os.path.join(ROOT, "include"), "-I", ORACLE, "-shared", "-Wl,-Bsymbolic", "-o", so,
                                              os.path.join(HERE, "flx_rays_gather_ref.c"), os.path.join(ORACLE, "flx_oracle_filter.c")])
    return RaysGatherRef(so)


class RaysGatherRef:
    def __init__(self, so):
        lib = C.CDLL(so)
        fp = C.POINTER(C.c_float)
        lib.flx_rays_gather_ref.argtypes = [C.POINTER(SceneView), C.POINTER(FrameParams), C.POINTER(RefVolume), fp, C.POINTER(C.c_uint32), fp, fp, C.c_uint32, C.c_int]
        lib.flx_rays_gather_ref.restype = C.c_int
        self.lib = lib

    def gather(self, scene, trace_params, rays, grid, sh, gain, vmap=None, maps=None, offsets=None, records=False, threads=0):
        """scene: a scene_io.Scene or a SceneView; trace_params: capi.TraceParams; rays [n, 8] float32; grid: VolumeGrid; sh float32 [probes, 36]; vmap and maps
        float32 [probes * bins, 4] or neither; offsets float32 [probes, 4] or None -> radiance rows as words, uint32 [n, 8]; with records=True -> (rows, path records
        float32 [n, samples, 16]: finalColor, importancyFactor, x + whether there is a last point, n; lookups float32 [n, samples, 4]: the E of every path)"""
        view = scene.view() if hasattr(scene, "view") else scene
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n, samples = rays.shape[0], int(trace_params.samples)
        fp = C.POINTER(C.c_float)
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
        out = np.zeros((n, 8), np.uint32)
        rec = np.zeros((n, samples, 16), np.float32) if records else None
        look = np.zeros((n, samples, 4), np.float32) if records else None
        params = frame_params_of(trace_params)
        rc = self.lib.flx_rays_gather_ref(C.byref(view), C.byref(params), C.byref(v), rays.ctypes.data_as(fp), out.ctypes.data_as(C.POINTER(C.c_uint32)),
                                          rec.ctypes.data_as(fp) if records else None, look.ctypes.data_as(fp) if records else None, n, threads)
        if rc != 0:
            raise RuntimeError("flx_rays_gather_ref failed: %d" % rc)
        return (out, rec, look) if records else out
