"""ctypes loader of the temporal ray images' CPU reference (tests/rays_temporal_ref/*.c) and the rings it runs over.  TEST INFRASTRUCTURE ONLY.

build(out_dir) compiles both files with gcc and the oracle Makefile's flags into one library in out_dir (outside git).  One includes oracle/flx_oracle.c, the other
oracle/flx_oracle_filter.c, so it needs no libflx_oracle.so; -Wl,-Bsymbolic keeps its copy of the oracle's exported names to itself where both are loaded.

A History holds the four rings in numpy, newest first, and is what flx_rays_image_temporal keeps on the device: frame() traces a frame's six planes with the
oracle's lightTrace, quantises them (flx_rays_planes_ref.quant), rotates the rings and runs the oracle's temporal_pass (and filter_chain_u8)."""
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
from flx_rays_planes_ref import CFLAGS, frame_params_of, quant  # noqa: E402


def build(out_dir):
    """-> a RaysTemporalRef over the library built in out_dir"""
    so = os.path.join(out_dir, "libflx_rays_temporal_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-I", os.path.join(ROOT, "include"), "-I", ORACLE, "-shared", "-Wl,-Bsymbolic", "-o", so,
                                              os.path.join(HERE, "flx_rays_temporal_ref.c"), os.path.join(HERE, "flx_rays_temporal_pass.c")])
    return RaysTemporalRef(so)


def depth_of(temporal_samples):
    """flx_frame_params' rule"""
    return 4 if temporal_samples <= 0 else min(16, temporal_samples)


class RaysTemporalRef:
    def __init__(self, so):
        lib = C.CDLL(so)
        lib.flx_rays_temporal_ref.argtypes = [C.POINTER(SceneView), C.POINTER(FrameParams), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.c_uint32,
                                              C.c_int]
        lib.flx_rays_temporal_ref.restype = C.c_int
        lib.flx_rays_temporal_pass_ref.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8),
                                                   C.POINTER(C.c_float), C.c_int]
        lib.flx_rays_temporal_pass_ref.restype = C.c_int
        self.lib = lib

    def planes(self, scene, trace_params, rays, use_filter, threads=0):
        """scene: a scene_io.Scene or a SceneView; trace_params: capi.TraceParams; rays [n, 8] float32 -> the six RGBA8 planes uint32 [6, n] a temporal frame stores
        of these rays: colour, colour ip, original colour, id, original id, location id"""
        view = scene.view() if hasattr(scene, "view") else scene
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n = rays.shape[0]
        out = np.zeros((6, n, 4), np.float32)
        fp = frame_params_of(trace_params)
        fp.use_filter, fp.is_temporal = int(use_filter), 1
        rc = self.lib.flx_rays_temporal_ref(C.byref(view), C.byref(fp), rays.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)), None, n, threads)
        if rc != 0:
            raise RuntimeError("flx_rays_temporal_ref failed: %d" % rc)
        return quant(out)

    def history(self, width, height, temporal_samples):
        return History(self, width, height, depth_of(temporal_samples))


class History:
    """the four rings of one history, zero and newest first: rings [4, N, H * W] uint32 (colour, colour ip, location id, original id)"""

    def __init__(self, ref, width, height, depth):
        self.ref, self.width, self.height, self.depth = ref, int(width), int(height), int(depth)
        self.rings = np.zeros((4, self.depth, self.width * self.height), np.uint32)

    def store(self, planes8, use_filter, hdr):
        """the six planes of a new frame (uint32 [6, n]) -> the image float32 [H, W, 4]: the rings rotate, the frame goes to slot 0, the oracle's pass runs"""
        planes8 = np.ascontiguousarray(planes8, np.uint32)
        assert planes8.shape == (6, self.width * self.height)
        self.rings = np.roll(self.rings, 1, axis=1)                 # TempTexture.unshift(TempTexture.pop())
        self.rings[0, 0], self.rings[1, 0], self.rings[2, 0], self.rings[3, 0] = planes8[0], planes8[1], planes8[5], planes8[4]
        rings = np.ascontiguousarray(self.rings)
        original_color, ident = np.ascontiguousarray(planes8[2]), np.ascontiguousarray(planes8[3])
        out = np.zeros((self.height, self.width, 4), np.float32)
        u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
        rc = self.ref.lib.flx_rays_temporal_pass_ref(self.width, self.height, int(hdr), int(use_filter), self.depth, u8(rings), u8(original_color), u8(ident),
                                                     out.ctypes.data_as(C.POINTER(C.c_float)), 0)
        if rc != 0:
            raise RuntimeError("flx_rays_temporal_pass_ref failed: %d" % rc)
        return out

    def frame(self, scene, trace_params, rays, use_filter, hdr):
        """one call of flx_rays_image_temporal on this history"""
        return self.store(self.ref.planes(scene, trace_params, rays, use_filter), use_filter, hdr)
