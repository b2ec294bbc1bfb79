"""ctypes loader of flx_camera_rays' CPU reference (tests/camera_ref/flx_camera_ref.c).  TEST INFRASTRUCTURE ONLY.

build(out_dir) compiles it with gcc and the oracle Makefile's floating-point flags into out_dir (outside git).  The file includes include/flx_camera.h, the text
the kernel compiles, and nothing of the oracle."""
import ctypes as C
import os
import subprocess

import numpy as np

from flexlight_hip.capi import Camera

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CFLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-comment"]


def build(out_dir):
    """-> a CameraRef over the library built in out_dir"""
    so = os.path.join(out_dir, "libflx_camera_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-I", os.path.join(ROOT, "include"), "-shared", "-o", so, os.path.join(HERE, "flx_camera_ref.c")])
    return CameraRef(so)


class CameraRef:
    def __init__(self, so):
        lib = C.CDLL(so)
        lib.flx_camera_rays_ref.argtypes = [C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
        lib.flx_camera_rays_ref.restype = C.c_int
        self.lib = lib

    def rays(self, cameras, width, height, region=None):
        """cameras: a capi.Camera or a sequence of them; region (x0, y0, w, h) or None -> ray rows float32 [cameras * w * h, 8], camera by camera, image order"""
        cameras = [cameras] if isinstance(cameras, Camera) else list(cameras)
        arr = (Camera * len(cameras))(*cameras)
        w, h = (int(region[2]), int(region[3])) if region is not None else (int(width), int(height))
        reg = (C.c_uint32 * 4)(*[int(v) for v in region]) if region is not None else None
        out = np.zeros((len(cameras) * w * h, 8), np.float32)
        rc = self.lib.flx_camera_rays_ref(arr, len(cameras), int(width), int(height), reg, out.ctypes.data_as(C.POINTER(C.c_float)))
        if rc != 0:
            raise RuntimeError("flx_camera_rays_ref failed: %d" % rc)
        return out
