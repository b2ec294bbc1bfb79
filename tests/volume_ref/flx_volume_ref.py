"""ctypes loader of the probe-volume calls' CPU reference (tests/volume_ref/flx_volume_ref.c).  TEST INFRASTRUCTURE ONLY.

build(out_dir) compiles it with gcc and the oracle Makefile's floating-point flags into out_dir (outside git).  The file includes include/flx_volume.h, the text
the kernels compile, and nothing of the oracle."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CFLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-comment"]


def build(out_dir):
    """-> a VolumeRef over the library built in out_dir"""
    so = os.path.join(out_dir, "libflx_volume_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-I", os.path.join(ROOT, "include"), "-shared", "-o", so, os.path.join(HERE, "flx_volume_ref.c")])
    return VolumeRef(so)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _rows4(a):
    a = np.ascontiguousarray(a, np.float32)
    assert a.ndim == 2 and a.shape[1] == 4
    return a


class VolumeRef:
    """grid: a flexlight_hip.capi.VolumeGrid, whose layout test_volume_cpu.py holds against the C compiler's"""

    def __init__(self, so):
        lib = C.CDLL(so)
        fp, u32, vp = C.POINTER(C.c_float), C.c_uint32, C.c_void_p
        lib.flx_volume_positions_ref.argtypes, lib.flx_volume_positions_ref.restype = [vp, fp], C.c_int
        lib.flx_volume_irradiance_ref.argtypes, lib.flx_volume_irradiance_ref.restype = [vp, fp, fp, fp, u32, fp], C.c_int
        lib.flx_volume_corners_ref.argtypes, lib.flx_volume_corners_ref.restype = [vp, fp, fp, fp, C.POINTER(u32), fp, fp, fp], C.c_int
        self.lib = lib

    def positions(self, grid):
        """-> the grid's position rows float32 [probes, 4]"""
        out = np.zeros((grid.probes, 4), np.float32)
        assert self.lib.flx_volume_positions_ref(C.byref(grid), _fp(out)) == 0
        return out

    def irradiance(self, grid, sh, positions, normals):
        """sh [probes, 36], positions [n, 4], normals [n, 4] -> irradiance rows float32 [n, 4]"""
        sh = np.ascontiguousarray(sh, np.float32).reshape(-1, 36)
        assert sh.shape[0] == grid.probes
        positions, normals = _rows4(positions), _rows4(normals)
        assert len(positions) == len(normals)
        out = np.zeros((len(positions), 4), np.float32)
        assert self.lib.flx_volume_irradiance_ref(C.byref(grid), _fp(sh), _fp(positions), _fp(normals), len(positions), _fp(out)) == 0
        return out

    def corners(self, grid, sh, position, normal):
        """one point that hit -> (probe indices uint32 [8], weights float32 [8], trilinear weights float32 [8], fractions float32 [3])"""
        sh = np.ascontiguousarray(sh, np.float32).reshape(-1, 36)
        assert sh.shape[0] == grid.probes
        position, normal = np.ascontiguousarray(position, np.float32).reshape(4), np.ascontiguousarray(normal, np.float32).reshape(4)
        index, weight, tri, fraction = np.zeros(8, np.uint32), np.zeros(8, np.float32), np.zeros(8, np.float32), np.zeros(3, np.float32)
        assert self.lib.flx_volume_corners_ref(C.byref(grid), _fp(sh), _fp(position), _fp(normal), index.ctypes.data_as(C.POINTER(C.c_uint32)), _fp(weight), _fp(tri),
                                               _fp(fraction)) == 0
        return index, weight, tri, fraction
