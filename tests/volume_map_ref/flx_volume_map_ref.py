"""ctypes loader of the directional-visibility calls' CPU reference (tests/volume_map_ref/flx_volume_map_ref.c).  TEST INFRASTRUCTURE ONLY.

build(out_dir) compiles it with gcc and tests/volume_ref's flags into out_dir (outside git).  The file includes include/flx_volume_map.h, the text the kernels
compile, and nothing of the oracle."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "volume_ref"))
from flx_volume_ref import CFLAGS  # noqa: E402


def build(out_dir):
    """-> a VolumeMapRef over the library built in out_dir"""
    so = os.path.join(out_dir, "libflx_volume_map_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-I", os.path.join(ROOT, "include"), "-shared", "-o", so, os.path.join(HERE, "flx_volume_map_ref.c")])
    return VolumeMapRef(so)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _up(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _rows4(a):
    a = np.ascontiguousarray(a, np.float32)
    assert a.ndim == 2 and a.shape[1] == 4
    return a


class VolumeMapRef:
    """grid: a flexlight_hip.capi.VolumeGrid; map: a flexlight_hip.capi.VolumeMap, whose layout test_volume_map_cpu.py holds against the C compiler's"""

    def __init__(self, so):
        lib = C.CDLL(so)
        fp, u32, vp, f = C.POINTER(C.c_float), C.c_uint32, C.c_void_p, C.c_float
        up = C.POINTER(u32)
        lib.flx_volume_map_rows_ref.argtypes, lib.flx_volume_map_rows_ref.restype = [fp, u32, u32, vp, fp], C.c_int
        lib.flx_volume_map_sphere_ref.argtypes, lib.flx_volume_map_sphere_ref.restype = [fp, u32, fp], C.c_int
        lib.flx_volume_map_irradiance_ref.argtypes, lib.flx_volume_map_irradiance_ref.restype = [vp, vp, fp, fp, fp, fp, u32, fp], C.c_int
        lib.flx_volume_map_decode_ref.argtypes, lib.flx_volume_map_decode_ref.restype = [f, f, fp], None
        lib.flx_volume_map_bin_direction_ref.argtypes, lib.flx_volume_map_bin_direction_ref.restype = [u32, u32, fp], None
        lib.flx_volume_map_bin_ref.argtypes, lib.flx_volume_map_bin_ref.restype = [u32, f, f, f], u32
        lib.flx_volume_map_texel_ref.argtypes, lib.flx_volume_map_texel_ref.restype = [u32, u32, fp], None
        lib.flx_volume_map_wv_ref.argtypes, lib.flx_volume_map_wv_ref.restype = [vp, f, fp], f
        lib.flx_volume_sphere_wv_ref.argtypes, lib.flx_volume_sphere_wv_ref.restype = [vp, f, fp], f
        lib.flx_volume_map_corners_ref.argtypes, lib.flx_volume_map_corners_ref.restype = [vp, vp, fp, fp, fp, up, up, fp, fp], C.c_int
        self.lib = lib

    def rows(self, radiance, n_probes, face_size, vmap):
        """radiance float32 [n_probes * 6 w w, 8] -> map rows float32 [n_probes * m m, 4]"""
        radiance = np.ascontiguousarray(radiance, np.float32).reshape(-1, 8)
        assert radiance.shape[0] == n_probes * 6 * face_size * face_size
        out = np.zeros((n_probes * vmap.size * vmap.size, 4), np.float32)
        assert self.lib.flx_volume_map_rows_ref(_fp(radiance), n_probes, face_size, C.byref(vmap), _fp(out)) == 0
        return out

    def sphere(self, radiance, face_size):
        """one probe's radiance rows -> its SH row's words 7, 11 and 15, float32 [3]"""
        radiance = np.ascontiguousarray(radiance, np.float32).reshape(-1, 8)
        assert radiance.shape[0] == 6 * face_size * face_size
        out = np.zeros(3, np.float32)
        assert self.lib.flx_volume_map_sphere_ref(_fp(radiance), face_size, _fp(out)) == 0
        return out

    def irradiance(self, grid, vmap, sh, maps, positions, normals):
        """sh [probes, 36], maps [probes * m m, 4], positions [n, 4], normals [n, 4] -> irradiance rows float32 [n, 4]"""
        sh = np.ascontiguousarray(sh, np.float32).reshape(-1, 36)
        maps = _rows4(np.asarray(maps, np.float32).reshape(-1, 4))
        assert sh.shape[0] == grid.probes and maps.shape[0] == grid.probes * vmap.size * vmap.size
        positions, normals = _rows4(positions), _rows4(normals)
        assert len(positions) == len(normals)
        out = np.zeros((len(positions), 4), np.float32)
        assert self.lib.flx_volume_map_irradiance_ref(C.byref(grid), C.byref(vmap), _fp(sh), _fp(maps), _fp(positions), _fp(normals), len(positions), _fp(out)) == 0
        return out

    def decode(self, u, v):
        out = np.zeros(3, np.float32)
        self.lib.flx_volume_map_decode_ref(float(u), float(v), _fp(out))
        return out

    def bin_direction(self, m, b):
        out = np.zeros(3, np.float32)
        self.lib.flx_volume_map_bin_direction_ref(m, b, _fp(out))
        return out

    def bin(self, m, direction):
        return int(self.lib.flx_volume_map_bin_ref(m, float(direction[0]), float(direction[1]), float(direction[2])))

    def texel(self, face_size, t):
        """-> (direction float32 [3], d_omega)"""
        out = np.zeros(4, np.float32)
        self.lib.flx_volume_map_texel_ref(face_size, t, _fp(out))
        return out[:3], out[3]

    def wv(self, grid, dist, q):
        q = np.ascontiguousarray(q, np.float32).reshape(4)
        return np.float32(self.lib.flx_volume_map_wv_ref(C.byref(grid), float(dist), _fp(q)))

    def sphere_wv(self, grid, dist, moments):
        moments = np.ascontiguousarray(moments, np.float32).reshape(3)
        return np.float32(self.lib.flx_volume_sphere_wv_ref(C.byref(grid), float(dist), _fp(moments)))

    def corners(self, grid, vmap, maps, position, normal):
        """one point that hit -> (probe indices uint32 [8], bins uint32 [8], weights float32 [8], distances float32 [8])"""
        maps = _rows4(np.asarray(maps, np.float32).reshape(-1, 4))
        position, normal = np.ascontiguousarray(position, np.float32).reshape(4), np.ascontiguousarray(normal, np.float32).reshape(4)
        index, bins, weight, dist = np.zeros(8, np.uint32), np.zeros(8, np.uint32), np.zeros(8, np.float32), np.zeros(8, np.float32)
        assert self.lib.flx_volume_map_corners_ref(C.byref(grid), C.byref(vmap), _fp(maps), _fp(position), _fp(normal), _up(index), _up(bins), _fp(weight), _fp(dist)) == 0
        return index, bins, weight, dist
