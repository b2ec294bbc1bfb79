"""ctypes loader of the CPU reference of a slab's bounds and keys (tests/ray_order_ref/flx_ray_order_ref.c).  TEST INFRASTRUCTURE ONLY.

build(out_dir) compiles it with gcc and the library's floating-point flags into out_dir (outside git).  The file includes include/flx_ray_key.h, the text the
kernels compile, and nothing else of the library."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CFLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-comment"]


def build(out_dir):
    """-> a RayOrderRef over the library built in out_dir"""
    so = os.path.join(out_dir, "libflx_ray_order_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-I", os.path.join(ROOT, "include"), "-shared", "-o", so, os.path.join(HERE, "flx_ray_order_ref.c")])
    return RayOrderRef(so)


class RayOrderRef:
    def __init__(self, so):
        lib = C.CDLL(so)
        u32p = C.POINTER(C.c_uint32)
        lib.flx_ray_order_keys_ref.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, u32p, u32p]
        lib.flx_ray_order_keys_ref.restype = C.c_uint32
        for name, count in (("flx_ray_order_morton_ref", 3), ("flx_ray_order_map_ref", 1), ("flx_ray_order_unmap_ref", 1)):
            getattr(lib, name).argtypes = [C.c_uint32] * count
            getattr(lib, name).restype = C.c_uint32
        self.lib = lib

    def keys(self, rays, hits):
        """ray rows float32 [n, 8], hit rows (32 bytes each, any dtype) -> (keys uint32 [n], bounds as bits uint32 [6]: lo x y z, hi x y z, live rays)"""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n = rays.shape[0]
        hits = np.ascontiguousarray(hits).reshape(n, -1).view(np.float32)
        assert hits.shape == (n, 8)
        keys, bounds = np.zeros(n, np.uint32), np.zeros(6, np.uint32)
        fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        live = self.lib.flx_ray_order_keys_ref(rays.ctypes.data_as(fp), hits.ctypes.data_as(fp), n, keys.ctypes.data_as(up), bounds.ctypes.data_as(up))
        return keys, bounds, int(live)

    def morton(self, qx, qy, qz):
        return int(self.lib.flx_ray_order_morton_ref(int(qx), int(qy), int(qz)))

    def map(self, bits):
        return int(self.lib.flx_ray_order_map_ref(int(bits)))

    def unmap(self, mapped):
        return int(self.lib.flx_ray_order_unmap_ref(int(mapped)))
