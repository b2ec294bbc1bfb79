"""ctypes loader of the light-probe calls' CPU reference (tests/probe_ref/flx_probe_ref.c).  TEST INFRASTRUCTURE ONLY.

build(out_dir) compiles it with gcc and the oracle Makefile's floating-point flags into out_dir (outside git).  The file includes include/flx_probe.h, the text
the kernels compile, and nothing of the oracle."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CFLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-comment"]


def build(out_dir):
    """-> a ProbeRef over the library built in out_dir"""
    so = os.path.join(out_dir, "libflx_probe_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-I", os.path.join(ROOT, "include"), "-shared", "-o", so, os.path.join(HERE, "flx_probe_ref.c")])
    return ProbeRef(so)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class ProbeRef:
    def __init__(self, so):
        lib = C.CDLL(so)
        fp, u32 = C.POINTER(C.c_float), C.c_uint32
        lib.flx_probe_rays_ref.argtypes, lib.flx_probe_rays_ref.restype = [fp, u32, u32, fp], C.c_int
        lib.flx_probe_weights_ref.argtypes, lib.flx_probe_weights_ref.restype = [u32, fp], C.c_int
        lib.flx_probe_reduce_ref.argtypes, lib.flx_probe_reduce_ref.restype = [fp, u32, u32, fp, fp], C.c_int
        lib.flx_probe_irradiance_ref.argtypes, lib.flx_probe_irradiance_ref.restype = [fp, fp, fp], None
        self.lib = lib

    def rays(self, positions, face_size):
        """positions [n, 3] or [n, 4] -> ray rows float32 [n * 6 w w, 8], probe by probe, texel order"""
        p = np.asarray(positions, np.float32)
        positions = np.zeros((p.shape[0], 4), np.float32)
        positions[:, :p.shape[1]] = p
        out = np.zeros((positions.shape[0] * 6 * face_size * face_size, 8), np.float32)
        assert self.lib.flx_probe_rays_ref(_fp(positions), positions.shape[0], int(face_size), _fp(out)) == 0
        return out

    def weights(self, face_size):
        """-> d_omega of every texel, float32 [6 w w]"""
        out = np.zeros(6 * face_size * face_size, np.float32)
        assert self.lib.flx_probe_weights_ref(int(face_size), _fp(out)) == 0
        return out

    def reduce(self, radiance, n_probes, face_size, sky=(0.0, 0.0, 0.0)):
        """radiance rows (n_probes * 6 w w x 32 bytes, any dtype) -> SH rows float32 [n_probes, 36]"""
        radiance = np.ascontiguousarray(radiance).reshape(-1).view(np.float32)
        assert radiance.size == n_probes * 6 * face_size * face_size * 8
        sky = np.array(sky, np.float32)
        out = np.zeros((n_probes, 36), np.float32)
        assert self.lib.flx_probe_reduce_ref(_fp(radiance), int(n_probes), int(face_size), _fp(sky), _fp(out)) == 0, "the 64 slots ended up unequal"
        return out

    def irradiance(self, sh, normal):
        sh, normal, out = np.ascontiguousarray(sh, np.float32).reshape(36), np.ascontiguousarray(normal, np.float32).reshape(3), np.zeros(3, np.float32)
        self.lib.flx_probe_irradiance_ref(_fp(sh), _fp(normal), _fp(out))
        return out
