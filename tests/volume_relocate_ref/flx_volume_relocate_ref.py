"""ctypes loader of the probe-relocation calls' CPU reference (tests/volume_relocate_ref/flx_volume_relocate_ref.c).  TEST INFRASTRUCTURE ONLY.

build(out_dir) compiles it with gcc and tests/volume_ref's flags into out_dir (outside git).  The file includes include/flx_volume_relocate.h, the text the kernels
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
    """-> a VolumeRelocateRef over the library built in out_dir"""
    so = os.path.join(out_dir, "libflx_volume_relocate_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-I", os.path.join(ROOT, "include"), "-shared", "-o", so, os.path.join(HERE, "flx_volume_relocate_ref.c")])
    return VolumeRelocateRef(so)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def _up(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32)) if a is not None else None


def _plane(a):
    """a plane of 16-byte rows of any dtype -> float32 [rows, 4] over the same bits"""
    return np.ascontiguousarray(a).reshape(-1).view(np.float32).reshape(-1, 4)


class VolumeRelocateRef:
    """grid: a flexlight_hip.capi.VolumeGrid; relocate: a flexlight_hip.capi.VolumeRelocate, whose layout test_volume_relocate_cpu.py holds against the C compiler's"""

    def __init__(self, so):
        lib = C.CDLL(so)
        fp, u32, vp = C.POINTER(C.c_float), C.c_uint32, C.c_void_p
        up, u64p = C.POINTER(u32), C.POINTER(C.c_uint64)
        lib.flx_volume_relocate_probes_ref.argtypes, lib.flx_volume_relocate_probes_ref.restype = [vp, vp, u32, fp, fp, u32, u32, fp], C.c_int
        lib.flx_volume_relocate_sums_ref.argtypes, lib.flx_volume_relocate_sums_ref.restype = [u32, fp, fp, u64p], C.c_int
        lib.flx_volume_relocate_sums_slots_ref.argtypes, lib.flx_volume_relocate_sums_slots_ref.restype = [u32, fp, fp, u64p], C.c_int
        lib.flx_volume_relocate_direction_ref.argtypes, lib.flx_volume_relocate_direction_ref.restype = [u32, u32, fp], C.c_int
        lib.flx_volume_relocate_positions_ref.argtypes, lib.flx_volume_relocate_positions_ref.restype = [vp, fp, vp, up, u32, u32, fp], C.c_int
        lib.flx_volume_relocate_lookup_ref.argtypes, lib.flx_volume_relocate_lookup_ref.restype = [vp, vp, fp, fp, fp, fp, fp, u32, fp], C.c_int
        self.lib = lib

    def relocate(self, grid, relocate, face_size, hit, normal, offsets, first_probe=0):
        """hit, normal: planes of n_probes * 6 w w rows; offsets [probes, 4] -> the updated offset rows float32 [probes, 4]; the arguments are left alone"""
        hit, normal = _plane(hit), _plane(normal)
        rays = 6 * face_size * face_size
        n = hit.shape[0] // rays
        assert hit.shape[0] == n * rays and normal.shape == hit.shape
        out = np.array(offsets, np.float32).reshape(-1, 4)
        assert out.shape[0] == grid.probes and first_probe + n <= grid.probes
        assert self.lib.flx_volume_relocate_probes_ref(C.byref(grid), C.byref(relocate), face_size, _fp(hit), _fp(normal), n, first_probe, _fp(out)) == 0
        return out

    def sums(self, face_size, hit, normal, slots=False):
        """one probe's reduction -> (H, B, closest-back key, closest-front key, farthest-front key) as Python ints; slots: reduced as the kernel's lanes do"""
        hit, normal = _plane(hit), _plane(normal)
        assert hit.shape[0] == 6 * face_size * face_size and normal.shape == hit.shape
        out = (C.c_uint64 * 5)()
        call = self.lib.flx_volume_relocate_sums_slots_ref if slots else self.lib.flx_volume_relocate_sums_ref
        assert call(face_size, _fp(hit), _fp(normal), out) == 0
        return tuple(int(x) for x in out)

    def direction(self, face_size, t):
        out = np.zeros(3, np.float32)
        assert self.lib.flx_volume_relocate_direction_ref(face_size, t, _fp(out)) == 0
        return out

    def directions(self, face_size):
        """-> float32 [6 w w, 3]"""
        return np.stack([self.direction(face_size, t) for t in range(6 * face_size * face_size)])

    def positions(self, grid, offsets, update=None, indices=None, n=None):
        """-> the position rows float32 [n, 4]: the whole grid (update None), or the update's list"""
        offsets = np.ascontiguousarray(offsets, np.float32).reshape(-1, 4)
        assert offsets.shape[0] == grid.probes
        if indices is not None:
            indices = np.ascontiguousarray(indices, np.uint32).reshape(-1)
            n = indices.shape[0]
        if update is None:
            n = grid.probes
        out = np.zeros((int(n), 4), np.float32)
        assert self.lib.flx_volume_relocate_positions_ref(C.byref(grid), _fp(offsets), C.byref(update) if update is not None else None, _up(indices), 1 if update is not None else 0,
                                                          int(n), _fp(out)) == 0
        return out

    def lookup(self, grid, sh, offsets, positions, normals, vmap=None, maps=None):
        """-> the irradiance rows float32 [n, 4]"""
        sh = np.ascontiguousarray(sh, np.float32).reshape(-1, 36)
        offsets = np.ascontiguousarray(offsets, np.float32).reshape(-1, 4)
        positions, normals = np.ascontiguousarray(positions, np.float32).reshape(-1, 4), np.ascontiguousarray(normals, np.float32).reshape(-1, 4)
        assert sh.shape[0] == grid.probes and offsets.shape[0] == grid.probes and positions.shape == normals.shape and (vmap is None) == (maps is None)
        if maps is not None:
            maps = np.ascontiguousarray(maps, np.float32).reshape(-1, 4)
            assert maps.shape[0] == grid.probes * vmap.bins
        out = np.zeros((positions.shape[0], 4), np.float32)
        assert self.lib.flx_volume_relocate_lookup_ref(C.byref(grid), C.byref(vmap) if vmap is not None else None, _fp(sh), _fp(maps), _fp(offsets), _fp(positions), _fp(normals),
                                                       positions.shape[0], _fp(out)) == 0
        return out
