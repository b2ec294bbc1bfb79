"""ctypes loader of the volume-update calls' CPU reference (tests/volume_update_ref/flx_volume_update_ref.c).  TEST INFRASTRUCTURE ONLY.

build(out_dir) compiles it with gcc and tests/volume_ref's flags into out_dir (outside git).  The file includes include/flx_volume_update.h, the text the kernels
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
    """-> a VolumeUpdateRef over the library built in out_dir"""
    so = os.path.join(out_dir, "libflx_volume_update_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-I", os.path.join(ROOT, "include"), "-shared", "-o", so, os.path.join(HERE, "flx_volume_update_ref.c")])
    return VolumeUpdateRef(so)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def _up(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32)) if a is not None else None


def _list(indices, n_list):
    if indices is None:
        return None, int(n_list)
    indices = np.ascontiguousarray(indices, np.uint32).reshape(-1)
    return indices, indices.shape[0]


class VolumeUpdateRef:
    """grid: a flexlight_hip.capi.VolumeGrid; update: a flexlight_hip.capi.VolumeUpdate, whose layout test_volume_update_cpu.py holds against the C compiler's"""

    def __init__(self, so):
        lib = C.CDLL(so)
        fp, u32, vp, f = C.POINTER(C.c_float), C.c_uint32, C.c_void_p, C.c_float
        up = C.POINTER(u32)
        lib.flx_volume_update_positions_ref.argtypes, lib.flx_volume_update_positions_ref.restype = [vp, vp, up, u32, fp], C.c_int
        lib.flx_volume_update_blend_ref.argtypes, lib.flx_volume_update_blend_ref.restype = [vp, vp, u32, up, u32, fp, fp, fp, fp, up], C.c_int
        lib.flx_volume_update_entry_ref.argtypes, lib.flx_volume_update_entry_ref.restype = [vp, up, u32], C.c_uint64
        lib.flx_volume_update_finite_ref.argtypes, lib.flx_volume_update_finite_ref.restype = [f], C.c_int
        lib.flx_volume_update_state_ref.argtypes, lib.flx_volume_update_state_ref.restype = [C.c_int, fp, fp, f], u32
        lib.flx_volume_update_word_ref.argtypes, lib.flx_volume_update_word_ref.restype = [f, f, f], f
        lib.flx_volume_update_map_row_ref.argtypes, lib.flx_volume_update_map_row_ref.restype = [u32, fp, fp, f, fp], C.c_int
        self.lib = lib

    def positions(self, grid, update, indices=None, n_list=None):
        """-> the entries' position rows float32 [n_list, 4]"""
        indices, n = _list(indices, n_list)
        out = np.zeros((n, 4), np.float32)
        assert self.lib.flx_volume_update_positions_ref(C.byref(grid), C.byref(update), _up(indices), n, _fp(out)) == 0
        return out

    def blend(self, grid, update, new_sh, sh, new_maps=None, maps=None, indices=None, n_list=None):
        """new_sh [n_list, 36], sh [probes, 36], new_maps [n_list * bins, 4] and maps [probes * bins, 4] or None -> (sh, maps or None, states uint32 [n_list]), the
        entries blended in ascending order; the arguments are left alone"""
        indices, n = _list(indices, n_list)
        new_sh = np.ascontiguousarray(new_sh, np.float32).reshape(-1, 36)
        sh = np.array(sh, np.float32).reshape(-1, 36)
        assert new_sh.shape[0] == n and sh.shape[0] == grid.probes
        bins = 0
        if maps is not None:
            new_maps, maps = np.ascontiguousarray(new_maps, np.float32).reshape(-1, 4), np.array(maps, np.float32).reshape(-1, 4)
            bins = maps.shape[0] // grid.probes
            assert maps.shape[0] == grid.probes * bins and new_maps.shape[0] == n * bins
        state = np.zeros(n, np.uint32)
        assert self.lib.flx_volume_update_blend_ref(C.byref(grid), C.byref(update), bins, _up(indices), n, _fp(new_sh), _fp(new_maps) if bins else None, _fp(sh),
                                                    _fp(maps) if bins else None, _up(state)) == 0
        return sh, maps, state

    def entry(self, update, j, indices=None):
        indices = np.ascontiguousarray(indices, np.uint32) if indices is not None else None
        return int(self.lib.flx_volume_update_entry_ref(C.byref(update), _up(indices), j))

    def finite(self, x):
        return bool(self.lib.flx_volume_update_finite_ref(np.float32(x)))

    def state(self, in_grid, new_sh, old_sh, h):
        new_sh, old_sh = np.ascontiguousarray(new_sh, np.float32).reshape(36), np.ascontiguousarray(old_sh, np.float32).reshape(36)
        return int(self.lib.flx_volume_update_state_ref(int(in_grid), _fp(new_sh), _fp(old_sh), float(h)))

    def word(self, old, new, h):
        """-> the blended word as float32"""
        return np.float32(self.lib.flx_volume_update_word_ref(np.float32(old), np.float32(new), np.float32(h)))

    def map_row(self, state, old, new, h):
        """-> (whether the row is stored, the row float32 [4])"""
        old, new = np.ascontiguousarray(old, np.float32).reshape(4), np.ascontiguousarray(new, np.float32).reshape(4)
        out = np.zeros(4, np.float32)
        stored = self.lib.flx_volume_update_map_row_ref(int(state), _fp(old), _fp(new), float(h), _fp(out))
        return bool(stored), out
