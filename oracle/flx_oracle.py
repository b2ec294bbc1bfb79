"""ctypes binding of the CPU oracle (oracle/libflx_oracle.so).  TEST INFRASTRUCTURE ONLY:
imported by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg, never by the product."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_HERE, "..", "web-ray-tracer_amd"))
from flexlight_hip.scene_io import Counters, FrameParams, GBuffers, SceneView  # noqa: E402

_LIB = None


def build():
    subprocess.check_call(["make", "-s", "-C", _HERE])


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libflx_oracle.so")
        if not os.path.exists(so):
            build()
        _LIB = C.CDLL(so)
        _LIB.flx_oracle_render.argtypes = [C.POINTER(SceneView), C.POINTER(FrameParams), C.POINTER(C.c_float),
                                           C.POINTER(GBuffers), C.POINTER(Counters), C.c_int]
        _LIB.flx_oracle_render.restype = C.c_int
        _LIB.flx_oracle_filter.argtypes = [C.POINTER(FrameParams), C.POINTER(GBuffers), C.POINTER(C.c_float), C.c_int]
        _LIB.flx_oracle_filter.restype = C.c_int
        _LIB.flx_oracle_render_sequence.argtypes = [C.POINTER(SceneView), C.POINTER(FrameParams), C.c_int, C.POINTER(C.c_float), C.c_int]
        _LIB.flx_oracle_render_sequence.restype = C.c_int
        _LIB.flx_oracle_render_sequence_frames.argtypes = [C.POINTER(SceneView), C.POINTER(FrameParams), C.c_int, C.POINTER(C.c_float), C.c_int]
        _LIB.flx_oracle_render_sequence_frames.restype = C.c_int
        _LIB.flx_oracle_trace.argtypes = [C.POINTER(SceneView), C.POINTER(FrameParams), C.POINTER(C.c_float), C.POINTER(GBuffers), C.POINTER(Counters), C.c_int]
        _LIB.flx_oracle_trace.restype = C.c_int
    return _LIB


def set_as_written(on):
    """walk fragment:591's ray in every bounce iteration, as the shader is written (same frames, more closest-hit walks)"""
    lib().flx_oracle_set_as_written(1 if on else 0)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def tile_rows(params):
    tr, tc, ti = params.tile_rows, params.tile_count, params.tile_index
    if tr == 0 or tc <= 1:
        return list(range(params.height))
    return [y for y in range(params.height) if (y // tr) % tc == ti]


def render(scene, params, gbuffers=False, threads=0):
    """Returns (rgba [rows, W, 4] float32, counters dict, gbuffers dict or None).

    A temporal frame (is_temporal = 1) goes through the sequence code as a run of ONE frame: it is traced with random_seed = 0 % N = 0 whatever
    params.random_seed says, and averaged over an empty history.  Its G-buffers are therefore those of frame 0 of a run, not of the frame params
    describes: for the G-buffers of frame f of a temporal run, use trace(), which traces params as given."""
    view = scene.view()
    rows = len(tile_rows(params))
    out = np.zeros((rows, params.width, 4), np.float32)
    cnt = Counters()
    gb, gbs = None, None
    if gbuffers:
        gbs = {n: np.zeros((rows, params.width, 4), np.float32) for n, _ in GBuffers._fields_}
        gb = GBuffers(*[_fp(gbs[n]) for n, _ in GBuffers._fields_])
    rc = lib().flx_oracle_render(C.byref(view), C.byref(params), _fp(out), C.byref(gb) if gb else None, C.byref(cnt), threads)
    if rc != 0:
        raise RuntimeError("flx_oracle_render failed: %d" % rc)
    return out, cnt.as_dict(), gbs


def trace(scene, params, threads=0):
    """flx_oracle_trace: the path-trace pass alone, from params as given (seed and camera included) -> the six float G-buffers the pass writes,
    a dict of [rows, W, 4] float32 planes (color, color_ip, original_color, id, original_id, location_id).  No temporal pass, no filter."""
    view = scene.view()
    rows = len(tile_rows(params))
    gbs = {n: np.zeros((rows, params.width, 4), np.float32) for n, _ in GBuffers._fields_}
    gb = GBuffers(*[_fp(gbs[n]) for n, _ in GBuffers._fields_])
    rc = lib().flx_oracle_trace(C.byref(view), C.byref(params), None, C.byref(gb), None, threads)
    if rc != 0:
        raise RuntimeError("flx_oracle_trace failed: %d" % rc)
    return gbs


def render_sequence_frames(scene, params_list, threads=0):
    """A temporal run whose frame f is traced from params_list[f] as given (the camera and the seed are the caller's) -> [n, H, W, 4] float32.
    All frames share width, height, temporal_samples and use_filter, and have is_temporal = 1."""
    view = scene.view()
    n = len(params_list)
    frames = (FrameParams * n)(*[FrameParams.from_buffer_copy(p) for p in params_list])
    out = np.zeros((n, params_list[0].height, params_list[0].width, 4), np.float32)
    rc = lib().flx_oracle_render_sequence_frames(C.byref(view), frames, n, _fp(out), threads)
    if rc != 0:
        raise RuntimeError("flx_oracle_render_sequence_frames failed: %d" % rc)
    return out


def render_sequence(scene, params, n_frames, threads=0):
    """Frames 0..n_frames-1 of a temporal run -> [n_frames, H, W, 4] float32 (canvas colour of every frame)."""
    view = scene.view()
    out = np.zeros((n_frames, params.height, params.width, 4), np.float32)
    rc = lib().flx_oracle_render_sequence(C.byref(view), C.byref(params), n_frames, _fp(out), threads)
    if rc != 0:
        raise RuntimeError("flx_oracle_render_sequence failed: %d" % rc)
    return out


def fxaa(frame):
    """the reference's FXAA pass over a [H, W, 4] float32 frame"""
    a = np.ascontiguousarray(frame, np.float32)
    out = np.empty_like(a)
    rc = lib().flx_oracle_fxaa(a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0], out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError("flx_oracle_fxaa failed: %d" % rc)
    return out


def taa(frames_newest_first):
    """the reference's TAA pass over up to nine [H, W, 4] float32 frames, newest first"""
    fs = [np.ascontiguousarray(f, np.float32) for f in frames_newest_first[:9]]
    out = np.empty_like(fs[0])
    ptrs = (C.c_void_p * len(fs))(*[f.ctypes.data for f in fs])
    rc = lib().flx_oracle_taa(ptrs, len(fs), fs[0].shape[1], fs[0].shape[0], out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError("flx_oracle_taa failed: %d" % rc)
    return out


def present(frame):
    """float RGBA frame [H, W, 4] -> the uint8 RGBA the canvas' drawing buffer holds"""
    a = np.ascontiguousarray(frame, np.float32)
    out = np.zeros(a.shape, np.uint8)
    rc = lib().flx_oracle_present(a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0], out.ctypes.data_as(C.c_void_p))
    if rc:
        raise RuntimeError("flx_oracle_present failed: %d" % rc)
    return out
