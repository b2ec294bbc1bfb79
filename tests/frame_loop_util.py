"""Helpers of the frame-loop tests with anti-aliasing and rasterizer frames (test_frame_loop_aa_gpu.py, test_raster_loop_gpu.py): run
frames through flx_frame_begin / flx_frame_end with two in flight, note the lane each frame went to, read device frames back."""
import ctypes as C

import numpy as np

from flexlight_hip import capi


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def lane_of_last_begun(ctx):
    """0: the frame begun last went to the first lane, 1: to the second (flx_frame_host_slots; host frames only), -1: device frame"""
    slots = (C.c_void_p * 4)()
    last = C.c_int()
    ctx._check(capi.LIB.flx_frame_host_slots(ctx._h, slots, C.byref(last)), "flx_frame_host_slots")
    return -1 if last.value < 0 else last.value // 2


def read_device(ptr, rows, width):
    out = np.empty((rows, width, 4), np.float32)
    hipMemcpy = C.CDLL("libamdhip64.so").hipMemcpy
    hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, 2) == 0      # hipMemcpyDeviceToHost
    return out


def run_loop(ctx, frames, depth=2, between=None):
    """frames: [(params, frame_begin kwargs)], begun in order with up to `depth` in flight.  between(i), if given, runs right before frame i is
    begun.  -> (outputs in begin order: float32 / uint8 [rows, W, 4], device frames copied to the host; lanes; last_chained after each begin)"""
    got, lanes, chained, pending = [], [], [], []

    def take():
        p, kw = pending.pop(0)
        out, ms = ctx.frame_end()
        assert ms > 0.0
        if kw.get("device"):
            out = read_device(out, ctx.tile_row_count(p), p.width)
        got.append(out)

    for i, (p, kw) in enumerate(frames):
        if ctx.frames_in_flight() == depth:
            take()
        if between:
            between(i)
        ctx.frame_begin(p, **kw)
        lanes.append(lane_of_last_begun(ctx))
        chained.append(ctx.last_chained())
        pending.append((p, kw))
    while pending:
        take()
    assert ctx.frames_in_flight() == 0
    return got, lanes, chained
