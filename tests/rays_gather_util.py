"""Helpers of the tests of traced batches with a volume (test_rays_gather_cpu.py, test_rays_gather_gpu.py, test_rays_gather_js_gpu.py): the CPU reference built once
per session, the pinhole rays of a 64 x 48 image of a golden scene, rays that miss and rays whose paths leave the scene after bounce 0, the grids of the tests placed
over a scene's first hit points, and reference rows computed once per key."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "rays_gather_ref"))
import flx_rays_gather_ref  # noqa: E402

import rays_trace_util  # noqa: E402
from rays_trace_util import assert_rows, same_rows, words_of  # noqa: E402,F401

WIDTH, HEIGHT = 64, 48
GAIN = float(np.float32(1.0 / math.pi))
INACTIVE = 1

_ref = []
_rays = {}
_want = {}


def reference(tmp_path_factory):
    """the CPU reference, built once per session"""
    if not _ref:
        _ref.append(flx_rays_gather_ref.build(str(tmp_path_factory.mktemp("rays_gather_ref"))))
    return _ref[0]


def wanted(key, make):
    """reference rows under `key`, computed once and left unchanged (read-only)"""
    if key not in _want:
        rows = make()
        for r in (rows if isinstance(rows, tuple) else (rows,)):
            r.setflags(write=False)
        _want[key] = rows
    return _want[key]


def trace_params(scene, samples, max_reflections, min_importancy=None, ambient=None):
    from flexlight_hip import capi
    p = capi.TraceParams.of_frame(scene.frame_params(width=WIDTH, height=HEIGHT, samples=samples, max_reflections=max_reflections, use_filter=0))
    if min_importancy is not None:
        p.min_importancy = min_importancy
    if ambient is not None:
        p.ambient[:] = ambient
    return p


def pinhole_rays(oracle, scenes, name):
    """-> (scene, rays float32 [48 * 64, 8] of the scene's camera, row 0 on top, first hit points float64 [k, 3] of the rays that hit)"""
    if name in _rays:
        return _rays[name]
    import ctypes as C
    sc = scenes(name)
    p = sc.frame_params(width=WIDTH, height=HEIGHT, samples=1, max_reflections=1, use_filter=0)
    lib, F3 = rays_trace_util._oracle_calls(oracle)
    view = sc.view()
    rays = np.zeros((HEIGHT * WIDTH, 8), np.float32)
    points = []
    one, half, two = np.float32(1.0), np.float32(0.5), np.float32(2.0)
    for row in range(HEIGHT):
        py_gl = HEIGHT - 1 - row
        for px in range(WIDTH):
            suv, d, ti, tri = F3(), F3(), C.c_int(), C.c_int()
            lib.flx_oracle_primary(C.byref(view), C.byref(p), px, py_gl, suv, C.byref(ti), C.byref(tri), d)
            nx = (np.float32(px) + half) / np.float32(WIDTH) * two - one
            ny = (np.float32(py_gl) + half) / np.float32(HEIGHT) * two - one
            rays[row * WIDTH + px] = [p.camera[0], p.camera[1], p.camera[2], nx, d[0], d[1], d[2], ny]
            suv2, ti2, tri2 = F3(), C.c_int(), C.c_int()
            lib.flx_oracle_ray_tracer(C.byref(view), F3(*p.camera), d, suv2, C.byref(ti2), C.byref(tri2), None)
            if tri2.value != -1:
                points.append(np.array(p.camera[:], np.float64) + np.array(d[:], np.float64) * suv2[0])
    rays.setflags(write=False)
    _rays[name] = (sc, rays, np.array(points))
    return _rays[name]


def batch(oracle, scenes, name):
    """the rays the device tests trace: the pinhole rays, a shuffled copy of them, eight rays that miss (aimed away from the scene from beyond its hit points) and eight
    whose first hit lies in the scene while the way on from there is open — from far outside towards hit points of the scene, so that paths reflected back towards
    the origin leave it after bounce 0 (cornell's open side is where its camera stands) -> (scene, rays float32 [2 * 3072 + 16, 8])"""
    sc, rays, points = pinhole_rays(oracle, scenes, name)
    rng = np.random.default_rng(len(name))
    shuffled = rays[rng.permutation(len(rays))]
    lo, hi = points.min(axis=0), points.max(axis=0)
    centre, extent = (lo + hi) / 2.0, float((hi - lo).max())
    camera = rays[0, 0:3].astype(np.float64)
    back = camera - centre
    back /= np.linalg.norm(back)
    extra = np.zeros((16, 8), np.float32)
    for k in range(8):
        start = camera + back * extent * (1.0 + k)
        away = back + rng.normal(size=3) * 0.05
        extra[k, 0:3], extra[k, 4:7] = start, away / np.linalg.norm(away)
        start = camera + back * extent * (0.5 + 0.25 * k)
        to = points[rng.integers(0, len(points))] - start
        extra[8 + k, 0:3], extra[8 + k, 4:7] = start, to / np.linalg.norm(to)
    extra[:, 3], extra[:, 7] = rng.uniform(-1.0, 1.0, 16), rng.uniform(-1.0, 1.0, 16)
    return sc, np.ascontiguousarray(np.concatenate([rays, shuffled, extra]), np.float32)


def spanning_grid(points, count=(3, 3, 3), normal_bias=0.01, visibility=True, floor=0.05):
    """a grid of `count` probes whose cells cover the points with a margin of a twentieth of their extent"""
    from flexlight_hip import capi
    lo, hi = points.min(axis=0), points.max(axis=0)
    pad = (hi - lo).max() * 0.05
    lo, hi = lo - pad, hi + pad
    spacing = [(hi[a] - lo[a]) / max(count[a] - 1, 1) for a in range(3)]
    return capi.VolumeGrid(tuple(lo), tuple(spacing), count, normal_bias, floor, capi.VOLUME_VISIBILITY if visibility else 0)


def small_grid(points, normal_bias=0.01, visibility=True, floor=0.05):
    """2 x 1 x 2 probes around the middle of the points, a quarter of their extent apart: the scene overhangs it on every side (clamped cells, and count - 2 = 0 on
    the second axis)"""
    from flexlight_hip import capi
    lo, hi = points.min(axis=0), points.max(axis=0)
    centre, step = (lo + hi) / 2.0, float((hi - lo).max()) * 0.25
    return capi.VolumeGrid(tuple(centre - step / 2.0), (step, step, step), (2, 1, 2), normal_bias, floor, capi.VOLUME_VISIBILITY if visibility else 0)


def inactive_offsets(probes):
    """offset rows that say INACTIVE of every probe: the lookup's W is 0 everywhere"""
    rows = np.zeros((probes, 4), np.float32)
    rows.view(np.uint32)[:, 3] = INACTIVE
    return rows
