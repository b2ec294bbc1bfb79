"""Helpers of the tests of ray images with a volume (test_rays_planes_gather_cpu.py, test_rays_planes_gather_gpu.py, test_rays_planes_gather_js_gpu.py): the CPU
reference built once per session, the pinhole rays of a 40 x 27 image of a golden scene (1080 rays: 16 blocks of 64 and a ragged one) and a handful that miss, the
grids of the tests, and reference planes computed once per key and left unchanged."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "rays_planes_gather_ref"))
import flx_rays_planes_gather_ref  # noqa: E402
from flx_rays_planes_gather_ref import CONSTANT, LIT, NO_POINT, PLANES, TEMPORAL_CANVAS, TEMPORAL_FILTER, quant  # noqa: E402,F401

import rays_trace_util  # noqa: E402
from rays_planes_util import assert_floats, assert_texels, same_floats  # noqa: E402,F401

WIDTH, HEIGHT = 40, 27
MISSES = 7
GAIN = float(np.float32(1.0 / math.pi))
INACTIVE = 1

_ref = []
_rays = {}
_want = {}


def reference(tmp_path_factory):
    """the CPU reference, built once per session"""
    if not _ref:
        _ref.append(flx_rays_planes_gather_ref.build(str(tmp_path_factory.mktemp("rays_planes_gather_ref"))))
    return _ref[0]


def wanted(key, make):
    """reference arrays under `key`, computed once and left unchanged (read-only)"""
    if key not in _want:
        rows = make()
        for r in (rows if isinstance(rows, tuple) else (rows,)):
            r.setflags(write=False)
        _want[key] = rows
    return _want[key]


def trace_params(scene, samples, max_reflections, min_importancy=None, ambient=None, seed=None):
    from flexlight_hip import capi
    p = capi.TraceParams.of_frame(scene.frame_params(width=WIDTH, height=HEIGHT, samples=samples, max_reflections=max_reflections, use_filter=1))
    if min_importancy is not None:
        p.min_importancy = min_importancy
    if ambient is not None:
        p.ambient[:] = ambient
    if seed is not None:
        p.random_seed = float(seed)
    return p


def image_rays(oracle, scenes, name):
    """-> (scene, rays float32 [27 * 40, 8] of the scene's pinhole camera, row 0 on top — flx_camera_rays' rows —, first hit points float64 [k, 3] of those that hit)"""
    if name in _rays:
        return _rays[name]
    import ctypes as C
    sc = scenes(name)
    p = sc.frame_params(width=WIDTH, height=HEIGHT, samples=1, max_reflections=1, use_filter=1)
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
    """the image's rays and MISSES rays aimed away from the scene from behind its camera -> (scene, rays float32 [1080 + 7, 8], points)"""
    sc, rays, points = image_rays(oracle, scenes, name)
    rng = np.random.default_rng(len(name) + 40)
    centre = (points.min(axis=0) + points.max(axis=0)) / 2.0
    extent = float((points.max(axis=0) - points.min(axis=0)).max())
    camera = rays[0, 0:3].astype(np.float64)
    back = camera - centre
    back /= np.linalg.norm(back)
    extra = np.zeros((MISSES, 8), np.float32)
    for k in range(MISSES):
        away = back + rng.normal(size=3) * 0.05
        extra[k, 0:3], extra[k, 4:7] = camera + back * extent * (1.0 + k), away / np.linalg.norm(away)
    extra[:, 3], extra[:, 7] = rng.uniform(-1.0, 1.0, MISSES), rng.uniform(-1.0, 1.0, MISSES)
    return sc, np.ascontiguousarray(np.concatenate([rays, extra]), np.float32), points


def spanning_grid(points, count=(4, 3, 4), normal_bias=0.01, visibility=True, floor=0.05):
    """a grid of `count` probes whose cells cover the points with a margin of a twentieth of their extent"""
    from flexlight_hip import capi
    lo, hi = points.min(axis=0), points.max(axis=0)
    pad = (hi - lo).max() * 0.05
    lo, hi = lo - pad, hi + pad
    spacing = [(hi[a] - lo[a]) / max(count[a] - 1, 1) for a in range(3)]
    return capi.VolumeGrid(tuple(lo), tuple(spacing), count, normal_bias, floor, capi.VOLUME_VISIBILITY if visibility else 0)


def half_grid(points, count=(4, 3, 4), normal_bias=0.01, visibility=True, floor=0.05):
    """the same probes over the lower half of the points' extent along x: about half of the last points fall inside it, the others beside it"""
    from flexlight_hip import capi
    lo, hi = points.min(axis=0), points.max(axis=0)
    pad = (hi - lo).max() * 0.05
    lo, hi = lo - pad, hi + pad
    hi[0] = (lo[0] + hi[0]) / 2.0
    spacing = [(hi[a] - lo[a]) / max(count[a] - 1, 1) for a in range(3)]
    return capi.VolumeGrid(tuple(lo), tuple(spacing), count, normal_bias, floor, capi.VOLUME_VISIBILITY if visibility else 0)


def inactive_offsets(probes):
    """offset rows that say INACTIVE of every probe: the lookup's W is 0 everywhere"""
    rows = np.zeros((probes, 4), np.float32)
    rows.view(np.uint32)[:, 3] = INACTIVE
    return rows


def edge_inactive_offsets(grid):
    """offset rows, no probe moved, that say INACTIVE of the two layers of probes with the largest x: a point in the grid's last cell along x, or beyond it (cells are
    clamped), finds eight inactive corners and W = 0; every other point finds live ones"""
    nx, ny, nz = grid.count[0], grid.count[1], grid.count[2]
    rows = np.zeros((grid.probes, 4), np.float32)
    words = rows.view(np.uint32).reshape(nz, ny, nx, 4)
    words[:, :, nx - 2:, 3] = INACTIVE
    return rows
