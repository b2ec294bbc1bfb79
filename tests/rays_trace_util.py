"""Helpers of the traced-ray tests (test_rays_trace_cpu.py, test_rays_trace_gpu.py, test_rays_trace_js_gpu.py): the CPU reference built once per session, a camera's
rays as ray rows (origin = the camera, direction = the primary ray's, noise = the pixel's NDC), rays no camera makes, and the comparison of radiance rows."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "rays_trace_ref"))
import flx_rays_trace_ref  # noqa: E402

# scene -> (width, height, samples, bounces, pixels that must compare): the frames the reference is validated on
FRAMES = {"dragon": (48, 27, 2, 4, 1296), "theater": (32, 18, 2, 6, 576), "cornell": (32, 24, 2, 3, 740)}

_ref = []
_camera = {}
_free = {}


def reference(tmp_path_factory):
    """the CPU reference, built once per session"""
    if not _ref:
        _ref.append(flx_rays_trace_ref.build(str(tmp_path_factory.mktemp("rays_trace_ref"))))
    return _ref[0]


def trace_params(frame_params):
    from flexlight_hip import capi
    return capi.TraceParams.of_frame(frame_params)


def _oracle_calls(oracle):
    from flexlight_hip.scene_io import FrameParams, SceneView
    F3 = C.c_float * 3
    lib = oracle.lib()
    lib.flx_oracle_primary.argtypes = [C.POINTER(SceneView), C.POINTER(FrameParams), C.c_uint32, C.c_uint32, F3, C.POINTER(C.c_int), C.POINTER(C.c_int), F3]
    lib.flx_oracle_primary.restype = None
    lib.flx_oracle_ray_tracer.argtypes = [C.c_void_p, F3, F3, F3, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
    lib.flx_oracle_ray_tracer.restype = None
    return lib, F3


def camera_rays(oracle, scenes, name):
    """-> (scene, frame params, rays [H * W, 8] in the frame's order (row 0 on top), compares bool [H * W], first hits [H * W, 5] float64: s, u, v, 2 x transform,
    entry as flx_oracle_ray_tracer gives them).  A pixel compares where flx_oracle_primary and flx_oracle_ray_tracer name the same triangle with the same (s, u, v)
    bits: the two hit rules differ on back faces, within 2^-16 of an edge, on ties and at the near plane."""
    if name in _camera:
        return _camera[name]
    w, h, samples, bounces, _ = FRAMES[name]
    sc = scenes(name)
    p = sc.frame_params(width=w, height=h, samples=samples, max_reflections=bounces, use_filter=0)
    lib, F3 = _oracle_calls(oracle)
    view = sc.view()
    rays = np.zeros((h * w, 8), np.float32)
    compares = np.zeros(h * w, bool)
    first = np.zeros((h * w, 5), np.float64)
    one, half, two = np.float32(1.0), np.float32(0.5), np.float32(2.0)
    for row in range(h):
        py_gl = h - 1 - row
        for px in range(w):
            k = row * w + px
            suv, d, ti, tri = F3(), F3(), C.c_int(), C.c_int()
            lib.flx_oracle_primary(C.byref(view), C.byref(p), px, py_gl, suv, C.byref(ti), C.byref(tri), d)
            nx = (np.float32(px) + half) / np.float32(w) * two - one          # primary_hit's NDC, float32 operation by operation
            ny = (np.float32(py_gl) + half) / np.float32(h) * two - one
            rays[k] = [p.camera[0], p.camera[1], p.camera[2], nx, d[0], d[1], d[2], ny]
            suv2, ti2, tri2 = F3(), C.c_int(), C.c_int()
            lib.flx_oracle_ray_tracer(C.byref(view), F3(*p.camera), d, suv2, C.byref(ti2), C.byref(tri2), None)
            compares[k] = tri.value == tri2.value and np.array_equal(np.array(suv[:], np.float32).view(np.uint32), np.array(suv2[:], np.float32).view(np.uint32))
            first[k] = [suv2[0], suv2[1], suv2[2], ti2.value, tri2.value]
    _camera[name] = (sc, p, rays, compares, first)
    return _camera[name]


def free_rays(oracle, scenes, name, n=2160):
    """rays that no camera makes, [n, 8]: half of them leave surfaces (first hits of the scene's camera rays, as many in every object space, pushed off along the geometric normal to the side
    the ray came from) in directions of that side's hemisphere, half start in free space around the scene and aim near its hit points; direction lengths in
    [0.25, 4], noise coordinates random in [-1, 1)"""
    if name in _free:
        return _free[name]
    sc, p, cam, _, first = camera_rays(oracle, scenes, name)
    rng = np.random.default_rng(sum(name.encode()))
    hit = np.flatnonzero(first[:, 4] != -1)
    spaces, counts = np.unique(first[hit, 3], return_counts=True)                                        # every object space gets as many points: the small objects too
    weight = (1.0 / counts)[np.searchsorted(spaces, first[hit, 3])]
    pick = rng.choice(hit, n // 2, p=weight / weight.sum())
    o, d = cam[pick, 0:3].astype(np.float64), cam[pick, 4:7].astype(np.float64)
    points = o + d * first[pick, 0:1]
    g = sc.arrays["geometry"].reshape(-1, 12).astype(np.float64)[first[pick, 4].astype(int)]
    rot = sc.arrays["rotation"].reshape(-1, 12).astype(np.float64)[first[pick, 3].astype(int)]          # the forward rotation of transform t is block 2 t: three vec4 columns
    cols = rot.reshape(-1, 3, 4)[:, :, 0:3]
    world = lambda v: cols[:, 0] * v[:, 0:1] + cols[:, 1] * v[:, 1:2] + cols[:, 2] * v[:, 2:3]
    a, b, c = world(g[:, 0:3]), world(g[:, 3:6]), world(g[:, 6:9])
    normal = np.cross(a - b, a - c)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    normal *= -np.sign((normal * d).sum(axis=1, keepdims=True))                                           # the side the camera ray came from
    extent = np.abs(points).max() + 1.0
    away = rng.normal(size=(len(pick), 3))
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    away *= np.sign((away * normal).sum(axis=1, keepdims=True))
    surface = np.concatenate([points + normal * (1e-3 * extent), away], axis=1)
    lo, hi = points.min(axis=0) - 0.25 * extent, points.max(axis=0) + 0.25 * extent
    start = rng.uniform(lo, hi, size=(n - n // 2, 3))
    aim = points[rng.integers(0, len(points), n - n // 2)] + rng.normal(size=(n - n // 2, 3)) * (0.05 * extent)
    to = aim - start
    to /= np.linalg.norm(to, axis=1, keepdims=True)
    both = np.concatenate([surface, np.concatenate([start, to], axis=1)], axis=0)
    both[:, 3:6] *= rng.uniform(0.25, 4.0, size=(n, 1))
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 4:7] = both[:, 0:3], both[:, 3:6]
    rays[:, 3], rays[:, 7] = rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)
    lengths = np.linalg.norm(rays[:, 4:7].astype(np.float64), axis=1)
    assert rays.shape == (2160, 8) and lengths.min() >= 0.2499 and lengths.max() <= 4.0001
    _free[name] = rays
    return rays


def words_of(rows):
    """radiance rows (uint8 [n, 32], numpy or torch) -> uint32 [n, 8]"""
    if not isinstance(rows, np.ndarray):
        rows = rows.detach().cpu().numpy()
    return np.ascontiguousarray(rows, np.uint8).reshape(-1, 32).view(np.uint32)


def same_rows(got, want):
    """bool per row: uint32 [n, 8] against uint32 [n, 8]; a NaN in a float word (0..4) equals any NaN there, as in ray_query_util.same_rows"""
    same = got == want
    nan = lambda b: (b & 0x7fffffff) > 0x7f800000
    same[:, 0:5] |= nan(got[:, 0:5]) & nan(want[:, 0:5])
    return same.all(axis=1)


def assert_rows(got, want, what=""):
    same = same_rows(got, want)
    bad = np.flatnonzero(~same)
    assert got.shape == want.shape and bad.size == 0, "%s: %d of %d rows differ, first %d: got %s want %s" % (
        what, bad.size, len(same), bad[0], ["%08x" % x for x in got[bad[0]]], ["%08x" % x for x in want[bad[0]]])
