"""Helpers of the camera tests (test_camera_cpu.py, test_camera_gpu.py, test_camera_js_gpu.py): the CPU reference built once per session, the cameras the tests use,
and float64 restatements of include/flexlight_hip_debug.h's "cameras" formulas."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "camera_ref"))
import flx_camera_ref  # noqa: E402

JITTER = (0.3, -0.45)
POSITION = (1.25, -0.5, 3.0)
FISHEYE_FOV = float(np.deg2rad(220.0))
SIZES = ((7, 5), (65, 3), (33, 31))

_ref = []


def reference(tmp_path_factory):
    """the CPU reference, built once per session"""
    if not _ref:
        _ref.append(flx_camera_ref.build(str(tmp_path_factory.mktemp("camera_ref"))))
    return _ref[0]


def rotated_basis(seed=5):
    """a random rotation, float32 [9]: rows right, up, forward (orthonormal to float32's precision)"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[2] = -q[2]
    return q.astype(np.float32).reshape(9)


def skewed_basis(seed=9):
    """a basis that is neither orthogonal nor normalised, float32 [9]: used as given"""
    rng = np.random.default_rng(seed)
    return (rotated_basis(seed).reshape(3, 3) * np.array([[1.7], [0.6], [2.3]]) + rng.normal(size=(3, 3)) * 0.2).astype(np.float32).reshape(9)


def cameras_of(capi, basis, jitter=JITTER, position=POSITION):
    """the four projections beside the pinhole, and all six faces: name -> Camera"""
    out = {
        "panorama": capi.Camera.panorama(position, basis, jitter=jitter),
        "fisheye": capi.Camera.fisheye(position, basis, fov=FISHEYE_FOV, jitter=jitter),
        "orthographic": capi.Camera.orthographic(position, basis, width=3.5, height=2.25, jitter=jitter),
    }
    for face in range(6):
        out["cube_face%d" % face] = capi.Camera.cube_face(position, face, basis, jitter=jitter)
    return out


FACES = {0: ((1, 0, 0), (0, 0, -1), (0, 1, 0)), 1: ((-1, 0, 0), (0, 0, 1), (0, 1, 0)), 2: ((0, 1, 0), (1, 0, 0), (0, 0, -1)),
         3: ((0, -1, 0), (1, 0, 0), (0, 0, 1)), 4: ((0, 0, 1), (1, 0, 0), (0, 1, 0)), 5: ((0, 0, -1), (-1, 0, 0), (0, 1, 0))}      # face -> F, R, U


def expected64(camera, width, height):
    """the header's formulas in float64 for a camera that is no pinhole, from the camera's float32 fields -> (origins [H * W, 3], directions [H * W, 3],
    noise [H * W, 2]) in image order, row 0 on top"""
    f64 = lambda a: np.array(list(a), np.float64)
    basis, extent, jitter, position = f64(camera.basis).reshape(3, 3), f64(camera.extent), f64(camera.jitter), f64(camera.position)
    px, row = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    py = height - 1 - row
    sx = (px + (0.5 + jitter[0])) / width * 2.0 - 1.0
    sy = (py + (0.5 + jitter[1])) / height * 2.0 - 1.0
    noise = np.stack([(px + 0.5) / width * 2.0 - 1.0, (py + 0.5) / height * 2.0 - 1.0], axis=-1).reshape(-1, 2)
    right, up, forward = basis
    world = lambda lx, ly, lz: (right * lx[..., None] + up * ly[..., None]) + forward * lz[..., None]
    origin = np.broadcast_to(position, (height, width, 3))
    projection = camera.projection
    if projection == 1:
        lon, lat = sx * (0.5 * extent[0]), sy * (0.5 * extent[1])
        d = world(np.sin(lon) * np.cos(lat), np.sin(lat), np.cos(lon) * np.cos(lat))
    elif projection == 2:
        q = np.sqrt(sx * sx + sy * sy)
        theta = q * (0.5 * extent[0])
        safe = np.where(q == 0.0, 1.0, q)
        d = world(np.where(q == 0.0, 0.0, np.sin(theta) * sx / safe), np.where(q == 0.0, 0.0, np.sin(theta) * sy / safe), np.where(q == 0.0, 1.0, np.cos(theta)))
    elif projection == 3:
        origin = position + (right * (sx * (0.5 * extent[0]))[..., None] + up * (sy * (0.5 * extent[1]))[..., None])
        d = np.broadcast_to(forward, (height, width, 3))
    elif projection == 4:
        F, R, U = (np.array(v, np.float64) for v in FACES[camera.face])
        l = F + R * sx[..., None] + U * sy[..., None]
        d = world(l[..., 0], l[..., 1], l[..., 2])
    else:
        raise ValueError("expected64: no pinhole")
    d = d / np.sqrt((d * d).sum(axis=-1, keepdims=True))
    return origin.reshape(-1, 3), d.reshape(-1, 3), noise


def assert_same_rows(got, want, what=""):
    """ray rows float32 [n, 8] against float32 [n, 8], bit for bit"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, "%s: %s rows against %s" % (what, got.shape, want.shape)
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert bad.size == 0, "%s: %d of %d rows differ, first %d: got %s want %s" % (
        what, bad.size, len(got), bad[0], ["%08x" % x for x in got.view(np.uint32)[bad[0]]], ["%08x" % x for x in want.view(np.uint32)[bad[0]]])
