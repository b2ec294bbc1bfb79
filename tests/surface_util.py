"""Helpers of the surface-row tests (test_surface_ref_cpu.py, test_surface_gpu.py, test_surface_js_gpu.py): the CPU reference built once per session, the frames
it is validated on, its planes computed once per key, and the comparison of planes as 32-bit words."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "surface_ref"))
import flx_surface_ref  # noqa: E402

# scene -> (width, height): the frames of the reference's validation and of the device's frame tests
FRAMES = {"cornell": (64, 48), "cornell_obj": (96, 54), "dragon": (96, 54), "theater": (96, 54)}
ALL = 255
BITS = (1, 2, 4, 8, 16, 32, 64, 128)
HIT, POSITION, GEOMETRY_NORMAL, NORMAL, UV, ALBEDO, RME, TPO = range(8)      # plane numbers of an all-planes result

_ref = []
_want = {}


def reference(tmp_path_factory):
    """the CPU reference, built once per session"""
    if not _ref:
        _ref.append(flx_surface_ref.build(str(tmp_path_factory.mktemp("surface_ref"))))
    return _ref[0]


def surface_params(scene, width, height):
    """a frame's params as the surface calls read them: the scene's camera at this size, the whole frame"""
    return scene.frame_params(width=width, height=height, samples=1, max_reflections=1, use_filter=0)


def wanted(key, make):
    """the reference's planes under `key`, computed once and left unchanged (read-only)"""
    if key not in _want:
        planes = make()
        planes.setflags(write=False)
        _want[key] = planes
    return _want[key]


def frame_wanted(ref, scenes, name, size=None):
    w, h = size or FRAMES[name]
    sc = scenes(name)
    p = surface_params(sc, w, h)
    return sc, p, wanted(("frame", name, w, h), lambda: ref.frame(sc, p))


def words_of(planes):
    """planes ([p, n, 4] float32, numpy or torch) -> uint32 [p, n, 4]"""
    if not isinstance(planes, np.ndarray):
        planes = planes.detach().cpu().numpy()
    return np.ascontiguousarray(planes).view(np.uint32).reshape(planes.shape[0], -1, 4)


def planes_of(all_planes, fields):
    """the planes of `fields` out of an all-planes result, in bit order"""
    return all_planes[[k for k in range(8) if fields >> k & 1]]


def assert_planes(got, want, what=""):
    """word for word: the reference's planes hold no NaN on these inputs (test_surface_ref_cpu.py asserts every float finite), so equal values have equal words"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, "%s: %d rows differ, first plane %d row %d: got %s want %s" % (
        what, len(bad), bad[0][0], bad[0][1], ["%08x" % x for x in got[bad[0][0], bad[0][1]]], ["%08x" % x for x in want[bad[0][0], bad[0][1]]])
