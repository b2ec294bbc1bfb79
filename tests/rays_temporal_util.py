"""Helpers of the temporal ray-image tests (test_rays_temporal_cpu.py, test_rays_temporal_gpu.py, test_rays_temporal_js_gpu.py): the CPU reference built once per
session, a frame's six planes traced once per key and left unchanged, and reference sequences over rings held in Python.  The rays are rays_trace_util's."""
import copy
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "rays_temporal_ref"))
import flx_rays_temporal_ref  # noqa: E402
from flx_rays_temporal_ref import depth_of  # noqa: E402,F401
from rays_planes_util import assert_floats, same_floats  # noqa: E402,F401

_ref = []
_planes = {}
_sequences = {}


def reference(tmp_path_factory):
    """the CPU reference, built once per session"""
    if not _ref:
        _ref.append(flx_rays_temporal_ref.build(str(tmp_path_factory.mktemp("rays_temporal_ref"))))
    return _ref[0]


def seeded(t, seed):
    """a copy of a TraceParams with another random_seed"""
    q = copy.copy(t)
    q.random_seed = float(seed)
    return q


def traced(ref, key, sc, t, rays, use_filter):
    """the reference's six RGBA8 planes (uint32 [6, n]) of these rays at this seed, computed once per (key, seed, use_filter) and left unchanged.  `key` names the
    scene state and the rays; the params other than the seed are one per key."""
    full = (key, float(t.random_seed), int(use_filter))
    if full not in _planes:
        planes = ref.planes(sc, t, rays, use_filter)
        planes.setflags(write=False)
        _planes[full] = planes
    return _planes[full]


def sequence(ref, key, sc, t, rays, width, height, temporal_samples, use_filter, hdr, frames, seeds=None):
    """the reference's images of `frames` calls on a fresh history, one set of rays standing still, seed f % N unless given: a list of float32 [H, W, 4], computed
    once per key and left unchanged"""
    n = depth_of(temporal_samples)
    seeds = tuple(seeds) if seeds is not None else tuple(f % n for f in range(frames))
    full = (key, width, height, n, int(use_filter), int(hdr), seeds)
    if full not in _sequences:
        history = ref.history(width, height, temporal_samples)
        out = []
        for f in range(frames):
            image = history.store(traced(ref, key, sc, seeded(t, seeds[f]), rays, use_filter), use_filter, hdr)
            image.setflags(write=False)
            out.append(image)
        _sequences[full] = out
    return _sequences[full]
