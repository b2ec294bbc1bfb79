"""renderer.traceImage(..., { temporal: true }) through the whole JavaScript path — FlexLight facade, scene graph, N-API addon, flx_rays_image_temporal — against the
Python binding's sequence on the same rays and params: the same bytes frame after frame, with the renderer's own seeds (its counter % N); resetRayHistory restarts
the sequence."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from flexlight_hip import capi
from rays_trace_util import FRAMES, camera_rays

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH = 4


def traced_by_node(tmp_path, rays, w, h, chain, frames, reset=None):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "web-ray-tracer_amd", "napi", "flexlight_napi.node")
    assert node, "node is part of the image"
    assert os.path.exists(addon), "N-API addon not built (run __graft_entry__.build())"
    rays_file, out = tmp_path / "rays.f32", tmp_path / "images.bin"
    np.ascontiguousarray(rays, np.float32).tofile(rays_file)
    command = [node, os.path.join(ROOT, "tools", "trace_rays.js"), "cornell", "--rays", str(rays_file), "--out", str(out), "--config-spp", "2", "--config-bounces", "3",
               "--filter", "%dx%d" % (w, h), "--hdr", "1", "--temporal", str(DEPTH), "--frames", str(frames), "--history", "5", "--chain", str(chain)]
    if reset is not None:
        command += ["--reset", str(reset)]
    info = json.loads(subprocess.check_output(command, timeout=300).decode().splitlines()[-1])
    assert (info["rays"], info["width"], info["height"], info["frames"], info["temporal"], info["history"], info["chain"]) == (w * h, w, h, frames, DEPTH, 5, bool(chain))
    got = np.fromfile(out, np.uint32)
    assert got.size == frames * w * h * 4
    return info["params"], got.reshape(frames, h, w, 4)


def sequence_of(hip, rays, w, h, q, chain, seeds):
    temporal = capi.RayTemporal(history=5, temporal_samples=DEPTH, use_filter=chain, hdr=1)
    hip.rays_history_reset(5)
    out = []
    for seed in seeds:
        t = capi.TraceParams(q["samples"], q["maxReflections"], q["minImportancy"], q["ambient"], seed, q["textureWidth"])
        out.append(hip.rays_image_temporal(rays, w, h, t, temporal).view(np.uint32))
    hip.rays_history_reset(5)
    return out


@pytest.mark.parametrize("chain", [1, 0])
def test_three_temporal_frames_are_the_python_calls_bytes(hip, oracle, scenes, tmp_path, chain):
    sc, p, rays, _, _ = camera_rays(oracle, scenes, "cornell")
    w, h = FRAMES["cornell"][0:2]
    q, got = traced_by_node(tmp_path, rays, w, h, chain, 3)
    assert (q["samples"], q["maxReflections"], q["textureWidth"]) == (2, 3, p.texture_width)
    hip.update_scene(sc)
    want = sequence_of(hip, rays, w, h, q, chain, (0, 1, 2))
    for f in range(3):
        assert np.array_equal(got[f], want[f]), "frame %d" % f
    assert not np.array_equal(want[0], want[1]) and np.isfinite(want[2].view(np.float32)).all() and (want[2].view(np.float32)[..., 3] > 0).mean() > 0.5


def test_reset_ray_history_restarts_the_sequence(hip, oracle, scenes, tmp_path):
    sc, p, rays, _, _ = camera_rays(oracle, scenes, "cornell")
    w, h = FRAMES["cornell"][0:2]
    q, got = traced_by_node(tmp_path, rays, w, h, 0, 4, reset=2)
    hip.update_scene(sc)
    want = sequence_of(hip, rays, w, h, q, 0, (0, 1))
    for f in range(4):                                                           # the counter and the history both start over at call 2
        assert np.array_equal(got[f], want[f % 2]), "frame %d" % f
    carried_on = sequence_of(hip, rays, w, h, q, 0, (0, 1, 2))
    assert not np.array_equal(carried_on[2], want[0])
