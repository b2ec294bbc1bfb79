"""renderer.traceRays(rays, { volume, gain, order }) through the whole JavaScript path — FlexLight facade, scene graph, N-API addon, flx_rays_trace_gather_device on a
handle whose SH rows, maps and offsets stay on the device — returns the C call's rows for the same volume; without `volume` it returns what it returned before; and
it throws its TypeErrors and the library's words."""
import copy
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from flexlight_hip import capi
from rays_gather_util import GAIN, pinhole_rays, words_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "trace_rays_gather.js")
GRID = ((-2.5, -3.0, -3.6), (2.0, 5.0, 1.3), (3, 2, 4))      # test_volume_relocate_js_gpu.py's grid in the Cornell box
RELOCATE = (0.25, 0.3, 20.0, 0.45, 2, 4)


def unpacked(path, n):
    """a rows file of the tool -> words uint32 [n, 8] as the library writes a radiance row (the transform doubled again)"""
    raw = np.fromfile(path, np.uint32)
    assert raw.size == 8 * n
    rows = np.zeros((n, 8), np.uint32)
    rows[:, 0:4] = raw[:4 * n].reshape(n, 4)
    rows[:, 4], rows[:, 5], rows[:, 7] = raw[4 * n:5 * n], raw[5 * n:6 * n], raw[7 * n:8 * n]
    rows[:, 6] = (raw[6 * n:7 * n].view(np.int32) * 2).view(np.uint32)
    return rows


@pytest.mark.parametrize("full", (False, True))
def test_trace_rays_with_a_volume_through_node_is_the_c_call(hip, oracle, scenes, tmp_path, full):
    """a plain handle with the default gain; a handle with map and offsets, a gain of its own and first-hit order"""
    node = shutil.which("node")
    assert node, "node is part of the image"
    assert os.path.exists(os.path.join(ROOT, "web-ray-tracer_amd", "napi", "flexlight_napi.node")), "N-API addon not built (run __graft_entry__.build())"
    sc = scenes("cornell")
    rays = pinhole_rays(oracle, scenes, "cornell")[1][::3].copy()
    n = len(rays)
    rays.tofile(str(tmp_path / "rays.f32"))
    floats = lambda v: ",".join(repr(float(x)) for x in v)      # noqa: E731
    command = [node, TOOL, "cornell", "--rays", str(tmp_path / "rays.f32"), "--origin", floats(GRID[0]), "--spacing", floats(GRID[1]), "--count", "3,2,4", "--bias", "0.0625",
               "--face", "4", "--samples", "3", "--bounces", "2", "--seed", "3", "--dir", str(tmp_path)]
    if full:
        command += ["--map", "4,2", "--relocate", floats(RELOCATE[:4]) + ",%d,%d" % RELOCATE[4:], "--gain", "0.75", "--order", "hits"]
    info = json.loads(subprocess.check_output(command, timeout=300).decode().splitlines()[-1])
    assert info["n"] == n and info["probes"] == 24 and info["hasOffsets"] == full and info["order"] == int(full)
    assert np.float32(info["gain"]) == np.float32(0.75 if full else GAIN)      # the default is Math.fround(1 / Math.PI)
    assert info["errors"] == {"notAHandle": "TypeError", "nullVolume": "TypeError", "numberVolume": "TypeError", "foreignHandle": "TypeError", "gainString": "TypeError",
                              "gainNegative": "Error", "group": "Error"}
    g, q = info["grid"], info["trace"]
    grid = capi.VolumeGrid(g["origin"], g["spacing"], g["count"], g["normalBias"], g["floor"], capi.VOLUME_VISIBILITY if g["visibility"] else 0)
    t = capi.TraceParams(q["samples"], q["maxReflections"], q["minImportancy"], q["ambient"], q["randomSeed"], q["textureWidth"])
    assert (t.samples, t.max_reflections) == (3, 2)
    sh = np.fromfile(str(tmp_path / "rows.bin"), np.float32).reshape(24, 36)
    vmap = capi.VolumeMap(4, 2) if full else None
    maps = np.fromfile(str(tmp_path / "maps.bin"), np.float32).reshape(-1, 4) if full else None
    offsets = np.fromfile(str(tmp_path / "offsets.bin"), np.float32).reshape(24, 4) if full else None
    used = copy.copy(sc)
    used.arrays = dict(sc.arrays, rotation=np.asarray(info["rotation"], np.float32), shift=np.asarray(info["shift"], np.float32))
    hip.update_scene(used)
    want = words_of(hip.trace_rays_gather(rays, t, grid, sh, vmap, maps, offsets, gain=info["gain"], order=info["order"]))
    got = unpacked(str(tmp_path / "gather.bin"), n)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]
    plain = words_of(hip.trace_rays(rays, t))
    assert np.array_equal(unpacked(str(tmp_path / "plain.bin"), n), plain)      # without `volume` the call is what it was
    hit = want[:, 5] != 0xffffffff
    assert hit.any() and (want[hit, 0:3] != plain[hit, 0:3]).any()                # ... and the volume is no no-op on these rays
