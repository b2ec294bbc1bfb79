"""renderer.bakeVolume(grid, options), renderer.renderIrradiance(volume) and renderer.irradianceRays(rays, volume) through the whole JavaScript path — FlexLight
facade, scene graph, N-API addon, flx_volume_bake_device / flx_frame_irradiance_device / flx_rays_irradiance_device on rows that stay on the device — return the
bytes of the Python calls on the cornell scene; a group of GPUs throws, as it does for traceProbes."""
import copy
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from flexlight_hip import capi
from rays_trace_util import camera_rays

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "render_irradiance.js")


def same(got, want):
    got, want = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    return got.shape == want.shape and np.array_equal(got, want)


def test_a_volume_through_node_is_the_python_calls(hip, oracle, scenes, tmp_path):
    node = shutil.which("node")
    assert node, "node is part of the image"
    assert os.path.exists(os.path.join(ROOT, "web-ray-tracer_amd", "napi", "flexlight_napi.node")), "N-API addon not built (run __graft_entry__.build())"
    sc = scenes("cornell")
    hip.update_scene(sc)
    first = hip.frame_surface(sc.frame_params(width=64, height=48, samples=1, max_reflections=1, use_filter=0), capi.SURFACE_POSITION)[0]
    hit = first[first[:, 3] != 0.0][:, :3]
    lo, hi = hit.min(axis=0), hit.max(axis=0)
    origin, spacing = (lo + 0.2 * (hi - lo)).astype(np.float32), (0.6 * (hi - lo)).astype(np.float32)
    rays = camera_rays(oracle, scenes, "cornell")[2]
    rays = np.ascontiguousarray(rays[np.linspace(0, len(rays) - 1, 300).astype(int)], np.float32)
    rays_file = tmp_path / "rays.f32"
    rays.tofile(rays_file)
    floats = lambda v: ",".join(repr(float(x)) for x in v)
    for visibility, order in ((1, "hits"), (0, None)):
        rows_file, image_file, out_file = tmp_path / "rows.bin", tmp_path / "image.bin", tmp_path / "rays.bin"
        command = [node, TOOL, "cornell", "--origin", floats(origin), "--spacing", floats(spacing), "--count", "2,2,2", "--bias", "0.03125", "--floor", "0.125",
                   "--visibility", str(visibility), "--face", "4", "--config-spp", "2", "--config-bounces", "3", "--sky", "0.5,0.25,0.125", "--width", "64", "--height", "48",
                   "--rows", str(rows_file), "--out", str(image_file), "--rays", str(rays_file), "--rays-out", str(out_file)] + (["--order", order] if order else [])
        info = json.loads(subprocess.check_output(command, timeout=300).decode().splitlines()[-1])
        assert (info["probes"], info["width"], info["height"], info["rays"], info["order"]) == (8, 64, 48, 300, order)
        g = info["grid"]
        grid = capi.VolumeGrid(g["origin"], g["spacing"], g["count"], g["normalBias"], g["floor"], capi.VOLUME_VISIBILITY if g["visibility"] else 0)
        assert (list(grid.origin), list(grid.spacing), grid.flags) == (origin.tolist(), spacing.tolist(), visibility)
        q = info["trace"]
        t = capi.TraceParams(q["samples"], q["maxReflections"], q["minImportancy"], q["ambient"], q["randomSeed"], q["textureWidth"])
        assert (t.samples, t.max_reflections) == (2, 3)
        used = copy.copy(sc)
        used.arrays = dict(sc.arrays, rotation=np.asarray(info["rotation"], np.float32), shift=np.asarray(info["shift"], np.float32))
        hip.update_scene(used)
        try:
            sh = hip.volume_bake(grid, t, capi.ProbeParams(face_size=4, order=1 if order else 0, sky=(0.5, 0.25, 0.125)))
            f = info["params"]
            p = sc.frame_params(width=f["width"], height=f["height"], samples=1, max_reflections=1, use_filter=0)
            p.camera[:] = f["camera"]
            p.view_matrix[:] = f["viewMatrix"]
            p.texture_width = f["textureWidth"]
            image = hip.frame_irradiance(p, grid, sh)
            rows = hip.rays_irradiance(grid, sh, rays, f["textureWidth"])
        finally:
            hip.update_scene(sc)
        assert np.isfinite(sh).all() and (sh[:, 7] > 0).all() and (image[..., 3] > 0).mean() > 0.5 and (rows[:, 3] > 0).sum() > 100
        assert same(np.fromfile(rows_file, np.float32).reshape(-1, 36), sh), "bakeVolume().rows()"
        assert same(np.fromfile(image_file, np.float32).reshape(48, 64, 4), image), "renderIrradiance"
        assert same(np.fromfile(out_file, np.float32).reshape(-1, 4), rows), "irradianceRays"


def test_a_group_throws_as_trace_probes_does(tmp_path):
    node = shutil.which("node")
    script = tmp_path / "group.js"
    script.write_text("""
const path = require('path');
const { PathTracerHIP } = require(path.join(%r, 'web-ray-tracer_amd', 'js', 'pathtracerHIP.js'));
const r = new PathTracerHIP({ width: 8, height: 8 }, {}, {}, {}, { devices: [0, 0] });
const said = [];
const grid = { origin: [0, 0, 0], spacing: [1, 1, 1], count: [2, 2, 2] };
for (const call of [() => r.bakeVolume(grid), () => r.renderIrradiance({ _handle: 1 }), () => r.irradianceRays(new Float32Array(8), { _handle: 1 })]) {
  try { call(); said.push('no error'); } catch (e) { said.push(e.message); }
}
console.log(JSON.stringify(said));
""" % ROOT)
    said = json.loads(subprocess.check_output([node, str(script)], timeout=120).decode().splitlines()[-1])
    assert said == ["bakeVolume: one GPU only (a group of GPUs traces no rays)", "renderIrradiance: one GPU only (a group of GPUs casts no rays)",
                    "irradianceRays: one GPU only (a group of GPUs casts no rays)"]
