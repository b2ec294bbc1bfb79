"""renderer.traceImage() through the whole JavaScript path — FlexLight facade, scene graph, N-API addon, flx_rays_image — against the Python binding's call on the same
rays and params: the same bytes; and a group of GPUs throws, as it does for traceRays."""
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


@pytest.mark.parametrize("hdr", [1, 0])
def test_trace_image_on_cornells_camera_rays_is_the_python_calls_bytes(hip, oracle, scenes, tmp_path, hdr):
    sc, p, rays, _, _ = camera_rays(oracle, scenes, "cornell")
    w, h = FRAMES["cornell"][0:2]
    node = shutil.which("node")
    addon = os.path.join(ROOT, "web-ray-tracer_amd", "napi", "flexlight_napi.node")
    assert node, "node is part of the image"
    assert os.path.exists(addon), "N-API addon not built (run __graft_entry__.build())"
    rays_file, out = tmp_path / "rays.f32", tmp_path / "image.bin"
    np.ascontiguousarray(rays, np.float32).tofile(rays_file)
    info = json.loads(subprocess.check_output([node, os.path.join(ROOT, "tools", "trace_rays.js"), "cornell", "--rays", str(rays_file), "--out", str(out),
                                               "--config-spp", "2", "--config-bounces", "3", "--filter", "%dx%d" % (w, h), "--hdr", str(hdr)], timeout=300).decode().splitlines()[-1])
    q = info["params"]
    assert (info["rays"], info["width"], info["height"], info["hdr"], info["renderer"]) == (w * h, w, h, bool(hdr), "pathtracer")
    assert (q["samples"], q["maxReflections"], q["randomSeed"], q["textureWidth"]) == (2, 3, 0, p.texture_width)
    t = capi.TraceParams(q["samples"], q["maxReflections"], q["minImportancy"], q["ambient"], q["randomSeed"], q["textureWidth"])
    got = np.fromfile(out, np.uint32)
    assert got.size == w * h * 4
    hip.update_scene(sc)
    want = hip.ray_image(rays, w, h, t, hdr=hdr)
    assert np.array_equal(got.reshape(h, w, 4), want.view(np.uint32))
    assert np.isfinite(want).all() and (want[..., 3] > 0).mean() > 0.5            # an image, not zeros


def test_a_group_throws_as_trace_rays_does(tmp_path):
    node = shutil.which("node")
    script = tmp_path / "group.js"
    script.write_text("""
const path = require('path');
const { FlexLight } = require(path.join(%r, 'web-ray-tracer_amd', 'js', 'flexlight.js'));
const { PathTracerHIP } = require(path.join(%r, 'web-ray-tracer_amd', 'js', 'pathtracerHIP.js'));
const r = new PathTracerHIP({ width: 8, height: 8 }, {}, {}, {}, { devices: [0, 0] });
const said = [];
for (const call of [() => r.traceImage(new Float32Array(8), 1, 1), () => r.traceRays(new Float32Array(8))]) {
  try { call(); said.push('no error'); } catch (e) { said.push(e.message); }
}
console.log(JSON.stringify(said));
""" % (ROOT, ROOT))
    said = json.loads(subprocess.check_output([node, str(script)], timeout=120).decode().splitlines()[-1])
    assert said == ["traceImage: one GPU only (a group of GPUs traces no rays)", "traceRays: one GPU only (a group of GPUs traces no rays)"]
