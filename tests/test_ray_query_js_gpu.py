"""renderer.castRays() through the whole JavaScript path — FlexLight facade, scene graph, host flattening, N-API addon, flx_rays_cast — against the same rays
through the ctypes binding of the fixture's arrays: the same words, bit for bit."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from flexlight_hip import capi
from ray_query_util import pack_rays
from test_walk_lds_gpu import make_rays

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("renderer", ["pathtracer", "rasterizer"])
def test_cast_rays_through_node_equals_the_python_call(hip, scenes, tmp_path, renderer):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "web-ray-tracer_amd", "napi", "flexlight_napi.node")
    assert node, "node is part of the image"
    assert os.path.exists(addon), "N-API addon not built (run __graft_entry__.build())"
    sc = scenes("cornell")
    every = make_rays(sc, set(), seed=7)
    rays = pack_rays(every[np.r_[0:24, 900:924, 1800:1816]])              # camera rays, rays from inside the scene, axis-aligned rays: 64 rows
    assert rays.shape == (64, 8)
    rays_file, out = tmp_path / "rays.f32", tmp_path / "hits.bin"
    rays.tofile(rays_file)
    info = json.loads(subprocess.check_output([node, os.path.join(ROOT, "tools", "cast_rays.js"), "cornell", "--rays", str(rays_file), "--out", str(out),
                                               "--what", "3", "--renderer", renderer], timeout=300).decode().splitlines()[-1])
    assert info["rays"] == 64 and info["renderer"] == renderer
    raw = np.fromfile(out, np.uint8)
    assert raw.size == 64 * (12 + 4 + 4 + 1)
    suv, entry, transform, occluded = raw[:768].view(np.uint32), raw[768:1024].view(np.int32), raw[1024:1280].view(np.int32), raw[1280:]
    hip.update_scene(sc)
    want = capi.unpack_hits(hip.cast_rays(rays, 3))
    assert (want["entry"] != -1).sum() >= 16 and 1 <= want["occluded"].sum() < 64 and info["hit"] == (want["entry"] != -1).sum()
    assert np.array_equal(suv, want["suv"].reshape(-1).view(np.uint32))
    assert np.array_equal(entry, want["entry"]) and np.array_equal(transform, want["transform2"] >> 1) and np.array_equal(occluded, want["occluded"])
