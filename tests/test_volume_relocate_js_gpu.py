"""renderer.relocateVolume(volume, { backShare, minFront, reach, limit, iterations, faceSize }) through the whole JavaScript path — FlexLight facade, scene graph,
N-API addon, flx_volume_relocate_device on offset rows that stay on the device — returns the offsets and states of the Python binding's passes on the cornell scene;
a handle that has offsets routes updateVolume and renderIrradiance through the relocated calls, whose rows and image are the C ABI's; a handle without offsets gives
today's bytes; bakeVolume(grid, { relocate }) relocates first and bakes from the moved positions; and the method throws its type errors and the library's words."""
import copy
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from flexlight_hip import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "relocate_volume.js")
# test_volume_relocate_gpu.py's grid in the Cornell box: probe 18 starts inside the short cuboid, probe 20 inside the tall one
GRID = ((-2.5, -3.0, -3.6), (2.0, 5.0, 1.3), (3, 2, 4))
RELOCATE = (0.25, 0.3, 20.0, 0.45, 3, 4)           # back_share, min_front, reach, limit; three passes and a frozen one; face size 4


def same(got, want):
    got, want = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    return got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("with_map", (False, True))
def test_relocation_through_node_is_the_python_calls(hip, scenes, tmp_path, with_map):
    node = shutil.which("node")
    assert node, "node is part of the image"
    assert os.path.exists(os.path.join(ROOT, "web-ray-tracer_amd", "napi", "flexlight_napi.node")), "N-API addon not built (run __graft_entry__.build())"
    sc = scenes("cornell")
    floats = lambda v: ",".join(repr(float(x)) for x in v)
    command = [node, TOOL, "cornell", "--origin", floats(GRID[0]), "--spacing", floats(GRID[1]), "--count", "3,2,4", "--bias", "0.0625", "--face", "2", "--sky", "0.5,0.25,0.125",
               "--seed", "3", "--update-seed", "7", "--relocate", floats(RELOCATE[:4]) + ",%d,%d" % RELOCATE[4:], "--dir", str(tmp_path)]
    command += ["--map", "2,1"] if with_map else []
    info = json.loads(subprocess.check_output(command, timeout=300).decode().splitlines()[-1])
    assert info["probes"] == 24 and not info["hadOffsets"] and info["sameOffsets"] and info["map"] == ({"size": 2, "sharpness": 1} if with_map else None)
    g = info["grid"]
    grid = capi.VolumeGrid(g["origin"], g["spacing"], g["count"], g["normalBias"], g["floor"], capi.VOLUME_VISIBILITY if g["visibility"] else 0)
    q, f = info["trace"], info["params"]
    trace = lambda seed: capi.TraceParams(q["samples"], q["maxReflections"], q["minImportancy"], q["ambient"], seed, q["textureWidth"])
    probe, vmap = capi.ProbeParams(face_size=2, sky=(0.5, 0.25, 0.125)), capi.VolumeMap(2, 1) if with_map else None
    relocate = capi.VolumeRelocate(*RELOCATE[:4])
    frozen = capi.VolumeRelocate(*RELOCATE[:4], flags=capi.RELOCATE_FREEZE)
    used = copy.copy(sc)
    used.arrays = dict(sc.arrays, rotation=np.asarray(info["rotation"], np.float32), shift=np.asarray(info["shift"], np.float32))
    hip.update_scene(used)
    try:
        p = sc.frame_params(width=f["width"], height=f["height"], samples=1, max_reflections=1, use_filter=0)
        p.camera[:] = f["camera"]
        p.view_matrix[:] = f["viewMatrix"]
        p.texture_width = f["textureWidth"]
        plain_sh, plain_maps = hip.volume_bake_map(grid, trace(3.0), probe, vmap) if with_map else (hip.volume_bake(grid, trace(3.0), probe), None)
        plain_image = hip.frame_irradiance_map(p, grid, plain_sh, vmap, plain_maps) if with_map else hip.frame_irradiance(p, grid, plain_sh)
        offsets = np.zeros((24, 4), np.float32)
        for k in range(RELOCATE[4] + 1):
            offsets = hip.volume_relocate(grid, frozen if k == RELOCATE[4] else relocate, RELOCATE[5], offsets, q["textureWidth"])
        sh, maps, states = hip.volume_update_relocated(grid, trace(7.0), probe, vmap, capi.VolumeUpdate(0.0, 0, 1), offsets, plain_sh, plain_maps, n_list=24)
        image = hip.frame_irradiance_relocated(p, grid, sh, offsets, vmap, maps)
        baked = hip.volume_bake_relocated(grid, trace(3.0), probe, offsets, vmap)
    finally:
        hip.update_scene(sc)
    read = lambda name, dtype, width: np.fromfile(tmp_path / name, dtype).reshape(-1, width)
    # a handle without offsets gives today's bytes
    assert same(read("plain_rows.bin", np.float32, 36), plain_sh), "bakeVolume().rows() before the relocation"
    assert same(read("plain_image.bin", np.float32, 4), plain_image.reshape(-1, 4)), "renderIrradiance before the relocation"
    # relocateVolume's offsets and states are the Python call's
    moved = np.abs(offsets[:, :3]).max(axis=1) > 0
    assert moved.sum() >= 2 and capi.relocate_states(offsets)[20] & capi.RELOCATE_INACTIVE and moved[18]
    assert same(read("offsets.bin", np.float32, 4), offsets), "relocateVolume().offsets"
    assert read("states.bin", np.uint32, 1).reshape(-1).tolist() == capi.relocate_states(offsets).tolist()
    # a handle with offsets goes through the relocated calls
    assert read("update_states.bin", np.uint32, 1).reshape(-1).tolist() == states.tolist() and set(states.tolist()) <= {1, 2}
    assert same(read("rows.bin", np.float32, 36), sh), "updateVolume on a relocated handle"
    assert not same(sh[moved], plain_sh[moved])
    if with_map:
        assert same(read("maps.bin", np.float32, 4), maps), "updateVolume on a relocated handle: the maps"
    assert same(read("image.bin", np.float32, 4), image.reshape(-1, 4)), "renderIrradiance on a relocated handle"
    assert not same(image, plain_image) and (image[..., 3] > 0).mean() > 0.5
    # bakeVolume(grid, { relocate }) relocates from zeros and bakes from the moved positions
    assert same(read("baked_offsets.bin", np.float32, 4), offsets), "bakeVolume({ relocate }).offsets()"
    assert same(read("baked_rows.bin", np.float32, 36), baked[0]), "bakeVolume({ relocate }).rows()"


def test_type_errors_and_the_librarys_words(tmp_path):
    node = shutil.which("node")
    script = tmp_path / "refused.js"
    script.write_text("""
const path = require('path');
const { FlexLight, Transform } = require(path.join(%r, 'web-ray-tracer_amd', 'js', 'flexlight.js'));
const scenes = require(path.join(%r, 'web-ray-tracer_amd', 'js', 'scenes', 'index.js'));
(async () => {
  Transform.reset();
  const log = console.log; console.log = () => {};
  const engine = new FlexLight({ width: 16, height: 16 }, { assetRoot: '/nonexistent' });
  await scenes.cornell(engine);
  console.log = log;
  engine.renderer = 'pathtracer';
  const renderer = engine.renderer;
  await renderer.updateScene();
  const volume = renderer.bakeVolume({ origin: [0, 0, 0], spacing: [1, 1, 1], count: [2, 1, 1] }, { faceSize: 1, samples: 1, maxReflections: 1 });
  const good = { minFront: 0.1, reach: 20, iterations: 1, faceSize: 1 };
  const said = [];
  const tries = [[{}, good], [volume, { reach: 20 }], [volume, { minFront: 0.1 }], [volume, Object.assign({}, good, { iterations: 1.5 })], [volume, Object.assign({}, good, { iterations: 65 })],
    [volume, Object.assign({}, good, { backShare: 1.5 })], [volume, Object.assign({}, good, { minFront: -1 })], [volume, Object.assign({}, good, { reach: 0 })],
    [volume, Object.assign({}, good, { limit: 0.75 })], [volume, Object.assign({}, good, { faceSize: 0 })], [volume, Object.assign({}, good, { faceSize: 257 })]];
  for (const [v, o] of tries) {
    try { renderer.relocateVolume(v, o); said.push('accepted'); } catch (e) { said.push((e instanceof TypeError ? 'TypeError: ' : e instanceof RangeError ? 'RangeError: ' : 'Error: ') + String(e.message)); }
  }
  const untouched = volume.offsets === undefined;
  const got = renderer.relocateVolume(volume, good);
  console.log(JSON.stringify({ said, untouched, offsets: got.offsets.length, states: got.states.length, has: typeof volume.offsets === 'function' }));
  renderer.halt();
})().catch(e => { console.error(e); process.exit(1); });
""" % (ROOT, ROOT))
    got = json.loads(subprocess.check_output([node, str(script)], timeout=300).decode().splitlines()[-1])
    said = got["said"]
    assert said[0].startswith("TypeError: relocateVolume: volume is what bakeVolume returned"), said
    assert said[1].startswith("TypeError: relocateVolume: minFront is a number") and said[2].startswith("TypeError: relocateVolume: reach is a number"), said
    assert all(s.startswith("RangeError: relocateVolume: iterations is a whole number") for s in said[3:5]), said
    assert "back_share is not one of 0 .. 1" in said[5] and "min_front is negative or not finite" in said[6] and "reach is not greater than 0 or not finite" in said[7], said
    assert "limit is not one of 0 .. 0.5" in said[8] and "face_size is not one of 1 .. 256" in said[9] and "face_size is not one of 1 .. 256" in said[10], said
    assert got["untouched"] and got["offsets"] == 8 and got["states"] == 2 and got["has"]      # a refused first call leaves the handle without offsets
