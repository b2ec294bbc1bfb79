"""The JavaScript host layer (web-ray-tracer_amd/js): the arrays it flattens for the GPU must equal what
the reference's own modules/scene.js emits (tests/golden/ref_<scene>.json holds their sha256, produced
by tools/ref_goldens.js from the reference itself), and the N-API addon must load and export the
renderer's entry points.  CPU only.  The OBJ / MTL assets the scenes import are the reference's own files, stored gzipped
under tests/golden/assets and unpacked into a temporary asset root for the module; the theater's texture is stored as the
pixels of it that its atlas reads (tests/analysis/make_texture_fixture.py)."""
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "tests", "golden", "assets")
# fixture -> the asset it stands in for: lossless, full size, black where the 512 x 512 atlas cell reads nothing
# (tools/host_arrays.js decodes images with PIL, which goes by the file's content, not its name)
STANDS_IN = {"holz_sampled.png": "holz.jpg"}
NODE = shutil.which("node")
sys.path.insert(0, os.path.join(ROOT, "web-ray-tracer_amd"))
from flexlight_hip.scene_io import Scene  # noqa: E402

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    """tests/golden/assets unpacked: <root>/objects/*.obj|*.mtl, <root>/textures/holz.jpg, as the scenes name them"""
    root = tmp_path_factory.mktemp("assets")
    for sub in sorted(os.listdir(ASSETS)):
        os.makedirs(str(root / sub))
        for name in sorted(os.listdir(os.path.join(ASSETS, sub))):
            src = os.path.join(ASSETS, sub, name)
            if name.endswith(".gz"):
                with gzip.open(src, "rb") as fin, open(str(root / sub / name[:-3]), "wb") as fout:
                    shutil.copyfileobj(fin, fout)
            else:
                shutil.copyfile(src, str(root / sub / STANDS_IN.get(name, name)))
    return str(root)


def host_arrays(scene, native=False, assets=None):
    cmd = [NODE, os.path.join(ROOT, "tools", "host_arrays.js"), scene] + (["--assets", assets] if assets else []) + (["--native"] if native else [])
    out = subprocess.check_output(cmd, timeout=300)
    return json.loads(out.decode().strip().splitlines()[-1])


def golden(scene):
    with open(os.path.join(ROOT, "tests", "golden", "ref_%s.json" % scene)) as fh:
        return json.load(fh)


def check(scene, native=False, assets=None):
    got, want = host_arrays(scene, native, assets), golden(scene)
    for key in ("textureLength", "bufferLength", "entriesPadded", "transforms"):
        assert got[key] == want[key], key
    for key, digest in want["sha256"].items():
        assert got["sha256"][key] == digest, "%s: array '%s' differs from the reference's" % (scene, key)
    stored = Scene.golden(scene)              # the texture atlases, against the scene file the reference's scene.js emitted
    for key in ("atlasAlbedo", "atlasPbr", "atlasTpo"):
        assert got["sha256"][key] == hashlib.sha256(stored.arrays[key].tobytes()).hexdigest(), "%s: atlas '%s' differs from the reference's" % (scene, key)


def test_cornell_arrays_equal_reference():
    check("cornell")                       # built purely through the API: no asset files needed


@pytest.mark.parametrize("scene", ["cornell_obj", "dragon", "theater"])
def test_imported_scene_arrays_equal_reference(scene, assets):
    check(scene, assets=assets)            # OBJ/MTL import + BVH builder + transforms


@pytest.mark.parametrize("scene", ["cornell_obj", "dragon"])
def test_native_import_arrays_equal_reference(scene, assets):
    """OBJ / MTL parsing, BVH build and flattening in native code (flx_mesh_* through the N-API addon),
    spliced into the JavaScript scene, and N3: the transform arrays from flx_transforms_pack — the whole scene still hashes to
    what the reference's own scene.js emits."""
    check(scene, native=True, assets=assets)


@pytest.mark.parametrize("native", [False, True], ids=["js_host", "native_import"])
def test_synthetic_100k_dragon_arrays_equal_reference(native, assets):
    """The >= 100k-triangle stand-in for the absent objects/dragon.obj (tools/make_dragon_100k.py: dragon_lp.obj split 1 -> 4,
    174 276 triangles): the scene built from it by the JavaScript host layer, and by the native importer, hashes to the arrays
    the reference's own scene.js emits for the same OBJ (tests/golden/ref_dragon_100k.json) — 289 189 entries."""
    if not os.path.exists(os.path.join(assets, "objects", "dragon_100k.obj")):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dragon_100k.py"), assets, assets])
    check("dragon_100k", native, assets)
    assert golden("dragon_100k")["triangles"] >= 100000


def test_golden_scene_file_matches_its_hashes():
    """The .flxs fixtures the GPU tests and bench.py load are the arrays the hashes describe."""
    import hashlib
    import sys
    sys.path.insert(0, os.path.join(ROOT, "web-ray-tracer_amd"))
    from flexlight_hip.scene_io import Scene
    for scene in ("cornell", "cornell_obj", "dragon", "theater", "dragon_100k"):
        sc, want = Scene.golden(scene), golden(scene)
        for key, digest in want["sha256"].items():
            assert hashlib.sha256(sc.arrays[key].tobytes()).hexdigest() == digest, (scene, key)
        assert sc.meta["textureLength"] == want["textureLength"]


def test_linalg_matches_known_values():
    js = """
const la = require('%s/web-ray-tracer_amd/js/linalg.js');
const out = { snap: [la.snap(2 + 1e-11), la.snap(2.5), la.snap(-3 - 1e-12)],
  unit: la.unit([3, 0, 4]), cross: la.cross([1, 0, 0], [0, 1, 0]),
  inv: la.pseudoInverse([[2, 0, 0], [0, 2, 0], [0, 0, 2]]), zero: la.unit([0, 0, 0]) };
console.log(JSON.stringify(out));""" % ROOT
    out = json.loads(subprocess.check_output([NODE, "-e", js]).decode())
    assert out["snap"] == [2, 2.5, -3]
    assert out["unit"] == [0.6, 0, 0.8] and out["cross"] == [0, 0, 1] and out["zero"] == [0, 0, 0]
    assert out["inv"] == [[0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5]]


def test_napi_addon_loads_and_exports():
    addon = os.path.join(ROOT, "web-ray-tracer_amd", "napi", "flexlight_napi.node")
    if not os.path.exists(addon):
        pytest.skip("addon not built (run __graft_entry__.build())")
    js = "const a = require('%s'); console.log(JSON.stringify({keys: Object.keys(a), version: a.version()}));" % addon
    out = json.loads(subprocess.check_output([NODE, "-e", js]).decode())
    for name in ("createContext", "destroyContext", "uploadScene", "uploadTransforms", "uploadLights", "uploadAtlas", "tileRowCount", "render", "renderBatch",
                 "meshImport", "meshCounts", "meshSetTransform", "meshMove", "meshScale", "meshSetMaterial", "meshBounding", "meshFlatten", "packTransforms", "fxaa", "taa", "taaReset", "present"):
        assert name in out["keys"]
    assert "flexlight-hip" in out["version"]


def test_renderer_object_has_the_reference_surface():
    """Members FlexLight expects of a renderer (reference modules/pathtracerWGL2.js:25-78,143,167,191)."""
    js = """
const fl = require('%s/web-ray-tracer_amd/js/flexlight.js');
const e = new fl.FlexLight({width: 16, height: 16});
e.renderer = 'pathtracer';
const r = e.renderer;
console.log(JSON.stringify({ type: r.type, fps: r.fps, fpsLimit: r.fpsLimit === Infinity,
  fns: ['render', 'halt', 'updateScene', 'updatePrimaryLightSources', 'renderFrame'].map(n => typeof r[n]),
  shared: r.config === e.config && r.camera === e.camera && r.scene === e.scene, canvas: r.canvas.width,
  api: e.api, exportsOk: ['Scene','Transform','Primitive','Triangle','Plane','Object3D','Cuboid','Bounding'].every(n => typeof fl[n] === 'function') }));""" % ROOT
    out = json.loads(subprocess.check_output([NODE, "-e", js]).decode())
    assert out["type"] == "pathtracer" and out["fpsLimit"] and out["shared"] and out["canvas"] == 16
    assert out["fns"] == ["function"] * 5 and out["exportsOk"] and out["api"] == "hip"
