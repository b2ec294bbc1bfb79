"""flx_textures_upload / flx_texture_update without a GPU: the numpy restatement of the atlas rule (tests/textures_util.py) held against the project's own
definition, sceneFile.buildAtlas, run under Node; the argument rules (csrc/flx_texture_args.h) in a stand-alone program under the sanitizers; the exports and
their bindings."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import textures_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("source,cell", tu.SIZE_PAIRS)
def test_the_numpy_atlas_is_build_atlas_of_the_javascript(tmp_path, source, cell):
    """random images of the source size, n = 1, tw and tw + 1 of them: buildAtlas under Node and textures_util.build_atlas give the same bytes (this one
    passes without the feature: it pins the yardstick the GPU tests use)"""
    node = shutil.which("node")
    assert node, "node is part of the image"
    rng = np.random.default_rng(source[0] * 131 + cell[0])
    tw = tu.cells_per_row(cell[0])
    images = [tu.random_image(rng, source) for _ in range(tw + 1)]
    files = []
    for k, image in enumerate(images):
        files.append(str(tmp_path / ("image%d.rgba" % k)))
        image.tofile(files[-1])
    for n in (1, tw, tw + 1):
        spec = {"cell": list(cell), "out": str(tmp_path / "atlas.rgba"),
                "images": [{"width": source[0], "height": source[1], "file": f} for f in files[:n]]}
        with open(tmp_path / "spec.json", "w") as fh:
            json.dump(spec, fh)
        info = json.loads(subprocess.check_output([node, os.path.join(ROOT, "tests", "textures_build_atlas.js"), str(tmp_path / "spec.json")], timeout=120).decode())
        want = np.fromfile(spec["out"], np.uint8).reshape(info["height"], info["width"], 4)
        got = tu.build_atlas(images[:n], cell)
        assert got.shape == want.shape == (cell[1] * n, cell[0] * tw, 4)
        assert np.array_equal(got, want), "n = %d" % n


def test_quantise_is_the_render_targets_rule():
    """textures_util.quantise against floor(clamp(x, 0, 1) * 255 + 0.5) in exact arithmetic wherever float32 rounding cannot matter, and its special values"""
    values = tu.float_edges()
    got = tu.quantise(values)
    assert got.dtype == np.uint8 and got.shape == values.shape
    k = np.arange(256)
    assert np.array_equal(tu.quantise((k / 255.0).astype(np.float32)), k.astype(np.uint8))
    assert list(tu.quantise(np.array([-0.0, -1.0, -np.inf, np.nan, 0.0, 1e-45], np.float32))) == [0] * 6
    assert list(tu.quantise(np.array([1.0, 2.0, np.inf, 3.4e38], np.float32))) == [255] * 4
    finite = np.isfinite(values)
    exact = np.floor(np.clip(values[finite].astype(np.float64), 0.0, 1.0) * 255.0 + 0.5)
    assert np.abs(got[finite].astype(np.float64) - exact).max() <= 1      # (a value a float32 ulp from a boundary may round across it: by one at most)


def test_argument_rules_in_a_stand_alone_program_under_the_sanitizers(tmp_path):
    """every refusal of flx_texture_args.h and their order, the images' byte counts and the atlas rule's integers, with a main of their own, built with
    -fsanitize=address,undefined and run directly"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is part of the image (the oracle is built with gcc)"
    exe = tmp_path / "texture_args"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "web-ray-tracer_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "texture_args_main.cc"), "-o", str(exe)])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) >= 20000


def test_the_library_exports_the_calls_and_capi_binds_them():
    from flexlight_hip import capi
    names = ["flx_textures_upload", "flx_textures_upload_device", "flx_texture_update", "flx_texture_update_device", "flx_group_textures_upload",
             "flx_group_texture_update", "flx_debug_atlas_read"]
    for name in names:
        assert name in capi.EXPORTS and hasattr(capi.LIB, name), name
        assert getattr(capi.LIB, name).argtypes is not None, name
    for method in ("upload_textures", "upload_textures_device", "update_texture", "update_texture_device", "atlas_read"):
        assert callable(getattr(capi.Context, method))
    for method in ("upload_textures", "update_texture"):
        assert callable(getattr(capi.Group, method))
    assert (capi.IMAGE_RGBA8, capi.IMAGE_RGBA32F) == (0, 1)
    header = open(os.path.join(ROOT, "include", "flexlight_hip_debug.h")).read()
    for name in names:
        assert name + "(" in header, name


def test_the_bindings_refuse_what_is_no_image():
    """what capi says itself, before the library is asked: no context is needed"""
    from flexlight_hip import capi
    ctx = capi.Context.__new__(capi.Context)
    ctx._h, ctx._device = None, 0
    with pytest.raises(ValueError, match=r"\[h, w, 4\]"):
        ctx.upload_textures(0, [np.zeros((4, 4, 3), np.uint8)], (16, 16))
    with pytest.raises(ValueError, match="uint8 or float32"):
        ctx.update_texture(0, 0, np.zeros((4, 4, 4), np.float64))
    with pytest.raises(TypeError, match="torch tensor or"):
        ctx.upload_textures_device(0, [np.zeros((4, 4, 4), np.uint8)], (16, 16))
    arr, keep = capi._host_images([np.zeros((3, 5, 4), np.uint8), np.zeros((2, 7, 4), np.float32)[:, ::1]], "upload_textures")
    assert (arr[0].width, arr[0].height, arr[0].format) == (5, 3, capi.IMAGE_RGBA8) and (arr[1].width, arr[1].height, arr[1].format) == (7, 2, capi.IMAGE_RGBA32F)
    assert arr[0].pixels == keep[0].ctypes.data
