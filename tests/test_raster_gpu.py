"""The rasterizer renderer on the GPU (flx_raster_render, k_raster) against its CPU reference (tests/raster_ref) bit for bit: frame
and work counters, on the four golden scenes, synthetic scenes, edge sizes, tile strips and two full-size frames."""
import os
import sys

import numpy as np
import pytest

import synth_scene
from raster_stacks_util import assert_same

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "raster_ref"))
import flx_raster_ref  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = ["cornell", "cornell_obj", "theater", "dragon"]


@pytest.fixture(scope="module")
def ref(oracle, tmp_path_factory):
    return flx_raster_ref.build(str(tmp_path_factory.mktemp("raster_ref")))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("hdr", [0, 1])
@pytest.mark.parametrize("size", [(64, 48), (96, 54)], ids=["64x48", "96x54"])
@pytest.mark.parametrize("name", GOLDEN)
def test_golden_scene_matches_reference(hip, ref, scenes, name, size, hdr):
    sc = scenes(name)
    hip.update_scene(sc)
    p = sc.frame_params(width=size[0], height=size[1], hdr=hdr)
    got, cnt = assert_same(hip, ref, sc, p, "%s %dx%d hdr %d" % (name, size[0], size[1], hdr))
    assert cnt["primary_hits"] > 0 and cnt["shades"] >= cnt["primary_hits"]
    assert cnt["closest_visits"] == 0 and cnt["closest_walks"] == 0
    # every value is a byte of the RGBA8 buffer: flx_present maps k / 255 back to k
    k = np.rint(got * 255.0)
    assert np.array_equal(k.astype(np.float32) / np.float32(255.0), got)
    assert np.array_equal(hip.present(got), k.astype(np.uint8))


SYNTH = {
    "many_transforms": dict(seed=11, n_objects=9, tris_per_object=24, n_transforms=9, n_lights=2),
    "no_lights": dict(seed=12, n_objects=3, tris_per_object=40, n_transforms=2, n_lights=0),
    "zero_strength_lights": dict(seed=13, n_objects=4, tris_per_object=30, n_transforms=3, n_lights=3),
    "degenerate_untextured": dict(seed=14, n_objects=2, tris_per_object=30, n_transforms=1, n_lights=1, textured=False, degenerate=6),
    "no_terminator": dict(seed=15, n_objects=3, tris_per_object=50, n_transforms=3, n_lights=1, exact_multiple=True),
    "axis_aligned": dict(seed=16, n_objects=3, tris_per_object=30, n_transforms=2, n_lights=2, axis_aligned_view=True, width=65, height=33),
}


@pytest.mark.parametrize("hdr", [0, 1])
@pytest.mark.parametrize("case", sorted(SYNTH))
def test_synthetic_scene_matches_reference(hip, ref, case, hdr):
    sc = synth_scene.make(**SYNTH[case])
    if case == "zero_strength_lights":
        lights = sc.arrays["lights"].reshape(-1, 6)
        lights[1, 3] = 0.0
        lights[2, 3] = -5.0
    hip.update_scene(sc)
    p = sc.frame_params(hdr=hdr)
    got, cnt = assert_same(hip, ref, sc, p, case)
    assert cnt["primary_hits"] > 0
    if case in ("no_lights",):
        assert cnt["shadow_walks"] == 0


def test_all_miss_frame_is_zero(hip, ref, scenes):
    sc = scenes("cornell")
    hip.update_scene(sc)
    p = sc.frame_params(width=40, height=24)
    p.camera[:] = [0.0, 0.0, 1.0e4]                       # far behind the box, looking further away (+z)
    p.view_matrix[:] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    got, cnt = assert_same(hip, ref, sc, p, "all miss")
    assert not got.any()
    assert cnt["primary_hits"] == 0 and cnt["shades"] == 0 and cnt["primary_visits"] > 0


@pytest.mark.parametrize("size", [(1, 1), (13, 7), (67, 35)], ids=["1x1", "13x7", "67x35"])
def test_odd_sizes(hip, ref, scenes, size):
    sc = scenes("theater")
    hip.update_scene(sc)
    assert_same(hip, ref, sc, sc.frame_params(width=size[0], height=size[1]), "theater %dx%d" % size)


@pytest.mark.parametrize("tile", [(8, 0, 3), (8, 2, 3), (5, 1, 2), (16, 6, 7)])
def test_tile_strips_equal_the_whole_frames_rows(hip, ref, scenes, tile):
    sc = scenes("dragon")
    hip.update_scene(sc)
    whole, _ = hip.raster_render(sc.frame_params(width=72, height=90))
    p = sc.frame_params(width=72, height=90, tile=tile)
    strip, _ = assert_same(hip, ref, sc, p, "strip %s" % (tile,))
    rows = hip.tile_rows(p)
    assert strip.shape[0] == len(rows)
    assert np.array_equal(_bits(strip), _bits(whole[rows]))


def test_device_output_equals_host_output(hip, scenes):
    torch = pytest.importorskip("torch")
    sc = scenes("cornell_obj")
    hip.update_scene(sc)
    p = sc.frame_params(width=80, height=45)
    host, _ = hip.raster_render(p)
    buf = torch.zeros((45, 80, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    hip.raster_render_device(p, buf.data_ptr())
    hip.sync()
    assert np.array_equal(_bits(buf.cpu().numpy()), _bits(host))
    ms, _ = hip.last_frame_ms()
    assert ms > 0.0


def test_exactly_one_output(hip, scenes):
    import ctypes as C
    from flexlight_hip import capi
    sc = scenes("cornell")
    hip.update_scene(sc)
    p = sc.frame_params(width=8, height=8)
    out = np.zeros((8, 8, 4), np.float32)
    assert capi.LIB.flx_raster_render(hip._h, C.byref(p), None, None, None) == 1
    assert capi.LIB.flx_raster_render(hip._h, C.byref(p), capi._fp(out), C.c_void_p(out.ctypes.data), None) == 1


@pytest.mark.parametrize("name", ["dragon", "theater"])
def test_full_size_frame(hip, ref, scenes, name):
    sc = scenes(name)
    hip.update_scene(sc)
    p = sc.frame_params()
    assert (p.width, p.height) == (1920, 1080)
    got, cnt = assert_same(hip, ref, sc, p, "%s 1080p" % name)
    if name == "dragon":                                   # translucent layers: more fragments shaded than pixels covered
        assert cnt["shades"] > cnt["primary_hits"]


def test_kernel_equals_the_literal_known_answers(hip, scenes):
    """tests/golden/raster_kat.json.gz (tests/analysis/make_raster_kat.py: main(), lookup() and the blend from the shader text): k_raster's pixels
    equal the literal pixels bit for bit, with the table's lights (zero-strength ones included) and hdr"""
    import copy
    import gzip
    import json
    data = json.load(gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raster_kat.json.gz"), "rt"))
    for case in data["cases"]:
        sc = copy.copy(scenes(case["scene"]))
        sc.arrays = dict(sc.arrays, lights=np.array(case["lights"], np.uint32).view(np.float32))
        hip.update_scene(sc)
        got, _ = hip.raster_render(sc.frame_params(width=case["width"], height=case["height"], hdr=case["hdr"]))
        for r in case["pixels"]:
            px, py_gl = r[0], r[1]
            assert list(_bits(got[case["height"] - 1 - py_gl, px])) == r[3:7], (case["scene"], case["hdr"], px, py_gl)
