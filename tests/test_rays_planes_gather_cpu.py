"""Ray images with a volume, without a GPU: the CPU reference (tests/rays_planes_gather_ref) is pinned before anything is held against it.  Where the volume has
nothing to say its planes are flx_rays_planes_ref's — the oracle's own lightTrace —; at one sample its colour is the gathered batches' radiance, the other
restatement of the same definition; its inputs are shown to exercise every class of sample; the calls are declared, exported and bound.  Every comparison is bit for
bit."""
import os

import numpy as np
import pytest

import rays_gather_util
import rays_planes_util
from rays_planes_gather_util import (CONSTANT, GAIN, LIT, NO_POINT, assert_floats, edge_inactive_offsets, half_grid, image_rays, inactive_offsets, reference, same_floats,
                                     spanning_grid, trace_params, wanted)
from volume_map_util import map_of, synthetic_maps
from volume_util import synthetic_sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("flx_rays_planes_gather_device", "flx_rays_planes_gather", "flx_rays_image_gather_device", "flx_rays_image_gather", "flx_rays_image_temporal_gather_device",
         "flx_rays_image_temporal_gather", "flx_camera_image_gather_device", "flx_camera_image_gather", "flx_camera_image_temporal_gather_device",
         "flx_camera_image_temporal_gather", "flx_debug_last_planes_gather")


@pytest.mark.parametrize("bounces", (0, 1, 3))
@pytest.mark.parametrize("samples", (1, 3))
@pytest.mark.parametrize("name", ("cornell", "dragon"))
def test_an_inactive_volume_gives_the_plain_planes(oracle, scenes, tmp_path_factory, name, samples, bounces):
    """every offset row inactive: W = 0 everywhere, every A is the params' ambient, and the five planes are flx_rays_planes_ref's bit for bit"""
    ref, plain = reference(tmp_path_factory), rays_planes_util.reference(tmp_path_factory)
    sc, rays, points = image_rays(oracle, scenes, name)
    grid = spanning_grid(points)
    sh, offsets = synthetic_sh(grid.probes, 3), inactive_offsets(grid.probes)
    t = trace_params(sc, samples, bounces)
    want, want_hit = rays_planes_util.wanted(plain, ("planes_gather", name, samples, bounces), sc, t, rays)
    assert want_hit.any()
    for vmap, maps in ((None, None), (map_of(4, 2), synthetic_maps(grid.probes, 4, 5))):
        got, hit, colour, classes = ref.planes(sc, t, rays, grid, sh, GAIN, vmap=vmap, maps=maps, offsets=offsets, details=True)
        assert np.array_equal(hit, want_hit)
        assert_floats(got, want, "%s S %d K %d map %s" % (name, samples, bounces, vmap is not None))
        assert (classes[hit] == (CONSTANT if bounces else NO_POINT)).all() and (classes[~hit] == 0).all()


def live_case(oracle, scenes, tmp_path_factory, name, samples, bounces, importancy=None):
    """the reference's planes with a volume that is live over half of the scene -> (scene, params, rays, grid, sh, offsets, planes, hit, colour, classes)"""
    ref = reference(tmp_path_factory)
    sc, rays, points = image_rays(oracle, scenes, name)
    grid = half_grid(points)
    sh, offsets = synthetic_sh(grid.probes, 7), edge_inactive_offsets(grid)
    t = trace_params(sc, samples, bounces, importancy)
    out = wanted(("cpu live", name, samples, bounces, importancy), lambda: ref.planes(sc, t, rays, grid, sh, GAIN, offsets=offsets, details=True))
    return (sc, t, rays, grid, sh, offsets) + out


@pytest.mark.parametrize("bounces", (1, 2, 4))
@pytest.mark.parametrize("name", ("cornell", "dragon"))
def test_one_sample_is_the_gathered_batch(oracle, scenes, tmp_path_factory, name, bounces):
    """samples == 1, a live volume: float32(c * plane2.rgb) — the mean times originalColor, which is what a radiance row holds — equals words 0 to 2 of
    flx_rays_gather_ref's rows bit for bit: the two restatements agree where their definitions coincide"""
    batches = rays_gather_util.reference(tmp_path_factory)
    sc, t, rays, grid, sh, offsets, planes, hit, colour, classes = live_case(oracle, scenes, tmp_path_factory, name, 1, bounces)
    rows = batches.gather(sc, t, rays, grid, sh, GAIN, offsets=offsets)
    assert np.array_equal(rows[:, 5] != 0xffffffff, hit) and hit.any()
    product = (colour * planes[2, :, 0:3]).astype(np.float32)
    assert same_floats(product[hit], rows[hit, 0:3].view(np.float32)).all()
    assert (classes[hit] == LIT).any()


def test_the_inputs_exercise_every_class(oracle, scenes, tmp_path_factory):
    """computed from the reference: at least a quarter of the hit rays have a plane-0 or plane-1 row that differs from the plain planes'; a sample that is lit, one
    that takes the constant because W is not > 0 and one without a last point (min_importancy > 1) all occur; last points fall inside and beside the grid"""
    plain = rays_planes_util.reference(tmp_path_factory)
    seen = set()
    for name, samples, bounces, importancy in (("cornell", 3, 3, None), ("dragon", 3, 2, None), ("cornell", 2, 3, 1.5)):
        sc, t, rays, grid, sh, offsets, planes, hit, colour, classes = live_case(oracle, scenes, tmp_path_factory, name, samples, bounces, importancy)
        seen |= set(np.unique(classes[hit]).tolist())
        if importancy is not None:
            assert (classes[hit] == NO_POINT).all()
            continue
        want, _ = rays_planes_util.wanted(plain, ("planes_gather live", name, samples, bounces), sc, t, rays)
        differs = (~same_floats(planes[0:2], want[0:2])).any(axis=(0, 2))
        print(name, "hit", int(hit.sum()), "rows that differ", int(differs[hit].sum()), "lit", int((classes == LIT).sum()), "constant", int((classes == CONSTANT).sum()))
        assert differs[hit].mean() >= 0.25 and not differs[~hit].any()
        assert_floats(planes[2:5], want[2:5], name + ": planes 2 to 4 do not see the volume")
        assert (classes[hit] == LIT).any() and (classes[hit] == CONSTANT).any()
    assert seen == {LIT, CONSTANT, NO_POINT}


def test_the_calls_are_declared_exported_and_bound():
    from flexlight_hip import capi
    header = open(os.path.join(ROOT, "include", "flexlight_hip_debug.h")).read()
    for call in CALLS:
        assert call + "(" in header and call in capi.EXPORTS and hasattr(capi.LIB, call)
    assert "frames, filter planes and ray images do not take a volume" not in header and "ray images with a volume" in header
    for bound in ("gather_volume", "ray_planes_gather_device", "ray_planes_gather", "ray_image_gather_device", "ray_image_gather", "rays_image_temporal_gather",
                  "camera_image_gather_device", "camera_image_gather", "camera_image_temporal_gather_device", "camera_image_temporal_gather", "last_planes_gather"):
        assert callable(getattr(capi.Context, bound))
