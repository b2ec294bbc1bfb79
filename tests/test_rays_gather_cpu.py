"""Traced batches with a volume, without a GPU: the CPU reference (tests/rays_gather_ref) is pinned before anything is held against it.  It carries a restatement of
the oracle's lightTrace, so it is held against the oracle's own (tests/rays_trace_ref) where the volume has nothing to say and where it says zero; its last points
are held against the surface reference's rows; the calls are declared, exported and bound; and the argument checks that need no device
(csrc/flx_gather_args.h) hold in a stand-alone program under the address and undefined-behaviour sanitizers.  Every comparison is bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rays_trace_util
import surface_util
from rays_gather_util import GAIN, assert_rows, inactive_offsets, pinhole_rays, reference, small_grid, spanning_grid, trace_params
from volume_map_util import map_of, synthetic_maps
from volume_util import synthetic_sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ("cornell", "cornell_obj", "dragon", "theater")
CALLS = ("flx_rays_trace_gather_device", "flx_rays_trace_gather", "flx_debug_last_gather")
# samples, max_reflections, min_importancy (None: the scene's): S in {1, 3} x bounces in {0, 1, 4}, and one threshold high enough that paths end on the loop guard
PARAMS = ((1, 0, None), (3, 0, None), (1, 1, None), (3, 1, None), (1, 4, None), (3, 4, None), (3, 4, 0.8))


@pytest.mark.parametrize("name", SCENES)
def test_the_restatement_is_the_oracles_light_trace(oracle, scenes, tmp_path_factory, name):
    """every offset row inactive: W = 0 everywhere, every A is the params' ambient, and the rows are flx_rays_trace_ref's — the oracle's own lightTrace — bit for bit"""
    ref, plain = reference(tmp_path_factory), rays_trace_util.reference(tmp_path_factory)
    sc, rays, points = pinhole_rays(oracle, scenes, name)
    grid = spanning_grid(points)
    sh, offsets = synthetic_sh(grid.probes, 3), inactive_offsets(grid.probes)
    ended_on_guard = False
    for samples, bounces, importancy in PARAMS:
        p = trace_params(sc, samples, bounces, importancy)
        want = plain.trace(sc, p, rays)
        for vmap, maps in ((None, None), (map_of(4, 2), synthetic_maps(grid.probes, 4, 5))):
            got = ref.gather(sc, p, rays, grid, sh, GAIN, vmap=vmap, maps=maps, offsets=offsets)
            assert_rows(got, want, "%s S %d K %d min %s map %s" % (name, samples, bounces, importancy, vmap is not None))
        if importancy is not None:
            full = plain.trace(sc, trace_params(sc, samples, bounces), rays)
            ended_on_guard = bool((want[:, 7] < full[:, 7]).any())
    assert ended_on_guard, "min_importancy 0.8 ends no path of %s on the loop guard" % name


@pytest.mark.parametrize("name", ("cornell", "dragon"))
def test_a_volume_of_zeros_is_an_ambient_of_zero(oracle, scenes, tmp_path_factory, name):
    """all-zero SH rows on the lattice, visibility off: every path that shaded has W > 0 and E = 0, so the rows are flx_rays_trace_ref's with ambient (0, 0, 0) — and
    not its rows with the scene's ambient, which the test needs to be different"""
    ref, plain = reference(tmp_path_factory), rays_trace_util.reference(tmp_path_factory)
    sc, rays, points = pinhole_rays(oracle, scenes, name)
    for grid in (spanning_grid(points, visibility=False), small_grid(points, visibility=False)):
        sh = np.zeros((grid.probes, 36), np.float32)
        for samples, bounces in ((1, 1), (3, 2)):
            p = trace_params(sc, samples, bounces, ambient=(0.25, 0.5, 0.75))
            got, records, lookups = ref.gather(sc, p, rays, grid, sh, GAIN, records=True)
            hit = got[:, 5] != 0xffffffff
            assert hit.any() and (records[hit, :, 11] == 1.0).all() and (lookups[hit, :, 3] > 0.0).all() and (lookups[hit, :, 0:3] == 0.0).all()
            assert_rows(got, plain.trace(sc, trace_params(sc, samples, bounces, ambient=(0.0, 0.0, 0.0)), rays), "%s S %d K %d" % (name, samples, bounces))
            assert not rays_trace_util.same_rows(got, plain.trace(sc, p, rays))[hit].all()


@pytest.mark.parametrize("name", ("cornell", "dragon"))
def test_the_last_point_is_the_surface_rows(oracle, scenes, tmp_path_factory, name):
    """max_reflections = 1, one sample: the one iteration's x and n are the FLX_SURFACE_POSITION and FLX_SURFACE_NORMAL rows of the surface reference for the same
    rays, bit for bit; hence the looked-up E is flx_volume_irradiance_of of those rows"""
    from flexlight_hip import capi
    ref, surface = reference(tmp_path_factory), surface_util.reference(tmp_path_factory)
    sc, rays, points = pinhole_rays(oracle, scenes, name)
    grid = spanning_grid(points)
    sh = synthetic_sh(grid.probes, 7)
    p = trace_params(sc, 1, 1)
    rows, records, lookups = ref.gather(sc, p, rays, grid, sh, GAIN, records=True)
    planes = surface.rays(sc, rays, p.texture_width)
    hit = rows[:, 5] != 0xffffffff
    assert hit.any()
    rec = records[:, 0].view(np.uint32)
    assert (rec[hit, 8:11] == planes[surface_util.POSITION][hit, 0:3]).all() and (records[hit, 0, 11] == 1.0).all()
    assert (rec[hit, 12:15] == planes[surface_util.NORMAL][hit, 0:3]).all()
    assert (rec[~hit] == 0).all()
    position, normal = planes[surface_util.POSITION][hit].view(np.float32), planes[surface_util.NORMAL][hit].view(np.float32)
    assert (position[:, 3] == 1.0).all()
    want = capi.volume_irradiance_of(grid, sh, position, normal)
    assert (lookups[hit, 0].view(np.uint32) == want.view(np.uint32)).all() and (want[:, 3] > 0.0).any()


def test_no_last_point_without_a_bounce(oracle, scenes, tmp_path_factory):
    """max_reflections = 0, and a threshold above 1: the loop guard fails before bounce 0, no path has a last point, every A is the constant"""
    ref, plain = reference(tmp_path_factory), rays_trace_util.reference(tmp_path_factory)
    sc, rays, points = pinhole_rays(oracle, scenes, "cornell")
    grid = spanning_grid(points)
    sh = synthetic_sh(grid.probes, 7)
    for bounces, importancy in ((0, None), (4, 1.5)):
        p = trace_params(sc, 3, bounces, importancy)
        rows, records, lookups = ref.gather(sc, p, rays, grid, sh, GAIN, records=True)
        assert (records[:, :, 11] == 0.0).all() and (lookups == 0.0).all() and (rows[:, 7] == 0).all()
        assert_rows(rows, plain.trace(sc, p, rays), "K %d min %s" % (bounces, importancy))


def test_the_calls_are_declared_exported_and_bound():
    from flexlight_hip import capi
    header = open(os.path.join(ROOT, "include", "flexlight_hip_debug.h")).read()
    for call in CALLS:
        assert call + "(" in header and call in capi.EXPORTS and hasattr(capi.LIB, call)
    assert "typedef struct flx_gather_volume" in header
    import ctypes as C
    assert C.sizeof(capi.GatherVolume) == 5 * C.sizeof(C.c_void_p) + 8
    assert np.float32(capi.GATHER_GAIN) == np.float32(1.0 / np.pi)
    for bound in ("trace_rays_gather_device", "trace_rays_gather", "last_gather"):
        assert callable(getattr(capi.Context, bound))


def test_argument_checks_in_a_stand_alone_program_under_the_sanitizers(tmp_path):
    """every refusal of flx_gather_args.h and the accepted borders — gain 0, gain FLT_MAX, a map without maps, each array against the rays and the radiance — and the
    slab rule, with a main of their own, built with -fsanitize=address,undefined, run directly"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is part of the image (the oracle is built with gcc)"
    exe = tmp_path / "gather_args"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "web-ray-tracer_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "gather_args_main.cc"), "-o", str(exe)])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) >= 60
