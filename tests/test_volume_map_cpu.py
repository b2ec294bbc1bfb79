"""Directional visibility without a GPU (include/flexlight_hip_debug.h, "directional visibility"; include/flx_volume_map.h): the CPU reference the GPU tests compare
against is itself held against float64 restatements written by hand and against the properties an octahedral moment map must have — among them the wall that the
isotropic weight leaks through —; the calls are declared, exported and bound; the map structure has the C compiler's layout; and the argument rules that need no
device (csrc/flx_volume_map_args.h) hold in a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from volume_map_util import (COUNTS, assert_same_rows, decode64, encode64, grid_of, lookup_map64, map_of, map_radiance, map_rows64, ndc64, point_set, reference,
                             synthetic_maps, synthetic_sh, unit_normals, volume_reference, wall_radiance)
from volume_util import at

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("flx_probe_map_device", "flx_probe_map", "flx_probes_sh_map_device", "flx_probes_sh_map", "flx_volume_bake_map_device", "flx_volume_bake_map",
         "flx_volume_irradiance_map_device", "flx_volume_irradiance_map", "flx_rays_irradiance_map_device", "flx_rays_irradiance_map", "flx_frame_irradiance_map_device",
         "flx_frame_irradiance_map", "flx_volume_irradiance_map_of", "flx_debug_last_volume_map")
ARGS_CASES = 153         # the cases tests/volume_map_args_main.cc runs
# float32 with one rounding per operation against the float64 restatements over the same inputs.  Each bound is the worst deviation measured on this test's own
# cases with a margin of 4x, as test_volume_cpu.py sets its bounds.  The map rows' error grows with the exponent: a direction off by an ulp is raised to 2^k.
DECODE_BOUND = 4 * 9.95e-8           # observed 9.95e-08
ROWS_BOUND = 4 * 4.02e-5             # observed 4.02e-05 (at k = 8, an exponent of 256; 2.6e-06 at k <= 5)
LOOKUP_BOUND = 4 * 3.11e-7           # observed 3.11e-07
MEAN_BOUND = 4 * 1.7e-7              # observed 1.70e-07
ROW_CASES = ((1, 1, 0), (2, 3, 1), (3, 4, 5), (4, 8, 5), (8, 8, 5), (5, 16, 0), (8, 2, 8), (2, 16, 8))      # (w, m, k)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return reference(tmp_path_factory)


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return volume_reference(tmp_path_factory)


def test_the_map_structure_matches_the_c_compiler(tmp_path):
    from flexlight_hip import capi
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stdio.h>
#include <stddef.h>
#include "flexlight_hip_debug.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(flx_volume_map), offsetof(flx_volume_map, size), offsetof(flx_volume_map, sharpness), offsetof(flx_volume_map, reserved));
  return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)]).decode().split()))
    m = capi.VolumeMap
    assert got == [C.sizeof(m), m.size.offset, m.sharpness.offset, m.reserved.offset] == [16, 0, 4, 8]
    q = capi.VolumeMap(4, 3)
    assert (q.size, q.sharpness, list(q.reserved), q.bins) == (4, 3, [0, 0], 16)
    assert (capi.VolumeMap().size, capi.VolumeMap().sharpness) == (8, 5)


@pytest.mark.parametrize("m", range(1, 17))
def test_every_bin_centre_encodes_to_its_bin(ref, m):
    for b in range(m * m):
        d = ref.bin_direction(m, b)
        assert np.isfinite(d).all() and ref.bin(m, d) == b, (m, b)
        assert ref.bin(m, 7.5 * d.astype(np.float64)) == b                     # the direction need not be of unit length
        assert encode64(m, decode64(ndc64(b % m, m), ndc64(b // m, m)))[0] == b


def test_no_direction_leaves_the_map(ref):
    rng = np.random.default_rng(4)
    odd = [(0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (np.nan, 1.0, 0.0), (1.0, np.nan, -1.0), (np.inf, 0.0, 1.0), (-np.inf, np.inf, -np.inf), (3.0e38, 3.0e38, -3.0e38),
           (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0e-45, 0.0, -1.0e-45)]
    for m in (1, 2, 3, 8, 16):
        for d in odd + rng.normal(size=(200, 3)).tolist():
            assert 0 <= ref.bin(m, d) < m * m
        assert ref.bin(m, (0.0, 0.0, 0.0)) == 0 and ref.bin(m, (np.nan, np.nan, np.nan)) == 0
    # the four quadrants above and the four below the horizon land in the map's inner diamond and its corners
    assert ref.bin(2, (-1.0, -1.0, 4.0)) == 0 and ref.bin(2, (1.0, 1.0, 4.0)) == 3
    assert ref.bin(4, (0.1, 0.1, 1.0)) == 2 * 4 + 2 and ref.bin(4, (0.1, 0.1, -1.0)) == 3 * 4 + 3 and ref.bin(4, (-0.1, -0.1, -1.0)) == 0


def test_decode_against_float64_by_hand(ref):
    worst = 0.0
    rng = np.random.default_rng(2)
    points = [(ndc64(bx, m), ndc64(by, m)) for m in range(1, 17) for bx in range(m) for by in range(m)] + rng.uniform(-1.0, 1.0, size=(500, 2)).tolist()
    for u, v in points:
        u, v = np.float32(u), np.float32(v)
        got = ref.decode(u, v).astype(np.float64)
        want = decode64(float(u), float(v))
        assert abs((got * got).sum() - 1.0) < 1.0e-6
        worst = max(worst, float(np.abs(got - want).max()))
    print("decode against float64: worst deviation %.3g over %d points" % (worst, len(points)))
    assert worst <= DECODE_BOUND, worst


def test_the_map_rows_against_float64_by_hand(ref):
    worst, cases = 0.0, 0
    for i, (w, m, k) in enumerate(ROW_CASES):
        vmap = map_of(m, k)
        radiance = map_radiance(3, w, 20 + i, nan=False)
        got = ref.rows(radiance, 3, w, vmap).astype(np.float64).reshape(3, m * m, 4)
        rays = 6 * w * w
        for p in range(3):
            want = map_rows64(radiance[p * rays:(p + 1) * rays], w, m, k)
            assert (got[p, :, 0:3] == 0).all() if p == 1 else (got[p, :, 0] > 0).any()
            some = want > 1.0e-30                         # (a sum that underflows float32 is not measured)
            worst = max(worst, float((np.abs(got[p] - want)[some] / want[some]).max()))
            cases += int(some.sum())
    print("map rows against float64: worst relative deviation %.3g over %d sums" % (worst, cases))
    assert worst <= ROWS_BOUND, worst


def test_the_lookup_against_float64_by_hand(ref):
    worst, cases, excluded = 0.0, 0, 0
    for k, count in enumerate(COUNTS):
        for visibility in (True, False):
            for bias in (0.0, 0.125):
                grid, vmap = grid_of(count, bias, visibility), map_of((2, 3, 8, 16)[k], 5)
                sh, maps = synthetic_sh(grid.probes, 11 + k), synthetic_maps(grid.probes, vmap.size, 3 + k)
                maps[np.isnan(maps)] = 1.0
                rng = np.random.default_rng(1100 + k)
                positions = np.ones((300, 4), np.float32)
                positions[:, :3] = at(grid, rng.uniform(-1.0, np.array(count, np.float64), size=(300, 3)))
                normals = unit_normals(rng, 300)
                got = ref.irradiance(grid, vmap, sh, maps, positions, normals).astype(np.float64)
                assert np.isfinite(got).all() and (got[:, 3] > 0).all()
                for r in range(300):
                    want, margin, bin_margin = lookup_map64(grid, vmap, sh, maps, positions[r], normals[r])
                    cases += 1
                    if margin <= LOOKUP_BOUND or bin_margin <= 1.0e-5:               # the branch dist > mean, or the nearest bin, may turn
                        excluded += 1
                        continue
                    worst = max(worst, float(np.abs(got[r] - want).max() / np.abs(want).max()))
    print("lookup with maps against float64: worst relative deviation %.3g over %d cases, %d excluded" % (worst, cases, excluded))
    assert excluded <= cases // 100
    assert worst <= LOOKUP_BOUND, worst


def test_constant_distance_gives_that_mean_in_every_bin(ref):
    worst = 0.0
    for w, m in ((1, 1), (2, 3), (4, 8), (8, 16)):
        for d in (0.25, 3.0, 1.7):
            radiance = np.zeros((6 * w * w, 8), np.float32)
            radiance[:, 0:4], radiance[:, 4] = 1.0, d
            rows = ref.rows(radiance, 1, w, map_of(m, 0)).astype(np.float64)
            assert (rows[:, 0] > 0).all()
            assert_same_rows(rows[:, 0:1].astype(np.float32), rows[:, 3:4].astype(np.float32), "all hit: the coverage is the weight")
            worst = max(worst, float(np.abs(rows[:, 1] / rows[:, 0] - np.float32(d)).max() / d), float(np.abs(rows[:, 2] / rows[:, 0] - float(np.float32(d)) ** 2).max() / d ** 2))
    print("constant distance: worst relative deviation of mean and mean square %.3g" % worst)
    assert worst <= MEAN_BOUND, worst


def test_the_wall_no_longer_leaks_and_the_open_side_is_no_longer_dimmed(ref):
    """the issue's table: w = 8, m = 8, k = 5, floor = 0; a wall one unit away on +x, open space to ten units elsewhere"""
    w, vmap = 8, map_of(8, 5)
    grid = grid_of((1, 1, 1), 0.0, True, floor=0.0)
    radiance = wall_radiance(ref, w)
    maps, sphere = ref.rows(radiance, 1, w, vmap), ref.sphere(radiance, w)
    # behind the wall: the point lies in direction +x of the probe, 3 away
    behind = maps[ref.bin(8, (1.0, 0.0, 0.0))]
    iso, directional = ref.sphere_wv(grid, 3.0, sphere), ref.wv(grid, 3.0, behind)
    print("behind the wall: isotropic wv %.6g, directional wv %.6g" % (iso, directional))
    assert iso == 1.0 and directional < 0.01
    # in the open: direction -x, 9 away
    open_side = maps[ref.bin(8, (-1.0, 0.0, 0.0))]
    iso, directional = ref.sphere_wv(grid, 9.0, sphere), ref.wv(grid, 9.0, open_side)
    print("in the open: isotropic wv %.6g, directional wv %.6g" % (iso, directional))
    assert iso < 0.5 and directional == 1.0
    # ... and through the lookup: one probe, points on either side of it (the lookup negates the direction from the point to the probe)
    sh = synthetic_sh(1, 1)
    sh[0, 7], sh[0, 11], sh[0, 15] = sphere
    o = np.array(list(grid.origin), np.float32)
    positions = np.array([[o[0] + 3.0, o[1], o[2], 1.0], [o[0] - 9.0, o[1], o[2], 1.0]], np.float32)
    normals = np.array([[0.0, 1.0, 0.0, 0.0]] * 2, np.float32)
    _, bins, weight, dist = ref.corners(grid, vmap, maps, positions[0], normals[0])
    assert (bins == ref.bin(8, (1.0, 0.0, 0.0))).all() and (dist == 3.0).all() and weight.max() < 0.01
    _, bins, weight, dist = ref.corners(grid, vmap, maps, positions[1], normals[1])
    assert (bins == ref.bin(8, (-1.0, 0.0, 0.0))).all() and (dist == 9.0).all() and weight.max() == np.float32(np.float32(0.25) + np.float32(0.2))


def test_a_bin_nothing_hit_leaves_the_probe_visible(ref):
    grid = grid_of((1, 1, 1), 0.0, True, floor=0.0)
    for q in ((0.0, 0.0, 0.0, 0.7), (-0.0, 5.0, 9.0, 0.7), (-1.0, 1.0, 1.0, 0.7), (0.0, np.nan, np.nan, 0.7)):
        assert ref.wv(grid, 100.0, q) == 1.0, q
    assert ref.wv(grid, 100.0, (1.0, 1.0, 1.0, 1.0)) == 0.0                  # a bin that did hit, at distance 1 with no variance: floor
    assert np.isnan(ref.wv(grid, 100.0, (np.nan, 1.0, 1.0, 1.0))) or ref.wv(grid, 100.0, (np.nan, 1.0, 1.0, 1.0)) == 1.0      # a NaN q[0] is not > 0: visible
    # a probe of only misses: every bin's first three words are 0.0 and its fourth is the filter's weight
    w, vmap = 3, map_of(4, 2)
    radiance = np.zeros((54, 8), np.float32)
    rows = ref.rows(radiance, 1, w, vmap)
    assert (rows[:, 0:3].view(np.uint32) == 0).all() and (rows[:, 3] > 0).all()


def test_a_nan_distance_gives_some_nan(ref):
    w, vmap = 4, map_of(3, 1)
    radiance = map_radiance(2, w, 5, nan=True)
    rows = ref.rows(radiance, 2, w, vmap).reshape(2, 9, 4)
    assert np.isfinite(rows[0]).all()
    assert np.isnan(rows[1, :, 1]).all() and np.isnan(rows[1, :, 2]).all() and np.isfinite(rows[1, :, 0]).all() and np.isfinite(rows[1, :, 3]).all()
    # ... which the weight's own text decides as it decides a NaN in an SH row's moments: dist > NaN does not hold, so a NaN mean leaves the probe visible, and a
    # NaN mean square under a finite mean is a NaN variance, den > 0 does not hold, ch = 0 and the weight is the floor
    grid = grid_of((1, 1, 1), 0.0, True, floor=0.125)
    assert ref.wv(grid, 100.0, (1.0, np.nan, 1.0, 1.0)) == 1.0 and ref.wv(grid, 100.0, (1.0, 1.0, np.nan, 1.0)) == 0.125


def test_without_the_flag_the_map_lookup_is_the_plain_lookup(ref, plain):
    for k, count in enumerate(COUNTS):
        grid, vmap = grid_of(count, 0.125, visibility=False), map_of(3 + k, 5)
        sh, maps = synthetic_sh(grid.probes, k), synthetic_maps(grid.probes, vmap.size, k)
        for kind in ("faces", "outside", "misses"):
            positions, normals = point_set(grid, kind, 129, 7 + k)
            assert_same_rows(ref.irradiance(grid, vmap, sh, maps, positions, normals), plain.irradiance(grid, sh, positions, normals), kind)


def test_the_calls_are_declared_exported_and_bound(ref):
    from flexlight_hip import capi
    header = open(os.path.join(ROOT, "include", "flexlight_hip_debug.h")).read()
    public = open(os.path.join(ROOT, "include", "flexlight_hip.h")).read()
    for name in CALLS:
        assert name in capi.EXPORTS and hasattr(capi.LIB, name) and name + "(" in header and name not in public, name
    for method in ("probe_map", "probe_map_device", "probes_sh_map", "probes_sh_map_device", "volume_bake_map", "volume_bake_map_device", "volume_irradiance_map",
                   "volume_irradiance_map_device", "rays_irradiance_map", "rays_irradiance_map_device", "frame_irradiance_map", "frame_irradiance_map_device", "last_volume_map"):
        assert callable(getattr(capi.Context, method))
    # the library's host export is the reference's definition
    grid, vmap = grid_of((3, 2, 4), 0.125), map_of(5, 3)
    sh, maps = synthetic_sh(grid.probes, 3), synthetic_maps(grid.probes, 5, 2)
    positions, normals = point_set(grid, "misses", 65, 1)
    assert_same_rows(capi.volume_irradiance_map_of(grid, vmap, sh, maps, positions, normals), ref.irradiance(grid, vmap, sh, maps, positions, normals))
    assert capi.volume_irradiance_map_of(grid, vmap, sh, maps, positions[0], normals[0, :3]).shape == (4,)


def test_argument_rules_in_a_stand_alone_program_under_the_sanitizers(tmp_path):
    """every refusal of flx_volume_map_args.h and their order, m and k at their ends, n_probes m m on either side of 2^31 (and where a 32-bit product would come back
    small), the maps array against every other array of a call: the header with a main of its own, built with -fsanitize=address,undefined, run directly"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is part of the image (the oracle is built with gcc)"
    exe = tmp_path / "volume_map_args"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "web-ray-tracer_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "volume_map_args_main.cc"), "-o", str(exe)])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) == ARGS_CASES
