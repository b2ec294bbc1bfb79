"""Directional visibility across its seams (include/flexlight_hip_debug.h, "directional visibility"): k_probe_map's launches of 32 768 probes — a launch less one
probe, a launch, a launch and a probe —, a grid of 16 bin groups by 4 097 probes, and the map lookup over a grid whose probes, and therefore map rows, lie past
32 768.  Synthetic rows against the CPU reference's bits, and the rows at each seam against calls of their own: a library whose later launches read the first
launch's rows fails here."""
import numpy as np
import pytest
import torch

from flexlight_hip import capi
from volume_map_util import assert_same_rows, finished, map_of, poisoned, reference, synthetic_maps, synthetic_sh, unit_normals
from volume_util import at

pytestmark = pytest.mark.gpu

LAUNCH = 32768          # FLX_VOLUME_MAP_LAUNCH: probes a launch of k_probe_map names with its grid's y
GRID = (33, 32, 32)     # 33 792 probes: test_probe_seams_gpu.py's grid


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return reference(tmp_path_factory)


def seam_radiance(n_probes, face_size, seed):
    """radiance rows float32 [n * 6 w w, 8], a third of them misses, no two probes alike"""
    rng = np.random.default_rng(seed)
    n = n_probes * 6 * face_size * face_size
    rows = np.zeros((n, 8), np.float32)
    rows[:, 3] = 1.0
    rows[:, 4] = np.exp2(rng.uniform(-4.0, 4.0, size=n))
    rows[rng.random(n) < 1.0 / 3.0] = 0.0
    return rows


def reduced(ctx, d_radiance, n, w, vmap):
    out = poisoned(n * vmap.bins, 16)
    torch.cuda.synchronize()
    assert ctx.probe_map_device(d_radiance, n, w, vmap, out=out) is out
    return finished(ctx, out, n * vmap.bins, 4).view(np.float32)


@pytest.fixture(scope="module")
def launch_rows(ref):
    """32 769 probes of w = 1, m = 2, which the three counts share: (radiance, the reference's rows)"""
    radiance = seam_radiance(LAUNCH + 1, 1, 5)
    return radiance, ref.rows(radiance, LAUNCH + 1, 1, map_of(2, 3))


@pytest.mark.parametrize("n", (LAUNCH - 1, LAUNCH, LAUNCH + 1))
def test_map_rows_across_a_launch(hip, launch_rows, n):
    radiance, want = launch_rows
    vmap = map_of(2, 3)
    d_radiance = torch.from_numpy(radiance).cuda()
    got = reduced(hip, d_radiance[:n * 6], n, 1, vmap)
    assert_same_rows(got, want[:n * 4], "%d probes" % n)
    assert hip.last_volume_map() == {"probes": n, "size": 2, "sharpness": 3, "launches": 1 if n <= LAUNCH else 2, "groups": n if n <= LAUNCH else 1, "face_size": 1}
    for p in sorted(p for p in {0, LAUNCH - 2, LAUNCH - 1, LAUNCH} if p < n):                 # the rows at the seam against calls of their own
        assert_same_rows(reduced(hip, d_radiance[p * 6:(p + 1) * 6], 1, 1, vmap), got[p * 4:(p + 1) * 4], "probe %d alone" % p)
    assert len(np.unique(got[np.isfinite(got).all(axis=1)].view(np.uint32), axis=0)) > n      # no two probes alike: a row read from another launch's would show


def test_map_rows_of_sixteen_bin_groups_by_many_probes(hip, ref):
    n, w, vmap = 4097, 2, map_of(16, 5)
    radiance = seam_radiance(n, w, 6)
    d_radiance = torch.from_numpy(radiance).cuda()
    got = reduced(hip, d_radiance, n, w, vmap)
    assert_same_rows(got, ref.rows(radiance, n, w, vmap), "4 097 probes of 16 x 16 bins")
    assert hip.last_volume_map() == {"probes": n, "size": 16, "sharpness": 5, "launches": 1, "groups": 16 * n, "face_size": 2}
    for p in (0, 4095, 4096):
        assert_same_rows(reduced(hip, d_radiance[p * 24:(p + 1) * 24], 1, w, vmap), got[p * 256:(p + 1) * 256], "probe %d alone" % p)


def test_the_map_lookup_reads_rows_past_32768(hip, ref):
    grid = capi.VolumeGrid((-1.0, 0.5, 2.0), (0.75, 1.25, 0.5), GRID, 0.0625, 0.05)
    vmap = map_of(2, 5)
    assert grid.probes == 33792
    sh, maps = synthetic_sh(grid.probes, 3), synthetic_maps(grid.probes, 2, 3)
    rng = np.random.default_rng(8)
    n = 1000
    g = rng.uniform(0.0, np.array(GRID, np.float64) - 1.0, size=(n, 3))
    g[: n // 2, 2] = rng.uniform(31.0 - 0.9, 31.0, size=n // 2)           # the last layer of cells: probes from 30 x 33 x 32 = 31 680 on, the upper corners from 32 736
    g[: n // 4, 1] = rng.uniform(30.1, 31.0, size=n // 4)                 # ... and its last rows: the four upper corners past 32 768
    positions = np.ones((n, 4), np.float32)
    positions[:, :3] = at(grid, g)
    normals = unit_normals(rng, n)
    index = np.array([ref.corners(grid, vmap, maps, positions[r], normals[r])[0] for r in range(n // 4)])
    assert ((index > LAUNCH).sum(axis=1) >= 4).all() and index.max() >= 33759          # (31 x 33 x 32 + 31 x 33: the last row of the last layer)
    want = ref.irradiance(grid, vmap, sh, maps, positions, normals)
    d_sh, d_maps = torch.from_numpy(sh).cuda(), torch.from_numpy(maps).cuda()
    d_positions, d_normals = torch.from_numpy(positions).cuda(), torch.from_numpy(normals).cuda()
    out = poisoned(n, 16)
    torch.cuda.synchronize()
    hip.volume_irradiance_map_device(grid, d_sh, d_positions, d_normals, vmap, d_maps, out=out)
    assert_same_rows(finished(hip, out, n, 4).view(np.float32), want, "33 x 32 x 32 probes, 2 x 2 bins")
