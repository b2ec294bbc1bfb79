"""Light probes and probe volumes across their seams (csrc/flx_probes.hip, csrc/flx_volume.hip): the second and later launches of k_probe_rays (32 768 probes a
launch), faces up to the largest the library accepts, the natural chunk of flx_probes_sh_device (2^21 rays, never lowered here), probes traced in several trace slabs,
and a volume whose grid is beyond one launch.  Every output goes into a poisoned buffer with spare rows behind it and is compared in all words of all rows, bit for
bit: with the CPU references (tests/probe_ref, tests/volume_ref) where they define the rows, with the calls a fused call is made of where it is fused, and with calls
that no multi-launch code has touched where the seam itself is the subject."""
import time

import numpy as np
import pytest
import torch

import volume_util
from flexlight_hip import capi
from probe_util import assert_same_words, cornell_probes, finished, poisoned, positions_of, reference, synthetic_radiance
from rays_trace_util import camera_rays

pytestmark = pytest.mark.gpu

LAUNCH = 32768          # PROBE_LAUNCH of csrc/flx_probes.hip: probes a launch of k_probe_rays names with its grid's y
# (face size, probes) on either side of the launch seam: the last launch full less one, exactly full, one probe in a second launch, one probe in a third; then
# R = 24, where the second launch's first ray row is not at LAUNCH * 6 and a probe spans more than one wave's stores
ACROSS = ((1, 32767), (1, 32768), (1, 32769), (1, 65537), (2, 32769))
# faces beyond test_probes_gpu.py's: 48, 64, 128, 256 have w w a multiple of 256 (a workgroup of k_probe_rays within one face: 9, 16, 64 and 256 workgroups a
# face), 256 the largest face there is; 20: w w = 400, so a workgroup straddles two faces and the face is the lane's own
LARGE_RAYS = ((20, 2), (48, 2), (64, 2), (128, 2), (256, 1))
# the reduction: 24 .. 1 536 texels a lane for 16 .. 128, 20 with R = 2 400 no multiple of 64 (the last trip has lanes without a texel); 1 probe: one wave of the
# workgroup works, 5: two workgroups, the second with one wave.  256: 6 144 texels a lane and rows + probe * R * 2 at 12.6 MB a probe; 3: a workgroup's fourth wave idle
LARGE_SUMS = ((16, (1, 5)), (20, (1, 5)), (32, (1, 5)), (48, (1, 5)), (64, (1, 5)), (128, (1, 5)), (256, (1, 3)))
GRID = (33, 32, 32)     # 33 792 probes: 132 workgroups of k_volume_positions, two launches of k_probe_rays; the last divide / modulo is by 32 and by 33
SEAM = slice(LAUNCH - 8, LAUNCH + 8)      # the sixteen probes around the first seam


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return reference(tmp_path_factory)


@pytest.fixture(scope="module")
def vref(tmp_path_factory):
    return volume_util.reference(tmp_path_factory)


def upload(array):
    out = torch.from_numpy(np.ascontiguousarray(array)).cuda()
    torch.cuda.synchronize()
    return out


def device_rays(ctx, positions, w):
    n = len(positions) * 6 * w * w
    out = poisoned(n, 32)
    d_positions = upload(positions)
    assert ctx.probe_rays_device(d_positions, w, out=out) is out
    return finished(ctx, out, n, 8)


def device_sh(ctx, d_positions, t, params):
    """flx_probes_sh_device into a poisoned output -> uint32 [n, 36]"""
    n = d_positions.shape[0]
    out = poisoned(n, 144)
    torch.cuda.synchronize()
    assert ctx.probes_sh_device(d_positions, t, params, out=out) is out
    return finished(ctx, out, n, 36)


def pairwise_different(rows):
    rows = np.ascontiguousarray(rows)
    return len(np.unique(rows.view(np.uint32).reshape(len(rows), -1), axis=0)) == len(rows)


# ---- 1. ray rows across launches ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w, n", ACROSS)
def test_ray_rows_across_launches(hip, ref, w, n):
    rays = 6 * w * w
    positions = positions_of(n, seed=n)
    want = ref.rays(positions, w)
    assert pairwise_different(positions[:, :3])
    for first in range(LAUNCH, n, LAUNCH):                 # the inputs tell a launch that reads or writes from the batch's start from one that does not
        for other in (0, first - LAUNCH, first - 1):
            assert not np.array_equal(want[first * rays], want[other * rays]), (first, other)
    assert_same_words(device_rays(hip, positions, w), want, "%d probes of w = %d" % (n, w))
    if (w, n) == (1, 32769):
        assert_same_words(hip.probe_rays(positions, w), want, "the host variant, %d probes of w = %d" % (n, w))


# ---- 2. large faces ----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w, n", LARGE_RAYS)
def test_ray_rows_of_large_faces(hip, ref, w, n):
    positions = positions_of(n, seed=w)
    assert_same_words(device_rays(hip, positions, w), ref.rays(positions, w), "%d probes of w = %d" % (n, w))


@pytest.mark.parametrize("w, counts", LARGE_SUMS)
def test_the_reduction_of_large_faces(hip, ref, w, counts):
    sky = (0.25, 0.5, 4.0)
    params = capi.ProbeParams(face_size=w, sky=sky)
    for n in counts:
        radiance = synthetic_radiance(n, w, seed=100 * w + n)
        want = ref.reduce(radiance, n, w, sky)
        assert np.isfinite(want).all() and (want[:, 3] > 0).all()
        out = poisoned(n, 144)
        d_radiance = upload(radiance.view(np.uint8))
        assert hip.probe_reduce_device(d_radiance, n, params, out=out) is out
        assert_same_words(finished(hip, out, n, 36), want, "%d probes of w = %d" % (n, w))
        if (w, n) == (64, 1):
            assert_same_words(hip.probe_reduce(radiance, n, params), want, "the host variant, %d probes of w = %d" % (n, w))


# ---- 3. flx_probes_sh_device across a launch seam ------------------------------------------------------------------------------------------------------------------------

def cornell_many(oracle, scenes, n):
    """-> (scene, trace params, n positions float32 [n, 4]): cornell_probes' five positions in turn, probe k moved towards the camera by (k // 5 + 1) of 0.25 / (n // 5
    + 1) of the way — the stretch between the camera and a first hit is free space —, so that no two rows are the same; word 3 is junk"""
    sc, t, five = cornell_probes(oracle, scenes)
    camera = np.array(list(camera_rays(oracle, scenes, "cornell")[1].camera), np.float64)
    k = np.arange(n)
    base = five[k % 5, :3].astype(np.float64)
    f = 0.25 * (k // 5 + 1) / (n // 5 + 1)
    positions = np.full((n, 4), 7.0, np.float32)
    positions[:, :3] = base + f[:, None] * (camera - base)
    assert pairwise_different(positions[:, :3])
    return sc, t, positions


def test_probes_across_a_launch_seam(hip, oracle, scenes):
    n = LAUNCH + 16
    sc, t, positions = cornell_many(oracle, scenes, n)
    hip.update_scene(sc)
    params = capi.ProbeParams(face_size=1, sky=(0.5, 0.25, 0.125))
    d_positions = upload(positions)
    try:
        hip.set_probe_chunk(0)
        got = device_sh(hip, d_positions, t, params)           # one chunk: two launches of k_probe_rays
        last = hip.last_probes()
        assert last == {"chunks": 1, "chunk": 349525, "face_size": 1, "n": n, "order": 0, "rays": 6, "reduce_groups": n // 4}, last
        hip.set_probe_chunk(4096)                              # every chunk is one launch that begins at its own first probe
        want = device_sh(hip, d_positions, t, params)
        last = hip.last_probes()
        assert (last["chunks"], last["chunk"], last["reduce_groups"]) == (9, 4096, 4), last
    finally:
        hip.set_probe_chunk(0)
    assert_same_words(got[0:8], want[0:8], "the first rows against the call in chunks of 4096")
    assert_same_words(got[LAUNCH - 8:n], want[LAUNCH - 8:n], "the rows from the seam on against the call in chunks of 4096")
    assert_same_words(got, want, "every row against the call in chunks of 4096")
    assert_same_words(got[SEAM], device_sh(hip, upload(positions[SEAM]), t, params), "the sixteen rows at the seam against a call of their own")
    assert_same_words(hip.probes_sh(positions, t, params), got, "the host variant")
    rows = got.view(np.float32)
    assert np.isfinite(rows).all() and (rows[:, 7] > 0).mean() > 0.5 and (rows[:, 3] > 0).all()
    assert pairwise_different(got[SEAM])


# ---- 4. the natural chunk ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_reflections", (2, 0))
def test_the_natural_chunk(hip, oracle, scenes, max_reflections):
    """six probes of face size 256: 2 359 296 rays, which the chunks cut at 5 probes = 1 966 080 rays and the trace of the three calls cuts at 2^21, so the two cuts
    are independent.  No debug knob is set.  A natural chunk is 2^21 rays by definition: the test cannot be smaller (its time: profiles/probes.txt, section 7).
    With 2 bounces the renderer, and the CPU reference of the trace with it, gives 22 of these rays a NaN colour (3 to 5 a probe, the same texels in every probe: the
    noise words are the texel's), so all 27 coefficient sums of all six rows are NaNs — equal bits here, where both sides run the same kernel over the same rows —
    and only the four sums of d_omega and of the distances are numbers.  Without a bounce no ray gives a NaN, and every word is a number that has to agree."""
    w, n, rays = 256, 6, 393216
    sc, t, positions = cornell_many(oracle, scenes, n)
    hip.update_scene(sc)
    t.samples, t.max_reflections = 1, max_reflections
    sky = (0.5, 0.25, 0.125)
    d_positions = upload(positions)
    hip.set_probe_chunk(0)
    hip.set_trace_slab(0)
    generated = hip.probe_rays_device(d_positions, w)
    radiance = hip.trace_rays_ordered_device(generated, t, order=0)
    want = hip.probe_reduce_device(radiance, n, capi.ProbeParams(face_size=w, sky=sky))
    hip.sync()
    assert hip.last_trace()["slabs"] == 2
    want = want.cpu().numpy()
    del generated, radiance
    moments = want[:, (3, 7, 11, 15)]
    assert np.isfinite(moments).all() and (moments > 0).all() and pairwise_different(moments)
    if max_reflections == 0:
        assert np.isfinite(want).all() and (want[:, 0:3] > 0).all() and pairwise_different(want[:, 0:3])
    for order in (0, capi.TRACE_ORDER_HITS):
        params = capi.ProbeParams(face_size=w, order=order, sky=sky)
        out = poisoned(n, 144)
        torch.cuda.synchronize()
        began = time.perf_counter()
        hip.probes_sh_device(d_positions, t, params, out=out)
        hip.sync()
        print("flx_probes_sh_device, 6 probes of face size 256, %d bounces, order %d: %.1f ms" % (max_reflections, order, 1e3 * (time.perf_counter() - began)))
        assert_same_words(finished(hip, out, n, 36), want, "order %d" % order)
        last = hip.last_probes()
        assert last == {"chunks": 2, "chunk": 5, "face_size": w, "n": n, "order": order, "rays": rays, "reduce_groups": 1}, last


# ---- 5. probes under trace slabs -----------------------------------------------------------------------------------------------------------------------------------------

def test_probes_under_trace_slabs(hip, oracle, scenes):
    sc, t, positions = cornell_probes(oracle, scenes)
    hip.update_scene(sc)
    d_positions = upload(positions)
    try:
        for order in (0, capi.TRACE_ORDER_HITS):
            params = capi.ProbeParams(face_size=8, order=order, sky=(0.5, 0.25, 0.125))
            hip.set_trace_slab(0)
            hip.set_query_groups(0)
            want = device_sh(hip, d_positions, t, params)
            assert np.isfinite(want.view(np.float32)).all() and hip.last_trace()["slabs"] == 1
            for slab, groups, slabs in ((100, 0, 20), (64, 1, 30)):      # 1 920 rays: 19 slabs of 100 and one of 20; 30 of 64, one workgroup taking ray after ray
                hip.set_trace_slab(slab)
                hip.set_query_groups(groups)
                assert_same_words(device_sh(hip, d_positions, t, params), want, "order %d, slabs of %d rays, %d query groups" % (order, slab, groups))
                last = hip.last_trace()
                assert (last["slabs"], last["slab"], last["n"]) == (slabs, slab, 1920), last
    finally:
        hip.set_trace_slab(0)
        hip.set_query_groups(0)


# ---- 6. a volume beyond one launch ---------------------------------------------------------------------------------------------------------------------------------------

def test_positions_of_a_grid_beyond_one_launch(hip, vref):
    grid = capi.VolumeGrid((0.1, -0.2, 0.3), (0.3, 0.7, 1.1), GRID)      # no spacing is a power of two
    want = vref.positions(grid)
    assert grid.probes == 33792 and pairwise_different(want[:, :3])
    out = poisoned(grid.probes, 16)
    torch.cuda.synchronize()
    assert hip.volume_positions_device(grid, out=out) is out
    assert_same_words(finished(hip, out, grid.probes, 4), want, "33 x 32 x 32")


@pytest.fixture(scope="module")
def baked(hip, oracle, scenes, vref):
    """-> (grid, the bake's SH rows uint32 [33 792, 36], trace params, probe params): the grid scaled into the hull of a frame's first hits on the Cornell box, as
    test_volume_gpu.py's cornell_volume does, baked at face size 1 with the default chunk"""
    sc, t, _ = cornell_probes(oracle, scenes)
    hip.update_scene(sc)
    p = sc.frame_params(width=64, height=48, samples=1, max_reflections=3, use_filter=0)
    planes = hip.frame_surface(p, capi.SURFACE_POSITION)[0]
    hit = planes[planes[:, 3] != 0.0][:, :3]
    assert len(hit) > 1000
    lo, hi = hit.min(axis=0), hit.max(axis=0)
    cells = np.array(GRID, np.float64) - 1.0
    grid = capi.VolumeGrid(lo + 0.2 * (hi - lo), 0.6 * (hi - lo) / cells, GRID, normal_bias=0.01 * float((hi - lo).max()))
    q = capi.ProbeParams(face_size=1, sky=(0.5, 0.25, 0.125))
    hip.set_probe_chunk(0)
    out = poisoned(grid.probes, 144)
    torch.cuda.synchronize()
    began = time.perf_counter()
    assert hip.volume_bake_device(grid, t, q, out=out) is out
    hip.sync()
    print("flx_volume_bake_device, 33 x 32 x 32 probes of face size 1: %.1f ms" % (1e3 * (time.perf_counter() - began)))
    rows = finished(hip, out, grid.probes, 36)
    last = hip.last_probes()
    assert last == {"chunks": 1, "chunk": 349525, "face_size": 1, "n": 33792, "order": 0, "rays": 6, "reduce_groups": 8448}, last
    return grid, rows, t, q


def test_the_bake_of_a_grid_beyond_one_launch(hip, oracle, scenes, vref, baked):
    grid, rows, t, q = baked
    hip.update_scene(cornell_probes(oracle, scenes)[0])
    positions = vref.positions(grid)
    assert pairwise_different(positions[SEAM, :3])
    assert np.isfinite(rows.view(np.float32)).all() and (rows.view(np.float32)[:, 7] > 0).mean() > 0.5
    assert_same_words(rows[SEAM], device_sh(hip, upload(positions[SEAM]), t, q), "the sixteen rows at the seam against probes_sh_device on their positions alone")
    try:
        hip.set_probe_chunk(4096)
        out = poisoned(grid.probes, 144)
        torch.cuda.synchronize()
        hip.volume_bake_device(grid, t, q, out=out)
        assert_same_words(finished(hip, out, grid.probes, 36), rows, "the bake in chunks of 4096")
        assert hip.last_probes()["chunks"] == 9
    finally:
        hip.set_probe_chunk(0)


def reached(vref, grid, sh, sets):
    """what the points of the sets reach, by the reference's own corners (corner 0 is the base) -> (bool [3]: a base index in the last cell of that axis, the
    highest probe index read)"""
    last_cell, highest = np.zeros(3, bool), 0
    for _, positions, normals in sets:
        for k in range(len(positions)):
            index = vref.corners(grid, sh, positions[k], normals[k])[0]
            base = int(index[0])
            at = np.array([base % GRID[0], base // GRID[0] % GRID[1], base // (GRID[0] * GRID[1])])
            last_cell |= at == np.array(GRID) - 2
            highest = max(highest, int(index.max()))
    return last_cell, highest


def test_the_lookup_over_a_grid_beyond_one_launch(hip, vref, baked):
    """the baked rows (real moments) and synthetic ones; 2 000 points in the first cell, on cell faces all over the grid, and outside it"""
    n = 2000
    tables = (("baked", baked[1].view(np.float32)), ("synthetic", volume_util.synthetic_sh(baked[0].probes, 2)))
    for visibility in (True, False):
        b = baked[0]
        grid = capi.VolumeGrid(tuple(b.origin), tuple(b.spacing), GRID, b.normal_bias, b.floor, capi.VOLUME_VISIBILITY if visibility else 0)
        sets = [(kind,) + volume_util.point_set(grid, kind, n, 1000 * k + n) for k, kind in enumerate(("one_cell", "faces", "outside"))]
        if visibility:                                         # (the corners do not depend on the flag or on the rows)
            last_cell, highest = reached(vref, grid, tables[1][1], sets)
            assert last_cell.all() and highest > LAUNCH, (last_cell, highest)
        for name, sh in tables:
            d_sh = upload(sh)
            for kind, positions, normals in sets:
                what = "%s rows, %s, visibility %d" % (name, kind, visibility)
                want = vref.irradiance(grid, sh, positions, normals)
                assert np.isfinite(want).all() and (want[:, 3] > 0).all(), what
                out = poisoned(n, 16)
                d_positions, d_normals = upload(positions), upload(normals)
                assert hip.volume_irradiance_device(grid, d_sh, d_positions, d_normals, out=out) is out
                assert_same_words(finished(hip, out, n, 4), want, what)
                last = hip.last_volume()
                assert last == {"n": n, "slabs": 1, "slab": n, "probes": grid.probes, "flags": grid.flags, "source": 0, "groups": 8}, last
