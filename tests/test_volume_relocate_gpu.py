"""Probe relocation on the device (include/flexlight_hip_debug.h, "probe relocation"): k_probe_relocate's offset rows and states are the CPU reference's bits
(tests/volume_relocate_ref, the same include/flx_volume_relocate.h) for every face size and probe count at which the kernel can go wrong, into arrays of poison;
k_volume_positions_offset's rows are; the whole path on the Cornell scene is the CPU chain — probe rays, surface rows, reduction — bit for bit, and the parts called
one after the other, whatever the chunk and the trace slab; the relocated lookups are the reference's bits, leave out dead probes whatever their rows hold, and with
zero offsets are the plain lookups; the relocated bake and update are their parts; a pass between two frames of the loop leaves them alone; every refusal says its
words and leaves the outputs as they were.

ONE READING OF THE ISSUE: the arithmetic list (first + j stride) cannot hold a skipped entry — the update calls' own rule refuses a list whose last entry is outside
the grid, and this call asks that rule first — so the skipped entries of the position tests are a list's."""
import numpy as np
import pytest
import torch

from flexlight_hip import capi
from probe_util import reference as probe_reference
from surface_util import reference as surface_reference
from volume_relocate_util import (FACES, FREEZE, INACTIVE, POISON, PROBE_COUNTS, REJECTED, SPARE, assert_same_rows, assert_same_words, back, device_words, grid_of, map_of,
                                  reference, relocate_of, rule_of, states_of, synthetic_case, synthetic_maps, synthetic_sh)
from volume_update_util import BLENDED, update_of
from volume_util import COUNTS, POINT_SETS, point_set

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 255, 256, 257, 1000)      # test_volume_gpu.py's
FIELDS = capi.SURFACE_HIT | capi.SURFACE_NORMAL
# a 3 x 2 x 4 grid in the Cornell box (the room is -5 .. 5): probe 18 = (0, 0, 3) starts inside the short cuboid and probe 20 = (2, 0, 3) inside the tall one
CORNELL_GRID = ((-2.5, -3.0, -3.6), (2.0, 5.0, 1.3), (3, 2, 4))
CORNELL_FACE = 4


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return reference(tmp_path_factory)


def cornell_relocate(flags=0):
    return capi.VolumeRelocate(0.25, 0.3, 20.0, 0.45, flags)


@pytest.fixture(scope="module")
def chain(tmp_path_factory, oracle, scenes, ref):
    """the CPU chain on the Cornell golden scene, computed once: three passes and a frozen one -> (scene, texture width, grid, the offset rows after each pass, the
    planes of the first pass)"""
    pref, sref = probe_reference(tmp_path_factory), surface_reference(tmp_path_factory)
    sc = scenes("cornell")
    tw = sc.frame_params(width=64, height=48, samples=1, max_reflections=1, use_filter=0).texture_width
    grid = capi.VolumeGrid(*CORNELL_GRID, normal_bias=0.05)
    offsets, rows, first = np.zeros((24, 4), np.float32), [], None
    for k in range(4):
        planes = sref.rays(sc, pref.rays(ref.positions(grid, offsets), CORNELL_FACE), tw)
        hit, normal = planes[0], planes[3]
        if first is None:
            first = (hit, normal)
        offsets = ref.relocate(grid, cornell_relocate(FREEZE if k == 3 else 0), CORNELL_FACE, hit, normal, offsets)
        rows.append(offsets)
    share = (first[1].view(np.float32)[:, 3] > 0).reshape(24, -1).mean(axis=1)
    assert share[18] > 0.9 and share[20] > 0.9                           # at least one probe starts inside a cuboid
    assert rule_of(states_of(rows[0]))[18] == 1 and states_of(rows[0])[20] == INACTIVE | (1 << 1) | REJECTED
    assert np.abs(rows[0][18, :3]).max() > 0.3 and not states_of(rows[3])[18] & INACTIVE      # ... and leaves it
    return sc, tw, grid, rows, first


@pytest.mark.parametrize("w", FACES)
def test_the_reduction_is_the_references_bits(hip, ref, w):
    """synthetic planes that hold every rule, REJECTED, ties across lanes and across a lane's own texels, empties and poison; first_probe != 0; the rows of the
    probes outside the run keep their poison"""
    grid, rays = grid_of((3, 2, 4)), 6 * w * w
    seen = set()
    for n in PROBE_COUNTS:
        first = (7, 21, 0, 19, 15)[PROBE_COUNTS.index(n)]                  # 21 + 3 and 19 + 5 and 15 + 9 end at the grid's end
        for flags in (0, FREEZE):
            relocate = relocate_of(flags=flags)
            hit, normal, old, flavours = synthetic_case(n, w, n + w, relocate)
            host = np.full((24, 4), POISON, np.uint32).view(np.float32).copy()
            host[first:first + n] = old
            want = ref.relocate(grid, relocate, w, hit, normal, host, first_probe=first)
            d_hit, d_normal, d_offsets = device_words(hit, 0), device_words(normal, 0), device_words(host, SPARE * 4)
            torch.cuda.synchronize()
            assert hip.probe_relocate_device(grid, relocate, d_hit, d_normal, n, w, d_offsets, first) is d_offsets
            got = back(hip, d_offsets, 24 * 4, 4)
            assert_same_words(got, want, "w %d, %d probes from %d, flags %d" % (w, n, first, flags))
            outside = np.ones(24, bool)
            outside[first:first + n] = False
            assert (got[outside] == POISON).all()
            assert hip.last_volume_relocate() == {"probes": n, "face_size": w, "chunks": 0, "chunk": 0, "groups": (n + 3) // 4, "flags": flags, "first": first, "fused": 0}
            if flags:
                assert_same_words(got[first:first + n, :3], old[:, :3], "freeze")
            else:
                seen.update(int(s) for s in got[first:first + n, 3])
            if n == 5:
                assert_same_words(hip.probe_relocate(grid, relocate, hit, normal, n, w, host, first), want, "the host variant")
    assert {(s >> 1) & 3 for s in seen} == {1, 2, 3} and {s & (INACTIVE | REJECTED) for s in seen} == {0, INACTIVE, REJECTED, INACTIVE | REJECTED}


def test_the_reduction_needs_no_scene_and_crosses_workgroups(ref):
    grid = capi.VolumeGrid((0.1, -0.2, 0.3), (0.3, 0.7, 1.1), (7, 5, 3))      # 105 probes: 27 workgroups, the last of one wave
    relocate = relocate_of()
    hit, normal, old, _ = synthetic_case(105, 3, 4, relocate)
    want = ref.relocate(grid, relocate, 3, hit, normal, old)
    with capi.Context(0) as fresh:
        d_offsets = device_words(old, SPARE * 4)
        fresh.probe_relocate_device(grid, relocate, device_words(hit, 0), device_words(normal, 0), 105, 3, d_offsets)
        assert_same_words(back(fresh, d_offsets, 105 * 4, 4), want, "105 probes, a context without a scene")


@pytest.mark.parametrize("count", ((1, 1, 1), (2, 2, 2), (3, 2, 4)))
def test_positions_with_offsets_are_the_references_bits(hip, ref, count):
    grid = grid_of(count)
    probes = grid.probes
    rng = np.random.default_rng(probes)
    offsets = rng.uniform(-0.3, 0.3, size=(probes, 4)).astype(np.float32)
    offsets.view(np.uint32)[:, 3] = rng.integers(0, 16, size=probes)
    d_offsets = device_words(offsets, 0)

    def run(update, indices, n, what):
        want = ref.positions(grid, offsets, update, indices, n)
        out = device_words(np.full((len(want), 4), POISON, np.uint32), SPARE * 4)
        d_indices = device_words(indices, 0) if indices is not None else None
        torch.cuda.synchronize()
        assert hip.volume_positions_offset_device(grid, d_offsets, update, d_indices, n, out=out) is out
        assert_same_words(back(hip, out, len(want) * 4, 4), want, what)
        assert_same_words(hip.volume_positions_offset(grid, offsets, update, indices, n), want, what + ", the host variant")
        return want

    whole = run(None, None, None, "the whole grid")
    assert (whole[:, 3].view(np.uint32) == 0).all() and not np.array_equal(whole, ref.positions(grid, np.zeros_like(offsets)))
    listed = np.array([probes - 1, 0, probes, 0xffffffff, probes // 2], np.uint32)[:max(1, min(5, probes))]      # (n_list is at most the grid's probes)
    got = run(update_of(0.5), listed, None, "a list with skipped entries")
    assert_same_words(got, whole[[int(e) if e < probes else probes - 1 for e in listed]], "a skipped entry gets the last probe's row")
    stride = max(1, (probes - 1) // 2)
    n = min(3, probes)
    got = run(update_of(0.5, (probes - 1) - (n - 1) * stride, stride), None, n, "first + j stride")
    assert_same_words(got, whole[[(probes - 1) - (n - 1 - j) * stride for j in range(n)]], "first + j stride names those probes")


def test_the_whole_path_on_cornell_is_the_cpu_chain_and_its_parts(hip, ref, chain):
    sc, tw, grid, rows, first = chain
    hip.update_scene(sc)
    relocate, frozen, w, rays = cornell_relocate(), cornell_relocate(FREEZE), CORNELL_FACE, 6 * CORNELL_FACE * CORNELL_FACE
    zeros = np.zeros((24, 4), np.float32)
    # the parts, one after the other: positions, rays, surface rows, reduction
    d_parts = device_words(zeros, SPARE * 4)
    d_positions = hip.volume_positions_offset_device(grid, d_parts)
    d_rays = hip.probe_rays_device(d_positions, w)
    planes = hip.surface_rays_device(d_rays.view(-1, 8), FIELDS, tw)
    hip.probe_relocate_device(grid, relocate, planes[0], planes[1], 24, w, d_parts)
    parts = back(hip, d_parts, 24 * 4, 4)
    assert_same_words(planes.cpu().numpy().view(np.uint32)[0], first[0], "the HIT plane against the CPU chain")
    assert_same_words(planes.cpu().numpy().view(np.uint32)[1], first[1], "the NORMAL plane against the CPU chain")
    assert_same_words(parts, rows[0], "the parts against the CPU chain")
    # the whole call: in one chunk, in chunks of 1 and of 5 probes (the last of 4), and with trace slabs of 64 rays
    for chunk, slab, chunks in ((0, 0, 1), (1, 0, 24), (5, 0, 5), (0, 64, 1), (5, 64, 5)):
        hip.set_probe_chunk(chunk)
        hip.set_trace_slab(slab)
        try:
            d_offsets = device_words(zeros, SPARE * 4)
            torch.cuda.synchronize()
            assert hip.volume_relocate_device(grid, relocate, w, d_offsets, tw) is d_offsets
            assert_same_words(back(hip, d_offsets, 24 * 4, 4), parts, "chunk %d, slab %d" % (chunk, slab))
            m = 24 - (chunks - 1) * (chunk or 24)
            assert hip.last_volume_relocate() == {"probes": 24, "face_size": w, "chunks": chunks, "chunk": chunk or (1 << 21) // rays, "groups": (m + 3) // 4, "flags": 0, "first": 0,
                                                  "fused": 1}
            last = hip.last_surface()
            assert last["fields"] == FIELDS and last["n"] == m * rays and last["slab"] == (slab or 1 << 21)
            if chunk == 5 and slab == 64:
                assert_same_words(hip.volume_relocate(grid, relocate, w, zeros, tw), parts, "the host variant in chunks and slabs")
        finally:
            hip.set_probe_chunk(0)
            hip.set_trace_slab(0)
    # three passes and a frozen one equal the same sequence on the CPU
    d_offsets = device_words(zeros, SPARE * 4)
    for k in range(4):
        hip.volume_relocate_device(grid, frozen if k == 3 else relocate, w, d_offsets, tw)
        assert_same_words(back(hip, d_offsets, 24 * 4, 4), rows[k], "pass %d" % k)
    assert_same_words(rows[3][:, :3], rows[2][:, :3], "the frozen pass moves nothing")
    assert_same_words(hip.volume_relocate(grid, relocate, w, texture_width=tw), rows[0], "the host variant from zeros")


def relocated_case(grid, k, rng):
    """SH rows, map rows (size 2) and offset rows of a grid: about a third of the probes dead, their rows NaNs"""
    sh, maps = synthetic_sh(grid.probes, k), synthetic_maps(grid.probes, 2, k)
    offsets = rng.uniform(-0.2, 0.2, size=(grid.probes, 4)).astype(np.float32)
    dead = rng.random(grid.probes) < 0.35
    offsets.view(np.uint32)[:, 3] = np.where(dead, INACTIVE | (1 << 1) | REJECTED, 3 << 1)
    sh[dead] = np.nan
    maps[np.repeat(dead, 4)] = np.nan
    return sh, maps, offsets, dead


def device_relocated(ctx, grid, d_sh, positions, normals, d_offsets, vmap=None, d_maps=None):
    n = len(positions)
    out = device_words(np.full((n, 4), POISON, np.uint32), SPARE * 4)
    d_positions, d_normals = torch.from_numpy(positions).cuda(), torch.from_numpy(normals).cuda()
    torch.cuda.synchronize()
    assert ctx.volume_irradiance_relocated_device(grid, d_sh, d_positions, d_normals, d_offsets, vmap, d_maps, out=out) is out
    return back(ctx, out, n * 4, 4)


@pytest.mark.parametrize("count", COUNTS)
def test_the_relocated_lookup_is_the_references_bits(hip, ref, count):
    """test_volume_gpu.py's grids, point sets and n; with and without a map of size 2, sharpness 1; inactive corners that hold NaN rows; zero offsets are the plain
    lookup's rows"""
    vmap = map_of(2, 1)
    rng = np.random.default_rng(sum(count))
    for bias in (0.0, 0.125):
        grid = grid_of(count, bias)
        for k, kind in enumerate(POINT_SETS):
            sh, maps, offsets, dead = relocated_case(grid, k, rng)
            d_sh, d_maps, d_offsets = torch.from_numpy(sh).cuda(), torch.from_numpy(maps).cuda(), torch.from_numpy(offsets).cuda()
            clean_sh, clean_maps = synthetic_sh(grid.probes, k), synthetic_maps(grid.probes, 2, k)
            d_clean_sh, d_clean_maps, d_zero = torch.from_numpy(clean_sh).cuda(), torch.from_numpy(clean_maps).cuda(), torch.zeros((grid.probes, 4), device="cuda")
            for n in NS:
                what = "%s, n = %d, bias %g" % (kind, n, bias)
                positions, normals = point_set(grid, kind, n, 1000 * k + n)
                got = device_relocated(hip, grid, d_sh, positions, normals, d_offsets)
                assert_same_rows(got.view(np.float32), ref.lookup(grid, sh, offsets, positions, normals), what)
                assert hip.last_volume()["n"] == n and hip.last_volume()["groups"] == (n + 255) // 256
                got = device_relocated(hip, grid, d_sh, positions, normals, d_offsets, vmap, d_maps)
                assert_same_rows(got.view(np.float32), ref.lookup(grid, sh, offsets, positions, normals, vmap, maps), what + ", map")
                if n in (65, 1000):
                    plain = hip.volume_irradiance_device(grid, d_clean_sh, torch.from_numpy(positions).cuda(), torch.from_numpy(normals).cuda())
                    mapped = hip.volume_irradiance_map_device(grid, d_clean_sh, torch.from_numpy(positions).cuda(), torch.from_numpy(normals).cuda(), vmap, d_clean_maps)
                    hip.sync()
                    assert_same_rows(device_relocated(hip, grid, d_clean_sh, positions, normals, d_zero).view(np.float32), plain.cpu().numpy(), what + ", zero offsets")
                    assert_same_rows(device_relocated(hip, grid, d_clean_sh, positions, normals, d_zero, vmap, d_clean_maps).view(np.float32), mapped.cpu().numpy(),
                                     what + ", zero offsets, map")
                if kind == "misses" and n == 257:
                    assert_same_rows(hip.volume_irradiance_relocated(grid, sh, positions, normals, offsets), ref.lookup(grid, sh, offsets, positions, normals), what + ", host")
                    assert_same_rows(hip.volume_irradiance_relocated(grid, sh, positions, normals, offsets, vmap, maps), ref.lookup(grid, sh, offsets, positions, normals, vmap, maps),
                                     what + ", host, map")
    # all eight corners inactive: four zeros
    offsets.view(np.uint32)[:, 3] = INACTIVE
    positions, normals = point_set(grid, "outside", 300, 9)
    assert (device_relocated(hip, grid, d_sh, positions, normals, torch.from_numpy(offsets).cuda()) == 0).all()


def cornell_baked(hip, chain):
    """-> (scene, trace params with one sample and one bounce, probe params, the 64 x 48 frame, the grid, the relocated offsets on the device and on the host)"""
    sc, tw, grid, rows, _ = chain
    hip.update_scene(sc)
    p = sc.frame_params(width=64, height=48, samples=1, max_reflections=1, use_filter=0)
    t = capi.TraceParams.of_frame(p)
    return sc, t, capi.ProbeParams(face_size=2, sky=(0.5, 0.25, 0.125)), p, grid, torch.from_numpy(rows[3]).cuda(), rows[3]


@pytest.mark.parametrize("m", (None, 2))
def test_the_relocated_bake_and_update_are_their_parts(hip, ref, chain, m):
    sc, t, q, p, grid, d_offsets, offsets = cornell_baked(hip, chain)
    vmap, bins = map_of(m, 1) if m else None, (m or 0) ** 2
    # the bake: positions with offsets, then the probes
    d_positions = hip.volume_positions_offset_device(grid, d_offsets)
    want = hip.probes_sh_map_device(d_positions, t, q, vmap) if m else (hip.probes_sh_device(d_positions, t, q), None)
    hip.sync()
    want_sh, want_maps = want[0].cpu().numpy(), want[1].cpu().numpy() if m else None
    d_sh, d_maps = device_words(np.full((24, 36), POISON, np.uint32), SPARE * 36), device_words(np.full((24 * bins, 4), POISON, np.uint32), SPARE * 4) if m else None
    torch.cuda.synchronize()
    got = hip.volume_bake_relocated_device(grid, t, q, d_offsets, vmap, out=d_sh, maps=d_maps)
    assert got[0] is d_sh and got[1] is d_maps
    assert_same_words(back(hip, d_sh, 24 * 36, 36), want_sh, "the relocated bake")
    if m:
        assert_same_words(back(hip, d_maps, 24 * bins * 4, 4), want_maps, "the relocated bake's maps")
    plain = hip.volume_bake_device(grid, t, q)
    hip.sync()
    moved = np.abs(offsets[:, :3]).max(axis=1) > 0
    assert moved.sum() >= 2 and (plain.cpu().numpy()[moved] != want_sh[moved]).any(axis=1).all()      # a moved probe sees something else
    host = hip.volume_bake_relocated(grid, t, q, offsets, vmap)
    assert_same_words(host[0], want_sh, "the host variant")
    if m:
        assert_same_words(host[1], want_maps, "the host variant's maps")
    # the update: positions of a list with offsets, the probes, the blend
    indices = np.array([18, 0, 24, 12, 20], np.uint32)                   # the two probes that started inside, one that moved off a wall, one out of range
    d_indices, update = device_words(indices, 0), update_of(0.5)
    t2 = capi.TraceParams(t.samples, t.max_reflections, t.min_importancy, tuple(t.ambient), t.random_seed + 1.0, t.texture_width)
    d_list = hip.volume_positions_offset_device(grid, d_offsets, update, d_indices)
    fresh = hip.probes_sh_map_device(d_list, t2, q, vmap) if m else (hip.probes_sh_device(d_list, t2, q), None)
    part_sh, part_maps = device_words(want_sh, 0), device_words(want_maps, 0) if m else None
    part_state = hip.volume_blend_device(grid, vmap, update, fresh[0], part_sh, fresh[1], part_maps, d_indices, state=True)
    hip.sync()
    got_sh, got_maps, d_state = device_words(want_sh, SPARE * 36), device_words(want_maps, SPARE * 4) if m else None, device_words(np.full(5, POISON, np.uint32), SPARE)
    torch.cuda.synchronize()
    assert hip.volume_update_relocated_device(grid, t2, q, vmap, update, d_offsets, got_sh, got_maps, d_indices, state=d_state) is d_state
    assert_same_words(back(hip, got_sh, 24 * 36, 36), part_sh.cpu().numpy().view(np.uint32).reshape(-1, 36), "the relocated update")
    if m:
        assert_same_words(back(hip, got_maps, 24 * bins * 4, 4), part_maps.cpu().numpy().view(np.uint32).reshape(-1, 4), "the relocated update's maps")
    states = back(hip, d_state, 5, 1).reshape(-1).tolist()
    assert states == part_state.cpu().numpy().view(np.uint32).tolist() and states[2] == 3 and states.count(BLENDED) >= 2
    host = hip.volume_update_relocated(grid, t2, q, vmap, update, offsets, want_sh, want_maps, indices)
    assert_same_words(host[0], part_sh.cpu().numpy().view(np.uint32).reshape(-1, 36), "the update's host variant")
    assert host[2].tolist() == states


def test_relocated_frame_and_rays_are_surface_then_lookup(hip, ref, oracle, scenes, chain):
    sc, t, q, p, grid, d_offsets, offsets = cornell_baked(hip, chain)
    vmap = map_of(2, 1)
    d_sh, d_maps = hip.volume_bake_relocated_device(grid, t, q, d_offsets, vmap)
    surface = capi.SURFACE_POSITION | capi.SURFACE_NORMAL
    planes = hip.frame_surface_device(p, surface)
    hip.sync()
    sh, maps, host_planes = d_sh.cpu().numpy(), d_maps.cpu().numpy(), planes.cpu().numpy()
    n = 64 * 48
    from rays_trace_util import camera_rays
    rays = camera_rays(oracle, scenes, "cornell")[2]
    rays = np.ascontiguousarray(rays[np.linspace(0, len(rays) - 1, 300).astype(int)], np.float32)
    rays[::11, 4:7] *= -1.0
    d_rays = torch.from_numpy(rays).cuda()
    ray_planes = hip.surface_rays_device(d_rays, surface, p.texture_width)
    for with_map in (False, True):
        mm, dm, hm = (vmap, d_maps, maps) if with_map else (None, None, None)
        want = hip.volume_irradiance_relocated_device(grid, d_sh, planes[0], planes[1], d_offsets, mm, dm)
        hip.sync()
        want = want.cpu().numpy()
        hit = host_planes[0][:, 3] != 0.0
        lit = want[:, 3] > 0              # (a point whose eight corners are all the dead probe 20 — the tall cuboid's front, beyond the grid's corner — gets four zeros)
        assert hit.sum() > 1000 and lit.sum() > 1000 and not lit[~hit].any() and (want[~lit] == 0).all() and 0 < (hit & ~lit).sum() < hit.sum() // 4
        assert_same_rows(want, ref.lookup(grid, sh, offsets, host_planes[0], host_planes[1], mm, hm), "the chain against the reference, map %d" % with_map)
        out = device_words(np.full((n, 4), POISON, np.uint32), SPARE * 4)
        torch.cuda.synchronize()
        assert hip.frame_irradiance_relocated_device(p, grid, d_sh, d_offsets, mm, dm, out=out) is out
        assert_same_rows(back(hip, out, n * 4, 4).view(np.float32), want, "the frame call, map %d" % with_map)
        assert hip.last_volume()["source"] == 2 and hip.last_volume()["n"] == n
        assert_same_rows(hip.frame_irradiance_relocated(p, grid, sh, offsets, mm, hm).reshape(-1, 4), want, "the frame call's host variant")
        want = hip.volume_irradiance_relocated_device(grid, d_sh, ray_planes[0], ray_planes[1], d_offsets, mm, dm)
        hip.sync()
        want = want.cpu().numpy()
        assert (want[:, 3] > 0).sum() > 100
        for slab, slabs in ((0, 1), (64, 5)):
            hip.set_trace_slab(slab)
            try:
                out = device_words(np.full((300, 4), POISON, np.uint32), SPARE * 4)
                torch.cuda.synchronize()
                assert hip.rays_irradiance_relocated_device(grid, d_sh, d_rays, d_offsets, mm, dm, p.texture_width, out=out) is out
                assert_same_rows(back(hip, out, 300 * 4, 4).view(np.float32), want, "the rays call, slab %d, map %d" % (slab, with_map))
                assert hip.last_volume()["slabs"] == slabs and hip.last_volume()["source"] == 1
            finally:
                hip.set_trace_slab(0)
        assert_same_rows(hip.rays_irradiance_relocated(grid, sh, rays, offsets, mm, hm, p.texture_width), want, "the rays call's host variant")
    # the dead probe (20, inside the tall cuboid) gets no weight: poisoning its rows changes no bit
    assert states_of(offsets)[20] & INACTIVE
    poisoned_sh = sh.copy()
    poisoned_sh[20] = np.nan
    a = hip.volume_irradiance_relocated_device(grid, torch.from_numpy(poisoned_sh).cuda(), planes[0], planes[1], d_offsets)
    b = hip.volume_irradiance_relocated_device(grid, d_sh, planes[0], planes[1], d_offsets)
    hip.sync()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_a_pass_between_two_frames_of_the_loop(hip, oracle, chain):
    sc, tw, grid, rows, _ = chain
    hip.update_scene(sc)
    frames = [sc.frame_params(width=48, height=36, samples=2, max_reflections=3, use_filter=0) for _ in range(2)]
    frames[1].random_seed = frames[0].random_seed + 1.0
    oracle_frames = [oracle.render(sc, f)[0] for f in frames]
    d_offsets = device_words(np.zeros((24, 4), np.float32), SPARE * 4)
    torch.cuda.synchronize()
    for f in frames:
        hip.frame_begin(f)
    assert hip.frames_in_flight() == 2
    hip.volume_relocate_device(grid, cornell_relocate(), CORNELL_FACE, d_offsets, tw)
    got = [hip.frame_end()[0] for _ in frames]
    assert_same_words(back(hip, d_offsets, 24 * 4, 4), rows[0], "between the frames")
    for image, frame in zip(got, oracle_frames):
        image = np.asarray(image).reshape(frame.shape)
        assert ((image.view(np.uint32) == frame.view(np.uint32)) | (np.isnan(image) & np.isnan(frame))).all()


def test_refusals(hip, chain):
    sc, tw, grid, rows, _ = chain
    hip.update_scene(sc)
    torch.cuda.empty_cache()                                             # (the allocations below are then the device's own, of exactly these sizes)
    good, w, rays = cornell_relocate(), 2, 24
    hip.volume_relocate(grid, good, w, texture_width=tw)
    before = (hip.last_volume_relocate(), hip.last_surface(), hip.last_volume())

    def poison(n_bytes):
        return torch.full((n_bytes,), 0xA5, dtype=torch.uint8, device="cuda")

    d_hit, d_normal, d_offsets, d_positions, d_indices, d_sh, d_points, d_normals, d_out = (poison(5 * rays * 16), poison(5 * rays * 16), poison(24 * 16), poison(24 * 16), poison(5 * 4),
                                                                                          poison(24 * 144), poison(7 * 16), poison(7 * 16), poison(7 * 16))
    short = poison(20 << 20)                                             # 20 MB, an allocation of its own: an array that ends a row past END is too short
    host = np.zeros((4096, 4), np.float32)
    torch.cuda.synchronize()
    H, N, O, P, I, S, X, Y, Z = (x.data_ptr() for x in (d_hit, d_normal, d_offsets, d_positions, d_indices, d_sh, d_points, d_normals, d_out))
    END = short.data_ptr() + (20 << 20)

    reduce = lambda r=good, h=H, nn=N, n=5, ww=w, f=3, o=O, gr=grid: hip.probe_relocate_device(gr, r, h, nn, n, ww, o, f)
    whole = lambda r=good, ww=w, o=O, gr=grid, t=tw: hip.volume_relocate_device(gr, r, ww, o, t)
    positions = lambda u=None, i=None, n=None, o=P, f=O, gr=grid: hip.volume_positions_offset_device(gr, f, u, i, n, out=o)
    lookup = lambda f=O, s=S, x=X, y=Y, z=Z, vm=None, m=None, gr=grid: hip.volume_irradiance_relocated_device(gr, s, x, y, f, vm, m, n=7, out=z)
    refused = []
    for name, call in (("flx_probe_relocate_device", reduce), ("flx_volume_relocate_device", whole)):
        bad = lambda **kw: relocate_of(**kw)
        refused += [
            (lambda call=call: call(r=None), name + ": the relocation is NULL"),
            (lambda call=call: call(r=bad(back_share=float("nan"))), name + ": back_share is not one of 0 .. 1"),
            (lambda call=call: call(r=bad(back_share=1.001)), name + ": back_share is not one of 0 .. 1"),
            (lambda call=call: call(r=bad(back_share=-0.001)), name + ": back_share is not one of 0 .. 1"),
            (lambda call=call: call(r=bad(min_front=-0.001)), name + ": min_front is negative or not finite"),
            (lambda call=call: call(r=bad(min_front=float("inf"))), name + ": min_front is negative or not finite"),
            (lambda call=call: call(r=bad(reach=0.0)), name + ": reach is not greater than 0 or not finite"),
            (lambda call=call: call(r=bad(reach=float("inf"))), name + ": reach is not greater than 0 or not finite"),
            (lambda call=call: call(r=bad(limit=0.501)), name + ": limit is not one of 0 .. 0.5"),
            (lambda call=call: call(r=bad(limit=float("nan"))), name + ": limit is not one of 0 .. 0.5"),
            (lambda call=call: call(r=bad(flags=2)), name + ": flags has a bit beyond FLX_VOLUME_RELOCATE_FREEZE"),
            (lambda call=call: call(r=bad(reserved=1)), name + ": the relocation's reserved word is not 0"),
            (lambda call=call: call(ww=0), name + ": face_size is not one of 1 .. 256"),
            (lambda call=call: call(ww=257), name + ": face_size is not one of 1 .. 256"),
            (lambda call=call: call(o=0), name + ": an array is NULL"),
            (lambda call=call: call(o=O + 4), name + ": an array is misaligned"),
            (lambda call=call: call(o=host.ctypes.data), name + ": the offsets are not nx \\* ny \\* nz rows of 16 bytes in memory of the context's device"),
            (lambda call=call: call(o=END - 24 * 16 + 16), name + ": the offsets are not nx \\* ny \\* nz rows of 16 bytes in memory of the context's device"),
            # the order: the relocation before the face size, the siblings before both
            (lambda call=call: call(r=bad(limit=1.0), ww=0), name + ": limit is not one of 0 .. 0.5"),
            (lambda call=call: call(gr=None, r=None), name + ": the grid is NULL"),
            (lambda call=call: call(gr=capi.VolumeGrid(count=(0, 1, 1)), r=None), name + ": a count of the grid is 0"),
        ]
    refused += [
        (lambda: reduce(f=20), "flx_probe_relocate_device: first_probe \\+ n_probes is beyond the grid's probes"),
        (lambda: reduce(f=0xffffffff, n=1), "flx_probe_relocate_device: first_probe \\+ n_probes is beyond the grid's probes"),      # (a 32-bit sum is 0)
        (lambda: reduce(n=25, f=0), "flx_probe_relocate_device: first_probe \\+ n_probes is beyond the grid's probes"),
        (lambda: hip.probe_relocate_device(capi.VolumeGrid(count=(1024, 1024, 1024)), good, H, N, 10923, 256, O, 0), "flx_probe_relocate_device: n_probes \\* 6 \\* face_size \\* face_size is 2\\^32 or more"),
        (lambda: reduce(h=0), "flx_probe_relocate_device: an array is NULL"),
        (lambda: reduce(nn=0), "flx_probe_relocate_device: an array is NULL"),
        (lambda: reduce(h=H + 8), "flx_probe_relocate_device: an array is misaligned"),
        (lambda: reduce(h=host.ctypes.data), "flx_probe_relocate_device: the HIT plane is not n_probes \\* 6 \\* face_size \\* face_size rows of 16 bytes in memory of the context's device"),
        (lambda: reduce(nn=END - 5 * rays * 16 + 16), "flx_probe_relocate_device: the NORMAL plane is not n_probes \\* 6 \\* face_size \\* face_size rows of 16 bytes in memory of the context's device"),
        (lambda: reduce(nn=H), "flx_probe_relocate_device: the arrays overlap"),
        (lambda: reduce(h=S + 16 * rays, nn=S, n=2), "flx_probe_relocate_device: the arrays overlap"),      # the last row of another
        (lambda: reduce(h=S, n=1, o=S + 16), "flx_probe_relocate_device: the arrays overlap"),
        (lambda: whole(t=0), "flx_rays_surface_device: texture_width"),
        (lambda: positions(f=0), "flx_volume_positions_offset_device: an array is NULL"),
        (lambda: positions(o=0), "flx_volume_positions_offset_device: an array is NULL"),
        (lambda: positions(f=O + 8), "flx_volume_positions_offset_device: an array is misaligned"),
        (lambda: positions(o=O), "flx_volume_positions_offset_device: the arrays overlap"),
        (lambda: positions(u=update_of(0.5), n=1, o=O + 16 * 23), "flx_volume_positions_offset_device: the arrays overlap"),      # the last row of the offsets
        (lambda: positions(o=END - 24 * 16 + 16), "flx_volume_positions_offset_device: the positions are not n rows of 16 bytes in memory of the context's device"),
        (lambda: positions(n=23), "flx_volume_positions_offset_device: n is not nx \\* ny \\* nz for the whole grid"),
        (lambda: positions(i=I, n=5), "flx_volume_positions_offset_device: indices are given without an update"),
        (lambda: positions(u=update_of(2.0), i=I, n=5), "flx_volume_positions_offset_device: hysteresis is not one of 0 .. 1"),
        (lambda: positions(u=update_of(0.5), i=I, n=25), "flx_volume_positions_offset_device: n_list is above the grid's probes"),
        (lambda: positions(u=update_of(0.5, 20, 1), n=5), "flx_volume_positions_offset_device: first \\+ \\(n_list - 1\\) \\* stride is not a probe of the grid"),
        (lambda: positions(u=update_of(0.5), i=I + 2, n=5), "flx_volume_positions_offset_device: an array is misaligned"),
        (lambda: positions(u=update_of(0.5), i=O + 32, n=5), "flx_volume_positions_offset_device: the arrays overlap"),
        (lambda: positions(gr=None), "flx_volume_positions_offset_device: the grid is NULL"),
        (lambda: lookup(f=0), "flx_volume_irradiance_relocated_device: an array is NULL"),
        (lambda: lookup(f=O + 4), "flx_volume_irradiance_relocated_device: an array is misaligned"),
        (lambda: lookup(f=host.ctypes.data), "flx_volume_irradiance_relocated_device: the offsets are not nx \\* ny \\* nz rows of 16 bytes in memory of the context's device"),
        (lambda: lookup(f=END - 24 * 16 + 16), "flx_volume_irradiance_relocated_device: the offsets are not nx \\* ny \\* nz rows of 16 bytes in memory of the context's device"),
        (lambda: lookup(f=S + 144), "flx_volume_irradiance_relocated_device: the arrays overlap"),
        (lambda: lookup(f=Z, gr=grid_of((1, 1, 1))), "flx_volume_irradiance_relocated_device: the arrays overlap"),
        (lambda: lookup(s=0), "flx_volume_irradiance_relocated_device: an array is NULL"),                      # the siblings' come first, in their words
        (lambda: lookup(gr=None, f=0), "flx_volume_irradiance_relocated_device: the grid is NULL"),
        (lambda: lookup(vm=capi.VolumeMap(17, 1), m=S, f=0), "flx_volume_irradiance_relocated_device: the map's size is not one of 1 .. 16"),
        (lambda: lookup(vm=capi.VolumeMap(2, 1), m=None), "flx_volume_irradiance_relocated_device: the maps array is NULL"),       # a map without its maps: the map calls' words
        (lambda: lookup(vm=None, m=S), "flx_volume_irradiance_relocated_device: the map is NULL"),
        # the host variants: the same rules
        (lambda: hip.volume_relocate(grid, relocate_of(reach=-1.0), w, texture_width=tw), "flx_volume_relocate: reach is not greater than 0 or not finite"),
        (lambda: hip.probe_relocate(grid, good, np.zeros((rays, 4), np.float32), np.zeros((rays, 4), np.float32), 1, w, np.zeros((24, 4), np.float32), 24),
         "flx_probe_relocate: first_probe \\+ n_probes is beyond the grid's probes"),
        (lambda: hip.volume_positions_offset(grid, np.zeros((23, 4), np.float32)), "one offset row per probe"),
    ]
    for call, words in refused:
        with pytest.raises((capi.FlexLightHipError, ValueError), match=r"(failed \(\d+\): .*(" + words + "))|(" + words + ")"):
            call()
    hip.sync()
    for buffer in (d_hit, d_normal, d_offsets, d_positions, d_indices, d_sh, d_points, d_normals, d_out, short):
        assert bool((buffer == 0xA5).all())                              # nothing was written
    # a host list that names a probe twice is no error here: positions are only read
    assert hip.volume_positions_offset(grid, np.zeros((24, 4), np.float32), update_of(0.5), [1, 5, 1]).shape == (3, 4)
    # no probes, no points: FLX_OK and nothing enqueued, the rules that need no array looked at first
    hip.probe_relocate_device(grid, good, 0, 0, 0, w, 0, 24)
    hip.volume_irradiance_relocated_device(grid, 0, 0, 0, 0, n=0, out=0)
    with pytest.raises(capi.FlexLightHipError, match="flx_probe_relocate_device: limit is not one of 0 .. 0.5"):
        hip.probe_relocate_device(grid, relocate_of(limit=2.0), 0, 0, 0, w, 0, 0)
    assert (hip.last_volume_relocate(), hip.last_surface(), hip.last_volume()) == before
    # the calls still work
    assert_same_words(hip.volume_relocate(grid, cornell_relocate(), CORNELL_FACE, texture_width=tw), rows[0], "after the refusals")
