"""Directional visibility on the device (include/flexlight_hip_debug.h, "directional visibility"): k_probe_map's rows and the map lookup's rows are the CPU
reference's bits (tests/volume_map_ref, the same include/flx_volume_map.h) for every face size, map size, sharpness, probe count, grid and point set at which the
kernels can go wrong; the fused calls are the calls they are made of, bit for bit, whatever the chunk or slab; a map lookup between two frames of the loop leaves them
alone; the plain calls give what they gave; every refusal says its words and leaves the outputs as they were."""
import numpy as np
import pytest
import torch

from flexlight_hip import capi
from probe_util import assert_same_words, cornell_probes
from volume_map_util import (COUNTS, POINT_SETS, assert_same_rows, finished, grid_of, map_of, map_radiance, point_set, poisoned, reference, synthetic_maps, synthetic_sh,
                             volume_reference)

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 255, 256, 257, 1000)      # a lane; a wave less one, a wave, a wave and a lane; the same of a workgroup; four workgroups, the last one short
SURFACE = capi.SURFACE_POSITION | capi.SURFACE_NORMAL
# (w, m, k, probes): every face size of 1 2 3 4 5 8 11 16, every map size of 1 2 3 4 8 16, every sharpness of 0 1 5 8, every probe count of 1 3 4 5 9, and the
# corners (1, 1), (1, 16), (16, 1), (16, 16).  w <= 3: lanes without a texel; m = 1: three of four waves without a bin; m = 3: a wave with one bin of four; m = 8,
# 16: 4 and 16 workgroups a probe; w = 16: two tiles of texels, the second one half full.
ROW_CASES = ((1, 1, 0, 1), (1, 16, 5, 3), (16, 1, 1, 4), (16, 16, 8, 3), (2, 2, 1, 5), (3, 3, 5, 9), (4, 4, 0, 4), (5, 8, 8, 5), (8, 8, 5, 9), (11, 3, 1, 3), (8, 16, 0, 1),
             (2, 4, 8, 1))
MAP_SIZES = (1, 3, 8, 16)                       # the map of the lookup tests' grid k


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return reference(tmp_path_factory)


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return volume_reference(tmp_path_factory)


def device_maps(ctx, radiance, n, w, vmap):
    """k_probe_map through flx_probe_map_device into a poisoned output -> float32 [n * bins, 4]"""
    out = poisoned(n * vmap.bins, 16)
    d_radiance = torch.from_numpy(radiance).cuda()
    torch.cuda.synchronize()
    assert ctx.probe_map_device(d_radiance, n, w, vmap, out=out) is out
    return finished(ctx, out, n * vmap.bins, 4).view(np.float32)


@pytest.mark.parametrize("w,m,k,n", ROW_CASES)
def test_map_rows_are_the_references_bits(hip, ref, w, m, k, n):
    vmap = map_of(m, k)
    radiance = map_radiance(n, w, 100 * w + m, nan=n != 1 or w == 2)
    want = ref.rows(radiance, n, w, vmap)
    got = device_maps(hip, radiance, n, w, vmap)
    assert_same_rows(got, want, "w %d, m %d, k %d, %d probes" % (w, m, k, n))
    assert hip.last_volume_map() == {"probes": n, "size": m, "sharpness": k, "launches": 1, "groups": n * ((m * m + 15) // 16), "face_size": w}
    if n >= 3:
        assert (got.reshape(n, m * m, 4)[1, :, 0:3].view(np.uint32) == 0).all() and (got.reshape(n, m * m, 4)[2, :, 0] > 0).any()      # only misses; only hits
    if n != 1 or w == 2:
        assert np.isnan(got.reshape(n, m * m, 4)[n - 1, :, 1:3]).all() and np.isfinite(got.reshape(n, m * m, 4)[:n - 1]).all()          # the NaN distance
    rays = 6 * w * w
    for p in range(n):                                     # a probe's rows depend on nothing else in the call
        assert_same_rows(device_maps(hip, radiance[p * rays:(p + 1) * rays], 1, w, vmap), want[p * m * m:(p + 1) * m * m], "probe %d alone" % p)
    if (w, m) == (5, 8):
        assert_same_rows(hip.probe_map(radiance, n, w, vmap), want, "the host variant")


def test_a_face_of_many_tiles(hip, ref):
    """w = 64: 24 576 texels are 24 tiles of 1024; the partial sums cross them in registers"""
    w, vmap = 64, map_of(4, 5)
    radiance = map_radiance(1, w, 9, nan=False)
    assert_same_rows(device_maps(hip, radiance, 1, w, vmap), ref.rows(radiance, 1, w, vmap), "w 64, m 4")
    radiance[6 * w * w - 1, 3:5] = (1.0, np.nan)           # ... and the last texel of the last tile is read
    got = device_maps(hip, radiance, 1, w, vmap)
    assert_same_rows(got, ref.rows(radiance, 1, w, vmap), "w 64, m 4, a NaN in the last texel")
    assert np.isnan(got[:, 1]).all()


def test_maps_need_no_scene(ref):
    w, vmap = 3, map_of(5, 3)
    radiance = map_radiance(4, w, 2)
    with capi.Context(0) as fresh:
        assert_same_rows(device_maps(fresh, radiance, 4, w, vmap), ref.rows(radiance, 4, w, vmap), "a context without a scene")
        assert_same_rows(fresh.probe_map(radiance, 4, w, vmap), ref.rows(radiance, 4, w, vmap), "its host variant")


def test_fused_probes_are_their_parts(hip, oracle, scenes, ref):
    sc, t, positions = cornell_probes(oracle, scenes)
    hip.update_scene(sc)
    w, n, vmap = 8, 5, map_of(8, 5)
    d_positions = torch.from_numpy(positions).cuda()
    torch.cuda.synchronize()
    sky = (0.5, 0.25, 0.125)
    params = capi.ProbeParams(face_size=w, sky=sky)
    generated = hip.probe_rays_device(d_positions, w)
    radiance = hip.trace_rays_ordered_device(generated, t, order=0)
    # the parts in both orders: the SH rows then the maps, the maps then the SH rows
    sh_first = hip.probe_reduce_device(radiance, n, params)
    maps_second = hip.probe_map_device(radiance, n, w, vmap)
    maps_first = hip.probe_map_device(radiance, n, w, vmap)
    sh_second = hip.probe_reduce_device(radiance, n, params)
    plain_sh = hip.probes_sh_device(d_positions, t, params)
    hip.sync()
    want_sh, want_maps = sh_first.cpu().numpy(), maps_second.cpu().numpy()
    assert_same_words(sh_second.cpu().numpy(), want_sh, "the SH rows behind the maps")
    assert_same_rows(maps_first.cpu().numpy(), want_maps, "the maps before the SH rows")
    assert_same_words(plain_sh.cpu().numpy(), want_sh, "flx_probes_sh_device")
    assert_same_rows(want_maps, ref.rows(radiance.cpu().numpy().view(np.float32).reshape(-1, 8), n, w, vmap), "the maps against the reference")
    assert np.isfinite(want_maps).all() and (want_maps[:, 0] > 0).any() and (want_maps[:, 0] <= want_maps[:, 3]).all()
    for chunk, chunks in ((2, 3), (0, 1)):
        hip.set_probe_chunk(chunk)
        try:
            out, maps = poisoned(n, 144), poisoned(n * 64, 16)
            torch.cuda.synchronize()
            got = hip.probes_sh_map_device(d_positions, t, params, vmap, out=out, maps=maps)
            assert got[0] is out and got[1] is maps
            assert_same_words(finished(hip, out, n, 36), want_sh, "the fused SH rows, chunk %d" % chunk)
            assert_same_rows(finished(hip, maps, n * 64, 4).view(np.float32), want_maps, "the fused maps, chunk %d" % chunk)
            assert hip.last_probes()["chunks"] == chunks
            assert hip.last_volume_map() == {"probes": n, "size": 8, "sharpness": 5, "launches": 1, "groups": 4 * (1 if chunk else n), "face_size": w}
            if chunk:
                host_sh, host_maps = hip.probes_sh_map(positions, t, params, vmap)
                assert_same_words(host_sh, want_sh, "the host variant's SH rows in chunks")
                assert_same_rows(host_maps, want_maps, "the host variant's maps in chunks")
        finally:
            hip.set_probe_chunk(0)


def cornell_volume(hip, oracle, scenes):
    """-> (scene, trace params, probe params with face size 4, a frame of 64 x 48, a 2 x 2 x 2 grid inside the hull of the frame's first hits): test_volume_gpu.py's"""
    sc, t, _ = cornell_probes(oracle, scenes)
    hip.update_scene(sc)
    p = sc.frame_params(width=64, height=48, samples=1, max_reflections=3, use_filter=0)
    planes = hip.frame_surface(p, capi.SURFACE_POSITION)[0]
    hit = planes[planes[:, 3] != 0.0][:, :3]
    lo, hi = hit.min(axis=0), hit.max(axis=0)
    grid = capi.VolumeGrid(lo + 0.2 * (hi - lo), 0.6 * (hi - lo), (2, 2, 2), normal_bias=0.01 * float((hi - lo).max()))
    return sc, t, capi.ProbeParams(face_size=4, sky=(0.5, 0.25, 0.125)), p, grid


def test_bake_with_maps_is_positions_then_fused(hip, oracle, scenes):
    sc, t, q, p, grid = cornell_volume(hip, oracle, scenes)
    vmap = map_of(4, 3)
    d_positions = hip.volume_positions_device(grid)
    want_sh, want_maps = hip.probes_sh_map_device(d_positions, t, q, vmap)
    plain_sh = hip.volume_bake_device(grid, t, q)
    hip.sync()
    want_sh, want_maps = want_sh.cpu().numpy(), want_maps.cpu().numpy()
    assert_same_words(plain_sh.cpu().numpy(), want_sh, "flx_volume_bake_device")
    out, maps = poisoned(8, 144), poisoned(8 * 16, 16)
    torch.cuda.synchronize()
    got = hip.volume_bake_map_device(grid, t, q, vmap, out=out, maps=maps)
    assert got[0] is out and got[1] is maps
    assert_same_words(finished(hip, out, 8, 36), want_sh, "the bake's SH rows")
    assert_same_rows(finished(hip, maps, 8 * 16, 4).view(np.float32), want_maps, "the bake's maps")
    assert hip.last_volume_map()["probes"] == 8
    host_sh, host_maps = hip.volume_bake_map(grid, t, q, vmap)
    assert_same_words(host_sh, want_sh, "the host variant's SH rows")
    assert_same_rows(host_maps, want_maps, "the host variant's maps")


def device_lookup(ctx, grid, vmap, d_sh, d_maps, positions, normals):
    n = len(positions)
    out = poisoned(n, 16)
    d_positions, d_normals = torch.from_numpy(positions).cuda(), torch.from_numpy(normals).cuda()
    torch.cuda.synchronize()
    assert ctx.volume_irradiance_map_device(grid, d_sh, d_positions, d_normals, vmap, d_maps, out=out) is out
    return finished(ctx, out, n, 4).view(np.float32)


@pytest.mark.parametrize("k", range(len(COUNTS)))
def test_the_map_lookup_is_the_references_bits(hip, ref, plain, k):
    """every point set, n, flag and bias, over synthetic maps that hold rows nothing hit, negative coverages and NaNs"""
    count, vmap = COUNTS[k], map_of(MAP_SIZES[k], 5)
    for visibility in (True, False):
        for bias in (0.0, 0.125):
            grid = grid_of(count, bias, visibility)
            for j, kind in enumerate(POINT_SETS):
                sh, maps = synthetic_sh(grid.probes, j), synthetic_maps(grid.probes, vmap.size, j)
                d_sh, d_maps = torch.from_numpy(sh).cuda(), torch.from_numpy(maps).cuda()
                for n in NS:
                    what = "%s, n = %d, visibility %d, bias %g" % (kind, n, visibility, bias)
                    positions, normals = point_set(grid, kind, n, 1000 * j + n)
                    want = ref.irradiance(grid, vmap, sh, maps, positions, normals)
                    assert_same_rows(device_lookup(hip, grid, vmap, d_sh, d_maps, positions, normals), want, what)
                    last = hip.last_volume()
                    assert last == {"n": n, "slabs": 1, "slab": n, "probes": grid.probes, "flags": grid.flags, "source": 0, "groups": (n + 255) // 256}, last
                    if not visibility and n == 257:
                        assert_same_rows(want, plain.irradiance(grid, sh, positions, normals), what + ": without the flag, the plain lookup")
                    if kind == "misses" and n == 257:
                        assert_same_rows(hip.volume_irradiance_map(grid, sh, positions, normals, vmap, maps), want, what + ", the host variant")


def test_frame_and_rays_with_maps_are_surface_then_lookup(hip, oracle, scenes, ref):
    sc, t, q, p, grid = cornell_volume(hip, oracle, scenes)
    vmap = map_of(8, 5)
    d_sh, d_maps = hip.volume_bake_map_device(grid, t, q, vmap)
    # the plain calls before the map calls
    plain_frame = hip.frame_irradiance_device(p, grid, d_sh)
    # a frame
    planes = hip.frame_surface_device(p, SURFACE)
    want = hip.volume_irradiance_map_device(grid, d_sh, planes[0], planes[1], vmap, d_maps)
    hip.sync()
    sh, maps, want, host_planes, plain_frame = d_sh.cpu().numpy(), d_maps.cpu().numpy(), want.cpu().numpy(), planes.cpu().numpy(), plain_frame.cpu().numpy()
    hit = host_planes[0][:, 3] != 0.0
    assert hit.sum() > 1000 and np.isfinite(want).all() and (want[hit][:, 3] > 0).all() and (want[~hit] == 0).all()
    assert_same_rows(want, ref.irradiance(grid, vmap, sh, maps, host_planes[0], host_planes[1]), "the chain over baked maps against the reference")
    assert not np.array_equal(want, plain_frame.reshape(-1, 4))        # the maps weigh the probes differently
    n = 64 * 48
    out = poisoned(n, 16)
    torch.cuda.synchronize()
    assert hip.frame_irradiance_map_device(p, grid, d_sh, vmap, d_maps, out=out) is out
    assert_same_rows(finished(hip, out, n, 4).view(np.float32), want, "the frame call")
    assert hip.last_volume() == {"n": n, "slabs": 1, "slab": n, "probes": 8, "flags": 1, "source": 2, "groups": 12}
    assert_same_rows(hip.frame_irradiance_map(p, grid, sh, vmap, maps).reshape(-1, 4), want, "the frame call's host variant")
    # ... and the plain call behind them gives what it gave
    again = hip.frame_irradiance_device(p, grid, d_sh)
    hip.sync()
    assert_same_rows(again.cpu().numpy().reshape(-1, 4), plain_frame.reshape(-1, 4), "the plain frame call after a map call")
    # 300 rays: pixels of the frame, strided, some turned away
    from rays_trace_util import camera_rays
    rays = camera_rays(oracle, scenes, "cornell")[2]
    rays = np.ascontiguousarray(rays[np.linspace(0, len(rays) - 1, 300).astype(int)], np.float32)
    rays[::11, 4:7] *= -1.0
    d_rays = torch.from_numpy(rays).cuda()
    torch.cuda.synchronize()
    plain_rays = hip.rays_irradiance_device(grid, d_sh, d_rays, p.texture_width)
    planes = hip.surface_rays_device(d_rays, SURFACE, p.texture_width)
    want = hip.volume_irradiance_map_device(grid, d_sh, planes[0], planes[1], vmap, d_maps)
    hip.sync()
    want, plain_rays = want.cpu().numpy(), plain_rays.cpu().numpy()
    assert (want[:, 3] > 0).sum() > 100
    for slab, slabs in ((0, 1), (64, 5), (100, 3)):          # flx_debug_set_trace_slab: 300 rays in 5 slabs (the last of 44) and in 3 of 100
        hip.set_trace_slab(slab)
        try:
            out = poisoned(300, 16)
            torch.cuda.synchronize()
            assert hip.rays_irradiance_map_device(grid, d_sh, d_rays, vmap, d_maps, p.texture_width, out=out) is out
            assert_same_rows(finished(hip, out, 300, 4).view(np.float32), want, "the rays call, slab %d" % slab)
            last = hip.last_volume()
            assert last == {"n": 300, "slabs": slabs, "slab": slab or 1 << 21, "probes": 8, "flags": 1, "source": 1, "groups": 2 if slab == 0 else 1}, last
            if slab == 100:
                assert_same_rows(hip.rays_irradiance_map(grid, sh, rays, vmap, maps, p.texture_width), want, "the rays call's host variant in slabs")
        finally:
            hip.set_trace_slab(0)
    again = hip.rays_irradiance_device(grid, d_sh, d_rays, p.texture_width)
    hip.sync()
    assert_same_rows(again.cpu().numpy(), plain_rays, "the plain rays call after a map call")


def test_a_map_lookup_between_two_frames_of_the_loop(hip, oracle, scenes):
    sc, t, q, p, grid = cornell_volume(hip, oracle, scenes)
    vmap = map_of(4, 5)
    sh, maps = hip.volume_bake_map(grid, t, q, vmap)
    want = hip.frame_irradiance_map(p, grid, sh, vmap, maps).reshape(-1, 4)
    frames = [sc.frame_params(width=48, height=36, samples=2, max_reflections=3, use_filter=0) for _ in range(2)]
    frames[1].random_seed = frames[0].random_seed + 1.0
    oracle_frames = [oracle.render(sc, f)[0] for f in frames]
    d_sh, d_maps = torch.from_numpy(sh).cuda(), torch.from_numpy(maps).cuda()
    out = poisoned(64 * 48, 16)
    torch.cuda.synchronize()
    for f in frames:
        hip.frame_begin(f)
    assert hip.frames_in_flight() == 2
    hip.frame_irradiance_map_device(p, grid, d_sh, vmap, d_maps, out=out)
    got = [hip.frame_end()[0] for _ in frames]
    assert_same_rows(finished(hip, out, 64 * 48, 4).view(np.float32), want, "between the frames")
    for image, frame in zip(got, oracle_frames):
        image = np.asarray(image).reshape(frame.shape)
        assert ((image.view(np.uint32) == frame.view(np.uint32)) | (np.isnan(image) & np.isnan(frame))).all()


def test_refusals(hip, oracle, scenes):
    sc, t, q, p, grid = cornell_volume(hip, oracle, scenes)
    torch.cuda.empty_cache()                                        # (the allocations below are then the device's own, of exactly these sizes)
    good = map_of(4, 3)
    sh, maps = hip.volume_bake_map(grid, t, q, good)
    hip.frame_irradiance_map(p, grid, sh, good, maps)
    before = (hip.last_volume(), hip.last_probes(), hip.last_surface(), hip.last_volume_map())
    n = 300
    d_sh = torch.full((8 * 144,), 0xA5, dtype=torch.uint8, device="cuda")
    d_maps = torch.full((8 * 16 * 16,), 0xA5, dtype=torch.uint8, device="cuda")
    d_radiance = torch.full((8 * 96 * 32,), 0xA5, dtype=torch.uint8, device="cuda")
    planes, out, d_rays, d_positions = poisoned(2 * n, 16), poisoned(n, 16), poisoned(n, 32), poisoned(8, 16)
    short = torch.full((20 << 20,), 0xA5, dtype=torch.uint8, device="cuda")     # 20 MB, an allocation of its own: 1 310 720 rows of 16 bytes
    host = np.zeros((4096, 4), np.float32)
    torch.cuda.synchronize()
    S, M, P, N, O, R, X, D, Q = (d_sh.data_ptr(), d_maps.data_ptr(), planes.data_ptr(), planes.data_ptr() + n * 16, out.data_ptr(), d_rays.data_ptr(), short.data_ptr(),
                                 d_radiance.data_ptr(), d_positions.data_ptr())
    rows_short = (20 << 20) // 16

    def bad_map(size=4, sharpness=3, reserved=(0, 0)):
        return capi.VolumeMap(size, sharpness, reserved)

    reduce_ = lambda vm=good, r=D, m=M, k=8, w=4: hip.probe_map_device(r, k, w, vm, out=m)
    fused = lambda vm=good, o=S, m=M, pos=(Q, 8): hip.probes_sh_map_device(pos, t, q, vm, out=o, maps=m)
    bake = lambda vm=good, o=S, m=M, gr=grid, qq=q: hip.volume_bake_map_device(gr, t, qq, vm, out=o, maps=m)
    lookup = lambda vm=good, m=M, s=S, pp=P, nn=N, o=O, k=n, gr=grid: hip.volume_irradiance_map_device(gr, s, pp, nn, vm, m, k, out=o)
    rays = lambda vm=good, m=M, s=S, r=(R, n), o=O, gr=grid: hip.rays_irradiance_map_device(gr, s, r, vm, m, p.texture_width, out=o)
    frame = lambda vm=good, m=M, s=S, o=X, gr=grid, f=p: hip.frame_irradiance_map_device(f, gr, s, vm, m, out=o)
    device_calls = (("flx_probe_map_device", reduce_), ("flx_probes_sh_map_device", fused), ("flx_volume_bake_map_device", bake), ("flx_volume_irradiance_map_device", lookup),
                    ("flx_rays_irradiance_map_device", rays), ("flx_frame_irradiance_map_device", frame))
    bad_maps = [
        (None, "the map is NULL"),
        (bad_map(size=0), "the map's size is not one of 1 .. 16"),
        (bad_map(size=17), "the map's size is not one of 1 .. 16"),
        (bad_map(size=65536), "the map's size is not one of 1 .. 16"),
        (bad_map(sharpness=9), "the map's sharpness is above 8"),
        (bad_map(reserved=(1, 0)), "a reserved word of the map is not 0"),
        (bad_map(reserved=(0, 1)), "a reserved word of the map is not 0"),
    ]
    refused = []
    for name, call in device_calls:
        refused += [(lambda call=call, vm=vm: call(vm=vm), name + ": " + words) for vm, words in bad_maps]
        refused += [
            (lambda call=call: call(m=0), name + ": the maps array is NULL"),
            (lambda call=call: call(m=host.ctypes.data), name + ": the maps are not n_probes \\* size \\* size rows of 16 bytes in memory of the context's device"),
            (lambda call=call: call(m=M + 4), name + ": the maps are not n_probes \\* size \\* size rows of 16 bytes in memory of the context's device, 16-byte aligned"),
            (lambda call=call: call(m=X + (20 << 20) - 2048 + 16), name + ": the maps are not n_probes \\* size \\* size rows of 16 bytes"),      # one row past the allocation's end
        ]
    refused += [
        # the rows of all maps on either side of 2^31 (the accepted side is then refused for the array, which is too short)
        (lambda: reduce_(k=0x800000, w=1, vm=bad_map(size=16)), "flx_probe_map_device: the maps have 2\\^31 rows or more"),
        (lambda: reduce_(k=0x7fffff, w=1, vm=bad_map(size=16), r=X), "flx_probe_map_device: the radiance is not n_probes \\* 6 \\* face_size \\* face_size rows"),
        (lambda: lookup(gr=capi.VolumeGrid(count=(0x800000, 1, 1)), vm=bad_map(size=16)), "flx_volume_irradiance_map_device: the maps have 2\\^31 rows or more"),
        (lambda: hip.volume_irradiance_map(capi.VolumeGrid(count=(1 << 29, 1, 1)), sh, host[:4], host[:4], bad_map(size=2), maps), "one SH row and size x size map rows per probe"),
        # the maps against every other array of their call
        (lambda: reduce_(m=D + 32), "flx_probe_map_device: the maps overlap another array"),
        (lambda: reduce_(r=M), "flx_probe_map_device: the maps overlap another array"),
        (lambda: fused(m=S), "flx_probes_sh_map_device: the maps overlap another array"),
        (lambda: fused(pos=(M + 16, 8)), "flx_probes_sh_map_device: the maps overlap another array"),
        (lambda: bake(m=S), "flx_volume_bake_map_device: the maps overlap another array"),
        (lambda: bake(o=M + 16), "flx_volume_bake_map_device: the maps overlap another array"),
        (lambda: lookup(s=M), "flx_volume_irradiance_map_device: the maps overlap another array"),
        (lambda: lookup(pp=M, k=4), "flx_volume_irradiance_map_device: the maps overlap another array"),
        (lambda: lookup(nn=M + 2032, k=4), "flx_volume_irradiance_map_device: the maps overlap another array"),
        (lambda: lookup(o=M + 1024, k=4), "flx_volume_irradiance_map_device: the maps overlap another array"),
        (lambda: rays(s=M), "flx_rays_irradiance_map_device: the maps overlap another array"),
        (lambda: rays(r=(M, 4)), "flx_rays_irradiance_map_device: the maps overlap another array"),
        (lambda: rays(r=(R, 4), o=M + 32), "flx_rays_irradiance_map_device: the maps overlap another array"),
        (lambda: frame(s=M), "flx_frame_irradiance_map_device: the maps overlap another array"),
        (lambda: frame(m=X + 64), "flx_frame_irradiance_map_device: the maps overlap another array"),
        # the siblings' own refusals come first, in their words
        (lambda: lookup(gr=None, vm=None), "flx_volume_irradiance_map_device: the grid is NULL"),
        (lambda: lookup(s=0, m=0), "flx_volume_irradiance_map_device: an array is NULL"),
        (lambda: lookup(o=P, m=P), "flx_volume_irradiance_map_device: the arrays overlap"),
        (lambda: bake(qq=None, vm=None), "flx_probes_sh_device: the probe params are NULL"),
        (lambda: bake(o=0, m=0), "flx_volume_bake_map_device: an array is NULL"),
        (lambda: fused(o=0, m=0), "flx_probes_sh_map_device: an array is NULL"),
        (lambda: frame(f=None, vm=None), "flx_frame_surface_device: params is NULL"),
        (lambda: reduce_(w=0, vm=None), "flx_probe_map_device: face_size is not one of 1 .. 256"),
        (lambda: reduce_(k=10923, w=256), "flx_probe_map_device: n_probes \\* 6 \\* face_size \\* face_size is 2\\^32 or more"),
        (lambda: reduce_(r=0), "flx_probe_map_device: an array is NULL"),
        (lambda: reduce_(r=host.ctypes.data), "flx_probe_map_device: the radiance is not n_probes \\* 6 \\* face_size \\* face_size rows in memory of the context's device"),
        # the host variants
        (lambda: hip.probe_map(np.zeros((96, 8), np.float32), 1, 4, bad_map(size=0)), "flx_probe_map: the map's size is not one of 1 .. 16"),
        (lambda: hip.probes_sh_map(np.zeros((2, 4), np.float32), t, q, bad_map(sharpness=200)), "flx_probes_sh_map: the map's sharpness is above 8"),
        (lambda: hip.volume_bake_map(grid, t, q, None), "flx_volume_bake_map: the map is NULL"),
        (lambda: hip.volume_irradiance_map(grid, sh, host[:4], host[:4], bad_map(reserved=(0, 9)), maps), "flx_volume_irradiance_map: a reserved word of the map is not 0"),
        (lambda: hip.rays_irradiance_map(grid, sh, np.zeros((4, 8), np.float32), None, maps), "flx_rays_irradiance_map: the map is NULL"),
        (lambda: hip.frame_irradiance_map(p, grid, sh, bad_map(size=17), np.zeros((8 * 289, 4), np.float32)), "flx_frame_irradiance_map: the map's size is not one of 1 .. 16"),
        (lambda: hip.frame_irradiance_map(p, grid, sh, good, maps[:-1]), "one SH row and size x size map rows per probe"),
    ]
    for call, words in refused:
        with pytest.raises((capi.FlexLightHipError, ValueError), match=r"(failed \(1\): .*(" + words + "))|(" + words + ")"):      # FLX_ERR_INVALID, or the binding's own refusal
            call()
    hip.sync()
    for buffer in (d_sh, d_maps, d_radiance, planes, out, d_rays, d_positions, short):
        assert bool((buffer == 0xA5).all())                        # nothing was written
    assert (hip.last_volume(), hip.last_probes(), hip.last_surface(), hip.last_volume_map()) == before      # ... and nothing enqueued
    # no probes, no points: FLX_OK and nothing enqueued, the map looked at first
    hip.probe_map_device(0, 0, 4, good, out=0)
    hip.volume_irradiance_map_device(grid, 0, 0, 0, good, 0, 0, out=0)
    hip.rays_irradiance_map_device(grid, 0, (0, 0), good, 0, p.texture_width, out=0)
    with pytest.raises(capi.FlexLightHipError, match="flx_volume_irradiance_map_device: the map's sharpness is above 8"):
        hip.volume_irradiance_map_device(grid, 0, 0, 0, bad_map(sharpness=9), 0, 0, out=0)
    with pytest.raises(capi.FlexLightHipError, match="flx_probe_map_device: the map is NULL"):
        hip.probe_map_device(0, 0, 4, None, out=0)
    assert (hip.last_volume(), hip.last_volume_map()) == (before[0], before[3])
    # the calls still work
    assert np.isfinite(hip.frame_irradiance_map(p, grid, sh, good, maps)).all()
