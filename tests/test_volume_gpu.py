"""Probe volumes on the device (include/flexlight_hip_debug.h, "probe volumes"): k_volume_positions' rows and k_volume_irradiance's rows are the CPU reference's bits
(tests/volume_ref, the same include/flx_volume.h) for every grid, count and point set at which the kernel can go wrong; the fused calls are the calls they are made of, bit for bit; a lookup between two frames of the loop leaves them alone; every refusal says its words and
leaves the output as it was."""
import numpy as np
import pytest
import torch

from flexlight_hip import capi
from probe_util import cornell_probes
from volume_util import COUNTS, POINT_SETS, assert_same_words, grid_of, point_set, reference, synthetic_sh

pytestmark = pytest.mark.gpu

SPARE = 8               # rows behind the last one that must keep their poison
NS = (1, 63, 64, 65, 255, 256, 257, 1000)      # a lane; a wave less one, a wave, a wave and a lane; the same of a workgroup; four workgroups, the last one short
SURFACE = capi.SURFACE_POSITION | capi.SURFACE_NORMAL


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return reference(tmp_path_factory)


def poisoned(rows, row_bytes):
    return torch.full(((rows + SPARE) * row_bytes,), 0xA5, dtype=torch.uint8, device="cuda")


def finished(ctx, out, rows, row_words):
    """a poisoned output after the call -> its uint32 [rows, row_words]: nothing past the last row was written"""
    ctx.sync()
    words = out.cpu().numpy().view(np.uint32)
    assert (words[rows * row_words:] == 0xA5A5A5A5).all()
    return words[:rows * row_words].reshape(rows, row_words)


def assert_same_rows(got, want, what):
    """irradiance rows bit for bit; a NaN equals any NaN (its payload is not defined)"""
    got, want = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 4), np.ascontiguousarray(want).view(np.uint32).reshape(-1, 4)
    nan = lambda b: (b & 0x7fffffff) > 0x7f800000
    bad = np.flatnonzero(~((got == want) | (nan(got) & nan(want))).all(axis=1))
    assert got.shape == want.shape and bad.size == 0, "%s: %d of %d rows differ, first %d: got %s want %s" % (
        what, bad.size, len(got), bad[0], ["%08x" % x for x in got[bad[0]]], ["%08x" % x for x in want[bad[0]]])


def device_lookup(ctx, grid, d_sh, positions, normals):
    n = len(positions)
    out = poisoned(n, 16)
    d_positions, d_normals = torch.from_numpy(positions).cuda(), torch.from_numpy(normals).cuda()
    torch.cuda.synchronize()
    assert ctx.volume_irradiance_device(grid, d_sh, d_positions, d_normals, out=out) is out
    return finished(ctx, out, n, 4)


@pytest.mark.parametrize("count", COUNTS)
def test_positions_are_the_references_bits(hip, ref, count):
    grid = grid_of(count)
    want = ref.positions(grid)
    out = poisoned(grid.probes, 16)
    torch.cuda.synchronize()
    assert hip.volume_positions_device(grid, out=out) is out
    assert_same_words(finished(hip, out, grid.probes, 4), want, "%d x %d x %d" % count)
    assert_same_words(hip.volume_positions(grid), want, "the host variant")


def test_positions_across_workgroups_and_without_a_scene(ref):
    grid = capi.VolumeGrid((0.1, -0.2, 0.3), (0.3, 0.7, 1.1), (7, 5, 9))      # 315 probes: two workgroups, the second one short; no spacing is a power of two
    with capi.Context(0) as fresh:
        out = poisoned(grid.probes, 16)
        torch.cuda.synchronize()
        fresh.volume_positions_device(grid, out=out)
        assert_same_words(finished(fresh, out, grid.probes, 4), ref.positions(grid), "315 probes, a context without a scene")


@pytest.mark.parametrize("count", COUNTS)
def test_the_lookup_is_the_references_bits(hip, ref, count):
    """every point set, n, flag and bias.  (The kernel has one path: the uniform path the issue describes measured inside the gather's spread and was deleted,
    profiles/volume.txt, so there is no count of waves by path to hold.)"""
    for visibility in (True, False):
        for bias in (0.0, 0.125):
            grid = grid_of(count, bias, visibility)
            for k, kind in enumerate(POINT_SETS):
                sh = synthetic_sh(grid.probes, k)              # (the seed turns the rows' kinds: the one probe of 1 x 1 x 1 is of every kind in turn)
                d_sh = torch.from_numpy(sh).cuda()
                for n in NS:
                    what = "%s, n = %d, visibility %d, bias %g" % (kind, n, visibility, bias)
                    positions, normals = point_set(grid, kind, n, 1000 * k + n)
                    want = ref.irradiance(grid, sh, positions, normals)
                    assert_same_rows(device_lookup(hip, grid, d_sh, positions, normals), want, what)
                    last = hip.last_volume()
                    assert last == {"n": n, "slabs": 1, "slab": n, "probes": grid.probes, "flags": grid.flags, "source": 0, "groups": (n + 255) // 256}, last
                    if kind == "misses" and n == 257:
                        assert_same_rows(hip.volume_irradiance(grid, sh, positions, normals), want, what + ", the host variant")


def test_a_lookup_needs_no_scene(ref):
    grid = grid_of((3, 2, 4), 0.125)
    sh = synthetic_sh(grid.probes, 3)
    positions, normals = point_set(grid, "misses", 300, 5)
    want = ref.irradiance(grid, sh, positions, normals)
    with capi.Context(0) as fresh:
        assert_same_rows(device_lookup(fresh, grid, torch.from_numpy(sh).cuda(), positions, normals), want, "a context without a scene")
        assert_same_rows(fresh.volume_irradiance(grid, sh, positions, normals), want, "its host variant")
        assert_same_rows(fresh.volume_irradiance(grid, sh, positions[:, :3], normals[:, :3])[positions[:, 3] == 1.0], want[positions[:, 3] == 1.0], "three floats a row")


def cornell_volume(hip, oracle, scenes):
    """-> (scene, trace params, probe params with face size 4, a frame of 64 x 48, a 2 x 2 x 2 grid inside the hull of the frame's first hits)"""
    sc, t, _ = cornell_probes(oracle, scenes)
    hip.update_scene(sc)
    p = sc.frame_params(width=64, height=48, samples=1, max_reflections=3, use_filter=0)
    planes = hip.frame_surface(p, capi.SURFACE_POSITION)[0]
    hit = planes[planes[:, 3] != 0.0][:, :3]
    assert len(hit) > 1000
    lo, hi = hit.min(axis=0), hit.max(axis=0)
    grid = capi.VolumeGrid(lo + 0.2 * (hi - lo), 0.6 * (hi - lo), (2, 2, 2), normal_bias=0.01 * float((hi - lo).max()))
    return sc, t, capi.ProbeParams(face_size=4, sky=(0.5, 0.25, 0.125)), p, grid


def test_bake_is_positions_then_probes(hip, oracle, scenes, ref):
    sc, t, q, p, grid = cornell_volume(hip, oracle, scenes)
    d_positions = hip.volume_positions_device(grid)
    want = hip.probes_sh_device(d_positions, t, q)
    hip.sync()
    assert_same_words(d_positions.cpu().numpy(), ref.positions(grid), "the grid's positions")
    want = want.cpu().numpy()
    assert np.isfinite(want).all() and (want[:, 7] > 0).all()
    out = poisoned(8, 144)
    torch.cuda.synchronize()
    assert hip.volume_bake_device(grid, t, q, out=out) is out
    assert_same_words(finished(hip, out, 8, 36), want, "the bake")
    assert hip.last_probes()["n"] == 8 and hip.last_probes()["face_size"] == 4
    assert_same_words(hip.volume_bake(grid, t, q), want, "the host variant")


def test_frame_and_rays_are_surface_then_lookup(hip, oracle, scenes, ref):
    sc, t, q, p, grid = cornell_volume(hip, oracle, scenes)
    d_sh = hip.volume_bake_device(grid, t, q)
    # a frame
    planes = hip.frame_surface_device(p, SURFACE)
    want = hip.volume_irradiance_device(grid, d_sh, planes[0], planes[1])
    hip.sync()
    sh, want, host_planes = d_sh.cpu().numpy(), want.cpu().numpy(), planes.cpu().numpy()
    hit = host_planes[0][:, 3] != 0.0
    assert hit.sum() > 1000 and np.isfinite(want).all() and (want[hit][:, 3] > 0).all() and (want[~hit] == 0).all()
    assert_same_rows(want, ref.irradiance(grid, sh, host_planes[0], host_planes[1]), "the chain against the reference")
    n = 64 * 48
    out = poisoned(n, 16)
    torch.cuda.synchronize()
    assert hip.frame_irradiance_device(p, grid, d_sh, out=out) is out
    assert_same_rows(finished(hip, out, n, 4), want, "the frame call")
    assert hip.last_volume() == {"n": n, "slabs": 1, "slab": n, "probes": 8, "flags": 1, "source": 2, "groups": 12}
    assert hip.last_surface()["frame"] == 1 and hip.last_surface()["fields"] == SURFACE
    assert hip.frame_irradiance_device(p, grid, d_sh).shape == (48, 64, 4)
    assert_same_rows(hip.frame_irradiance(p, grid, sh).reshape(-1, 4), want, "the frame call's host variant")
    # 300 rays: pixels of the frame, strided, their directions scaled and some turned away
    from rays_trace_util import camera_rays
    rays = camera_rays(oracle, scenes, "cornell")[2]
    rays = np.ascontiguousarray(rays[np.linspace(0, len(rays) - 1, 300).astype(int)], np.float32)
    rays[::11, 4:7] *= -1.0
    d_rays = torch.from_numpy(rays).cuda()
    torch.cuda.synchronize()
    planes = hip.surface_rays_device(d_rays, SURFACE, p.texture_width)
    want = hip.volume_irradiance_device(grid, d_sh, planes[0], planes[1])
    hip.sync()
    want = want.cpu().numpy()
    assert (want[:, 3] > 0).sum() > 100
    for slab, slabs in ((0, 1), (64, 5), (100, 3)):          # flx_debug_set_trace_slab: 300 rays in 5 slabs (the last of 44) and in 3 of 100
        hip.set_trace_slab(slab)
        try:
            out = poisoned(300, 16)
            torch.cuda.synchronize()
            assert hip.rays_irradiance_device(grid, d_sh, d_rays, p.texture_width, out=out) is out
            assert_same_rows(finished(hip, out, 300, 4), want, "the rays call, slab %d" % slab)
            last = hip.last_volume()
            assert last == {"n": 300, "slabs": slabs, "slab": slab or 1 << 21, "probes": 8, "flags": 1, "source": 1, "groups": 2 if slab == 0 else 1}, last
            if slab == 100:
                assert_same_rows(hip.rays_irradiance(grid, sh, rays, p.texture_width), want, "the rays call's host variant in slabs")
        finally:
            hip.set_trace_slab(0)
    assert_same_rows(hip.rays_irradiance(grid, sh, rays, p.texture_width), want, "the rays call's host variant")


def test_a_lookup_between_two_frames_of_the_loop(hip, oracle, scenes):
    sc, t, q, p, grid = cornell_volume(hip, oracle, scenes)
    sh = hip.volume_bake(grid, t, q)
    want = hip.frame_irradiance(p, grid, sh).reshape(-1, 4)
    frames = [sc.frame_params(width=48, height=36, samples=2, max_reflections=3, use_filter=0) for _ in range(2)]
    frames[1].random_seed = frames[0].random_seed + 1.0
    oracle_frames = [oracle.render(sc, f)[0] for f in frames]
    d_sh = torch.from_numpy(sh).cuda()
    out = poisoned(64 * 48, 16)
    torch.cuda.synchronize()
    for f in frames:
        hip.frame_begin(f)
    assert hip.frames_in_flight() == 2
    hip.frame_irradiance_device(p, grid, d_sh, out=out)
    got = [hip.frame_end()[0] for _ in frames]
    assert_same_rows(finished(hip, out, 64 * 48, 4), want, "between the frames")
    for image, frame in zip(got, oracle_frames):
        image = np.asarray(image).reshape(frame.shape)
        assert ((image.view(np.uint32) == frame.view(np.uint32)) | (np.isnan(image) & np.isnan(frame))).all()
    assert not np.array_equal(got[0], got[1])


def test_refusals(hip, oracle, scenes):
    sc, t, q, p, grid = cornell_volume(hip, oracle, scenes)
    torch.cuda.empty_cache()                                        # (the allocations below are then the device's own, of exactly these sizes)
    sh = hip.volume_bake(grid, t, q)
    hip.frame_irradiance(p, grid, sh)
    before, probes_before, surface_before = hip.last_volume(), hip.last_probes(), hip.last_surface()
    n = 300
    d_sh = torch.full((8 * 144,), 0xA5, dtype=torch.uint8, device="cuda")
    planes, out, d_rays = poisoned(2 * n, 16), poisoned(n, 16), poisoned(n, 32)
    host = np.zeros((4096, 4), np.float32)
    short = torch.full((20 << 20,), 0xA5, dtype=torch.uint8, device="cuda")     # 20 MB, an allocation of its own: 1 310 720 rows of 16 bytes, 145 635 SH rows and 80 bytes
    torch.cuda.synchronize()
    S, P, N, O, R, X = d_sh.data_ptr(), planes.data_ptr(), planes.data_ptr() + n * 16, out.data_ptr(), d_rays.data_ptr(), short.data_ptr()
    rows_short = (20 << 20) // 16

    def g(**kw):
        made = capi.VolumeGrid(tuple(grid.origin), tuple(grid.spacing), tuple(grid.count), grid.normal_bias, grid.floor, grid.flags)
        for k, v in kw.items():
            if k in ("origin", "spacing", "count"):
                for a in range(3):
                    getattr(made, k)[a] = v[a]
            else:
                setattr(made, k, v)
        return made

    def frame_with(**kw):
        f = sc.frame_params(width=64, height=48, samples=1, max_reflections=3, use_filter=0)
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    nan, inf = float("nan"), float("inf")
    lookup = lambda gr=grid, s=S, pp=P, nn=N, m=n, o=O: hip.volume_irradiance_device(gr, s, pp, nn, m, out=o)
    positions = lambda gr=grid, o=P: hip.volume_positions_device(gr, out=o)
    bake = lambda gr=grid, tt=t, qq=q, o=S: hip.volume_bake_device(gr, tt, qq, out=o)
    rays = lambda gr=grid, s=S, r=(R, n), o=O, tw=p.texture_width: hip.rays_irradiance_device(gr, s, r, tw, out=o)
    frame = lambda f=p, gr=grid, s=S, o=X: hip.frame_irradiance_device(f, gr, s, out=o)
    grids = [
        (None, "the grid is NULL"),
        (g(count=(0, 2, 2)), "a count of the grid is 0"),
        (g(count=(2, 2, 0)), "a count of the grid is 0"),
        (g(count=(2048, 1024, 1024)), "the grid has 2\\^31 probes or more"),
        (g(count=(65536, 65536, 1)), "the grid has 2\\^31 probes or more"),
        (g(count=(641, 6700417, 1)), "the grid has 2\\^31 probes or more"),
        (g(origin=(0.0, nan, 0.0)), "origin or spacing holds a value that is not finite"),
        (g(spacing=(1.0, 1.0, inf)), "origin or spacing holds a value that is not finite"),
        (g(spacing=(1.0, 0.0, 1.0)), "a spacing is not greater than 0"),
        (g(spacing=(-1.0, 1.0, 1.0)), "a spacing is not greater than 0"),
        (g(normal_bias=-0.5), "normal_bias is negative or not finite"),
        (g(normal_bias=nan), "normal_bias is negative or not finite"),
        (g(floor=1.5), "floor is not one of 0 .. 1"),
        (g(floor=-0.5), "floor is not one of 0 .. 1"),
        (g(floor=nan), "floor is not one of 0 .. 1"),
        (g(flags=2), "flags has a bit beyond FLX_VOLUME_VISIBILITY"),
        (g(reserved=1), "reserved is not 0"),
    ]
    refused = []
    for bad, words in grids:
        refused += [(lambda bad=bad: lookup(gr=bad), "flx_volume_irradiance_device: " + words), (lambda bad=bad: positions(gr=bad), "flx_volume_positions_device: " + words),
                    (lambda bad=bad: bake(gr=bad), "flx_volume_bake_device: " + words), (lambda bad=bad: rays(gr=bad), "flx_rays_irradiance_device: " + words),
                    (lambda bad=bad: frame(gr=bad), "flx_frame_irradiance_device: " + words)]
    refused += [
        (lambda: hip.volume_positions(g(count=(0, 1, 1))), "flx_volume_positions: a count of the grid is 0"),
        (lambda: hip.volume_bake(g(flags=4), t, q), "flx_volume_bake: flags has a bit beyond FLX_VOLUME_VISIBILITY"),
        (lambda: hip.volume_irradiance(g(floor=2.0), sh, host[:4], host[:4]), "flx_volume_irradiance: floor is not one of 0 .. 1"),
        (lambda: hip.rays_irradiance(g(reserved=7), sh, np.zeros((4, 8), np.float32)), "flx_rays_irradiance: reserved is not 0"),
        (lambda: hip.frame_irradiance(p, g(normal_bias=-1.0), sh), "flx_frame_irradiance: normal_bias is negative or not finite"),
        # the arrays of the lookup
        (lambda: lookup(s=0), "flx_volume_irradiance_device: an array is NULL"),
        (lambda: lookup(pp=0), "flx_volume_irradiance_device: an array is NULL"),
        (lambda: lookup(nn=0), "flx_volume_irradiance_device: an array is NULL"),
        (lambda: lookup(o=0), "flx_volume_irradiance_device: an array is NULL"),
        (lambda: lookup(s=sh.ctypes.data), "the SH rows are not nx \\* ny \\* nz rows of 144 bytes in memory of the context's device"),      # host memory
        (lambda: lookup(s=S + 4), "the SH rows are not nx \\* ny \\* nz rows of 144 bytes in memory of the context's device, 16-byte aligned"),
        (lambda: lookup(gr=g(count=(145636, 1, 1)), s=X), "the SH rows are not nx \\* ny \\* nz rows of 144 bytes"),      # the allocation is one row too short
        (lambda: lookup(pp=host.ctypes.data), "the positions are not n rows of 16 bytes in memory of the context's device"),
        (lambda: lookup(pp=P + 8), "the positions are not n rows of 16 bytes in memory of the context's device, 16-byte aligned"),
        (lambda: lookup(pp=X, m=rows_short + 1), "the positions are not n rows of 16 bytes"),                                   # one row too short
        (lambda: lookup(nn=host.ctypes.data), "the normals are not n rows of 16 bytes in memory of the context's device"),
        (lambda: lookup(pp=X, nn=X + 16, m=rows_short), "the normals are not n rows of 16 bytes"),                              # one row too short (the positions before it fit)
        (lambda: lookup(o=host.ctypes.data), "the irradiance rows are not n rows of 16 bytes in memory of the context's device"),
        (lambda: lookup(o=O + 4), "the irradiance rows are not n rows of 16 bytes in memory of the context's device, 16-byte aligned"),
        (lambda: lookup(pp=X, nn=X, o=X + 16, m=rows_short), "the irradiance rows are not n rows of 16 bytes"),
        (lambda: lookup(o=P), "flx_volume_irradiance_device: the arrays overlap"),
        (lambda: lookup(o=N + 16, m=4), "flx_volume_irradiance_device: the arrays overlap"),
        (lambda: lookup(nn=P + 16), "flx_volume_irradiance_device: the arrays overlap"),
        (lambda: lookup(o=S + 16 * 71, m=1), "flx_volume_irradiance_device: the arrays overlap"),
        (lambda: hip.volume_irradiance(grid, sh[:7], host[:4], host[:4]), "one SH row per probe"),
        # ... of the others
        (lambda: positions(o=0), "flx_volume_positions_device: an array is NULL"),
        (lambda: positions(o=host.ctypes.data), "the positions are not nx \\* ny \\* nz rows of 16 bytes in memory of the context's device"),
        (lambda: positions(gr=g(count=(rows_short + 1, 1, 1)), o=X), "the positions are not nx \\* ny \\* nz rows of 16 bytes"),
        (lambda: bake(o=0), "flx_volume_bake_device: an array is NULL"),
        (lambda: bake(o=S + 8), "the SH rows are not nx \\* ny \\* nz rows of 144 bytes in memory of the context's device, 16-byte aligned"),
        (lambda: bake(gr=g(count=(145636, 1, 1)), o=X), "the SH rows are not nx \\* ny \\* nz rows of 144 bytes"),
        (lambda: rays(s=0), "flx_rays_irradiance_device: an array is NULL"),
        (lambda: rays(r=(0, n)), "flx_rays_irradiance_device: an array is NULL"),
        (lambda: rays(o=0), "flx_rays_irradiance_device: an array is NULL"),
        (lambda: rays(r=(host.ctypes.data, 4)), "the rays are not n rows of 32 bytes in memory of the context's device"),
        (lambda: rays(r=(X, rows_short // 2 + 1)), "the rays are not n rows of 32 bytes"),
        (lambda: rays(o=O + 8), "the irradiance rows are not n rows of 16 bytes in memory of the context's device, 16-byte aligned"),
        (lambda: rays(o=R + 32), "flx_rays_irradiance_device: the arrays overlap"),
        (lambda: frame(s=0), "flx_frame_irradiance_device: an array is NULL"),
        (lambda: frame(o=0), "flx_frame_irradiance_device: an array is NULL"),
        (lambda: frame(o=host.ctypes.data), "the irradiance rows are not width \\* height rows of 16 bytes in memory of the context's device"),
        (lambda: frame(f=frame_with(width=1024, height=1281)), "the irradiance rows are not width \\* height rows of 16 bytes"),      # 1 311 744 rows
        (lambda: frame(s=X, o=X + 144), "flx_frame_irradiance_device: the arrays overlap"),
        # the parts' own refusals, in their own words
        (lambda: bake(tt=None), "flx_rays_trace_ordered: params is NULL"),
        (lambda: bake(qq=None), "flx_probes_sh_device: the probe params are NULL"),
        (lambda: bake(qq=capi.ProbeParams(face_size=0)), "flx_probes_sh_device: face_size is not one of 1 .. 256"),
        (lambda: hip.volume_bake(grid, t, capi.ProbeParams(face_size=4, order=2)), "flx_probes_sh_device: order has a bit beyond FLX_TRACE_ORDER_HITS"),
        (lambda: rays(tw=0), "flx_rays_surface_device: texture_width is less than 1"),
        (lambda: hip.rays_irradiance(grid, sh, np.zeros((4, 8), np.float32), 0), "flx_rays_surface_device: texture_width is less than 1"),
        (lambda: frame(f=None), "flx_frame_surface_device: params is NULL"),
        (lambda: frame(f=frame_with(width=0)), "flx_frame_surface_device: width or height is 0"),
        (lambda: frame(f=frame_with(texture_width=0)), "flx_frame_surface_device: texture_width is less than 1"),
        (lambda: frame(f=frame_with(tile_rows=8, tile_index=0, tile_count=2)), "the tile policy does not name the whole frame"),
        (lambda: hip.frame_irradiance(frame_with(height=0), grid, sh), "flx_frame_surface_device: width or height is 0"),
    ]
    for call, words in refused:
        with pytest.raises((capi.FlexLightHipError, ValueError), match=r"(failed \(1\): .*(" + words + "))|(" + words + ")"):      # FLX_ERR_INVALID, or the binding's own refusal
            call()
    hip.sync()
    for buffer in (d_sh, planes, out, d_rays, short):
        assert bool((buffer == 0xA5).all())                        # nothing was written
    assert (hip.last_volume(), hip.last_probes(), hip.last_surface()) == (before, probes_before, surface_before)      # ... and nothing enqueued
    # no points: FLX_OK and nothing enqueued, the grid looked at first
    hip.volume_irradiance_device(grid, 0, 0, 0, 0, out=0)
    hip.rays_irradiance_device(grid, 0, (0, 0), p.texture_width, out=0)
    with pytest.raises(capi.FlexLightHipError, match="flx_volume_irradiance_device: a count of the grid is 0"):
        hip.volume_irradiance_device(g(count=(1, 0, 1)), 0, 0, 0, 0, out=0)
    assert hip.last_volume() == before
    with capi.Context(0) as fresh:                                 # the calls that cast or trace need a scene, in their parts' words
        for call, words in ((lambda: fresh.volume_bake(grid, t, q), "flx_rays_trace_ordered: no scene"), (lambda: fresh.rays_irradiance(grid, sh, np.zeros((4, 8), np.float32)), "flx_rays_surface_device: no scene"),
                            (lambda: fresh.frame_irradiance(p, grid, sh), "flx_frame_surface_device: no scene")):
            with pytest.raises(capi.FlexLightHipError, match=r"failed \(3\): " + words):      # FLX_ERR_NO_SCENE
                call()
    # the calls still work
    assert np.isfinite(hip.frame_irradiance(p, grid, sh)).all()
