"""The ray-batch calls run through each other on ONE context (cast, trace, surface rows of rays and of a frame, planes, image, temporal images: the host path they
share is csrc/flx_query.hip's and csrc/flx_rays_host.h's — the producer wait, the growth of the scratch and of the staging, the slab loop, the host-memory wrapper)
against each of them run alone on a second context: every output bit for bit, compared as uint32 so that a NaN compares, no tolerance.  The first context runs the
device calls back to back with nothing waited for in between, so the scratch grows under work in flight: 2 rays first, then 130 rays in slabs of 64, 64 and 2; a
frame's rows (n, not two per ray) in between.  Both contexts are made here and not the suite's shared one, whose scratch other tests have grown already.  Every
device output goes into a buffer poisoned with 0xA5 with rows to spare behind it.  130 rays at 2 samples, images of 13 x 10, a frame of 16 x 16."""
import numpy as np
import pytest
import torch

from flexlight_hip import capi
from rays_trace_util import camera_rays, free_rays, trace_params

pytestmark = pytest.mark.gpu

SPARE = 8          # rows behind an output that must keep their poison
N, SLAB, W, H = 130, 64, 13, 10
SCENE = "dragon"   # three transforms: the rays are pre-transformed; surfaces of glass and metal


def poisoned(rows, row_bytes):
    return torch.full(((rows + SPARE) * row_bytes,), 0xA5, dtype=torch.uint8, device="cuda")


def words_of(buffer, rows, row_bytes, what):
    """a poisoned device buffer -> its first `rows` rows as uint32; the rows behind them kept their poison"""
    words = buffer.cpu().numpy().view(np.uint32)
    used = rows * row_bytes // 4
    assert (words[used:] == 0xA5A5A5A5).all(), what + ": rows behind the output were written"
    return words[:used].copy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1)


def device_calls(ctx, source, t, frame, alone):
    """the eight device steps -> {step: uint32 words}.  alone: every call on its own, waited for; else back to back, the surface rows' and the canvas image's rays
    written on a side stream immediately before the call that names that stream (after calls that named none)"""
    outs = {"cast 2": poisoned(2, 32), "trace": poisoned(N, 32), "surface": poisoned(8 * N, 16), "frame surface": poisoned(8 * 256, 16), "planes8": poisoned(5 * N, 4),
            "planes32": poisoned(5 * N, 16), "image": poisoned(N, 16), "temporal chain": poisoned(N, 16), "temporal canvas": poisoned(N, 16), "cast": poisoned(N, 32)}
    rows = {"cast 2": (2, 32), "trace": (N, 32), "surface": (8 * N, 16), "frame surface": (8 * 256, 16), "planes8": (5 * N, 4), "planes32": (5 * N, 16), "image": (N, 16),
            "temporal chain": (N, 16), "temporal canvas": (N, 16), "cast": (N, 32)}
    d = source.clone()
    late = [torch.zeros_like(source), torch.zeros_like(source)]      # rays that are there only when the side stream has written them
    busy = torch.ones((1024, 1024), device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()

    def produced(k):
        nonlocal busy
        if alone:
            return d, None
        with torch.cuda.stream(side):
            for _ in range(4):
                busy = busy @ busy * 1e-3                         # work in front of the write, so that the rays are not there when the call returns
            late[k].copy_(source)
        return late[k], side

    wait = ctx.sync if alone else (lambda: None)
    ctx.cast_rays_device(d[:2], outs["cast 2"]); wait()                                                          # 1. the scratch starts small
    ctx.trace_rays_device(d, t, outs["trace"]); wait()                                                           # 2. hits, slots and last grow
    rays, stream = produced(0)
    ctx.surface_rays_device(rays, capi.SURFACE_ALL, t.texture_width, outs["surface"], stream); wait()            # 3. the producer wait, after calls without one
    ctx.frame_surface_device(frame, capi.SURFACE_ALL, outs["frame surface"]); wait()                             # 4. the scratch: n rows, more than two per ray of a slab
    ctx.ray_planes_device(d, t, outs["planes8"], outs["planes32"]); wait()                                       # 5.
    ctx.ray_image_device(d, W, H, t, hdr=1, out=outs["image"]); wait()                                           # 6.
    ctx.rays_image_temporal(d, W, H, t, capi.RayTemporal(history=0, use_filter=1), device=True, out=outs["temporal chain"]); wait()      # 7.
    rays, stream = produced(1)
    ctx.rays_image_temporal(rays, W, H, t, capi.RayTemporal(history=1, use_filter=0), device=True, out=outs["temporal canvas"], stream=stream); wait()
    ctx.cast_rays_device(d, outs["cast"]); wait()                                                                # 8.
    ctx.sync()
    side.synchronize()
    assert torch.equal(d, source) and (alone or (torch.equal(late[0], source) and torch.equal(late[1], source)))      # the rays are read only
    return {step: words_of(outs[step], *rows[step], step) for step in outs}


def host_calls(ctx, rays, t, frame):
    """the host-memory twin of every device step -> {step: uint32 words}; the temporal images on histories no call has used"""
    p8, p32 = ctx.ray_planes(rays, t, floats=True)
    return {"cast 2": bits(ctx.cast_rays(rays[:2])), "trace": bits(ctx.trace_rays(rays, t)), "surface": bits(ctx.surface_rays(rays, capi.SURFACE_ALL, t.texture_width)),
            "frame surface": bits(ctx.frame_surface(frame, capi.SURFACE_ALL)), "planes8": bits(p8), "planes32": bits(p32), "image": bits(ctx.ray_image(rays, W, H, t, hdr=1)),
            "temporal chain": bits(ctx.rays_image_temporal(rays, W, H, t, capi.RayTemporal(history=2, use_filter=1))),
            "temporal canvas": bits(ctx.rays_image_temporal(rays, W, H, t, capi.RayTemporal(history=3, use_filter=0))), "cast": bits(ctx.cast_rays(rays))}


def records(ctx):
    return (ctx.last_query(), ctx.last_trace(), ctx.last_surface(), ctx.last_ray_planes(), ctx.debug_last_ray_temporal())


def test_the_calls_through_each_other_equal_each_call_alone(oracle, scenes):
    sc, p, _, _, _ = camera_rays(oracle, scenes, SCENE)
    rays = np.ascontiguousarray(free_rays(oracle, scenes, SCENE)[1015:1015 + N])      # 65 rays that leave surfaces, 65 from free space
    t = trace_params(p)
    frame = sc.frame_params(width=16, height=16, samples=1, max_reflections=1, use_filter=0)
    assert t.samples == 2 and rays.shape == (N, 8) and W * H == N
    source = torch.from_numpy(rays).cuda()
    got = {}
    for alone in (False, True):
        with capi.Context(0) as ctx:
            ctx.update_scene(sc)
            ctx.set_trace_slab(SLAB)
            device = device_calls(ctx, source, t, frame, alone)
            after = records(ctx)
            host = host_calls(ctx, rays, t, frame)
            got[alone] = (device, after)
            for step in device:
                assert np.array_equal(host[step], device[step]), "%s, %s: the host call differs from the device call" % ("alone" if alone else "through each other", step)
    (mixed, mixed_records), (single, single_records) = got[False], got[True]
    hit = mixed["cast"].reshape(N, 8)[:, 3].view(np.int32) != -1
    assert 0.3 < hit.mean() < 0.95                                                   # hits and misses both
    for step in mixed:
        assert np.array_equal(mixed[step], single[step]), "%s: through the other calls it differs from the call alone" % step
    assert np.array_equal(mixed["cast 2"], mixed["cast"][:16])
    # what ran: slabs of 64, 64 and 2 for every batch of rays, the frame's rows in one piece; the same on both contexts
    assert mixed_records == single_records
    query, trace, surface, planes, temporal = mixed_records
    assert (query["n"], query["what"]) == (N, capi.RAYS_CLOSEST | capi.RAYS_OCCLUDED)
    assert (trace["slabs"], trace["slab"], trace["n"], trace["samples"]) == (3, SLAB, N, 2)
    assert (surface["slabs"], surface["n"], surface["frame"]) == (1, 256, 1)
    assert (planes["slabs"], planes["slab"], planes["n"], planes["samples"]) == (3, SLAB, N, 2)
    assert (temporal["slabs"], temporal["slab"], temporal["n"], temporal["history"], temporal["depth"], temporal["fused"]) == (3, SLAB, N, 1, 4, 1)
