"""Traced ray batches on the GPU (flx_rays_trace, flx_rays_trace_device: csrc/flx_rays_trace.hip) against the CPU reference (tests/rays_trace_ref, which calls the
oracle's own rayTracer and lightTrace): every word of every row, a NaN equal to a NaN.  On a camera's rays the rows' words 0..3 also equal flx_render's own frame
wherever the frame's hit rule and rayTracer agree (rays_trace_util.camera_rays)."""
import numpy as np
import pytest
import torch

from flexlight_hip import capi
from rays_trace_util import FRAMES, assert_rows, camera_rays, free_rays, reference, trace_params, words_of
from scene_update_util import reflatten_by_rule, with_geometry

pytestmark = pytest.mark.gpu

MISS = np.array([0, 0, 0, 0, 0, 0xffffffff, 0, 0], np.uint32)


@pytest.fixture(scope="module")
def ref(tmp_path_factory, oracle):
    return reference(tmp_path_factory)


_want = {}


def wanted(ref, key, sc, t, rays):
    """the reference's rows, computed once per key"""
    if key not in _want:
        _want[key] = ref.trace(sc, t, rays)
    return _want[key]


def traced(hip, rays, t, n=None):
    """rays (numpy [n, 8]) through trace_rays_device into a poisoned buffer with eight rows behind the last -> words [n, 8]; nothing else is written"""
    d = torch.from_numpy(np.ascontiguousarray(rays[:n] if n is not None else rays)).cuda()
    keep = d.clone()
    n = d.shape[0]
    out = torch.full((n + 8, 32), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert hip.trace_rays_device(d, t, out) is out
    hip.sync()
    got = words_of(out)
    assert (got[n:] == 0xA5A5A5A5).all() and torch.equal(d, keep)              # nothing beyond row n - 1 is written; the rays are read only
    return got[:n]


# ---- a camera's rays: the reference's rows and the library's own frame ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(FRAMES))
def test_a_cameras_rays_equal_the_reference_and_the_frame(hip, oracle, scenes, ref, name):
    sc, p, rays, compares, _ = camera_rays(oracle, scenes, name)
    assert compares.sum() >= FRAMES[name][4]
    t = trace_params(p)
    hip.update_scene(sc)
    got = traced(hip, rays, t)
    assert_rows(got, wanted(ref, ("camera", name), sc, t, rays), name)
    frame = hip.render(p)[0].reshape(-1, 4).view(np.uint32)
    differ = np.flatnonzero((got[:, 0:4] != frame).any(axis=1) & compares)
    assert differ.size == 0, (name, differ[:8])
    host = words_of(hip.trace_rays(rays, t))                                     # the host call: the same rows
    assert np.array_equal(host, got)
    assert np.array_equal(capi.unpack_radiance(hip.trace_rays(rays[:5], t))["entry"], got[:5, 5].view(np.int32))
    info = hip.last_trace()
    assert (info["slabs"], info["n"], info["samples"], info["chunk"]) == (1, 5, p.samples, 256)


# ---- rays that no camera makes -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dragon", "theater"])
def test_free_rays_equal_the_reference(hip, oracle, scenes, ref, name):
    """dragon: three transforms, glass and metals, the lane walk; theater: atlases, 9 lights, the lockstep walk"""
    sc, p, _, _, _ = camera_rays(oracle, scenes, name)
    rays, t = free_rays(oracle, scenes, name), trace_params(p)
    want = wanted(ref, ("free", name, p.samples), sc, t, rays)
    hit = want[:, 5].view(np.int32) != -1
    assert rays.shape[0] == 2160 and hit.mean() >= 0.30 and (~hit).mean() >= 0.05 and (want[:, 7] > p.samples).mean() >= 0.10      # the conditions on the inputs
    assert (want[~hit] == MISS).all()
    hip.update_scene(sc)
    assert_rows(traced(hip, rays, t), want, name)
    assert hip.last_trace()["lockstep"] == int(name == "theater")               # both kernels run across the two scenes


# ---- shapes where the refill can go wrong -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dragon", "theater"])
def test_sizes_samples_groups_and_slabs(hip, oracle, scenes, ref, name):
    sc, p, _, _, _ = camera_rays(oracle, scenes, name)
    rays = free_rays(oracle, scenes, name)[900:1260]                              # rays from surfaces and rays from free space
    hip.update_scene(sc)
    try:
        for samples in (1, 3):
            t = trace_params(p)
            t.samples = samples
            want = wanted(ref, ("shapes", name, samples), sc, t, rays)
            assert 0.2 < (want[:257, 5].view(np.int32) != -1).mean() < 0.95
            for groups in (0, 1):                                                 # one workgroup: every lane takes item after item
                hip.set_query_groups(groups)
                for n in (1, 63, 64, 65, 257):
                    assert_rows(traced(hip, rays, t, n), want[:n], "%s S %d groups %d n %d" % (name, samples, groups, n))
                    info = hip.last_trace()
                    assert (info["slabs"], info["n"], info["samples"]) == (1, n, samples)
                    units = -(-n // 64) * samples                                # (block of 64 rays, sample) pairs; four of them fill a workgroup
                    assert info["path_groups"] == (groups or min(-(-units // 4), hip.device_info()[1] * 8)) and info["query_groups"] == 1
            # a slab ceiling forced small: three slabs and more, a ragged last one, slabs that are no whole blocks of 64 rays, under both workgroup settings
            for groups, slab, n in ((0, 100, 257), (1, 100, 257), (0, 64, 360), (1, 1, 5), (0, 129, 360)):
                hip.set_query_groups(groups)
                hip.set_trace_slab(slab)
                assert_rows(traced(hip, rays, t, n), want[:n], "%s S %d groups %d slab %d n %d" % (name, samples, groups, slab, n))
                info = hip.last_trace()
                assert info["slabs"] == -(-n // slab) >= 3 and (slab == 1 or n % slab != 0) and info["slab"] == slab      # (a ragged last slab wherever a slab has more than one ray)
                hip.set_trace_slab(0)
    finally:
        hip.set_query_groups(0)
        hip.set_trace_slab(0)


# ---- the loop guard --------------------------------------------------------------------------------------------------------------------------------------------------

def test_loop_guard_cases(hip, oracle, scenes, ref):
    sc, p, rays, _, first = camera_rays(oracle, scenes, "dragon")
    hit = first[:, 4] != -1
    ambient = np.array(p.ambient[:], np.float32).view(np.uint32)
    hip.update_scene(sc)
    for key, value in (("max_reflections", 0), ("min_importancy", 2.0), ("max_reflections", 1)):
        t = trace_params(p)
        setattr(t, key, value)
        want = wanted(ref, ("guard", key, value), sc, t, rays)
        got = traced(hip, rays, t)
        assert_rows(got, want, "%s = %s" % (key, value))
        if (key, value) != ("max_reflections", 1):
            assert hit.sum() > 1000 and (got[hit, 0:3] == ambient).all() and (got[hit, 7] == 0).all() and (got[hit, 3].view(np.float32) == 1.0).all()      # rgb = ambient, nothing shaded
        else:
            assert (got[hit, 7] == p.samples).all()


# ---- order ---------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_batch_sees_the_lights_uploaded_before_it(hip, oracle, scenes, ref):
    import copy
    sc, p, _, _, _ = camera_rays(oracle, scenes, "theater")
    rays, t = free_rays(oracle, scenes, "theater")[:512], trace_params(p)
    lights = sc.arrays["lights"].reshape(-1, 6).copy()[::2]
    lights[:, 0:3] += np.float32(3.0)
    lights[:, 3] *= np.float32(0.5)
    other = copy.copy(sc)
    other.arrays = dict(sc.arrays, lights=np.ascontiguousarray(lights.reshape(-1)))
    before, after = wanted(ref, ("free512", "theater"), sc, t, rays), ref.trace(other, t, rays)
    assert (before != after).any(axis=1).mean() > 0.2
    hip.update_scene(sc)
    assert_rows(traced(hip, rays, t), before, "the scene's lights")
    hip.update_primary_light_sources(lights)
    assert_rows(traced(hip, rays, t), after, "other lights")


def test_a_batch_sees_the_rows_updated_before_it(hip, oracle, scenes, ref):
    sc, p, rays, _, first = camera_rays(oracle, scenes, "cornell")
    t = trace_params(p)
    entry = int(first[len(first) // 2 + 16, 4])                                 # the triangle the centre pixel sees
    assert entry >= 0
    g = sc.arrays["geometry"].reshape(-1, 12).copy()
    assert g[entry, 10] == 2
    g[entry, [1, 4, 7]] += np.float32(500.0)                                      # the triangle leaves, out of every ray's way
    moved = with_geometry(sc, reflatten_by_rule(g))
    before, after = wanted(ref, ("camera", "cornell"), sc, t, rays), ref.trace(moved, t, rays)
    assert (before[:, 5] == entry).sum() > 10 and (after[:, 5] != entry).all() and (before != after).any(axis=1).sum() > 10
    hip.update_scene(sc)
    assert_rows(traced(hip, rays, t), before, "as uploaded")
    hip.update_scene_rows(entry, g[entry:entry + 1])
    assert_rows(traced(hip, rays, t), after, "after flx_scene_update")


def test_a_batch_between_two_frames_of_the_loop(hip, oracle, scenes, ref):
    sc, p, _, _, _ = camera_rays(oracle, scenes, "dragon")
    rays, t = free_rays(oracle, scenes, "dragon"), trace_params(p)
    want = wanted(ref, ("free", "dragon", p.samples), sc, t, rays)
    hip.update_scene(sc)
    params = [sc.frame_params(width=96, height=54, samples=2, max_reflections=4, use_filter=0) for _ in range(2)]
    params[1].random_seed = params[0].random_seed + 1.0
    oracle_frames = [oracle.render(sc, q)[0] for q in params]
    d = torch.from_numpy(rays).cuda()
    torch.cuda.synchronize()
    for q in params:
        hip.frame_begin(q)
    assert hip.frames_in_flight() == 2
    out = hip.trace_rays_device(d, t)
    frames = [hip.frame_end()[0] for _ in params]
    hip.sync()
    assert_rows(words_of(out), want, "between two frames")
    for got, frame in zip(frames, oracle_frames):
        got = np.asarray(got).reshape(frame.shape)
        assert ((got.view(np.uint32) == frame.view(np.uint32)) | (np.isnan(got) & np.isnan(frame))).all()
    assert not np.array_equal(frames[0], frames[1])


def test_a_batch_waits_for_the_stream_that_writes_its_rays(hip, oracle, scenes, ref):
    sc, p, _, _, _ = camera_rays(oracle, scenes, "theater")
    rays, t = free_rays(oracle, scenes, "theater"), trace_params(p)
    want = wanted(ref, ("free", "theater", p.samples), sc, t, rays)
    hip.update_scene(sc)
    source = torch.from_numpy(rays).cuda()
    d = torch.zeros_like(source)
    busy = torch.ones((2048, 2048), device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):
            busy = busy @ busy * 1e-4                               # work in front of the write, so that the rays are not there when the call returns
        d.copy_(source)
        out = hip.trace_rays_device(d, t, stream=side)
    hip.sync()
    assert_rows(words_of(out), want, "rays written on a side stream")
    side.synchronize()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_refusals(hip, oracle, scenes, ref):
    sc, p, _, _, _ = camera_rays(oracle, scenes, "theater")
    rays_host, t = free_rays(oracle, scenes, "theater")[:256], trace_params(p)
    want = wanted(ref, ("free", "theater", p.samples), sc, t, free_rays(oracle, scenes, "theater"))[:256]
    with capi.Context(0) as fresh:
        for call in (lambda: fresh.trace_rays(rays_host, t), lambda: fresh.trace_rays_device(torch.zeros((4, 8), device="cuda"), t),
                     lambda: fresh.trace_rays_device((0, 0), t, 0)):
            with pytest.raises(capi.FlexLightHipError, match=r"failed \(3\): flx_rays_trace: no scene and transforms uploaded"):      # FLX_ERR_NO_SCENE
                call()
        assert fresh.last_trace()["slabs"] == 0
    hip.update_scene(sc)
    rays = torch.from_numpy(rays_host).cuda()
    out = torch.full((256, 32), 0xA5, dtype=torch.uint8, device="cuda")
    both = torch.zeros((512, 8), dtype=torch.float32, device="cuda")
    host = np.zeros((256, 8), np.float32)
    torch.cuda.synchronize()
    hip.trace_rays_device(rays, t, out)
    hip.sync()
    before = hip.last_trace()
    out.fill_(0xA5)
    torch.cuda.synchronize()

    def with_(**kw):
        q = trace_params(p)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    invalid = r"failed \(1\): "
    refused = [
        (lambda: hip.trace_rays_device(rays, None, out), "flx_rays_trace: params is NULL"),
        (lambda: hip.trace_rays(rays_host, None), "flx_rays_trace: params is NULL"),
        (lambda: hip.trace_rays_device(rays, with_(samples=0), out), "samples is less than 1"),
        (lambda: hip.trace_rays_device((0, 0), with_(samples=-3), 0), "samples is less than 1"),                                                   # for n == 0 too
        (lambda: hip.trace_rays(rays_host, with_(max_reflections=-1)), "max_reflections is negative"),
        (lambda: hip.trace_rays_device(rays, with_(texture_width=0), out), "texture_width is less than 1"),
        (lambda: hip.trace_rays_device((host.ctypes.data, 256), t, out), "the rays are not n rows in memory of the context's device"),            # host memory
        (lambda: hip.trace_rays_device(rays, t, host.ctypes.data), "the radiance is not n rows in memory of the context's device"),
        (lambda: hip.trace_rays_device((rays.data_ptr() + 4, 255), t, out), "the rays are not n rows in memory of the context's device, 16-byte aligned"),
        (lambda: hip.trace_rays_device(rays, t, out.data_ptr() + 8), "the radiance is not n rows in memory of the context's device, 16-byte aligned"),
        (lambda: hip.trace_rays_device((rays.data_ptr(), 1 << 28), t, out.data_ptr()), "the rays are not n rows"),                                 # 8 GB: the allocation ends first
        (lambda: hip.trace_rays_device((0, 4), t, out), "an array is NULL"),
        (lambda: hip.trace_rays_device(rays, t, 0), "an array is NULL"),
        (lambda: hip.trace_rays_device(both, t, both.data_ptr()), "the rays and the radiance overlap"),                                            # the same array
        (lambda: hip.trace_rays_device((both.data_ptr(), 256), t, both.data_ptr() + 255 * 32), "the rays and the radiance overlap"),               # the radiance begins in the last ray
        (lambda: hip.trace_rays_device((both.data_ptr() + 32, 256), t, both.data_ptr()), "the rays and the radiance overlap"),
    ]
    for call, message in refused:
        with pytest.raises(capi.FlexLightHipError, match=invalid + ".*" + message):
            call()
        assert hip.last_trace() == before, message                  # nothing was enqueued
    torch.cuda.synchronize()
    assert (out == 0xA5).all()
    # n == 0: FLX_OK, nothing enqueued
    hip.trace_rays_device(torch.zeros((0, 8), dtype=torch.float32, device="cuda"), t)
    hip.trace_rays_device((0, 0), t, 0)
    assert hip.trace_rays(np.zeros((0, 8), np.float32), t).shape == (0, 32)
    assert hip.last_trace() == before
    hip.trace_rays_device((both.data_ptr(), 256), t, both.data_ptr() + 256 * 32)      # side by side in one allocation: no overlap
    got = hip.trace_rays_device(rays, t, out)                       # after the refusals the next batch is right
    hip.sync()
    assert_rows(words_of(got), want, "after the refusals")
