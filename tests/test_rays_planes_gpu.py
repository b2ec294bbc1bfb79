"""Filter planes of ray batches and denoised ray images on the GPU (flx_rays_planes[_device], flx_rays_image[_device]: csrc/flx_rays_planes.hip) against the CPU
reference (tests/rays_planes_ref, which calls the oracle's own rayTracer and lightTrace and writes the planes by fragment_main's filter branch) and the oracle's own
denoise chain: every float bit for bit (a NaN equal to a NaN), every RGBA8 texel.  On a camera's rays the planes also equal flx_render_planes_device's wherever the
frame's hit rule and rayTracer agree (rays_trace_util.camera_rays), and the image equals flx_render's filtered frame.  Every output goes into a buffer poisoned with
0xA5 with rows to spare behind the last plane."""
import numpy as np
import pytest
import torch

from flexlight_hip import capi
from rays_planes_util import assert_floats, assert_texels, oracle_chain, quant, reference, wanted
from rays_trace_util import FRAMES, camera_rays, free_rays, trace_params
from scene_update_util import reflatten_by_rule, with_geometry

pytestmark = pytest.mark.gpu

SPARE = 8          # rows behind the last plane that must keep their poison


@pytest.fixture(scope="module")
def ref(tmp_path_factory, oracle):
    return reference(tmp_path_factory)


def poisoned(rows, row_bytes):
    return torch.full(((rows + SPARE) * row_bytes,), 0xA5, dtype=torch.uint8, device="cuda")


def on_device(rays, n=None):
    return torch.from_numpy(np.ascontiguousarray(rays[:n] if n is not None else rays)).cuda()


def planes_of(hip, rays, t, n=None, bytes_=True, floats=True, stream=None, d=None):
    """rays (numpy [n, 8]) through ray_planes_device into poisoned buffers -> (planes8 uint32 [5, n] or None, planes32 float32 [5, n, 4] or None): nothing past
    5 n rows is written, the rays are read only, and plane p starts at row p * n"""
    if d is None:
        d = on_device(rays, n)
    keep = d.clone()
    n = d.shape[0]
    out8 = poisoned(5 * n, 4) if bytes_ else None
    out32 = poisoned(5 * n, 16) if floats else None
    torch.cuda.synchronize()
    got8, got32 = hip.ray_planes_device(d, t, planes8=out8, planes32=out32, stream=stream)
    assert got8 is out8 and got32 is out32
    hip.sync()
    assert torch.equal(d, keep)
    p8 = p32 = None
    if bytes_:
        words = out8.cpu().numpy().view(np.uint32)
        assert (words[5 * n:] == 0xA5A5A5A5).all()
        p8 = words[:5 * n].reshape(5, n)
    if floats:
        words = out32.cpu().numpy().view(np.uint32)
        assert (words[5 * n * 4:] == 0xA5A5A5A5).all()
        p32 = words[:5 * n * 4].view(np.float32).reshape(5, n, 4)
    return p8, p32


def image_of(hip, rays, w, h, t, hdr, stream=None, d=None):
    """rays through ray_image_device into a poisoned buffer -> float32 [h, w, 4]"""
    if d is None:
        d = on_device(rays)
    keep = d.clone()
    out = poisoned(w * h, 16)
    torch.cuda.synchronize()
    assert hip.ray_image_device(d, w, h, t, hdr=hdr, out=out, stream=stream) is out
    hip.sync()
    words = out.cpu().numpy().view(np.uint32)
    assert (words[w * h * 4:] == 0xA5A5A5A5).all() and torch.equal(d, keep)
    return words[:w * h * 4].view(np.float32).reshape(h, w, 4)


def assert_planes(got8, got32, want, what):
    if got32 is not None:
        assert_floats(got32, want, what + ": planes32")
    if got8 is not None:
        assert_texels(got8, quant(want), what + ": planes8")


# ---- a camera's rays: the reference's planes, the library's own planes and its own filtered frame -----------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(FRAMES))
def test_a_cameras_rays_equal_the_reference_the_frames_planes_and_the_filtered_frame(hip, oracle, scenes, ref, name):
    sc, p, rays, compares, _ = camera_rays(oracle, scenes, name)
    w, h, samples, bounces, must = FRAMES[name]
    assert compares.sum() >= must
    t = trace_params(p)
    want, hit = wanted(ref, ("camera", name), sc, t, rays)
    hip.update_scene(sc)
    got8, got32 = planes_of(hip, rays, t)
    assert_planes(got8, got32, want, name)
    info = hip.last_ray_planes()
    assert (info["slabs"], info["n"], info["samples"], info["block"]) == (1, w * h, samples, 64)
    q = sc.frame_params(width=w, height=h, samples=samples, max_reflections=bounces, use_filter=1)
    frame_planes = torch.full((5, w * h), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    hip.render_planes_device(q, frame_planes.data_ptr())
    hip.sync()
    differ = (got8 != frame_planes.cpu().numpy().view(np.uint32)) & compares[None, :]
    assert not differ.any(), (name, np.argwhere(differ)[:8])
    for hdr in (0, 1):
        image = image_of(hip, rays, w, h, t, hdr)
        assert_floats(image, oracle_chain(oracle, want, w, h, hdr, key=("camera", name)), "%s hdr %d: the oracle's chain" % (name, hdr))
        if name != "cornell":
            assert compares.all()                                                # 1296 and 576 in FRAMES: the whole image is flx_render's
            q.hdr = hdr
            assert_floats(image, hip.render(q)[0], "%s hdr %d: flx_render with use_filter = 1" % (name, hdr))
        assert_floats(hip.ray_image(rays, w, h, t, hdr=hdr), image, "%s hdr %d: the host call" % (name, hdr))
    host8, host32 = hip.ray_planes(rays, t, floats=True)                          # the host calls: the same bytes
    assert np.array_equal(host8, got8) and np.array_equal(host32.view(np.uint32), got32.view(np.uint32))
    assert np.array_equal(hip.ray_planes(rays[:5], t), got8[:, :5])
    assert tuple(capi.unpack_planes(host8)) == capi.PLANE_NAMES
    assert (hip.last_ray_planes()["n"], hip.last_ray_planes()["slabs"]) == (5, 1)


# ---- rays that no camera makes, laid out as an image ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dragon", "theater"])
def test_free_rays_equal_the_reference_and_the_oracles_chain(hip, oracle, scenes, ref, name):
    """dragon: three transforms, glass and metals, the lane walk; theater: atlases, 9 lights, the lockstep walk"""
    sc, p, _, _, _ = camera_rays(oracle, scenes, name)
    rays, t = free_rays(oracle, scenes, name), trace_params(p)
    want, hit = wanted(ref, ("free", name, p.samples), sc, t, rays)
    assert rays.shape[0] == 2160 == 60 * 36 and hit.mean() >= 0.30 and (~hit).mean() >= 0.05      # the conditions on the inputs
    assert (want[:, ~hit].view(np.uint32) == 0).all()
    hip.update_scene(sc)
    got8, got32 = planes_of(hip, rays, t)
    assert_planes(got8, got32, want, name)
    assert hip.last_ray_planes()["lockstep"] == int(name == "theater")               # both builds run across the two scenes
    for hdr in (0, 1):
        assert_floats(image_of(hip, rays, 60, 36, t, hdr), oracle_chain(oracle, want, 60, 36, hdr, key=("free", name)), "%s hdr %d" % (name, hdr))
    assert hip.last_ray_planes()["lockstep"] == int(name == "theater")


# ---- shapes where the refill and the plane layout can go wrong ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dragon", "theater"])
def test_sizes_samples_groups_and_slabs(hip, oracle, scenes, ref, name):
    sc, p, _, _, _ = camera_rays(oracle, scenes, name)
    rays = free_rays(oracle, scenes, name)[900:1260]                              # rays from surfaces and rays from free space
    cus = hip.device_info()[1]
    hip.update_scene(sc)
    try:
        for samples in (1, 3):
            t = trace_params(p)
            t.samples = samples
            want, hit = wanted(ref, ("shapes", name, samples), sc, t, rays)
            assert 0.2 < hit[:257].mean() < 0.95
            for groups in (0, 1):                                                 # one workgroup: every lane takes ray after ray
                hip.set_query_groups(groups)
                for n in (1, 63, 64, 65, 257):
                    got8, got32 = planes_of(hip, rays, t, n)
                    assert_planes(got8, got32, want[:, :n], "%s S %d groups %d n %d" % (name, samples, groups, n))
                    info = hip.last_ray_planes()
                    assert (info["slabs"], info["n"], info["samples"]) == (1, n, samples)
                    assert info["groups"] == (groups or min(-(-(-(-n // 64)) // 4), cus * 8)) and info["query_groups"] == 1
            # a slab ceiling forced small: three slabs and more, a ragged last one, slabs that are no whole blocks of 64 rays, under both workgroup settings
            for groups, slab, n in ((0, 100, 257), (1, 100, 257), (0, 64, 360), (1, 1, 5), (0, 129, 360)):
                hip.set_query_groups(groups)
                hip.set_trace_slab(slab)
                got8, got32 = planes_of(hip, rays, t, n)
                assert_planes(got8, got32, want[:, :n], "%s S %d groups %d slab %d n %d" % (name, samples, groups, slab, n))
                info = hip.last_ray_planes()
                assert info["slabs"] == -(-n // slab) >= 3 and (slab == 1 or n % slab != 0) and (info["slab"], info["n"], info["samples"]) == (slab, n, samples)
                hip.set_trace_slab(0)
            hip.set_query_groups(0)
            hip.set_trace_slab(129)                                               # one kind of plane alone, over slabs
            only8, none32 = planes_of(hip, rays, t, 360, floats=False)
            none8, only32 = planes_of(hip, rays, t, 360, bytes_=False)
            assert none32 is None and none8 is None
            assert_planes(only8, only32, want, "%s S %d one kind of plane" % (name, samples))
            hip.set_trace_slab(0)
            only8, _ = planes_of(hip, rays, t, 65, floats=False)
            _, only32 = planes_of(hip, rays, t, 65, bytes_=False)
            assert_planes(only8, only32, want[:, :65], "%s S %d one kind of plane, n 65" % (name, samples))
    finally:
        hip.set_query_groups(0)
        hip.set_trace_slab(0)


# ---- the loop guard --------------------------------------------------------------------------------------------------------------------------------------------------------

def test_loop_guard_cases(hip, oracle, scenes, ref):
    sc, p, rays, _, first = camera_rays(oracle, scenes, "dragon")
    hit = first[:, 4] != -1
    hip.update_scene(sc)
    for key, value in (("max_reflections", 0), ("min_importancy", 2.0), ("max_reflections", 1)):
        t = trace_params(p)
        setattr(t, key, value)
        want, _ = wanted(ref, ("guard", key, value), sc, t, rays)
        got8, got32 = planes_of(hip, rays, t)
        assert_planes(got8, got32, want, "%s = %s" % (key, value))
        if (key, value) != ("max_reflections", 1):                                # nothing shaded: the colour is the ambient light's, the accumulators are untouched
            ambient = np.array(p.ambient[:], np.float32)
            assert hit.sum() > 1000 and (got32[0][hit, 0:3] == ambient - np.floor(ambient)).all()
            assert (got32[2][hit, 0:3] == 1.0).all() and (got32[3][hit, 0:3] == 0.0).all()


# ---- order -------------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_batch_sees_the_lights_uploaded_before_it(hip, oracle, scenes, ref):
    import copy
    sc, p, _, _, _ = camera_rays(oracle, scenes, "theater")
    rays, t = free_rays(oracle, scenes, "theater")[:512], trace_params(p)
    lights = sc.arrays["lights"].reshape(-1, 6).copy()[::2]
    lights[:, 0:3] += np.float32(3.0)
    lights[:, 3] *= np.float32(0.5)
    other = copy.copy(sc)
    other.arrays = dict(sc.arrays, lights=np.ascontiguousarray(lights.reshape(-1)))
    before, after = wanted(ref, ("free512", "theater"), sc, t, rays)[0], ref.planes(other, t, rays)[0]
    assert (quant(before) != quant(after)).any(axis=0).mean() > 0.2
    hip.update_scene(sc)
    assert_planes(*planes_of(hip, rays, t), before, "the scene's lights")
    hip.update_primary_light_sources(lights)
    assert_planes(*planes_of(hip, rays, t), after, "other lights")


def test_a_batch_sees_the_rows_updated_before_it(hip, oracle, scenes, ref):
    sc, p, rays, _, first = camera_rays(oracle, scenes, "cornell")
    t = trace_params(p)
    entry = int(first[len(first) // 2 + 16, 4])                                 # the triangle the centre pixel sees
    assert entry >= 0
    g = sc.arrays["geometry"].reshape(-1, 12).copy()
    assert g[entry, 10] == 2
    g[entry, [1, 4, 7]] += np.float32(500.0)                                      # the triangle leaves, out of every ray's way
    moved = with_geometry(sc, reflatten_by_rule(g))
    before, after = wanted(ref, ("camera", "cornell"), sc, t, rays)[0], ref.planes(moved, t, rays)[0]
    assert (first[:, 4] == entry).sum() > 10 and (quant(before) != quant(after)).any(axis=0).sum() > 10
    hip.update_scene(sc)
    assert_planes(*planes_of(hip, rays, t), before, "as uploaded")
    hip.update_scene_rows(entry, g[entry:entry + 1])
    assert_planes(*planes_of(hip, rays, t), after, "after flx_scene_update")


def test_a_ray_image_between_two_frames_of_the_loop(hip, oracle, scenes, ref):
    sc, p, _, _, _ = camera_rays(oracle, scenes, "dragon")
    rays, t = free_rays(oracle, scenes, "dragon"), trace_params(p)
    want, _ = wanted(ref, ("free", "dragon", p.samples), sc, t, rays)
    hip.update_scene(sc)
    params = [sc.frame_params(width=96, height=54, samples=2, max_reflections=4, use_filter=0) for _ in range(2)]
    params[1].random_seed = params[0].random_seed + 1.0
    oracle_frames = [oracle.render(sc, q)[0] for q in params]
    d = on_device(rays)
    out = poisoned(2160, 16)
    torch.cuda.synchronize()
    for q in params:
        hip.frame_begin(q)
    assert hip.frames_in_flight() == 2
    hip.ray_image_device(d, 60, 36, t, hdr=1, out=out)
    frames = [hip.frame_end()[0] for _ in params]
    hip.sync()
    words = out.cpu().numpy().view(np.uint32)
    assert (words[2160 * 4:] == 0xA5A5A5A5).all()
    assert_floats(words[:2160 * 4].view(np.float32).reshape(36, 60, 4), oracle_chain(oracle, want, 60, 36, 1, key=("free", "dragon")), "between two frames")
    for got, frame in zip(frames, oracle_frames):
        got = np.asarray(got).reshape(frame.shape)
        assert ((got.view(np.uint32) == frame.view(np.uint32)) | (np.isnan(got) & np.isnan(frame))).all()
    assert not np.array_equal(frames[0], frames[1])


def test_a_batch_waits_for_the_stream_that_writes_its_rays(hip, oracle, scenes, ref):
    sc, p, _, _, _ = camera_rays(oracle, scenes, "theater")
    rays, t = free_rays(oracle, scenes, "theater"), trace_params(p)
    want, _ = wanted(ref, ("free", "theater", p.samples), sc, t, rays)
    hip.update_scene(sc)
    source = on_device(rays)
    d, e = torch.zeros_like(source), torch.zeros_like(source)
    busy = torch.ones((2048, 2048), device="cuda")
    out8, out = poisoned(5 * 2160, 4), poisoned(2160, 16)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):
            busy = busy @ busy * 1e-4                               # work in front of the write, so that the rays are not there when the call returns
        d.copy_(source)
        hip.ray_planes_device(d, t, planes8=out8, stream=side)
        for _ in range(8):
            busy = busy @ busy * 1e-4
        e.copy_(source)
        hip.ray_image_device(e, 60, 36, t, hdr=0, out=out, stream=side)
    hip.sync()
    assert_texels(out8.cpu().numpy().view(np.uint32)[:5 * 2160].reshape(5, 2160), quant(want), "rays written on a side stream")
    assert_floats(out.cpu().numpy().view(np.float32)[:2160 * 4].reshape(36, 60, 4), oracle_chain(oracle, want, 60, 36, 0, key=("free", "theater")), "an image of them")
    side.synchronize()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_refusals(hip, oracle, scenes, ref):
    sc, p, _, _, _ = camera_rays(oracle, scenes, "theater")
    all_rays, t = free_rays(oracle, scenes, "theater"), trace_params(p)
    rays_host = all_rays[:256]
    want = wanted(ref, ("free", "theater", p.samples), sc, t, all_rays)[0][:, :256]
    with capi.Context(0) as fresh:
        for call, name in ((lambda: fresh.ray_planes(rays_host, t), "flx_rays_planes"), (lambda: fresh.ray_planes_device(torch.zeros((4, 8), device="cuda"), t), "flx_rays_planes_device"),
                           (lambda: fresh.ray_planes_device((0, 0), t, 0, 0), "flx_rays_planes_device"), (lambda: fresh.ray_image(rays_host, 16, 16, t), "flx_rays_image"),
                           (lambda: fresh.ray_image_device((0, 0), 0, 0, t, out=0), "flx_rays_image_device")):
            with pytest.raises(capi.FlexLightHipError, match=r"failed \(3\): %s: no scene and transforms uploaded" % name):      # FLX_ERR_NO_SCENE
                call()
        assert fresh.last_ray_planes()["slabs"] == 0
    hip.update_scene(sc)
    torch.cuda.empty_cache()                                        # (the allocations below are then the device's own, of exactly these sizes)
    rays = on_device(rays_host)
    out8, out32, image = poisoned(5 * 256, 4), poisoned(5 * 256, 16), poisoned(256, 16)
    both = torch.zeros((2048, 8), dtype=torch.float32, device="cuda")
    many = torch.zeros((1 << 21, 8), dtype=torch.float32, device="cuda")                      # 64 MB of rays ...
    short = torch.full((20 << 20,), 0xA5, dtype=torch.uint8, device="cuda")                   # ... and 20 MB: too short for their byte planes (40 MB), float planes and image
    host = np.zeros((5 * 256, 4), np.float32)
    torch.cuda.synchronize()
    hip.ray_planes_device(rays, t, planes8=poisoned(5 * 256, 4))
    hip.sync()
    before = hip.last_ray_planes()
    torch.cuda.synchronize()

    def with_(**kw):
        q = trace_params(p)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    B, R = both.data_ptr(), rays.data_ptr()
    invalid = r"failed \(1\): "
    refused = [
        (lambda: hip.ray_planes_device(rays, None, out8), "flx_rays_planes_device: params is NULL"),
        (lambda: hip.ray_planes(rays_host, None), "flx_rays_planes: params is NULL"),
        (lambda: hip.ray_image_device(rays, 16, 16, None, out=image), "flx_rays_image_device: params is NULL"),
        (lambda: hip.ray_image(rays_host, 16, 16, None), "flx_rays_image: params is NULL"),
        (lambda: hip.ray_planes_device(rays, with_(samples=0), out8), "samples is less than 1"),
        (lambda: hip.ray_planes_device((0, 0), with_(samples=-3), 0, 0), "samples is less than 1"),                                                # for n == 0 too
        (lambda: hip.ray_planes(rays_host, with_(max_reflections=-1)), "max_reflections is negative"),
        (lambda: hip.ray_image_device(rays, 16, 16, with_(texture_width=0), out=image), "texture_width is less than 1"),
        (lambda: hip.ray_planes_device(rays, t, 0, 0), "flx_rays_planes_device: planes8 and planes32 are both NULL"),
        (lambda: hip.ray_image_device((R, 0), 0, 16, t, out=image), "flx_rays_image_device: width or height is 0"),
        (lambda: hip.ray_image_device((R, 0), 16, 0, t, out=image), "flx_rays_image_device: width or height is 0"),
        (lambda: hip.ray_image(np.zeros((0, 8), np.float32), 0, 0, t), "flx_rays_image: width or height is 0"),
        (lambda: hip.ray_image_device((R, 1 << 32), 65536, 65536, t, out=image.data_ptr()), "flx_rays_image_device: width \\* height is 2\\^32 or more"),
        (lambda: hip.ray_planes_device((0, 4), t, out8), "flx_rays_planes_device: an array is NULL"),
        (lambda: hip.ray_image_device((0, 256), 16, 16, t, out=image), "flx_rays_image_device: an array is NULL"),
        (lambda: hip.ray_image_device(rays, 16, 16, t, out=0), "flx_rays_image_device: an array is NULL"),
        (lambda: hip.ray_planes_device((host.ctypes.data, 256), t, out8), "the rays are not n rows in memory of the context's device"),             # host memory
        (lambda: hip.ray_planes_device(rays, t, host.ctypes.data), "planes8 is not 5 n texels in memory of the context's device"),
        (lambda: hip.ray_planes_device(rays, t, out8, host.ctypes.data), "planes32 is not 5 n rows in memory of the context's device"),
        (lambda: hip.ray_image_device(rays, 16, 16, t, out=host.ctypes.data), "the image is not width \\* height float4 in memory of the context's device"),
        (lambda: hip.ray_planes_device((R + 4, 255), t, out8), "the rays are not n rows in memory of the context's device, 16-byte aligned"),
        (lambda: hip.ray_planes_device(rays, t, out8.data_ptr() + 4), "planes8 is not 5 n texels in memory of the context's device, 16-byte aligned"),
        (lambda: hip.ray_planes_device(rays, t, None, out32.data_ptr() + 8), "planes32 is not 5 n rows in memory of the context's device, 16-byte aligned"),
        (lambda: hip.ray_image_device(rays, 16, 16, t, out=image.data_ptr() + 8), "the image is not width \\* height float4 in memory of the context's device, 16-byte aligned"),
        (lambda: hip.ray_planes_device((R, 1 << 28), t, out8.data_ptr()), "the rays are not n rows"),                                              # 8 GB: the allocation ends first
        (lambda: hip.ray_image_device((R, 1 << 28), 1 << 14, 1 << 14, t, out=image.data_ptr()), "the rays are not width \\* height rows"),
        (lambda: hip.ray_planes_device(many, t, short.data_ptr()), "planes8 is not 5 n texels"),                                                   # allocations too short
        (lambda: hip.ray_planes_device(many, t, None, short.data_ptr()), "planes32 is not 5 n rows"),
        (lambda: hip.ray_image_device(many, 2048, 1024, t, out=short.data_ptr()), "the image is not width \\* height float4"),
        (lambda: hip.ray_planes_device((B, 256), t, B), "flx_rays_planes_device: the rays and an output overlap"),                                 # the same array
        (lambda: hip.ray_planes_device((B, 256), t, None, B + 255 * 32), "flx_rays_planes_device: the rays and an output overlap"),                # the floats begin in the last ray
        (lambda: hip.ray_planes_device((B + 5 * 256 * 4 - 16, 256), t, B), "flx_rays_planes_device: the rays and an output overlap"),              # the rays begin in the fifth byte plane
        (lambda: hip.ray_planes_device((B, 256), t, out8, B + 16), "flx_rays_planes_device: the rays and an output overlap"),
        (lambda: hip.ray_planes_device(rays, t, B, B), "flx_rays_planes_device: planes8 and planes32 overlap"),
        (lambda: hip.ray_planes_device(rays, t, B + 5 * 256 * 16 - 16, B), "flx_rays_planes_device: planes8 and planes32 overlap"),                 # the bytes begin in the fifth float plane
        (lambda: hip.ray_planes_device(rays, t, B, B + 5 * 256 * 4 - 16), "flx_rays_planes_device: planes8 and planes32 overlap"),
        (lambda: hip.ray_image_device((B, 256), 16, 16, t, out=B), "flx_rays_image_device: the rays and an output overlap"),
        (lambda: hip.ray_image_device((B, 256), 16, 16, t, out=B + 255 * 32), "flx_rays_image_device: the rays and an output overlap"),
        (lambda: hip.ray_image_device((B + 255 * 16, 256), 16, 16, t, out=B), "flx_rays_image_device: the rays and an output overlap"),
    ]
    messages = set()
    for call, message in refused:
        with pytest.raises(capi.FlexLightHipError, match=invalid + ".*" + message) as caught:
            call()
        messages.add(str(caught.value))
        assert hip.last_ray_planes() == before, message                 # nothing was enqueued
    assert len(messages) >= 20                                      # every refusal says it in words of its own (the same rule refused twice says them twice)
    torch.cuda.synchronize()
    for buffer in (out8, out32, image, short):
        assert (buffer == 0xA5).all()
    assert not both.any() and not many.any()
    # n == 0: FLX_OK, nothing enqueued, no array looked at
    hip.ray_planes_device(torch.zeros((0, 8), dtype=torch.float32, device="cuda"), t)
    hip.ray_planes_device((0, 0), t, 0, 0)
    assert hip.ray_planes(np.zeros((0, 8), np.float32), t).shape == (5, 0)
    assert hip.last_ray_planes() == before
    hip.ray_planes_device((B, 256), t, B + 256 * 32, B + 256 * 32 + 5 * 256 * 4)      # side by side in one allocation: no overlap
    hip.ray_image_device((B, 256), 16, 16, t, out=B + 256 * 32)
    hip.sync()
    got8, got32 = planes_of(hip, rays_host, t)                      # after the refusals the next call is right
    assert_planes(got8, got32, want, "after the refusals")
    assert_floats(image_of(hip, rays_host, 16, 16, t, 1), oracle_chain(oracle, want, 16, 16, 1), "an image after the refusals")
