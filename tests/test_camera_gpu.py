"""Cameras on the device (include/flexlight_hip_debug.h, "cameras"): k_camera_rays' rows are the CPU reference's bits (tests/camera_ref, the same
include/flx_camera.h) for every projection, face, size, region and batch; the image calls are flx_rays_image[_temporal]_device on those rays, bit for bit; the
ray call needs no scene; every refusal says its words and leaves the output as it was."""
import numpy as np
import pytest
import torch

from flexlight_hip import capi
from camera_util import JITTER, POSITION, assert_same_rows, cameras_of, reference, skewed_basis
from rays_trace_util import FRAMES, camera_rays, trace_params

pytestmark = pytest.mark.gpu

SPARE = 8          # rows behind the last one that must keep their poison
SIZES = ((1, 1), (7, 5), (64, 1), (65, 3), (33, 31))      # one lane; less than a wave; exactly a wave; one ray past a wave; more than one workgroup


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return reference(tmp_path_factory)


def poisoned(rows, row_bytes):
    return torch.full(((rows + SPARE) * row_bytes,), 0xA5, dtype=torch.uint8, device="cuda")


def every_camera():
    """all five projections, every face, with jitter and a basis that is no rotation (the pinhole: that matrix as its view matrix)"""
    basis = skewed_basis()
    return [capi.Camera(capi.CAMERA_PINHOLE, POSITION, basis, jitter=JITTER)] + list(cameras_of(capi, basis).values())


def device_rows(ctx, cameras, w, h, region=None):
    """camera_rays_device into a poisoned buffer -> float32 [n, 8]: nothing past the last row is written"""
    n = (len(cameras) if isinstance(cameras, list) else 1) * (region[2] * region[3] if region else w * h)
    out = poisoned(n, 32)
    torch.cuda.synchronize()
    assert ctx.camera_rays_device(cameras, w, h, region=region, out=out) is out
    ctx.sync()
    words = out.cpu().numpy().view(np.uint32)
    assert (words[n * 8:] == 0xA5A5A5A5).all()
    return words[:n * 8].view(np.float32).reshape(n, 8)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_device_rows_are_the_references_bits(hip, ref, size):
    w, h = size
    cams = every_camera()
    assert len(cams) == 10
    want = ref.rays(cams, w, h)
    assert np.isfinite(want).all()
    assert_same_rows(device_rows(hip, cams, w, h), want, "ten cameras in one call, %d x %d" % size)
    assert_same_rows(hip.camera_rays(cams, w, h), want, "the host variant")
    if size == (7, 5):
        for k, cam in enumerate(cams):
            assert_same_rows(device_rows(hip, cam, w, h), want[k * w * h:(k + 1) * w * h], "camera %d alone" % k)


def test_a_region_aligned_to_nothing_and_mixed_batches(hip, ref):
    w, h, region = 33, 31, (5, 7, 13, 9)
    cams = every_camera()
    mixed = [cams[1], cams[0], cams[7]]                     # a panorama, the pinhole, a cube face
    whole = ref.rays(mixed, w, h).reshape(3, h, w, 8)
    got = device_rows(hip, mixed, w, h, region)
    assert_same_rows(got, ref.rays(mixed, w, h, region=region), "three cameras' region")
    assert np.array_equal(got.reshape(3, 9, 13, 8).view(np.uint32), whole[:, 7:16, 5:18].view(np.uint32))      # the whole image's rows of those pixels
    assert_same_rows(hip.camera_rays(mixed, w, h, region=region), got, "the host variant")
    assert_same_rows(device_rows(hip, mixed, w, h, (32, 30, 1, 1)), whole[:, 30, 32], "the last pixel")
    # more cameras than one launch takes in its arguments (32): 33 ends a launch with one camera, 65 takes three launches
    for count in (32, 33, 65):
        many = [cams[k % 10] for k in range(count)]
        assert_same_rows(device_rows(hip, many, 7, 5), ref.rays(many, 7, 5), "%d cameras" % count)


def bits(image, ctx=None):
    """the words of an image; ctx: the context whose stream a tensor is still being written on"""
    if ctx is not None:
        ctx.sync()
    return np.ascontiguousarray(image.detach().cpu().numpy() if isinstance(image, torch.Tensor) else image).view(np.uint32)


def test_camera_images_are_ray_images_of_the_generated_rays(hip, oracle, scenes, ref):
    sc, p, rays, _, _ = camera_rays(oracle, scenes, "cornell")
    w, h = FRAMES["cornell"][0:2]
    t = trace_params(p)
    hip.update_scene(sc)
    pinhole = capi.Camera.pinhole(p)
    d = hip.camera_rays_device(pinhole, w, h)
    hip.sync()
    assert_same_rows(d.cpu().numpy(), rays, "cornell's own camera: the oracle's primary rays")
    panorama = capi.Camera.panorama(tuple(p.camera), skewed_basis(), jitter=JITTER)
    for cam, cw, ch in ((pinhole, w, h), (panorama, 32, 16)):
        generated = hip.camera_rays_device(cam, cw, ch)
        for hdr in (0, 1):
            want = hip.ray_image_device(generated, cw, ch, t, hdr=hdr)
            out = poisoned(cw * ch, 16)
            torch.cuda.synchronize()
            hip.camera_image_device(cam, cw, ch, t, hdr=hdr, out=out)
            hip.sync()
            words = out.cpu().numpy().view(np.uint32)
            assert (words[cw * ch * 4:] == 0xA5A5A5A5).all()
            assert np.array_equal(words[:cw * ch * 4], bits(want).reshape(-1)), (cam.projection, hdr)
            assert np.array_equal(bits(hip.camera_image(cam, cw, ch, t, hdr=hdr)).reshape(-1), bits(want).reshape(-1))
            image = want.cpu().numpy()
            assert np.isfinite(image).all() and (image[..., 3] > 0).any()
        assert hip.last_ray_planes()["n"] == cw * ch


@pytest.mark.parametrize("use_filter", [1, 0])
def test_temporal_camera_images_frame_by_frame(hip, oracle, scenes, use_filter):
    sc, p, _, _, _ = camera_rays(oracle, scenes, "cornell")
    w, h = FRAMES["cornell"][0:2]
    hip.update_scene(sc)
    cam = capi.Camera.pinhole(p, jitter=(0.25, -0.125))
    generated = hip.camera_rays_device(cam, w, h)
    temporal = capi.RayTemporal(history=3, temporal_samples=2, use_filter=use_filter, hdr=1)      # three frames on a ring of two slots
    seeded = lambda seed: capi.TraceParams(p.samples, p.max_reflections, p.min_importancy, tuple(p.ambient), seed, p.texture_width)
    hip.rays_history_reset(3)
    want = [bits(hip.rays_image_temporal(generated, w, h, seeded(f % 2), temporal, device=True), hip) for f in range(3)]
    hip.rays_history_reset(3)
    got = [bits(hip.camera_image_temporal_device(cam, w, h, seeded(f % 2), temporal), hip) for f in range(3)]
    assert hip.debug_last_ray_temporal()["history"] == 3 and hip.debug_last_ray_temporal()["depth"] == 2
    hip.rays_history_reset(3)
    host = [bits(hip.camera_image_temporal(cam, w, h, seeded(f % 2), temporal)) for f in range(3)]
    hip.rays_history_reset(3)
    for f in range(3):
        assert np.array_equal(got[f], want[f]) and np.array_equal(host[f], want[f]), "frame %d" % f
    assert not np.array_equal(want[0], want[2])            # the history counts: seed 0 again, another image


def test_a_camera_image_between_two_frames_of_the_loop(hip, oracle, scenes):
    sc, p, _, _, _ = camera_rays(oracle, scenes, "cornell")
    t = trace_params(p)
    hip.update_scene(sc)
    cam = capi.Camera.panorama(tuple(p.camera), skewed_basis())
    want = bits(hip.ray_image_device(hip.camera_rays_device(cam, 32, 16), 32, 16, t, hdr=1), hip)
    params = [sc.frame_params(width=48, height=36, samples=2, max_reflections=3, use_filter=0) for _ in range(2)]
    params[1].random_seed = params[0].random_seed + 1.0
    oracle_frames = [oracle.render(sc, q)[0] for q in params]
    out = poisoned(32 * 16, 16)
    torch.cuda.synchronize()
    for q in params:
        hip.frame_begin(q)
    assert hip.frames_in_flight() == 2
    hip.camera_image_device(cam, 32, 16, t, hdr=1, out=out)
    frames = [hip.frame_end()[0] for _ in params]
    hip.sync()
    words = out.cpu().numpy().view(np.uint32)
    assert (words[32 * 16 * 4:] == 0xA5A5A5A5).all() and np.array_equal(words[:32 * 16 * 4], want.reshape(-1))
    for got, frame in zip(frames, oracle_frames):
        got = np.asarray(got).reshape(frame.shape)
        assert ((got.view(np.uint32) == frame.view(np.uint32)) | (np.isnan(got) & np.isnan(frame))).all()
    assert not np.array_equal(frames[0], frames[1])


def test_rays_need_no_scene_and_images_do(ref):
    cams = every_camera()
    t = capi.TraceParams()
    with capi.Context(0) as fresh:
        assert_same_rows(device_rows(fresh, cams, 7, 5), ref.rays(cams, 7, 5), "a context without a scene")
        assert_same_rows(fresh.camera_rays(cams[2], 65, 3), ref.rays(cams[2], 65, 3), "its host variant")
        out = poisoned(16, 16)
        temporal = capi.RayTemporal()
        for call, name in ((lambda: fresh.camera_image(cams[1], 4, 4, t), "flx_camera_image"), (lambda: fresh.camera_image_device(cams[1], 4, 4, t, out=out), "flx_camera_image_device"),
                           (lambda: fresh.camera_image_temporal(cams[1], 4, 4, t, temporal), "flx_camera_image_temporal"),
                           (lambda: fresh.camera_image_temporal_device(cams[1], 4, 4, t, temporal, out=out), "flx_camera_image_temporal_device"),
                           (lambda: fresh.camera_image_device(None, 0, 0, None, out=0), "flx_camera_image_device")):
            with pytest.raises(capi.FlexLightHipError, match=r"failed \(3\): %s: no scene and transforms uploaded" % name):      # FLX_ERR_NO_SCENE
                call()
        fresh.sync()
        assert (out.cpu().numpy() == 0xA5).all() and fresh.last_ray_planes()["slabs"] == 0


def test_refusals(hip, oracle, scenes):
    sc, p, _, _, _ = camera_rays(oracle, scenes, "cornell")
    t = trace_params(p)
    hip.update_scene(sc)
    torch.cuda.empty_cache()                                        # (the allocations below are then the device's own, of exactly these sizes)
    good = capi.Camera.panorama(POSITION, skewed_basis(), jitter=JITTER)
    rows, image = poisoned(2 * 16, 32), poisoned(16, 16)
    short = torch.full((20 << 20,), 0xA5, dtype=torch.uint8, device="cuda")                   # 20 MB: too short for 1024 x 1024 rays (32 MB) and for a 2048 x 1024 image (32 MB)
    host = np.zeros((64, 8), np.float32)
    temporal = capi.RayTemporal(history=6, temporal_samples=3, use_filter=1, hdr=1)
    hip.rays_history_reset(6)
    hip.camera_image_temporal_device(good, 4, 4, t, temporal)       # a history to be left as it is
    hip.ray_image_device(hip.camera_rays_device(good, 4, 4), 4, 4, t)
    hip.sync()
    before, before_temporal = hip.last_ray_planes(), hip.debug_last_ray_temporal()
    torch.cuda.synchronize()

    def cam(**kw):
        c = capi.Camera.panorama(POSITION, skewed_basis(), jitter=JITTER)
        for k, v in kw.items():
            if isinstance(v, tuple):
                index, value = v
                getattr(c, k)[index] = value
            else:
                setattr(c, k, v)
        return c

    def with_(**kw):
        q = trace_params(p)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    R, I = rows.data_ptr(), image.data_ptr()
    rays_device = lambda cameras, w=4, h=4, region=None, out=rows: hip.camera_rays_device(cameras, w, h, region=region, out=out)
    image_device = lambda c, w=4, h=4, q=t, out=image: hip.camera_image_device(c, w, h, q, out=out)
    over_time = lambda c, w=4, h=4, q=t, tt=temporal, out=image: hip.camera_image_temporal_device(c, w, h, q, tt, out=out)
    nan, inf = float("nan"), float("inf")
    refused = [
        (lambda: rays_device(None), "flx_camera_rays_device: cameras is NULL or n_cameras is 0"),
        (lambda: rays_device([]), "flx_camera_rays_device: cameras is NULL or n_cameras is 0"),
        (lambda: hip.camera_rays([], 4, 4), "flx_camera_rays: cameras is NULL or n_cameras is 0"),
        (lambda: rays_device(good, 0, 4), "flx_camera_rays_device: width or height is 0"),
        (lambda: rays_device(good, 4, 0), "flx_camera_rays_device: width or height is 0"),
        (lambda: hip.camera_rays(good, 0, 0), "flx_camera_rays: width or height is 0"),
        (lambda: rays_device(good, 65536, 65536, out=R), "n_cameras \\* width \\* height is 2\\^32 or more"),
        (lambda: rays_device([good] * 4, 32768, 32768, out=R), "n_cameras \\* width \\* height is 2\\^32 or more"),
        (lambda: rays_device(good, region=(1, 1, 0, 2)), "flx_camera_rays_device: the region is empty"),
        (lambda: rays_device(good, region=(1, 1, 2, 0)), "flx_camera_rays_device: the region is empty"),
        (lambda: rays_device(good, region=(2, 0, 3, 1)), "flx_camera_rays_device: the region leaves the image"),
        (lambda: rays_device(good, region=(0, 3, 1, 2)), "flx_camera_rays_device: the region leaves the image"),
        (lambda: rays_device(good, region=(4, 0, 1, 1)), "flx_camera_rays_device: the region leaves the image"),
        (lambda: hip.camera_rays(good, 4, 4, region=(0, 0, 5, 4)), "flx_camera_rays: the region leaves the image"),
        (lambda: rays_device(cam(projection=5)), "flx_camera_rays_device: camera 0: projection is none of"),
        (lambda: rays_device(cam(projection=-1)), "camera 0: projection is none of"),
        (lambda: rays_device([good, cam(projection=4, face=6)]), "flx_camera_rays_device: camera 1: face is not one of 0 .. 5"),
        (lambda: rays_device(cam(face=-1)), "camera 0: face is not one of 0 .. 5"),
        (lambda: rays_device(cam(position=(1, nan))), "camera 0: position, basis, extent or jitter holds a value that is not finite"),
        (lambda: rays_device(cam(basis=(8, inf))), "holds a value that is not finite"),
        (lambda: rays_device(cam(extent=(1, -inf))), "holds a value that is not finite"),
        (lambda: rays_device(cam(jitter=(0, nan))), "holds a value that is not finite"),
        (lambda: rays_device(cam(jitter=(0, 0.6))), "camera 0: jitter is outside \\[-0.5, 0.5\\]"),
        (lambda: rays_device(cam(jitter=(1, -0.5000001))), "jitter is outside \\[-0.5, 0.5\\]"),
        (lambda: rays_device(cam(extent=(0, 0.0))), "camera 0: an extent the projection reads is not above 0"),
        (lambda: rays_device(cam(extent=(1, -1.0))), "an extent the projection reads is not above 0"),
        (lambda: rays_device(cam(projection=2, extent=(0, -2.0))), "an extent the projection reads is not above 0"),
        (lambda: hip.camera_rays([good, good, cam(projection=3, extent=(1, 0.0))], 4, 4), "flx_camera_rays: camera 2: an extent the projection reads is not above 0"),
        (lambda: rays_device(good, out=0), "flx_camera_rays_device: the output is NULL"),
        (lambda: rays_device(good, out=host.ctypes.data), "the output is not n_cameras \\* w \\* h rows in memory of the context's device"),      # host memory
        (lambda: rays_device(good, out=R + 8), "in memory of the context's device, 16-byte aligned"),
        (lambda: rays_device(good, 1024, 1024, out=short.data_ptr()), "the output is not n_cameras \\* w \\* h rows"),                     # an allocation too short
        # the image calls: the params and the size in flx_rays_image's words, the camera's in its own, the image
        (lambda: image_device(good, q=None), "flx_camera_image_device: params is NULL"),
        (lambda: hip.camera_image(good, 4, 4, None), "flx_camera_image: params is NULL"),
        (lambda: over_time(good, q=with_(samples=0)), "flx_camera_image_temporal_device: samples is less than 1"),
        (lambda: image_device(good, q=with_(max_reflections=-1)), "max_reflections is negative"),
        (lambda: image_device(good, q=with_(texture_width=0)), "texture_width is less than 1"),
        (lambda: image_device(good, 0, 4), "flx_rays_image_device: width or height is 0"),
        (lambda: hip.camera_image(good, 4, 0, t), "flx_rays_image_device: width or height is 0"),
        (lambda: over_time(good, 0, 0), "flx_rays_image_temporal_device: width or height is 0"),
        (lambda: image_device(good, 65536, 65536, out=I), "flx_rays_image_device: width \\* height is 2\\^32 or more"),
        (lambda: over_time(good, tt=None), "flx_rays_image_temporal_device: temporal is NULL"),
        (lambda: over_time(good, tt=capi.RayTemporal(history=8)), "flx_rays_image_temporal_device: history is not one of 0 .. 7"),
        (lambda: hip.camera_image_temporal(good, 4, 4, t, capi.RayTemporal(history=6, use_filter=2)), "use_filter is neither 0 nor 1"),
        (lambda: over_time(good, tt=capi.RayTemporal(history=6, hdr=-1)), "hdr is neither 0 nor 1"),
        (lambda: image_device(None), "flx_camera_image_device: cameras is NULL or n_cameras is 0"),
        (lambda: over_time(None), "flx_camera_image_temporal_device: cameras is NULL or n_cameras is 0"),
        (lambda: image_device(cam(projection=9)), "flx_camera_image_device: camera 0: projection is none of"),
        (lambda: over_time(cam(jitter=(0, 0.75))), "flx_camera_image_temporal_device: camera 0: jitter is outside"),
        (lambda: hip.camera_image(cam(extent=(0, 0.0)), 4, 4, t), "flx_camera_image: camera 0: an extent the projection reads is not above 0"),
        (lambda: image_device(good, out=0), "flx_camera_image_device: the image is NULL"),
        (lambda: over_time(good, out=0), "flx_camera_image_temporal_device: the image is NULL"),
        (lambda: image_device(good, out=host.ctypes.data), "the image is not width \\* height float4 in memory of the context's device"),
        (lambda: over_time(good, out=I + 8), "the image is not width \\* height float4 in memory of the context's device, 16-byte aligned"),
        (lambda: image_device(good, 2048, 1024, out=short.data_ptr()), "the image is not width \\* height float4"),
    ]
    for call, words in refused:
        with pytest.raises(capi.FlexLightHipError, match=r"failed \(1\): .*" + words):      # FLX_ERR_INVALID
            call()
    hip.sync()
    for buffer in (rows, image, short):
        assert bool((buffer == 0xA5).all())                        # nothing was written
    assert hip.last_ray_planes() == before and hip.debug_last_ray_temporal() == before_temporal      # ... and nothing traced
    # the history is exactly what it was: the next image continues it (the head moves on by one slot of three)
    hip.camera_image_temporal_device(good, 4, 4, t, temporal)
    after = hip.debug_last_ray_temporal()
    assert after["depth"] == 3 and after["head"] == (before_temporal["head"] + 2) % 3
    hip.rays_history_reset(6)
    # the calls still work
    assert np.isfinite(device_rows(hip, good, 4, 4)).all()
