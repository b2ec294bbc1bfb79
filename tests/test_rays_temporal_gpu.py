"""Temporal accumulation of ray images on the GPU (flx_rays_image_temporal[_device], flx_rays_history_reset: csrc/flx_rays_planes.hip, the temporal instantiations of
k_rays_planes) against the CPU reference (tests/rays_temporal_ref: the oracle's own lightTrace for a frame's six planes, its own temporal_pass and filter_chain_u8
over rings held in Python): every frame of every sequence bit for bit on every pixel (a NaN equal to a NaN).  On a camera's rays the sequences also equal
flx_render's temporal sequences wherever the frame's hit rule and rayTracer agree (rays_trace_util.camera_rays).  Every image goes into a buffer poisoned with 0xA5
with rows to spare behind it.  Images are at most 48 x 27 at 2 samples."""
import copy

import numpy as np
import pytest
import torch

from flexlight_hip import capi
from rays_planes_util import oracle_chain, reference as planes_reference, wanted
from rays_temporal_util import assert_floats, depth_of, reference, same_floats, seeded, sequence, traced
from rays_trace_util import FRAMES, camera_rays, free_rays, trace_params
from scene_update_util import reflatten_by_rule, with_geometry

pytestmark = pytest.mark.gpu

SPARE = 8          # rows behind the image that must keep their poison


@pytest.fixture(scope="module")
def ref(tmp_path_factory, oracle):
    return reference(tmp_path_factory)


@pytest.fixture()
def fresh(hip):
    """the shared context with no ray history and the library's own launch shapes, before and after"""
    hip.set_query_groups(0)
    hip.set_trace_slab(0)
    hip.rays_history_reset(-1)
    yield hip
    hip.set_query_groups(0)
    hip.set_trace_slab(0)
    hip.rays_history_reset(-1)


def on_device(rays):
    return torch.from_numpy(np.ascontiguousarray(rays, np.float32)).cuda()


def poisoned(rows):
    return torch.full(((rows + SPARE) * 16,), 0xA5, dtype=torch.uint8, device="cuda")


def image_of(hip, d, w, h, t, temporal, stream=None):
    """device rays through rays_image_temporal into a poisoned buffer -> float32 [h, w, 4]: only width * height rows are written, the rays are read only"""
    keep = d.clone()
    out = poisoned(w * h)
    torch.cuda.synchronize()
    assert hip.rays_image_temporal(d, w, h, t, temporal, device=True, out=out, stream=stream) is out
    hip.sync()
    words = out.cpu().numpy().view(np.uint32)
    assert (words[w * h * 4:] == 0xA5A5A5A5).all() and torch.equal(d, keep)
    return words[:w * h * 4].view(np.float32).reshape(h, w, 4)


def frame_sequence(hip, sc, w, h, samples, bounces, depth, use_filter, hdr, frames):
    """flx_render's temporal sequence after flx_temporal_reset, seed f % N"""
    hip.temporal_reset()
    out = []
    for f in range(frames):
        q = sc.frame_params(width=w, height=h, samples=samples, max_reflections=bounces, use_filter=use_filter, hdr=hdr)
        q.is_temporal, q.temporal_samples, q.random_seed = 1, depth, float(f % depth_of(depth))
        out.append(hip.render(q)[0])
    return out


# ---- 1. a camera's rays, standing still ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,depth", [("dragon", 1), ("dragon", 4), ("dragon", 5), ("theater", 1), ("theater", 4), ("theater", 5), ("theater", 16),
                                        ("cornell", 1), ("cornell", 4), ("cornell", 5)])
def test_a_cameras_rays_standing_still(fresh, oracle, scenes, ref, name, depth):
    """N + 2 frames, so the ring wraps; N = 5: a full group of four slots plus the stand-ins; N = 1: no history at all"""
    hip = fresh
    sc, p, rays, compares, _ = camera_rays(oracle, scenes, name)
    w, h, samples, bounces, must = FRAMES[name]
    assert compares.sum() >= must and compares.size == w * h
    t, frames = trace_params(p), depth + 2
    hip.update_scene(sc)
    d = on_device(rays)
    pixels = compares.reshape(h, w)
    for use_filter in (0, 1):
        for hdr in (0, 1):
            what = "%s N %d use_filter %d hdr %d" % (name, depth, use_filter, hdr)
            want = sequence(ref, ("camera", name), sc, t, rays, w, h, depth, use_filter, hdr, frames)
            temporal = capi.RayTemporal(history=3, temporal_samples=depth, use_filter=use_filter, hdr=hdr)
            hip.rays_history_reset(3)
            got = []
            for f in range(frames):
                got.append(image_of(hip, d, w, h, seeded(t, f % depth), temporal))
                assert_floats(got[f], want[f], "%s frame %d: the reference" % (what, f))
                info = hip.debug_last_ray_temporal()
                assert (info["slabs"], info["depth"], info["history"], info["n"], info["samples"], info["fused"]) == (1, depth, 3, w * h, samples, 1)
                assert info["head"] == (depth - 1 - f) % depth
            rendered = frame_sequence(hip, sc, w, h, samples, bounces, depth, use_filter, hdr, frames)
            for f in range(frames):
                if not use_filter:
                    differ = ~same_floats(got[f], rendered[f]).all(axis=2) & pixels
                    assert not differ.any(), ("%s frame %d: flx_render" % (what, f), np.argwhere(differ)[:8])
                elif name != "cornell":
                    assert compares.all()
                    assert_floats(got[f], rendered[f], "%s frame %d: flx_render" % (what, f))
    temporal = capi.RayTemporal(history=3, temporal_samples=depth, use_filter=1, hdr=1)
    hip.rays_history_reset(3)
    want = sequence(ref, ("camera", name), sc, t, rays, w, h, depth, 1, 1, frames)
    for f in range(2):                                                        # the host call: the same bits
        assert_floats(hip.rays_image_temporal(rays, w, h, seeded(t, f % depth), temporal), want[f], "%s N %d: the host call, frame %d" % (name, depth, f))


# ---- 2. history that does not match ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("use_filter", [0, 1])
def test_history_that_does_not_match(fresh, oracle, scenes, ref, use_filter):
    """the rays change at frame 2 (the camera moved, free rays swapped in for a third of the image), flx_scene_update moves a triangle between frames 3 and 4: the
    reference is given the same state frame by frame"""
    hip = fresh
    sc, p, rays, _, first = camera_rays(oracle, scenes, "cornell")
    w, h = FRAMES["cornell"][:2]
    t = trace_params(p)
    moved_rays = rays.copy()
    moved_rays[:, 0:3] += np.array([0.35, -0.2, 0.15], np.float32)              # the camera moved: the same directions from another place
    moved_rays[::3] = free_rays(oracle, scenes, "cornell")[:len(moved_rays[::3])]
    entry = int(first[len(first) // 2 + 16, 4])                                  # the triangle the centre pixel sees
    g = sc.arrays["geometry"].reshape(-1, 12).copy()
    assert entry >= 0 and g[entry, 10] == 2 and (first[:, 4] == entry).sum() > 10
    g[entry, [1, 4, 7]] += np.float32(500.0)                                      # the triangle leaves, out of every ray's way
    moved_scene = with_geometry(sc, reflatten_by_rule(g))
    states = [("still", sc, rays)] * 2 + [("moved rays", sc, moved_rays)] * 2 + [("moved scene", moved_scene, moved_rays)] * 3
    history = ref.history(w, h, 4)
    hip.update_scene(sc)
    temporal = capi.RayTemporal(history=1, temporal_samples=4, use_filter=use_filter, hdr=1)
    images = []
    for f, (stage, scene, frame_rays) in enumerate(states):
        if f == 4:
            hip.update_scene_rows(entry, g[entry:entry + 1])
        q = seeded(t, f % 4)
        want = history.store(traced(ref, ("mismatch", stage), scene, q, frame_rays, use_filter), use_filter, 1)
        images.append(image_of(hip, on_device(frame_rays), w, h, q, temporal))
        assert_floats(images[f], want, "use_filter %d frame %d (%s)" % (use_filter, f, stage))
    # the states are felt: frames 2 and 4 are not what the unchanged state would have given
    still = sequence(ref, ("mismatch", "still"), sc, t, rays, w, h, 4, use_filter, 1, 5)
    assert not np.array_equal(images[2], still[2]) and not np.array_equal(images[4], still[4])
    hip.update_scene(sc)


# ---- 3. shapes where the indexing can go wrong ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dragon", "theater"])
def test_sizes_slabs_and_groups(fresh, oracle, scenes, ref, name):
    """one partial block (35 rays), 130 rays, 1296 = 20 x 64 + 16; slabs of 64 and 128 rays (the ring index is the ray's index in the image, not in the slab) and one
    workgroup: three-frame sequences equal the default launch's, which equals the reference"""
    hip = fresh
    sc, p, _, _, _ = camera_rays(oracle, scenes, name)
    t = trace_params(p)
    pool = free_rays(oracle, scenes, name)[500:1796]                              # rays from surfaces and rays from free space
    hip.update_scene(sc)
    for w, h in ((7, 5), (13, 10), (48, 27)):
        n = w * h
        rays = pool[::1296 // n][:n]
        d = on_device(rays)
        for use_filter in (0, 1):
            temporal = capi.RayTemporal(history=6, temporal_samples=4, use_filter=use_filter, hdr=1)
            want = sequence(ref, ("shapes", name, n), sc, t, rays, w, h, 4, use_filter, 1, 3)
            for slab, groups in ((0, 0), (64, 0), (128, 0), (0, 1), (64, 1)):
                hip.set_trace_slab(slab)
                hip.set_query_groups(groups)
                hip.rays_history_reset(6)
                for f in range(3):
                    got = image_of(hip, d, w, h, seeded(t, f), temporal)
                    assert_floats(got, want[f], "%s %d x %d use_filter %d slab %d groups %d frame %d" % (name, w, h, use_filter, slab, groups, f))
                    info = hip.debug_last_ray_temporal()
                    assert info["slabs"] == (-(-n // slab) if slab else 1) and (info["n"], info["head"], info["fused"]) == (n, 3 - f, 1)
    assert hip.debug_last_ray_temporal()["slabs"] == 21                           # 1296 rays in slabs of 64: twenty full ones and one of 16


# ---- 4. independence ---------------------------------------------------------------------------------------------------------------------------------------------------------

def test_histories_frames_and_plain_images_do_not_touch_each_other(fresh, oracle, scenes, ref, tmp_path_factory):
    """histories 0 and 7 interleaved with different rays, with a temporal flx_render sequence and with plain flx_rays_image calls: each of the four equals its own
    sequence run alone"""
    hip = fresh
    sc, p, cam, _, _ = camera_rays(oracle, scenes, "theater")
    w, h, samples, bounces, _ = FRAMES["theater"]
    t = trace_params(p)
    free = free_rays(oracle, scenes, "theater")[800:800 + w * h]
    a_want = sequence(ref, ("camera", "theater"), sc, t, cam, w, h, 4, 1, 1, 5)
    b_want = sequence(ref, ("free576", "theater"), sc, t, free, w, h, 3, 0, 0, 5)
    hip.update_scene(sc)
    c_want = frame_sequence(hip, sc, w, h, samples, bounces, 4, 0, 1, 5)
    planes = wanted(planes_reference(tmp_path_factory), ("free576", "theater"), sc, t, free)[0]
    d_want = oracle_chain(oracle, planes, w, h, 1, key=("free576", "theater"))
    ta = capi.RayTemporal(history=0, temporal_samples=4, use_filter=1, hdr=1)
    tb = capi.RayTemporal(history=7, temporal_samples=3, use_filter=0, hdr=0)
    d_cam, d_free = on_device(cam), on_device(free)
    hip.temporal_reset()
    for f in range(5):
        assert_floats(image_of(hip, d_cam, w, h, seeded(t, f % 4), ta), a_want[f], "history 0, frame %d" % f)
        assert_floats(image_of(hip, d_free, w, h, seeded(t, f % 3), tb), b_want[f], "history 7, frame %d" % f)
        q = sc.frame_params(width=w, height=h, samples=samples, max_reflections=bounces, use_filter=0, hdr=1)
        q.is_temporal, q.temporal_samples, q.random_seed = 1, 4, float(f % 4)
        assert_floats(hip.render(q)[0], c_want[f], "flx_render's temporal frame %d" % f)
        plain = hip.ray_image_device(d_free, w, h, t, hdr=1)
        hip.sync()
        assert_floats(plain.cpu().numpy(), d_want, "a plain ray image after frame %d" % f)
    assert not np.array_equal(c_want[0], c_want[1])


# ---- 5. key and reset --------------------------------------------------------------------------------------------------------------------------------------------------------

def test_key_and_reset(fresh, oracle, scenes, ref):
    hip = fresh
    sc, p, rays, _, _ = camera_rays(oracle, scenes, "theater")
    w, h = FRAMES["theater"][:2]
    t = trace_params(p)
    hip.update_scene(sc)
    d = on_device(rays)
    key = ("camera", "theater")
    four = sequence(ref, key, sc, t, rays, w, h, 4, 0, 1, 8)
    other = sequence(ref, key, sc, t, rays, w, h, 4, 1, 0, 8)                     # history 5 carries on all along, through the chain
    fresh5 = sequence(ref, key, sc, t, rays, w, h, 5, 0, 1, 2)
    tall = sequence(ref, key, sc, t, rays, h, w, 4, 0, 1, 2)                      # the same rays as an image of 18 x 32: another key
    counts = {2: 0, 5: 0}

    def frame(history, want, f, depth=4, size=(w, h), use_filter=0, hdr=1, what=""):
        temporal = capi.RayTemporal(history=history, temporal_samples=depth, use_filter=use_filter, hdr=hdr)
        assert_floats(image_of(hip, d, size[0], size[1], seeded(t, f % depth), temporal), want[f], "%s: history %d frame %d" % (what, history, f))
        assert hip.debug_last_ray_temporal()["head"] == (depth - 1 - f) % depth

    def carries_on(what):
        frame(5, other, counts[5], use_filter=1, hdr=0, what=what)
        counts[5] += 1

    frame(2, four, 0, what="fresh"); frame(2, four, 1, what="fresh"); carries_on("beside a fresh history")
    frame(2, fresh5, 0, depth=5, what="another N starts afresh"); frame(2, fresh5, 1, depth=5, what="another N"); carries_on("beside another N")
    frame(2, four, 0, what="back to N = 4: afresh again"); frame(2, four, 1, what="N = 4"); frame(2, four, 2, what="N = 4")
    frame(2, tall, 0, size=(h, w), what="another size starts afresh"); frame(2, tall, 1, size=(h, w), what="another size"); carries_on("beside another size")
    frame(2, four, 0, what="the size back: afresh"); frame(2, four, 1, what="the size back")
    hip.rays_history_reset(2)
    frame(2, four, 0, what="after flx_rays_history_reset(2)"); carries_on("after the reset of another history")
    frame(2, four, 1, what="after the reset"); frame(2, four, 2, what="after the reset"); frame(2, four, 3, what="after the reset"); frame(2, four, 4, what="the ring wraps")
    hip.rays_history_reset(-1)
    frame(2, four, 0, what="after flx_rays_history_reset(-1)")
    counts[5] = 0
    carries_on("after flx_rays_history_reset(-1)")
    carries_on("after flx_rays_history_reset(-1)")
    hip.rays_history_reset(7)                                                    # a history never used
    frame(2, four, 1, what="after the reset of an unused history")
    assert not np.array_equal(four[0], four[1]) and not np.array_equal(other[4], other[5])


# ---- 6. ordering ---------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_an_image_waits_for_the_stream_that_writes_its_rays(fresh, oracle, scenes, ref):
    hip = fresh
    sc, p, rays, _, _ = camera_rays(oracle, scenes, "theater")
    w, h = FRAMES["theater"][:2]
    t = trace_params(p)
    want = sequence(ref, ("camera", "theater"), sc, t, rays, w, h, 4, 1, 1, 2)
    hip.update_scene(sc)
    temporal = capi.RayTemporal(history=4, temporal_samples=4, use_filter=1, hdr=1)
    source = on_device(rays)
    d, e = torch.zeros_like(source), torch.zeros_like(source)
    busy = torch.ones((2048, 2048), device="cuda")
    outs = [poisoned(w * h), poisoned(w * h)]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for f, target in enumerate((d, e)):
            for _ in range(8):
                busy = busy @ busy * 1e-4                           # work in front of the write, so that the rays are not there when the call returns
            target.copy_(source)
            hip.rays_image_temporal(target, w, h, seeded(t, f), temporal, device=True, out=outs[f], stream=side)
    hip.sync()
    for f in range(2):
        assert_floats(outs[f].cpu().numpy().view(np.float32)[:w * h * 4].reshape(h, w, 4), want[f], "rays written on a side stream, frame %d" % f)
    side.synchronize()


def test_a_temporal_image_between_two_frames_of_the_loop(fresh, oracle, scenes, ref):
    hip = fresh
    sc, p, rays, _, _ = camera_rays(oracle, scenes, "dragon")
    w, h = FRAMES["dragon"][:2]
    t = trace_params(p)
    want = sequence(ref, ("camera", "dragon"), sc, t, rays, w, h, 4, 0, 1, 2)
    hip.update_scene(sc)
    temporal = capi.RayTemporal(history=0, temporal_samples=4, use_filter=0, hdr=1)
    params = [sc.frame_params(width=96, height=54, samples=2, max_reflections=4, use_filter=0) for _ in range(2)]
    params[1].random_seed = params[0].random_seed + 1.0
    oracle_frames = [oracle.render(sc, q)[0] for q in params]
    d = on_device(rays)
    outs = [poisoned(w * h), poisoned(w * h)]
    torch.cuda.synchronize()
    for q in params:
        hip.frame_begin(q)
    assert hip.frames_in_flight() == 2
    for f in range(2):
        hip.rays_image_temporal(d, w, h, seeded(t, f), temporal, device=True, out=outs[f])
    frames = [hip.frame_end()[0] for _ in params]
    hip.sync()
    for f in range(2):
        words = outs[f].cpu().numpy().view(np.uint32)
        assert (words[w * h * 4:] == 0xA5A5A5A5).all()
        assert_floats(words[:w * h * 4].view(np.float32).reshape(h, w, 4), want[f], "between two frames, image %d" % f)
    for got, frame in zip(frames, oracle_frames):
        assert_floats(np.asarray(got).reshape(frame.shape), frame, "a frame of the loop")
    assert not np.array_equal(frames[0], frames[1])


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_history_as_it_was(fresh, oracle, scenes, ref):
    hip = fresh
    sc, p, all_rays, _, _ = camera_rays(oracle, scenes, "theater")
    rays_host, t = all_rays[160:416], trace_params(p)                             # 16 x 16 of them
    ok = capi.RayTemporal(history=2, temporal_samples=4, use_filter=1, hdr=1)
    with capi.Context(0) as bare:
        for call, name in ((lambda: bare.rays_image_temporal(rays_host, 16, 16, t, ok), "flx_rays_image_temporal"),
                           (lambda: bare.rays_image_temporal((0, 0), 0, 0, t, None, device=True, out=0), "flx_rays_image_temporal_device")):
            with pytest.raises(capi.FlexLightHipError, match=r"failed \(3\): %s: no scene and transforms uploaded" % name):      # FLX_ERR_NO_SCENE
                call()
        assert bare.debug_last_ray_temporal()["slabs"] == 0
        bare.rays_history_reset(-1)                                              # nothing to release: FLX_OK
    hip.update_scene(sc)
    rays = on_device(rays_host)
    image = poisoned(256)
    both = torch.zeros((2048, 8), dtype=torch.float32, device="cuda")
    host = np.zeros((256, 4), np.float32)
    R, B = rays.data_ptr(), both.data_ptr()

    def with_(**kw):
        q = trace_params(p)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def temporal_(**kw):
        q = capi.RayTemporal(history=2, temporal_samples=4, use_filter=1, hdr=1)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def dev(r, w, h, q, tt, out):
        return lambda: hip.rays_image_temporal(r, w, h, q, tt, device=True, out=out)

    D, Hst = "flx_rays_image_temporal_device: ", "flx_rays_image_temporal: "
    refused = [
        (dev(rays, 16, 16, None, ok, image), D + "params is NULL"),
        (lambda: hip.rays_image_temporal(rays_host, 16, 16, None, ok), Hst + "params is NULL"),
        (dev(rays, 16, 16, with_(samples=0), ok, image), D + "samples is less than 1"),
        (lambda: hip.rays_image_temporal(rays_host, 16, 16, with_(max_reflections=-1), ok), Hst + "max_reflections is negative"),
        (dev(rays, 16, 16, with_(texture_width=0), ok, image), D + "texture_width is less than 1"),
        (dev((R, 0), 0, 16, t, ok, image), D + "width or height is 0"),
        (dev((R, 0), 16, 0, t, ok, image), D + "width or height is 0"),
        (lambda: hip.rays_image_temporal(np.zeros((0, 8), np.float32), 0, 0, t, ok), Hst + "width or height is 0"),
        (dev((R, 1 << 32), 65536, 65536, t, ok, image.data_ptr()), D + "width \\* height is 2\\^32 or more"),
        (dev(rays, 16, 16, t, None, image), D + "temporal is NULL"),
        (lambda: hip.rays_image_temporal(rays_host, 16, 16, t, None), Hst + "temporal is NULL"),
        (dev(rays, 16, 16, t, temporal_(history=8), image), D + "history is not one of 0 \\.\\. 7"),
        (dev(rays, 16, 16, t, temporal_(history=-1), image), D + "history is not one of 0 \\.\\. 7"),
        (lambda: hip.rays_image_temporal(rays_host, 16, 16, t, temporal_(history=1 << 20)), Hst + "history is not one of 0 \\.\\. 7"),
        (dev(rays, 16, 16, t, temporal_(use_filter=2), image), D + "use_filter is neither 0 nor 1"),
        (dev(rays, 16, 16, t, temporal_(use_filter=-1), image), D + "use_filter is neither 0 nor 1"),
        (dev(rays, 16, 16, t, temporal_(hdr=2), image), D + "hdr is neither 0 nor 1"),
        (lambda: hip.rays_image_temporal(rays_host, 16, 16, t, temporal_(hdr=-1)), Hst + "hdr is neither 0 nor 1"),
        (dev((0, 256), 16, 16, t, ok, image), D + "an array is NULL"),
        (dev(rays, 16, 16, t, ok, 0), D + "an array is NULL"),
        (dev((host.ctypes.data, 256), 16, 16, t, ok, image), D + "the rays are not width \\* height rows in memory of the context's device"),
        (dev(rays, 16, 16, t, ok, host.ctypes.data), D + "the image is not width \\* height float4 in memory of the context's device"),
        (dev((R + 4, 255), 15, 17, t, ok, image), D + "the rays are not width \\* height rows in memory of the context's device, 16-byte aligned"),
        (dev(rays, 16, 16, t, ok, image.data_ptr() + 8), D + "the image is not width \\* height float4 in memory of the context's device, 16-byte aligned"),
        (dev((R, 1 << 28), 1 << 14, 1 << 14, t, ok, image.data_ptr()), D + "the rays are not width \\* height rows"),            # 8 GB: the allocation ends first
        (dev((B, 256), 16, 16, t, ok, B), D + "the rays and an output overlap"),
        (dev((B, 256), 16, 16, t, ok, B + 255 * 32), D + "the rays and an output overlap"),
        (lambda: hip.rays_history_reset(-2), "flx_rays_history_reset: history is not one of -1 \\.\\. 7"),
        (lambda: hip.rays_history_reset(8), "flx_rays_history_reset: history is not one of -1 \\.\\. 7"),
    ]
    want = sequence(ref, ("camera256", "theater"), sc, t, rays_host, 16, 16, 4, 1, 1, len(refused) + 2)
    assert_floats(image_of(hip, rays, 16, 16, seeded(t, 0), ok), want[0], "frame 0")
    messages = set()
    for k, (call, message) in enumerate(refused):
        before = hip.debug_last_ray_temporal()
        with pytest.raises(capi.FlexLightHipError, match=r"failed \(1\): " + message) as caught:
            call()
        messages.add(str(caught.value))
        assert hip.debug_last_ray_temporal() == before, message                   # nothing was enqueued
        f = k + 1                                                                 # the history is what it was: neither rotated nor re-keyed
        assert_floats(image_of(hip, rays, 16, 16, seeded(t, f % 4), ok), want[f], "the frame after the refusal '%s'" % message)
    assert len(messages) >= 20                                      # every refusal says it in words of its own (the same rule refused twice says them twice)
    torch.cuda.synchronize()
    assert (image == 0xA5).all() and not both.any()
    hip.rays_image_temporal((B, 256), 16, 16, seeded(t, 0), capi.RayTemporal(history=0, temporal_samples=4, use_filter=0, hdr=0), device=True, out=B + 256 * 32)
    hip.sync()                                                      # side by side in one allocation: no overlap
