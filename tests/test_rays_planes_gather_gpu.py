"""Ray images with a volume on the GPU (flx_rays_planes_gather, flx_rays_image[_temporal]_gather, flx_camera_image[_temporal]_gather and their _device calls:
csrc/flx_rays_planes_gather.hip) against the CPU reference (tests/rays_planes_gather_ref, which test_rays_planes_gather_cpu.py pins): every row of every plane, bit
for bit, a NaN equal to a NaN.  The rays are a 40 x 27 pinhole image (1080 rays: 16 blocks of 64 and a ragged one) and seven rays that miss; the volumes are 4 x 3 x
4 probes with face size 4, baked on the device, copied down once and handed to both sides as the same floats: the bake is not under test."""
import numpy as np
import pytest
import torch

import rays_temporal_util
from flexlight_hip import capi
from flexlight_hip.scene_io import FrameParams
from rays_planes_gather_util import (GAIN, HEIGHT, TEMPORAL_CANVAS, TEMPORAL_FILTER, WIDTH, assert_floats, assert_texels, batch, half_grid, inactive_offsets, quant,
                                     reference, same_floats, trace_params, wanted)
from volume_map_util import map_of
from volume_relocate_util import relocate_of

pytestmark = pytest.mark.gpu

SCENES = ("cornell", "dragon")            # the lockstep walk; no lockstep copy
FORMS = ("plain", "map", "offsets", "map_offsets")
FACE, MAP = 4, 4
N = WIDTH * HEIGHT
# samples, max_reflections, the planes asked for: samples 1, 2, 8 x bounces 0, 1, 2, 4 x planes8 only, planes32 only, both — every value, each pair of values once
CASES = ((1, 0, "both"), (2, 1, "planes8"), (8, 2, "planes32"), (1, 4, "planes32"), (2, 2, "both"), (8, 4, "planes8"), (1, 1, "both"), (8, 0, "planes8"), (2, 4, "planes32"),
         (1, 2, "planes8"), (2, 0, "planes32"), (8, 1, "both"))

_volumes = {}


@pytest.fixture(scope="module")
def ref(tmp_path_factory, oracle):
    return reference(tmp_path_factory)


def on_device(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def volume(hip, oracle, scenes, name):
    """the scene uploaded; -> (scene, rays [1087, 8], grid, {form: (vmap, sh, maps, offsets) as host arrays}), baked once per scene over the lower half of its hit
    points: the map forms with a map of size 4, the offset forms after one relocation pass from the lattice, its distances in the scene's units"""
    sc, rays, points = batch(oracle, scenes, name)
    hip.update_scene(sc)
    grid = half_grid(points)
    if name not in _volumes:
        vmap = map_of(MAP, 3)
        t, probe = trace_params(sc, 1, 2), capi.ProbeParams(FACE)
        down = lambda x: x.detach().cpu().numpy().copy()      # noqa: E731
        sh, maps = hip.volume_bake_map_device(grid, t, probe, vmap)
        offsets = torch.zeros((grid.probes, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        extent = float((points.max(axis=0) - points.min(axis=0)).max())      # in the scene's own units: a probe that sees a front face anywhere in the scene stays active
        hip.volume_relocate_device(grid, relocate_of(min_front=0.1 * min(grid.spacing[:]), reach=4.0 * extent), FACE, offsets, t.texture_width)
        sh_moved, maps_moved = hip.volume_bake_relocated_device(grid, t, probe, offsets, vmap)
        hip.sync()
        sh, maps, offsets, sh_moved, maps_moved = down(sh), down(maps), down(offsets), down(sh_moved), down(maps_moved)
        assert np.isfinite(offsets[:, 0:3]).all() and ((offsets.view(np.uint32)[:, 3] & capi.RELOCATE_INACTIVE) == 0).any()
        _volumes[name] = {"plain": (None, sh, None, None), "map": (vmap, sh, maps, None), "offsets": (None, sh_moved, None, offsets),
                          "map_offsets": (vmap, sh_moved, maps_moved, offsets)}
    return sc, rays, grid, _volumes[name]


def resident(hip, grid, form, gain=GAIN, reserved=0):
    """a form's arrays on the device -> (the GatherVolume over them, the tensors and their copies for the read-only check)"""
    vmap, sh, maps, offsets = form
    arrays = [on_device(sh), on_device(maps), on_device(offsets)]
    return hip.gather_volume(grid, arrays[0], vmap, arrays[1], arrays[2], gain, reserved), [(a, a.clone()) for a in arrays if a is not None]


def unchanged(pairs):
    return all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in pairs)      # (as words: a dead probe's rows are NaN)


def poisoned(rows, row_bytes):
    return torch.full((rows + 8, row_bytes), 0xA5, dtype=torch.uint8, device="cuda")


def gathered(hip, rays, t, grid, form, which="both", n=None, gain=GAIN, stream=None):
    """rays (numpy) through ray_planes_gather_device into poisoned buffers with eight rows behind the last -> (planes8 uint32 [5, n] or None, planes32 float32 [5, n, 4]
    or None); nothing beyond the planes is written, the inputs are read only"""
    d = on_device(rays[:n] if n is not None else rays)
    n = d.shape[0]
    vol, pairs = resident(hip, grid, form, gain)
    pairs.append((d, d.clone()))
    out8 = poisoned(5 * n, 4) if which != "planes32" else None
    out32 = poisoned(5 * n, 16) if which != "planes8" else None
    torch.cuda.synchronize()
    hip.ray_planes_gather_device(d, t, vol, out8, out32, stream)
    hip.sync()
    got8 = got32 = None
    if out8 is not None:
        words = out8.cpu().numpy().view(np.uint32).reshape(-1)
        assert (words[5 * n:] == 0xA5A5A5A5).all()
        got8 = words[:5 * n].reshape(5, n)
    if out32 is not None:
        words = out32.cpu().numpy().view(np.uint32).reshape(-1, 4)
        assert (words[5 * n:] == 0xA5A5A5A5).all()
        got32 = words[:5 * n].view(np.float32).reshape(5, n, 4)
    assert unchanged(pairs)
    return got8, got32


def expected(ref, key, sc, t, rays, grid, form, gain=GAIN, mode=0):
    vmap, sh, maps, offsets = form
    return wanted(key, lambda: ref.planes(sc, t, rays, grid, sh, gain, vmap=vmap, maps=maps, offsets=offsets, mode=mode))


def assert_planes(got8, got32, want, what, n=None):
    want = want[:, :n] if n is not None else want
    if got32 is not None:
        assert_floats(got32, want, what + " planes32")
    if got8 is not None:
        assert_texels(got8, quant(want), what + " planes8")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", SCENES)
def test_every_form_equals_its_reference(hip, oracle, scenes, ref, name, form):
    """the image's rays and the rays that miss, over CASES"""
    sc, rays, grid, forms = volume(hip, oracle, scenes, name)
    for samples, bounces, which in CASES:
        t = trace_params(sc, samples, bounces)
        want, hit = expected(ref, (name, form, samples, bounces), sc, t, rays, grid, forms[form])
        what = "%s %s S %d K %d %s" % (name, form, samples, bounces, which)
        got8, got32 = gathered(hip, rays, t, grid, forms[form], which)
        assert (got8 is not None) == (which != "planes32") and (got32 is not None) == (which != "planes8")
        assert_planes(got8, got32, want, what)
        assert hit[:N].sum() > N // 2 and not hit[N:].any()
        if (samples, bounces) == (2, 2):      # the baked volume is no no-op on these rays: a quarter of the rows that hit differ from the constant ambient's
            vmap, sh, maps, _ = forms[form]
            constant, _ = expected(ref, (name, form, "constant"), sc, t, rays, grid, (vmap, sh, maps, inactive_offsets(grid.probes)))
            assert (~same_floats(want[0:2], constant[0:2])).any(axis=(0, 2))[hit].mean() >= 0.25
    info = hip.last_planes_gather()
    assert (info["n"], info["slabs"], info["slab"], info["flags"], info["mode"], info["samples"]) == (len(rays), 1, 1 << 21, FORMS.index(form), 0, CASES[-1][0])
    assert info["lockstep"] == hip.last_ray_planes()["lockstep"] and info["groups"] == (((len(rays) + 63) // 64) + 3) // 4
    assert (info["lockstep"] == 1) == (name == "cornell")


@pytest.mark.parametrize("name", SCENES)
def test_a_high_threshold_and_a_gain_of_zero(hip, oracle, scenes, ref, name):
    """min_importancy > 1: no sample has a last point; min_importancy 0.8: samples end on the loop guard; gain 0: a lit sample adds nothing"""
    sc, rays, grid, forms = volume(hip, oracle, scenes, name)
    for importancy, gain in ((1.5, GAIN), (0.8, GAIN), (None, 0.0)):
        t = trace_params(sc, 2, 3, importancy)
        want, _ = expected(ref, (name, "map_offsets", 2, 3, importancy, gain), sc, t, rays, grid, forms["map_offsets"], gain)
        got8, got32 = gathered(hip, rays, t, grid, forms["map_offsets"], gain=gain)
        assert_planes(got8, got32, want, "%s min %s gain %s" % (name, importancy, gain))


@pytest.mark.parametrize("name", SCENES)
def test_seams(hip, oracle, scenes, ref, name):
    """n = 1, 63, 64, 65 and 1080; slabs of 64 rays; one workgroup and the full grid"""
    sc, rays, grid, forms = volume(hip, oracle, scenes, name)
    t, form = trace_params(sc, 2, 2), forms["map_offsets"]
    want, _ = expected(ref, (name, "map_offsets", 2, 2), sc, t, rays, grid, form)
    try:
        for groups in (1, 0, ((N + 63) // 64 + 3) // 4):
            hip.set_query_groups(groups)
            for n in (1, 63, 64, 65, N):
                got8, got32 = gathered(hip, rays, t, grid, form, n=n)
                assert_planes(got8, got32, want, "%s n %d groups %d" % (name, n, groups), n)
                info = hip.last_planes_gather()
                assert (info["n"], info["slabs"]) == (n, 1) and info["groups"] == (groups if groups else ((n + 63) // 64 + 3) // 4)
            hip.set_trace_slab(64)
            got8, got32 = gathered(hip, rays, t, grid, form)
            assert_planes(got8, got32, want, "%s slabs of 64, groups %d" % (name, groups))
            info = hip.last_planes_gather()
            assert (info["n"], info["slabs"], info["slab"]) == (len(rays), (len(rays) + 63) // 64, 64)
            hip.set_trace_slab(0)
    finally:
        hip.set_query_groups(0)
        hip.set_trace_slab(0)


@pytest.mark.parametrize("name", SCENES)
def test_an_inactive_volume_is_the_plain_call(hip, oracle, scenes, ref, name):
    """every probe inactive: flx_rays_planes_device's own output, device against device"""
    sc, rays, grid, forms = volume(hip, oracle, scenes, name)
    d = on_device(rays)
    for samples, bounces in ((1, 1), (3, 4), (2, 0)):
        t = trace_params(sc, samples, bounces)
        plain8, plain32 = hip.ray_planes_device(d, t, True, True)
        hip.sync()
        for form in ("plain", "map"):
            vmap, sh, maps, _ = forms[form]
            got8, got32 = gathered(hip, rays, t, grid, (vmap, sh, maps, inactive_offsets(grid.probes)))
            assert_texels(got8, plain8.cpu().numpy().view(np.uint32), "%s S %d K %d" % (name, samples, bounces))
            assert_floats(got32, plain32.cpu().numpy(), "%s S %d K %d" % (name, samples, bounces))


def image_params(hdr):
    p = FrameParams()
    p.width, p.height, p.hdr = WIDTH, HEIGHT, int(hdr)
    return p


@pytest.mark.parametrize("name", SCENES)
def test_an_image_is_the_chain_over_the_planes(hip, oracle, scenes, ref, name):
    """flx_rays_image_gather_device equals flx_filter_planes_device over the planes call's planes8; the host call and the camera calls equal it"""
    sc, rays, grid, forms = volume(hip, oracle, scenes, name)
    t, form = trace_params(sc, 2, 2), forms["map"]
    d = on_device(rays[:N])
    vol, pairs = resident(hip, grid, form)
    want, _ = expected(ref, (name, "map", 2, 2), sc, t, rays, grid, form)
    for hdr in (1, 0):
        planes8, _ = hip.ray_planes_gather_device(d, t, vol, True, None)
        chained = torch.empty((HEIGHT, WIDTH, 4), dtype=torch.float32, device="cuda")
        hip.filter_planes_device(image_params(hdr), planes8.data_ptr(), chained.data_ptr())
        out = poisoned(N, 16)
        hip.ray_image_gather_device(d, WIDTH, HEIGHT, t, vol, hdr, out)
        hip.sync()
        assert_texels(planes8.cpu().numpy().view(np.uint32), quant(want[:, :N]), name)
        image = out.cpu().numpy().view(np.float32).reshape(-1, 4)
        assert (image[N:].view(np.uint32) == 0xA5A5A5A5).all()
        image = image[:N].reshape(HEIGHT, WIDTH, 4)
        assert_floats(image, chained.cpu().numpy(), "%s hdr %d" % (name, hdr))
        assert np.isfinite(image).all() and (image[:, :, 0:3] > 0.0).any()
        assert_floats(hip.ray_image_gather(rays[:N], WIDTH, HEIGHT, t, vol, hdr), image, "%s host hdr %d" % (name, hdr))
        info = hip.last_planes_gather()
        assert (info["n"], info["slabs"], info["flags"], info["mode"]) == (N, 1, 1, 0)
    # the camera calls: flx_camera_rays_device's rays, which are the image's
    camera = capi.Camera.pinhole(sc.frame_params(width=WIDTH, height=HEIGHT, samples=1, max_reflections=1, use_filter=1))
    made = hip.camera_rays_device(camera, WIDTH, HEIGHT)
    want_image = hip.ray_image_gather_device(made, WIDTH, HEIGHT, t, vol, 1)
    got_image = hip.camera_image_gather_device(camera, WIDTH, HEIGHT, t, vol, 1)
    hip.sync()
    assert_floats(got_image.cpu().numpy(), want_image.cpu().numpy(), name + " camera")
    assert_floats(hip.camera_image_gather(camera, WIDTH, HEIGHT, t, vol, 1), want_image.cpu().numpy(), name + " camera, host")
    assert np.array_equal(made.cpu().numpy().view(np.uint32), rays[:N].view(np.uint32))
    assert unchanged(pairs)


@pytest.mark.parametrize("use_filter", (1, 0))
@pytest.mark.parametrize("name", SCENES)
def test_three_temporal_frames(hip, oracle, scenes, ref, tmp_path_factory, name, use_filter):
    """three frames with rotating seeds on a fresh history: tests/rays_temporal_ref's pass over the reference's six planes, with the filter and with the canvas; the
    host call and the camera calls on histories of their own give the same frames"""
    temporal_ref = rays_temporal_util.reference(tmp_path_factory)
    sc, rays, grid, forms = volume(hip, oracle, scenes, name)
    form, depth, hdr = forms["offsets"], 3, 1
    image_rays = rays[:N]
    d = on_device(image_rays)
    vol, pairs = resident(hip, grid, form)
    camera = capi.Camera.pinhole(sc.frame_params(width=WIDTH, height=HEIGHT, samples=1, max_reflections=1, use_filter=1))
    history = temporal_ref.history(WIDTH, HEIGHT, depth)
    mode = TEMPORAL_FILTER if use_filter else TEMPORAL_CANVAS
    for h in range(4):
        hip.rays_history_reset(h)
    for frame in range(3):
        t = trace_params(sc, 2, 2, seed=frame % depth)
        six, _ = expected(ref, (name, "offsets", 2, 2, "temporal", mode, frame), sc, t, image_rays, grid, form, mode=mode)
        want = history.store(quant(six), use_filter, hdr)
        out = poisoned(N, 16)
        hip.rays_image_temporal_gather(d, WIDTH, HEIGHT, t, capi.RayTemporal(0, depth, use_filter, hdr), vol, device=True, out=out)
        hip.sync()
        got = out.cpu().numpy().view(np.float32).reshape(-1, 4)
        assert (got[N:].view(np.uint32) == 0xA5A5A5A5).all()
        got = got[:N].reshape(HEIGHT, WIDTH, 4)
        assert_floats(got, want, "%s filter %d frame %d" % (name, use_filter, frame))
        info, plain = hip.last_planes_gather(), hip.debug_last_ray_temporal()
        assert (info["n"], info["slabs"], info["mode"], info["flags"], info["samples"]) == (N, 1, mode, 2, 2)
        assert (plain["history"], plain["depth"], plain["n"], plain["fused"]) == (0, depth, N, 1)
        assert_floats(hip.rays_image_temporal_gather(image_rays, WIDTH, HEIGHT, t, capi.RayTemporal(1, depth, use_filter, hdr), vol), want, "host, frame %d" % frame)
        by_camera = hip.camera_image_temporal_gather_device(camera, WIDTH, HEIGHT, t, capi.RayTemporal(2, depth, use_filter, hdr), vol)
        hip.sync()
        assert_floats(by_camera.cpu().numpy(), want, "camera, frame %d" % frame)
        assert_floats(hip.camera_image_temporal_gather(camera, WIDTH, HEIGHT, t, capi.RayTemporal(3, depth, use_filter, hdr), vol), want, "camera, host, frame %d" % frame)
    assert unchanged(pairs)
    for h in range(4):
        hip.rays_history_reset(h)


def test_the_host_planes_call_and_a_producer_stream(hip, oracle, scenes, ref):
    """host rays with the volume's arrays on the device, planes8 alone and both; rays written on another stream; the same call twice; n == 0"""
    sc, rays, grid, forms = volume(hip, oracle, scenes, "dragon")
    t = trace_params(sc, 2, 2)
    for name in FORMS:
        want, _ = expected(ref, ("dragon", name, 2, 2), sc, t, rays, grid, forms[name])
        vol, pairs = resident(hip, grid, forms[name])
        got8, got32 = hip.ray_planes_gather(rays, t, vol, floats=True)
        assert_planes(got8, got32, want, "host " + name)
        assert_texels(hip.ray_planes_gather(rays, t, vol), quant(want), "host, planes8 alone, " + name)
        assert unchanged(pairs)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        made = torch.from_numpy(rays).cuda(non_blocking=False) * 1.0      # written on the side stream
    torch.cuda.current_stream().synchronize()
    vol, pairs = resident(hip, grid, forms["map"])
    want, _ = expected(ref, ("dragon", "map", 2, 2), sc, t, rays, grid, forms["map"])
    for _ in range(2):                                                    # the scratch is reused
        out8, out32 = hip.ray_planes_gather_device(made, t, vol, True, True, side)
        hip.sync()
        assert_planes(out8.cpu().numpy().view(np.uint32), out32.cpu().numpy(), want, "producer stream")
    before = hip.last_planes_gather()
    assert hip.ray_planes_gather_device((0, 0), t, vol, 0, 0) == (0, 0)   # n == 0: nothing is looked at but the scene and the params
    assert hip.ray_planes_gather(np.zeros((0, 8), np.float32), t, vol).shape == (5, 0)
    assert hip.last_planes_gather() == before


def test_refusals(hip, oracle, scenes, ref):
    """every refusal in order — the sibling's own under the new call's name, then the volume's in flx_rays_trace_gather's words, then the overlap —, each with its
    status and message, nothing written, nothing recorded, the history what it was"""
    sc, rays_host, grid, forms = volume(hip, oracle, scenes, "cornell")
    t = trace_params(sc, 1, 1)
    vmap, sh_host, maps_host, offsets_host = forms["map_offsets"]
    n, w, h = 256, 16, 16
    rays_host = rays_host[:n]
    rays, sh, maps, offsets = on_device(rays_host), on_device(sh_host), on_device(maps_host), on_device(offsets_host)
    out8, out32, image = poisoned(5 * n, 4), poisoned(5 * n, 16), poisoned(n, 16)
    host = np.zeros((5 * n, 4), np.float32)
    camera = capi.Camera.pinhole(sc.frame_params(width=w, height=h, samples=1, max_reflections=1, use_filter=1))
    temporal = capi.RayTemporal(5, 3, 1, 1)
    good = hip.gather_volume(grid, sh, vmap, maps, offsets)
    torch.cuda.synchronize()
    with capi.Context(0) as fresh:
        with pytest.raises(capi.FlexLightHipError, match=r"failed \(3\): flx_rays_planes_gather_device: no scene and transforms uploaded"):
            fresh.ray_planes_gather_device(rays, t, good, out8)
        with pytest.raises(capi.FlexLightHipError, match=r"failed \(3\): flx_camera_image_gather_device: no scene and transforms uploaded"):
            fresh.camera_image_gather_device(camera, w, h, t, good, out=image)
        assert fresh.last_planes_gather()["slabs"] == 0
    hip.rays_history_reset(5)
    hip.rays_image_temporal_gather(rays, w, h, t, temporal, good, device=True)
    hip.sync()
    before, history_before = hip.last_planes_gather(), hip.debug_last_ray_temporal()

    def with_(**kw):
        q = trace_params(sc, 1, 1)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def grid_with(**kw):
        g = half_grid(batch(oracle, scenes, "cornell")[2])
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    def vol(g=grid, s=sh.data_ptr(), m=vmap, d=maps.data_ptr(), f=offsets.data_ptr(), gain=GAIN, reserved=0):      # (addresses: the library judges them, not the binding)
        return hip.gather_volume(g, s, m, d, f, gain, reserved)

    def planes(v=good, params=t, r=rays, o8=out8, o32=out32):
        return lambda: hip.ray_planes_gather_device(r, params, v, o8, o32)

    def picture(v=good, params=t, r=rays, o=image, width=w, height=h):
        return lambda: hip.ray_image_gather_device(r, width, height, params, v, 1, o)

    def over_time(v=good, params=t, r=rays, o=image, tt=temporal):
        return lambda: hip.rays_image_temporal_gather(r, w, h, params, tt, v, device=True, out=o)

    both = torch.zeros((2048, 8), dtype=torch.float32, device="cuda")
    big = torch.zeros((grid.probes * 16 + 5 * n * 2, 4), dtype=torch.float32, device="cuda")      # room for the maps, then for the float planes
    B, R = both.data_ptr(), rays.data_ptr()
    P, I, T, C, CT = ("flx_rays_planes_gather_device: ", "flx_rays_image_gather_device: ", "flx_rays_image_temporal_gather_device: ", "flx_camera_image_gather_device: ",
                      "flx_camera_image_temporal_gather_device: ")
    overlap = "an array of the volume overlaps the rays, a plane output or the image"
    refused = [
        # 1. the sibling's own, under the new call's name — each before a volume that would be refused too
        (planes(None, params=None), P + "params is NULL"),
        (planes(None, params=with_(samples=0)), P + "samples is less than 1"),
        (planes(None, params=with_(max_reflections=-1), r=(0, 0), o8=0, o32=0), P + "max_reflections is negative"),      # for n == 0 too
        (picture(None, params=with_(texture_width=0)), I + "texture_width is less than 1"),
        (planes(None, o8=0, o32=0), P + "planes8 and planes32 are both NULL"),
        (picture(None, r=(R, 0), width=0), I + "width or height is 0"),
        (over_time(None, tt=None), T + "temporal is NULL"),
        (over_time(None, tt=capi.RayTemporal(8, 3, 1, 1)), T + "history is not one of 0 .. 7"),
        (over_time(None, tt=capi.RayTemporal(0, 3, 2, 1)), T + "use_filter is neither 0 nor 1"),
        (planes(None, r=(0, n)), P + "an array is NULL"),
        (picture(None, o=0), I + "an array is NULL"),
        (planes(None, r=(host.ctypes.data, n)), P + "the rays are not n rows in memory of the context's device"),
        (planes(None, o8=out8.data_ptr() + 4), P + "planes8 is not 5 n texels in memory of the context's device, 16-byte aligned"),
        (planes(None, o32=host.ctypes.data), P + "planes32 is not 5 n rows in memory of the context's device"),
        (picture(None, o=image.data_ptr() + 8), I + "the image is not width \\* height float4 in memory of the context's device, 16-byte aligned"),
        (planes(None, r=(B, n), o8=B), P + "the rays and an output overlap"),
        (planes(None, o8=B, o32=B), P + "planes8 and planes32 overlap"),
        (over_time(None, r=(B, n), o=B + 255 * 32), T + "the rays and an output overlap"),
        (lambda: hip.camera_image_gather_device(None, w, h, t, None, out=image), C + "cameras is NULL or n_cameras is 0"),
        (lambda: hip.camera_image_gather_device(camera, w, h, t, None, out=0), C + "the image is NULL"),
        (lambda: hip.camera_image_temporal_gather_device(camera, w, h, t, temporal, None, out=host.ctypes.data), CT + "the image is not width \\* height float4"),
        # 2. the volume: NULL, its grid, its map, its arrays, then its own words, in flx_rays_trace_gather's words
        (planes(None), P + "the volume is NULL"),
        (picture(None), I + "the volume is NULL"),
        (over_time(None), T + "the volume is NULL"),
        (lambda: hip.camera_image_gather_device(camera, w, h, t, None, out=image), C + "the volume is NULL"),
        (lambda: hip.camera_image_temporal_gather_device(camera, w, h, t, temporal, None, out=image), CT + "the volume is NULL"),
        (planes(vol(g=None)), P + "the grid is NULL"),
        (planes(vol(g=grid_with(count=(4, 0, 4)))), P + "a count of the grid is 0"),
        (picture(vol(g=grid_with(spacing=(1.0, -1.0, 1.0)))), I + "a spacing is not greater than 0"),
        (over_time(vol(g=grid_with(flags=2))), T + "flags has a bit beyond FLX_VOLUME_VISIBILITY"),
        (planes(vol(g=grid_with(reserved=1))), P + "reserved is not 0"),
        (planes(vol(m=capi.VolumeMap(17, 3))), P + "the map's size is not one of 1 .. 16"),
        (picture(vol(m=capi.VolumeMap(4, 9))), I + "the map's sharpness is above 8"),
        (planes(vol(s=None)), P + "an array is NULL"),
        (planes(vol(s=sh_host.ctypes.data)), P + "the SH rows are not nx \\* ny \\* nz rows of 144 bytes in memory of the context's device"),
        (picture(vol(s=sh.data_ptr() + 4)), I + "the SH rows are not nx \\* ny \\* nz rows of 144 bytes in memory of the context's device, 16-byte aligned"),
        (planes(vol(d=maps_host.ctypes.data)), P + "the maps are not n_probes \\* size \\* size rows of 16 bytes in memory of the context's device"),
        (planes(vol(s=big.data_ptr(), d=big.data_ptr() + 16)), P + "the maps overlap another array"),
        (over_time(vol(f=offsets_host.ctypes.data)), T + "the offsets are not nx \\* ny \\* nz rows of 16 bytes"),
        (planes(vol(f=sh.data_ptr() + 144)), P + "the arrays overlap"),
        (planes(vol(gain=-1.0, reserved=1, d=None)), P + "gain is negative or not finite"),                                   # the gain before the reserved word and the pair
        (picture(vol(gain=float("inf"))), I + "gain is negative or not finite"),
        (over_time(vol(gain=float("nan"))), T + "gain is negative or not finite"),
        (planes(vol(reserved=1, d=None)), P + "the volume's reserved word is not 0"),                                         # the reserved word before the pair
        (planes(vol(d=None)), P + "map and maps are not both given or both NULL"),
        (picture(vol(m=None)), I + "map and maps are not both given or both NULL"),
        (lambda: hip.camera_image_gather_device(camera, w, h, t, vol(gain=-2.0), out=image), C + "gain is negative or not finite"),
        (lambda: hip.camera_image_temporal_gather_device(camera, w, h, t, temporal, vol(reserved=9), out=image), CT + "the volume's reserved word is not 0"),
        (planes(vol(gain=-1.0, f=rays.data_ptr())), P + "gain is negative or not finite"),                                    # the gain before the overlap
        # 3. an array of the volume that overlaps the rays, a plane output or the image
        (planes(vol(f=rays.data_ptr())), P + overlap),
        (planes(vol(s=both.data_ptr()), r=(B + grid.probes * 144 - 16, n)), P + overlap),
        (planes(vol(d=big.data_ptr()), o8=None, o32=big.data_ptr() + grid.probes * 256 - 16), P + overlap),
        (planes(vol(d=big.data_ptr()), o8=big.data_ptr() + grid.probes * 256 - 16, o32=None), P + overlap),
        (picture(vol(d=big.data_ptr()), o=big.data_ptr() + grid.probes * 256 - 16), I + overlap),
        (over_time(vol(s=both.data_ptr()), r=(B + grid.probes * 144 - 16, n)), T + overlap),
        (lambda: hip.camera_image_gather_device(camera, w, h, t, vol(d=big.data_ptr()), out=big.data_ptr() + grid.probes * 256 - 16), C + overlap),
        # the host calls, under their own names: host rays, the volume's arrays on the device
        (lambda: hip.ray_planes_gather(rays_host, None, good), "flx_rays_planes_gather: params is NULL"),
        (lambda: hip.ray_planes_gather(rays_host, t, None), "flx_rays_planes_gather: the volume is NULL"),
        (lambda: hip.ray_planes_gather(rays_host, t, vol(s=sh_host.ctypes.data)), "flx_rays_planes_gather: the SH rows are not nx \\* ny \\* nz rows of 144 bytes in memory"),
        (lambda: hip.ray_image_gather(rays_host, w, h, t, vol(gain=-0.5)), "flx_rays_image_gather: gain is negative or not finite"),
        (lambda: hip.rays_image_temporal_gather(rays_host, w, h, t, temporal, vol(d=None)), "flx_rays_image_temporal_gather: map and maps are not both given or both NULL"),
        (lambda: hip.camera_image_gather(camera, w, h, t, vol(g=grid_with(floor=2.0))), "flx_camera_image_gather: floor is not one of 0 .. 1"),
        (lambda: hip.camera_image_temporal_gather(camera, w, h, t, temporal, vol(reserved=5)), "flx_camera_image_temporal_gather: the volume's reserved word is not 0"),
    ]
    for k, (call, message) in enumerate(refused):
        with pytest.raises(capi.FlexLightHipError, match=r"failed \(1\): " + message):
            call()
    hip.sync()
    for out in (out8, out32, image):
        assert (out.cpu().numpy() == 0xA5).all()                                   # nothing was enqueued
    assert hip.last_planes_gather() == before and hip.debug_last_ray_temporal() == history_before      # ... nor recorded, and the history was not rotated
    # the accepted borders: gain 0 and the largest gain
    for gain in (0.0, float(np.finfo(np.float32).max)):
        hip.ray_planes_gather_device(rays, t, vol(gain=gain), out8, out32)
    hip.sync()
    assert (out32.cpu().numpy().view(np.float32).reshape(-1, 4)[:n, 3] == 1.0).any()
    hip.rays_history_reset(5)
