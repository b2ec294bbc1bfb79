"""Surface rows on the GPU (flx_rays_surface, flx_frame_surface and their _device forms: csrc/flx_surface.hip) against the CPU reference (tests/surface_ref, which
calls the oracle's own rayTracer / primary_hit and executes lightTrace's first statements; tests/test_surface_ref_cpu.py holds it against the oracle's frames):
every word of every row of every plane.  The reference's floats are all finite on these inputs, so equal values have equal words."""
import copy

import numpy as np
import pytest
import torch

import textures_util as tu
from flexlight_hip import capi
from rays_trace_util import camera_rays, free_rays
from scene_update_util import reflatten_by_rule, with_geometry
from surface_util import ALBEDO, ALL, BITS, FRAMES, HIT, NORMAL, UV, assert_planes, frame_wanted, planes_of, reference, surface_params, wanted, words_of

pytestmark = pytest.mark.gpu

GUARD = 256
MISS_HIT = np.array([0, 0, 0, 0xffffffff], np.uint32)


@pytest.fixture(scope="module")
def ref(tmp_path_factory, oracle):
    return reference(tmp_path_factory)


def guarded(n, fields):
    """the output of a device call: the planes' bytes and 256 guard bytes behind them, all 0xA5"""
    return torch.full((capi.surface_planes(fields) * n * 16 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")


def planes_in(out, n, fields):
    """-> words [planes, n, 4] of a guarded output whose guard bytes kept their pattern"""
    raw = out.cpu().numpy()
    size = capi.surface_planes(fields) * n * 16
    assert (raw[size:] == 0xA5).all(), "the guard bytes behind popcount(fields) * n * 16 were written"
    return raw[:size].view(np.uint32).reshape(capi.surface_planes(fields), n, 4)


def surfaced(hip, rays, tw, fields=ALL, stream=None):
    """rays (numpy [n, 8]) through surface_rays_device into a guarded buffer -> words [planes, n, 4]; the rays are read only"""
    d = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
    keep = d.clone()
    out = guarded(d.shape[0], fields)
    torch.cuda.synchronize()
    assert hip.surface_rays_device(d, fields, tw, out, stream) is out
    hip.sync()
    assert torch.equal(d, keep)
    return planes_in(out, d.shape[0], fields)


def free_wanted(ref, oracle, scenes, name):
    sc = scenes(name)
    rays = free_rays(oracle, scenes, name)
    tw = int(sc.meta["textureWidth"])
    return sc, rays, tw, wanted(("free", name), lambda: ref.rays(sc, rays, tw))


# ---- 1. frames -----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,size", [(n, FRAMES[n]) for n in sorted(FRAMES)] + [("cornell", (13, 7))])
def test_a_frames_planes_equal_the_reference(hip, scenes, ref, name, size):
    """13 x 7: neither dimension is a multiple of the 8 x 8 screen tile"""
    sc, p, want = frame_wanted(ref, scenes, name, size)
    hip.update_scene(sc)
    got = words_of(hip.frame_surface(p, ALL))
    assert_planes(got, want, "%s %dx%d" % ((name,) + size))
    info = hip.last_surface()
    assert (info["slabs"], info["n"], info["fields"], info["frame"]) == (1, size[0] * size[1], ALL, 1)
    alpha = hip.render(p)[0].reshape(-1, 4)[:, 3]
    entry = got[HIT, :, 3].view(np.int32)
    assert np.array_equal(entry >= 0, alpha == 1.0) and (entry >= -1).all() and (entry >= 0).any()
    q = surface_params(sc, *size)
    q.tile_rows, q.tile_index, q.tile_count = 8, 0, 1                         # x/0/1 names the whole frame too
    q.samples, q.max_reflections, q.use_filter, q.is_temporal = 0, -1, 7, 1    # ... and nothing but width, height, camera, view_matrix and texture_width is read
    assert np.array_equal(words_of(hip.frame_surface(q, ALL)), got)


# ---- 2. ray batches ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dragon", "theater"])
def test_ray_batches_equal_the_reference(hip, oracle, scenes, ref, name):
    """dragon: three transforms, one turned, smooth normals; theater: all three atlases.  Origins inside the scene: back faces, and a share of misses."""
    sc, rays, tw, want = free_wanted(ref, oracle, scenes, name)
    entry = want[HIT, :, 3].view(np.int32)
    hit = entry != -1
    sign = want[NORMAL, :, 3].view(np.float32)
    print("%s: %.3f hit, %.3f back faces, %d transforms" % (name, hit.mean(), (sign > 0).mean(), len(np.unique(want[UV, hit, 2]))))
    assert rays.shape[0] == 2160 and hit.mean() >= 0.30 and (~hit).mean() >= 0.05 and (sign > 0).mean() >= 0.02      # the conditions on the inputs
    if name == "dragon":
        assert len(np.unique(want[UV, hit, 2])) == 3
    else:
        a = sc.arrays["attributes"].reshape(-1, 28)[entry[hit]]
        assert (a[:, 15] != -1).mean() > 0.1 and (a[:, 16] != -1).mean() > 0.1      # (no entry of theater names a translucency texture: test_a_scene_that_names_textures_of_all_three_atlases)
    assert (want[HIT, ~hit] == MISS_HIT).all() and (want[1:, ~hit] == 0).all()
    hip.update_scene(sc)
    try:
        for n in (1, 63, 64, 65, 2160):
            assert_planes(surfaced(hip, rays[:n], tw), want[:, :n], "%s n %d" % (name, n))
            info = hip.last_surface()
            assert (info["slabs"], info["n"], info["fields"], info["frame"]) == (1, n, ALL, 0)
        misses = rays[~hit]
        got = surfaced(hip, misses, tw)                                          # a batch of misses only
        assert (got[HIT] == MISS_HIT).all() and (got[1:] == 0).all()
        hip.set_query_groups(1)                                                  # one workgroup: every lane of the first-hit launch takes ray after ray
        assert_planes(surfaced(hip, rays, tw), want, "%s, one query group" % name)
        assert hip.last_surface()["query_groups"] == 1
        hip.set_query_groups(0)
        hip.set_trace_slab(64)                                                   # 2160 rays span 34 slabs, the last one of 48 rays
        assert_planes(surfaced(hip, rays, tw), want, "%s, slabs of 64" % name)
        info = hip.last_surface()
        assert (info["slabs"], info["slab"]) == (34, 64)
        hip.set_trace_slab(0)
        assert_planes(surfaced(hip, rays, tw), want, "%s again" % name)          # the same bits every time
        assert np.array_equal(words_of(hip.surface_rays(rays, ALL, tw)), want)    # the host call
    finally:
        hip.set_query_groups(0)
        hip.set_trace_slab(0)


# ---- 3. the mask ---------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fields", list(BITS) + [1 | 32])
def test_only_the_planes_asked_for_are_written(hip, oracle, scenes, ref, fields):
    sc, rays, tw, want = free_wanted(ref, oracle, scenes, "theater")
    n = 321                                                                      # more than one workgroup of k_surface, a ragged last wave
    hip.update_scene(sc)
    everything = surfaced(hip, rays[:n], tw)
    assert_planes(everything, want[:, :n], "all planes")
    got = surfaced(hip, rays[:n], tw, fields)                                    # (surfaced holds the 256 guard bytes behind popcount(fields) * n * 16)
    assert got.shape == (capi.surface_planes(fields), n, 4)
    assert_planes(got, planes_of(everything, fields), "fields %d" % fields)
    p = surface_params(sc, 13, 7)
    frame_all = words_of(hip.frame_surface(p, ALL))
    out = guarded(13 * 7, fields)
    hip.frame_surface_device(p, fields, out)
    hip.sync()
    assert_planes(planes_in(out, 13 * 7, fields), planes_of(frame_all, fields), "a frame's fields %d" % fields)
    unpacked = capi.unpack_surface(got.view(np.float32), fields)
    assert set(unpacked) - {"entry", "transform2"} == {capi.SURFACE_NAMES[k] for k in range(8) if fields >> k & 1}


# ---- 4. textures ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_no_atlas_uploaded_takes_the_default_branch(hip, oracle, scenes, ref):
    sc, rays, tw, want = free_wanted(ref, oracle, scenes, "theater")
    view = sc.view()
    for which in range(3):
        view.atlas[which] = None
        view.atlas_w[which] = view.atlas_h[which] = 0
    bare = ref.rays(view, rays, tw)
    textured = (want[ALBEDO:] != bare[ALBEDO:]).any(axis=(0, 2))
    assert textured.mean() > 0.2 and np.array_equal(bare[:ALBEDO], want[:ALBEDO])   # the atlases show in the material planes and nowhere else
    hip.update_scene(sc)
    try:
        for which in range(3):
            hip.upload_textures(which, [], (512, 512))                           # an empty list: no atlas
        assert_planes(surfaced(hip, rays, tw), bare, "no atlas")
    finally:
        hip.update_scene(sc)


def test_a_scene_that_names_textures_of_all_three_atlases(hip, ref):
    """synth_scene's textured scene: three transforms, five cells per atlas on the reference's too-tall canvas, texture_width 128"""
    import synth_scene
    sc = synth_scene.make(seed=3, textured=True, width=64, height=48)
    p = surface_params(sc, 64, 48)
    want = wanted(("frame", "synth"), lambda: ref.frame(sc, p))
    entry = want[HIT, :, 3].view(np.int32)
    a = sc.arrays["attributes"].reshape(-1, 28)[entry[entry != -1]]
    assert p.texture_width == 128 and min((a[:, c] != -1).mean() for c in (15, 16, 17)) > 0.2 and np.isfinite(want[1:4].view(np.float32)).all()
    hip.update_scene(sc)
    assert_planes(words_of(hip.frame_surface(p, ALL)), want, "synth")


def test_a_texture_update_shows_in_the_planes(hip, oracle, scenes, ref):
    sc, rays, tw, want = free_wanted(ref, oracle, scenes, "theater")
    cell = (2048 // tw, 2048 // tw)
    w, h = sc.meta["atlas"]["albedo"]
    assert (w, h) == (2048, cell[1])                                             # one cell
    atlas = sc.arrays["atlasAlbedo"].reshape(h, w, 4)
    cells = tu.cut_cells(atlas, 1, cell)
    built = tu.build_atlas(cells, cell)
    image = tu.random_image(np.random.default_rng(5), (37, 53))
    other = copy.copy(sc)
    other.arrays = dict(sc.arrays, atlasAlbedo=np.ascontiguousarray(tu.replace_cell(built, 0, image, cell).reshape(-1)))
    after = ref.rays(other, rays, tw)
    assert (after[ALBEDO] != want[ALBEDO]).any(axis=1).mean() > 0.1 and np.array_equal(after[:ALBEDO], want[:ALBEDO])
    hip.update_scene(sc)
    try:
        hip.upload_textures(0, cells, cell)
        rebuilt = copy.copy(sc)
        rebuilt.arrays = dict(sc.arrays, atlasAlbedo=np.ascontiguousarray(built.reshape(-1)))
        assert_planes(surfaced(hip, rays, tw), ref.rays(rebuilt, rays, tw), "the atlas built on the device")
        hip.update_texture(0, 0, image)
        assert_planes(surfaced(hip, rays, tw), after, "after flx_texture_update")
    finally:
        hip.update_scene(sc)


# ---- 5. agreement with the neighbours ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dragon", "theater"])
def test_the_hit_plane_is_flx_rays_casts(hip, oracle, scenes, ref, name):
    sc, rays, tw, _ = free_wanted(ref, oracle, scenes, name)
    hip.update_scene(sc)
    cast = hip.cast_rays(rays, capi.RAYS_CLOSEST).view(np.uint32).reshape(-1, 8)
    got = surfaced(hip, rays, tw, 1 | 16)
    assert np.array_equal(got[0], cast[:, 0:4]) and np.array_equal(got[1, :, 2], cast[:, 4])
    assert (cast[:, 3].view(np.int32) >= 0).mean() > 0.3


@pytest.mark.parametrize("name", ["dragon", "theater", "cornell"])
def test_the_frame_call_and_the_rays_call_agree_on_a_cameras_rays(hip, oracle, scenes, ref, name):
    sc, p, rays, compares, _ = camera_rays(oracle, scenes, name)
    hip.update_scene(sc)
    frame = words_of(hip.frame_surface(p, ALL))
    batch = surfaced(hip, rays, p.texture_width)
    agree = frame[HIT, :, 3] == batch[HIT, :, 3]                                  # both hit rules name the same entry (or both none)
    print("%s: the hit rules agree on the entry for %d of %d pixels, on s, u, v too for %d" % (name, agree.sum(), agree.size, compares.sum()))
    assert agree.mean() > 0.9
    assert_planes(frame[:, agree], batch[:, agree], name)


# ---- 6. the device variant -----------------------------------------------------------------------------------------------------------------------------------------

def test_rays_written_on_a_side_stream_and_tensors_out(hip, oracle, scenes, ref):
    sc, rays, tw, want = free_wanted(ref, oracle, scenes, "dragon")
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
        out = hip.surface_rays_device(d, ALL, tw, stream=side)
    hip.sync()
    assert isinstance(out, torch.Tensor) and out.dtype == torch.float32 and tuple(out.shape) == (8, 2160, 4)
    assert_planes(words_of(out), want, "rays written on a side stream")
    assert np.array_equal(words_of(out), words_of(hip.surface_rays(rays, ALL, tw)))      # the host variant
    side.synchronize()
    p = surface_params(sc, 96, 54)
    planes = hip.frame_surface_device(p, 1 | 8 | 32)
    hip.sync()
    assert tuple(planes.shape) == (3, 96 * 54, 4) and np.array_equal(words_of(planes), words_of(hip.frame_surface(p, 1 | 8 | 32)))


def test_refusals(hip, oracle, scenes, ref):
    sc, rays_host, tw, want = free_wanted(ref, oracle, scenes, "theater")
    rays_host = rays_host[:256]
    p = surface_params(sc, 32, 18)
    with capi.Context(0) as fresh:
        for call, name in ((lambda: fresh.surface_rays(rays_host, ALL, tw), "flx_rays_surface"), (lambda: fresh.surface_rays_device((0, 0), ALL, tw, 0), "flx_rays_surface_device"),
                           (lambda: fresh.frame_surface(p, ALL), "flx_frame_surface"), (lambda: fresh.frame_surface_device(p, 0, 0), "flx_frame_surface_device")):
            with pytest.raises(capi.FlexLightHipError, match=r"failed \(3\): %s: no scene and transforms uploaded" % name):      # FLX_ERR_NO_SCENE
                call()
        assert fresh.last_surface()["slabs"] == 0
    hip.update_scene(sc)
    frame_before = hip.render(p)[0]
    rays = torch.from_numpy(rays_host).cuda()
    out = guarded(256, ALL)
    both = torch.zeros((256 * (32 + 128) // 4,), dtype=torch.float32, device="cuda")      # room for 256 rays and their eight planes side by side
    host = np.zeros((256 * 128,), np.uint8)
    torch.cuda.synchronize()
    hip.surface_rays_device(rays, ALL, tw, out)
    hip.sync()
    before = hip.last_surface()
    out.fill_(0xA5)
    torch.cuda.synchronize()

    def frame_with(**kw):
        q = surface_params(sc, 32, 18)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    o, r, b = out.data_ptr(), rays.data_ptr(), both.data_ptr()
    refused = [
        (lambda: hip.surface_rays_device(rays, 0, tw, out), "flx_rays_surface_device: fields asks for no plane"),
        (lambda: hip.surface_rays(rays_host, 0, tw), "flx_rays_surface: fields asks for no plane"),
        (lambda: hip.surface_rays_device((0, 0), 256, tw, 0), "flx_rays_surface_device: fields has a bit beyond FLX_SURFACE_TPO"),      # for n == 0 too
        (lambda: hip.surface_rays_device(rays, ALL, 0, out), "flx_rays_surface_device: texture_width is less than 1"),
        (lambda: hip.surface_rays(rays_host, ALL, -4), "flx_rays_surface: texture_width is less than 1"),
        (lambda: hip.frame_surface_device(None, ALL, o), "flx_frame_surface_device: params is NULL"),
        (lambda: hip.frame_surface(None, ALL), "flx_frame_surface: params is NULL"),
        (lambda: hip.frame_surface_device(frame_with(width=0), ALL, o), "flx_frame_surface_device: width or height is 0"),
        (lambda: hip.frame_surface_device(frame_with(height=0), ALL, o), "width or height is 0"),
        (lambda: hip.frame_surface_device(frame_with(texture_width=0), ALL, o), "flx_frame_surface_device: texture_width is less than 1"),
        (lambda: hip.frame_surface_device(frame_with(), 512, o), "flx_frame_surface_device: fields has a bit beyond"),
        (lambda: hip.frame_surface_device(frame_with(tile_rows=8, tile_index=0, tile_count=2), ALL, o), "the tile policy does not name the whole frame"),
        (lambda: hip.frame_surface(frame_with(tile_rows=8, tile_index=1, tile_count=2), ALL), "flx_frame_surface: the tile policy does not name the whole frame"),
        (lambda: hip.frame_surface_device(frame_with(tile_rows=8, tile_index=0, tile_count=0), ALL, o), "the tile policy does not name the whole frame"),
        (lambda: hip.surface_rays_device((rays_host.ctypes.data, 256), ALL, tw, out), "the rays are not n rows in memory of the context's device"),      # host memory
        (lambda: hip.surface_rays_device(rays, ALL, tw, host.ctypes.data), "the planes are not popcount\\(fields\\) \\* n rows in memory of the context's device"),
        (lambda: hip.frame_surface_device(p, ALL, host.ctypes.data), "the planes are not popcount\\(fields\\) \\* width \\* height rows in memory of the context's device"),
        (lambda: hip.surface_rays_device((r + 4, 255), ALL, tw, out), "the rays are not n rows in memory of the context's device, 16-byte aligned"),
        (lambda: hip.surface_rays_device(rays, ALL, tw, o + 8), "the planes are not popcount\\(fields\\) \\* n rows in memory of the context's device, 16-byte aligned"),
        (lambda: hip.surface_rays_device((r, 1 << 28), 1, tw, o), "the rays are not n rows"),                                                     # 8 GB: the allocation ends first
        (lambda: hip.frame_surface_device(frame_with(width=8192, height=8192), ALL, o), "the planes are not popcount"),                           # 8 GB: the allocation ends first
        (lambda: hip.surface_rays_device((0, 4), ALL, tw, out), "an array is NULL"),
        (lambda: hip.surface_rays_device(rays, ALL, tw, 0), "flx_rays_surface_device: an array is NULL"),
        (lambda: hip.frame_surface_device(p, ALL, 0), "flx_frame_surface_device: an array is NULL"),
        (lambda: hip.surface_rays_device((b, 256), 1, tw, b), "the rays and the planes overlap"),                                                  # the same array
        (lambda: hip.surface_rays_device((b, 256), ALL, tw, b + 255 * 32), "the rays and the planes overlap"),                                     # the planes begin in the last ray
        (lambda: hip.surface_rays_device((b + 256 * 128 - 16, 256), ALL, tw, b), "the rays and the planes overlap"),                                # the rays begin in the last plane's last row
    ]
    for call, message in refused:
        with pytest.raises(capi.FlexLightHipError, match=r"failed \(1\): .*" + message):
            call()
        assert hip.last_surface() == before, message               # nothing was enqueued
    torch.cuda.synchronize()
    assert (out == 0xA5).all()
    # n == 0: FLX_OK, nothing enqueued
    empty = hip.surface_rays_device(torch.zeros((0, 8), dtype=torch.float32, device="cuda"), ALL, tw)
    assert tuple(empty.shape) == (8, 0, 4)
    hip.surface_rays_device((0, 0), ALL, tw, 0)
    assert hip.surface_rays(np.zeros((0, 8), np.float32), 1 | 32, tw).shape == (2, 0, 4)
    assert hip.last_surface() == before
    both[256 * 32:].copy_(rays.reshape(-1))                         # side by side in one allocation: no overlap
    hip.surface_rays_device((b + 256 * 128, 256), ALL, tw, b)
    hip.sync()
    assert_planes(both[:256 * 32].cpu().numpy().view(np.uint32).reshape(8, 256, 4), want[:, :256], "the planes in front of their rays")
    assert_planes(surfaced(hip, rays_host, tw), want[:, :256], "after the refusals")
    after = hip.render(p)[0]
    assert np.array_equal(after.view(np.uint32), frame_before.view(np.uint32))      # a frame rendered afterwards equals one rendered before


# ---- 7. ordering ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_call_sees_the_rows_updated_on_the_device_before_it(hip, scenes, ref):
    sc, p, want = frame_wanted(ref, scenes, "cornell")
    entry = int(want[HIT, (FRAMES["cornell"][1] // 2) * FRAMES["cornell"][0] + FRAMES["cornell"][0] // 2, 3])      # the triangle the centre pixel sees
    assert entry >= 0
    g = sc.arrays["geometry"].reshape(-1, 12).copy()
    assert g[entry, 10] == 2
    g[entry, [1, 4, 7]] += np.float32(500.0)                                      # the triangle leaves, out of every ray's way
    moved = with_geometry(sc, reflatten_by_rule(g))
    after = ref.frame(moved, p)
    assert (want[HIT, :, 3] == entry).sum() > 10 and (after[HIT, :, 3] != entry).all()
    hip.update_scene(sc)
    try:
        assert_planes(words_of(hip.frame_surface(p, ALL)), want, "as uploaded")
        rows = torch.from_numpy(g[entry:entry + 1].copy()).cuda()
        torch.cuda.synchronize()
        hip.update_scene_rows_device(entry, rows)
        planes = hip.frame_surface_device(p, ALL)                                   # enqueued behind the update, no wait of the host in between
        hip.sync()
        assert_planes(words_of(planes), after, "after flx_scene_update_device")
    finally:
        hip.update_scene(sc)


def test_a_call_between_two_frames_of_the_loop(hip, oracle, scenes, ref):
    sc, rays, tw, want = free_wanted(ref, oracle, scenes, "dragon")
    _, p, want_frame = frame_wanted(ref, scenes, "dragon")
    hip.update_scene(sc)
    params = [sc.frame_params(width=96, height=54, samples=2, max_reflections=4, use_filter=0) for _ in range(2)]
    params[1].random_seed = params[0].random_seed + 1.0
    alone = []
    for q in params:
        hip.frame_begin(q)
        alone.append(np.asarray(hip.frame_end()[0]).copy())
    d = torch.from_numpy(rays).cuda()
    torch.cuda.synchronize()
    for q in params:
        hip.frame_begin(q)
    assert hip.frames_in_flight() == 2
    out = hip.surface_rays_device(d, ALL, tw)
    planes = hip.frame_surface_device(p, ALL)
    frames = [np.asarray(hip.frame_end()[0]).copy() for _ in params]
    hip.sync()
    assert_planes(words_of(out), want, "rays between two frames")
    assert_planes(words_of(planes), want_frame, "a frame's planes between two frames")
    for got, frame in zip(frames, alone):
        assert np.array_equal(got.view(np.uint32), frame.view(np.uint32))         # the frames in flight finish unchanged
    assert not np.array_equal(frames[0], frames[1])
