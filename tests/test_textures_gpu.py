"""flx_textures_upload[_device] and flx_texture_update[_device] on the GPU (csrc/flx_atlas.hip, csrc/flx_scene.hip): the atlas the device builds and the cell it
replaces are the bytes of the numpy restatement of sceneFile.buildAtlas (tests/textures_util.py; tests/test_textures_cpu.py holds that against the JavaScript), read
back through flx_debug_atlas_read; frames, counters, rasterized frames and traced rays of a context whose atlases were built on the device equal those of one that
was handed the finished atlases; a cell update is ordered between the frames in flight as a row update is.  Every comparison is bit equality."""
import ctypes as C

import numpy as np
import pytest

import synth_scene
import textures_util as tu
from parity_util import bit_mismatches

pytestmark = pytest.mark.gpu

# cell sizes beyond the CPU test's: one cell a row, the smallest cell, two wide cells a row, a width that is no multiple of 4 (row tails, unaligned cell origins)
GPU_PAIRS = tu.SIZE_PAIRS + [((9, 7), (2048, 2)), ((3, 3), (1, 1)), ((40, 5), (1024, 2)), ((6, 9), (5, 5))]


def images_for(rng, source, n):
    """n images of the source size, bytes and floats in turn"""
    return [tu.random_image(rng, source, floats=(k % 2 == 1)) for k in range(n)]


def on_device(images):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in images]


def upload_atlas(ctx, which, atlas):
    """flx_atlas_upload of a finished atlas [H, W, 4] uint8: today's way in"""
    from flexlight_hip import capi
    atlas = np.ascontiguousarray(atlas, np.uint8)
    rc = capi.LIB.flx_atlas_upload(ctx._h, which, atlas.ctypes.data_as(C.POINTER(C.c_uint8)), atlas.shape[1], atlas.shape[0])
    assert rc == 0, capi.LIB.flx_last_error(ctx._h)


@pytest.mark.parametrize("rows", ["tw + 1", "2 tw"])
@pytest.mark.parametrize("source,cell", GPU_PAIRS)
def test_the_built_atlas_is_the_numpy_atlas(hip, source, cell, rows):
    """a second cell row exists (n = tw + 1: one cell in it; 2 tw: full) and the rows no cell reaches are transparent black; formats mixed in one list; from host
    memory and from device memory"""
    tw = tu.cells_per_row(cell[0])
    n = tw + 1 if rows == "tw + 1" else 2 * tw
    rng = np.random.default_rng(cell[0] * 7 + cell[1] + n)
    images = images_for(rng, source, n)
    want = tu.build_atlas(images, cell)
    hip.upload_textures(1, images, cell)
    got = hip.atlas_read(1)
    assert got.shape == want.shape and np.array_equal(got, want), "from host memory"
    hip.upload_textures_device(2, on_device(images), cell)
    got = hip.atlas_read(2)
    assert got.shape == want.shape and np.array_equal(got, want), "from device memory"
    unused = want[cell[1] * ((n + tw - 1) // tw):]                    # (the too-tall canvas: rows without a cell, wherever a row holds more than one)
    assert (unused.size > 0 or tw == 1) and not unused.any()


def test_a_smaller_atlas_in_the_buffer_of_a_larger_one_is_clean(hip):
    """the buffer is reused: what the 0xFF atlas left outside the new cells must be gone"""
    cell, n = (7, 5), tu.cells_per_row(7) + 1
    upload_atlas(hip, 1, np.full((2048, 2048, 4), 0xFF, np.uint8))
    assert hip.atlas_read(1).min() == 0xFF
    rng = np.random.default_rng(5)
    images = images_for(rng, (5, 3), n)
    want = tu.build_atlas(images, cell)
    assert want.nbytes < 2048 * 2048 * 4
    hip.upload_textures_device(1, on_device(images), cell)
    assert np.array_equal(hip.atlas_read(1), want)
    upload_atlas(hip, 1, np.full((2048, 2048, 4), 0xFF, np.uint8))
    hip.upload_textures(1, images, cell)
    assert np.array_equal(hip.atlas_read(1), want)
    hip.upload_textures(1, [], cell)                                  # "none", as flx_atlas_upload(ctx, which, NULL, 0, 0)
    assert hip.atlas_read(1).shape == (0, 0, 4)


def test_float_sources_are_stored_as_a_render_target_stores_them(hip):
    """every byte's two boundaries from both sides, -0, negatives, values above 1, the infinities and NaN; picked first, then quantised"""
    values = tu.float_edges()
    values = np.concatenate([values, np.zeros(-values.size % 4, np.float32)])
    image = values.reshape(1, -1, 4)
    cell = (image.shape[1], 1)
    want = tu.quantise(image)
    assert len(np.unique(want)) == 256
    hip.upload_textures(1, [image], cell)
    assert np.array_equal(hip.atlas_read(1)[:, :cell[0]], want)
    hip.upload_textures_device(1, on_device([image]), cell)
    assert np.array_equal(hip.atlas_read(1)[:, :cell[0]], want)
    # resampled: three destination texels a source texel, and a third of the source's
    for wide in (3 * cell[0] if 3 * cell[0] <= 2048 else 2048, cell[0] // 3):
        hip.upload_textures_device(1, on_device([image]), (wide, 2))
        assert np.array_equal(hip.atlas_read(1), tu.build_atlas([image], (wide, 2)))
    hip.upload_textures(1, [np.zeros((1, cell[0], 4), np.uint8)], cell)
    hip.update_texture(1, 0, image)
    assert np.array_equal(hip.atlas_read(1)[:, :cell[0]], want)
    hip.update_texture_device(1, 0, on_device([image[:, ::-1].copy()])[0])
    assert np.array_equal(hip.atlas_read(1)[:, :cell[0]], want[:, ::-1])


@pytest.mark.parametrize("cell,n", [((683, 2), 5), ((7, 5), 294), ((16, 16), 129)])
def test_a_cell_update_changes_its_cell_and_no_other_byte(hip, cell, n):
    """index 0, tw - 1, tw (the first cell of the second cell row) and the last; sources of other sizes than the build's, bytes and floats, from host and from
    device memory; the whole atlas read back equals the numpy atlas with that one cell replaced"""
    tw = tu.cells_per_row(cell[0])
    assert n > tw
    rng = np.random.default_rng(n)
    want = tu.build_atlas(images_for(rng, (11, 3), n), cell)
    hip.upload_textures(2, tu.cut_cells(want, n, cell), cell)
    assert np.array_equal(hip.atlas_read(2), want)
    sources = [(37, 53), (1, 1), cell, (5, 3)]
    for k, index in enumerate([0, tw - 1, tw, n - 1]):
        image = tu.random_image(rng, sources[k], floats=(k % 2 == 0))
        want = tu.replace_cell(want, index, image, cell)
        if k < 2:
            hip.update_texture_device(2, index, on_device([image])[0])
        else:
            hip.update_texture(2, index, image)
        assert np.array_equal(hip.atlas_read(2), want), "index %d" % index
    for index in (tw, 0):                                         # one right after the other: the second waits for the stage the first is copied from
        image = tu.random_image(rng, (9, 9))
        want = tu.replace_cell(want, index, image, cell)
        hip.update_texture_device(2, index, on_device([image])[0])
    assert np.array_equal(hip.atlas_read(2), want)


# ---- frames -------------------------------------------------------------------------------------------------------------------------------------------------------
CELL = (16, 16)


@pytest.fixture(scope="module")
def textured():
    """synth_scene's textured scene with its atlases cut back into per-cell images and composited again (synth_scene fills the whole canvas with noise: only its
    cells are textures) -> (scene, params of a 64 x 48 frame, per atlas: the cells and the atlas)"""
    import copy
    sc = synth_scene.make(seed=3, textured=True, width=64, height=48)
    n = sc.meta["atlas"]["albedo"][1] // CELL[1]
    assert n == 5
    cells, atlases = [], []
    for key in ("atlasAlbedo", "atlasPbr", "atlasTpo"):
        full = sc.arrays[key].reshape(CELL[1] * n, CELL[0] * tu.cells_per_row(CELL[0]), 4)
        cells.append(tu.cut_cells(full, n, CELL))
        atlases.append(tu.build_atlas(cells[-1], CELL))
    sc = copy.copy(sc)
    sc.arrays = dict(sc.arrays, atlasAlbedo=atlases[0].reshape(-1), atlasPbr=atlases[1].reshape(-1), atlasTpo=atlases[2].reshape(-1))
    p = sc.frame_params(width=64, height=48, samples=2, max_reflections=3, use_filter=0)
    return sc, p, cells, atlases


def context_with(sc, cells=None, device=True):
    """a context of its own with the scene; cells: its three atlases built on the device from them instead of handed over finished"""
    from flexlight_hip import capi
    ctx = capi.Context(0)
    ctx.update_scene(sc)
    if cells is not None:
        for which in range(3):
            if device:
                ctx.upload_textures_device(which, on_device(cells[which]), CELL)
            else:
                ctx.upload_textures(which, cells[which], CELL)
    return ctx


def camera_rays(p, n=256):
    from flexlight_hip import capi
    side = int(np.sqrt(n))
    x, y = np.meshgrid(np.linspace(-0.6, 0.6, side), np.linspace(-0.4, 0.4, side))
    rays = np.zeros((side * side, 8), np.float32)
    rays[:, 0:3] = list(p.camera)
    rays[:, 4], rays[:, 5], rays[:, 6] = x.reshape(-1), y.reshape(-1), 1.0
    rays[:, [3, 7]] = capi.noise_coordinates(side * side)
    return rays


def shown_cell(ctx, p, atlas, cells, before):
    """-> (index, image, frame): an albedo cell whose replacement by its inverse changes the frame"""
    for index in range(len(cells)):
        image = 255 - cells[index]
        ctx.update_texture(0, index, image)
        frame = ctx.render(p)[0]
        if bit_mismatches(frame, before):
            return index, image, frame
        ctx.update_texture(0, index, cells[index])
    raise AssertionError("no albedo cell shows in the frame")


def test_frames_of_a_device_built_atlas_equal_frames_of_the_finished_one(textured):
    from flexlight_hip import capi
    sc, p, cells, atlases = textured
    rays, tp = camera_rays(p), capi.TraceParams.of_frame(p)
    with context_with(sc) as old, context_with(sc, cells) as new:
        for which in range(3):
            assert np.array_equal(new.atlas_read(which), atlases[which]) and np.array_equal(old.atlas_read(which), atlases[which])
        want, want_cnt, _ = old.render(p, counters=True)
        got, cnt, _ = new.render(p, counters=True)
        assert want_cnt["atlas_texels"] > 0 and cnt == want_cnt
        assert bit_mismatches(got, want) == 0
        assert bit_mismatches(new.raster_render(p)[0], old.raster_render(p)[0]) == 0
        assert np.array_equal(new.trace_rays(rays, tp), old.trace_rays(rays, tp))
        assert capi.unpack_radiance(old.trace_rays(rays, tp))["alpha"].sum() > 0
        # one texture replaced in place: the frame changes, and it is the frame of a context that was handed the atlas with that cell replaced
        index, image, changed = shown_cell(new, p, atlases[0], cells[0], got)
        assert bit_mismatches(changed, want) > 0
        replaced = tu.replace_cell(atlases[0], index, image, CELL)
        assert np.array_equal(new.atlas_read(0), replaced)
        upload_atlas(old, 0, replaced)
        assert bit_mismatches(changed, old.render(p)[0]) == 0
        assert bit_mismatches(new.raster_render(p)[0], old.raster_render(p)[0]) == 0
        assert np.array_equal(new.trace_rays(rays, tp), old.trace_rays(rays, tp))
        # ... a float image of another size, from device memory
        image = tu.random_image(np.random.default_rng(11), (23, 9), floats=True)
        new.update_texture_device(0, index, on_device([image])[0])
        upload_atlas(old, 0, tu.replace_cell(atlases[0], index, image, CELL))
        assert bit_mismatches(new.render(p)[0], old.render(p)[0]) == 0
    with context_with(sc, cells, device=False) as host:
        assert bit_mismatches(host.render(p)[0], want) == 0


@pytest.mark.parametrize("served", [False, True])
def test_an_update_falls_between_the_frames_in_flight(textured, served):
    """two lanes, two frames in flight: the frame begun before flx_texture_update_device shows the old texture, the next one the new; and the same where the frame
    server takes the frames: its launch ends (the frame posted to it completes first), the next frame shows the new texture"""
    sc, p, cells, atlases = textured
    with context_with(sc, cells) as ctx:
        old = ctx.render(p)[0]
        index, image, new = shown_cell(ctx, p, atlases[0], cells[0], old)
        ctx.update_texture(0, index, cells[0][index])
        ctx.set_frame_lanes(2)
        ctx.set_frame_chain(3 if served else 0)
        if served:
            assert ctx.frame_server_takes(p) == 1
        d_image, d_back = on_device([image])[0], on_device([cells[0][index]])[0]
        ctx.frame_begin(p)
        assert ctx.last_chained() == (3 if served else 0)
        ctx.update_texture_device(0, index, d_image)
        ctx.frame_begin(p)
        first, second = ctx.frame_end()[0], ctx.frame_end()[0]
        assert bit_mismatches(first, old) == 0 and bit_mismatches(second, new) == 0
        ctx.frame_begin(p)                                        # both lanes busy with the new texture; then back
        ctx.frame_begin(p)
        ctx.update_texture_device(0, index, d_back)
        third, fourth = ctx.frame_end()[0], ctx.frame_end()[0]
        ctx.frame_begin(p)
        fifth = ctx.frame_end()[0]
        assert bit_mismatches(third, new) == 0 and bit_mismatches(fourth, new) == 0 and bit_mismatches(fifth, old) == 0
        assert np.array_equal(ctx.atlas_read(0), atlases[0])


def test_the_source_may_still_be_written_on_the_producer_stream(hip):
    """the tensor is filled on a torch side stream behind work that takes a while, and that stream is passed: the build and the update wait for it"""
    import torch
    cell = (16, 8)
    rng = np.random.default_rng(2)
    images = images_for(rng, (37, 53), 3)
    final = [torch.from_numpy(a).cuda() for a in images]
    late = [torch.zeros_like(t) for t in final]
    busy = torch.ones((2048, 2048), device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(20):
            busy = busy @ busy * 1e-4
        for t, f in zip(late, final):
            t.copy_(f)
    hip.upload_textures_device(1, late, cell, stream=side)
    want = tu.build_atlas(images, cell)
    assert np.array_equal(hip.atlas_read(1), want)
    image = tu.random_image(rng, (20, 20), floats=True)
    final, late = torch.from_numpy(image).cuda(), torch.zeros((20, 20, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(20):
            busy = busy @ busy * 1e-4
        late.copy_(final)
    hip.update_texture_device(1, 2, late, stream=side)
    assert np.array_equal(hip.atlas_read(1), tu.replace_cell(want, 2, image, cell))
    torch.cuda.synchronize()


def test_refusals_leave_the_atlas_and_the_frame_as_they_were(textured):
    """every refusal, with its message; after each the atlas read back and a frame are what they were.  Argument errors answered with a status: nothing runs"""
    import torch
    from flexlight_hip import capi
    sc, p, cells, atlases = textured
    lib = capi.LIB
    hiprt = C.CDLL("libamdhip64.so")
    texel = np.zeros(64, np.uint8)
    good = capi.Image(texel.ctypes.data, 2, 2, capi.IMAGE_RGBA8)
    tensor = torch.zeros((4, 4, 4), dtype=torch.uint8, device="cuda")
    ftensor = torch.zeros((4, 4, 4), dtype=torch.float32, device="cuda")
    exact = C.c_void_p()
    assert hiprt.hipMalloc(C.byref(exact), C.c_size_t(1 << 21)) == 0         # an allocation of exactly 2^19 texels
    with context_with(sc, cells) as ctx:
        h = ctx._h
        frame = ctx.render(p)[0]

        def refused(rc, message):
            assert rc == 1, rc                                                # FLX_ERR_INVALID
            assert message in lib.flx_last_error(h).decode(), lib.flx_last_error(h).decode()
            for which in range(3):
                assert np.array_equal(ctx.atlas_read(which), atlases[which])
            assert bit_mismatches(ctx.render(p)[0], frame) == 0

        def one(pixels, w, h_, fmt):
            return (capi.Image * 1)(capi.Image(pixels, w, h_, fmt))
        host = texel.ctypes.data
        # the upload, in the order the rules are said: each case breaks every later rule too
        refused(lib.flx_textures_upload(h, 3, None, 1, 0, 0), "which must be 0, 1 or 2")
        refused(lib.flx_textures_upload(h, -1, None, 0, 16, 16), "which must be 0, 1 or 2")
        refused(lib.flx_textures_upload(h, 0, None, 1, 0, 0), "images is NULL")
        refused(lib.flx_textures_upload(h, 0, one(None, 0, 0, 9), 1, 0, 0), "cell_w must be 1 .. 2048")
        refused(lib.flx_textures_upload(h, 0, one(None, 0, 0, 9), 1, 2049, 0), "cell_w must be 1 .. 2048")
        refused(lib.flx_textures_upload(h, 0, one(None, 0, 0, 9), 1, 16, 0), "cell_h is 0")
        refused(lib.flx_textures_upload(h, 0, one(None, 0, 0, 9), 1, 16, 16), "pixels are NULL")
        refused(lib.flx_textures_upload(h, 0, one(host, 0, 2, 9), 1, 16, 16), "width or height is 0")
        refused(lib.flx_textures_upload(h, 0, one(host, 2, 0, 9), 1, 16, 16), "width or height is 0")
        refused(lib.flx_textures_upload(h, 0, one(host, 2, 2, 2), 1, 16, 16), "format is neither")
        refused(lib.flx_textures_upload(h, 1, (capi.Image * 3)(good, good, capi.Image(host, 2, 2, 5)), 3, 16, 16), "format is neither")
        refused(lib.flx_textures_upload(h, 2, one(host, 2, 2, 0), 1, 16, 1 << 31), "2^31 texels high")
        refused(lib.flx_textures_upload_device(h, 0, one(None, 4, 4, 0), 1, 16, 16, None), "pixels are NULL")
        # device variants: a host pointer, a tensor one texel too short, a misaligned view
        not_there = "not in memory of the context's device"
        refused(lib.flx_textures_upload_device(h, 0, one(host, 2, 2, 0), 1, 16, 16, None), not_there)
        refused(lib.flx_textures_upload_device(h, 0, one(exact.value, (1 << 19) + 1, 1, 0), 1, 16, 16, None), not_there)
        refused(lib.flx_textures_upload_device(h, 0, one(exact.value + 4, 1 << 19, 1, 0), 1, 16, 16, None), not_there)
        refused(lib.flx_textures_upload_device(h, 0, one(tensor.data_ptr() + 2, 2, 2, 0), 1, 16, 16, None), not_there)
        refused(lib.flx_textures_upload_device(h, 0, one(ftensor.data_ptr() + 4, 2, 2, 1), 1, 16, 16, None), not_there)
        refused(lib.flx_textures_upload_device(h, 0, (capi.Image * 2)(capi.Image(tensor.data_ptr(), 4, 4, 0), capi.Image(host, 2, 2, 0)), 2, 16, 16, None), not_there)
        # the update
        refused(lib.flx_texture_update(h, 3, 0, None), "which must be 0, 1 or 2")
        refused(lib.flx_texture_update(h, 0, 0, None), "image is NULL")
        refused(lib.flx_texture_update(h, 0, 5, one(None, 0, 0, 9)), "index is not a cell")
        refused(lib.flx_texture_update(h, 0, 0xffffffff, one(host, 2, 2, 0)), "index is not a cell")
        refused(lib.flx_texture_update(h, 0, 4, one(None, 0, 0, 9)), "pixels are NULL")
        refused(lib.flx_texture_update(h, 0, 4, one(host, 2, 0, 9)), "width or height is 0")
        refused(lib.flx_texture_update(h, 0, 4, one(host, 2, 2, 9)), "format is neither")
        refused(lib.flx_texture_update_device(h, 0, 4, one(host, 2, 2, 0), None), not_there)
        refused(lib.flx_texture_update_device(h, 0, 4, one(exact.value, (1 << 19) + 1, 1, 0), None), not_there)
        refused(lib.flx_texture_update_device(h, 0, 4, one(ftensor.data_ptr() + 4, 2, 2, 1), None), not_there)
        # what was accepted all along still is: the exact allocation as the image it holds, the aligned views
        assert hiprt.hipMemset(exact, 0x5a, C.c_size_t(1 << 21)) == 0 and hiprt.hipDeviceSynchronize() == 0
        ctx.update_texture_device(0, 4, (exact.value, 1 << 19, 1, 0))
        ctx.update_texture_device(0, 4, (tensor.data_ptr() + 4, 3, 1, 0))
        ctx.update_texture_device(0, 4, (ftensor.data_ptr() + 16, 3, 1, 1))
        ctx.update_texture(0, 4, cells[0][4])
        assert np.array_equal(ctx.atlas_read(0), atlases[0])
        # a finished atlas has no known cells: no cell update after it, nor after "none", nor before anything
        upload_atlas(ctx, 1, atlases[1])
        refused(lib.flx_texture_update(h, 1, 0, one(host, 2, 2, 0)), "no atlas built by flx_textures_upload is resident")
        ctx.upload_textures(1, cells[1], CELL)
        ctx.update_texture(1, 0, cells[1][0])
        ctx.upload_textures(2, [], CELL)
        assert lib.flx_texture_update(h, 2, 0, one(host, 2, 2, 0)) == 1 and "no atlas built" in lib.flx_last_error(h).decode()
    with capi.Context(0) as fresh:
        assert lib.flx_texture_update(fresh._h, 0, 0, one(host, 2, 2, 0)) == 1 and "no atlas built" in lib.flx_last_error(fresh._h).decode()
        assert fresh.atlas_read(0).shape == (0, 0, 4)
    assert hiprt.hipFree(exact) == 0


def test_a_group_builds_and_updates_on_all_its_contexts(textured):
    from flexlight_hip import capi
    sc, p, cells, atlases = textured
    with context_with(sc, cells) as one, capi.Group([0, 0]) as g:
        g.update_scene(sc)
        for which in range(3):
            g.upload_textures(which, cells[which], CELL)
        for rank in range(2):
            for which in range(3):
                assert np.array_equal(g.context(rank).atlas_read(which), atlases[which])
        want = one.render(p)[0]
        assert bit_mismatches(g.render(p)[0][0], want) == 0
        index, image, changed = shown_cell(one, p, atlases[0], cells[0], want)
        g.update_texture(0, index, image)
        assert bit_mismatches(g.render(p)[0][0], changed) == 0
        for rank in range(2):
            assert np.array_equal(g.context(rank).atlas_read(0), tu.replace_cell(atlases[0], index, image, CELL))
        with pytest.raises(capi.FlexLightHipError, match="index is not a cell"):
            g.update_texture(0, 5, image)
