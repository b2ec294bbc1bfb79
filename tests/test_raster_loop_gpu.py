"""Rasterizer frames in the library's frame loop (flx_frame_begin with FLX_FRAME_RASTERIZER): every loop frame equals flx_raster_render's frame bit
for bit in all three formats, on both lanes — the RGBA8 bytes, which k_raster stores itself, equal flx_present of that frame.  With FLX_FRAME_FXAA /
FLX_FRAME_TAA the frame equals raster_render followed by flx_fxaa / flx_taa; raster and path frames interleave in one loop."""
import numpy as np
import pytest

from flexlight_hip import capi
from frame_loop_util import bits, run_loop

pytestmark = pytest.mark.gpu

FORMATS = [dict(), dict(device=True), dict(rgba8=True)]


def moving(sc, f, **kw):
    p = sc.frame_params(**kw)
    p.camera[0] += 0.05 * f
    p.camera[2] -= 0.03 * f
    return p


def assert_equal(got, want, what):
    if want.dtype == np.uint8:
        assert got.dtype == np.uint8 and np.array_equal(got, want), what
    else:
        bad = np.argwhere((bits(got) != bits(want)).any(axis=-1))
        assert bad.size == 0, "%s: %d pixels differ, first %s" % (what, len(bad), bad[0])


def check_loop(ctx, ref, ps, aa=None, want_fn=None):
    """every params of ps in each format (cycled), rasterizer frames; -> the lanes the host frames went to"""
    frames = [(p, dict(FORMATS[f % 3], rasterizer=True, antialiasing=aa)) for f, p in enumerate(ps)]
    want = [want_fn(p) if want_fn else ref.raster_render(p)[0] for p in ps]
    got, lanes, chained = run_loop(ctx, frames)
    for f, (p, kw) in enumerate(frames):
        assert_equal(got[f], ref.present(want[f]) if kw.get("rgba8") else want[f], "frame %d %s" % (f, kw))
    assert chained == [0] * len(frames)
    return [lanes[f] for f in range(len(frames)) if not frames[f][1].get("device")]


@pytest.mark.parametrize("name,size", [("cornell", (64, 48)), ("cornell_obj", (96, 54)), ("theater", (96, 54)), ("dragon", (160, 90))])
def test_loop_frames_equal_raster_render(hip, scenes, name, size):
    """six frames per format with a moving camera; the path-tracing fields of the params (samples, bounces, filter, temporal) are ignored"""
    sc = scenes(name)
    hip.update_scene(sc)
    ps = []
    for f in range(18):
        p = moving(sc, f, width=size[0], height=size[1], samples=1 + f % 3, max_reflections=f % 4, use_filter=f % 2)
        p.is_temporal = (f // 2) % 2
        ps.append(p)
    lanes = check_loop(hip, hip, ps)
    assert set(lanes) == {0, 1}, lanes


def test_full_size_loop_frame(hip, scenes):
    sc = scenes("cornell_obj")
    hip.update_scene(sc)
    ps = [moving(sc, f, width=1920, height=1080) for f in range(3)]
    check_loop(hip, hip, ps)


@pytest.mark.parametrize("shape", [dict(width=1, height=1), dict(width=7, height=5), dict(width=64, height=48, tile=(8, 1, 3)),
                                   dict(width=70, height=45, tile=(4, 2, 3))], ids=["1x1", "7x5", "strips-8-of-3", "strips-4-of-3"])
def test_edge_sizes_and_strips(hip, scenes, shape):
    sc = scenes("cornell")
    hip.update_scene(sc)
    ps = [moving(sc, f, **shape) for f in range(6)]
    check_loop(hip, hip, ps)


@pytest.mark.parametrize("name", ["cornell_obj", "theater"])
def test_fxaa_frames_equal_raster_render_then_fxaa(hip, scenes, name):
    sc = scenes(name)
    hip.update_scene(sc)
    ps = [moving(sc, f, width=96, height=54) for f in range(9)]
    lanes = check_loop(hip, hip, ps, aa="fxaa", want_fn=lambda p: hip.fxaa(hip.raster_render(p)[0]))
    assert set(lanes) == {0, 1}, lanes


def test_taa_frames_equal_raster_render_then_taa(scenes):
    """12 frames: the ring of nine wraps; a fresh context does raster_render + flx_taa in the same order"""
    sc = scenes("cornell_obj")
    ps = [moving(sc, f, width=96, height=54) for f in range(12)]
    with capi.Context(0) as ref, capi.Context(0) as ctx:
        ref.update_scene(sc)
        ctx.update_scene(sc)
        lanes = check_loop(ctx, ref, ps, aa="taa", want_fn=lambda p: ref.taa(ref.raster_render(p)[0]))
    assert set(lanes) == {0}, lanes


def test_raster_and_path_frames_alternate(hip, scenes):
    sc = scenes("cornell_obj")
    hip.update_scene(sc)
    kinds = ["raster", "path", "raster-fxaa", "path-fxaa", "raster", "raster", "path", "path", "raster-fxaa", "path"]
    ps = [moving(sc, f, width=96, height=54, samples=2, max_reflections=3, use_filter=f % 2) for f in range(len(kinds))]
    want, frames = [], []
    for f, (p, k) in enumerate(zip(ps, kinds)):
        frame = hip.raster_render(p)[0] if k.startswith("raster") else hip.render(p)[0]
        want.append(hip.fxaa(frame) if k.endswith("fxaa") else frame)
        frames.append((p, dict(FORMATS[f % 3], rasterizer=k.startswith("raster"), antialiasing="fxaa" if k.endswith("fxaa") else None)))
    got, _, _ = run_loop(hip, frames)
    for f, (p, kw) in enumerate(frames):
        assert_equal(got[f], hip.present(want[f]) if kw.get("rgba8") else want[f], "frame %d %s %s" % (f, kinds[f], kw))


def unorm8(b):
    return (b.astype(np.float32) / np.float32(255)).astype(np.float32)


@pytest.mark.parametrize("name", ["cornell", "theater"])
def test_the_byte_plane_equals_the_quantized_float_frame(hip, scenes, name):
    """k_raster's RGBA8 plane (the texture of the loop's FXAA pass) against k_quantize of its float frame: where FXAA's early-out copies the centre
    texel, the pass's output is that texel itself"""
    sc = scenes(name)
    hip.update_scene(sc)
    p = sc.frame_params(width=96, height=54)
    frame = hip.raster_render(p)[0]
    quantized = hip.present(frame)                           # k_quantize of the float frame
    fx = hip.fxaa(frame)
    early = (bits(fx) == bits(unorm8(quantized))).all(axis=-1)
    assert early.mean() > 0.5, early.mean()
    got, _, _ = run_loop(hip, [(p, dict(rasterizer=True, antialiasing="fxaa")), (p, dict(rasterizer=True, antialiasing="fxaa", rgba8=True))])
    assert np.array_equal(bits(got[0])[early], bits(unorm8(quantized))[early])
    assert np.array_equal(got[1][early], quantized[early])
