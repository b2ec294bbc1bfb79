"""Anti-aliased path-tracer frames in the library's frame loop (flx_frame_begin with FLX_FRAME_FXAA / FLX_FRAME_TAA OR'ed into the format).

An FXAA loop frame is flx_render followed by flx_fxaa, bit for bit: the float frame (FLX_FRAME_FLOAT), the same in device memory (FLX_FRAME_DEVICE)
and flx_present of it (FLX_FRAME_RGBA8, which the pass stores itself).  TAA loop frames rotate the same nine-frame ring as flx_taa, so N of them equal
N calls of render + flx_taa on a fresh context.  Frames of every kind interleave with frames the frame server takes, and come out in begin order."""
import ctypes as C

import numpy as np
import pytest

from flexlight_hip import capi
from flexlight_hip.scene_io import view_matrix
from frame_loop_util import bits, run_loop

pytestmark = pytest.mark.gpu

FORMATS = [dict(), dict(device=True), dict(rgba8=True)]


def moving(sc, f, **kw):
    p = sc.frame_params(**kw)
    p.camera[0] += 0.05 * f
    p.camera[2] -= 0.03 * f
    return p


def jittered(sc, f, width, height, **kw):
    """the TAA camera: a sub-pixel turn of the view per frame (taa.js:120-127)"""
    p = sc.frame_params(width=width, height=height, **kw)
    cam = sc.meta["camera"]
    jx, jy = 0.3 / min(width, height) * np.array([[0, 1], [1, 0], [-0.7, 0.4], [0.2, -0.9], [0.5, 0.5], [-0.4, -0.3], [0.1, 0.6], [-0.6, -0.2], [0.7, -0.1]])[f % 9]
    p.view_matrix[:] = view_matrix(cam["fx"] + jx, cam["fy"] + jy, cam["fov"], width, height).tolist()
    return p


def expect(want_float, kw, ctx):
    if kw.get("rgba8"):
        return ctx.present(want_float)
    return want_float


def assert_equal(got, want, what):
    if want.dtype == np.uint8:
        assert got.dtype == np.uint8 and np.array_equal(got, want), what
    else:
        bad = np.argwhere((bits(got) != bits(want)).any(axis=-1))
        assert bad.size == 0, "%s: %d pixels differ, first %s" % (what, len(bad), bad[0])


@pytest.mark.parametrize("case", [
    dict(name="cornell", width=64, height=48, samples=2, max_reflections=3, use_filter=0),
    dict(name="cornell", width=64, height=48, samples=2, max_reflections=3, use_filter=1),
    dict(name="cornell_obj", width=96, height=54, samples=4, max_reflections=3, use_filter=0),
    dict(name="cornell_obj", width=96, height=54, samples=4, max_reflections=3, use_filter=1),
    dict(name="cornell_obj", width=96, height=54, samples=2, max_reflections=3, use_filter=0, temporal=True),
], ids=["cornell", "cornell-filter", "cornell_obj", "cornell_obj-filter", "cornell_obj-temporal"])
def test_fxaa_frames_equal_render_then_fxaa(scenes, case):
    """six frames per format, a moving camera: both lanes serve FXAA frames (temporal frames stay on the first lane)"""
    case = dict(case)
    name, temporal = case.pop("name"), case.pop("temporal", False)
    sc = scenes(name)
    ps = []
    for f in range(6 * len(FORMATS)):
        p = moving(sc, f, **case)
        if temporal:
            p.is_temporal = 1
            p.random_seed = float(f % 4)
        ps.append(p)
    with capi.Context(0) as ref, capi.Context(0) as ctx:
        ref.update_scene(sc)
        ctx.update_scene(sc)
        want = [ref.fxaa(ref.render(p)[0]) for p in ps]
        frames = [(p, dict(FORMATS[f % 3], antialiasing="fxaa")) for f, p in enumerate(ps)]
        got, lanes, chained = run_loop(ctx, frames)
        for f, (p, kw) in enumerate(frames):
            assert_equal(got[f], expect(want[f], kw, ref), "frame %d %s" % (f, kw))
    host_lanes = [lanes[f] for f in range(len(frames)) if not frames[f][1].get("device")]
    assert set(host_lanes) == ({0} if temporal else {0, 1}), lanes
    assert chained == [0] * len(frames)


def taa_sequence(sc, sizes):
    """12 jittered frames, sizes[f] = (W, H) of frame f"""
    return [jittered(sc, f, *sizes[f], samples=2, max_reflections=3, use_filter=0) for f in range(12)]


@pytest.mark.parametrize("variant", ["plain", "size-change", "reset"])
def test_taa_frames_rotate_the_same_ring_as_flx_taa(scenes, variant):
    """12 TAA loop frames (the ring of nine wraps) equal a fresh context doing render + flx_taa in the same order; a change of size resets the
    ring; flx_taa_reset applies to the frames begun after it"""
    sc = scenes("cornell")
    sizes = [(64, 48)] * 12 if variant != "size-change" else [(64, 48)] * 5 + [(80, 40)] * 7
    reset_at = 6 if variant == "reset" else None
    ps = taa_sequence(sc, sizes)
    with capi.Context(0) as ref, capi.Context(0) as ctx:
        ref.update_scene(sc)
        ctx.update_scene(sc)
        want = []
        for f, p in enumerate(ps):
            if f == reset_at:
                ref.taa_reset()
            want.append(ref.taa(ref.render(p)[0]))
        frames = [(p, dict(FORMATS[f % 3], antialiasing="taa")) for f, p in enumerate(ps)]
        got, lanes, _ = run_loop(ctx, frames, between=lambda i: ctx.taa_reset() if i == reset_at else None)
        for f, (p, kw) in enumerate(frames):
            assert got[f].shape[:2] == (p.height, p.width)
            assert_equal(got[f], expect(want[f], kw, ref), "frame %d %s" % (f, kw))
    assert set(lanes) <= {0, -1}, lanes                      # TAA frames run on the first lane, where the ring is


def test_aa_frames_interleave_with_served_frames(hip, scenes):
    """plain frames the frame server takes, FXAA / TAA frames and plain frames on the lanes, in one loop: begin order and bits kept, the AA frames
    never chained"""
    sc = scenes("dragon")
    hip.update_scene(sc)
    hip.taa_reset()                                           # (the session's context: the ring starts empty, as the fresh one's)
    hip.set_frame_chain(3)
    try:
        ps = [moving(sc, f, width=128, height=96, samples=1, max_reflections=2, use_filter=0) for f in range(10)]
        assert all(hip.frame_server_takes(p) for p in ps)
        kinds = ["served", "fxaa", "served", "taa", "fxaa", "served", "served", "taa", "fxaa", "served"]
        with capi.Context(0) as ref:
            ref.update_scene(sc)
            want = []
            for p, k in zip(ps, kinds):
                frame = ref.render(p)[0]
                want.append(ref.fxaa(frame) if k == "fxaa" else ref.taa(frame) if k == "taa" else frame)
            frames = [(p, dict(FORMATS[f % 3], **({} if k == "served" else dict(antialiasing=k)))) for f, (p, k) in enumerate(zip(ps, kinds))]
            got, _, chained = run_loop(hip, frames)
            for f, (p, kw) in enumerate(frames):
                assert_equal(got[f], expect(want[f], kw, ref), "frame %d %s %s" % (f, kinds[f], kw))
        for f, k in enumerate(kinds):
            assert chained[f] == (3 if k == "served" else 0), (kinds, chained)
    finally:
        hip.set_frame_chain(2)
        hip.taa_reset()


def refused(ctx, fn, match):
    before = ctx.frames_in_flight()
    with pytest.raises(capi.FlexLightHipError, match=match):
        fn()
    assert ctx.frames_in_flight() == before


def test_refusals_leave_nothing_in_flight(hip, scenes):
    sc = scenes("cornell")
    hip.update_scene(sc)
    p = sc.frame_params(width=64, height=48, samples=1, max_reflections=2, use_filter=0)
    strip = sc.frame_params(width=64, height=48, samples=1, max_reflections=2, use_filter=0, tile=(8, 1, 3))
    begin = lambda q, fmt: hip._check(capi.LIB.flx_frame_begin(hip._h, C.byref(q), fmt), "flx_frame_begin")
    for in_flight in (0, 1):
        if in_flight:
            hip.frame_begin(p)
        refused(hip, lambda: begin(p, capi.FRAME_FXAA | capi.FRAME_TAA), "FLX_FRAME_FXAA and FLX_FRAME_TAA together")
        refused(hip, lambda: begin(p, capi.FRAME_FXAA | capi.FRAME_TAA | capi.FRAME_RASTERIZER | 1), "together")
        for unknown in (0x40, 0x80, 0x200, 0x400, 0x1000, 0x10000, 0x40000000):
            refused(hip, lambda: begin(p, unknown), "unknown flags")
            refused(hip, lambda: begin(p, capi.FRAME_FXAA | capi.FRAME_RASTERIZER | unknown), "unknown flags")
        for low in (3, 4, 0xf):                                # (format & 0x0f is the format itself)
            refused(hip, lambda: begin(p, low | capi.FRAME_FXAA), "format is FLX_FRAME_FLOAT")
        for aa in ("fxaa", "taa"):
            refused(hip, lambda: hip.frame_begin(strip, antialiasing=aa), "whole frames only")
            refused(hip, lambda: hip.frame_begin(strip, rasterizer=True, antialiasing=aa), "whole frames only")
        for flag in (capi.FRAME_FXAA, capi.FRAME_TAA, capi.FRAME_RASTERIZER):
            refused(hip, lambda: hip._check(capi.LIB.flx_frame_begin_gathered(hip._h, C.byref(p), flag, -1), "flx_frame_begin_gathered"), "takes no flags")
        if in_flight:
            hip.frame_end()
    with pytest.raises(ValueError):
        hip.frame_begin(p, antialiasing="msaa")
    assert hip.frames_in_flight() == 0
    g = capi.Group([0])
    try:
        g.update_scene(sc)
        for flag in (capi.FRAME_FXAA, capi.FRAME_TAA, capi.FRAME_RASTERIZER):
            with pytest.raises(capi.FlexLightHipError, match="format is"):
                g._check(capi.LIB.flx_group_frame_begin(g._h, C.byref(p), 8, flag), "flx_group_frame_begin")
            assert g.frames_in_flight() == 0
    finally:
        g.close()
    # after the refusals the loop works as before
    got, _, _ = run_loop(hip, [(p, {}), (p, dict(antialiasing="fxaa"))])
    assert_equal(got[0], hip.render(p)[0], "plain frame after the refusals")
    assert_equal(got[1], hip.fxaa(hip.render(p)[0]), "FXAA frame after the refusals")
