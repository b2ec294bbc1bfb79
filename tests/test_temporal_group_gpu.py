"""Temporal accumulation on a group of contexts (flx_group_frame_begin / _end), every context keeping the history of its own strips.

A temporal sequence through the group's frame loop equals the same sequence on one context frame by frame, bit for bit: float frames on the
contexts' lanes, filter frames with the five render targets (after the temporal pass) exchanged and the chain on context 0, and the canvas' bytes
equal to flx_present of the one context's float frame.  The history starts again where it does on one context (a size or temporalSamples change,
flx_temporal_reset) and where tile_rows changes.  Single contexts render temporal strips of their own rows.  Groups name device 0 several times,
as tests/test_group_gpu.py does."""
import numpy as np
import pytest

from parity_util import assert_parity

pytestmark = pytest.mark.gpu


def temporal_params(sc, w, h, n, spp, bounces, filt, hdr):
    p = sc.frame_params(width=w, height=h, samples=spp, max_reflections=bounces, use_filter=filt, hdr=hdr)
    p.is_temporal, p.temporal_samples = 1, n
    return p


def copy_params(p, **kw):
    q = type(p).from_buffer_copy(p)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def sequence(p, n):
    """2N + 1 frames of a temporal run, frame f traced with seed f % N; the camera moves at two frames, one frame without temporal accumulation in the middle"""
    out = []
    for f in range(2 * n + 1):
        q = copy_params(p, random_seed=float(f % n))
        if f >= 2:
            q.camera[0] = p.camera[0] + 0.05
        if f >= n + 2:
            q.camera[1] = p.camera[1] + 0.05
        if f == n:
            q.is_temporal, q.random_seed = 0, 0.0
        out.append(q)
    return out


def single_frames(ctx, seq):
    ctx.temporal_reset()
    return [ctx.render(q)[0] for q in seq]


def group_frames(g, seq, tile_rows, rgba8=False, lanes=3):
    """the frames through the group's loop, as many in flight as it has lanes"""
    got = []
    for q in seq:
        if g.frames_in_flight() == lanes:
            got.append(g.frame_end()[0])
        g.frame_begin(q, tile_rows=tile_rows, rgba8=rgba8)
    while g.frames_in_flight():
        got.append(g.frame_end()[0])
    return got


@pytest.fixture(scope="module")
def one():
    from flexlight_hip import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


CASES = [
    # name, w, h, N, spp, bounces, filter, ranks, tile_rows
    ("cornell", 96, 72, 4, 1, 3, 0, 2, 8),
    ("dragon", 200, 117, 4, 1, 3, 0, 3, 8),          # 15 strips, the last one 5 rows
    ("theater", 96, 54, 3, 1, 2, 0, 4, 5),           # history depth 3: vec4(0) stand-ins; strips of 5 rows
    ("cornell", 64, 24, 4, 1, 2, 0, 5, 8),           # 3 strips: contexts 3 and 4 own no rows
    ("cornell_obj", 128, 72, 4, 2, 3, 1, 3, 8),      # the filter: planes after the temporal pass exchanged, the chain on context 0
]


@pytest.mark.parametrize("hdr", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=["cornell_2", "dragon_3_ragged", "theater_4_n3_rows5", "cornell_5_idle", "cornell_obj_filter_3"])
def test_group_loop_equals_one_context_frame_by_frame(one, scenes, case, hdr):
    from flexlight_hip import capi
    name, w, h, n, spp, bounces, filt, ranks, tr = case
    sc = scenes(name)
    one.update_scene(sc)
    seq = sequence(temporal_params(sc, w, h, n, spp, bounces, filt, hdr), n)
    want = single_frames(one, seq)
    assert not np.array_equal(want[1], want[0])
    with capi.Group([0] * ranks) as g:
        g.update_scene(sc)
        for lanes in (2, 3):
            g.set_frame_lanes(lanes)
            g.temporal_reset()
            got = group_frames(g, seq, tr, lanes=lanes)
            assert len(got) == len(seq)
            for f, (a, b) in enumerate(zip(got, want)):
                assert np.array_equal(a, b, equal_nan=True), "%s lanes %d frame %d" % (name, lanes, f)
        # the canvas' bytes: flx_present of the one context's float frame
        g.temporal_reset()
        got8 = group_frames(g, seq, tr, rgba8=True, lanes=3)
        for f, (a, b) in enumerate(zip(got8, want)):
            assert np.array_equal(a, one.present(b)), "%s RGBA8 frame %d" % (name, f)


def test_group_sequence_matches_oracle(scenes, oracle):
    from flexlight_hip import capi
    sc = scenes("dragon")
    p = temporal_params(sc, 160, 90, 4, 1, 3, 0, 1)
    want = oracle.render_sequence(sc, p, 5)
    with capi.Group([0, 0, 0]) as g:
        g.update_scene(sc)
        got = group_frames(g, [copy_params(p, random_seed=float(f % 4)) for f in range(5)], 8)
    for f in range(5):
        rms, mism = assert_parity(got[f], want[f], "group temporal frame %d" % f)
        assert mism == 0, "frame %d: %d floats differ (rms %s)" % (f, mism, rms)


def test_history_starts_again_where_it_does_on_one_context(one, scenes):
    """a size change and a temporalSamples change reset both the group's and the one context's history; a change of tile_rows the group's
    (the one context is reset by hand there); flx_group_temporal_reset: the next frame equals frame 0 of a fresh run"""
    from flexlight_hip import capi
    sc = scenes("cornell")
    one.update_scene(sc)
    base = temporal_params(sc, 96, 72, 4, 1, 3, 0, 1)
    seq = [copy_params(base, random_seed=float(f % 4)) for f in range(3)]
    seq += [copy_params(base, width=80, height=64, random_seed=float(f % 4)) for f in range(3)]             # new size
    seq += [copy_params(base, width=80, height=64, temporal_samples=3, random_seed=float(f % 3)) for f in range(3)]      # another depth
    for q in seq[3:]:
        q.view_matrix[:] = sc.frame_params(width=q.width, height=q.height).view_matrix[:]
    want = single_frames(one, seq)
    with capi.Group([0, 0, 0]) as g:
        g.update_scene(sc)
        got = group_frames(g, seq, 8)
        for f, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b, equal_nan=True), "frame %d" % f
        # another tile_rows: the group's history starts again — like a reset one context
        more = [copy_params(seq[-1], random_seed=float(f % 3)) for f in range(3)]
        one.temporal_reset()
        want_more = [one.render(q)[0] for q in more]
        got_more = group_frames(g, more, 5)
        for f, (a, b) in enumerate(zip(got_more, want_more)):
            assert np.array_equal(a, b, equal_nan=True), "tile_rows 5 frame %d" % f
        # flx_group_temporal_reset: the next frame equals frame 0 of a fresh run (and without it, it does not)
        assert not np.array_equal(group_frames(g, [more[0]], 5)[0], want_more[0])
        g.temporal_reset()
        again = group_frames(g, [more[0]], 5)[0]
        assert np.array_equal(again, want_more[0], equal_nan=True)


def test_strips_of_single_contexts_stitch_to_the_whole_frame(scenes):
    """one context per tile, K temporal frames each: the rows of every context (flx_tile_row_at) put together equal the whole frame"""
    from flexlight_hip import capi
    sc = scenes("dragon")
    p = temporal_params(sc, 120, 61, 4, 1, 3, 0, 1)
    whole = capi.Context(0)
    ctxs = [capi.Context(0) for _ in range(3)]
    try:
        for c in [whole] + ctxs:
            c.update_scene(sc)
        for f in range(6):
            q = copy_params(p, random_seed=float(f % 4))
            want = whole.render(q)[0]
            got = np.zeros_like(want)
            for r, c in enumerate(ctxs):
                t = copy_params(q, tile_rows=8, tile_index=r, tile_count=3)
                part = c.render(t)[0]
                rows = capi.Context.tile_rows(t)
                assert part.shape[0] == len(rows)
                got[rows] = part
            assert np.array_equal(got, want, equal_nan=True), "frame %d" % f
    finally:
        for c in [whole] + ctxs:
            c.close()


def test_a_context_that_switches_tile_layout_starts_fresh(scenes):
    """the ring is keyed by the tile policy: strips of the same row count but another tile_index are a fresh history.  Strips of one row, so that a
    packed row of one layout is the image row next to the other's: neighbouring pixels often share a location id, and a stale history would count"""
    from flexlight_hip import capi
    sc = scenes("dragon")
    p = temporal_params(sc, 96, 64, 4, 1, 3, 0, 1)
    a, b = capi.Context(0), capi.Context(0)
    try:
        a.update_scene(sc)
        b.update_scene(sc)
        for f in range(3):
            a.render(copy_params(p, random_seed=float(f), tile_rows=1, tile_index=0, tile_count=2))
            b.render(copy_params(p, random_seed=float(f), tile_rows=1, tile_index=1, tile_count=2))
        q = copy_params(p, random_seed=3.0, tile_rows=1, tile_index=1, tile_count=2)
        got = a.render(q)[0]
        with_history = b.render(q)[0]
        b.temporal_reset()
        fresh = b.render(q)[0]
        assert got.shape == (32, 96, 4)
        assert not np.array_equal(with_history, fresh)       # (the history of these rows does change the frame)
        assert np.array_equal(got, fresh, equal_nan=True)
        # ... and a context given no rows does nothing
        idle = copy_params(p, height=16, random_seed=0.0, tile_rows=8, tile_index=2, tile_count=3)
        assert a.render(idle)[0].shape == (0, 96, 4)
    finally:
        a.close()
        b.close()


def test_tiled_temporal_filter_frames_are_refused(one, scenes):
    from flexlight_hip import capi
    sc = scenes("cornell")
    one.update_scene(sc)
    p = copy_params(temporal_params(sc, 64, 64, 4, 1, 2, 1, 1), tile_rows=8, tile_index=0, tile_count=2)
    with pytest.raises(capi.FlexLightHipError, match="tiled"):
        one.render(p)


def test_the_stateless_entry_points_still_refuse_temporal_frames(scenes):
    from flexlight_hip import capi
    sc = scenes("cornell")
    p = temporal_params(sc, 64, 48, 4, 1, 2, 0, 1)
    with capi.Group([0, 0]) as g:
        g.update_scene(sc)
        with pytest.raises(capi.FlexLightHipError, match="temporal"):
            g.render(p)
        with pytest.raises(capi.FlexLightHipError, match="temporal"):
            g.render_rgba8(p)
        with pytest.raises(capi.FlexLightHipError, match="FLX_FRAME_DEVICE"):
            g.frame_begin(p, device=True)
