"""flx_scene_update (csrc/flx_refit.hip): rows of the uploaded scene replaced and every box refitted on the device.

The yardstick throughout is a FRESH context that received the re-flattened scene through flx_scene_upload — today's path: host flatten, build_threaded,
build_lockstep, five synchronous copies.  Min and max are exact, so everything is compared bit for bit: the four scene arrays (flx_debug_scene_read), frames and
work counters of every kernel family the arrays feed, the frame loop on one and two lanes and through the frame server, a device group.  The scenes are the
smallest at which a kernel can go wrong: two entries; 257 (a subtree crosses a block of 256); 5 000 over three transforms (past HOT_MAX = 4096: the threaded order
is not the original order); 40 nested boxes; a box that skips nothing; zeros of both signs; a vertex beyond the fast box test's bound."""
import numpy as np
import pytest

import synth_scene
from flexlight_hip import capi
from parity_util import bit_mismatches
from scene_update_util import TRIANGLE, bits, by_hand, chain, layered, moved, reflatten, reflatten_by_rule, rows_for_update, with_geometry

pytestmark = pytest.mark.gpu

W, H = 64, 48


def arrays_of(ctx, scene):
    n = scene.arrays["geometry"].size // 12
    return {w: ctx.scene_read(w, n if w in ("geometry", "attributes") else None) for w in ("geometry", "attributes", "walk", "fwd")}


def assert_arrays_equal_a_fresh_upload(ctx, scene):
    """the device arrays of ctx against those of a fresh context that was given `scene` whole"""
    with capi.Context(0) as fresh:
        fresh.update_scene(scene)
        want, got = arrays_of(fresh, scene), arrays_of(ctx, scene)
        for w in want:
            assert got[w].shape == want[w].shape, w
            bad = np.flatnonzero((bits(got[w]) != bits(want[w])).any(axis=1))
            assert bad.size == 0, "%s: %d rows differ from a fresh upload's, first %d: %s vs %s" % (w, bad.size, bad[0], got[w][bad[0]], want[w][bad[0]])
        assert ctx.walk_fast_boxes() == fresh.walk_fast_boxes()


def update(ctx, scene, first=0, count=None, attributes=True):
    n = scene.arrays["geometry"].size // 12
    g, a = rows_for_update(scene, first, n - first if count is None else count)
    ctx.update_scene_rows(first, g, a if attributes else None)


@pytest.fixture(scope="module")
def big():
    return synth_scene.make_sized(5000, 3, seed=5, width=W, height=H)


@pytest.fixture(scope="module")
def big_moved(big):
    return moved(big, 11)


@pytest.fixture(scope="module")
def small():
    """at most 128 entries, all in transform 0: the lockstep walk over the forward-ordered copy"""
    return synth_scene.make_sized(60, 1, seed=6, width=W, height=H)


def render_fresh(scene, p, **kw):
    with capi.Context(0) as fresh:
        fresh.update_scene(scene)
        return fresh.render(p, counters=True, **kw)[:2]


# ---- arrays ---------------------------------------------------------------------------------------------------------------------------------------------

def hand_scenes():
    return {
        "two": lambda: by_hand([("box", 1, None), ("tri", TRIANGLE)]),
        "257": lambda: synth_scene.make_sized(257, 1, seed=3, width=W, height=H),
        "5000": lambda: synth_scene.make_sized(5000, 3, seed=5, width=W, height=H),
        "chain40": lambda: chain(40),
    }


@pytest.mark.parametrize("name", ["two", "257", "5000", "chain40"])
def test_all_rows_updated_equal_a_fresh_upload(name):
    old = hand_scenes()[name]()
    new = moved(old, 21)
    with capi.Context(0) as ctx:
        ctx.update_scene(old)
        update(ctx, new)
        assert_arrays_equal_a_fresh_upload(ctx, new)


def test_boxes_over_whole_blocks_and_superblocks_equal_a_fresh_upload():
    """198 808 entries: the refit's second level — boxes whose whole blocks end inside a superblock of 256 blocks, reach its end, cross into the next, cover whole ones"""
    old = layered()
    g = old.arrays["geometry"].reshape(-1, 12)
    ends = np.flatnonzero((g[:, 10] == 1) & (g[:, 6] > 256))
    blocks = np.stack([(ends + 1 + 255) // 256, (ends + g[ends, 6].astype(np.int64) + 1) // 256 - 1], 1)      # first and last whole block of each
    assert (blocks[:, 0] // 256 != blocks[:, 1] // 256).sum() >= 3 and (blocks[:, 0] // 256 == blocks[:, 1] // 256).sum() >= 3
    assert blocks[0, 1] // 256 - blocks[0, 0] // 256 >= 2                 # the root: whole superblocks between
    new = moved(old, 22, flatten=reflatten_by_rule)
    with capi.Context(0) as ctx:
        ctx.update_scene(old)
        update(ctx, new)
        assert_arrays_equal_a_fresh_upload(ctx, new)
        update(ctx, old, 70000, 5)                           # a few rows in the middle: everything above them follows
        part = old.arrays["geometry"].reshape(-1, 12).copy()
        keep = new.arrays["geometry"].reshape(-1, 12)
        part[:70000], part[70005:] = keep[:70000], keep[70005:]
        att = new.arrays["attributes"].reshape(-1, 28).copy()
        att[70000:70005] = old.arrays["attributes"].reshape(-1, 28)[70000:70005]
        assert_arrays_equal_a_fresh_upload(ctx, with_geometry(new, reflatten_by_rule(part), att))


def test_the_257_entry_scene_has_a_subtree_across_the_block():
    g = synth_scene.make_sized(257, 1, seed=3).arrays["geometry"].reshape(-1, 12)
    crossing = [i for i in range(1, 256) if g[i, 10] == 1 and i + int(g[i, 6]) >= 256]
    assert crossing, "no box but the root spans entries 255 | 256"


@pytest.mark.parametrize("span", ["first triangle", "last triangle", "box to box", "one block's last row"])
def test_a_span_of_rows_updated_equals_a_fresh_upload(big, span):
    g = big.arrays["geometry"].reshape(-1, 12)
    tris, boxes = np.flatnonzero(g[:, 10] == 2), np.flatnonzero(g[:, 10] == 1)
    if span == "first triangle":
        first, count = int(tris[0]), 1
    elif span == "last triangle":
        first, count = int(tris[-1]), 1
    elif span == "box to box":                              # both ends are box rows, well inside the array and in different blocks
        first = int(boxes[boxes > 700][0])
        count = int(boxes[boxes > 1900][0]) - first + 1
        assert g[first, 10] == 1 and g[first + count - 1, 10] == 1
    else:
        first, count = 255, 2                               # rows 255 and 256
    new = moved(big, 31, rows=slice(first, first + count))
    with capi.Context(0) as ctx:
        ctx.update_scene(big)
        update(ctx, new, first, count)
        assert_arrays_equal_a_fresh_upload(ctx, new)


def test_a_box_that_skips_nothing_keeps_its_floats():
    keep = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    old = by_hand([("box", 3, None), ("box", 0, keep), ("tri", TRIANGLE), ("tri", [v + 1.0 for v in TRIANGLE])])
    new = moved(old, 41)
    assert (new.arrays["geometry"].reshape(-1, 12)[1, :6] == keep).all()
    with capi.Context(0) as ctx:
        ctx.update_scene(old)
        update(ctx, new)                                    # (hands noise in words 0..5 of both boxes)
        assert (ctx.scene_read("geometry", 4)[1, :6] == np.float32(keep)).all()
        assert_arrays_equal_a_fresh_upload(ctx, new)


@pytest.mark.parametrize("name", ["two", "257"])
def test_zeros_of_both_signs_order_as_math_min_orders_them(name):
    """-0.0 and +0.0 on one axis of a triangle (and, in the larger scene, of triangles in different blocks): the boxes above hold min -0.0, max +0.0"""
    old = hand_scenes()[name]()
    g = old.arrays["geometry"].reshape(-1, 12).copy()
    tris = np.flatnonzero(g[:, 10] == 2)
    for k, t in enumerate((tris[0], tris[-1])):
        g[t, [0, 3, 6]] = [-0.0, 0.0, 0.0] if k == 0 else [0.0, 0.0, -0.0]
    if name == "257":
        g[tris[1:-1], 0] = np.abs(g[tris[1:-1], 0]) + 1.0   # every other x lies above zero: the root's min x is a zero
        g[tris[1:-1], 3] = np.abs(g[tris[1:-1], 3]) + 1.0
        g[tris[1:-1], 6] = np.abs(g[tris[1:-1], 6]) + 1.0
    new = with_geometry(old, reflatten(g))
    root = new.arrays["geometry"].reshape(-1, 12)[0]
    assert bits(root[0:1])[0] == 0x80000000                 # min x = -0.0
    with capi.Context(0) as ctx:
        ctx.update_scene(old)
        update(ctx, new)
        assert bits(ctx.scene_read("geometry", 1)[0, 0:1])[0] == 0x80000000
        assert_arrays_equal_a_fresh_upload(ctx, new)


def test_without_attributes_the_attribute_rows_stay(big):
    new = moved(big, 51, attributes=False)
    assert (new.arrays["attributes"] == big.arrays["attributes"]).all()
    with capi.Context(0) as ctx:
        ctx.update_scene(big)
        update(ctx, new, attributes=False)
        assert_arrays_equal_a_fresh_upload(ctx, new)


def test_two_updates_in_a_row(big):
    first = moved(big, 61)
    second = moved(first, 62, rows=slice(1000, 3000))
    with capi.Context(0) as ctx:
        ctx.update_scene(big)
        update(ctx, first)
        update(ctx, second, 1000, 2000)
        assert_arrays_equal_a_fresh_upload(ctx, second)


def test_a_vertex_beyond_the_fast_box_bound_clears_the_flag_for_good(big, big_moved):
    g = big_moved.arrays["geometry"].reshape(-1, 12).copy()
    t = int(np.flatnonzero(g[:, 10] == 2)[0])
    g[t, 8] = 1e18                                          # > 2^59
    far = with_geometry(big_moved, reflatten(g))
    p = far.frame_params(width=W, height=H)
    with capi.Context(0) as ctx:
        ctx.update_scene(big)
        assert ctx.walk_fast_boxes() == 1
        update(ctx, far, t, 1)
        update(ctx, far)
        assert ctx.walk_fast_boxes() == 0
        assert_arrays_equal_a_fresh_upload(ctx, far)
        got, cnt, _ = ctx.render(p, counters=True)
        want, want_cnt = render_fresh(far, p)
        assert bit_mismatches(got, want) == 0 and cnt == want_cnt
        update(ctx, big_moved)                              # back inside the bound: the flag stays cleared until a full upload — the frame is the same
        assert ctx.walk_fast_boxes() == 0
        got, cnt, _ = ctx.render(p, counters=True)
        want, want_cnt = render_fresh(big_moved, p)
        assert bit_mismatches(got, want) == 0 and cnt == want_cnt
        ctx.update_scene(big_moved)
        assert ctx.walk_fast_boxes() == 1


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------------------

def frame_cases():
    return ["default", "lockstep", "filter", "temporal", "raster", "no angle table"]


@pytest.mark.parametrize("case", frame_cases())
def test_frames_after_an_update_equal_a_fresh_contexts(big, big_moved, small, case):
    """every family of kernels the scene arrays feed; a frame of the OLD scene is rendered first, so that whatever the context derives from the geometry
    (the shading's angle table) has to follow the update"""
    old, new = (small, moved(small, 71)) if case == "lockstep" else (big, big_moved)
    p = new.frame_params(width=W, height=H, use_filter=1 if case == "filter" else 0)
    p.is_temporal = 1 if case == "temporal" else 0

    def frame(ctx):
        if case == "raster":
            return ctx.raster_render(p, counters=True)
        return ctx.render(p, counters=True)[:2]

    with capi.Context(0) as ctx, capi.Context(0) as fresh:
        for c in (ctx, fresh):
            c.set_angle_table(case != "no angle table")
        ctx.update_scene(old)
        before = frame(ctx)
        update(ctx, new)
        if case == "temporal":
            ctx.temporal_reset()
        got = frame(ctx)
        fresh.update_scene(new)
        want = frame(fresh)
        assert bit_mismatches(got[0], want[0]) == 0 and got[1] == want[1]
        assert bit_mismatches(got[0], before[0]) != 0        # (the scene did move)
        if case == "default":
            assert ctx.last_pipeline() == 3
        if case == "lockstep":
            assert ctx.last_pipeline() == 1 and ctx.last_trace_kernel()[1] == 1


# ---- the frame loop -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes,served", [(1, False), (2, False), (2, True), (3, True)])
def test_a_frame_begun_before_the_update_shows_the_old_scene(big, big_moved, lanes, served):
    """frame_begin (old), update, frame_begin (new), end both: on one lane, on two (the second frame goes to the twin, which shares the arrays), and through the
    frame server, whose launch ends at the update and starts again"""
    p = big.frame_params(width=W, height=H)
    want_old, want_new = render_fresh(big, p)[0], render_fresh(big_moved, p)[0]
    with capi.Context(0) as ctx:
        ctx.set_frame_lanes(lanes)
        ctx.set_frame_chain(3 if served else 0)
        ctx.update_scene(big)
        for rep in range(2):                                # (the second time round the twin exists and the update finds frames of both lanes)
            new = big_moved if rep == 0 else big
            if rep == 1:                                    # (one frame more: on two lanes the frame begun before the update is now the twin's)
                ctx.frame_begin(p)
                ctx.frame_end()
            ctx.frame_begin(p)
            first_kind = ctx.last_chained()
            update(ctx, new)
            ctx.frame_begin(p)
            assert (first_kind, ctx.last_chained()) == ((3, 3) if served else (0, 0))
            a = ctx.frame_end()[0]
            b = ctx.frame_end()[0]
            assert bit_mismatches(a, want_old if rep == 0 else want_new) == 0, "the frame begun before the update"
            assert bit_mismatches(b, want_new if rep == 0 else want_old) == 0, "the frame begun after the update"


# ---- a device group -------------------------------------------------------------------------------------------------------------------------------------

def test_a_group_of_two_contexts_follows(big, big_moved):
    p = big.frame_params(width=W, height=H)
    want = render_fresh(big_moved, p)[0]
    g = capi.Group([0, 0])
    try:
        g.update_scene(big)
        g.render(p)
        rows, attrs = rows_for_update(big_moved, 0, big_moved.arrays["geometry"].size // 12)
        g.update_scene_rows(0, rows, attrs)
        got = g.render(p)[0][0]
        assert bit_mismatches(got, want) == 0
    finally:
        g.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------

def status_of(ctx, first, g, a=None):
    g = np.ascontiguousarray(g, np.float32)
    fp = lambda x: None if x is None else capi._fp(np.ascontiguousarray(x, np.float32))
    return capi.LIB.flx_scene_update(ctx._h, first, g.size // 12, fp(g), fp(a))


def test_refused_updates_leave_the_scene_as_it_was(big):
    INVALID, NO_SCENE = 1, 3
    n = big.arrays["geometry"].size // 12
    g = big.arrays["geometry"].reshape(-1, 12)
    box, tri = int(np.flatnonzero(g[:, 10] == 1)[3]), int(np.flatnonzero(g[:, 10] == 2)[3])
    p = big.frame_params(width=W, height=H)

    def changed(row, word, value):
        r = g[row:row + 1].copy()
        r[0, word] = value
        return r

    with capi.Context(0) as ctx:
        assert status_of(ctx, 0, g[:1]) == NO_SCENE
        ctx.update_scene(big)
        before = ctx.render(p)[0]
        arrays = arrays_of(ctx, big)
        assert status_of(ctx, n - 1, g[:2]) == INVALID                               # the range leaves the array
        assert status_of(ctx, n + 1, g[:0]) == INVALID
        assert status_of(ctx, box, changed(box, 6, g[box, 6] + 1)) == INVALID        # skip count
        assert status_of(ctx, box, changed(box, 9, g[box, 9] + 1)) == INVALID        # transform number, of a box and of a triangle
        assert status_of(ctx, tri, changed(tri, 9, g[tri, 9] + 1)) == INVALID
        assert status_of(ctx, tri, changed(tri, 10, 1)) == INVALID                   # kind
        assert status_of(ctx, n - 1, changed(n - 1, 10, 2)) == INVALID               # (a padding row turned triangle)
        for bad in (np.nan, np.inf, -np.inf):
            assert status_of(ctx, tri, changed(tri, 4, bad)) == INVALID              # a vertex that is not finite
        later = np.concatenate([g[tri:tri + 1], changed(tri + 1, 0, np.nan)]) if g[tri + 1, 10] == 2 else None
        if later is not None:
            assert status_of(ctx, tri, later) == INVALID                             # .. in a later row: the rows before it are not taken either
        assert b"finite" in capi.LIB.flx_last_error(ctx._h)
        assert status_of(ctx, 0, g[:0]) == 0                                         # no rows: nothing
        after = arrays_of(ctx, big)
        for w in arrays:
            assert (bits(arrays[w]) == bits(after[w])).all(), w
        assert bit_mismatches(ctx.render(p)[0], before) == 0
        assert status_of(ctx, tri, g[tri:tri + 1]) == 0                              # the same rows again are taken
        assert bit_mismatches(ctx.render(p)[0], before) == 0


def test_a_scene_uploaded_with_a_nan_vertex_takes_no_updates():
    """Math.min carries NaN into every box above; the device's min does not: refused, not guessed at"""
    sc = by_hand([("box", 2, None), ("tri", TRIANGLE), ("tri", [v + 1.0 for v in TRIANGLE])])
    g = sc.arrays["geometry"].reshape(-1, 12).copy()
    g[1, 2] = np.nan
    with capi.Context(0) as ctx:
        ctx.update_scene(with_geometry(sc, g))
        assert status_of(ctx, 2, g[2:3]) == 1
        ctx.update_scene(sc)
        assert status_of(ctx, 2, g[2:3]) == 0
