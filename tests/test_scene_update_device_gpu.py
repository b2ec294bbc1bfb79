"""flx_scene_update_device (k_rows_check_stage in csrc/flx_refit.hip): flx_scene_update for rows that are in device memory, checked there by a kernel.

The yardstick is never the code under test: the four scene arrays (flx_debug_scene_read) are held, bit for bit, against a FRESH context that received the
re-flattened scene through flx_scene_upload, and every refusal against what the host call flx_scene_update answers for the same rows on a second context
(and against the rules restated in numpy, scene_update_device_util.refusal).  The rows are torch tensors made with torch.from_numpy(rows).cuda().  The
shapes are the smallest at which the kernel's indexing can go wrong: it runs a lane per 16 bytes in workgroups of 256 (85 1/3 rows) and reduces per wave of 64
lanes (21 1/3 rows), so spans of 1, 63, 64, 65 and 257 rows, spans from rows 0, 1, 255 and 256, and offending rows at 0, 64, 255 and the end of 300."""
import ctypes as C

import numpy as np
import pytest
import torch

import synth_scene
from flexlight_hip import capi
from parity_util import bit_mismatches
from scene_update_device_util import FAST_BOX_BOUND, MESSAGES, POSITIONS, SPAN, is_box, is_triangle, refusal, refusal_cases, span_with
from scene_update_util import TRIANGLE, bits, by_hand, chain, moved, reflatten, rows_for_update, with_geometry

pytestmark = pytest.mark.gpu

W, H = 64, 48
OK, INVALID, NO_SCENE = 0, 1, 3
WHICH = ("geometry", "attributes", "walk", "fwd")


def entries(scene):
    return scene.arrays["geometry"].size // 12


def arrays_of(ctx, scene):
    return {w: ctx.scene_read(w, entries(scene) if w in ("geometry", "attributes") else None) for w in WHICH}


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


def on_device(rows):
    return torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda()


def update(ctx, scene, first=0, count=None, attributes=True, device=True):
    """rows [first, first + count) of `scene` (box rows with noise for their six floats) handed over in device memory, or device=False through the host call"""
    g, a = rows_for_update(scene, first, entries(scene) - first if count is None else count)
    if device:
        ctx.update_scene_rows_device(first, on_device(g), on_device(a) if attributes else None)
    else:
        ctx.update_scene_rows(first, g, a if attributes else None)


def render_fresh(scene, p):
    with capi.Context(0) as fresh:
        fresh.update_scene(scene)
        return fresh.render(p)[0]


def hand_scenes():
    return {
        "two": lambda: by_hand([("box", 1, None), ("tri", TRIANGLE)]),
        "257": lambda: synth_scene.make_sized(257, 1, seed=3, width=W, height=H),
        "5000": lambda: synth_scene.make_sized(5000, 3, seed=5, width=W, height=H),
        "chain40": lambda: chain(40),
    }


@pytest.fixture(scope="module")
def big():
    return synth_scene.make_sized(5000, 3, seed=5, width=W, height=H)


@pytest.fixture(scope="module")
def big_moved(big):
    return moved(big, 11)


# ---- arrays ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["two", "257", "5000", "chain40"])
def test_all_rows_updated_from_device_memory_equal_a_fresh_upload(name):
    old = hand_scenes()[name]()
    new = moved(old, 21)
    with capi.Context(0) as ctx:
        ctx.update_scene(old)
        update(ctx, new)
        assert_arrays_equal_a_fresh_upload(ctx, new)


def spans(g):
    """name -> (first, count) in the 5 000-entry scene (5 120 rows, the last 120 of them terminators)"""
    boxes, live = np.flatnonzero(g[:, 10] == 1), np.flatnonzero(g[:, 10] != 0)
    out = {"%d rows" % n: (300, n) for n in (1, 63, 64, 65, 257)}
    out.update({"from row %d" % f: (f, 70) for f in (0, 1, 255, 256)})
    out["to the last live row"] = (int(live[-1]) - 99, 100)
    first = int(boxes[boxes > 700][0])
    out["box to box"] = (first, int(boxes[boxes > 1900][0]) - first + 1)
    out["terminators"] = (int(live[-1]) - 9, 40)
    return out


SPANS = ["1 rows", "63 rows", "64 rows", "65 rows", "257 rows", "from row 0", "from row 1", "from row 255", "from row 256", "to the last live row", "box to box",
         "terminators"]


@pytest.mark.parametrize("span", SPANS)
def test_a_span_of_rows_updated_from_device_memory_equals_a_fresh_upload(big, span):
    g = big.arrays["geometry"].reshape(-1, 12)
    first, count = spans(g)[span]
    assert sorted(spans(g)) == sorted(SPANS)
    new = moved(big, 31, rows=slice(first, first + count))
    if span == "box to box":
        assert g[first, 10] == 1 and g[first + count - 1, 10] == 1
    if span == "to the last live row":
        assert g[first + count - 1, 10] != 0 and g[first + count, 10] == 0
    if span == "terminators":                               # words 6 and 9 of a terminator are free to differ: they arrive as they are given
        ng = new.arrays["geometry"].reshape(-1, 12).copy()
        dead = np.flatnonzero(ng[:, 10] == 0)
        dead = dead[(dead >= first) & (dead < first + count)]
        assert dead.size == 30
        ng[dead, 6], ng[dead, 9] = 7.0, 5.0
        new = with_geometry(new, ng)
    with capi.Context(0) as ctx:
        ctx.update_scene(big)
        update(ctx, new, first, count)
        assert_arrays_equal_a_fresh_upload(ctx, new)


def test_without_attributes_the_attribute_rows_stay(big):
    new = moved(big, 51, attributes=False)
    assert (new.arrays["attributes"] == big.arrays["attributes"]).all()
    with capi.Context(0) as ctx:
        ctx.update_scene(big)
        update(ctx, new, attributes=False)
        assert_arrays_equal_a_fresh_upload(ctx, new)


def test_with_attributes_the_rows_arrive_whole(big):
    """all 28 words of every attribute row of the span replaced by another scene's (here: noise, so that no word can keep its value unnoticed)"""
    first, count = 255, 1000
    new = moved(big, 52, rows=slice(first, first + count))
    a = new.arrays["attributes"].reshape(-1, 28).copy()
    a[first:first + count] = np.random.default_rng(53).normal(size=(count, 28)).astype(np.float32)
    assert (bits(a[first:first + count]) != bits(big.arrays["attributes"].reshape(-1, 28)[first:first + count])).all()
    new = with_geometry(new, new.arrays["geometry"], a)
    with capi.Context(0) as ctx:
        ctx.update_scene(big)
        update(ctx, new, first, count)
        assert_arrays_equal_a_fresh_upload(ctx, new)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------

def device_answer(ctx, first, g, a=None):
    """(status, flx_last_error) of flx_scene_update_device for these rows"""
    tg, ta = on_device(g), None if a is None else on_device(a)
    rc = capi.LIB.flx_scene_update_device(ctx._h, first, tg.shape[0], C.c_void_p(tg.data_ptr()), None if ta is None else C.c_void_p(ta.data_ptr()), None)
    return rc, capi.LIB.flx_last_error(ctx._h).decode()


def host_answer(ctx, first, g, a=None):
    g = np.ascontiguousarray(g, np.float32)
    rc = capi.LIB.flx_scene_update(ctx._h, first, g.shape[0], capi._fp(g), None if a is None else capi._fp(np.ascontiguousarray(a, np.float32)))
    return rc, capi.LIB.flx_last_error(ctx._h).decode()


class Pair:
    """the 5 000-entry scene on two contexts — one takes the device call, its twin the host call — with the arrays and a frame of the first as they are"""

    def __init__(self, scene):
        self.scene = scene
        self.g = scene.arrays["geometry"].reshape(-1, 12)
        self.a = scene.arrays["attributes"].reshape(-1, 28)
        self.p = scene.frame_params(width=W, height=H)
        self.ctx, self.twin = capi.Context(0), capi.Context(0)
        for c in (self.ctx, self.twin):
            c.update_scene(scene)
        self.arrays = arrays_of(self.ctx, scene)
        self.frame = self.ctx.render(self.p)[0]

    def refused_alike(self, first, rows, rule, attributes=False):
        a = self.a[first:first + len(rows)] if attributes else None
        got, want = device_answer(self.ctx, first, rows, a), host_answer(self.twin, first, rows, a)
        assert want == (INVALID, MESSAGES[rule]) and refusal(self.g, first, rows) == MESSAGES[rule]      # (the yardsticks agree)
        assert got == want

    def assert_untouched(self):
        after = arrays_of(self.ctx, self.scene)
        for w in WHICH:
            assert (bits(after[w]) == bits(self.arrays[w])).all(), w
        assert bit_mismatches(self.ctx.render(self.p)[0], self.frame) == 0

    def close(self):
        self.ctx.close()
        self.twin.close()


@pytest.fixture(scope="module")
def pair(big):
    pr = Pair(big)
    yield pr
    pr.close()


@pytest.mark.parametrize("case", sorted(refusal_cases()))
def test_a_refused_row_is_refused_as_the_host_call_refuses_it(pair, case):
    """the offending row at 0, 64, 255 and last of a span of 300 rows; the rows with their attribute rows for one of the four"""
    wanted, change, rule = refusal_cases()[case]
    for position in POSITIONS:
        first, at = span_with(pair.g, wanted, position)
        rows = pair.g[first:first + SPAN].copy()
        rows[at] = change(rows[at])
        pair.refused_alike(first, rows, rule, attributes=position == 64)
    pair.assert_untouched()


@pytest.mark.parametrize("gap", [1, 2, 40, 200])
def test_of_two_offending_rows_the_lower_one_is_reported(pair, gap):
    """the lower row breaks the LAST rule of the host's order, the higher row the first: the row decides, not the rule (gap 1, 2: both in one wave's lanes;
    40: in two waves of one workgroup; 200: in two workgroups)"""
    first, at = span_with(pair.g, lambda g: is_triangle(g) & np.roll(g[:, 10] != 0, -gap), 20)
    rows = pair.g[first:first + SPAN].copy()
    rows[at, 8] = np.nan
    rows[at + gap, 10] = 3.0 - rows[at + gap, 10]
    pair.refused_alike(first, rows, 3)
    rows[at, 8] = pair.g[first + at, 8]
    pair.refused_alike(first, rows, 0)                      # (the higher row alone is refused for its own rule)
    pair.assert_untouched()


def test_of_two_offended_rules_in_one_row_the_hosts_first_is_reported(pair):
    first, at = span_with(pair.g, is_triangle, 100)
    rows = pair.g[first:first + SPAN].copy()
    rows[at, 0], rows[at, 9] = np.inf, rows[at, 9] + 1      # transform number before vertices
    pair.refused_alike(first, rows, 1)
    rows[at, 10] = 1.0                                      # kind before everything (as a box it would break the skip count too)
    pair.refused_alike(first, rows, 0)
    first, at = span_with(pair.g, is_box, 100)
    rows = pair.g[first:first + SPAN].copy()
    rows[at, 6], rows[at, 9] = rows[at, 6] + 1, rows[at, 9] + 1      # a box: transform number before skip count
    pair.refused_alike(first, rows, 1)
    rows[at, :6] = np.nan                                   # (a box's six floats are ignored: no offence)
    rows[at, 9] = pair.g[first + at, 9]
    pair.refused_alike(first, rows, 2)
    pair.assert_untouched()


def test_the_argument_checks_are_the_host_calls(big, pair):
    n = entries(big)
    g = pair.g
    with capi.Context(0) as empty:
        assert device_answer(empty, 0, g[:1]) == (NO_SCENE, "flx_scene_update before flx_scene_upload")
    for first, rows in ((n - 1, g[:2]), (n, g[:1])):
        got = device_answer(pair.ctx, first, rows)
        assert got == host_answer(pair.twin, first, rows) and got[0] == INVALID and "leave the entry array" in got[1]
    tg = on_device(g[:4])
    call = capi.LIB.flx_scene_update_device
    assert call(pair.ctx._h, n + 1, 0, C.c_void_p(tg.data_ptr()), None, None) == INVALID      # (a range that leaves the array, even of no rows: as the host call)
    assert call(pair.ctx._h, 0, 0, None, None, None) == OK                                   # no rows: nothing
    assert call(pair.ctx._h, 0, 4, None, None, None) == INVALID
    assert capi.LIB.flx_last_error(pair.ctx._h).decode() == "flx_scene_update: geometry is NULL"
    pair.assert_untouched()
    assert device_answer(pair.ctx, 0, g[:4])[0] == OK                                        # the same rows again are taken
    pair.assert_untouched()


def test_a_scene_uploaded_with_a_nan_vertex_takes_no_updates():
    sc = by_hand([("box", 2, None), ("tri", TRIANGLE), ("tri", [v + 1.0 for v in TRIANGLE])])
    g = sc.arrays["geometry"].reshape(-1, 12).copy()
    g[1, 2] = np.nan
    with capi.Context(0) as ctx, capi.Context(0) as twin:
        for c in (ctx, twin):
            c.update_scene(with_geometry(sc, g))
        got = device_answer(ctx, 2, g[2:3])
        assert got == host_answer(twin, 2, g[2:3]) and got[0] == INVALID and "NaN" in got[1]
        ctx.update_scene(sc)
        assert device_answer(ctx, 2, g[2:3])[0] == OK


# ---- pointers -------------------------------------------------------------------------------------------------------------------------------------------

def test_rows_that_are_not_in_the_devices_memory_are_refused(pair):
    g = np.ascontiguousarray(pair.g[:SPAN])
    a = np.ascontiguousarray(pair.a[:SPAN])
    tg, ta = on_device(np.concatenate([g, g])), on_device(a)      # (room behind the rows for the offset pointer)
    call = lambda gp, ap=None: capi.LIB.flx_scene_update_device(pair.ctx._h, 0, SPAN, C.c_void_p(gp), None if ap is None else C.c_void_p(ap), None)
    message = "flx_scene_update_device: the rows are not in memory of the context's device, 16-byte aligned"
    for gp, ap in ((g.ctypes.data, None), (tg.data_ptr(), a.ctypes.data), (tg.data_ptr() + 4, None), (tg.data_ptr(), ta.data_ptr() + 4)):
        assert call(gp, ap) == INVALID
        assert capi.LIB.flx_last_error(pair.ctx._h).decode() == message
    with pytest.raises(capi.FlexLightHipError, match="not in memory"):
        pair.ctx.update_scene_rows_device(0, (g.ctypes.data, SPAN))
    pair.assert_untouched()
    assert call(tg.data_ptr(), ta.data_ptr()) == OK
    pair.assert_untouched()


def test_the_binding_refuses_tensors_of_another_shape_type_or_place(pair):
    t = on_device(pair.g[:SPAN])
    for bad in (t.double(), t.reshape(-1), t[:, :11], t.t(), t.cpu(), pair.g[:SPAN]):
        with pytest.raises((ValueError, TypeError)):
            pair.ctx.update_scene_rows_device(0, bad)
    with pytest.raises(ValueError):
        pair.ctx.update_scene_rows_device(0, t, on_device(pair.a[:SPAN - 1]))
    pair.assert_untouched()


def test_a_tensor_on_another_device_is_refused(pair):
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    t = torch.from_numpy(np.ascontiguousarray(pair.g[:SPAN])).to("cuda:1")
    rc = capi.LIB.flx_scene_update_device(pair.ctx._h, 0, SPAN, C.c_void_p(t.data_ptr()), None, None)
    assert rc == INVALID and "not in memory of the context's device" in capi.LIB.flx_last_error(pair.ctx._h).decode()
    with pytest.raises(ValueError):
        pair.ctx.update_scene_rows_device(0, t)
    pair.assert_untouched()


# ---- the fast box test's bound ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("beyond", [False, True])
def test_a_vertex_at_the_fast_box_bound_keeps_the_flag_and_the_next_float_clears_it(big, big_moved, beyond):
    g = big_moved.arrays["geometry"].reshape(-1, 12).copy()
    t = int(np.flatnonzero(g[:, 10] == 2)[100])
    g[t, 8] = np.nextafter(FAST_BOX_BOUND, np.float32(np.inf)) if beyond else FAST_BOX_BOUND
    assert float(FAST_BOX_BOUND) == 2.0 ** 59
    far = with_geometry(big_moved, reflatten(g))
    p = far.frame_params(width=W, height=H)
    with capi.Context(0) as ctx:
        ctx.update_scene(big)
        assert ctx.walk_fast_boxes() == 1
        update(ctx, far)
        assert ctx.walk_fast_boxes() == (0 if beyond else 1)
        assert_arrays_equal_a_fresh_upload(ctx, far)
        assert bit_mismatches(ctx.render(p)[0], render_fresh(far, p)) == 0
        update(ctx, big_moved)                              # back inside the bound: a cleared flag stays cleared until a full upload, the frame is the same
        assert ctx.walk_fast_boxes() == (0 if beyond else 1)
        assert bit_mismatches(ctx.render(p)[0], render_fresh(big_moved, p)) == 0


# ---- ordering -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes,served", [(1, False), (2, False), (2, True), (3, True)])
def test_a_frame_begun_before_the_update_shows_the_old_scene(big, big_moved, lanes, served):
    """frame_begin (old), update, frame_begin (new), end both — tests/test_scene_update_gpu.py's loop with the rows in device memory"""
    p = big.frame_params(width=W, height=H)
    want_old, want_new = render_fresh(big, p), render_fresh(big_moved, p)
    with capi.Context(0) as ctx:
        ctx.set_frame_lanes(lanes)
        ctx.set_frame_chain(3 if served else 0)
        ctx.update_scene(big)
        for rep in range(2):                                # (the second time round the twin exists and the update finds frames of both lanes)
            new = big_moved if rep == 0 else big
            if rep == 1:
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


@pytest.mark.parametrize("order", ["device device", "device host", "host device"])
def test_two_updates_in_a_row_share_the_stage(big, order):
    """no synchronisation between them, and a frame in flight in front of the first so that its scatter has not run when the second call begins: the second
    may overwrite the staged rows only when the first has consumed them"""
    first = moved(big, 61)
    second = moved(first, 62, rows=slice(1000, 3000))
    p = big.frame_params(width=W, height=H)
    kinds = [k == "device" for k in order.split()]
    with capi.Context(0) as ctx:
        ctx.set_frame_lanes(1)
        ctx.update_scene(big)
        ctx.frame_begin(p)
        update(ctx, first, device=kinds[0])
        update(ctx, second, 1000, 2000, device=kinds[1])
        ctx.frame_end()
        assert_arrays_equal_a_fresh_upload(ctx, second)


def test_rows_a_torch_stream_is_still_writing_are_waited_for(big):
    """the rows are the result of a torch op on a side stream, enqueued behind enough work that it has not run when the call is made; the call is given the
    stream and the host does not wait"""
    g, a = rows_for_update(big, 0, entries(big))
    delta = np.zeros_like(g)
    tri = g[:, 10] == 2
    delta[tri, :9] = np.random.default_rng(71).normal(scale=0.2, size=(int(tri.sum()), 9)).astype(np.float32)
    want = with_geometry(big, reflatten(g + delta))         # (one float32 addition per word, here as there; the boxes' noise is not looked at)
    rows_old, d = on_device(g), on_device(delta)
    busy = torch.ones(1 << 25, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with capi.Context(0) as ctx:
        ctx.update_scene(big)
        with torch.cuda.stream(side):
            for _ in range(50):
                busy.sin_()
            rows = rows_old + d
        ctx.update_scene_rows_device(0, rows, stream=side)
        assert_arrays_equal_a_fresh_upload(ctx, want)
    side.synchronize()
