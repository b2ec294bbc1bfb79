"""flx_scene_upload_device (csrc/flx_derive.hip): flx_scene_upload for arrays that are in device memory, everything the host call decides and derives done by kernels.

The yardstick is the host call: two contexts get the same arrays, one through flx_scene_upload, the other through flx_scene_upload_device from torch tensors (over a
one-triangle scene it held before), and the four device arrays (flx_debug_scene_read), the scene's sizes (flx_debug_last_walk_lds out[4..6]), walk_fast_boxes and a
small frame are equal bit for bit.  Refusals are held against what flx_scene_upload answers for the same array and against the rules restated in numpy
(scene_upload_device_util.refusal).  The sizes are the smallest at which the kernels can go wrong: the hot cap of 4096 on both sides (with the threshold depth split
inside a level), the 256-entry borders of the scan blocks, FLX_LOCK_MAX on both sides, one and three transforms; the dragon once for the scans over more than one level.
synth_scene.make_sized makes no scene of fewer than 7 entries (9 with three transforms): the one-entry scene is a triangle by hand, and those two sizes run too."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import synth_scene
from flexlight_hip import capi
from flexlight_hip.scene_io import Scene
from parity_util import bit_mismatches
from scene_update_device_util import KIND, MESSAGES as UPDATE_MESSAGES
from scene_update_util import bits, moved, rows_for_update
from scene_upload_device_util import (FAST_BOX_BOUND, MESSAGES, POINTER_MESSAGE, POSITIONS, REFUSAL_ENTRIES, SKIP, TRANSFORM, TYPE, decoy, fractional_words,
                                      last_box_reaches_the_end, offend, one_triangle, overlapping_boxes, refusal, rows, scene_of, terminator_in_the_middle)

pytestmark = pytest.mark.gpu

W, H = 64, 48
OK, INVALID = 0, 1
WHICH = ("geometry", "attributes", "walk", "fwd")


def entries(scene):
    return scene.arrays["geometry"].size // 12


def on_device(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def tensors(scene):
    g, a = rows(scene)
    ids = scene.arrays["ids"]
    return on_device(g), on_device(a), on_device(ids, np.int32) if ids.size else None


def upload_device(ctx, scene, prior=True):
    """the scene's transforms, lights and atlases the usual way (with a one-triangle scene), then its entries from device memory"""
    if prior:
        ctx.update_scene(decoy(scene))
    ctx.upload_scene_device(*tensors(scene))


def state_of(ctx, scene):
    out = {w: ctx.scene_read(w, entries(scene) if w in ("geometry", "attributes") else None) for w in WHICH}
    sizes = ctx.last_walk_lds()
    out["sizes"] = np.array([sizes["walk_hot"], sizes["walk_entries"], sizes["fwd_entries"]], np.float32)
    out["fast"] = np.array([ctx.walk_fast_boxes()], np.float32)
    return out


def assert_states_equal(got, want):
    for w in want:
        assert got[w].shape == want[w].shape, w
        bad = np.flatnonzero((bits(got[w]) != bits(want[w])).reshape(got[w].shape[0], -1).any(axis=1))
        assert bad.size == 0, "%s: %d rows differ from the host upload's, first %d: %s vs %s" % (w, bad.size, bad[0], got[w][bad[0]], want[w][bad[0]])


def assert_same_as_the_host_upload(scene, frame=True):
    with capi.Context(0) as host, capi.Context(0) as device:
        host.update_scene(scene)
        upload_device(device, scene)
        assert_states_equal(state_of(device, scene), state_of(host, scene))
        if frame:
            p = scene.frame_params(width=W, height=H)
            assert bit_mismatches(device.render(p)[0], host.render(p)[0]) == 0
        return state_of(device, scene)


@functools.lru_cache(maxsize=None)
def sized(n, transforms):
    return synth_scene.make_sized(n, transforms, seed=n % 97, width=W, height=H)


def render_fresh(scene, p):
    with capi.Context(0) as fresh:
        fresh.update_scene(scene)
        return fresh.render(p)[0]


# ---- the central test -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cornell", "cornell_obj", "theater"])
def test_a_fixture_uploaded_from_device_memory_is_the_host_uploads_scene(name):
    assert_same_as_the_host_upload(Scene.golden(name))


SIZES = [(n, t) for n in (255, 256, 257, 4095, 4096, 4097, 5000) for t in (1, 3)] + [(127, 1), (128, 1), (7, 1), (9, 3)]


@pytest.mark.parametrize("n,transforms", SIZES)
def test_a_sized_scene_uploaded_from_device_memory_is_the_host_uploads_scene(n, transforms):
    """walk_hot = min(n, 4096) + 1; fwd_entries = n + 1: 128 and 129 at n = 127 and 128, either side of FLX_LOCK_MAX"""
    state = assert_same_as_the_host_upload(sized(n, transforms))
    assert tuple(state["sizes"]) == (min(n, 4096) + 1, n + 1, n + 1)


def test_one_entry():
    state = assert_same_as_the_host_upload(one_triangle())
    assert tuple(state["sizes"]) == (2, 2, 2)


def test_the_dragon_arrays():
    """289 189 entries: 1 130 scan blocks, hence block totals that are scanned in turn"""
    scene = Scene.golden("dragon_100k")
    assert entries(scene) > 65536
    assert_same_as_the_host_upload(scene, frame=False)


# ---- hand-made lists ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("make", [terminator_in_the_middle, last_box_reaches_the_end])
def test_a_hand_made_list(make):
    assert_same_as_the_host_upload(make())


def test_a_fractional_skip_count_and_transform_number_are_truncated():
    scene = fractional_words(sized(257, 3))
    g = scene.arrays["geometry"].reshape(-1, 12)
    assert g[1, 6] == 2.5 and g[3, 9] == 1.5
    assert_same_as_the_host_upload(scene)


def test_a_nan_vertex_carries_over_to_the_updates():
    scene = sized(257, 1)
    g, a = rows(scene)
    t = int(np.flatnonzero(g[:, 10] == 2)[40])
    g[t, 4] = np.nan
    scene = scene_of(scene, g, a)
    assert_same_as_the_host_upload(scene, frame=False)
    with capi.Context(0) as host, capi.Context(0) as device:
        host.update_scene(scene)
        upload_device(device, scene)
        answers = []
        for ctx in (host, device):
            rc = capi.LIB.flx_scene_update(ctx._h, 0, 1, capi._fp(np.ascontiguousarray(g[:1])), None)
            answers.append((rc, capi.LIB.flx_last_error(ctx._h).decode()))
        assert answers[0] == answers[1] and answers[0][0] == INVALID and "NaN" in answers[0][1]
        with pytest.raises(capi.FlexLightHipError, match="NaN"):
            device.update_scene_rows_device(0, on_device(g[:1]))


@pytest.mark.parametrize("beyond", [False, True])
def test_a_box_coordinate_beyond_the_fast_box_bound_clears_the_flag(beyond):
    scene = sized(257, 1)
    g, a = rows(scene)
    box = int(np.flatnonzero(g[:, 10] == 1)[5])
    g[box, 3] = np.nextafter(FAST_BOX_BOUND, np.float32(np.inf)) if beyond else FAST_BOX_BOUND
    state = assert_same_as_the_host_upload(scene_of(scene, g, a))
    assert state["fast"][0] == (0 if beyond else 1)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------

def device_answer(ctx, g, a, n=None):
    tg, ta = on_device(g), on_device(a)
    rc = capi.LIB.flx_scene_upload_device(ctx._h, C.c_void_p(tg.data_ptr()), C.c_void_p(ta.data_ptr()), g.shape[0] if n is None else n, None, 0, None)
    return rc, capi.LIB.flx_last_error(ctx._h).decode()


def host_answer(ctx, g, a):
    g, a = np.ascontiguousarray(g, np.float32), np.ascontiguousarray(a, np.float32)
    rc = capi.LIB.flx_scene_upload(ctx._h, capi._fp(g), capi._fp(a), g.shape[0], None, 0)
    return rc, capi.LIB.flx_last_error(ctx._h).decode()


class Pair:
    """a scene on two contexts — one takes the device call, its twin the host call — with the state and a frame of the first as they are"""

    def __init__(self, scene):
        self.scene = scene
        self.p = scene.frame_params(width=W, height=H)
        self.ctx, self.twin = capi.Context(0), capi.Context(0)
        for c in (self.ctx, self.twin):
            c.update_scene(scene)
        self.state = state_of(self.ctx, scene)
        self.frame = self.ctx.render(self.p)[0]

    def refused_alike(self, g, a, rule):
        got, want = device_answer(self.ctx, g, a), host_answer(self.twin, g, a)
        assert want == (INVALID, MESSAGES[rule]) and refusal(g) == MESSAGES[rule]      # (the yardsticks agree)
        assert got == want

    def assert_untouched(self):
        assert_states_equal(state_of(self.ctx, self.scene), self.state)
        assert bit_mismatches(self.ctx.render(self.p)[0], self.frame) == 0

    def close(self):
        self.ctx.close()
        self.twin.close()


@pytest.fixture(scope="module")
def pair():
    pr = Pair(sized(257, 3))
    yield pr
    pr.close()


@pytest.fixture(scope="module")
def candidate():
    g, a = rows(sized(REFUSAL_ENTRIES, 3))
    return g[:REFUSAL_ENTRIES], a[:REFUSAL_ENTRIES]


@pytest.mark.parametrize("rule", [TRANSFORM, SKIP, TYPE])
def test_a_refused_array_is_refused_as_the_host_call_refuses_it(pair, candidate, rule):
    """the offending entry at 0, 64, 255 and last of 300, alone and with a later offender of another rule"""
    for position in POSITIONS:
        at = REFUSAL_ENTRIES - 1 if position == "last" else position
        g, a = candidate[0].copy(), candidate[1]
        offend(g, at, rule)
        pair.refused_alike(g, a, rule)
        if at + 37 < REFUSAL_ENTRIES:
            offend(g, at + 37, (rule + 2) % 3)
            pair.refused_alike(g, a, rule)
    pair.assert_untouched()


def test_of_two_offended_rules_in_one_entry_the_hosts_first_is_reported(pair, candidate):
    g, a = candidate[0].copy(), candidate[1]
    g[100, 9], g[100, 10] = -1.0, 3.0
    pair.refused_alike(g, a, TRANSFORM)
    g[100, 10], g[100, 6] = 1.0, -1.0
    pair.refused_alike(g, a, TRANSFORM)
    g[100, 9] = 0.0
    pair.refused_alike(g, a, SKIP)
    pair.assert_untouched()


def test_the_argument_checks_are_the_host_calls(pair, candidate):
    g, a = candidate
    tg, ta = on_device(g), on_device(a)
    call = capi.LIB.flx_scene_upload_device
    message = lambda: capi.LIB.flx_last_error(pair.ctx._h).decode()
    for args in ((None, C.c_void_p(ta.data_ptr()), 300, None, 0), (C.c_void_p(tg.data_ptr()), None, 300, None, 0), (C.c_void_p(tg.data_ptr()), C.c_void_p(ta.data_ptr()), 0, None, 0)):
        assert call(pair.ctx._h, *args, None) == INVALID and message() == "flx_scene_upload: empty scene"
    assert call(pair.ctx._h, C.c_void_p(tg.data_ptr()), C.c_void_p(ta.data_ptr()), 300, None, 5, None) == INVALID and message() == "flx_scene_upload: ids is NULL"
    assert call(pair.ctx._h, C.c_void_p(tg.data_ptr()), C.c_void_p(ta.data_ptr()), 1 << 28, None, 0, None) == INVALID
    assert message() == "flx_scene_upload: more than 2^28 - 1 entries"
    pair.assert_untouched()


def test_arrays_that_are_not_in_the_devices_memory_are_refused(pair, candidate):
    """every one of these is refused by the pointer check, before a kernel is launched"""
    g, a = np.ascontiguousarray(candidate[0]), np.ascontiguousarray(candidate[1])
    n = g.shape[0]
    tg, ta, ti = on_device(np.concatenate([g, g])), on_device(np.concatenate([a, a])), on_device(np.arange(8), np.int32)
    vp = C.c_void_p

    def call(gp, ap, rows=n, ip=None, n_ids=0):
        rc = capi.LIB.flx_scene_upload_device(pair.ctx._h, vp(gp), vp(ap), rows, None if ip is None else vp(ip), n_ids, None)
        return rc, capi.LIB.flx_last_error(pair.ctx._h).decode()

    refused = (INVALID, POINTER_MESSAGE)
    assert call(g.ctypes.data, ta.data_ptr()) == refused            # a host pointer
    assert call(tg.data_ptr(), a.ctypes.data) == refused
    assert call(tg.data_ptr() + 4, ta.data_ptr()) == refused        # misaligned
    assert call(tg.data_ptr(), ta.data_ptr() + 8) == refused
    assert call(tg.data_ptr(), ta.data_ptr(), ip=ti.data_ptr() + 4, n_ids=4) == refused
    assert call(tg.data_ptr(), ta.data_ptr(), rows=1 << 27) == refused      # tensors far shorter than n_entries_padded rows (beyond any allocation torch made for them)
    with pytest.raises(capi.FlexLightHipError, match="not in memory"):
        pair.ctx.upload_scene_device((g.ctypes.data, n), ta[:n])
    pair.assert_untouched()


def test_the_binding_refuses_tensors_of_another_shape_type_or_place(pair, candidate):
    g, a = on_device(candidate[0]), on_device(candidate[1])
    for bad in (g.double(), g.reshape(-1), g[:, :11], g.t(), g.cpu(), candidate[0]):
        with pytest.raises((ValueError, TypeError)):
            pair.ctx.upload_scene_device(bad, a)
    with pytest.raises(ValueError):
        pair.ctx.upload_scene_device(g, a[:-1])
    with pytest.raises(ValueError):
        pair.ctx.upload_scene_device(g, a, on_device(np.arange(4), np.int64))
    pair.assert_untouched()


def test_after_the_refusals_the_array_itself_is_taken(pair, candidate):
    g, a = candidate
    assert device_answer(pair.ctx, g, a)[0] == OK
    with capi.Context(0) as host:
        want = scene_of(pair.scene, g, a)
        want.arrays["ids"] = np.zeros(0, np.int32)
        host.update_scene(pair.scene)
        assert host_answer(host, g, a)[0] == OK
        assert_states_equal(state_of(pair.ctx, want), state_of(host, want))
    pair.ctx.update_scene(pair.scene)                               # (the module's pair as the other tests expect it)
    pair.assert_untouched()


# ---- after a device upload ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("device_rows", [False, True])
def test_row_updates_after_a_device_upload_equal_a_fresh_host_upload(device_rows):
    old = sized(5000, 3)
    new = moved(old, 21)
    g, a = rows_for_update(new, 0, entries(new))
    with capi.Context(0) as ctx, capi.Context(0) as fresh:
        upload_device(ctx, old)
        if device_rows:
            ctx.update_scene_rows_device(0, on_device(g), on_device(a))
        else:
            ctx.update_scene_rows(0, g, a)
        fresh.update_scene(new)
        assert_states_equal(state_of(ctx, new), state_of(fresh, new))
        # their refusals are the usual ones
        live = int(np.flatnonzero(g[:, 10] == 2)[10])
        bad = g[live:live + 1].copy()
        bad[0, 10] = 1.0
        with pytest.raises(capi.FlexLightHipError, match="changes its kind"):
            ctx.update_scene_rows(live, bad)
        with pytest.raises(capi.FlexLightHipError, match="changes its kind"):
            ctx.update_scene_rows_device(live, on_device(bad))
        bad = g[live:live + 1].copy()
        bad[0, 9] += 1
        with pytest.raises(capi.FlexLightHipError, match="changes its transform number"):
            ctx.update_scene_rows(live, bad)
        bad = g[live:live + 1].copy()
        bad[0, 2] = np.inf
        with pytest.raises(capi.FlexLightHipError, match="not finite"):
            ctx.update_scene_rows_device(live, on_device(bad))
        assert_states_equal(state_of(ctx, new), state_of(fresh, new))


def test_a_host_upload_over_a_device_upload_then_takes_rows_of_both_kinds():
    """One context: a device upload (h_entry_meta left on the device), a HOST upload of another scene over it (h_entry_meta back on the host), then rows from host
    memory into one span and rows from device memory into the rest, through the one stage and the events made once; 257 and 300 entries: either side of the
    256-entry blocks of the refit and derive kernels.  A refused row in between says what the table says and changes nothing."""
    base, new = sized(300, 3), moved(sized(300, 3), 33)
    n, mid = entries(new), 137
    g, a = rows_for_update(new, 0, n)
    with capi.Context(0) as ctx, capi.Context(0) as fresh:
        upload_device(ctx, sized(257, 3))
        ctx.update_scene(base)
        ctx.update_scene_rows(0, g[:mid], a[:mid])
        before = state_of(ctx, new)
        live = mid + int(np.flatnonzero(g[mid:, 10] == 2)[3])
        bad = g[live:live + 1].copy()
        bad[0, 10] = 1.0
        assert capi.LIB.flx_scene_update(ctx._h, live, 1, capi._fp(bad), None) == INVALID
        assert capi.LIB.flx_last_error(ctx._h).decode() == UPDATE_MESSAGES[KIND]
        assert_states_equal(state_of(ctx, new), before)
        ctx.update_scene_rows_device(mid, on_device(g[mid:]), on_device(a[mid:]))
        fresh.update_scene(new)
        assert_states_equal(state_of(ctx, new), state_of(fresh, new))
        p = new.frame_params(width=W, height=H)
        assert bit_mismatches(ctx.render(p)[0], fresh.render(p)[0]) == 0


# ---- ordering -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [1, 2])
def test_a_frame_begun_before_the_upload_shows_the_old_scene(lanes):
    old = sized(5000, 3)
    other = sized(4097, 3)
    new = copy.copy(other)                                          # another topology under the old scene's transforms, lights and atlases
    new.arrays = dict(old.arrays, geometry=other.arrays["geometry"], attributes=other.arrays["attributes"], ids=other.arrays["ids"])
    new.meta = old.meta
    p = old.frame_params(width=W, height=H)
    want_old, want_new = render_fresh(old, p), render_fresh(new, p)
    assert bit_mismatches(want_old, want_new) > 0
    with capi.Context(0) as ctx:
        ctx.set_frame_lanes(lanes)
        ctx.set_frame_chain(0)
        ctx.update_scene(old)
        for rep in range(2):                                        # (the second time round the second lane exists)
            now, then = (new, old) if rep == 0 else (old, new)
            if rep == 1:
                ctx.frame_begin(p)
                ctx.frame_end()
            ctx.frame_begin(p)
            upload_device(ctx, now, prior=False)
            ctx.frame_begin(p)
            a = ctx.frame_end()[0]
            b = ctx.frame_end()[0]
            assert bit_mismatches(a, want_new if rep == 1 else want_old) == 0, "the frame begun before the upload"
            assert bit_mismatches(b, want_old if rep == 1 else want_new) == 0, "the frame begun after the upload"


def test_arrays_a_torch_stream_is_still_writing_are_waited_for():
    scene = sized(5000, 3)
    g, a, ids = tensors(scene)
    busy = torch.ones(1 << 25, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with capi.Context(0) as ctx, capi.Context(0) as host:
        host.update_scene(scene)
        ctx.update_scene(decoy(scene))
        with torch.cuda.stream(side):
            for _ in range(50):
                busy.sin_()
            late = torch.zeros_like(g) + g
        ctx.upload_scene_device(late, a, ids, stream=side)
        assert_states_equal(state_of(ctx, scene), state_of(host, scene))
    side.synchronize()


# ---- an improperly nested list --------------------------------------------------------------------------------------------------------------------------

def test_overlapping_boxes_walk_alike_under_both_uploads():
    scene = overlapping_boxes()
    rng = np.random.default_rng(5)
    rays = np.zeros((16, 7), np.float32)
    rays[:, 0:3] = [0.0, 0.0, -8.0]
    rays[:, 3:6] = np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.15, 0.15, (16, 3))
    rays[:, 6] = 30.0
    with capi.Context(0) as host, capi.Context(0) as device:
        host.update_scene(scene)
        upload_device(device, scene)
        for w in ("geometry", "attributes", "fwd"):                 # (the forward-ordered copy has no depth in it)
            assert (bits(device.scene_read(w, 6 if w != "fwd" else None)) == bits(host.scene_read(w, 6 if w != "fwd" else None))).all(), w
        hits = 0
        for variant in (0, 1):
            got, want = device.debug_walk(variant, rays), host.debug_walk(variant, rays)
            assert (bits(got) == bits(want)).all(), variant
            hits += int((want[:, 5] >= 0).sum())
        assert hits > 0
