"""flx_scene_splice_device on the GPU: after every accepted splice the context holds, bit for bit, what a second context holds that was given the arrays of the
numpy restatement (scene_splice_util.splice_rule, which test_scene_splice_cpu.py holds against the flatten) through flx_scene_upload — the geometry and attribute
rows, both derived copies, the ids — and renders the same frame with the same work counters; a refused splice says what the table says and leaves all of it as
it was."""
import ctypes as C

import numpy as np
import pytest
import torch

from flexlight_hip import capi
from parity_util import bit_mismatches
from scene_splice_util import (BEYOND_MESSAGE, CUT, DIRECT, H, IDS, MESSAGES, NAN_MESSAGE, NO_PARENT, NO_SCENE_MESSAGE, NOTHING_MESSAGE, PARENT, POINTER_MESSAGE,
                               SIZE_MESSAGE, W, base_scene, end_of, mesh, padded, refusal, splice_rule, triangles, with_arrays)
from scene_update_util import bits, reflatten_by_rule
from scene_upload_device_util import MESSAGES as UPLOAD_MESSAGES, SKIP, TRANSFORM, TYPE
from tree_build_util import face_order_rows, host_block, random_soup

pytestmark = pytest.mark.gpu

OK, INVALID, NO_SCENE = 0, 1, 3                                      # FLX_OK, FLX_ERR_INVALID, FLX_ERR_NO_SCENE
WHICH = ("geometry", "attributes", "walk", "fwd")
ROWS_LANES = 256                                                    # k_splice_rows: lanes per workgroup, a lane per 16 bytes


def on_device(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def arrays(scene):
    return scene.arrays["geometry"].reshape(-1, 12), scene.arrays["attributes"].reshape(-1, 28), scene.arrays["ids"]


def state_of(ctx, scene):
    """the five arrays of flx_debug_scene_read, and the scalars beside them"""
    n = scene.arrays["geometry"].size // 12
    out = {w: ctx.scene_read(w, n if w in ("geometry", "attributes") else None) for w in WHICH}
    out["ids"] = ctx.scene_read("ids", scene.arrays["ids"].size).astype(np.float32)      # (ids are below 2^24)
    one_more = np.zeros(scene.arrays["ids"].size + 1, np.float32)
    assert capi.LIB.flx_debug_scene_read(ctx._h, 4, capi._fp(one_more), one_more.size) == INVALID, "the context holds more ids"
    assert capi.LIB.flx_debug_scene_read(ctx._h, 0, capi._fp(np.zeros(12 * n + 1, np.float32)), 12 * n + 1) == INVALID, "the context holds more entries"
    sizes = ctx.last_walk_lds()
    out["sizes"] = np.array([sizes["walk_hot"], sizes["walk_entries"], sizes["fwd_entries"]], np.float32)
    out["fast"] = np.array([ctx.walk_fast_boxes()], np.float32)
    return out


def assert_states_equal(got, want):
    for w in want:
        assert got[w].shape == want[w].shape, w
        if got[w].size == 0:
            continue
        bad = np.flatnonzero((bits(got[w]) != bits(want[w])).reshape(got[w].shape[0], -1).any(axis=1))
        assert bad.size == 0, "%s: %d rows differ, first %d: %s vs %s" % (w, bad.size, bad[0], got[w][bad[0]], want[w][bad[0]])


def block_tensors(block, with_ids=True):
    if block is None:
        return None, None, None
    return on_device(block[0]), on_device(block[1]), on_device(block[2], np.int32) if with_ids and len(block[2]) else None


class Pair:
    """two contexts for the whole module: `device` takes the splices, `host` the expected arrays through flx_scene_upload"""

    def __init__(self):
        self.device, self.host = capi.Context(0), capi.Context(0)

    def close(self):
        self.device.close()
        self.host.close()

    def assert_same(self, want):
        assert_states_equal(state_of(self.device, want), state_of(self.host, want))
        p = want.frame_params(width=W, height=H, samples=1, max_reflections=2)
        got_frame, got_counters, _ = self.device.render(p, counters=True)
        want_frame, want_counters, _ = self.host.render(p, counters=True)
        assert bit_mismatches(got_frame, want_frame) == 0 and got_counters == want_counters
        return want_frame

    def spliced(self, scene, first, n_old, parent, block=None, with_ids=True):
        """`scene` uploaded, spliced on the device; the rule's arrays uploaded to the host context; both compared -> (the expected scene, its frame)"""
        g, a, ids = arrays(scene)
        want = with_arrays(scene, *splice_rule(g, a, ids, first, n_old, parent, block, block_ids=with_ids))
        assert refusal(g, ids, first, n_old, parent) is None
        self.device.update_scene(scene)
        self.host.update_scene(want)
        self.device.splice_scene_device(first, n_old, None if parent == NO_PARENT else parent, *block_tensors(block, with_ids))
        return want, self.assert_same(want)


@pytest.fixture(scope="module")
def pair():
    pr = Pair()
    yield pr
    pr.close()


@pytest.fixture(scope="module")
def base():
    return base_scene()


# ---- replace ----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("triangles_in_block", [57, 6])
def test_a_block_three_boxes_deep_is_replaced(pair, base, triangles_in_block):
    """B inside V inside W inside the root: three skip counts change, by a larger block and by a smaller one"""
    scene, where, box = base
    block = mesh(triangles_in_block, 41)
    assert (block[0].shape[0] > where["B"][1]) == (triangles_in_block == 57)
    want, frame = pair.spliced(scene, *where["B"], box["V"], block)
    g = want.arrays["geometry"].reshape(-1, 12)
    delta = block[0].shape[0] - where["B"][1]
    for name in ("root", "W", "V"):
        assert g[box[name], 6] == arrays(scene)[0][box[name], 6] + delta
    pair.host.update_scene(scene)
    p = scene.frame_params(width=W, height=H, samples=1, max_reflections=2)
    assert bit_mismatches(pair.host.render(p)[0], frame) > 0          # (the block is in view)


def test_the_padding_follows_the_last_entry(pair, base):
    scene, where, box = base
    end = end_of(arrays(scene)[0])
    assert 256 < end < 512
    over, _ = pair.spliced(scene, end, 0, 0, triangles(512 - end + 1, 44))                   # one entry over a multiple of 256
    assert over.arrays["geometry"].size // 12 == 768
    exact, _ = pair.spliced(scene, end, 0, NO_PARENT, triangles(512 - end, 45))              # ends on one: no row of zeros behind the last entry
    assert exact.arrays["geometry"].size // 12 == 512 and exact.arrays["geometry"].reshape(-1, 12)[511, 10] == 2
    whole_w = 1 + int(arrays(scene)[0][box["W"], 6])
    assert end - whole_w < 256
    under, _ = pair.spliced(scene, box["W"], whole_w, 0)                                      # back under one
    assert under.arrays["geometry"].size // 12 == 256


# ---- insert -----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("place", ["appended to the root", "the root's first child", "at top level behind everything"])
def test_a_block_is_inserted(pair, base, place):
    scene, where, box = base
    end = end_of(arrays(scene)[0])
    first, parent = {"appended to the root": (end, 0), "the root's first child": (1, 0), "at top level behind everything": (end, NO_PARENT)}[place]
    want, _ = pair.spliced(scene, first, 0, parent, mesh(23, 46))
    assert want.arrays["geometry"].reshape(-1, 12)[0, 6] == arrays(scene)[0][0, 6] + (0 if parent == NO_PARENT else mesh(23, 46)[0].shape[0])


# ---- remove -----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,parent", [("B", "V"), ("E", "root"), ("D", "U")])
def test_a_block_is_removed(pair, base, name, parent):
    """a middle block; the last block of the scene; the only child of a box, which stays with skip count 0 and its six floats"""
    scene, where, box = base
    want, _ = pair.spliced(scene, *where[name], box[parent])
    if name == "D":
        g, old = want.arrays["geometry"].reshape(-1, 12), arrays(scene)[0]
        assert g[box["U"], 10] == 1 and g[box["U"], 6] == 0 and (bits(g[box["U"], :6]) == bits(old[box["U"], :6])).all()


# ---- lane counts, ids ---------------------------------------------------------------------------------------------------------------------------------------

def test_a_block_that_ends_inside_a_workgroup_in_front_of_a_tail_of_one_row(pair, base):
    scene, where, box = base
    block = mesh(11, 47)
    rows = block[0].shape[0]
    assert rows * 3 % ROWS_LANES and rows * 7 % ROWS_LANES
    assert where["F"][0] + where["F"][1] + 1 == end_of(arrays(scene)[0])      # behind F: E, one row
    pair.spliced(scene, *where["F"], box["root"], block)


def test_a_block_without_ids_and_a_scene_without(pair, base):
    scene, where, box = base
    want, _ = pair.spliced(scene, *where["B"], box["V"], mesh(9, 48), with_ids=False)
    assert want.arrays["ids"].size == scene.arrays["ids"].size - mesh(23, 32)[2].size
    bare = with_arrays(scene, *arrays(scene)[:2], np.zeros(0, np.int32))
    want, _ = pair.spliced(bare, *where["B"], box["V"], mesh(9, 48))
    assert np.array_equal(want.arrays["ids"], mesh(9, 48)[2] + where["B"][0])
    want, _ = pair.spliced(bare, *where["B"], box["V"], mesh(9, 48), with_ids=False)
    assert want.arrays["ids"].size == 0


def test_replace_mesh_device_builds_the_block_and_splices_it(pair, base):
    scene, where, box = base
    soup = random_soup(300, 21, centre=(0.0, 0.0, 8.0), extent=3.0, size=0.8)
    block = host_block(soup)
    rows = face_order_rows(block, soup)
    g, a, ids = arrays(scene)
    want = with_arrays(scene, *splice_rule(g, a, ids, *where["B"], box["V"], block))
    pair.device.update_scene(scene)
    pair.host.update_scene(want)
    assert pair.device.replace_mesh_device(*where["B"], box["V"], on_device(rows[0]), on_device(rows[1])) == block[0].shape[0]
    pair.assert_same(want)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------------

def answer(ctx, first, n_old, parent, block=None, n_new=None, ids=True):
    tg, ta, ti = block_tensors(block, ids)
    vp = C.c_void_p
    rc = capi.LIB.flx_scene_splice_device(ctx._h, first, n_old, parent, vp(tg.data_ptr()) if block else None, vp(ta.data_ptr()) if block else None,
                                          (block[0].shape[0] if block else 0) if n_new is None else n_new, vp(ti.data_ptr()) if ti is not None else None,
                                          ti.shape[0] if ti is not None else 0, None)
    return rc, capi.LIB.flx_last_error(ctx._h).decode()


class Held:
    """the base scene on a context, with its state and a frame as they are"""

    def __init__(self, scene):
        self.scene = scene
        self.p = scene.frame_params(width=W, height=H, samples=1, max_reflections=2)
        self.ctx = capi.Context(0)
        self.ctx.update_scene(scene)
        self.state = state_of(self.ctx, scene)
        self.frame = self.ctx.render(self.p)[0]

    def assert_untouched(self):
        assert_states_equal(state_of(self.ctx, self.scene), self.state)
        assert bit_mismatches(self.ctx.render(self.p)[0], self.frame) == 0


@pytest.fixture(scope="module")
def held(base):
    h = Held(base[0])
    yield h
    h.ctx.close()


def test_what_is_refused_before_an_entry_is_read(held, base):
    scene, where, box = base
    block = mesh(9, 48)
    end = end_of(arrays(scene)[0])
    with capi.Context(0) as empty:
        assert answer(empty, *where["B"], box["V"], block) == (NO_SCENE, NO_SCENE_MESSAGE)
    assert answer(held.ctx, where["B"][0], 0, box["V"]) == (INVALID, NOTHING_MESSAGE)
    tg, ta, ti = block_tensors(block)
    vp, n = C.c_void_p, block[0].shape[0]
    hg = np.ascontiguousarray(block[0])

    def call(gp, ap, rows=n, ip=None, n_ids=0):
        rc = capi.LIB.flx_scene_splice_device(held.ctx._h, *where["B"], box["V"], vp(gp) if gp else None, vp(ap) if ap else None, rows, vp(ip) if ip else None, n_ids, None)
        return rc, capi.LIB.flx_last_error(held.ctx._h).decode()

    refused = (INVALID, POINTER_MESSAGE)
    assert call(hg.ctypes.data, ta.data_ptr()) == refused            # a host pointer
    assert call(tg.data_ptr() + 4, ta.data_ptr()) == refused         # misaligned
    assert call(tg.data_ptr(), ta.data_ptr() + 8) == refused
    assert call(tg.data_ptr(), None) == refused and call(None, ta.data_ptr()) == refused
    assert call(tg.data_ptr(), ta.data_ptr(), ip=ti.data_ptr() + 4, n_ids=4) == refused
    assert call(tg.data_ptr(), ta.data_ptr(), ip=None, n_ids=4) == refused
    assert call(tg.data_ptr(), ta.data_ptr(), rows=1 << 27) == refused      # far beyond any allocation torch made for them
    # the rows that go must lie in front of `end`: beyond the array, and inside its padding
    assert answer(held.ctx, end, 600, NO_PARENT, block) == (INVALID, BEYOND_MESSAGE)
    assert answer(held.ctx, end, 1, 0, block) == (INVALID, BEYOND_MESSAGE)
    assert answer(held.ctx, end + 1, 0, NO_PARENT, block) == (INVALID, BEYOND_MESSAGE)
    assert answer(held.ctx, 0, end, NO_PARENT) == (INVALID, SIZE_MESSAGE)      # nothing would be left
    held.assert_untouched()


def test_every_rule_is_refused_with_its_message(held, base):
    scene, where, box = base
    g, _, ids = arrays(scene)
    block = mesh(9, 48)
    triangle = int(np.flatnonzero(g[:200, 10] == 2)[-1])
    cases = [
        (where["B"], triangle, PARENT), (where["F"], box["V"], PARENT), (where["B"], where["F"][0], PARENT), ((end_of(g), 0), box["V"], PARENT),
        (where["B"], box["W"], DIRECT), (where["B"], box["root"], DIRECT), (where["D"], NO_PARENT, DIRECT), ((where["B"][0] + 2, 0), box["W"], DIRECT),
        ((box["V"], 3), box["W"], CUT), ((where["B"][0], where["B"][1] - 1), box["V"], CUT),
    ]
    for (first, n_old), parent, rule in cases:
        assert refusal(g, ids, first, n_old, parent) == MESSAGES[rule], (first, n_old, parent)
        assert answer(held.ctx, first, n_old, parent, block) == (INVALID, MESSAGES[rule]), (first, n_old, parent)
    held.assert_untouched()


def test_of_two_broken_rules_the_first_offenders_first_is_named(held, base):
    scene, where, box = base
    g, _, ids = arrays(scene)
    block = mesh(9, 48)
    triangle = int(np.flatnonzero(g[:200, 10] == 2)[0])
    for (first, n_old), parent, rule in [((box["V"], 3), triangle, PARENT),      # an early triangle for the parent (a), rows that cut V (c)
                                         ((box["V"], 3), box["root"], DIRECT),   # W reaches them (b) before V is cut (c)
                                         ((box["U"], 2), box["V"], PARENT)]:     # V ends in front of them (a) before U is cut (c)
        assert refusal(g, ids, first, n_old, parent) == MESSAGES[rule]
        assert answer(held.ctx, first, n_old, parent, block) == (INVALID, MESSAGES[rule]), (first, n_old, parent)
    held.assert_untouched()


def test_ids_out_of_order_and_a_nan_scene_are_refused(base):
    scene, where, box = base
    g, a, ids = arrays(scene)
    block = mesh(9, 48)
    late = ids.copy()
    late[[-1, -2]] = late[[-2, -1]]
    early = ids.copy()
    early[[0, 1]] = early[[1, 0]]
    for bad_ids, (first, n_old), parent, rule in [(late, where["B"], box["V"], IDS), (late, where["B"], box["W"], DIRECT), (early, where["B"], box["W"], IDS)]:
        h = Held(with_arrays(scene, g, a, bad_ids))
        try:
            assert refusal(g, bad_ids, first, n_old, parent) == MESSAGES[rule]
            assert answer(h.ctx, first, n_old, parent, block) == (INVALID, MESSAGES[rule])
            h.assert_untouched()
        finally:
            h.ctx.close()
    nan = g.copy()
    nan[int(np.flatnonzero(g[:, 10] == 2)[7]), 4] = np.nan
    poisoned = with_arrays(scene, nan, a, ids)
    with capi.Context(0) as ctx:
        ctx.update_scene(poisoned)
        before = state_of(ctx, poisoned)
        assert answer(ctx, *where["B"], box["V"], block) == (INVALID, NAN_MESSAGE)
        assert_states_equal(state_of(ctx, poisoned), before)


def test_a_bad_block_is_refused_as_an_upload_refuses_it(held, base):
    scene, where, box = base
    good = mesh(9, 48)
    for rule in (TRANSFORM, SKIP, TYPE):
        g = good[0].copy()
        if rule == TRANSFORM:
            g[3, 9] = -1.0
        elif rule == SKIP:
            g[0, 6] = 4096.0                                        # beyond the assembled array
        else:
            g[5, 10] = 3.0
        assert answer(held.ctx, *where["B"], box["V"], (g, good[1], good[2])) == (INVALID, UPLOAD_MESSAGES[rule])
    held.assert_untouched()


# ---- ordering -----------------------------------------------------------------------------------------------------------------------------------------------

def test_rows_a_torch_stream_is_still_writing_are_waited_for(pair, base):
    scene, where, box = base
    block = mesh(57, 41)
    g, a, ids = arrays(scene)
    want = with_arrays(scene, *splice_rule(g, a, ids, *where["B"], box["V"], block))
    tg, ta, ti = block_tensors(block)
    busy = torch.ones(1 << 25, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    pair.device.update_scene(scene)
    pair.host.update_scene(want)
    with torch.cuda.stream(side):
        for _ in range(50):
            busy.sin_()
        late_g, late_a, late_i = torch.zeros_like(tg) + tg, torch.zeros_like(ta) + ta, torch.zeros_like(ti) + ti
    pair.device.splice_scene_device(*where["B"], box["V"], late_g, late_a, late_i, stream=side)
    pair.assert_same(want)
    side.synchronize()


@pytest.mark.parametrize("device_rows", [False, True])
def test_row_updates_after_a_splice_equal_a_fresh_upload(pair, base, device_rows):
    scene, where, box = base
    block = mesh(57, 41)
    want, _ = pair.spliced(scene, *where["B"], box["V"], block)
    first, rows = where["B"][0], block[0].shape[0]
    moved = block[0].copy()
    moved[moved[:, 10] == 2, :9] += np.float32(0.03125)
    moved[moved[:, 10] == 1, :6] = 99.0                             # (the device computes a box row's six floats)
    if device_rows:
        pair.device.update_scene_rows_device(first, on_device(moved))
    else:
        pair.device.update_scene_rows(first, moved)
    g, a, ids = arrays(want)
    g = g.copy()
    g[first:first + rows] = moved
    after = with_arrays(want, reflatten_by_rule(g), a, ids)
    pair.host.update_scene(after)
    pair.assert_same(after)
    bad = moved[:1].copy()
    bad[0, 6] += 1
    with pytest.raises(capi.FlexLightHipError, match="changes its skip count"):
        pair.device.update_scene_rows(first, bad)


@pytest.mark.parametrize("lanes", [1, 2])
def test_a_frame_begun_before_the_splice_shows_the_old_scene(base, lanes):
    scene, where, box = base
    block = mesh(57, 41)
    g, a, ids = arrays(scene)
    new = with_arrays(scene, *splice_rule(g, a, ids, *where["B"], box["V"], block))
    p = scene.frame_params(width=W, height=H)
    with capi.Context(0) as fresh:
        fresh.update_scene(scene)
        want_old = fresh.render(p)[0]
        fresh.update_scene(new)
        want_new = fresh.render(p)[0]
    assert bit_mismatches(want_old, want_new) > 0
    tensors = block_tensors(block)
    with capi.Context(0) as ctx:
        ctx.set_frame_lanes(lanes)
        ctx.set_frame_chain(0)
        ctx.update_scene(scene)
        for rep in range(2):                                        # (the second time round the second lane exists)
            if rep == 1:
                ctx.update_scene(scene)
                ctx.frame_begin(p)
                ctx.frame_end()
            ctx.frame_begin(p)
            ctx.splice_scene_device(*where["B"], box["V"], *tensors)
            ctx.frame_begin(p)
            before = ctx.frame_end()[0]
            after = ctx.frame_end()[0]
            assert bit_mismatches(before, want_old) == 0, "the frame begun before the splice"
            assert bit_mismatches(after, want_new) == 0, "the frame begun after the splice"
