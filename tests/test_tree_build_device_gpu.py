"""flx_tree_build_device + flx_tree_emit_device (csrc/flx_build.hip): a mesh's block of the entry array built on the device from triangle rows in device memory.

The yardstick is the host builder: flx_mesh_import_obj + flx_mesh_flatten of the same triangles in the same order (tree_build_util.host_block); the device's three
arrays equal its arrays bit for bit, all 12 + 28 words of every row and the ids.  The soups are the smallest that reach each branch of the builder
(tests/test_tree_build_cpu.py asserts that they do).  Refusals carry their own messages, the first offending row and its first rule; the end-to-end test splices a
block behind a synthetic scene and renders it beside the same arrays made on the host."""
import ctypes as C

import numpy as np
import pytest
import torch

import synth_scene
from flexlight_hip import capi
from parity_util import bit_mismatches
from scene_upload_device_util import decoy, scene_of
from tree_build_util import SOUPS, bits, case, face_order_rows, host_block, random_soup

pytestmark = pytest.mark.gpu

W, H = 64, 48
OK, INVALID = 0, 1
KIND, TRANSFORM, FINITE = 0, 1, 2
MESSAGES = (
    "flx_tree_build_device: a row is not a triangle (word 10 is not 2)",
    "flx_tree_build_device: a row's transform number (word 9) differs from row 0's or is no whole number in [0, 2^20)",
    "flx_tree_build_device: a vertex is not finite",
)
COUNT_MESSAGE = "flx_tree_build_device: n_triangles is 0 or above 2^24"
POINTER_MESSAGE = "flx_tree_build_device: the rows are not in memory of the context's device, 16-byte aligned"
NO_BUILD_MESSAGE = "flx_tree_emit_device without a successful flx_tree_build_device"
ROWS_MESSAGE = "flx_tree_emit_device: d_triangles is not the build's n_triangles rows in memory of the context's device, 16-byte aligned"
ARRAY_MESSAGE = "flx_tree_emit_device: an array is not in memory of the context's device, 16-byte aligned, or too short for the build"


def on_device(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()      # (a copy: the fixtures are read-only)


def assert_block_equals(got, want):
    for name, g, w in zip(("geometry", "attributes", "ids"), got, want):
        g = g.cpu().numpy()
        assert g.shape == w.shape, name
        g, w = (g, w) if name == "ids" else (bits(g), bits(w))
        bad = np.flatnonzero((g != w).reshape(g.shape[0], -1).any(axis=1))
        assert bad.size == 0, "%s: %d rows differ from the host builder's, first %d: %s vs %s" % (name, bad.size, bad[0], got[0][int(bad[0])] if name != "ids" else g[bad[0]], w[bad[0]])


@pytest.fixture(scope="module")
def ctx():
    with capi.Context(0) as c:
        yield c


@pytest.mark.parametrize("name", sorted(SOUPS))
def test_the_devices_block_is_the_host_builders(ctx, name):
    _, block, rows = case(name)
    triangles, attributes = on_device(rows[0]), on_device(rows[1])
    first = ctx.build_tree_device(triangles, attributes)
    assert_block_equals(first, block)
    again = ctx.build_tree_device(triangles, attributes)
    for a, b in zip(first, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_without_attributes_the_attribute_rows_are_zeros(ctx):
    _, block, rows = case("n257")
    g, a, ids = ctx.build_tree_device(on_device(rows[0]))
    assert_block_equals((g, a, ids), (block[0], np.zeros_like(block[1]), block[2]))


def test_emit_may_be_called_again_into_other_arrays(ctx):
    _, block, rows = case("n256")
    triangles, attributes = on_device(rows[0]), on_device(rows[1])
    ctx.build_tree_device(triangles, attributes)
    g, a, ids = (torch.full(block[0].shape, 7.0).cuda(), torch.full(block[1].shape, 7.0).cuda(), torch.full(block[2].shape, 7, dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    vp = C.c_void_p
    assert capi.LIB.flx_tree_emit_device(ctx._h, vp(triangles.data_ptr()), vp(attributes.data_ptr()), vp(g.data_ptr()), vp(a.data_ptr()), vp(ids.data_ptr())) == OK
    assert_block_equals((g, a, ids), block)


def test_rows_a_torch_stream_is_still_writing_are_waited_for(ctx):
    _, block, rows = case("n65537")
    g, a = on_device(rows[0]), on_device(rows[1])
    busy = torch.ones(1 << 25, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(50):
            busy.sin_()
        late = torch.zeros_like(g) + g
    assert_block_equals(ctx.build_tree_device(late, a, stream=side), block)
    side.synchronize()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------

def answer(ctx, rows, n=None, address=None):
    entries = C.c_uint32(12345)
    rc = capi.LIB.flx_tree_build_device(ctx._h, C.c_void_p(rows.data_ptr() if address is None else address), rows.shape[0] if n is None else n, None, C.byref(entries))
    return rc, capi.LIB.flx_last_error(ctx._h).decode()


def emit_answer(ctx, triangles, g, a, ids, attributes=None):
    vp = C.c_void_p
    rc = capi.LIB.flx_tree_emit_device(ctx._h, vp(triangles), None if attributes is None else vp(attributes), vp(g), vp(a), vp(ids))
    return rc, capi.LIB.flx_last_error(ctx._h).decode()


def offend(g, at, rule):
    if rule == KIND:
        g[at, 10] = 1.0 if at % 2 else 0.0
    elif rule == TRANSFORM:
        g[at, 9] = {0: -1.0, 64: 1.0, 255: 1048576.0, 299: np.nan}.get(at, -2.0)      # out of range on either side, another number than row 0's, NaN
    else:
        g[at, (0, 4, 8)[at % 3]] = (np.inf, -np.inf, np.nan)[at % 3]


class Scene:
    """a context with a scene and a frame of it, to see that refusals leave both alone"""

    def __init__(self):
        self.scene = synth_scene.make_sized(300, 1, seed=5, width=W, height=H)
        self.p = self.scene.frame_params(width=W, height=H)
        self.ctx = capi.Context(0)
        self.ctx.update_scene(self.scene)
        self.frame = self.ctx.render(self.p)[0]

    def assert_untouched(self):
        assert bit_mismatches(self.ctx.render(self.p)[0], self.frame) == 0


@pytest.fixture(scope="module")
def held():
    s = Scene()
    yield s
    s.ctx.close()


@pytest.fixture(scope="module")
def candidate():
    rows = face_order_rows(host_block(random_soup(300, 31)), random_soup(300, 31))
    return rows


def assert_emit_is_refused(ctx):
    t = torch.zeros(4096, device="cuda")
    assert emit_answer(ctx, t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr()) == (INVALID, NO_BUILD_MESSAGE)


def test_emit_before_any_build_is_refused():
    with capi.Context(0) as fresh:
        assert_emit_is_refused(fresh)


@pytest.mark.parametrize("rule", [KIND, TRANSFORM, FINITE])
def test_an_offending_row_is_refused_with_its_message(held, candidate, rule):
    """the offender at row 0, 64, 255 and the last of 300, alone and with a later offender of another rule; after each refusal nothing is kept"""
    for at in (0, 64, 255, 299):
        g = candidate[0].copy()
        offend(g, at, rule)
        held.ctx.build_tree_device(on_device(candidate[0]))           # a tree that the refused build must not leave behind
        assert answer(held.ctx, on_device(g)) == (INVALID, MESSAGES[rule])
        assert_emit_is_refused(held.ctx)
        if at + 37 < 300:
            offend(g, at + 37, (rule + 2) % 3)
            assert answer(held.ctx, on_device(g)) == (INVALID, MESSAGES[rule])
    held.assert_untouched()


def test_of_two_offended_rules_in_one_row_the_first_is_reported(held, candidate):
    g = candidate[0].copy()
    g[100, 10], g[100, 9], g[100, 3] = 3.0, 4.0, np.inf
    assert answer(held.ctx, on_device(g)) == (INVALID, MESSAGES[KIND])
    g[100, 10] = 2.0
    assert answer(held.ctx, on_device(g)) == (INVALID, MESSAGES[TRANSFORM])
    g[100, 9] = 0.0
    assert answer(held.ctx, on_device(g)) == (INVALID, MESSAGES[FINITE])
    held.assert_untouched()


def test_a_transform_number_that_is_no_whole_number_is_refused(held, candidate):
    """every row agrees with row 0, but the boxes would carry bits the host builder never emits: a fraction, -0"""
    for value in (0.5, -0.0, 3.25):
        g = candidate[0].copy()
        g[:, 9] = value
        assert answer(held.ctx, on_device(g)) == (INVALID, MESSAGES[TRANSFORM])
    g = candidate[0].copy()
    g[:, 9] = 1048575.0
    assert answer(held.ctx, on_device(g))[0] == OK
    held.assert_untouched()


def test_counts_and_pointers_are_refused(held, candidate):
    g = np.ascontiguousarray(candidate[0])
    t = on_device(np.concatenate([g, g]))
    ctx = held.ctx
    assert answer(ctx, t, n=0) == (INVALID, COUNT_MESSAGE)
    assert answer(ctx, t, n=(1 << 24) + 1) == (INVALID, COUNT_MESSAGE)
    assert answer(ctx, t, n=300, address=g.ctypes.data) == (INVALID, POINTER_MESSAGE)      # a host pointer
    assert answer(ctx, t, n=300, address=t.data_ptr() + 4) == (INVALID, POINTER_MESSAGE)   # misaligned
    assert answer(ctx, t, n=1 << 24) == (INVALID, POINTER_MESSAGE)                          # far beyond the allocation
    assert_emit_is_refused(ctx)
    with pytest.raises((ValueError, TypeError)):
        ctx.build_tree_device(t[:, :11])
    with pytest.raises(ValueError):
        ctx.build_tree_device(t, on_device(candidate[1]))             # fewer attribute rows than triangles
    held.assert_untouched()


def test_emit_checks_its_arrays_against_the_build(held, candidate):
    ctx = held.ctx
    triangles = on_device(candidate[0])
    entries = ctx.build_tree_device(triangles)[0].shape[0]
    g, a, ids = torch.zeros((entries, 12), device="cuda"), torch.zeros((entries, 28), device="cuda"), torch.zeros(300, dtype=torch.int32, device="cuda")
    host = np.zeros((entries, 28), np.float32)
    assert emit_answer(ctx, host.ctypes.data, g.data_ptr(), a.data_ptr(), ids.data_ptr()) == (INVALID, ROWS_MESSAGE)
    assert emit_answer(ctx, triangles.data_ptr() + 4, g.data_ptr(), a.data_ptr(), ids.data_ptr()) == (INVALID, ROWS_MESSAGE)
    assert emit_answer(ctx, triangles.data_ptr(), host.ctypes.data, a.data_ptr(), ids.data_ptr()) == (INVALID, ARRAY_MESSAGE)
    assert emit_answer(ctx, triangles.data_ptr(), g.data_ptr(), a.data_ptr() + 8, ids.data_ptr()) == (INVALID, ARRAY_MESSAGE)
    assert emit_answer(ctx, triangles.data_ptr(), g.data_ptr(), a.data_ptr(), ids.data_ptr(), attributes=host.ctypes.data) == (INVALID, ARRAY_MESSAGE)
    assert emit_answer(ctx, triangles.data_ptr(), g.data_ptr(), a.data_ptr(), ids.data_ptr())[0] == OK
    held.assert_untouched()


def test_emit_refuses_arrays_too_short_for_the_build(ctx):
    """rows that are not n_triangles of the build, an output array shorter than n_entries: device memory, aligned, but the allocation ends before the array would.
    (A few words in the allocator's 2 MB block of small tensors against a build whose arrays take 3 MB and more: a row short need not leave an allocation.)"""
    _, block, rows = case("n65537")
    triangles, attributes = on_device(rows[0]), on_device(rows[1])
    g, a, ids = ctx.build_tree_device(triangles, attributes)
    few = torch.zeros((4, 12), device="cuda")
    torch.cuda.synchronize()
    assert emit_answer(ctx, few.data_ptr(), g.data_ptr(), a.data_ptr(), ids.data_ptr()) == (INVALID, ROWS_MESSAGE)
    assert emit_answer(ctx, triangles.data_ptr(), few.data_ptr(), a.data_ptr(), ids.data_ptr()) == (INVALID, ARRAY_MESSAGE)
    assert emit_answer(ctx, triangles.data_ptr(), g.data_ptr(), few.data_ptr(), ids.data_ptr()) == (INVALID, ARRAY_MESSAGE)
    assert emit_answer(ctx, triangles.data_ptr(), g.data_ptr(), a.data_ptr(), ids.data_ptr(), attributes=few.data_ptr()) == (INVALID, ARRAY_MESSAGE)
    assert emit_answer(ctx, triangles.data_ptr(), g.data_ptr(), a.data_ptr(), ids.data_ptr(), attributes=attributes.data_ptr())[0] == OK
    assert_block_equals((g, a, ids), block)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------------

def test_a_block_spliced_behind_a_scene_renders_as_the_hosts_arrays_do():
    base = synth_scene.make_sized(200, 1, seed=3, width=W, height=H)
    first = base.meta["textureLength"]
    soup = random_soup(300, 21, centre=(0.0, 0.0, 8.0), extent=3.0, size=0.8)
    block = host_block(soup)
    rows = face_order_rows(block, soup)
    total = first + block[0].shape[0]
    padded = (total + 255) // 256 * 256
    # on the host
    hg, ha = np.zeros((padded, 12), np.float32), np.zeros((padded, 28), np.float32)
    hg[:first], ha[:first] = base.arrays["geometry"].reshape(-1, 12)[:first], base.arrays["attributes"].reshape(-1, 28)[:first]
    hg[first:total], ha[first:total] = block[0], block[1]
    want = scene_of(base, hg, ha)
    assert np.array_equal(want.arrays["ids"], np.concatenate([base.arrays["ids"], block[2] + first]))
    p = base.frame_params(width=W, height=H, samples=1, max_reflections=2)
    with capi.Context(0) as host, capi.Context(0) as device:
        host.update_scene(base)
        alone = host.render(p)[0]
        host.update_scene(want)
        device.update_scene(decoy(base))
        # on the device
        g, a, ids = device.build_tree_device(on_device(rows[0]), on_device(rows[1]))
        dg, da = torch.zeros((padded, 12), device="cuda"), torch.zeros((padded, 28), device="cuda")
        dg[:first], da[:first] = on_device(hg[:first]), on_device(ha[:first])
        dg[first:total], da[first:total] = g, a
        dids = torch.cat([on_device(base.arrays["ids"], np.int32), ids + first])
        device.upload_scene_device(dg, da, dids, stream=torch.cuda.current_stream())
        got_frame, got_counters, _ = device.render(p, counters=True)
        want_frame, want_counters, _ = host.render(p, counters=True)
        assert bit_mismatches(got_frame, want_frame) == 0 and got_counters == want_counters
        assert bit_mismatches(want_frame, alone) > 0                  # (the block is in view)
        # the block's rows move: a row update refits what the build made
        moved = block[0].copy()
        moved[moved[:, 10] == 2, :9] += np.float32(0.03125)
        device.update_scene_rows_device(first, on_device(moved))
        host.update_scene_rows(first, moved)
        assert (bits(device.scene_read("geometry", total)) == bits(host.scene_read("geometry", total))).all()
        assert (bits(device.scene_read("attributes", total)) == bits(host.scene_read("attributes", total))).all()
