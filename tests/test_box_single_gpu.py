"""The box test's single-comparison form (csrc/flx_device.h: rayCuboidInterval<true>) and the scene hint that selects it (DeviceScene::walk_thick_boxes).

The form replaces the interval test's three cross-pair comparisons by lo(tmax) >= hi(tmin); whatever it is not sure of goes to the exact quotients, so it must give
the shader's boolean for EVERY box, flat ones included — the hint decides speed alone.  Held here:

- literal rows: the committed tables and rows built for each outcome of the form (tests/box_single_util.py) through flx_debug_intersect 7 (bounded scenes) and 8
  (scenes that are not), bit for bit against the oracle's rayCuboid and the per-pixel kernel's (fn 5); the edge table's box rows packed into small scenes and walked
  by the frame kernels' lane walk with the form forced to 0 and to 1, against the literal walks;
- small frames: the dragon and a scene half of whose boxes are flat through the frame kernels and the frame server with either form forced — the oracle's frame
  and, where the kernel counts, its work counters (the frame server does not take a counted frame);
- the hint after every way a box can enter the scene, and the oracle's frame after each."""
import gzip
import json
import os

import numpy as np
import pytest

from box_single_util import (bounded_rows, flattened, half_flat_scene, nan_corner_rows, oracle_ray_cuboid, thick_scene)
from intersect_edges_util import OHI, literal_walks, packed_scenes, same_walks
from scene_splice_util import splice_rule
from scene_upload_device_util import scene_of
from scene_update_util import reflatten

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
W, H = 96, 54


@pytest.fixture()
def forms(hip):
    """the session's context; whatever a test forces is taken back"""
    yield hip
    hip.set_box_test(-1)
    hip.set_frame_lanes(2)
    hip.set_frame_chain(2)
    hip.set_pipeline(0)
    hip.set_wavefront_organisation(0)
    hip.set_frame_front(1)


def _orders(n):
    """table order; reversed; a seeded shuffle (waves of mixed outcomes); calls of 1, 63 and 65 rows (a wave with one row, one short of full, one lane over)"""
    yield "table_order", [np.arange(n)]
    yield "reversed", [np.arange(n)[::-1]]
    yield "shuffled", [np.random.default_rng(3).permutation(n)]
    calls, pos, k = [], 0, 0
    while pos < n:
        c = (1, 63, 65)[k % 3]
        calls.append(np.arange(pos, min(pos + c, n)))
        pos, k = pos + c, k + 1
    yield "calls_of_1_63_65", calls


def _run(hip, fn, rows, want, classes):
    failures = []
    for name, calls in _orders(len(rows)):
        for idx in calls:
            got = hip.debug_intersect(fn, rows[idx])
            for p in np.flatnonzero(got != want[idx])[:5]:
                failures.append("fn %d %s: %s: row %s want %g got %g" % (fn, name, classes[idx[p]], " ".join("%08x" % x for x in rows[idx[p]].view(np.uint32)), want[idx[p]], got[p]))
    assert not failures, "%d rows differ\n%s" % (len(failures), "\n".join(failures[:20]))


# ---- literal rows ----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def edge_kat():
    return json.load(gzip.open(os.path.join(HERE, "golden", "intersect_edge_kat.json.gz"), "rt"))


def test_the_committed_tables_through_the_single_comparison_form(hip, edge_kat):
    """every row of tests/golden/intersect_kat.json.gz and intersect_edge_kat.json.gz: fn 7 on the rows whose box keeps flx_scene_upload's bound (what fn 2 runs),
    fn 8 on every row, against the tables' literal answers"""
    plain = json.load(gzip.open(os.path.join(HERE, "golden", "intersect_kat.json.gz"), "rt"))["ray_cuboid"]
    for table, cls in ((plain, lambda r: "intersect_kat"), (edge_kat["ray_cuboid"], lambda r: r[14])):
        rows = np.array([r[0:13] for r in table], np.uint32).view(np.float32)
        want = np.array([r[13] for r in table], np.float32)
        classes = [cls(r) for r in table]
        with np.errstate(invalid="ignore"):
            bounded = np.flatnonzero(np.all(np.abs(rows[:, 7:13]) <= OHI, axis=1))
        assert len(bounded) >= len(rows) - 260 and 300 <= want.sum() <= len(rows) - 300
        _run(hip, 7, rows[bounded], want[bounded], [classes[k] for k in bounded])
        _run(hip, 8, rows, want, classes)


def test_rows_built_for_each_outcome_of_the_form(hip, oracle):
    """tmin and tmax 0, 1, 2, 4, 8 float32 steps apart and just under / over 2^-20 relative; flat boxes on each axis, hit and missed; the origin on a face; l below
    2^-60; directions outside the reciprocal's range; NaN in a corner (a scene that is not bounded: fn 8, 6) — every row is the oracle's rayCuboid in both forms of the
    walk kernels' test and in the per-pixel kernel's (test_box_single_cpu.py asserts which outcome of the form the rows land in)"""
    rows, classes = bounded_rows()
    want = oracle_ray_cuboid(oracle, rows)
    assert len(rows) >= 2000 and 400 <= want.sum() <= len(rows) - 400
    for fn in (7, 2, 5, 8, 6):
        _run(hip, fn, rows, want, classes)
    rows, classes = nan_corner_rows()
    want = oracle_ray_cuboid(oracle, rows)
    for fn in (8, 6, 5):
        _run(hip, fn, rows, want, classes)


def test_edge_rows_through_the_lane_walk_in_either_form(forms, edge_kat):
    """the edge table's box rows, 32 to a scene (flat boxes among them), walked by the frame kernels' lane walk (flx_debug_walk variant 0, flx_debug_walk_staged with
    half the tree in LDS) with the form forced to 0 and to 1: hit, entry, shadow answer and both visit counts are the literal walk's — a box boolean that flips
    changes a visit count by one"""
    failures, scenes = [], 0
    for name, sc, rays, classes in packed_scenes(edge_kat, False):
        if not name.startswith("box"):
            continue
        want = literal_walks(sc, rays)
        forms.update_scene(sc)
        for form in (0, 1):
            forms.set_box_test(form)
            for run, got in (("walk", forms.debug_walk(0, rays)), ("staged", forms.debug_walk_staged(len(rays) + 1, rays)[:, :8])):
                for k in np.flatnonzero(~same_walks(got, want)):
                    failures.append("%s / form %d / %s / %s: ray %d want %s got %s" % (name, form, run, classes[k], k, want[k].tolist(),
                                                                                     got[k, 0:3].view(np.uint32).tolist() + got[k, 3:8].astype(np.int64).tolist()))
        scenes += 1
    assert scenes >= 130
    assert not failures, "%d walks differ from the literal walks\n%s" % (len(failures), "\n".join(failures[:30]))


# ---- small frames ----------------------------------------------------------------------------------------------------------------------------------------------

def _loop(ctx, ps):
    got, kinds = [], []
    for p in ps:
        if ctx.frames_in_flight() == 2:
            got.append(ctx.frame_end()[0])
        ctx.frame_begin(p)
        kinds.append(ctx.last_chained())
    while ctx.frames_in_flight():
        got.append(ctx.frame_end()[0])
    return got, kinds


@pytest.fixture(scope="module")
def small_frames(oracle, scenes):
    """(scene, the 96 x 54 frame, the 96 x 56 frame the server takes — its rows are whole strips of 8 —, the oracle's (frame, counters) of both), computed once"""
    out = {}
    for name, sc in (("dragon", scenes("dragon")), ("half_flat", half_flat_scene())):
        ps = [sc.frame_params(width=W, height=h, samples=2, max_reflections=4, use_filter=0) for h in (H, 56)]
        out[name] = (sc, ps, [oracle.render(sc, p)[:2] for p in ps])
    return out


@pytest.mark.parametrize("form", [0, 1], ids=["cross_pairs", "single_comparison"])
@pytest.mark.parametrize("name", ["dragon", "half_flat"])
def test_small_frames_through_the_frame_kernels_and_the_server(forms, small_frames, name, form):
    sc, ps, want = small_frames[name]
    forms.update_scene(sc)
    assert forms.walk_thick_boxes() == (1 if name == "dragon" else 0)
    forms.set_pipeline(3)
    forms.set_wavefront_organisation(2)
    forms.set_box_test(form)
    for front in (0, 2):                                     # k_wf_shade0 in front of the frame kernel; the front inside it
        forms.set_frame_front(front)
        for p, (frame, counters) in zip(ps, want):
            got, cnt, _ = forms.render(p, counters=True)
            assert forms.last_organisation() in (2, 3) and forms.last_box_test() == form      # the kernel of the form asked for is the one that ran
            assert np.array_equal(got, frame, equal_nan=True) and cnt == counters, (front, p.height)
            assert np.array_equal(forms.render(p)[0], frame, equal_nan=True), (front, p.height)      # the kernels that do not count
    forms.set_frame_front(1)
    forms.set_frame_chain(3)
    forms.set_frame_lanes(2)
    # 54 rows are no whole strips of 8: the loop renders that frame on its lanes; the 56-row frame goes to the server
    got, kinds = _loop(forms, [ps[0], ps[1], ps[1], ps[0], ps[1]])
    assert [k == 3 for k in kinds] == [False, True, True, False, True], kinds
    assert forms.last_box_test() == form                     # (the server's launch, the last one made)
    for g, k in zip(got, (0, 1, 1, 0, 1)):
        assert np.array_equal(g, want[k][0], equal_nan=True)


# ---- the hint ----------------------------------------------------------------------------------------------------------------------------------------------------

def _assert_oracle_frame(ctx, oracle, sc):
    """the scene the context holds renders as the oracle renders `sc`, through the frame kernel in the form the hint selects and in the other one"""
    p = sc.frame_params(width=64, height=48, samples=1, max_reflections=3, use_filter=0)
    frame, counters, _ = oracle.render(sc, p)
    ctx.set_pipeline(3)
    ctx.set_wavefront_organisation(2)
    for form in (-1, 1, 0):
        ctx.set_box_test(form)
        got, cnt, _ = ctx.render(p, counters=True)
        assert np.array_equal(got, frame, equal_nan=True) and cnt == counters, form
        assert ctx.last_box_test() == (ctx.walk_thick_boxes() if form < 0 else form)      # left to the hint, the launch follows it
    ctx.set_box_test(-1)


def test_the_hint_after_a_host_upload_and_a_vertex_update(forms, oracle, scenes):
    thick = thick_scene()
    forms.update_scene(thick)
    assert forms.walk_thick_boxes() == 1
    _assert_oracle_frame(forms, oracle, thick)
    forms.update_scene(half_flat_scene())
    assert forms.walk_thick_boxes() == 0
    forms.update_scene(thick)
    assert forms.walk_thick_boxes() == 1                      # a later thick scene gets the hint back
    sc, first, rows = flattened(thick, 5)
    forms.update_scene_rows(first, rows)                      # the refit makes leaf 5's box flat, on the device
    assert forms.walk_thick_boxes() == 0
    _assert_oracle_frame(forms, oracle, sc)
    forms.update_scene(thick)
    assert forms.walk_thick_boxes() == 1
    import torch
    forms.update_scene_rows_device(first, torch.from_numpy(rows).cuda())
    assert forms.walk_thick_boxes() == 0
    _assert_oracle_frame(forms, oracle, sc)


def test_the_hint_after_a_device_upload_a_splice_and_a_tree_build(forms, oracle):
    import torch
    dev = lambda a, dtype=np.float32: torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()
    thick, half = thick_scene(), half_flat_scene()
    for sc, want in ((thick, 1), (half, 0)):
        # (the transforms, lights and atlases of a scene_of / by_hand scene are those of `thick`: the host upload brings them, the device upload the entries)
        forms.update_scene(thick if want == 0 else half)
        forms.upload_scene_device(dev(sc.arrays["geometry"].reshape(-1, 12)), dev(sc.arrays["attributes"].reshape(-1, 28)), dev(sc.arrays["ids"], np.int32))
        assert forms.walk_thick_boxes() == want              # k_derive_check looks at every box in the pass that checks the bound
        _assert_oracle_frame(forms, oracle, sc)
    # a block behind the last leaf, inside the root box: a box over two triangles — tilted, then in one plane
    g, a, ids = thick.arrays["geometry"].reshape(-1, 12), thick.arrays["attributes"].reshape(-1, 28), thick.arrays["ids"]
    end = 37
    assert g[end - 1, 10] == 2 and g[end, 10] == 0
    for flat, want in ((False, 1), (True, 0)):
        bg, ba = g[1:4].copy(), a[1:4].copy()                 # leaf 0's rows, moved up and to the back
        bg[1:3, [1, 4, 7]] += np.float32(7.0)
        bg[1:3, [2, 5, 8]] += np.float32(1.0)
        if flat:
            bg[1:3, [2, 5, 8]] = np.float32(8.5)
        block = (bg, ba, np.array([1, 2], np.int32))
        wg, wa, wids = splice_rule(g, a, ids, end, 0, 0, block)
        spliced = scene_of(thick, wg, wa)
        assert np.array_equal(spliced.arrays["ids"], wids)
        forms.update_scene(thick)
        forms.splice_scene_device(end, 0, 0, dev(bg), dev(ba), dev(block[2], np.int32))
        assert forms.walk_thick_boxes() == want              # the check that follows the splice's refit sees the refitted boxes
        _assert_oracle_frame(forms, oracle, spliced)
    # a tree built on the device enters the scene through the splice (or a device upload): its boxes are looked at there
    forms.update_scene(thick)
    tg, ta = g[g[:, 10] == 2][:8].copy(), a[g[:, 10] == 2][:8].copy()
    tg[:, [1, 4, 7]] += np.float32(7.0)
    rows = forms.replace_mesh_device(end, 0, 0, dev(tg), dev(ta))
    got = forms.scene_read("geometry", end + rows)
    boxes = got[got[:, 10] == 1]
    assert forms.walk_thick_boxes() == int(bool(np.all(boxes[:, 0:3] < boxes[:, 3:6])))
    wg, wa = np.zeros_like(g), np.zeros_like(a)
    wg[:end + rows], wa[:end + rows] = got, forms.scene_read("attributes", end + rows)
    _assert_oracle_frame(forms, oracle, scene_of(thick, wg, wa))
