"""The GPU's box and triangle tests on the float borders of their predicates (tests/golden/intersect_edge_kat.json.gz, tests/analysis/make_intersect_edge_kat.py):
rows on which the boolean from one product per quotient differs from the shader's, rows the interval test is not sure about (Markstein's corrected quotients decide),
rows just outside its 2^-21 band, |a| around 2^-40, directions, origins and l on the borders of the fast range, boxes beyond it, det / u / v / s on BIAS, 1, l, 2^60,
infinite and NaN.  Bit for bit (NaN == NaN) against answers derived from the shader text, for the walk kernels' routines (flx_debug_intersect fn 0, 1, 2, and 6: the
box test of a scene whose boxes are not bounded) and the per-pixel kernel's (3, 4, 5).

k_debug_intersect runs 64 rows per wave and recipOf / recipOfDet (optionally the box fallback) choose their path by a ballot of the wave, so every table runs in
four arrangements that must all give every row the same answer: table order; sorted, so that waves are homogeneous in the path their rows take; interleaved, so
that every wave holds exactly one row that is out of range (and all 64 lanes divide: this bears on fn 0, 1, 3, 4 and on fn 2; under fn 5 and 6 every lane divides
anyway and the arrangement is one more order); and in calls of 1, 63 and 65 rows.

flx_debug_intersect tests functions, and a rewritten walk may stop calling them: the same rows are therefore packed into small scenes (intersect_edges_util.packed_scenes)
and walked by every flx_debug_walk variant and by flx_debug_walk_staged against the literal walks of tests/analysis/make_walk_kat.py."""
import gzip
import json
import os
import sys

import numpy as np
import pytest

from flexlight_hip import capi
from intersect_edges_util import OHI, far_triangle_scene, literal_walks, packed_scenes, same_walks, small_scene, with_geometry

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "analysis"))
import make_intersect_edge_kat as gen      # noqa: E402   (the replay of the decision structure: used for the ORDER of rows only)


@pytest.fixture(scope="module")
def kat():
    return json.load(gzip.open(os.path.join(HERE, "golden", "intersect_edge_kat.json.gz"), "rt"))


def _f32(rows, a, b):
    return np.array([r[a:b] for r in rows], np.uint32).view(np.float32)


def arrangements(keys, out_of_range):
    """(name, index per position) of the four arrangements of n rows; keys: the path of every row (a tuple); out_of_range: bool per row"""
    n = len(keys)
    yield "table_order", [np.arange(n)]
    yield "homogeneous_waves", [np.array(sorted(range(n), key=lambda i: (keys[i], i)))]
    inside, outside = np.flatnonzero(~out_of_range), np.flatnonzero(out_of_range)
    assert len(inside) >= 63 and len(outside) >= 1
    blocks = max(-(-len(inside) // 63), len(outside))
    idx = np.resize(inside, blocks * 63).reshape(blocks, 63)
    waves = [np.insert(idx[b], b % 64, outside[b % len(outside)]) for b in range(blocks)]       # one lane out of range per wave, in a lane that moves
    yield "one_lane_out_of_range", [np.concatenate(waves)]
    calls, pos, k = [], 0, 0
    while pos < n:
        c = (1, 63, 65)[k % 3]
        calls.append(np.arange(pos, min(pos + c, n)))
        pos, k = pos + c, k + 1
    yield "calls_of_1_63_65", calls


def run_table(hip, fn, inputs, want, classes, keys, out_of_range):
    """every arrangement against `want`, bit for bit; failures per class with the first rows' inputs as hex words"""
    want = want.reshape(len(inputs), -1)
    failures = []
    for name, calls in arrangements(keys, out_of_range):
        bad = set()
        for idx in calls:
            got = hip.debug_intersect(fn, inputs[idx]).reshape(len(idx), -1)
            w = want[idx]
            same = ((got.view(np.uint32) == w.view(np.uint32)) | (np.isnan(got) & np.isnan(w))).all(axis=1)
            for p in np.flatnonzero(~same):
                if idx[p] not in bad:
                    bad.add(int(idx[p]))
                    if len(bad) <= 400:
                        failures.append((name, int(idx[p]), got[p]))
    if failures:
        per = {}
        for name, i, got in failures:
            per.setdefault((name, classes[i]), []).append((i, got))
        lines = []
        for (name, cls), rows in sorted(per.items()):
            i, got = rows[0]
            lines.append("%s / %s: %d rows, first row %d: in %s want %s got %s" % (name, cls, len(rows), i, " ".join("%08x" % x for x in inputs[i].view(np.uint32)),
                         " ".join("%08x" % x for x in want[i].view(np.uint32)), " ".join("%08x" % x for x in got.view(np.uint32))))
        pytest.fail("fn %d: %d (arrangement, class) pairs differ from the literal answers\n%s" % (fn, len(per), "\n".join(lines)))


def box_bounded(r):
    return all(abs(float(gen.unbits(w))) <= OHI for w in r[7:13])           # (NaN and inf fail the comparison)


@pytest.mark.parametrize("fn", [2, 6, 5], ids=["walk_kernels_bounded_scene", "walk_kernels_unbounded_scene", "per_pixel_kernel"])
def test_ray_cuboid_edges(hip, kat, fn):
    """fn 2 stands for a scene with walk_fast_boxes = 1: it runs the rows whose box keeps that scene's bound and no others; fn 6 (the flag off) and the per-pixel
    kernel's division run every row, the unbounded ones included"""
    rows = [r for r in kat["ray_cuboid"] if fn != 2 or box_bounded(r)]
    if fn == 2:
        assert not any(r[14].startswith("unbounded") for r in rows) and len(rows) >= len(kat["ray_cuboid"]) - 260
    else:
        assert sum(1 for r in rows if r[14].startswith("unbounded")) >= 180
    paths = [gen.box_paths(r, flag=1 if fn == 2 else 0) for r in rows]
    keys = [p[:3] for p in paths]
    fast_on = np.array([gen.box_paths(r)[0] for r in rows])
    want = np.array([r[13] for r in rows], np.float32)
    assert 1000 <= want.sum() <= len(rows) - 1000
    run_table(hip, fn, _f32(rows, 0, 13), want, [r[14] for r in rows], keys, ~fast_on)


def tri_paths(rows):
    det = np.array([float(gen.tri_values(r)["det"]) for r in rows])
    with np.errstate(invalid="ignore"):
        in_range = np.abs(det) <= 2.0 ** 60                                  # recipOfDet's / recipOf's upper end; NaN is out of range
        needed = ~(np.abs(det) < 2.0 ** -16)
    return in_range, needed


@pytest.mark.parametrize("fn", [0, 3], ids=["walk_kernels", "per_pixel_kernel"])
def test_moeller_trumbore_edges(hip, kat, fn):
    rows = kat["moeller_trumbore"]
    in_range, needed = tri_paths(rows)
    want = _f32(rows, 16, 19)
    assert np.count_nonzero(want[:, 0]) >= 300
    run_table(hip, fn, _f32(rows, 0, 16), want, [r[19] for r in rows], list(zip(in_range.tolist(), needed.tolist())), ~in_range & needed)


@pytest.mark.parametrize("fn", [1, 4], ids=["walk_kernels", "per_pixel_kernel"])
def test_moeller_trumbore_cull_edges(hip, kat, fn):
    rows = kat["moeller_trumbore_cull"]
    in_range, needed = tri_paths(rows)
    want = np.array([r[16] for r in rows], np.float32)
    assert want.sum() >= 150
    run_table(hip, fn, _f32(rows, 0, 16), want, [r[17] for r in rows], list(zip(in_range.tolist(), needed.tolist())), ~in_range & needed)


# ---- the scene flag ------------------------------------------------------------------------------------------------------------------------------------

def test_walk_fast_boxes_is_computed_from_the_box_entries(hip):
    """flx_scene_upload's walk_fast_boxes: 1 up to a largest box coordinate of 2^59 itself, 0 from its float successor on, for +-inf and NaN, in the first and in
    the last box entry and in any of the six coordinates; triangle entries do not count"""
    sc = small_scene()
    g0 = sc.arrays["geometry"].reshape(-1, 12).copy()
    boxes, tris = np.flatnonzero(g0[:, 10] == 1), np.flatnonzero(g0[:, 10] == 2)
    assert len(boxes) >= 3 and boxes[0] == 0
    hip.update_scene(sc)
    assert hip.walk_fast_boxes() == 1
    up = np.nextafter(np.float32(OHI), np.float32(np.inf))
    for entry in (boxes[0], boxes[-1]):
        for k in range(6):
            sign = -1.0 if k < 3 else 1.0
            for value, want in ((OHI, 1), (up, 0), (np.inf, 0), (np.nan, 0), (2.0 ** 100, 0)):
                g = g0.copy()
                g[entry, k] = sign * value
                hip.update_scene(with_geometry(sc, g))
                assert hip.walk_fast_boxes() == want, (entry, k, value)
    for value in (up, 2.0 ** 100, np.inf, np.nan):
        g = g0.copy()
        g[tris[0], 2], g[tris[-1], 7] = value, -value
        hip.update_scene(with_geometry(sc, g))
        assert hip.walk_fast_boxes() == 1, value
    hip.update_scene(sc)
    assert hip.walk_fast_boxes() == 1                                       # and a later bounded scene gets the flag back


def test_triangle_beyond_the_bound_under_bounded_boxes(hip):
    """a floor triangle that reaches 2^61 under a root box cut at 2^59: the scene keeps walk_fast_boxes = 1 (boxes alone decide), and every walk answers the rays at
    that triangle as the literal walk of the shader text does (tests/analysis/make_walk_kat.py over the same arrays): hit, entry, shadow answer, both visit counts"""
    sc, rays = far_triangle_scene()
    g = sc.arrays["geometry"].reshape(-1, 12)
    hip.update_scene(sc)
    assert hip.walk_fast_boxes() == 1
    want = literal_walks(sc, rays)
    assert (want[:, 4] != -1).sum() >= 5 and want[1::4, 6].sum() + want[2::4, 6].sum() >= 16      # objects are hit, the far floor shadows
    runs = [("variant %d" % v, hip.debug_walk(v, rays)) for v in (0, 1, 2)] + [("staged %d" % c, hip.debug_walk_staged(c, rays)[:, :8]) for c in (0, len(g) // 2, len(g))]
    for name, got in runs:
        assert np.array_equal(got[:, 0:3].view(np.uint32).astype(np.int64), want[:, 0:3]), name
        assert np.array_equal(got[:, 3:8].astype(np.int64), want[:, 3:8]), name


# ---- the same borders through the walks ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("two_spaces", [False, True], ids=["one_space", "two_spaces"])
def test_edge_rows_through_the_walks(hip, kat, two_spaces):
    """the table's box and triangle rows, 32 to a scene, through flx_debug_walk variants 0, 1, 2 and flx_debug_walk_staged with nothing, half and all of the tree in
    LDS: hit to the bit, entry, shadow answer and BOTH visit counts are the literal walk's.  With two object spaces (the second one the world halved) the rows pass
    through walkLoadRay / the change of object space; the lockstep walk (variant 2) takes one space only and must say so"""
    failures, scenes = [], 0
    for name, sc, rays, classes in packed_scenes(kat, two_spaces):
        want = literal_walks(sc, rays)
        hip.update_scene(sc)
        assert hip.walk_fast_boxes() == 1
        entries = 2 * len(rays) + 2
        runs = [("variant %d" % v, lambda v=v: hip.debug_walk(v, rays)) for v in (0, 1)] + [("staged %d" % c, lambda c=c: hip.debug_walk_staged(c, rays)[:, :8]) for c in (0, entries // 2, entries)]
        if two_spaces:
            with pytest.raises(capi.FlexLightHipError):
                hip.debug_walk(2, rays)
        else:
            runs.append(("variant 2", lambda: hip.debug_walk(2, rays)))
        for run, call in runs:
            got = call()
            for k in np.flatnonzero(~same_walks(got, want)):
                failures.append("%s / %s / %s: ray %d %s want %s got %s" % (name, run, classes[k], k, " ".join("%08x" % x for x in rays[k].view(np.uint32)), want[k].tolist(),
                                                                           got[k, 0:3].view(np.uint32).tolist() + got[k, 3:8].astype(np.int64).tolist()))
        scenes += 1
    assert scenes >= 150
    assert not failures, "%d rays differ from the literal walks\n%s" % (len(failures), "\n".join(failures[:30]))
