"""Shared by tests/test_intersect_edges_cpu.py and tests/test_intersect_edges_gpu.py: the small scenes around walk_fast_boxes and the literal walks over them."""
import os
import sys

import numpy as np

import synth_scene

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "analysis"))

OHI = float(2.0 ** 59)          # flx_scene_upload's bound of a box coordinate


def small_scene(**kw):
    return synth_scene.make(seed=11, n_objects=2, tris_per_object=8, n_transforms=1, n_lights=1, width=32, height=24, **kw)


def with_geometry(sc, g):
    arrays = dict(sc.arrays)
    arrays["geometry"] = np.ascontiguousarray(g, np.float32).reshape(-1)
    return type(sc)(sc.meta, arrays)


def far_triangle_scene():
    """a floor triangle that reaches 2^61 under a root box cut at 2^59 (every box bounded, a triangle not), and 96 rays: at the objects, from above at the near end of
    that floor (never a hit: v along the 2^61 edge stays below BIAS within rayTracer's 2^32) and from below at points 2^46 .. 2^58 away on it, which only shadowTest
    with a long l finds: (scene, rays [96, 7] float32: origin, direction, shadowTest's l)"""
    sc = small_scene(floor_far=2.0 ** 61)
    g = sc.arrays["geometry"].reshape(-1, 12).copy()
    assert g[0, 10] == 1 and g[0, 5] == np.float32(2.0 ** 61)
    g[0, 5] = OHI
    sc = with_geometry(sc, g)
    rng = np.random.default_rng(5)
    rays = np.zeros((96, 7), np.float32)
    for j in range(96):
        if j % 4 == 0:
            o, target, l = np.array([rng.uniform(-5, 5), rng.uniform(0, 6), rng.uniform(-8, 0)]), np.array([rng.uniform(-4, 4), rng.uniform(-4, 4), 10.0]), 1e9
        elif j % 4 == 3:
            o, target, l = np.array([rng.uniform(-5, 5), rng.uniform(0, 6), rng.uniform(-8, 0)]), np.array([rng.uniform(-20, 20), -6.0, 2.0 ** rng.uniform(2, 31)]), 1e9
        else:
            o, target = np.array([rng.uniform(-5, 5), rng.uniform(-9, -6.5), rng.uniform(-4, 0)]), np.array([rng.uniform(-20, 20), -6.0, 2.0 ** rng.uniform(46, 58)])
            l = rng.choice([np.inf, 2.0 ** 60, 2.0 ** 40])
        d = target - o
        rays[j, 0:3], rays[j, 3:6], rays[j, 6] = o, d / np.linalg.norm(d), l
    return sc, rays


def literal_walks(sc, rays):
    """[n, 8] int64 like flx_debug_walk's columns (s, u, v as bit patterns; 2 x transform, entry, entries fetched, shadowed, entries fetched), from the literal
    walks of the shader text (tests/analysis/make_walk_kat.py), a NaN in a box test taken through min / max as their defining comparisons"""
    import make_walk_kat as walk
    A = walk.Arrays(sc)
    before, walk.PIN_NAN = walk.PIN_NAN, True
    try:
        want = []
        for r in rays:
            o, d = [walk.f32(x) for x in r[0:3]], [walk.f32(x) for x in r[3:6]]
            (suv, tI, tri), fetched = walk.ray_tracer(A, o, d)
            shadow, sfetched = walk.shadow_test(A, o, d, walk.f32(r[6]))
            want.append([walk.bits(x) for x in suv] + [tI if tri != -1 else 0, tri, fetched, shadow, sfetched])
    finally:
        walk.PIN_NAN = before
    return np.array(want, np.int64)


# ---- the table's rows packed into small scenes (the same borders through the walks) ------------------------------------------------------------------

PER_SCENE = 32
ROOT = float(2.0 ** 58)         # the root box and the boxes over the triangle rows: bounded (walk_fast_boxes = 1), and wide enough for every row packed


def _entry(kind, coords, transform, skip=0.0):
    g = np.zeros(12, np.float32)
    g[:len(coords)] = coords
    if kind == 1: g[6] = skip
    g[9], g[10] = transform, kind
    return g


def _scene(entries, two_spaces, seed):
    rotation, shift = np.zeros((2 if two_spaces else 1, 24), np.float32), np.zeros((2 if two_spaces else 1, 8), np.float32)
    for t in range(rotation.shape[0]):
        scale = 2.0 if t else 1.0                                  # object space 1 is the world halved: a power of two keeps every border of a row exactly
        for r in range(3):
            rotation[t, 4 * r + r], rotation[t, 12 + 4 * r + r] = scale, 1.0 / scale
    att = [np.zeros(28, np.float32) for _ in entries]
    return synth_scene._package(np.random.default_rng(seed), seed, entries, att, rotation, shift, rotation.shape[0], 1, 0, 32, 24, 1, 1, False)


def packed_scenes(kat, two_spaces):
    """(name, scene, rays [n, 7] float32, classes): a root box, then 32 (box, triangle) pairs.  Box scenes: the boxes of 32 ray_cuboid rows, a triangle under each, ray k
    the ray of row k — adversarial for box k, and it meets the other 31 as well; a box boolean that flips changes a visit count by one.  Triangle scenes: the
    triangles of 32 moeller_trumbore rows, each under a wide box, ray k the ray of row k; a predicate that flips changes the hit or the shadow answer.  two_spaces:
    every second pair stands in object space 1 (the world halved, coordinates halved with it), which takes its rays through the walks' change of object space"""
    f = lambda words: np.array(words, np.uint32).view(np.float32)
    small = lambda v: bool(np.all(np.abs(v) <= ROOT))              # (NaN and inf fail)
    groups = []
    rows = [r for r in kat["ray_cuboid"] if small(f(r[1:4])) and small(f(r[7:13]))]
    for at in range(0, len(rows), PER_SCENE):
        groups.append(("box", at, rows[at:at + PER_SCENE]))
    rows = kat["moeller_trumbore"]
    for at in range(0, len(rows), PER_SCENE):
        groups.append(("tri", at, rows[at:at + PER_SCENE]))
    for kind, at, chunk in groups:
        entries = [_entry(1, [-ROOT] * 3 + [ROOT] * 3, 0, skip=2 * len(chunk))]
        rays = np.zeros((len(chunk), 7), np.float32)
        for k, r in enumerate(chunk):
            t = k % 2 if two_spaces else 0
            h = np.float32(0.5 if t else 1.0)
            if kind == "box":
                l, o, d, mn, mx = f(r[0:1])[0], f(r[1:4]), f(r[4:7]), f(r[7:10]), f(r[10:13])
                tri = np.array([mn[0], mn[1], mn[2], mx[0], mn[1], mn[2], mn[0], mx[1], mx[2]], np.float32)
                entries += [_entry(1, np.concatenate([mn, mx]) * h, t, skip=1), _entry(2, tri * h, t)]
            else:
                l, o, d = f(r[15:16])[0], f(r[9:12]), f(r[12:15])
                entries += [_entry(1, np.array([-ROOT] * 3 + [ROOT] * 3, np.float32) * h, t, skip=1), _entry(2, f(r[0:9]) * h, t)]
            rays[k, 0:3], rays[k, 3:6], rays[k, 6] = o, d, l
        yield "%s rows %d.. (%s)" % (kind, at, "two spaces" if two_spaces else "one space"), _scene(entries, two_spaces, at), rays, [r[-2] if kind == "box" else r[-1] for r in chunk]


def same_walks(got, want):
    """flx_debug_walk's [n, 8] float32 against literal_walks' [n, 8] int64: (s, u, v) to the bit with NaN == NaN, the other columns as numbers; -> bool per ray"""
    gb, wb = got[:, 0:3].view(np.uint32).astype(np.int64), want[:, 0:3]
    nan = lambda b: (b & 0x7fffffff) > 0x7f800000
    return ((gb == wb) | (nan(gb) & nan(wb))).all(axis=1) & (got[:, 3:8].astype(np.int64) == want[:, 3:8]).all(axis=1)
