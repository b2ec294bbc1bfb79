"""Shared by tests/test_box_single_cpu.py and tests/test_box_single_gpu.py: box-test rows built to land in each outcome of the interval test's single-comparison form
(csrc/flx_device.h: rayCuboidInterval<true>), the oracle's rayCuboid over rows, and small scenes with and without flat boxes.

A row is flx_debug_intersect's box row: l, origin 3, direction 3, min 3, max 3 (13 float32)."""
import ctypes as C

import numpy as np

from scene_update_util import by_hand, reflatten, with_geometry

F3 = C.c_float * 3
D21 = 2.0 ** -21                # the interval test's lo(x) = x - 2^-21 |x|, hi(x) = x + 2^-21 |x|
LO, HI, OHI = 2.0 ** -60, 2.0 ** 60, 2.0 ** 59


def oracle_ray_cuboid(oracle, rows):
    """the oracle's rayCuboid (fragment:161-167) of every row -> float32 0 / 1"""
    lib = oracle.lib()
    lib.flx_oracle_ray_cuboid.argtypes = [C.c_float, F3, F3, F3, F3]
    lib.flx_oracle_ray_cuboid.restype = C.c_int
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 13)
    return np.array([lib.flx_oracle_ray_cuboid(float(r[0]), F3(*r[1:4]), F3(*r[4:7]), F3(*r[7:10]), F3(*r[10:13])) for r in rows], np.float32)


def ulps(x, k):
    """x moved by k float32 steps (k may be negative)"""
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
    return x


def _row(l, o, d, mn, mx):
    return np.array([l] + list(o) + list(d) + list(mn) + list(mx), np.float32)


def _axes(row, perm):
    """the row with its three axes permuted"""
    out = row.copy()
    for base in (1, 4, 7, 10):
        out[base:base + 3] = row[base:base + 3][list(perm)]
    return out


PERMS = ((0, 1, 2), (1, 2, 0), (2, 0, 1))


def graze_rows():
    """a ray that enters through the y slab at tmin and leaves through the x slab at tmax (z: a slab far wider), the two differing by 0, +-1, 2, 4, 8 float32 steps and by
    just under and just over 2^-20 relative — the corner of the box grazed from outside and from inside the interval test's tolerance — with quotients that are exact
    (a direction of ones) and quotients that round; every arrangement of the axes.  The form is sure of a hit from tmax / tmin >= (1 + 2^-21) / (1 - 2^-21), 1 + 2^-20
    and a little; a corner coordinate, a reciprocal and a product round by 2^-24 each, which moves the ratio of the two products by up to 6 x 2^-24 = 0.375 x 2^-20:
    "under" is 0.6 x 2^-20 and "over" 1.4 x 2^-20, clear of the border by more than that.  -> (rows, classes)"""
    rows, classes = [], []
    rng = np.random.default_rng(41)
    for t in [np.float32(3.7), np.float32(1.0), np.float32(4096.0)] + list(rng.uniform(0.5, 90.0, 5).astype(np.float32)):
        gaps = [("%+d_ulp" % k, ulps(t, k)) for k in (0, 1, -1, 2, -2, 4, -4, 8, -8)]
        for name, factor in (("under_2^-20", 1.0 + 0.6 * 2.0 ** -20), ("over_2^-20", 1.0 + 1.4 * 2.0 ** -20), ("over_2^-19", 1.0 + 2.0 ** -19)):
            gaps += [("+" + name, np.float32(t * factor)), ("-" + name, np.float32(t / factor))]
        for d in ((1.0, 1.0, 2.0 ** -10), (0.7, 0.7, 0.1), (0.3, 0.3, -0.2)):
            for name, far in gaps:
                # o = 0: tmin = y0 / d.y, tmax = x1 / d.x, with y0 = t d.y and x1 = far d.x as float32 products; x0 below, y1 above
                y0, x1 = np.float32(t * np.float32(d[1])), np.float32(far * np.float32(d[0]))
                row = _row(1.0e9, (0.0, 0.0, 0.0), d, (x1 - np.float32(2.0), y0, -1000.0), (x1, y0 + np.float32(2.0), 1000.0))
                for perm in PERMS:
                    rows.append(_axes(row, perm))
                    classes.append("graze " + name)
    return np.array(rows, np.float32), classes


def flat_rows():
    """a flat box on each axis (min == max there), crossed inside its rectangle and beside it, from both sides, with l beyond and short of the plane"""
    rows, classes = [], []
    rng = np.random.default_rng(42)
    for k in range(40):
        plane = np.float32(rng.uniform(-5, 5))
        lo, size = rng.uniform(-4, 0, 2).astype(np.float32), rng.uniform(0.5, 4, 2).astype(np.float32)
        inside = rng.uniform(0.1, 0.9, 2)
        side = -1.0 if k % 2 else 1.0
        for hit in (True, False):
            p = lo + size * (inside if hit else inside + 1.5)                  # where the ray crosses the plane
            o = np.array([plane - side * rng.uniform(1, 6), p[0] - rng.uniform(-1, 1), p[1] - rng.uniform(-1, 1)], np.float32)
            d = np.array([plane, p[0], p[1]], np.float32) - o
            d = (d / np.linalg.norm(d)).astype(np.float32)
            dist = float(np.linalg.norm(np.array([plane, p[0], p[1]], np.float64) - o))
            for l, what in ((1.0e9, "long"), (0.5 * dist, "short")):
                row = _row(l, o, d, (plane, lo[0], lo[1]), (plane, lo[0] + size[0], lo[1] + size[1]))
                for perm in PERMS:
                    rows.append(_axes(row, perm))
                    classes.append("flat axis %d %s l %s" % (perm.index(0), "crossed" if hit else "missed", what))
    return np.array(rows, np.float32), classes


def on_face_rows():
    """the origin exactly on a face of the box (one quotient is zero), leaving, entering and sliding along it; on the plane of a flat box too"""
    rows, classes = [], []
    rng = np.random.default_rng(43)
    for k in range(30):
        mn = rng.uniform(-4, 0, 3).astype(np.float32)
        mx = (mn + rng.uniform(0.5, 4, 3)).astype(np.float32)
        if k % 3 == 0:
            mx[0] = mn[0]                                                   # flat on the axis the origin stands on
        o = (mn + (mx - mn) * rng.uniform(0.2, 0.8, 3)).astype(np.float32)
        o[0] = mn[0] if k % 2 else mx[0]
        for name, dx in (("into", 0.5), ("out_of", -0.5), ("along", 0.0)):
            d = np.array([dx if k % 2 else -dx, rng.uniform(-1, 1), rng.uniform(-1, 1)], np.float32)
            row = _row(1.0e9 if k % 5 else 0.25, o, d, mn, mx)
            for perm in PERMS:
                rows.append(_axes(row, perm))
                classes.append("origin on a face %s%s" % (name, " flat" if k % 3 == 0 else ""))
    return np.array(rows, np.float32), classes


def short_l_rows():
    """l below 2^-60 (the interval test does not decide), zero, denormal: from inside the box (tmin < 0 < l) and from outside"""
    rows, classes = [], []
    for l in (2.0 ** -61, ulps(2.0 ** -60, -1), 2.0 ** -60, ulps(2.0 ** -60, 1), 2.0 ** -70, 2.0 ** -130, 1.0e-45, 0.0):
        for o, where in (((0.1, 0.2, 0.3), "inside"), ((0.1, 0.2, -5.0), "outside"), ((1.0, 0.2, 0.3), "on a face")):
            row = _row(l, o, (0.3, 0.2, 0.9), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
            for perm in PERMS:
                rows.append(_axes(row, perm))
                classes.append("l %g from %s" % (l, where))
    return np.array(rows, np.float32), classes


def direction_rows():
    """a direction component outside the range in which the reciprocal is proven (|d| below 2^-60, above 2^60, zero, infinite, NaN), and an origin beyond 2^59"""
    rows, classes = [], []
    values = [0.0, -0.0, 1.0e-40, 2.0 ** -61, ulps(2.0 ** -60, -1), 2.0 ** -60, ulps(2.0 ** 60, 1), 2.0 ** 60, 2.0 ** 61, np.inf, -np.inf, np.nan]
    for v in values:
        for o in ((0.1, 0.2, -5.0), (0.1, 0.2, 0.3), (3.0, 0.2, -5.0)):
            row = _row(1.0e9, o, (v, 0.2, 0.9), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
            for perm in PERMS:
                rows.append(_axes(row, perm))
                classes.append("direction %r" % float(np.float32(v)))
    for v in (ulps(OHI, -1), OHI, ulps(OHI, 1), 2.0 ** 61):
        row = _row(np.inf, (0.1, 0.2, -v), (0.0, 0.0, 1.0), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
        for perm in PERMS:
            rows.append(_axes(row, perm))
            classes.append("origin at %r" % float(np.float32(v)))
    return np.array(rows, np.float32), classes


def nan_corner_rows():
    """NaN in one of the six corner coordinates (such a scene is not bounded: walk_fast_boxes = 0), with rays that would hit and miss the box without it"""
    rows, classes = [], []
    for at in range(6):
        for o, d in (((0.1, 0.2, -5.0), (0.0, 0.0, 1.0)), ((0.1, 0.2, -5.0), (0.01, 0.02, 1.0)), ((3.0, 0.2, -5.0), (0.01, 0.02, 1.0)), ((0.1, 0.2, 0.3), (0.3, -0.2, 0.9))):
            row = _row(1.0e9, o, d, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
            row[7 + at] = np.nan
            rows.append(row)
            classes.append("NaN in corner word %d" % at)
    return np.array(rows, np.float32), classes


def bounded_rows():
    """every family whose boxes keep flx_scene_upload's bound -> (rows, classes)"""
    parts = [graze_rows(), flat_rows(), on_face_rows(), short_l_rows(), direction_rows()]
    return np.concatenate([p[0] for p in parts]), sum((p[1] for p in parts), [])


# ---- the interval test's single-comparison form, restated (which outcome a row lands in) -------------------------------------------------------------------------

def single_form_outcome(row):
    """'true' / 'false' / 'unsure' of rayCuboidInterval<true> for a row of a bounded scene, from float32 products as the device makes them (NaN: unsure)"""
    f = np.float32
    r = np.asarray(row, np.float32)
    l, o, d, mn, mx = r[0], r[1:4], r[4:7], r[7:10], r[10:13]
    with np.errstate(all="ignore"):
        ad = np.abs(d)
        fast = bool(np.all((ad >= f(LO)) & (ad <= f(HI))) and np.all(np.abs(o) <= f(OHI)))
        y = (f(1.0) / d).astype(np.float32)
        q0, q1 = ((mn - o) * y).astype(np.float32), ((mx - o) * y).astype(np.float32)
        near, far = np.fmin(q0, q1), np.fmax(q0, q1)
        tmin, tmax = f(np.fmax(np.fmax(near[0], near[1]), near[2])), f(np.fmin(np.fmin(far[0], far[1]), far[2]))
        fma = lambda a, b, c: f(np.float64(a) * np.float64(b) + np.float64(c))          # (a product of two float32 is exact in float64: one rounding, as the FMA)
        tmin_hi, tmin_lo = fma(abs(tmin), f(D21), tmin), fma(-abs(tmin), f(D21), tmin)
        tmax_hi, tmax_lo = fma(abs(tmax), f(D21), tmax), fma(-abs(tmax), f(D21), tmax)
        bias = f(2.0 ** -16)
        sure_true = bool(tmax_lo >= tmin_hi) and bool(tmax_lo >= bias) and bool(tmin_hi < l)
        sure_false = bool(tmax_hi < np.fmax(tmin_lo, bias)) or bool(tmin_lo >= l)
    if not (fast and bool(l >= f(LO)) and (sure_true or sure_false)):
        return "unsure"
    return "true" if sure_true else "false"


# ---- small scenes ------------------------------------------------------------------------------------------------------------------------------------------------

LEAVES = 12


def _leaf_triangles(k, flat):
    """two triangles of leaf k in a 4 x 3 grid in front of the camera: a quad in a plane x, y or z = const (flat: its box has no room on that axis) or a tilted pair"""
    cx, cy, cz = -4.5 + 3.0 * (k % 4), -3.0 + 3.0 * (k // 4), 7.0 + 0.25 * (k % 3)
    if flat:
        axis = (k // 2) % 3
        corners = {0: [(cx, cy - 1, cz - 1), (cx, cy + 1, cz - 1), (cx, cy + 1, cz + 1), (cx, cy - 1, cz + 1)],
                   1: [(cx - 1, cy, cz - 1), (cx + 1, cy, cz - 1), (cx + 1, cy, cz + 1), (cx - 1, cy, cz + 1)],
                   2: [(cx - 1, cy - 1, cz), (cx + 1, cy - 1, cz), (cx + 1, cy + 1, cz), (cx - 1, cy + 1, cz)]}[axis]
    else:
        corners = [(cx - 1, cy - 1, cz - 0.5), (cx + 1, cy - 1, cz + 0.25), (cx + 1, cy + 1, cz + 0.5), (cx - 1, cy + 1, cz - 0.25)]
    a, b, c, d = [list(map(float, p)) for p in corners]
    return [a + b + c, a + c + d]


def leaf_scene(flat_leaves, width=96, height=54):
    """a root box over LEAVES boxes of two triangles each (37 entries); the leaves in `flat_leaves` are flat: -> Scene"""
    entries = [("box", 3 * LEAVES, None)]
    for k in range(LEAVES):
        tris = _leaf_triangles(k, k in flat_leaves)
        entries += [("box", 2, None), ("tri", tris[0]), ("tri", tris[1])]
    return by_hand(entries, seed=7, width=width, height=height)


def half_flat_scene(**kw):
    """half of the leaf boxes flat: two on each axis"""
    return leaf_scene(set(range(0, LEAVES, 2)), **kw)


def thick_scene(**kw):
    return leaf_scene(set(), **kw)


def flattened(scene, leaf):
    """the scene with the two triangles of leaf `leaf` moved into the plane z = 7 (its box is flat afterwards), re-flattened -> (scene, first row, rows [3, 12] as an
    application hands them to flx_scene_update)"""
    g = scene.arrays["geometry"].reshape(-1, 12).copy()
    first = 1 + 3 * leaf
    assert g[first, 10] == 1 and g[first, 6] == 2
    g[first + 1:first + 3, [2, 5, 8]] = 7.0
    return with_geometry(scene, reflatten(g)), first, g[first:first + 3].copy()


def thick_numpy(geometry):
    """flx_debug_boxes_thick restated: every box row has min < max on all three axes (NaN fails the comparison)"""
    g = np.ascontiguousarray(geometry, np.float32).reshape(-1, 12)
    box = g[g[:, 10] == 1]
    with np.errstate(invalid="ignore"):
        return int(bool(np.all(box[:, 0:3] < box[:, 3:6])))
