"""Helpers of the flx_scene_update tests: a host-side re-flatten of a scene whose vertices moved (the flatten's own recursion over the children of every box,
with Math.min / Math.max's order of zeros — modules/scene.js:242-256, 269-279), scenes made by hand, and the refit rule in plain numpy."""
import copy

import numpy as np

import synth_scene


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def js_min(a, b):
    """Math.min of two float32 arrays without NaN: -0 is below +0"""
    return np.where(a == b, np.where(np.signbit(a), a, b), np.minimum(a, b)).astype(np.float32)


def js_max(a, b):
    return np.where(a == b, np.where(np.signbit(a), b, a), np.maximum(a, b)).astype(np.float32)


def reflatten(geometry):
    """geometry [n, 12] -> a copy whose box rows (kind 1) hold what the flatten computes from the triangle rows as they stand: a box joins the boxes of its
    children, a triangle's box is the min / max of its vertices.  A box with nothing beneath it (skip 0), or with no triangle beneath it, keeps its floats."""
    g = np.array(geometry, np.float32).reshape(-1, 12).copy()
    n = g.shape[0]
    lo = np.zeros((n, 3), np.float32)
    hi = np.zeros((n, 3), np.float32)
    has = np.zeros(n, bool)
    for i in range(n - 1, -1, -1):
        kind = g[i, 10]
        if kind == 2:
            v = g[i, :9].reshape(3, 3)
            lo[i] = js_min(js_min(v[0], v[1]), v[2])
            hi[i] = js_max(js_max(v[0], v[1]), v[2])
            has[i] = True
        elif kind == 1:
            j, end = i + 1, i + int(g[i, 6])
            while j <= end:                                   # the children, each with its subtree behind it
                if has[j]:
                    lo[i], hi[i] = (js_min(lo[i], lo[j]), js_max(hi[i], hi[j])) if has[i] else (lo[j].copy(), hi[j].copy())
                    has[i] = True
                j += 1 + (int(g[j, 6]) if g[j, 10] == 1 else 0)
            if has[i]:
                g[i, 0:3], g[i, 3:6] = lo[i], hi[i]
    return g


def refit_rule(geometry):
    """THE RULE flx_scene_update's kernel implements, literally: words 0..5 of box row i with skip s > 0 = min / max (as unsigned keys that order -0 below +0)
    over the vertices of all triangle rows in (i, i + s].  -> (boxes [n, 6] float32, answered [n] bool: box rows with a triangle beneath them)"""
    g = np.ascontiguousarray(geometry, np.float32).reshape(-1, 12)
    n = g.shape[0]
    u = g[:, :9].view(np.uint32).astype(np.int64)
    key = np.where(u & 0x80000000, 0xffffffff - u, u | 0x80000000).reshape(n, 3, 3)      # [row, vertex, axis]
    tri = g[:, 10] == 2
    kmin = np.where(tri[:, None], key.min(1), 0xffffffff)
    kmax = np.where(tri[:, None], key.max(1), 0)
    # sparse tables of the two range queries
    tmin, tmax = [kmin], [kmax]
    w = 1
    while 2 * w <= n:
        tmin.append(np.minimum(tmin[-1][:n - 2 * w + 1], tmin[-1][w:n - w + 1]))
        tmax.append(np.maximum(tmax[-1][:n - 2 * w + 1], tmax[-1][w:n - w + 1]))
        w *= 2
    out = np.zeros((n, 6), np.float32)
    answered = np.zeros(n, bool)
    boxes = np.flatnonzero((g[:, 10] == 1) & (g[:, 6] >= 1))
    lo, hi = boxes + 1, boxes + g[boxes, 6].astype(np.int64)
    level = np.floor(np.log2(hi - lo + 1)).astype(np.int64)
    for k in np.unique(level):
        at = level == k
        mn = np.minimum(tmin[k][lo[at]], tmin[k][hi[at] - (1 << k) + 1])
        mx = np.maximum(tmax[k][lo[at]], tmax[k][hi[at] - (1 << k) + 1])
        some = ~((mn[:, 0] == 0xffffffff) & (mx[:, 0] == 0))
        keys = np.concatenate([mn, mx], axis=1)[some]
        back = np.where(keys & 0x80000000, keys & 0x7fffffff, 0xffffffff - keys).astype(np.uint32)
        out[boxes[at][some]] = back.view(np.float32)
        answered[boxes[at][some]] = True
    return out, answered


def reflatten_by_rule(geometry):
    """reflatten() for scenes too large for its loop: the boxes by refit_rule (vectorised)"""
    g = np.array(geometry, np.float32).reshape(-1, 12).copy()
    boxes, answered = refit_rule(g)
    g[answered, :6] = boxes[answered]
    return g


def with_geometry(scene, geometry, attributes=None):
    sc = copy.copy(scene)
    sc.arrays = dict(scene.arrays, geometry=np.ascontiguousarray(geometry, np.float32).reshape(-1))
    if attributes is not None:
        sc.arrays["attributes"] = np.ascontiguousarray(attributes, np.float32).reshape(-1)
    return sc


def moved(scene, seed, rows=None, scale=0.2, attributes=True, flatten=None):
    """the scene with the vertices (and, attributes=True, the normals) of the triangle rows in `rows` (a slice; None: all) moved by a seeded rng, re-flattened"""
    rng = np.random.default_rng(seed)
    g = scene.arrays["geometry"].reshape(-1, 12).copy()
    a = scene.arrays["attributes"].reshape(-1, 28).copy()
    pick = np.zeros(g.shape[0], bool)
    pick[rows if rows is not None else slice(None)] = True
    pick &= g[:, 10] == 2
    g[pick, :9] += rng.normal(scale=scale, size=(int(pick.sum()), 9)).astype(np.float32)
    if attributes:
        a[pick, :9] += rng.normal(scale=0.05, size=(int(pick.sum()), 9)).astype(np.float32)
    return with_geometry(scene, (flatten or reflatten)(g), a)


def rows_for_update(scene, first, count, seed=99):
    """rows [first, first + count) of the scene as an application hands them to flx_scene_update: words 0..5 of the box rows are NOT the boxes (the device
    computes them) but noise"""
    g = scene.arrays["geometry"].reshape(-1, 12)[first:first + count].copy()
    a = scene.arrays["attributes"].reshape(-1, 28)[first:first + count].copy()
    box = g[:, 10] == 1
    g[box, :6] = np.random.default_rng(seed).normal(scale=100.0, size=(int(box.sum()), 6)).astype(np.float32)
    return g, a


def by_hand(entries, seed=0, width=64, height=48):
    """entries: [('box', skip, six floats or None) | ('tri', nine floats)] in transform 0 -> Scene (one light, no textures)"""
    geo, att = [], []
    for e in entries:
        g = np.zeros(12, np.float32)
        a = np.zeros(28, np.float32)
        if e[0] == "box":
            g[6], g[10] = e[1], 1
            if e[2] is not None:
                g[:6] = e[2]
        else:
            g[:9], g[10] = e[1], 2
            a[0:9] = np.tile([0, 0, -1], 3)
            a[15:18] = -1
            a[18:24] = [0.8, 0.7, 0.6, 1, 0, 0]
            a[24:27] = [0, 0, 1]
        geo.append(g)
        att.append(a)
    rotation = np.zeros((1, 24), np.float32)
    rotation[0, [0, 5, 10, 12, 17, 22]] = 1
    sc = synth_scene._package(np.random.default_rng(seed), seed, geo, att, rotation, np.zeros((1, 8), np.float32), 1, 1, 0, width, height, 2, 3, False)
    return with_geometry(sc, reflatten(sc.arrays["geometry"]))


TRIANGLE = [-3.0, -2.0, 6.0, 3.0, -2.0, 6.5, 0.0, 3.0, 7.0]


def chain(depth=40):
    """`depth` nested boxes over one triangle"""
    return by_hand([("box", depth - k, None) for k in range(depth)] + [("tri", TRIANGLE)])


def layered(groups=7, leaves=7100, tris=3, seed=0):
    """A root box over `groups` boxes over `leaves` boxes of `tris` triangles each, made without a Python loop per entry: with the defaults 198 808 entries, 777 blocks
    of 256 in 4 superblocks of 65 536 — group boxes that end inside a superblock, reach its end and cross into the next one, a root over whole superblocks."""
    rng = np.random.default_rng(seed)
    leaf = 1 + tris
    group = 1 + leaves * leaf
    n = 1 + groups * group
    g = np.zeros((n, 12), np.float32)
    a = np.zeros((n, 28), np.float32)
    g[:, 10] = 2
    g[0, 6], g[0, 10] = n - 1, 1
    starts = 1 + group * np.arange(groups)
    g[starts, 6], g[starts, 10] = group - 1, 1
    leaf_at = (starts[:, None] + 1 + leaf * np.arange(leaves)[None, :]).reshape(-1)
    g[leaf_at, 6], g[leaf_at, 10] = tris, 1
    tri = g[:, 10] == 2
    centre = rng.uniform(-8, 8, (int(tri.sum()), 1, 3)) + [0, 0, 12]
    g[tri, :9] = (centre + rng.normal(scale=0.1, size=(int(tri.sum()), 3, 3))).reshape(-1, 9)
    a[tri, 0:9] = np.tile([0, 0, -1], 3)
    a[tri, 15:18] = -1
    a[tri, 18:24] = [0.8, 0.7, 0.6, 1, 0, 0]
    a[tri, 24:27] = [0, 0, 1]
    rotation = np.zeros((1, 24), np.float32)
    rotation[0, [0, 5, 10, 12, 17, 22]] = 1
    sc = synth_scene._package(rng, seed, list(reflatten_by_rule(g)), list(a), rotation, np.zeros((1, 8), np.float32), 1, 1, 0, 64, 48, 2, 3, False)
    return sc
