"""Helpers of the first-hit-order tests (test_ray_order_cpu.py, test_ray_order_gpu.py, test_ray_order_js_gpu.py): the CPU reference of bounds and keys built once per
session, a hand-made table of slabs as ray rows with synthetic hit rows, an independent numpy computation of bounds, cells and keys, and the obvious Morton loop."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ray_order_ref"))
import flx_ray_order_ref  # noqa: E402

DEAD = 0xFFFFFFFF
_ref = []


def reference(tmp_path_factory):
    """the CPU reference, built once per session"""
    if not _ref:
        _ref.append(flx_ray_order_ref.build(str(tmp_path_factory.mktemp("ray_order_ref"))))
    return _ref[0]


def rows_at(points, entries=None):
    """ray rows and hit rows whose hit points are exactly `points` [n, 3]: the origin is the point, s is 1 and the direction a zero of the point's sign (p + 0 keeps
    every bit of p, -0 included).  entries: the hit rows' word 3 (by default 7, a hit)"""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    n = len(points)
    rays, hits = np.zeros((n, 8), np.float32), np.zeros((n, 8), np.uint32)
    rays[:, 0:3] = points
    rays[:, 4:7] = np.copysign(np.float32(0.0), points)
    rays[:, 3], rays[:, 7] = np.linspace(-1, 1, n, endpoint=False), np.linspace(1, -1, n, endpoint=False)
    hits[:, 0] = np.float32(1.0).view(np.uint32)
    hits[:, 3] = np.full(n, 7, np.int32).view(np.uint32) if entries is None else np.asarray(entries, np.int32).view(np.uint32)
    return rays, hits


def tables():
    """name -> (ray rows, hit rows): the slabs of the hand-made table"""
    rng = np.random.default_rng(20)
    out = {}
    # rays whose hit points take a multiplication and an addition, with a NaN and an infinite hit point among them, a miss, and points on lo and hi
    n = 300
    rays, hits = np.zeros((n, 8), np.float32), np.zeros((n, 8), np.uint32)
    rays[:, 0:3] = rng.uniform(-5, 5, (n, 3))
    rays[:, 4:7] = rng.normal(size=(n, 3)) * rng.uniform(0.25, 4.0, (n, 1))
    s = rng.uniform(0.01, 20.0, n).astype(np.float32)
    entry = rng.integers(0, 1000, n).astype(np.int32)
    s[10], s[11], s[12] = np.nan, np.inf, -np.inf                   # first hits at no finite point: dead, though the entry says hit
    entry[20:40:3] = -1                                             # misses (their s is what cast_rays writes: 0)
    s[20:40:3] = 0.0
    hits[:, 0], hits[:, 3] = s.view(np.uint32), entry.view(np.uint32)
    hits[:, 1:3] = rng.uniform(0, 1, (n, 2)).astype(np.float32).view(np.uint32)
    out["general"] = (rays, hits)
    # a flat axis: every y equal
    p = rng.uniform(-2, 2, (64, 3)).astype(np.float32)
    p[:, 1] = np.float32(0.75)
    out["flat axis"] = rows_at(p)
    # -0 and +0: alone on x (lo = -0, hi = +0: an extent of 0), with larger values on y (lo = -0), with smaller ones on z (hi = +0)
    p = np.zeros((8, 3), np.float32)
    p[:, 0] = [-0.0, 0.0, 0.0, -0.0, 0.0, -0.0, -0.0, 0.0]
    p[:, 1] = [0.0, -0.0, 1.0, 2.0, 0.5, 0.25, -0.0, 0.0]
    p[:, 2] = [0.0, -0.0, -1.0, -2.0, -0.5, -0.25, -0.0, 0.0]
    out["zeros"] = rows_at(p)
    # an extent that overflows: hi - lo = inf on x; y and z ordinary
    p = rng.uniform(-1, 1, (16, 3)).astype(np.float32)
    p[:, 0] = np.where(np.arange(16) % 2 == 0, np.float32(-3e38), np.float32(3e38))
    p[5, 0] = 0.0
    out["overflow"] = rows_at(p)
    # misses only
    out["misses"] = rows_at(rng.uniform(-1, 1, (70, 3)), entries=np.full(70, -1))
    # one live ray alone, among misses
    e = np.full(9, -1)
    e[4] = 3
    out["one live"] = rows_at(rng.uniform(-1, 1, (9, 3)), entries=e)
    # one ray
    out["one ray"] = rows_at([[1.0, 2.0, 3.0]])
    return out


def mapped(bits):
    """the sign-flip mapping of float bits to uint32, in numpy"""
    bits = np.asarray(bits, np.uint32)
    return np.where(bits >> 31 != 0, ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def morton_loop(qx, qy, qz):
    """the obvious loop: bit 3k+2 is x's bit k, 3k+1 y's, 3k z's"""
    key = 0
    for k in range(10):
        key |= ((int(qx) >> k) & 1) << (3 * k + 2) | ((int(qy) >> k) & 1) << (3 * k + 1) | ((int(qz) >> k) & 1) << (3 * k)
    return key


def numpy_keys(rays, hits):
    """-> (keys uint32 [n], lo float32 [3], hi float32 [3], cells uint32 [n, 3], live bool [n]) in numpy's float32, an operation a rounding; lo / hi None where no ray
    is live"""
    rays, hits = np.asarray(rays, np.float32).reshape(-1, 8), np.ascontiguousarray(hits).reshape(len(rays), -1).view(np.uint32)
    n = len(rays)
    with np.errstate(all="ignore"):
        s = hits[:, 0:1].view(np.float32)
        sd = (s * rays[:, 4:7]).astype(np.float32)
        p = (rays[:, 0:3] + sd).astype(np.float32)
        live = (hits[:, 3].view(np.int32) != -1) & np.isfinite(p).all(axis=1)
        keys, cells = np.full(n, DEAD, np.uint32), np.zeros((n, 3), np.uint32)
        if not live.any():
            return keys, None, None, cells, live
        lo, hi = np.zeros(3, np.float32), np.zeros(3, np.float32)
        for k in range(3):
            m = mapped(p[live, k].view(np.uint32))
            lo[k], hi[k] = p[live, k][np.argmin(m)], p[live, k][np.argmax(m)]
            e = np.float32(hi[k] - lo[k])
            if e > 0 and np.isfinite(e):
                scale = np.float32(np.float32(1024.0) / e)
                t = ((p[:, k] - lo[k]).astype(np.float32) * scale).astype(np.float32)
                cells[live, k] = np.minimum(np.float32(1023.0), np.floor(t[live])).astype(np.uint32)
        for i in np.flatnonzero(live):
            keys[i] = morton_loop(*cells[i])
    return keys, lo, hi, cells, live
