"""Helpers of the probe-volume tests (test_volume_cpu.py, test_volume_gpu.py, test_volume_js_gpu.py): the CPU reference built once per session, grids, synthetic
SH rows, the point sets at which the lookup kernel takes another path, and a float64 restatement of include/flx_volume.h's lookup written by hand."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "volume_ref"))
import flx_volume_ref  # noqa: E402

from probe_util import A, assert_same_words, basis64  # noqa: E402,F401

COUNTS = ((1, 1, 1), (2, 2, 2), (3, 2, 4), (1, 3, 1))      # one probe; one cell; several cells with an odd count; a line of probes across the second axis
ORIGIN = (-1.0, 0.5, 2.0)
SPACING = (0.75, 1.25, 0.5)
POINT_SETS = ("one_cell", "alternate", "one_lane", "faces", "outside", "misses", "miss_wave", "all_miss")

_ref = []


def reference(tmp_path_factory):
    """the CPU reference, built once per session"""
    if not _ref:
        _ref.append(flx_volume_ref.build(str(tmp_path_factory.mktemp("volume_ref"))))
    return _ref[0]


def grid_of(count, normal_bias=0.0, visibility=True, floor=0.05):
    from flexlight_hip import capi
    return capi.VolumeGrid(ORIGIN, SPACING, count, normal_bias, floor, capi.VOLUME_VISIBILITY if visibility else 0)


def synthetic_sh(probes, seed):
    """SH rows float32 [probes, 36] with a fixed seed.  Band 0 is 1 .. 2 and the other coefficients are within 0.2, so that an irradiance is well away from 0 for
    every unit normal.  The moments go by kind = (probe + seed) % 4:
      0  coverage > 0, a mean distance of 0.2 .. 2 and a variance of 0.2 .. 1 times its square
      1  no coverage: words 7, 11 and 15 are 0.0
      2  variance exactly 0: coverage 2, mean 1.5 (sum 3), mean square 2.25 (sum 4.5) — every operation exact
      3  a mean of 1000, beyond every distance of the tests"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((probes, 9, 4), np.float64)
    rows[:, :, 0:3] = rng.uniform(-0.2, 0.2, size=(probes, 9, 3))
    rows[:, 0, 0:3] = rng.uniform(1.0, 2.0, size=(probes, 3))
    weight = rng.uniform(12.0, 13.0, size=probes)
    coverage = weight * rng.uniform(0.3, 1.0, size=probes)
    mean = rng.uniform(0.2, 2.0, size=probes)
    var = mean * mean * rng.uniform(0.2, 1.0, size=probes)
    kind = (np.arange(probes) + seed) % 4
    mean = np.where(kind == 3, 1000.0, mean)
    rows[:, 0, 3] = weight
    rows[:, 1, 3] = coverage
    rows[:, 2, 3] = coverage * mean
    rows[:, 3, 3] = coverage * (mean * mean + var)
    rows[kind == 1, 1:4, 3] = 0.0
    rows[kind == 2, 1, 3], rows[kind == 2, 2, 3], rows[kind == 2, 3, 3] = 2.0, 3.0, 4.5
    return rows.reshape(probes, 36).astype(np.float32)


def unit_normals(rng, n):
    v = rng.normal(size=(n, 3))
    v /= np.sqrt((v * v).sum(axis=1, keepdims=True))
    out = np.zeros((n, 4), np.float32)
    out[:, :3] = v
    out[:, 3] = rng.choice([-1.0, 0.0, 1.0], size=n)      # signDir, which the lookup ignores
    return out


def at(grid, g):
    """grid coordinates float64 [n, 3] -> positions float32 [n, 3]: origin + (float32)g * spacing in float32, one rounding per operation — a probe's own position
    for whole numbers"""
    g32 = np.asarray(g, np.float64).astype(np.float32)
    step = (g32 * np.array(list(grid.spacing), np.float32)).astype(np.float32)
    return (np.array(list(grid.origin), np.float32) + step).astype(np.float32)


def point_set(grid, kind, n, seed):
    """-> (positions float32 [n, 4], normals float32 [n, 4]) of one of POINT_SETS:
      one_cell   every point inside the cell at the grid's origin: a wave's lanes read the same eight rows
      alternate  points alternating lane by lane between the first cell and the last one (where the grid has two cells)
      one_lane   the first cell, but lane 37 of every wave (the last point of a shorter one) in the last cell
      faces      whole and half grid coordinates: points on cell faces, on edges and at probe positions (distance 0 where there is no bias)
      outside    grid coordinates from 3 cells below the grid to 3 above it, and some far away
      misses     the first cell and the last, a third of the points misses (word 3 is 0.0 or -0.0; a hit's is 1.0, 5.0 or a NaN)
      miss_wave  one_cell with lanes 64 .. 127 all misses
      all_miss   nothing but misses"""
    rng = np.random.default_rng(seed)
    count = np.array(list(grid.count), np.float64)
    cells = np.maximum(count - 1.0, 1.0)
    inside = rng.uniform(0.1, 0.9, size=(n, 3))
    last = np.maximum(count - 2.0, 0.0)
    lane = np.arange(n)
    if kind in ("one_cell", "miss_wave", "all_miss"):
        g = inside
    elif kind == "alternate":
        g = inside + np.where((lane % 2 == 1)[:, None], last, 0.0)
    elif kind == "one_lane":
        odd = (lane % 64 == 37) | (lane == n - 1)
        g = inside + np.where(odd[:, None], last, 0.0)
    elif kind == "faces":
        g = np.floor(rng.uniform(0.0, 2.0 * cells + 1.0, size=(n, 3))) / 2.0
    elif kind == "outside":
        g = rng.uniform(-3.0, count + 2.0, size=(n, 3))
        g[::7] *= 1.0e6
    elif kind == "misses":
        g = inside + np.where((rng.random(n) < 0.5)[:, None], last, 0.0)
    else:
        raise ValueError(kind)
    positions = np.ones((n, 4), np.float32)
    positions[:, :3] = at(grid, g)
    if kind == "misses":
        word = rng.choice(np.array([0.0, -0.0, 1.0, 1.0, 5.0, np.nan], np.float32), size=n)
        positions[:, 3] = word
    if kind == "miss_wave":
        positions[64:128, 3] = 0.0
    if kind == "all_miss":
        positions[:, 3] = 0.0
    return positions, unit_normals(rng, n)


def irradiance64(row, n):
    """an SH row float64 [36] -> E float64 [3] for the normal, as include/flx_probe.h defines it"""
    b = basis64(np.asarray(n, np.float64))
    p = row.reshape(9, 4)[:, 0:3] * b[:, None]
    return A[0] * p[0] + A[1] * p[1:4].sum(axis=0) + A[2] * p[4:9].sum(axis=0)


def lookup64(grid, sh, position, normal):
    """The lookup of include/flexlight_hip_debug.h ("probe volumes", steps 1 - 7) restated by hand in float64 over the same float32 inputs.
    -> (row float64 [4], margin): margin is the least |dist - mean| / max(dist, mean) over the corners whose visibility branch was asked (inf where none was)"""
    origin, spacing = np.array(list(grid.origin), np.float64), np.array(list(grid.spacing), np.float64)
    count = [int(c) for c in grid.count]
    position, n = np.asarray(position, np.float64), np.asarray(normal, np.float64)[:3]
    sh = np.asarray(sh, np.float64).reshape(-1, 36)
    if position[3] == 0.0:
        return np.zeros(4), np.inf
    x = n * float(grid.normal_bias) + position[:3]
    g = (x - origin) / spacing
    base, f = [0, 0, 0], [0.0, 0.0, 0.0]
    for a in range(3):
        q = g[a] if g[a] >= 0.0 else 0.0
        q = q if q <= count[a] - 1 else float(count[a] - 1)
        base[a] = min(int(q), count[a] - 2) if count[a] >= 2 else 0
        f[a] = q - base[a]
    total, s, margin = 0.0, np.zeros(3), np.inf
    for k in range(8):
        bit = [(k >> a) & 1 for a in range(3)]
        at_ = [min(base[a] + bit[a], count[a] - 1) for a in range(3)]
        row = sh[(at_[2] * count[1] + at_[1]) * count[0] + at_[0]]
        t = 1.0
        for a in range(3):
            t *= f[a] if bit[a] else 1.0 - f[a]
        d = origin + np.array(at_, np.float64) * spacing - x
        dist = np.sqrt((d * d).sum())
        direction = d / dist if dist != 0.0 else np.zeros(3)
        c = (float(direction @ n) + 1.0) * 0.5
        wb = c * c + 0.2
        wv = 1.0
        if (grid.flags & 1) and row[7] > 0.0:
            mean, mean2 = row[11] / row[7], row[15] / row[7]
            var = abs(mean2 - mean * mean)
            margin = min(margin, abs(dist - mean) / max(dist, mean))
            if dist > mean:
                delta = dist - mean
                den = var + delta * delta
                ch = var / den if den > 0.0 else 0.0
                wv = max(ch * ch * ch, float(grid.floor))
        w = t * wb * wv
        total += w
        s += w * irradiance64(row, n)
    if total > 0.0:
        return np.array([s[0] / total, s[1] / total, s[2] / total, total]), margin
    return np.zeros(4), margin
