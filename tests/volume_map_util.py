"""Helpers of the directional-visibility tests (test_volume_map_cpu.py, test_volume_map_gpu.py, test_volume_map_seams_gpu.py, test_volume_map_js_gpu.py): the CPU
reference built once per session, synthetic radiance rows and maps, the point sets of the lookup tests, and float64 restatements of include/flx_volume_map.h's
decode, encode, map rows and lookup written by hand."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "volume_map_ref"))
import flx_volume_map_ref  # noqa: E402

from probe_util import SPARE, finished, poisoned, quadrature64  # noqa: E402,F401
from volume_util import COUNTS, POINT_SETS, grid_of, irradiance64, point_set, synthetic_sh, unit_normals  # noqa: E402,F401
from volume_util import reference as volume_reference  # noqa: E402,F401

_ref = []


def reference(tmp_path_factory):
    """the CPU reference, built once per session"""
    if not _ref:
        _ref.append(flx_volume_map_ref.build(str(tmp_path_factory.mktemp("volume_map_ref"))))
    return _ref[0]


def map_of(size, sharpness):
    from flexlight_hip import capi
    return capi.VolumeMap(size, sharpness)


def same_rows(got, want):
    """float32 [n, k] against the same: bit for bit, or a NaN where a NaN is wanted (a sum that meets a NaN is some NaN) -> bool [n]"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, "%s against %s" % (got.shape, want.shape)
    return ((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all(axis=1)


def assert_same_rows(got, want, what=""):
    ok = same_rows(got, want)
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, "%s: %d of %d rows differ, first %d: got %s want %s" % (what, bad.size, len(ok), bad[0], np.asarray(got)[bad[0]], np.asarray(want)[bad[0]])


def map_radiance(n_probes, face_size, seed, nan=True):
    """radiance rows float32 [n_probes * 6 w w, 8] with a fixed seed: about a third of a probe's rows are misses (zeros); distances span 2^-4 .. 2^4.  Where there are
    three probes or more, probe 1 is only misses and probe 2 only hits.  nan: the last probe's texel 0 hits at a NaN distance."""
    rng = np.random.default_rng(seed)
    rays = 6 * face_size * face_size
    n = n_probes * rays
    rows = np.zeros((n, 8), np.float32)
    rows[:, 0:3] = rng.uniform(0.0, 2.0, size=(n, 3))
    rows[:, 3] = rng.choice(np.array([1.0, 0.5, 7.0], np.float32), size=n)
    rows[:, 4] = np.exp2(rng.uniform(-4.0, 4.0, size=n))
    miss = (rng.random(n) < 1.0 / 3.0).reshape(n_probes, rays)
    if n_probes >= 3:
        miss[1], miss[2] = True, False
    rows[miss.reshape(-1)] = 0.0
    if nan:
        at = (n_probes - 1) * rays
        rows[at, 3], rows[at, 4] = 1.0, np.nan
    return rows


def wall_radiance(ref, face_size):
    """the probe of the issue's table: a wall one unit away on its +x side, open space to ten units elsewhere — rays with dx > 0 hit at min(1 / dx, 10), all others
    at 10; every texel hits"""
    rays = 6 * face_size * face_size
    rows = np.zeros((rays, 8), np.float32)
    rows[:, 0:4] = 1.0
    for t in range(rays):
        d, _ = ref.texel(face_size, t)
        rows[t, 4] = min(1.0 / float(d[0]), 10.0) if d[0] > 0 else 10.0
    return rows


def synthetic_maps(probes, size, seed):
    """map rows float32 [probes * m m, 4] with a fixed seed, by kind = (row + seed) % 6:
      0, 1  coverage > 0, a mean distance of 0.2 .. 2 and a variance of 0.2 .. 1 times its square
      2     q[0] = 0: nothing hit in that direction
      3     a negative q[0]
      4     variance exactly 0: coverage 2, mean 1.5, mean square 2.25
      5     a mean of 1000, beyond every distance of the tests
    and row 1 of every seventh probe holds a NaN mean"""
    rng = np.random.default_rng(seed)
    n = probes * size * size
    weight = rng.uniform(0.5, 1.0, size=n)
    coverage = weight * rng.uniform(0.3, 1.0, size=n)
    mean = rng.uniform(0.2, 2.0, size=n)
    var = mean * mean * rng.uniform(0.2, 1.0, size=n)
    kind = (np.arange(n) + seed) % 6
    mean = np.where(kind == 5, 1000.0, mean)
    rows = np.stack([coverage, coverage * mean, coverage * (mean * mean + var), weight], axis=1)
    rows[kind == 2, 0:3] = 0.0
    rows[kind == 3, 0] *= -1.0
    rows[kind == 4, 0:3] = (2.0, 3.0, 4.5)
    rows = rows.astype(np.float32)
    nan_rows = np.arange(0, probes, 7) * size * size + (1 if size > 1 else 0)
    rows[nan_rows, 1] = np.nan
    return rows


# ---- float64 restatements, written by hand from include/flexlight_hip_debug.h's "directional visibility" ----

def ndc64(i, m):
    return (i + 0.5) / m * 2.0 - 1.0


def sgn64(a):
    return 1.0 if a >= 0.0 else -1.0


def decode64(u, v):
    z = 1.0 - abs(u) - abs(v)
    x, y = ((1.0 - abs(v)) * sgn64(u), (1.0 - abs(u)) * sgn64(v)) if z < 0.0 else (u, v)
    d = np.array([x, y, z], np.float64)
    return d / np.sqrt((d * d).sum())


def encode64(m, d):
    """-> (bin, margin): margin is the least distance of the two grid coordinates from a whole number — where it is tiny, float32 may round into the next bin"""
    x, y, z = [float(a) for a in d]
    l1 = abs(x) + abs(y) + abs(z)
    if not l1 > 0.0:
        return 0, np.inf
    px, py = x / l1, y / l1
    if z < 0.0:
        px, py = (1.0 - abs(py)) * sgn64(px), (1.0 - abs(px)) * sgn64(py)
    index, margin = [], np.inf
    for p in (px, py):
        g = max((p + 1.0) * 0.5 * m, 0.0)
        index.append(min(int(g), m - 1))
        margin = min(margin, abs(g - round(g)))
    return index[1] * m + index[0], margin


def map_rows64(radiance, face_size, size, sharpness):
    """one probe's radiance rows float32 [6 w w, 8] -> its map rows float64 [m m, 4]"""
    radiance = np.asarray(radiance, np.float32).reshape(-1, 8)
    d, dw, _ = quadrature64(face_size)
    hit = radiance[:, 3] != 0.0
    s = radiance[:, 4].astype(np.float64)
    out = np.zeros((size * size, 4), np.float64)
    for b in range(size * size):
        direction = decode64(ndc64(b % size, size), ndc64(b // size, size))
        c = np.maximum(d @ direction, 0.0) ** (2 ** sharpness)
        g = dw * c
        out[b] = [(g * hit).sum(), (g * s)[hit].sum(), (g * s * s)[hit].sum(), g.sum()]
    return out


def lookup_map64(grid, vmap, sh, maps, position, normal):
    """The lookup with maps restated by hand in float64 over the same float32 inputs.
    -> (row float64 [4], margin, bin margin): margin as volume_util.lookup64's for the branch dist > mean, bin margin the least encode64 margin over the corners"""
    origin, spacing = np.array(list(grid.origin), np.float64), np.array(list(grid.spacing), np.float64)
    count = [int(c) for c in grid.count]
    position, n = np.asarray(position, np.float64), np.asarray(normal, np.float64)[:3]
    sh = np.asarray(sh, np.float64).reshape(-1, 36)
    maps = np.asarray(maps, np.float64).reshape(-1, 4)
    m = int(vmap.size)
    if position[3] == 0.0:
        return np.zeros(4), np.inf, np.inf
    x = n * float(grid.normal_bias) + position[:3]
    g = (x - origin) / spacing
    base, f = [0, 0, 0], [0.0, 0.0, 0.0]
    for a in range(3):
        q = g[a] if g[a] >= 0.0 else 0.0
        q = q if q <= count[a] - 1 else float(count[a] - 1)
        base[a] = min(int(q), count[a] - 2) if count[a] >= 2 else 0
        f[a] = q - base[a]
    total, s, margin, bin_margin = 0.0, np.zeros(3), np.inf, np.inf
    for k in range(8):
        bit = [(k >> a) & 1 for a in range(3)]
        at_ = [min(base[a] + bit[a], count[a] - 1) for a in range(3)]
        p = (at_[2] * count[1] + at_[1]) * count[0] + at_[0]
        t = 1.0
        for a in range(3):
            t *= f[a] if bit[a] else 1.0 - f[a]
        d = origin + np.array(at_, np.float64) * spacing - x
        dist = np.sqrt((d * d).sum())
        direction = d / dist if dist != 0.0 else np.zeros(3)
        c = (float(direction @ n) + 1.0) * 0.5
        wb = c * c + 0.2
        b, bm = encode64(m, -direction)
        bin_margin = min(bin_margin, bm)
        q = maps[p * m * m + b]
        wv = 1.0
        if (grid.flags & 1) and q[0] > 0.0:
            mean, mean2 = q[1] / q[0], q[2] / q[0]
            var = abs(mean2 - mean * mean)
            margin = min(margin, abs(dist - mean) / max(dist, mean))
            if dist > mean:
                delta = dist - mean
                den = var + delta * delta
                ch = var / den if den > 0.0 else 0.0
                wv = max(ch * ch * ch, float(grid.floor))
        w = t * wb * wv
        total += w
        s += w * irradiance64(sh[p], n)
    if total > 0.0:
        return np.array([s[0] / total, s[1] / total, s[2] / total, total]), margin, bin_margin
    return np.zeros(4), margin, bin_margin
