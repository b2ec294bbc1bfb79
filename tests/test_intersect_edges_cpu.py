"""The adversarial intersection table (tests/golden/intersect_edge_kat.json.gz) on the CPU: the committed file is what its generator writes, it still holds the rows
per path that make it adversarial (so that a regenerated table cannot quietly lose them), and the C oracle's moellerTrumbore, moellerTrumboreCull, rayCuboid and
walks give the literal answers on its rows and scenes."""
import ctypes as C
import gzip
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from intersect_edges_util import far_triangle_scene, literal_walks, packed_scenes

HERE = os.path.dirname(os.path.abspath(__file__))
GEN = os.path.join(HERE, "analysis", "make_intersect_edge_kat.py")
F3 = C.c_float * 3
F9 = C.c_float * 9


@pytest.fixture(scope="module")
def kat():
    return json.load(gzip.open(os.path.join(HERE, "golden", "intersect_edge_kat.json.gz"), "rt"))


def test_generator_rederives_the_committed_table():
    """make_intersect_edge_kat.py --check: same seed, same rows, every quotient verified against exact rational arithmetic, every count condition asserted"""
    out = subprocess.run([sys.executable, "-W", "ignore", GEN, "--check"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "matches" in out.stdout


def test_committed_table_keeps_its_rows_per_path(kat):
    """the counts per class and per path of the device's decision structure, from the committed file: the conditions of the generator, and the figures themselves pinned"""
    import make_intersect_edge_kat as gen
    c = gen.counts(kat)
    gen.check_conditions(c)
    assert os.path.getsize(os.path.join(HERE, "golden", "intersect_edge_kat.json.gz")) < 512 * 1024
    assert all(len(r) == 16 for r in kat["ray_cuboid"]) and all(len(r) == 20 for r in kat["moeller_trumbore"]) and all(len(r) == 18 for r in kat["moeller_trumbore_cull"])
    assert c["box_nan_rows"] >= 30                                           # rows with a NaN in min / max are kept, pinned
    assert sum(c["margin"][k][0] + c["margin"][k][1] for k in c["margin"]) >= 300
    assert c["fallback_rows"] >= 1000


def test_oracle_on_the_edge_rows(oracle, kat):
    """the C oracle (oracle/flx_oracle.c) gives the same bits as the literal float32 transcription on every row, NaN rows (its own pin of min / max) included"""
    lib = oracle.lib()
    lib.flx_oracle_moeller_trumbore.argtypes = [F9, F3, F3, C.c_float, F3]
    lib.flx_oracle_moeller_trumbore_cull.argtypes = [F9, F3, F3, C.c_float]
    lib.flx_oracle_moeller_trumbore_cull.restype = C.c_int
    lib.flx_oracle_ray_cuboid.argtypes = [C.c_float, F3, F3, F3, F3]
    lib.flx_oracle_ray_cuboid.restype = C.c_int
    fl = lambda words: [struct.unpack("<f", struct.pack("<I", w))[0] for w in words]
    bits = lambda x: struct.unpack("<I", struct.pack("<f", x))[0]
    same = lambda got, want: all(g == w or (g & 0x7fffffff) > 0x7f800000 and (w & 0x7fffffff) > 0x7f800000 for g, w in zip(got, want))      # NaN == NaN
    for r in kat["moeller_trumbore"]:
        out = F3()
        lib.flx_oracle_moeller_trumbore(F9(*fl(r[0:9])), F3(*fl(r[9:12])), F3(*fl(r[12:15])), fl(r[15:16])[0], out)
        assert same([bits(x) for x in out], r[16:19]), r
    for r in kat["moeller_trumbore_cull"]:
        assert lib.flx_oracle_moeller_trumbore_cull(F9(*fl(r[0:9])), F3(*fl(r[9:12])), F3(*fl(r[12:15])), fl(r[15:16])[0]) == r[16], r
    for r in kat["ray_cuboid"]:
        assert lib.flx_oracle_ray_cuboid(fl(r[0:1])[0], F3(*fl(r[1:4])), F3(*fl(r[4:7])), F3(*fl(r[7:10])), F3(*fl(r[10:13]))) == r[13], r


def oracle_walks(oracle, sc, rays):
    """[n, 8] int64 in literal_walks' columns, from the C oracle's rayTracer and shadowTest"""
    L = oracle.lib()
    L.flx_oracle_ray_tracer.argtypes = [C.c_void_p, F3, F3, F3, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
    L.flx_oracle_ray_tracer.restype = None
    L.flx_oracle_shadow_test.argtypes = [C.c_void_p, F3, F3, C.c_float, C.POINTER(C.c_uint64)]
    L.flx_oracle_shadow_test.restype = C.c_int
    view = sc.view()
    out = []
    for r in rays:
        o, d = F3(*r[0:3]), F3(*r[3:6])
        s, ti, tri, v = F3(), C.c_int(), C.c_int(), C.c_uint64(0)
        L.flx_oracle_ray_tracer(C.byref(view), o, d, s, C.byref(ti), C.byref(tri), C.byref(v))
        got = [struct.unpack("<I", struct.pack("<f", x))[0] for x in s] + [ti.value if tri.value != -1 else 0, tri.value, v.value]
        v2 = C.c_uint64(0)
        out.append(got + [L.flx_oracle_shadow_test(C.byref(view), o, d, r[6], C.byref(v2)), v2.value])
    return np.array(out, np.int64)


@pytest.mark.parametrize("two_spaces", [False, True], ids=["one_space", "two_spaces"])
def test_oracle_walks_the_packed_rows(oracle, kat, two_spaces):
    """the table's rows packed into scenes of 32 (box, triangle) pairs: the oracle's walks against the literal walks — hit to the bit (NaN == NaN), entry, shadow answer, visits —
    and the scenes do what they are for: rays end in hits and misses, shadows and none, and visit counts vary from ray to ray"""
    nan = lambda b: (b & 0x7fffffff) > 0x7f800000
    scenes = hits = shadows = rays_total = 0
    visits = set()
    for name, sc, rays, classes in packed_scenes(kat, two_spaces):
        want, got = literal_walks(sc, rays), oracle_walks(oracle, sc, rays)
        same = ((got[:, 0:3] == want[:, 0:3]) | (nan(got[:, 0:3]) & nan(want[:, 0:3]))).all(axis=1) & (got[:, 3:8] == want[:, 3:8]).all(axis=1)
        assert same.all(), (name, [(classes[k], got[k].tolist(), want[k].tolist()) for k in np.flatnonzero(~same)[:3]])
        scenes, rays_total, hits, shadows = scenes + 1, rays_total + len(rays), hits + int((want[:, 4] != -1).sum()), shadows + int(want[:, 6].sum())
        visits |= set(want[:, 5].tolist())
    assert scenes >= 150 and hits >= rays_total // 5 and rays_total - hits >= rays_total // 10 and shadows >= rays_total // 20 and len(visits) >= 20


def test_oracle_walks_the_far_triangle_scene(oracle):
    """a triangle beyond 2^59 under bounded boxes: the oracle's rayTracer and shadowTest against the literal walks (hit to the bit, entry, shadow answer, visits)"""
    sc, rays = far_triangle_scene()
    want = literal_walks(sc, rays)
    L = oracle.lib()
    L.flx_oracle_ray_tracer.argtypes = [C.c_void_p, F3, F3, F3, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
    L.flx_oracle_ray_tracer.restype = None
    L.flx_oracle_shadow_test.argtypes = [C.c_void_p, F3, F3, C.c_float, C.POINTER(C.c_uint64)]
    L.flx_oracle_shadow_test.restype = C.c_int
    view = sc.view()
    g = sc.arrays["geometry"].reshape(-1, 12)
    assert (want[:, 4] != -1).sum() >= 5 and want[1::4, 6].sum() + want[2::4, 6].sum() >= 16      # objects are hit, the far floor shadows
    for r, w in zip(rays, want):
        o, d = F3(*r[0:3]), F3(*r[3:6])
        s, ti, tri, v = F3(), C.c_int(), C.c_int(), C.c_uint64(0)
        L.flx_oracle_ray_tracer(C.byref(view), o, d, s, C.byref(ti), C.byref(tri), C.byref(v))
        got = [struct.unpack("<I", struct.pack("<f", x))[0] for x in s] + [ti.value if tri.value != -1 else 0, tri.value, v.value]
        v2 = C.c_uint64(0)
        got += [L.flx_oracle_shadow_test(C.byref(view), o, d, r[6], C.byref(v2)), v2.value]
        assert got == list(w), (r, got, w)
