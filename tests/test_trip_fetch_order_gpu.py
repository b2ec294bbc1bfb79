"""The order of a walk trip's fetch (FLX_WALK_LANE_STEP, csrc/flx_frame_common.h; walkFetchIssue / walkFetchArrive, csrc/flx_device.h).  The persistent frame
kernels and the frame server issue the loads of a lane's next entry BEFORE the triangle test of the entry it stands at has run: a triangle's successor is its
link whatever the test says.  What may go wrong with that order, and the smallest scenes on which it would:

  * the change of object space replaces the ray the triangle test of the OLD entry still reads: a leaf's last triangle links across a LINK_XFORM seam
    (objects in different spaces back to back);
  * a shadow walk that ends on its triangle has loaded an entry it never visits: no visit may be counted for it, no ray reloaded, no end of walk read
    (lights inside the geometry, so that many shadow walks are cut short);
  * a triangle whose link is of kind 0 or 3 (the end of the list) or leads straight to another object's root: an object of ONE triangle;
  * a triangle and its successor on different sides of the LDS-staged tree top: walk_hot one below, at and one above the launch's ldsCount;
  * no LINK_XFORM at all: one transform.

Every scene runs with the front outside the frame kernel, inside it, and in a kernel of its own; counted and uncounted; one goes through the frame server.
Every frame is the oracle's bit for bit, and the work counters are the oracle's."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import synth_scene

pytestmark = pytest.mark.gpu

COUNTERS = ("closest_visits", "shadow_visits", "shades", "closest_walks", "shadow_walks")
FRONTS = {"front_outside": 0, "front_inside": 2, "front_kernel": 3}
FAMILY = {"front_outside": "frame", "front_inside": "frame_front", "front_kernel": "frame"}      # whose ldsCount the launch takes (tests/test_walk_lds_gpu.py)
KIND = {"frame": 2, "frame_front": 3}
LIGHTS_SEED = 1                 # chosen on the CPU: the oracle's shadow test cuts half of the sampled shadow walks short (cut_short_fraction: 0.496)
SINGLE_ENTRIES = 200
F3 = C.c_float * 3


def frame_params(sc):
    return sc.frame_params(width=64, height=48, samples=2, max_reflections=3, use_filter=0)


def config(hip, front):
    hip.set_pipeline(3)
    hip.set_wavefront_organisation(2)
    hip.set_frame_front(front)


def restore(hip):
    hip.set_pipeline(0)
    hip.set_wavefront_organisation(0)
    hip.set_frame_front(1)


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------------------

def world_triangles(sc):
    """[n, 3, 3] world-space vertices of the scene's triangles, and their entry indices"""
    g = sc.arrays["geometry"].reshape(-1, 12)
    rot = sc.arrays["rotation"].reshape(-1, 24)
    sh = sc.arrays["shift"].reshape(-1, 8)
    idx = np.flatnonzero(g[:, 10] == 2)
    out = np.zeros((idx.size, 3, 3))
    for k, i in enumerate(idx):
        t = int(g[i, 9])
        m = np.stack([rot[t, 0:3], rot[t, 4:7], rot[t, 8:11]]).astype(np.float64)
        out[k] = g[i, :9].reshape(3, 3).astype(np.float64) @ m.T + sh[t, 0:3]
    return out, idx


def top_level(sc):
    """(first entry, entries) of every child of the root box, in order"""
    g = sc.arrays["geometry"].reshape(-1, 12)
    end, i, kids = 1 + int(g[0, 6]), 1, []
    while i < end:
        n = 1 + (int(g[i, 6]) if g[i, 10] == 1 else 0)
        kids.append((i, n))
        i += n
    return kids


@functools.lru_cache(maxsize=None)
def seam_scene(n_lights=2, seed=0):
    return synth_scene.make(seed=seed, n_objects=3, tris_per_object=40, n_transforms=3, n_lights=n_lights)


@functools.lru_cache(maxsize=None)
def lights_scene():
    """the seam scene with its two lights at the centroids of two objects: inside the triangle soup, so that a shadow ray from almost anywhere meets a triangle"""
    base = seam_scene(2, LIGHTS_SEED)
    sc = copy.copy(base)
    tris, idx = world_triangles(base)
    objects = [k for k in top_level(base) if k[1] > 1]
    lights = np.array(base.arrays["lights"], np.float32).reshape(-1, 6).copy()
    for k in range(2):
        first, n = objects[k]
        inside = (idx >= first) & (idx < first + n)
        lights[k, 0:3] = tris[inside].reshape(-1, 3).mean(0)
    sc.arrays = dict(base.arrays, lights=lights.reshape(-1))
    return sc


def cut_short_fraction(oracle, sc):
    """the share of shadow walks that end on a triangle hit, by the oracle's own shadow test, over the rays from every triangle's centroid (lifted off its plane) to
    every light.  (The oracle counts walks and visits, not how a walk ended: its shadow test is asked directly.)"""
    L = oracle.lib()
    L.flx_oracle_shadow_test.argtypes = [C.c_void_p, F3, F3, C.c_float, C.POINTER(C.c_uint64)]
    L.flx_oracle_shadow_test.restype = C.c_int
    view = sc.view()
    tris, _ = world_triangles(sc)
    lights = sc.arrays["lights"].reshape(-1, 6)
    cut = total = 0
    for tri in tris:
        n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
        n /= np.linalg.norm(n) + 1e-30
        for light in lights:
            o = tri.mean(0)
            d = light[0:3].astype(np.float64) - o
            o = o + 1e-2 * (n if n @ d > 0 else -n)
            d = light[0:3].astype(np.float64) - o
            v = C.c_uint64(0)
            cut += L.flx_oracle_shadow_test(C.byref(view), F3(*o), F3(*d), float(np.linalg.norm(d)), C.byref(v))
            total += 1
    return cut / total


def with_single_triangle(base, which):
    """`base` with top-level object number `which` (counted among the objects, the floor's triangles left out) cut down to ONE triangle, a child of the root"""
    g = base.arrays["geometry"].reshape(-1, 12)
    a = base.arrays["attributes"].reshape(-1, 28)
    entries = 1 + int(g[0, 6])
    first, n = [k for k in top_level(base) if k[1] > 1][which]
    tri = first + int(np.flatnonzero(g[first:first + n, 10] == 2)[0])
    keep = list(range(first)) + [tri] + list(range(first + n, entries))
    padded = ((len(keep) + 255) // 256) * 256
    geometry, attributes = np.zeros((padded, 12), np.float32), np.zeros((padded, 28), np.float32)
    geometry[:len(keep)], attributes[:len(keep)] = g[keep], a[keep]
    geometry[0, 6] = len(keep) - 1
    ids = np.flatnonzero(geometry[:, 10] == 2).astype(np.int32)
    sc = copy.copy(base)
    sc.meta = dict(base.meta, textureLength=len(keep), bufferLength=int(ids.size), entriesPadded=padded)
    sc.arrays = dict(base.arrays, geometry=geometry.reshape(-1), attributes=attributes.reshape(-1), ids=ids)
    return sc


@functools.lru_cache(maxsize=None)
def single_scene(which):
    return with_single_triangle(synth_scene.make_sized(SINGLE_ENTRIES, 3, seed=7), which)


@functools.lru_cache(maxsize=None)
def sized(entries, n_transforms):
    return synth_scene.make_sized(entries, n_transforms, seed=10 * entries + n_transforms)


_caps = {}


def cap(hip, family):
    """the ldsCount a frame-kernel launch of this family stages at three transforms (flx_debug_last_walk_lds after a frame of a scene past every cap)"""
    if family not in _caps:
        sc = sized(5000, 3)
        hip.update_scene(sc)
        try:
            config(hip, 2 if family == "frame_front" else 0)
            hip.render(sc.frame_params(use_filter=0))
            info = hip.last_walk_lds()
        finally:
            restore(hip)
        assert info["kind"] == KIND[family] and info["n_transforms"] == 3 and 0 < info["lds_count"] < info["walk_hot"], info
        _caps[family] = info["lds_count"]
    return _caps[family]


def scene_of(hip, name, front_name):
    if name == "xform_seam":
        return seam_scene()
    if name == "lights_inside":
        return lights_scene()
    if name == "single_middle":
        return single_scene(1)
    if name == "single_last":
        return single_scene(2)
    if name.startswith("lds_top"):
        return sized(cap(hip, FAMILY[front_name]) - 1 + int(name[7:]), 3)      # walk_hot = cap + d
    if name == "one_transform":
        return sized(600, 1)
    if name == "one_transform_soup":
        return synth_scene.make(seed=1, n_objects=3, tris_per_object=40, n_transforms=1)
    raise KeyError(name)


_oracle_frames = {}


def oracle_frame(oracle, sc):
    if id(sc) not in _oracle_frames:
        want, cnt, _ = oracle.render(sc, frame_params(sc))
        _oracle_frames[id(sc)] = (sc, want, cnt)                 # (the scene is kept: its id stays its own)
    return _oracle_frames[id(sc)][1:]


SCENES = ["xform_seam", "lights_inside", "single_middle", "single_last", "lds_top-1", "lds_top+0", "lds_top+1", "one_transform", "one_transform_soup"]


# ---- the scenes are what they are meant to be (CPU side of the GPU cases) --------------------------------------------------------------------------------

def test_the_scenes_hold_what_the_cases_need(oracle):
    seam = seam_scene()
    g = seam.arrays["geometry"].reshape(-1, 12)
    kids = [k for k in top_level(seam) if k[1] > 1]
    assert len(kids) == 3
    for (first, n), (nxt, _) in zip(kids[:-1], kids[1:]):
        assert g[first + n - 1, 10] == 2 and g[nxt, 10] == 1 and g[first + n - 1, 9] != g[nxt, 9]      # a leaf's last triangle, then a root in another space
    frac = cut_short_fraction(oracle, lights_scene())
    print("shadow walks cut short (sampled):", frac)
    assert frac >= 0.25
    _, cnt = oracle_frame(oracle, lights_scene())
    assert cnt["shadow_walks"] > 1000
    for which in (1, 2):
        sc = single_scene(which)
        g = sc.arrays["geometry"].reshape(-1, 12)
        kids = top_level(sc)
        lone = [k for k in kids[2:] if k[1] == 1]
        assert len(lone) == 1 and g[lone[0][0], 10] == 2 and g[lone[0][0], 9] == which
        assert (lone[0] == kids[-1]) == (which == 2)                     # its successor: the next object's root, or the end of the list
        assert 1 + int(g[0, 6]) == sc.meta["textureLength"] and not g[sc.meta["textureLength"]:, 10].any()


# ---- the frames -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("front_name", list(FRONTS))
@pytest.mark.parametrize("name", SCENES)
def test_frames_equal_the_oracle_counted_and_uncounted(hip, oracle, name, front_name):
    sc = scene_of(hip, name, front_name)
    want, want_cnt = oracle_frame(oracle, sc)
    hip.update_scene(sc)
    p = frame_params(sc)
    try:
        config(hip, FRONTS[front_name])
        counted, cnt, _ = hip.render(p, counters=True)
        info, organisation = hip.last_walk_lds(), hip.last_organisation()
        plain = hip.render(p)[0]
    finally:
        restore(hip)
    assert organisation == KIND[FAMILY[front_name]] and info["kind"] == organisation, (organisation, info)      # the frame kernel rendered it
    if name.startswith("lds_top"):
        d = int(name[7:])
        assert info["lds_count"] == min(cap(hip, FAMILY[front_name]), info["walk_hot"]) and (info["walk_hot"] > info["lds_count"]) == (d == 1), info
    assert np.array_equal(counted, want, equal_nan=True)
    assert {k: cnt[k] for k in COUNTERS} == {k: want_cnt[k] for k in COUNTERS}
    assert np.array_equal(plain.view(np.uint32), counted.view(np.uint32))


@pytest.mark.parametrize("name", ["xform_seam", "lights_inside"])
def test_served_frames_equal_the_oracle(hip, oracle, name):
    """the same trip in k_wf_server: frames through the frame server, three in flight"""
    sc = scene_of(hip, name, "front_outside")
    want, _ = oracle_frame(oracle, sc)
    hip.update_scene(sc)
    hip.set_frame_chain(3)
    hip.set_frame_lanes(3)
    p = frame_params(sc)
    try:
        assert hip.frame_server_takes(p)
        hip.frame_begin(p)                                       # (the frame that follows update_scene itself goes to the lanes)
        hip.frame_end()
        got, kinds = [], []
        for _ in range(4):
            if hip.frames_in_flight() == 3:
                got.append(hip.frame_end()[0].copy())
            hip.frame_begin(p)
            kinds.append(hip.last_chained())
        while hip.frames_in_flight():
            got.append(hip.frame_end()[0].copy())
        assert kinds == [3] * 4, kinds
        assert hip.last_walk_lds()["kind"] == 4
        for f in got:
            assert np.array_equal(f, want, equal_nan=True)
    finally:
        hip.set_frame_lanes(2)
        hip.set_frame_chain(2)
