"""The walks where the LDS-staged tree top ends.  Every walk of the wavefront path reads the threaded, hot-first entry array from two places: entries
i < ldsCount from the copy its launch staged in LDS, every other one from global memory (walkFetchT / walkFetchP / walkFetchG / walkLoadEntry,
csrc/flx_device.h).  ldsCount is what is left of the launch's LDS after the pre-transformed rays, capped at the scene's walk_hot; it depends on the number of
transforms T and on the kernel (rounds, the frame kernel with two or three shade waves, the frame server and its slot depth).

Scenes of an exact size (synth_scene.make_sized) put walk_hot on either side of every such cap, of HOT_MAX (4096 entries ordered by depth) and of the
128-entry thresholds (lockstep copy, automatic pipeline, frame server).  flx_debug_last_walk_lds reports what a launch staged; flx_debug_walk_staged walks
single rays with any ldsCount and counts the fetches from each place.  Every frame and every walk is compared bit for bit, work counters included, with the
C oracle."""
import ctypes as C
import functools

import numpy as np
import pytest

import synth_scene
from flexlight_hip import capi

pytestmark = pytest.mark.gpu

F3 = C.c_float * 3
BIG = 5000                      # entries of the scenes well past every cap (walk_hot = 4097)
STAGED_LDS_LIMIT = 160 * 1024   # flx_debug_walk_staged's dynamic-LDS limit
# wavefront configurations: (organisation, front) -> the launch family that runs when the frame kernel fits
CONFIGS = {"rounds": (1, 0), "frame": (2, 0), "frame_front": (2, 2), "front_kernel": (2, 3)}
FAMILY = {"rounds": "rounds", "frame": "frame", "frame_front": "frame_front", "front_kernel": "frame"}
KIND = {"rounds": 1, "frame": 2, "frame_front": 3}


@functools.lru_cache(maxsize=None)
def sized(entries, n_transforms):
    return synth_scene.make_sized(entries, n_transforms, seed=10 * entries + n_transforms)


_oracle_frames = {}


def oracle_frame(oracle, entries, n_transforms):
    key = (entries, n_transforms)
    if key not in _oracle_frames:
        sc = sized(entries, n_transforms)
        want, cnt, _ = oracle.render(sc, sc.frame_params(use_filter=0))
        _oracle_frames[key] = (want, cnt)
    return _oracle_frames[key]


def config(hip, name):
    organisation, front = CONFIGS[name]
    hip.set_pipeline(3)
    hip.set_wavefront_organisation(organisation)
    hip.set_frame_front(front)


def restore(hip):
    hip.set_pipeline(0)
    hip.set_wavefront_organisation(0)
    hip.set_frame_front(1)
    hip.set_lockstep(True)


_caps = {}


def cap(hip, family, n_transforms):
    """the ldsCount a launch of this family takes at T transforms, read from the hook after a frame of a scene past every cap; None: the frame kernel does
    not take T (the frame went to the rounds)"""
    key = (family, n_transforms)
    if key not in _caps:
        sc = sized(BIG, n_transforms)
        hip.update_scene(sc)
        try:
            config(hip, family)
            hip.render(sc.frame_params(use_filter=0))
            info = hip.last_walk_lds()
        finally:
            restore(hip)
        assert info["walk_hot"] == 4097 and info["n_transforms"] == n_transforms, info
        if info["kind"] != KIND[family]:
            assert family != "rounds" and info["kind"] == 1, info
            _caps[key] = None
        else:
            assert 0 < info["lds_count"] < info["walk_hot"], info
            assert info["pre"] == (1 if family != "rounds" else int(n_transforms <= 3)), info
            _caps[key] = info["lds_count"]
    return _caps[key]


# ---- rays and the oracle's walks ---------------------------------------------------------------------------------------------------------------------

def threaded_order(g):
    """original entry index of every threaded index, as build_threaded (csrc/flx_scene.hip) lays them out: the shared terminator, the shallowest 4096 entries
    (stable by depth), the rest in original order"""
    depth, stack = np.zeros(g.shape[0], np.int64), []
    for i in range(g.shape[0]):
        while stack and i > stack[-1]:
            stack.pop()
        depth[i] = len(stack)
        if g[i, 10] == 1:
            stack.append(i + int(g[i, 6]))
    order = [i for i in range(g.shape[0]) if g[i, 10] != 0]
    by_depth = sorted(order, key=lambda i: depth[i])
    hot = set(by_depth[:4096])
    return [None] + by_depth[:4096] + [i for i in order if i not in hot]


def entry_centre(sc, i):
    g = sc.arrays["geometry"].reshape(-1, 12)
    local = g[i, :9].reshape(3, 3).mean(0) if g[i, 10] == 2 else 0.5 * (g[i, 0:3] + g[i, 3:6])
    t = int(g[i, 9])
    r = sc.arrays["rotation"].reshape(-1, 24)[t]
    m = np.stack([r[0:3], r[4:7], r[8:11]])
    return m @ local + sc.arrays["shift"].reshape(-1, 8)[t, 0:3]


def make_rays(sc, targets, seed):
    """camera rays, rays from inside the scene, axis-aligned rays, and rays aimed at the entries whose threaded indices are in `targets` (each side of
    every boundary tested) from points nearby: [n, 7] float32 (origin, direction, l)"""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-9.0, -7.0, 0.0]), np.array([9.0, 7.0, 20.0])
    cam = np.array([sc.meta["camera"][k] for k in "xyz"])
    rows = []
    for _ in range(900):
        rows.append((cam, rng.uniform(lo, hi) - cam))
    for _ in range(900):
        rows.append((rng.uniform(lo, hi), rng.normal(size=3)))
    for k in range(360):
        d = np.zeros(3)
        d[k % 3] = 1.0 if (k // 3) % 2 else -1.0
        if k >= 180:
            d[(k + 1) % 3] = rng.uniform(-1, 1)                  # one component zero
        rows.append((rng.uniform(lo, hi), d))
    order = threaded_order(sc.arrays["geometry"].reshape(-1, 12))
    for t in sorted(targets):
        if 1 <= t < len(order):
            c = entry_centre(sc, order[t])
            for _ in range(6):
                d = rng.normal(size=3)
                d /= np.linalg.norm(d)
                rows.append((c - 1.5 * d, d))
                rows.append((cam, c - cam))
    rays = np.zeros((len(rows), 7), np.float32)
    for j, (o, d) in enumerate(rows):
        rays[j, 0:3], rays[j, 3:6], rays[j, 6] = o, d, rng.uniform(0.5, 25.0)
    return rays


def oracle_walks(oracle, sc, rays):
    """[n, 8] like flx_debug_walk: s, u, v, transform, triangle, closest-hit visits, shadowed, shadow visits (flx_oracle_ray_tracer, flx_oracle_shadow_test)"""
    L = oracle.lib()
    L.flx_oracle_ray_tracer.argtypes = [C.c_void_p, F3, F3, F3, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
    L.flx_oracle_ray_tracer.restype = None
    L.flx_oracle_shadow_test.argtypes = [C.c_void_p, F3, F3, C.c_float, C.POINTER(C.c_uint64)]
    L.flx_oracle_shadow_test.restype = C.c_int
    view = sc.view()
    out = np.zeros((rays.shape[0], 8), np.float64)
    suv = np.zeros((rays.shape[0], 3), np.float32)
    for j, r in enumerate(rays):
        o, d = F3(*r[0:3]), F3(*r[3:6])
        s, ti, tri, v = F3(), C.c_int(), C.c_int(), C.c_uint64(0)
        L.flx_oracle_ray_tracer(C.byref(view), o, d, s, C.byref(ti), C.byref(tri), C.byref(v))
        suv[j] = list(s)
        out[j, 3:6] = ti.value, tri.value, v.value
        v2 = C.c_uint64(0)
        out[j, 6] = L.flx_oracle_shadow_test(C.byref(view), o, d, r[6], C.byref(v2))
        out[j, 7] = v2.value
    return suv, out


def staged_bytes(n_staged, n_transforms):
    return n_staged * 48 + n_transforms * 64 + 64 * n_transforms * 40


# ---- A. single rays with any ldsCount --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entries", [600, BIG])
@pytest.mark.parametrize("n_transforms", [1, 2, 3, 4, 6])
def test_staged_walk_equals_the_oracle_at_every_boundary(hip, oracle, n_transforms, entries):
    sc = sized(entries, n_transforms)
    caps = {c for c in (cap(hip, f, n_transforms) for f in ("rounds", "frame", "frame_front")) if c is not None}
    hip.update_scene(sc)
    info = hip.last_walk_lds()
    assert info["walk_hot"] == min(entries, 4096) + 1 and info["walk_entries"] == entries + 1
    assert (info["lds_count"], info["pre"], info["kind"], info["n_transforms"]) == (0, 0, 0, 0)      # nothing launched since the upload
    wh, full = info["walk_hot"], info["walk_entries"]
    fit = (STAGED_LDS_LIMIT - staged_bytes(0, n_transforms)) // 48                # the most the debug kernel can stage at this T
    values = sorted({0, 1, 2, 64, wh - 1, wh, wh + 1, min(fit, wh)} | caps)
    rays = make_rays(sc, {v for v in values if 0 < v < full} | {v - 1 for v in values if 1 < v <= full}, seed=entries + n_transforms)
    want_suv, want = oracle_walks(oracle, sc, rays)
    hit = want[:, 4] != -1
    assert hit.mean() > 0.3
    base = hip.debug_walk_staged(0, rays)
    assert (base[:, 8] == 0).all()
    ran = []
    for v in values:
        staged = min(v, wh)
        if staged_bytes(staged, n_transforms) > STAGED_LDS_LIMIT:
            with pytest.raises(capi.FlexLightHipError, match="LDS"):
                hip.debug_walk_staged(v, rays)
            continue
        got = hip.debug_walk_staged(v, rays)
        ran.append(v)
        assert np.array_equal(got[:, :8].view(np.uint32), base[:, :8].view(np.uint32)), v              # the same as the walk without LDS, to the bit
        assert np.array_equal(got[hit, 0:3].view(np.uint32), want_suv[hit].view(np.uint32)), v
        assert np.array_equal(got[:, 4], want[:, 4]), v
        assert np.array_equal(got[hit, 3], want[hit, 3]), v
        assert np.array_equal(got[:, 5], want[:, 5]) and np.array_equal(got[:, 7], want[:, 7]), v    # visits
        assert np.array_equal(got[:, 6], want[:, 6]), v
        assert np.array_equal(got[:, 8] + got[:, 9], want[:, 5] + want[:, 7]), v                      # every visit is one fetch from one place
        both = ((got[:, 8] > 0) & (got[:, 9] > 0)).mean()
        if staged == 0:
            assert (got[:, 8] == 0).all()
        elif staged >= full:
            assert (got[:, 9] == 0).all(), v                                                           # the whole tree in LDS
        elif staged <= 64:
            assert both > 0.9, (v, both)                    # every walk fetches the root (entry 1) or the terminator (entry 0) from LDS, most go deeper
        else:
            assert both > 0, (v, both)                      # (the rays aimed at entries v - 1 and v cross the boundary)
    assert ran[:4] == [0, 1, 2, 64]
    assert set(caps) & set(ran) or entries == BIG and n_transforms >= 4      # a production cap was walked unless none fits the debug kernel


# ---- B, E. frames of every organisation on both sides of its cap and of HOT_MAX ---------------------------------------------------------------------

def frame_cases():
    cases = []
    for T in (1, 2, 4, 5):
        for family in ("rounds", "frame", "frame_front") if T <= 4 else ("rounds",):      # (the frame kernel does not take five: the T5-big case)
            for d in (-1, 0, 1):
                cases.append(("cap", T, family, d))
        cases.append(("big", T, None, 0))
    for T in (1, 6):
        for entries in (4095, 4096, 4097, 6000):
            cases.append(("hot", T, None, entries))
    return cases


def case_id(c):
    kind, T, family, d = c
    return "T%d-%s" % (T, "%s%+d" % (family, d) if kind == "cap" else ("big" if kind == "big" else "hot%d" % d))


@pytest.mark.parametrize("case", frame_cases(), ids=case_id)
def test_frames_at_the_lds_boundary_equal_the_oracle(hip, oracle, case):
    kind, T, family, d = case
    caps = {f: cap(hip, f, T) for f in ("rounds", "frame", "frame_front")}        # (before this case's scene goes up)
    assert (caps["frame"] is None) == (caps["frame_front"] is None) == (T >= 5), caps      # the frame kernel takes T <= 4
    if kind == "cap":
        entries = caps[family] - 1 + d                       # walk_hot = cap + d
    else:
        entries = BIG if kind == "big" else d
    sc = sized(entries, T)
    want, want_cnt = oracle_frame(oracle, entries, T)
    hip.update_scene(sc)
    p = sc.frame_params(use_filter=0)
    try:
        for name in CONFIGS:
            config(hip, name)
            got, cnt, _ = hip.render(p, counters=True)
            info = hip.last_walk_lds()
            organisation = hip.last_organisation()
            assert np.array_equal(got, want, equal_nan=True), (name, entries, T)
            assert cnt == want_cnt, (name, entries, T)
            assert info["walk_hot"] == min(entries, 4096) + 1 and info["n_transforms"] == T
            c = caps[FAMILY[name]]
            if c is None:                                    # refused: the rounds take the frame
                assert organisation == 1 and info["kind"] == 1, (name, info)
                c = caps["rounds"]
            else:
                assert organisation == KIND[FAMILY[name]] and info["kind"] == organisation, (name, info)
            assert info["lds_count"] == min(c, info["walk_hot"]), (name, info, c)
            if kind == "cap" and FAMILY[name] == family:
                assert (info["walk_hot"] > info["lds_count"]) == (d == 1), (name, info)
    finally:
        restore(hip)


def test_the_caps_fall_where_the_budgets_put_them(hip):
    """what the hook reports, family by family (the caps the frame test above is built on): the frame kernel with the front inside has one shade wave
    more and so more LDS for the tree; the rounds give every thread rays up to three transforms and stage 3328 entries (156 KB) from four on; neither the
    frame kernel nor the server take five"""
    got = {(f, T): cap(hip, f, T) for f in ("rounds", "frame", "frame_front") for T in (1, 2, 3, 4, 5, 6)}
    print("ldsCount caps:", got)
    for T in (1, 2, 3, 4):
        assert got["frame", T] < got["frame_front", T]
        if T > 1:
            assert got["frame", T] < got["frame", T - 1] and got["rounds", T] != got["rounds", T - 1]
    assert got["rounds", 4] == got["rounds", 5] == got["rounds", 6] == 156 * 1024 // 48
    assert got["frame", 5] is None and got["frame_front", 5] is None and got["frame", 6] is None


# ---- C. the frame server ---------------------------------------------------------------------------------------------------------------------------

def _turned(sc, f):
    """the scene's last transform turned by 0.05 f about y (its inverse with it)"""
    r = np.array(sc.arrays["rotation"], np.float32).reshape(-1, 24).copy()
    t = r.shape[0] - 1
    c, s = np.cos(0.05 * f), np.sin(0.05 * f)
    turn = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    m = turn @ np.stack([r[t, 0:3], r[t, 4:7], r[t, 8:11]]).astype(np.float64)
    mi = np.linalg.inv(m)
    for k in range(3):
        r[t, 4 * k:4 * k + 3] = m[k]
        r[t, 12 + 4 * k:12 + 4 * k + 3] = mi[k]
    return r.reshape(-1)


@pytest.mark.parametrize("moving", [False, True], ids=["still", "moving"])
@pytest.mark.parametrize("n_transforms", [1, 2, 4, 5])
def test_served_frames_past_the_cap_equal_their_render(hip, n_transforms, moving):
    import copy
    sc = sized(BIG, n_transforms)
    hip.set_server_moving_scenes(moving)                     # still: every changed upload ends the launch, which reads the transforms once
    hip.update_scene(sc)
    hip.set_frame_chain(3)
    hip.set_frame_lanes(2)
    p = sc.frame_params(use_filter=0)
    try:
        assert hip.frame_server_takes(p) == (n_transforms <= 4)
        hip.frame_begin(p)                                   # (the frame that follows update_scene itself goes to the lanes)
        hip.frame_end()
        N = 6
        ps, got, kinds, flags = [], [], [], []
        for f in range(N):
            if hip.frames_in_flight() == 2:
                got.append(hip.frame_end()[0].copy())
            if moving and f >= 2:
                hip.update_transforms(_turned(sc, f), sc.arrays["shift"])
            q = copy.copy(p)
            q.random_seed = float(f % 3)
            q.camera[0] = p.camera[0] + 0.05 * f
            ps.append(q)
            hip.frame_begin(q)
            kinds.append(hip.last_chained())
            flags.append(hip.server_moving())
        while hip.frames_in_flight():
            got.append(hip.frame_end()[0].copy())
        info = hip.last_walk_lds()
        if n_transforms <= 4:
            assert kinds == [3] * N, kinds
            assert (info["kind"], info["pre"], info["n_transforms"]) == (4, 1, n_transforms), info
            assert 0 < info["lds_count"] < info["walk_hot"], info                     # the server walks past its LDS top
            assert flags == [False] * 2 + [moving] * (N - 2), flags     # a moving scene's launch takes the transforms per frame from the first move on
        else:
            assert 3 not in kinds, kinds
        for f in range(N):
            hip.update_transforms(_turned(sc, f) if moving and f >= 2 else sc.arrays["rotation"], sc.arrays["shift"])
            want = hip.render(ps[f])[0]
            assert np.array_equal(got[f], want, equal_nan=True), f
    finally:
        hip.update_transforms(sc.arrays["rotation"], sc.arrays["shift"])
        hip.set_server_moving_scenes(1)
        hip.set_frame_lanes(2)
        hip.set_frame_chain(2)


def test_a_moving_scene_gives_the_server_less_of_the_tree(hip):
    """a scene that moves keeps its transforms per slot in LDS: its launch stages fewer entries than the still scene's, and both frames are right"""
    import copy
    sc = sized(BIG, 4)
    hip.update_scene(sc)
    hip.set_frame_chain(3)
    p = sc.frame_params(use_filter=0)
    counts = []
    try:
        for moving in (False, True):
            hip.set_server_moving_scenes(moving)
            hip.frame_begin(p)
            hip.frame_end()
            for f in range(3):
                if moving:
                    hip.update_transforms(_turned(sc, f + 1), sc.arrays["shift"])
                q = copy.copy(p)
                q.random_seed = float(f)
                hip.frame_begin(q)
                assert hip.last_chained() == 3
                hip.frame_end()
            counts.append(hip.last_walk_lds()["lds_count"])
    finally:
        hip.update_transforms(sc.arrays["rotation"], sc.arrays["shift"])
        hip.set_server_moving_scenes(1)
        hip.set_frame_chain(2)
    assert 0 < counts[1] < counts[0] < 4097, counts


# ---- D. the 128-entry thresholds ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entries", [127, 128])
def test_the_128_entry_thresholds(hip, oracle, entries):
    small = entries + 1 <= 128                               # fwd_entries = walk_entries = entries + 1
    sc = sized(entries, 1)
    hip.update_scene(sc)
    info = hip.last_walk_lds()
    assert (info["fwd_entries"], info["walk_entries"], info["walk_hot"]) == (entries + 1, entries + 1, entries + 1)
    rays = make_rays(sc, set(), seed=entries)
    want_suv, want = oracle_walks(oracle, sc, rays)
    hit = want[:, 4] != -1
    for variant in (0, 1, 2):
        if variant == 2 and not small:
            with pytest.raises(capi.FlexLightHipError, match="lockstep"):
                hip.debug_walk(2, rays)
            continue
        got = hip.debug_walk(variant, rays)
        assert np.array_equal(got[hit, 0:3].view(np.uint32), want_suv[hit].view(np.uint32)), variant
        assert np.array_equal(got[:, 4:8], want[:, 4:8]), variant
    want_img, want_cnt = oracle_frame(oracle, entries, 1)
    p = sc.frame_params(use_filter=0)
    try:
        for pipeline in (1, 2):
            for lock in (True, False):
                hip.set_pipeline(pipeline)
                hip.set_lockstep(lock)
                got, cnt, _ = hip.render(p, counters=True)
                assert np.array_equal(got, want_img, equal_nan=True) and cnt == want_cnt, (pipeline, lock)
                if pipeline == 1:
                    assert hip.last_trace_kernel()[1] == int(lock and small), (lock, hip.last_trace_kernel())
        hip.set_pipeline(0)
        hip.set_lockstep(True)
        got, cnt, _ = hip.render(p, counters=True)
        assert np.array_equal(got, want_img, equal_nan=True) and cnt == want_cnt
        assert (hip.last_pipeline() == 3) == (not small), hip.last_pipeline()
        hip.set_frame_chain(3)
        assert hip.frame_server_takes(p) == (not small)
    finally:
        hip.set_frame_chain(2)
        restore(hip)
