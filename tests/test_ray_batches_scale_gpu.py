"""The ray-batch calls at the sizes their users run them at (flx_rays_cast, flx_rays_trace, flx_rays_trace_ordered, flx_rays_surface, flx_rays_planes, their _device
forms, and flx_debug_hit_keys), bit for bit against the references the small tests use: full persistent grids — one workgroup of k_ray_query per compute unit,
eight of k_rays_paths / k_rays_planes —, the slab loop at the library's own ceiling (2^21 rays, or (2^24 / samples) & ~63), and k_hit_bounds beyond one trip of its
grid.  No knob is set: no set_trace_slab, no set_query_groups.  The natural values are the subject, so the sizes are what they are; they come from the launch rules
and the device's compute units.

A row depends on its ray row and the scene alone (csrc/flx_rays_trace.hip's header; a cast's hit row, a surface row and the five planes likewise: k_ray_query,
k_surface and k_rays_planes read rays[r], hits[r] and the scene, and the noise is the ray row's words 3 and 7), so a batch of any size is tiled from the base rays
the small tests have reference rows for (ray_scale_util): nothing new is computed on the CPU but the rows at the one new sample count.  Every output goes into a
buffer poisoned with 0xA5 with eight spare rows behind the last; all words of all rows are compared, a NaN equal to a NaN only where the call's own same_rows lets
it; the rays stay as they were.  Each case prints the wall time of its call."""
import numpy as np
import pytest
import torch

from flexlight_hip import capi
from ray_order_util import reference as key_reference, rows_at
from ray_query_util import expected_words, pack_rays, same_rows as same_hit_rows, scene_walks, words_of
from ray_scale_util import assert_tiled, base_of, exactly, index_map, poisoned, rays_unchanged, rows_of, tiled_rays, timed
from rays_planes_util import PLANES, quant, reference as planes_reference, same_floats, wanted as planes_wanted
from rays_trace_util import camera_rays, free_rays, reference as trace_reference, same_rows as same_radiance_rows, trace_params
from surface_util import BITS, HIT, NORMAL, TPO, planes_of, reference as surface_reference
from test_ray_order_gpu import shuffled_camera_rays
from test_rays_trace_gpu import wanted as trace_wanted
from test_surface_gpu import free_wanted as surface_wanted

pytestmark = pytest.mark.gpu

QUERY_LANES = 1024                 # lanes of a workgroup of k_ray_query (QUERY_THREADS, csrc/flx_query.hip)
QUERY_WAVES = QUERY_LANES // 64
PATH_LANES = 256                   # lanes of a workgroup of k_rays_paths and k_rays_planes: four waves, a wave a unit of 64 rays
SLAB = 1 << 21                     # FLX_TRACE_SLAB_RAYS (csrc/flx_query_args.h): the rays of a natural slab up to eight samples
SLOTS = 1 << 24                    # FLX_TRACE_SLAB_SLOTS: from nine samples on a slab has (SLOTS / samples) & ~63 rays
S1 = SLAB + 65                     # one natural slab, then a block of 64 rays and one ray
SLAB9 = (SLOTS // 9) & ~63
S9 = SLAB9 + 65
BOUNDS_LANES = 262144              # ORDER_BOUNDS_GROUPS (1024) * ORDER_THREADS (256), csrc/flx_rays_order.hip: the rays one trip of k_hit_bounds' grid takes


def cus(hip):
    return hip.device_info()[1]


def Q1(hip):
    """one ray more than a lane of every workgroup of k_ray_query's full grid takes: launch_ray_query asks for C + 1 workgroups and gets C"""
    return cus(hip) * QUERY_LANES + 1


def P1(hip):
    """at one sample k_rays_paths, and k_rays_planes at any, ask for one workgroup beyond cus * 8"""
    return cus(hip) * 8 * PATH_LANES + 1


def path_groups(hip, rays, samples):
    """workgroups of k_rays_paths for a slab of `rays` rays: four (block of 64 rays, sample) units fill one, at most eight a compute unit"""
    return min(-(-(-(-rays // 64) * samples) // 4), cus(hip) * 8)


def query_groups(hip, rays):
    return min(-(-rays // QUERY_LANES), cus(hip))


@pytest.fixture(autouse=True)
def released():
    """the big tensors of a test go back to the device when it ends: the largest case holds a few hundred MB"""
    yield
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def trace_ref(tmp_path_factory, oracle):
    return trace_reference(tmp_path_factory)


@pytest.fixture(scope="module")
def planes_ref(tmp_path_factory, oracle):
    return planes_reference(tmp_path_factory)


@pytest.fixture(scope="module")
def surface_ref(tmp_path_factory, oracle):
    return surface_reference(tmp_path_factory)


@pytest.fixture(scope="module")
def keys_ref(tmp_path_factory):
    return key_reference(tmp_path_factory)


# ---- 1. casts ------------------------------------------------------------------------------------------------------------------------------------------------------------

def cast(hip, base, idx, what, label):
    """the tiled rays through cast_rays_device into a poisoned buffer -> (hit rows int32 [n, 8] on the device, the record of the launch)"""
    n = idx.shape[0]
    d = tiled_rays(base, idx)
    out = poisoned(n, 32)
    with timed(hip, "flx_rays_cast_device, %s, %d rays, what %d" % (label, n, what)):
        assert hip.cast_rays_device(d, out, what) is out
    got = rows_of(out, n, 32)
    assert rays_unchanged(d, base, idx)
    return got, hip.last_query()


@pytest.mark.parametrize("entries,n_transforms", [(600, 3), (5000, 4)])
def test_casts_on_the_full_grid(hip, oracle, entries, n_transforms):
    """600 entries, three transforms: pre-transformed rays, the whole tree in LDS; 5000 entries, four transforms: rays transformed on the fly, the tree partly in LDS.
    C * 1024 rays give every lane of the full grid one ray, one more makes a lane take a second while the other waves draw from the same cursor, and 2^21 + 65 make
    every lane take eight and more (a cast is one launch whatever n: the slab loop is not its)."""
    sc, rays7, want_suv, want = scene_walks(oracle, entries, n_transforms)
    base, label = pack_rays(rays7), "%d entries, %d transforms" % (entries, n_transforms)
    C, chunk = cus(hip), capi.QUERY_CHUNK
    hip.update_scene(sc)
    for n, what in ((C * QUERY_LANES, 7), (Q1(hip), 7), (Q1(hip), 3), (S1, 7)):
        idx = index_map(n, len(base))
        got, info = cast(hip, base, idx, what, label)
        assert_tiled(got, expected_words(want_suv, want, what), idx, same_hit_rows, "%s n %d what %d" % (label, n, what))
        groups = query_groups(hip, n)
        assert groups == C and (n == C * QUERY_LANES or groups * QUERY_LANES < n)      # the full grid, and beyond C * 1024 rays fewer lanes than rays
        assert (info["n"], info["what"], info["chunk"], info["groups"], info["pre"]) == (n, what, chunk, groups, int(n_transforms <= 3)), info
        assert info["draws"] == -(-n // chunk) + groups * QUERY_WAVES and 1 <= info["waves"] <= groups * QUERY_WAVES, info      # every wave ends on one draw past the last chunk
        if entries == 600:
            assert info["lds_count"] == 601
        else:
            assert 0 < info["lds_count"] < 4097
        del got, idx


# ---- 2. traces ------------------------------------------------------------------------------------------------------------------------------------------------------------

def traced(hip, base, idx, t, label, order=None):
    """the tiled rays through trace_rays_device (order None) or trace_rays_ordered_device into a poisoned buffer -> radiance rows int32 [n, 8] on the device"""
    n = idx.shape[0]
    d = tiled_rays(base, idx)
    out = poisoned(n, 32)
    if order is None:
        with timed(hip, "flx_rays_trace_device, %s, %d rays, %d samples, %d bounces" % (label, n, t.samples, t.max_reflections)):
            assert hip.trace_rays_device(d, t, out) is out
    else:
        with timed(hip, "flx_rays_trace_ordered_device, %s, %d rays, %d samples, %d bounces" % (label, n, t.samples, t.max_reflections)):
            assert hip.trace_rays_ordered_device(d, t, out, order=order) is out
    got = rows_of(out, n, 32)
    assert rays_unchanged(d, base, idx)
    return got


def free_case(hip, oracle, scenes, ref, name):
    """a scene uploaded -> (its free rays, its frame's trace params, the reference's rows of them: test_rays_trace_gpu's, computed once a session)"""
    sc, p, _, _, _ = camera_rays(oracle, scenes, name)
    base, t = free_rays(oracle, scenes, name), trace_params(p)
    want = trace_wanted(ref, ("free", name, p.samples), sc, t, base)
    hip.update_scene(sc)
    return base, t, want


@pytest.mark.parametrize("name", ["dragon", "theater"])
def test_traces_on_the_full_grid_and_across_the_natural_slab(hip, oracle, scenes, trace_ref, name):
    """dragon: the lane walk, three transforms; theater: the lockstep walk, atlases, nine lights.  Two samples, 4 and 6 bounces: the scenes' frames'."""
    base, t, want = free_case(hip, oracle, scenes, trace_ref, name)
    C, S = cus(hip), t.samples
    for n in (P1(hip), S1):
        idx = index_map(n, len(base))
        got = traced(hip, base, idx, t, name)
        assert_tiled(got, want, idx, same_radiance_rows, "%s n %d" % (name, n))
        info = hip.last_trace()
        assert (info["n"], info["samples"], info["slab"], info["lockstep"]) == (n, S, SLAB, int(name == "theater")), info
        if n == S1:                                                                # the record's workgroups are the last slab's: 65 rays
            assert (info["slabs"], info["path_groups"], info["query_groups"]) == (2, path_groups(hip, 65, S), 1), info
        else:
            assert -(-(-(-n // 64) * S) // 4) > C * 8                             # more workgroups asked for than the cap gives
            assert (info["slabs"], info["path_groups"], info["query_groups"]) == (1, C * 8, C), info
        del got, idx


def test_a_trace_across_the_slot_bound_slab(hip, oracle, scenes, trace_ref):
    """nine samples: a slab is bound by its 2^24 slots, 1 864 128 rays, and a second one takes 65.  Cornell's shuffled camera rays (768 of them: the index map runs
    mod 768, to which 977 is prime too), one bounce."""
    sc, p, _, _, _ = camera_rays(oracle, scenes, "cornell")
    base, t = shuffled_camera_rays(oracle, scenes, "cornell"), trace_params(p)
    t.samples, t.max_reflections = 9, 1
    want = trace_ref.trace(sc, t, base)                                            # the one new computation on the CPU: these params' rows of the base rays
    assert 0.5 < (want[:, 5].view(np.int32) != -1).mean() and (want[:, 7] == 9).mean() > 0.5
    hip.update_scene(sc)
    idx = index_map(S9, len(base))
    got = traced(hip, base, idx, t, "cornell")
    assert_tiled(got, want, idx, same_radiance_rows, "cornell n %d" % S9)
    info = hip.last_trace()
    assert (info["n"], info["samples"], info["slab"], info["slabs"]) == (S9, 9, SLAB9, 2) and SLAB9 == 1864128, info
    assert (info["path_groups"], info["query_groups"]) == (path_groups(hip, 65, 9), 1), info


# ---- 3. the ordered trace -----------------------------------------------------------------------------------------------------------------------------------------------

def test_an_ordered_trace_across_the_natural_slab(hip, oracle, scenes, trace_ref):
    """a full slab's bounds, keys and sort (2^21 rays: 1024 sort workgroups, eight trips of k_hit_bounds) in front of its paths kernel, then a slab of 65"""
    base, t, want = free_case(hip, oracle, scenes, trace_ref, "dragon")
    T = hip.last_ray_order()["T"]
    idx = index_map(S1, len(base))
    got = traced(hip, base, idx, t, "dragon", order=capi.TRACE_ORDER_HITS)
    assert_tiled(got, want, idx, same_radiance_rows, "dragon, ordered, n %d" % S1)
    info, trace = hip.last_ray_order(), hip.last_trace()
    last = [base_of(row, len(base)) for row in range(SLAB, S1)]
    hits = int((want[last, 5].view(np.int32) != -1).sum())                         # every hit of these rays lies at a finite point
    assert 0 < hits < 65
    assert (info["ordered"], info["n"], info["groups"], info["passes"], info["live"]) == (1, S1, -(-65 // T), 4, hits), info
    assert (trace["slabs"], trace["slab"], trace["n"], trace["path_groups"]) == (2, SLAB, S1, path_groups(hip, 65, t.samples)), trace


# ---- 4. bounds and keys beyond one trip of k_hit_bounds ---------------------------------------------------------------------------------------------------------------------

def order_rows(n):
    """-> (ray rows, hit rows, live rows, extremes built: words of the bounds that only rows at or beyond BOUNDS_LANES decide).  Points uniform in [-1, 1)^3; about a
    tenth of the rows dead (entry -1), every seventh of those at +-5: outside every live point; the extremes +-3 of the axes sit
      n > BOUNDS_LANES + 5:  on six rows at or beyond BOUNDS_LANES, an axis and a side each: row BOUNDS_LANES itself (lane 0 of workgroup 0 on its second trip), the
                             last row, and four rows of other trips, workgroups and lanes;
      n = BOUNDS_LANES + 1:  on row BOUNDS_LANES alone, which as one point decides one side of every axis: three of the six words, the most one row can;
      n = BOUNDS_LANES:      no row is beyond the first trip: on rows of six different workgroups, the last row among them, so that the atomics still meet."""
    rng = np.random.default_rng(n)
    points = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    entries = np.full(n, 7, np.int32)
    dead = np.flatnonzero(rng.random(n) < 0.1)
    entries[dead] = -1
    points[dead[::7]] = np.where(rng.random((len(dead[::7]), 3)) < 0.5, np.float32(-5.0), np.float32(5.0))
    L = BOUNDS_LANES
    sides = [(0, 3.0), (1, -3.0), (2, 3.0), (0, -3.0), (1, 3.0), (2, -3.0)]
    if n >= L + 6:
        trips = n // L
        assert trips >= 7
        rows = [L, n - 1, 2 * L + 256 * 5 + 17, 3 * L + 256 * 300 + 100, 5 * L + 256 * 700 + 3, 6 * L + 256 * 1023 + 255]
    elif n > L:
        assert n == L + 1
        rows, sides = [L, L, L], sides[:3]
    else:
        assert n == L
        rows = [k * 256 + lane for k, lane in ((0, 0), (1, 63), (400, 64), (777, 129), (1022, 255), (1023, 255))]
        assert rows[-1] == n - 1 and len({r // 256 for r in rows}) == 6
    for row in set(rows):
        assert row < n
        entries[row] = 7
        if abs(points[row]).max() > 1.0:                                           # (a row that was dead and far: back inside)
            points[row] = np.float32(0.25)
    for row, (axis, value) in zip(rows, sides):
        points[row, axis] = np.float32(value)
    rays, hits = rows_at(points, entries)
    return rays, hits, int((entries != -1).sum()), len(sides)


@pytest.mark.parametrize("n", [BOUNDS_LANES, BOUNDS_LANES + 1, 1 << 21])
def test_bounds_and_keys_beyond_one_trip_of_the_bounds_grid(hip, keys_ref, n):
    """k_hit_bounds launches at most 1024 workgroups of 256 lanes and a lane strides on from there: from 262 145 rays on a lane takes a second ray, at 2^21 eight.
    The order only affects speed, so no radiance row shows wrong bounds; flx_debug_hit_keys does."""
    rays, hits, built, extremes = order_rows(n)
    want, want_bounds, live = keys_ref.keys(rays, hits)
    assert live == built and 0.85 * n < live < 0.95 * n
    if extremes == 6:
        assert np.array_equal(want_bounds.view(np.float32), np.array([-3, -3, -3, 3, 3, 3], np.float32))      # no dead row at +-5 moved them
    if n > BOUNDS_LANES:
        # the precondition that makes the case meaningful: the first trip's rows alone give other bounds, on every word a row beyond it can decide
        _, first_bounds, _ = keys_ref.keys(rays[:BOUNDS_LANES], hits[:BOUNDS_LANES])
        assert (first_bounds != want_bounds).sum() == extremes == (3 if n == BOUNDS_LANES + 1 else 6)
    torch.cuda.synchronize()
    with timed(hip, "flx_debug_hit_keys, %d rays" % n):
        keys, bounds = hip.hit_keys(rays, hits)
    assert np.array_equal(bounds.view(np.uint32), want_bounds), (n, bounds, want_bounds.view(np.float32))      # bits: -0 is not +0
    differ = np.flatnonzero(keys != want)
    assert differ.size == 0, (n, differ.size, differ[:8], keys[differ[:8]], want[differ[:8]])
    assert (keys != 0xFFFFFFFF).sum() == live and len(np.unique(keys)) > live // 8      # the cells tell the points apart


# ---- 5. surface rows and planes -----------------------------------------------------------------------------------------------------------------------------------------------

def test_surface_rows_across_the_natural_slab(hip, oracle, scenes, surface_ref):
    """theater: all three atlases.  The hit, the shading normal and the translucency / particle density / opacity plane: three planes, 100 MB"""
    sc, base, tw, want = surface_wanted(surface_ref, oracle, scenes, "theater")
    fields = BITS[HIT] | BITS[NORMAL] | BITS[TPO]
    want = planes_of(want, fields)
    hip.update_scene(sc)
    n = S1
    idx = index_map(n, len(base))
    d = tiled_rays(base, idx)
    out = poisoned(3 * n, 16)
    with timed(hip, "flx_rays_surface_device, theater, %d rays, fields %d" % (n, fields)):
        assert hip.surface_rays_device(d, fields, tw, out) is out
    got = rows_of(out, 3 * n, 16)
    assert rays_unchanged(d, base, idx)
    for p, plane in enumerate(("hit", "normal", "tpo")):                           # plane p starts at row p * n
        assert_tiled(got[p * n:(p + 1) * n], want[p], idx, exactly, "theater n %d plane %s" % (n, plane))
    info = hip.last_surface()
    assert (info["slabs"], info["slab"], info["n"], info["fields"], info["frame"], info["query_groups"]) == (2, SLAB, n, fields, 0, 1), info


def same_float_rows(got, want):
    return same_floats(got.view(np.float32), want.view(np.float32)).all(axis=1)


def test_planes_on_the_full_grid_and_across_the_natural_slab(hip, oracle, scenes, planes_ref):
    """dragon, its frame's two samples and four bounces; both kinds of plane at once"""
    sc, p, _, _, _ = camera_rays(oracle, scenes, "dragon")
    base, t = free_rays(oracle, scenes, "dragon"), trace_params(p)
    want, _ = planes_wanted(planes_ref, ("free", "dragon", p.samples), sc, t, base)
    want8 = quant(want)
    C = cus(hip)
    hip.update_scene(sc)
    for n in (P1(hip), S1):
        idx = index_map(n, len(base))
        d = tiled_rays(base, idx)
        out8, out32 = poisoned(5 * n, 4), poisoned(5 * n, 16)
        with timed(hip, "flx_rays_planes_device, dragon, %d rays, %d samples, %d bounces" % (n, t.samples, t.max_reflections)):
            got = hip.ray_planes_device(d, t, planes8=out8, planes32=out32)
        assert got[0] is out8 and got[1] is out32
        got8, got32 = rows_of(out8, 5 * n, 4), rows_of(out32, 5 * n, 16)
        assert rays_unchanged(d, base, idx)
        for k, plane in enumerate(PLANES):                                         # plane k starts at row k * n
            assert_tiled(got32[k * n:(k + 1) * n], want[k], idx, same_float_rows, "dragon n %d planes32 %s" % (n, plane))
            assert_tiled(got8[k * n:(k + 1) * n], want8[k].reshape(-1, 1), idx, exactly, "dragon n %d planes8 %s" % (n, plane))
        info = hip.last_ray_planes()
        assert (info["n"], info["samples"], info["slab"], info["lockstep"], info["block"]) == (n, t.samples, SLAB, 0, 64), info
        if n == S1:                                                                # the record's workgroups are the last slab's: 65 rays, two blocks
            assert (info["slabs"], info["groups"], info["query_groups"]) == (2, 1, 1), info
        else:
            assert -(-(-(-n // 64)) // 4) == C * 8 + 1                             # one workgroup more asked for than the cap gives
            assert (info["slabs"], info["groups"], info["query_groups"]) == (1, C * 8, C), info
        del got, got8, got32, out8, out32, d, idx


# ---- 6. the host twins ------------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_host_calls_equal_the_device_calls(hip, oracle, scenes, trace_ref):
    """cast_rays and trace_rays at C * 1024 + 1 rays: the staging buffers at a size of their own, the rows the device calls'"""
    n = Q1(hip)
    sc, rays7, want_suv, want = scene_walks(oracle, 600, 3)
    base = pack_rays(rays7)
    idx = index_map(n, len(base))
    host_rays = np.ascontiguousarray(base[idx.cpu().numpy()])
    hip.update_scene(sc)
    got, _ = cast(hip, base, idx, 7, "600 entries, 3 transforms")
    assert_tiled(got, expected_words(want_suv, want, 7), idx, same_hit_rows, "cast, n %d" % n)
    with timed(hip, "flx_rays_cast, %d rays, what 7" % n):
        host = hip.cast_rays(host_rays, 7)
    assert np.array_equal(words_of(host), got.cpu().numpy().view(np.uint32))
    assert hip.last_query()["groups"] == cus(hip)
    del got
    base, t, want = free_case(hip, oracle, scenes, trace_ref, "dragon")
    host_rays = np.ascontiguousarray(base[idx.cpu().numpy()])
    got = traced(hip, base, idx, t, "dragon")
    assert_tiled(got, want, idx, same_radiance_rows, "trace, n %d" % n)
    before = hip.last_trace()
    with timed(hip, "flx_rays_trace, dragon, %d rays" % n):
        host = hip.trace_rays(host_rays, t)
    assert np.array_equal(words_of(host), got.cpu().numpy().view(np.uint32))
    assert hip.last_trace() == before and before["query_groups"] == cus(hip)      # the same slabs and workgroups
