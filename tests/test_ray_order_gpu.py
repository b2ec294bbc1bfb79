"""Traced ray batches in first-hit order on the GPU (flx_rays_trace_ordered[_device], flx_debug_sort_keys, flx_debug_hit_keys: csrc/flx_rays_order.hip,
csrc/flx_rays_trace.hip): the sort alone against numpy's stable argsort, bounds and keys against the CPU reference that compiles include/flx_ray_key.h
(tests/ray_order_ref), and the ordered batch against the unordered one — all eight words of every row, no row left out."""
import numpy as np
import pytest
import torch

from flexlight_hip import capi
from ray_order_util import DEAD, reference as key_reference, tables
from rays_trace_util import FRAMES, assert_rows, camera_rays, free_rays, reference as trace_reference, trace_params, words_of

pytestmark = pytest.mark.gpu

BAD_BIT = r"failed \(1\): flx_rays_trace_ordered: order has a bit beyond FLX_TRACE_ORDER_HITS"


@pytest.fixture(scope="module")
def keys_ref(tmp_path_factory):
    return key_reference(tmp_path_factory)


def sort_T(hip):
    T = hip.last_ray_order()["T"]
    assert T >= 64 and T % 64 == 0
    return T


# ---- 1. the sort alone -----------------------------------------------------------------------------------------------------------------------------------------------

def key_set(kind, n, rng):
    if kind == "equal":
        return np.full(n, 0x12345678, np.uint32)
    if kind == "ascending":
        return np.arange(n, dtype=np.uint32) * np.uint32(977)
    if kind == "descending":
        return (np.uint32(0xFFFFFFFF) - np.arange(n, dtype=np.uint32) * np.uint32(977)).astype(np.uint32)
    if kind == "random":
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if kind.startswith("byte "):
        byte = int(kind[5:])
        fixed = np.uint32(0xA55A3CC3) & ~np.uint32(0xFF << (8 * byte))
        return (rng.integers(0, 256, n, dtype=np.uint64).astype(np.uint32) << np.uint32(8 * byte)) | fixed
    if kind == "alternating":
        return np.where(np.arange(n) % 2 == 0, np.uint32(0), np.uint32(DEAD)).astype(np.uint32)
    if kind == "mostly dead":
        keys = rng.integers(0, 1 << 30, n, dtype=np.uint64).astype(np.uint32)
        keys[rng.random(n) < 0.9] = DEAD
        return keys
    raise ValueError(kind)


KEY_SETS = ["equal", "ascending", "descending", "random", "byte 0", "byte 1", "byte 2", "byte 3", "alternating", "mostly dead"]


@pytest.mark.parametrize("kind", KEY_SETS)
def test_the_sort_alone_equals_numpys_stable_argsort(hip, kind):
    T = sort_T(hip)
    rng = np.random.default_rng(len(kind) * 131 + sum(kind.encode()))
    for n in (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 3 * T + 17):
        keys = key_set(kind, n, rng)
        got = hip.sort_keys(keys)
        want = np.argsort(keys, kind="stable").astype(np.uint32)
        assert np.array_equal(got, want), (kind, n, np.flatnonzero(got != want)[:8])
        if kind == "equal":
            assert np.array_equal(got, np.arange(n, dtype=np.uint32))          # equal keys keep the caller's order


@pytest.mark.parametrize("n", ["17 T + 5", "2^21"])
def test_the_sort_where_the_scan_takes_more_than_one_tile(hip, n):
    """the count table of 17 workgroups is 4352 words, one more tile of 4096 than one; the largest slab's is 2^18 words, 64 tiles: many equal keys, so that a place
    lost or a carry dropped between two tiles shows as a wrong or unstable order"""
    T = sort_T(hip)
    n = 17 * T + 5 if n == "17 T + 5" else 1 << 21
    rng = np.random.default_rng(n)
    keys = (rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) & np.uint32(0x3F0F0703))
    keys[rng.random(n) < 0.25] = DEAD
    got = hip.sort_keys(keys)
    want = np.argsort(keys, kind="stable").astype(np.uint32)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def test_the_sort_refuses_what_it_cannot_take(hip):
    for keys in (np.zeros(0, np.uint32), np.zeros((1 << 21) + 1, np.uint32)):
        with pytest.raises(capi.FlexLightHipError, match=r"failed \(1\): flx_debug_sort_keys: n is 0 or above 2\^21"):
            hip.sort_keys(keys)
    with pytest.raises(capi.FlexLightHipError, match=r"failed \(1\): flx_debug_hit_keys: n is 0 or above 2\^21"):
        hip.hit_keys(np.zeros((0, 8), np.float32), np.zeros((0, 32), np.uint8))


# ---- 2. bounds and keys ----------------------------------------------------------------------------------------------------------------------------------------------

def assert_keys(hip, keys_ref, rays, hits, what):
    keys, bounds = hip.hit_keys(rays, hits)
    want, want_bounds, live = keys_ref.keys(rays, hits)
    assert np.array_equal(keys, want), (what, np.flatnonzero(keys != want)[:8])
    if live:
        assert np.array_equal(bounds.view(np.uint32), want_bounds), (what, bounds, want_bounds.view(np.float32))      # bits: -0 is not +0
    else:
        assert (keys == DEAD).all()
    return keys, live


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_bounds_and_keys_of_a_scenes_free_rays_equal_the_reference(hip, oracle, scenes, keys_ref, name):
    sc, _, _, _, _ = camera_rays(oracle, scenes, name)
    rays = free_rays(oracle, scenes, name)
    hip.update_scene(sc)
    hits = hip.cast_rays(rays, capi.RAYS_CLOSEST)
    keys, live = assert_keys(hip, keys_ref, rays, hits, name)
    assert live == (capi.unpack_hits(hits)["entry"] != -1).sum() and 0.3 * len(rays) < live < len(rays)          # hits and misses; every hit lies at a finite point
    assert len(np.unique(keys)) > live // 4                                                         # the cells tell the hit points apart


@pytest.mark.parametrize("name", sorted(tables()))
def test_bounds_and_keys_of_the_hand_made_table_equal_the_reference(hip, keys_ref, name):
    rays, hits = tables()[name]
    assert_keys(hip, keys_ref, rays, hits, name)


# ---- 3. the ordered batch equals the unordered batch --------------------------------------------------------------------------------------------------------------------

def traced(hip, rays, t, order):
    """rays (numpy [n, 8]) through the device call into a poisoned buffer with eight rows behind the last -> words [n, 8]; order None: flx_rays_trace_device"""
    d = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
    keep = d.clone()
    n = d.shape[0]
    out = torch.full((n + 8, 32), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if order is None:
        assert hip.trace_rays_device(d, t, out) is out
    else:
        assert hip.trace_rays_ordered_device(d, t, out, order=order) is out
    hip.sync()
    got = words_of(out)
    assert (got[n:] == 0xA5A5A5A5).all() and torch.equal(d, keep)              # nothing beyond row n - 1 is written; the rays are read only
    return got[:n]


def shuffled_camera_rays(oracle, scenes, name):
    _, _, rays, _, _ = camera_rays(oracle, scenes, name)
    return np.ascontiguousarray(rays[np.random.default_rng(7).permutation(len(rays))])


def missing_rays(n=200):
    """rays that start far outside every scene and point away from it"""
    rng = np.random.default_rng(3)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = 1.0e4 + rng.uniform(0, 10, (n, 3))
    rays[:, 4:7] = rng.uniform(0.1, 1.0, (n, 3))
    rays[:, 3], rays[:, 7] = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    return rays


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_the_ordered_batch_equals_the_unordered_batch(hip, oracle, scenes, name):
    sc, p, _, _, _ = camera_rays(oracle, scenes, name)
    free = free_rays(oracle, scenes, name)
    sets = {"shuffled camera": shuffled_camera_rays(oracle, scenes, name), "free": free, "misses": missing_rays(), "one": free[1100:1101], "65": free[1050:1115]}
    T = sort_T(hip)
    hip.update_scene(sc)
    try:
        for samples in (1, 2):
            t = trace_params(p)
            t.samples = samples
            for what, rays in sets.items():
                n = len(rays)
                want = traced(hip, rays, t, None)
                assert hip.last_ray_order()["ordered"] == 0
                hit = want[:, 5].view(np.int32) != -1
                assert (what == "misses" and not hit.any()) or (what != "misses" and hit.any())
                for slab in (64, 100, 0):
                    for groups in (1, 0):
                        hip.set_trace_slab(slab)
                        hip.set_query_groups(groups)
                        got = traced(hip, rays, t, capi.TRACE_ORDER_HITS)
                        assert_rows(got, want, "%s %s S %d slab %d groups %d" % (name, what, samples, slab, groups))
                        last = n - (n - 1) // slab * slab if slab else n                      # the rays of the last slab
                        info, trace = hip.last_ray_order(), hip.last_trace()
                        assert (info["ordered"], info["T"], info["groups"], info["passes"], info["n"]) == (1, T, -(-last // T), 4, n)
                        assert info["live"] == hit[n - last:].sum()                           # every hit of these rays lies at a finite point
                        assert (trace["slabs"], trace["n"], trace["samples"]) == (-(-n // slab) if slab else 1, n, samples)
    finally:
        hip.set_query_groups(0)
        hip.set_trace_slab(0)


def test_the_ordered_batch_equals_the_cpu_reference(hip, oracle, scenes, tmp_path_factory):
    ref = trace_reference(tmp_path_factory)
    sc, p, _, _, _ = camera_rays(oracle, scenes, "cornell")
    rays, t = shuffled_camera_rays(oracle, scenes, "cornell"), trace_params(p)
    hip.update_scene(sc)
    want = ref.trace(sc, t, rays)
    assert 0.5 < (want[:, 5].view(np.int32) != -1).mean() and (want[:, 7] > t.samples).mean() > 0.1
    assert_rows(traced(hip, rays, t, capi.TRACE_ORDER_HITS), want, "cornell, shuffled camera rays")


# ---- 4. the host call, order 0 ------------------------------------------------------------------------------------------------------------------------------------------

def test_the_host_call_equals_the_device_call_and_order_0_is_the_unordered_call(hip, oracle, scenes):
    sc, p, _, _, _ = camera_rays(oracle, scenes, "dragon")
    rays, t = free_rays(oracle, scenes, "dragon"), trace_params(p)
    hip.update_scene(sc)
    plain = words_of(hip.trace_rays(rays, t))
    before = hip.last_trace()
    device = traced(hip, rays, t, capi.TRACE_ORDER_HITS)
    assert hip.last_ray_order()["ordered"] == 1
    host = words_of(hip.trace_rays_ordered(rays, t))
    assert np.array_equal(host, device)
    assert_rows(host, plain, "the host call")
    assert hip.last_trace() == before                                                       # the same slabs and workgroups
    zero = words_of(hip.trace_rays_ordered(rays, t, order=0))
    assert np.array_equal(zero, plain)
    info = hip.last_ray_order()
    assert (info["ordered"], info["groups"], info["passes"], info["n"], info["live"]) == (0, 0, 0, len(rays), 0)
    assert np.array_equal(traced(hip, rays, t, 0), plain) and hip.last_trace() == before
    assert hip.trace_rays_ordered(np.zeros((0, 8), np.float32), t).shape == (0, 32)          # n == 0: FLX_OK, nothing enqueued
    hip.trace_rays_ordered_device((0, 0), t, 0)
    assert hip.last_ray_order() == info


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------------------------------------

def test_refusals(hip, oracle, scenes):
    sc, p, _, _, _ = camera_rays(oracle, scenes, "theater")
    rays_host, t = free_rays(oracle, scenes, "theater")[:256], trace_params(p)
    with capi.Context(0) as fresh:
        for call in (lambda: fresh.trace_rays_ordered(rays_host, t), lambda: fresh.trace_rays_ordered_device((0, 0), t, 0, order=2)):
            with pytest.raises(capi.FlexLightHipError, match=r"failed \(3\): flx_rays_trace_ordered: no scene and transforms uploaded"):      # FLX_ERR_NO_SCENE
                call()
        assert fresh.last_ray_order()["ordered"] == 0 and fresh.last_ray_order()["n"] == 0
    hip.update_scene(sc)
    rays = torch.from_numpy(rays_host).cuda()
    out = torch.full((256, 32), 0xA5, dtype=torch.uint8, device="cuda")
    host = np.zeros((256, 8), np.float32)
    torch.cuda.synchronize()
    plain = hip.trace_rays_device(rays, t)
    hip.trace_rays_ordered_device(rays, t, out)
    hip.sync()
    want = words_of(plain)
    assert_rows(words_of(out), want, "before the refusals")
    before, before_trace = hip.last_ray_order(), hip.last_trace()
    assert before["ordered"] == 1
    out.fill_(0xA5)
    torch.cuda.synchronize()
    bad = trace_params(p)
    bad.samples = 0
    invalid = r"failed \(1\): "
    refused = [
        (lambda: hip.trace_rays_ordered_device(rays, t, out, order=2), BAD_BIT),
        (lambda: hip.trace_rays_ordered_device(rays, t, out, order=3), BAD_BIT),
        (lambda: hip.trace_rays_ordered_device(rays, t, out, order=0x80000000), BAD_BIT),
        (lambda: hip.trace_rays_ordered(rays_host, t, order=4), BAD_BIT),
        (lambda: hip.trace_rays_ordered_device((0, 0), t, 0, order=2), BAD_BIT),                                                        # for n == 0 too
        (lambda: hip.trace_rays_ordered_device(rays, None, out), invalid + "flx_rays_trace_ordered: params is NULL"),
        (lambda: hip.trace_rays_ordered(rays_host, bad, order=2), invalid + "flx_rays_trace_ordered: samples is less than 1"),           # the params are said first
        (lambda: hip.trace_rays_ordered_device((host.ctypes.data, 256), t, out), invalid + "flx_rays_trace_ordered_device: the rays are not n rows in memory of the context's device"),
        (lambda: hip.trace_rays_ordered_device(rays, t, out.data_ptr() + 8), invalid + "flx_rays_trace_ordered_device: the radiance is not n rows in memory of the context's device, 16-byte aligned"),
        (lambda: hip.trace_rays_ordered_device((0, 4), t, out), invalid + "flx_rays_trace_ordered_device: an array is NULL"),
        (lambda: hip.trace_rays_ordered_device(rays, t, rays.data_ptr()), invalid + "flx_rays_trace_ordered_device: the rays and the radiance overlap"),
    ]
    for call, message in refused:
        with pytest.raises(capi.FlexLightHipError, match=message):
            call()
        assert hip.last_ray_order() == before and hip.last_trace() == before_trace, message      # a refused call leaves the record as it was
    torch.cuda.synchronize()
    assert (out == 0xA5).all()
    hip.trace_rays_device(rays, t, out)                                                        # an unordered batch: the record says so
    after = hip.last_ray_order()
    assert (after["ordered"], after["n"]) == (0, 256)
    got = hip.trace_rays_ordered_device(rays, t, out)                                          # after the refusals the next ordered batch is right
    hip.sync()
    assert_rows(words_of(got), want, "after the refusals")


# ---- 6. a frame in flight -----------------------------------------------------------------------------------------------------------------------------------------------

def test_an_ordered_batch_between_a_frames_begin_and_its_end(hip, oracle, scenes):
    sc, p, _, _, _ = camera_rays(oracle, scenes, "dragon")
    rays, t = free_rays(oracle, scenes, "dragon"), trace_params(p)
    hip.update_scene(sc)
    q = sc.frame_params(width=96, height=54, samples=2, max_reflections=4, use_filter=0)
    alone = np.asarray(hip.render(q)[0]).copy()
    want = words_of(hip.trace_rays(rays, t))
    d = torch.from_numpy(rays).cuda()
    torch.cuda.synchronize()
    hip.frame_begin(q)
    assert hip.frames_in_flight() == 1
    out = hip.trace_rays_ordered_device(d, t)
    frame = np.asarray(hip.frame_end()[0])
    hip.sync()
    assert_rows(words_of(out), want, "between a frame's begin and its end")
    assert hip.last_ray_order()["ordered"] == 1
    frame = frame.reshape(alone.shape)
    assert ((frame.view(np.uint32) == alone.view(np.uint32)) | (np.isnan(frame) & np.isnan(alone))).all()      # the frame is the frame rendered alone
