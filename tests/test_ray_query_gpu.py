"""Ray queries on the GPU (flx_rays_cast, flx_rays_cast_device: csrc/flx_query.hip) against the C oracle's rayTracer and shadowTest, bit for bit: (s, u, v) as bit
patterns where the oracle hits, every other word of a hit row as a number.  Scenes and rays are test_walk_lds_gpu's (synth_scene.make_sized, make_rays: 2160
rows); the oracle's walks are made once per scene (ray_query_util.scene_walks)."""
import numpy as np
import pytest
import torch

from flexlight_hip import capi
from intersect_edges_util import literal_walks, packed_scenes, same_walks
from ray_query_util import COUNT, EVERY_WHAT, debug_walk_columns, expected_words, pack_rays, same_rows, scene_walks, words_of
from scene_update_util import reflatten_by_rule, with_geometry
from test_walk_lds_gpu import oracle_walks

pytestmark = pytest.mark.gpu

LANES = 1024          # lanes of a workgroup of the query kernel
WAVES = LANES // 64


def assert_rows(got, want, what, nan_equal=False):
    same = same_rows(got, want, nan_equal)
    bad = np.flatnonzero(~same)
    assert bad.size == 0, "what %d: %d of %d rows differ, first %d: got %s want %s" % (what, bad.size, len(same), bad[0], ["%08x" % x for x in got[bad[0]]], ["%08x" % x for x in want[bad[0]]])


# ---- every `what`, both ray paths, the tree wholly and partly in LDS ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entries,n_transforms", [(600, 1), (600, 3), (600, 4), (600, 6), (5000, 1), (5000, 4)])
def test_every_what_equals_the_oracle(hip, oracle, entries, n_transforms):
    sc, rays7, want_suv, want = scene_walks(oracle, entries, n_transforms)
    rays = pack_rays(rays7)
    hip.update_scene(sc)
    assert hip.last_query() == dict.fromkeys(("lds_count", "pre", "groups", "waves", "n", "what", "chunk", "draws"), 0)      # nothing launched since the upload
    got = {}
    for what in EVERY_WHAT:
        got[what] = words_of(hip.cast_rays(rays, what))
        assert_rows(got[what], expected_words(want_suv, want, what), what)
        info, lds = hip.last_query(), hip.last_walk_lds()
        assert (info["n"], info["what"], info["chunk"]) == (2160, what, capi.QUERY_CHUNK)
        assert info["pre"] == int(n_transforms <= 3)              # pre-transformed rays where they fit beside a useful tree top, on the fly beyond: both paths run across the T values
        if entries == 600:
            assert info["lds_count"] == lds["walk_entries"] == 601      # the whole tree is walked from LDS
        else:
            assert 0 < info["lds_count"] < lds["walk_hot"] == 4097
        assert info["groups"] == 3 and 1 <= info["waves"] <= 3 * WAVES and info["draws"] == -(-2160 // capi.QUERY_CHUNK) + 3 * WAVES      # every wave ends on one draw past the last chunk
    for what in (1, 2, 3):                                        # the words an uncounted run writes are the same in the counted run
        assert np.array_equal(got[what][:, 0:6], got[what | COUNT][:, 0:6])
        assert (got[what][:, 6:8] == 0).all()
    assert got[7][:, 6].max() > 64 and got[7][:, 7].max() > 16     # long walks among them


def test_both_ray_paths_ran(hip, oracle):
    pre = set()
    for n_transforms in (3, 4):
        sc, rays7, want_suv, want = scene_walks(oracle, 600, n_transforms)
        hip.update_scene(sc)
        assert_rows(words_of(hip.cast_rays(pack_rays(rays7[:64]), 7)), expected_words(want_suv[:64], want[:64], 7), 7)
        pre.add(hip.last_query()["pre"])
    assert pre == {0, 1}


# ---- sizes and refills --------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_transforms", [3, 4])
def test_sizes_and_refills(hip, oracle, n_transforms):
    sc, rays7, want_suv, want = scene_walks(oracle, 600, n_transforms)
    chunk = capi.QUERY_CHUNK
    hip.update_scene(sc)
    all_rays = torch.from_numpy(pack_rays(rays7)).cuda()
    try:
        for groups in (0, 1):
            hip.set_query_groups(groups)
            for n in (1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2160):
                rays = all_rays[:n].clone()
                hits = torch.full((n + 8, 32), 0xA5, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                out = hip.cast_rays_device(rays, hits, 7)
                assert out is hits
                hip.sync()
                got = words_of(hits)
                assert_rows(got[:n], expected_words(want_suv[:n], want[:n], 7), 7)
                assert (got[n:] == 0xA5A5A5A5).all(), (groups, n)                   # nothing beyond row n - 1 is written
                assert torch.equal(rays, all_rays[:n])                              # the rays are read only
                info = hip.last_query()
                launched = groups or min(-(-n // LANES), hip.device_info()[1])
                assert (info["n"], info["groups"], info["chunk"]) == (n, launched, chunk), info
                assert 1 <= info["waves"] <= min(launched * WAVES, -(-n // chunk)) and info["draws"] == -(-n // chunk) + launched * WAVES, info
                if groups == 1 and n == 2160:
                    assert info["groups"] * LANES < n                               # fewer lanes than rays: lanes took a second and a third ray
            before = hip.last_query()
            empty = torch.zeros((0, 8), dtype=torch.float32, device="cuda")
            hip.cast_rays_device(empty, what=7)                                     # n = 0: no error, nothing enqueued
            hip.cast_rays_device((0, 0), 0, 3)
            assert hip.cast_rays(np.zeros((0, 8), np.float32), 3).shape == (0, 32)
            assert hip.last_query() == before
    finally:
        hip.set_query_groups(0)


# ---- edge rays -----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_transforms", [3, 4])
def test_degenerate_rays_equal_the_oracle(hip, oracle, n_transforms):
    sc, rays7, _, want_all = scene_walks(oracle, 600, n_transforms)
    base = rays7[np.flatnonzero((want_all[:, 4] != -1) & (want_all[:, 6] == 1))[0]].copy()      # a ray that hits and is shadowed within its l
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    rows, names = [], []

    def add(name, **kw):
        r = base.copy()
        for k, v in kw.items():
            r[{"ox": 0, "oy": 1, "oz": 2, "dx": 3, "dy": 4, "dz": 5, "l": 6}[k]] = v
        rows.append(r)
        names.append(name)

    add("as it is")
    for k in ("dx", "dy", "dz"):
        add("NaN " + k, **{k: nan})
    add("zero direction", dx=0, dy=0, dz=0)
    for k in ("ox", "oy", "oz"):
        add("+inf " + k, **{k: inf})
        add("-inf " + k, **{k: -inf})
    for k in ("dx", "dy", "dz"):
        for sign in (1.0, -1.0):
            add("axis %s%s" % ("+" if sign > 0 else "-", k), **dict({"dx": 0, "dy": 0, "dz": 0}, **{k: sign}))
    add("axis +dz with -0", dx=-0.0, dy=-0.0, dz=1.0)
    for name, l in (("l 0", 0.0), ("l negative", -3.0), ("l +inf", inf), ("l NaN", nan), ("l -inf", -inf), ("l tiny", 1e-30)):
        add(name, l=l)
    rays7e = np.array(rows, np.float32)
    want_suv, want = oracle_walks(oracle, sc, rays7e)
    assert want[0, 4] != -1 and want[0, 6] == 1 and (want[-6:, 4] == want[0, 4]).all()      # l does not touch the closest hit
    assert want[names.index("l 0"), 6] == 0 and want[names.index("l +inf"), 6] == 1
    hip.update_scene(sc)
    for what in (7, 3, 5, 6):
        got, exp = words_of(hip.cast_rays(pack_rays(rays7e), what)), expected_words(want_suv, want, what)
        # every word equals the oracle's; the one allowance: where the ORACLE's own s, u or v is a NaN the device's must be a NaN too, of any sign and payload (an invalid
        # operation makes another NaN on the CPU than on the GPU: intersect_edges_util.same_walks) - a NaN against a number, or a number against a NaN, differs
        same = same_rows(got, exp, nan_equal=True)
        assert same.all(), (what, [(names[k], ["%08x" % x for x in got[k]], ["%08x" % x for x in exp[k]]) for k in np.flatnonzero(~same)])


# ---- the adversarial table -----------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kat():
    import gzip
    import json
    import os
    return json.load(gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "intersect_edge_kat.json.gz"), "rt"))


@pytest.mark.parametrize("two_spaces", [False, True], ids=["one_space", "two_spaces"])
def test_edge_rows_through_the_query(hip, kat, two_spaces):
    """tests/test_intersect_edges_gpu.py's packed scenes through flx_rays_cast with both walks counted, under both forms of the box test"""
    failures, scenes = [], 0
    try:
        for name, sc, rays, classes in packed_scenes(kat, two_spaces):
            want = literal_walks(sc, rays)
            hip.update_scene(sc)
            for form in (0, 1):
                hip.set_box_test(form)
                got = debug_walk_columns(hip.cast_rays(pack_rays(rays), 7))
                for k in np.flatnonzero(~same_walks(got, want)):
                    failures.append("%s / box test %d / %s: ray %d want %s got %s" % (name, form, classes[k], k, want[k].tolist(), got[k, 0:3].view(np.uint32).tolist() + got[k, 3:8].astype(np.int64).tolist()))
            scenes += 1
    finally:
        hip.set_box_test(-1)
    assert scenes >= 150
    assert not failures, "%d rays differ from the literal walks\n%s" % (len(failures), "\n".join(failures[:30]))


# ---- agreement with the hook ---------------------------------------------------------------------------------------------------------------------------------------

def test_what_7_equals_flx_debug_walk(hip, oracle):
    sc, rays7, _, _ = scene_walks(oracle, 600, 3)
    hip.update_scene(sc)
    hook = hip.debug_walk(0, rays7)
    got = debug_walk_columns(hip.cast_rays(pack_rays(rays7), 7))
    assert np.array_equal(got.view(np.uint32), hook.view(np.uint32))


# ---- ordering ------------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_query_sees_the_rows_updated_before_it(hip, oracle):
    sc, rays7, want_suv, want = scene_walks(oracle, 600, 3)
    k = int(np.flatnonzero(want[:, 4] != -1)[0])
    entry = int(want[k, 4])
    near = np.flatnonzero(want[:, 4] == entry)                       # every ray whose closest hit is that triangle, and some more
    pick = np.unique(np.concatenate([near, np.arange(64)]))
    rays = pack_rays(rays7[pick])
    hip.update_scene(sc)
    assert_rows(words_of(hip.cast_rays(rays, 7)), expected_words(want_suv[pick], want[pick], 7), 7)
    g = sc.arrays["geometry"].reshape(-1, 12).copy()
    assert g[entry, 10] == 2
    g[entry, [1, 4, 7]] += np.float32(500.0)                         # the triangle leaves, out of every ray's way
    moved = with_geometry(sc, reflatten_by_rule(g))
    hip.update_scene_rows(entry, g[entry:entry + 1])
    new_suv, new = oracle_walks(oracle, moved, rays7[pick])
    assert (new[np.isin(pick, near), 4] != entry).all() and not np.array_equal(new[:, 4], want[pick, 4])
    assert_rows(words_of(hip.cast_rays(rays, 7)), expected_words(new_suv, new, 7), 7)


def test_a_query_between_two_frames_of_the_loop(hip, oracle):
    sc, rays7, want_suv, want = scene_walks(oracle, 600, 3)
    hip.update_scene(sc)
    params = [sc.frame_params(use_filter=0), sc.frame_params(use_filter=0)]
    params[1].random_seed = params[0].random_seed + 1.0
    alone = [hip.render(p)[0] for p in params]
    rays = torch.from_numpy(pack_rays(rays7)).cuda()
    torch.cuda.synchronize()
    for p in params:
        hip.frame_begin(p)
    assert hip.frames_in_flight() == 2
    hits = hip.cast_rays_device(rays, what=7)
    frames = [hip.frame_end()[0] for _ in params]
    hip.sync()
    assert_rows(words_of(hits), expected_words(want_suv, want, 7), 7)
    for got, ref in zip(frames, alone):
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert not np.array_equal(frames[0], frames[1])


def test_a_query_waits_for_the_stream_that_writes_its_rays(hip, oracle):
    sc, rays7, want_suv, want = scene_walks(oracle, 600, 3)
    hip.update_scene(sc)
    source = torch.from_numpy(pack_rays(rays7)).cuda()
    rays = torch.zeros_like(source)
    busy = torch.ones((2048, 2048), device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):
            busy = busy @ busy * 1e-4                               # work in front of the write, so that the rays are not there when the call returns
        rays.copy_(source)
        hits = hip.cast_rays_device(rays, what=7, stream=side)
    hip.sync()
    assert_rows(words_of(hits), expected_words(want_suv, want, 7), 7)
    side.synchronize()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------------

def test_refusals(hip, oracle):
    sc, rays7, want_suv, want = scene_walks(oracle, 600, 3)
    rays_host = pack_rays(rays7[:256])
    with capi.Context(0) as fresh:
        for call in (lambda: fresh.cast_rays(rays_host, 3), lambda: fresh.cast_rays_device(torch.zeros((4, 8), device="cuda"), what=3)):
            with pytest.raises(capi.FlexLightHipError, match=r"failed \(3\): flx_rays_cast: no scene and transforms uploaded"):      # FLX_ERR_NO_SCENE
                call()
        assert fresh.last_query()["groups"] == 0
    hip.update_scene(sc)
    rays = torch.from_numpy(rays_host).cuda()
    hits = torch.full((256, 32), 0xA5, dtype=torch.uint8, device="cuda")
    both = torch.zeros((512, 8), dtype=torch.float32, device="cuda")
    host = np.zeros((256, 8), np.float32)
    torch.cuda.synchronize()
    hip.cast_rays_device(rays, hits, 1)
    hip.sync()
    before = hip.last_query()
    hits.fill_(0xA5)
    torch.cuda.synchronize()
    invalid = r"failed \(1\): "
    refused = [
        (lambda: hip.cast_rays_device(rays, hits, 0), "what asks for neither"),
        (lambda: hip.cast_rays_device(rays, hits, 4), "what asks for neither"),
        (lambda: hip.cast_rays_device(rays, hits, 8 | 3), "what has a bit beyond"),
        (lambda: hip.cast_rays(rays_host, 16), "what has a bit beyond"),
        (lambda: hip.cast_rays(rays_host, 0), "what asks for neither"),
        (lambda: hip.cast_rays_device((host.ctypes.data, 256), hits, 3), "the rays are not n rows in memory of the context's device"),            # host memory
        (lambda: hip.cast_rays_device(rays, host.ctypes.data, 3), "the hits are not n rows in memory of the context's device"),
        (lambda: hip.cast_rays_device((rays.data_ptr() + 4, 255), hits, 3), "the rays are not n rows in memory of the context's device, 16-byte aligned"),
        (lambda: hip.cast_rays_device(rays, hits.data_ptr() + 8, 3), "the hits are not n rows in memory of the context's device, 16-byte aligned"),
        (lambda: hip.cast_rays_device((rays.data_ptr(), 1 << 28), hits.data_ptr(), 3), "the rays are not n rows"),                                          # 8 GB: the allocation ends first
        (lambda: hip.cast_rays_device((0, 4), hits, 3), "an array is NULL"),
        (lambda: hip.cast_rays_device(both, both.data_ptr(), 3), "the rays and the hits overlap"),                                              # the same array
        (lambda: hip.cast_rays_device((both.data_ptr(), 256), both.data_ptr() + 255 * 32, 3), "the rays and the hits overlap"),                 # the hits begin in the last ray
        (lambda: hip.cast_rays_device((both.data_ptr() + 32, 256), both.data_ptr(), 3), "the rays and the hits overlap"),
    ]
    for call, message in refused:
        with pytest.raises(capi.FlexLightHipError, match=invalid + ".*" + message):
            call()
        assert hip.last_query() == before, message                  # nothing was enqueued
    torch.cuda.synchronize()
    assert (hits == 0xA5).all()
    hip.cast_rays_device((both.data_ptr(), 256), both.data_ptr() + 256 * 32, 3)      # side by side in one allocation: no overlap
    out = hip.cast_rays_device(rays, hits, 7)                       # after the refusals the next query is right
    hip.sync()
    assert_rows(words_of(out), expected_words(want_suv[:256], want[:256], 7), 7)
