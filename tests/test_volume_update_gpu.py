"""Volume updates on the device (include/flexlight_hip_debug.h, "volume updates"): k_volume_positions_list's rows and k_volume_blend's rows and states are the CPU
reference's bits (tests/volume_update_ref, the same include/flx_volume_update.h) for every grid, map size, list, list length and hysteresis at which the kernels can
go wrong, into poisoned outputs; the fused call is the three calls it is made of, bit for bit, whatever the chunk; an update with h = 0 onto zeroed rows is the bake;
two updates are the reference's blend of two bakes; a lookup reads updated rows as it reads any; an update between two frames of the loop leaves them alone; every
refusal says its words and leaves the outputs as they were.

A SKIPPED entry's state word is written (3): the state array is no part of the volume.  What keeps its poison is every row of the volume that the list does not name,
the words behind the last state, and a state array that was not given."""
import numpy as np
import pytest
import torch

from flexlight_hip import capi
from probe_util import cornell_probes
from volume_update_util import (BLENDED, FLAVOUR_STATE, GRIDS, HYSTERESES, KEPT, MAP_SIZES, POISON, SKIPPED, SPARE, TAKEN, assert_same_words, back, device_words, entries_of, grid_of,
                                lists_of, map_of, reference, synthetic_case, update_of)

pytestmark = pytest.mark.gpu

NS = (0, 1, 3, 4, 5, 8, 9)             # no entry; a wave; a workgroup less one, a workgroup, a workgroup and a wave; two workgroups; two and a wave
FACES = (1, 2, 4)                      # the face size of the bakes over grid k


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return reference(tmp_path_factory)


def poisoned_volume(probes, bins, entries, sh, maps):
    """the resident rows of the probes a list names among rows of poison -> (sh float32 [probes, 36], maps float32 [probes * bins, 4] or None, listed bool [probes])"""
    listed = np.zeros(probes, bool)
    listed[[e for e in entries if e < probes]] = True
    host_sh = np.full((probes, 36), POISON, np.uint32).view(np.float32)
    host_sh[listed] = sh[listed]
    host_maps = None
    if bins:
        host_maps = np.full((probes, bins, 4), POISON, np.uint32).view(np.float32)
        host_maps[listed] = maps.reshape(probes, bins, 4)[listed]
        host_maps = host_maps.reshape(-1, 4)
    return host_sh, host_maps, listed


@pytest.mark.parametrize("count", GRIDS)
def test_positions_of_a_list_are_the_references_bits(hip, ref, count):
    grid = grid_of(count)
    for n_list in NS:
        for name, indices, (first, stride), n in lists_of(grid.probes, n_list, seed=n_list):
            update = update_of(0.5, first, stride)
            want = ref.positions(grid, update, indices, n)
            out = device_words(np.full((n, 4), POISON, np.uint32), SPARE * 4)
            d_indices = device_words(indices, 0) if indices is not None and n else None
            torch.cuda.synchronize()
            assert hip.volume_positions_list_device(grid, update, d_indices, n, out=out) is out
            assert_same_words(back(hip, out, n * 4, 4), want, "%s, %d entries" % (name, n))
            if n:
                assert_same_words(hip.volume_positions_list(grid, update, indices, n), want, "%s, %d entries, the host variant" % (name, n))
    with capi.Context(0) as fresh:                                       # no scene is needed
        assert_same_words(fresh.volume_positions_list(grid, update_of(0.5), n_list=grid.probes), ref.positions(grid, update_of(0.5), n_list=grid.probes), "a fresh context")


@pytest.mark.parametrize("m", MAP_SIZES)
@pytest.mark.parametrize("count", GRIDS)
def test_the_blend_is_the_references_bits(hip, ref, count, m):
    """synthetic rows that hold every state, NaNs and infinities in new and in old SH rows and in single map rows, and zero-initialised old rows, among rows of poison"""
    grid, vmap, bins = grid_of(count), map_of(m, 5) if m else None, (m or 0) * (m or 0)
    probes = grid.probes
    seen = set()
    for n_list in NS:
        for k, (name, indices, (first, stride), n) in enumerate(lists_of(probes, n_list, seed=n_list)):
            entries = entries_of(indices, first, stride, n)
            sh, maps, new_sh, new_maps, flavours = synthetic_case(probes, bins, entries, n_list + k)
            host_sh, host_maps, listed = poisoned_volume(probes, bins, entries, sh, maps)
            d_indices = device_words(indices, 0) if indices is not None and n else None
            d_new_sh = device_words(new_sh, 0) if n else 0
            d_new_maps = device_words(new_maps if n else np.zeros((1, 4), np.float32), 0) if bins else None      # (no entries: a map still comes with its maps)
            for h in HYSTERESES:
                what = "%s, %d entries, h %g" % (name, n, h)
                update = update_of(h, first, stride)
                want_sh, want_maps, want_state = ref.blend(grid, update, new_sh, host_sh, new_maps, host_maps, indices, n)
                d_sh, d_state = device_words(host_sh, SPARE * 36), device_words(np.full(n, POISON, np.uint32), SPARE)
                d_maps = device_words(host_maps, SPARE * 4) if bins else None
                torch.cuda.synchronize()
                with_state = h != 0.97 or n == 0
                got = hip.volume_blend_device(grid, vmap, update, d_new_sh, d_sh, d_new_maps, d_maps, d_indices, n, state=d_state if with_state else None)
                assert got is (d_state if with_state else None)
                got_sh = back(hip, d_sh, probes * 36, 36)
                assert_same_words(got_sh, want_sh, what)
                assert (got_sh[~listed] == POISON).all()                  # the probes the list does not name
                if bins:
                    got_maps = back(hip, d_maps, probes * bins * 4, 4)
                    assert_same_words(got_maps, want_maps, what + ", maps")
                    assert (got_maps.reshape(probes, -1)[~listed] == POISON).all()
                got_state = back(hip, d_state, n, 1).reshape(-1)
                if with_state:
                    assert got_state.tolist() == want_state.tolist(), what
                    seen.update(got_state.tolist())
                    for j, e in enumerate(entries):                       # what the rows were made to hold is what the states say
                        expected = SKIPPED if e >= probes else FLAVOUR_STATE[flavours[j]] if h != 0.0 or FLAVOUR_STATE[flavours[j]] == KEPT else TAKEN
                        assert got_state[j] == expected, (what, j, flavours[j])
                else:
                    assert (got_state == POISON).all()                    # no state array: nothing else is written
                if n:
                    assert hip.last_volume_update() == {"entries": n, "groups": (n + 3) // 4, "size": m or 0, "listed": int(indices is not None), "chunks": 0, "fused": 0}
                if n and h == 0.5 and name in ("out_of_range", "arithmetic"):
                    host = hip.volume_blend(grid, vmap, update, new_sh, host_sh, new_maps, host_maps, indices, n)
                    assert_same_words(host[0], want_sh, what + ", the host variant")
                    assert host[2].tolist() == want_state.tolist()
                    if bins:
                        assert_same_words(host[1], want_maps, what + ", the host variant's maps")
    if probes >= 8:
        assert seen == {BLENDED, TAKEN, KEPT, SKIPPED}                    # (every state in ONE call: the next test)


def test_every_state_in_one_call_needs_no_scene(ref):
    grid, vmap = grid_of((3, 2, 4)), map_of(3, 5)
    indices = np.array([23, 1, 24, 5, 9, 2, 17, 0xffffffff, 11], np.uint32)
    sh, maps, new_sh, new_maps, _ = synthetic_case(24, 9, [int(x) for x in indices], 0)
    want_sh, want_maps, want_state = ref.blend(grid, update_of(0.97), new_sh, sh, new_maps, maps, indices)
    assert set(want_state.tolist()) == {BLENDED, TAKEN, KEPT, SKIPPED}
    with capi.Context(0) as fresh:
        d_sh, d_maps = device_words(sh, 0), device_words(maps, 0)
        state = fresh.volume_blend_device(grid, vmap, update_of(0.97), device_words(new_sh, 0), d_sh, device_words(new_maps, 0), d_maps, device_words(indices, 0), state=True)
        assert_same_words(back(fresh, d_sh, 24 * 36, 36), want_sh, "a context without a scene")
        assert_same_words(back(fresh, d_maps, 24 * 9 * 4, 4), want_maps, "its maps")
        assert state.cpu().numpy().view(np.uint32).tolist() == want_state.tolist()


def cornell_grid(hip, oracle, scenes, count):
    """-> (scene, trace params with one sample and one bounce, a frame of 64 x 48, a grid of that count inside the hull of the frame's first hits)"""
    sc, t, _ = cornell_probes(oracle, scenes)
    hip.update_scene(sc)
    t.samples, t.max_reflections = 1, 1
    p = sc.frame_params(width=64, height=48, samples=1, max_reflections=1, use_filter=0)
    planes = hip.frame_surface(p, capi.SURFACE_POSITION)[0]
    hit = planes[planes[:, 3] != 0.0][:, :3]
    lo, hi = hit.min(axis=0), hit.max(axis=0)
    cells = np.maximum(np.array(count, np.float64) - 1.0, 1.0)
    grid = capi.VolumeGrid(lo + 0.2 * (hi - lo), 0.6 * (hi - lo) / cells, count, normal_bias=0.01 * float((hi - lo).max()))
    return sc, t, p, grid


def seeded(t, seed):
    return capi.TraceParams(t.samples, t.max_reflections, t.min_importancy, tuple(t.ambient), seed, t.texture_width)


@pytest.mark.parametrize("m", (None, 3))
def test_the_fused_update_is_its_three_parts(hip, oracle, scenes, m):
    sc, t, p, grid = cornell_grid(hip, oracle, scenes, (2, 2, 2))
    vmap, bins, q = map_of(m, 5) if m else None, (m or 0) ** 2, capi.ProbeParams(face_size=2, sky=(0.5, 0.25, 0.125))
    indices = np.array([6, 0, 8, 3, 5], np.uint32)                       # five entries, one of them out of range
    d_indices = device_words(indices, 0)
    resident = hip.volume_bake_map_device(grid, seeded(t, 3.0), q, vmap) if m else (hip.volume_bake_device(grid, seeded(t, 3.0), q), None)
    hip.sync()
    update = update_of(0.5)
    # the parts, onto copies of the resident rows
    d_positions = hip.volume_positions_list_device(grid, update, d_indices)
    fresh = hip.probes_sh_map_device(d_positions, t, q, vmap) if m else (hip.probes_sh_device(d_positions, t, q), None)
    want_sh, want_maps = resident[0].clone(), resident[1].clone() if m else None
    want_state = hip.volume_blend_device(grid, vmap, update, fresh[0], want_sh, fresh[1], want_maps, d_indices, state=True)
    hip.sync()
    want_sh, want_state = want_sh.cpu().numpy(), want_state.cpu().numpy().view(np.uint32)
    assert want_state.tolist() == [BLENDED, BLENDED, SKIPPED, BLENDED, BLENDED]
    assert not np.array_equal(want_sh, resident[0].cpu().numpy())
    for chunk, chunks in ((0, 1), (2, 3)):                                # flx_debug_set_probe_chunk: five entries in one chunk and in three
        hip.set_probe_chunk(chunk)
        try:
            got_sh, got_maps = device_words(resident[0].cpu().numpy(), SPARE * 36), device_words(resident[1].cpu().numpy(), SPARE * 4) if m else None
            d_state = device_words(np.full(5, POISON, np.uint32), SPARE)
            torch.cuda.synchronize()
            assert hip.volume_update_device(grid, t, q, vmap, update, got_sh, got_maps, d_indices, state=d_state) is d_state
            assert_same_words(back(hip, got_sh, 8 * 36, 36), want_sh, "the fused SH rows, chunk %d" % chunk)
            if m:
                assert_same_words(back(hip, got_maps, 8 * bins * 4, 4), want_maps.cpu().numpy(), "the fused maps, chunk %d" % chunk)
            assert back(hip, d_state, 5, 1).reshape(-1).tolist() == want_state.tolist()
            assert hip.last_volume_update() == {"entries": 5, "groups": 2, "size": m or 0, "listed": 1, "chunks": chunks, "fused": 1}
            assert hip.last_probes()["chunks"] == chunks and hip.last_probes()["n"] == 5
            if chunk:
                host = hip.volume_update(grid, t, q, vmap, update, resident[0].cpu().numpy(), resident[1].cpu().numpy() if m else None, indices)
                assert_same_words(host[0], want_sh, "the host variant in chunks")
                assert host[2].tolist() == want_state.tolist()
                if m:
                    assert_same_words(host[1], want_maps.cpu().numpy(), "the host variant's maps in chunks")
        finally:
            hip.set_probe_chunk(0)


@pytest.mark.parametrize("k", range(len(GRIDS)))
def test_an_update_with_h_zero_onto_zeroed_rows_is_the_bake(hip, oracle, scenes, k):
    sc, t, p, grid = cornell_grid(hip, oracle, scenes, GRIDS[k])
    probes, q = grid.probes, capi.ProbeParams(face_size=FACES[k], sky=(0.5, 0.25, 0.125))
    update = update_of(0.0, 0, 1)
    for m in (None, (1, 3, 8)[k]):
        vmap, bins = map_of(m, 5) if m else None, (m or 0) ** 2
        baked = hip.volume_bake_map_device(grid, t, q, vmap) if m else (hip.volume_bake_device(grid, t, q), None)
        d_sh, d_maps = device_words(np.zeros((probes, 36), np.float32), SPARE * 36), device_words(np.zeros((probes * bins, 4), np.float32), SPARE * 4) if m else None
        state = hip.volume_update_device(grid, t, q, vmap, update, d_sh, d_maps, None, probes, state=True)
        got_sh = back(hip, d_sh, probes * 36, 36)
        state, want_sh = state.cpu().numpy().view(np.uint32), baked[0].cpu().numpy()
        taken = state == TAKEN
        assert taken.sum() >= (probes + 1) // 2 and ((state == TAKEN) | (state == KEPT)).all()
        assert_same_words(got_sh[taken], want_sh[taken], "grid %d, m %s: the bake's SH rows" % (k, m))
        assert not np.isfinite(want_sh[~taken]).all(axis=1).any() and (got_sh[~taken] == 0).all()       # a poisoned bake row is rejected: the zeros stay
        if m:
            got_maps, want_maps = back(hip, d_maps, probes * bins * 4, 4).reshape(probes, bins, 4), baked[1].cpu().numpy().reshape(probes, bins, 4)
            fine = np.isfinite(want_maps).all(axis=2) & taken[:, None]    # (a map row with a word that is not finite keeps its zeros)
            assert_same_words(got_maps[fine], want_maps[fine], "grid %d, m %d: the bake's maps" % (k, m))
            assert (got_maps[~fine] == 0).all()


def test_two_updates_are_the_references_blend_of_two_bakes(hip, oracle, scenes, ref):
    sc, t, p, grid = cornell_grid(hip, oracle, scenes, (3, 2, 4))
    vmap, q = map_of(3, 5), capi.ProbeParams(face_size=2, sky=(0.5, 0.25, 0.125))
    first, second = seeded(t, 11.0), seeded(t, 12.0)
    a, b = hip.volume_bake_map_device(grid, first, q, vmap), hip.volume_bake_map_device(grid, second, q, vmap)
    hip.sync()
    a, b = [x.cpu().numpy() for x in a], [x.cpu().numpy() for x in b]
    assert not np.array_equal(a[0], b[0])                                # another seed, other rows
    d_sh, d_maps = device_words(np.zeros((24, 36), np.float32), SPARE * 36), device_words(np.zeros((24 * 9, 4), np.float32), SPARE * 4)
    zeros_sh, zeros_maps = np.zeros((24, 36), np.float32), np.zeros((24 * 9, 4), np.float32)
    s1 = hip.volume_update_device(grid, first, q, vmap, update_of(0.0), d_sh, d_maps, None, 24, state=True)
    s2 = hip.volume_update_device(grid, second, q, vmap, update_of(0.5), d_sh, d_maps, None, 24, state=True)
    want_sh, want_maps, w1 = ref.blend(grid, update_of(0.0), a[0], zeros_sh, a[1], zeros_maps, n_list=24)
    want_sh, want_maps, w2 = ref.blend(grid, update_of(0.5), b[0], want_sh, b[1], want_maps, n_list=24)
    assert_same_words(back(hip, d_sh, 24 * 36, 36), want_sh, "two updates")
    assert_same_words(back(hip, d_maps, 24 * 9 * 4, 4), want_maps, "two updates' maps")
    assert s1.cpu().numpy().view(np.uint32).tolist() == w1.tolist() and s2.cpu().numpy().view(np.uint32).tolist() == w2.tolist()
    assert (w2 == BLENDED).sum() >= 12
    # with equal seeds an update is deterministic: a rotating eighth, twice
    again = [device_words(np.ascontiguousarray(want_sh), 0), device_words(np.ascontiguousarray(want_sh), 0)]
    for d in again:
        hip.volume_update_device(grid, first, q, None, update_of(0.97, 1, 8), d, None, None, 3)
    hip.sync()
    assert torch.equal(again[0], again[1]) and not np.array_equal(again[0].cpu().numpy().view(np.uint32).reshape(24, 36)[[1, 9, 17]], want_sh.view(np.uint32)[[1, 9, 17]])
    # a lookup after the updates reads the rows as it reads any: the device's lookup on the updated rows is the host definition's on the reference's rows
    planes = hip.frame_surface(p, capi.SURFACE_POSITION | capi.SURFACE_NORMAL)
    pick = np.flatnonzero(planes[0][:, 3] != 0.0)[::7][:300]
    positions, normals = np.ascontiguousarray(planes[0][pick]), np.ascontiguousarray(planes[1][pick])
    got = hip.volume_irradiance_map_device(grid, d_sh, torch.from_numpy(positions).cuda(), torch.from_numpy(normals).cuda(), vmap, d_maps)
    hip.sync()
    want = capi.volume_irradiance_map_of(grid, vmap, want_sh, want_maps, positions, normals)
    assert_same_words(got.cpu().numpy(), want, "the lookup after two updates")
    assert np.isfinite(want).all() and (want[:, 3] > 0).all()


def test_an_update_between_two_frames_of_the_loop(hip, oracle, scenes):
    sc, t, p, grid = cornell_grid(hip, oracle, scenes, (2, 2, 2))
    vmap, q, update = map_of(3, 5), capi.ProbeParams(face_size=2, sky=(0.5, 0.25, 0.125)), update_of(0.5, 1, 2)
    sh, maps = hip.volume_bake_map(grid, seeded(t, 5.0), q, vmap)
    want_sh, want_maps, want_state = hip.volume_update(grid, t, q, vmap, update, sh, maps, n_list=4)
    frames = [sc.frame_params(width=48, height=36, samples=2, max_reflections=3, use_filter=0) for _ in range(2)]
    frames[1].random_seed = frames[0].random_seed + 1.0
    oracle_frames = [oracle.render(sc, f)[0] for f in frames]
    d_sh, d_maps, d_state = device_words(sh, SPARE * 36), device_words(maps, SPARE * 4), device_words(np.full(4, POISON, np.uint32), SPARE)
    torch.cuda.synchronize()
    for f in frames:
        hip.frame_begin(f)
    assert hip.frames_in_flight() == 2
    hip.volume_update_device(grid, t, q, vmap, update, d_sh, d_maps, None, 4, state=d_state)
    got = [hip.frame_end()[0] for _ in frames]
    assert_same_words(back(hip, d_sh, 8 * 36, 36), want_sh, "between the frames")
    assert_same_words(back(hip, d_maps, 8 * 9 * 4, 4), want_maps, "between the frames, maps")
    assert back(hip, d_state, 4, 1).reshape(-1).tolist() == want_state.tolist()
    for image, frame in zip(got, oracle_frames):
        image = np.asarray(image).reshape(frame.shape)
        assert ((image.view(np.uint32) == frame.view(np.uint32)) | (np.isnan(image) & np.isnan(frame))).all()


def test_refusals(hip, oracle, scenes):
    sc, t, p, grid = cornell_grid(hip, oracle, scenes, (2, 2, 2))
    torch.cuda.empty_cache()                                             # (the allocations below are then the device's own, of exactly these sizes)
    vmap, q, good = map_of(4, 3), capi.ProbeParams(face_size=2), update_of(0.5)
    sh, maps = hip.volume_bake_map(grid, t, q, vmap)
    hip.volume_update(grid, t, q, vmap, good, sh, maps, n_list=8)
    before = (hip.last_volume_update(), hip.last_probes(), hip.last_volume_map())

    def poison(n_bytes):
        return torch.full((n_bytes,), 0xA5, dtype=torch.uint8, device="cuda")

    d_sh, d_maps, d_new_sh, d_new_maps, d_indices, d_state, d_positions = (poison(8 * 144), poison(8 * 16 * 16), poison(5 * 144), poison(5 * 16 * 16), poison(5 * 4), poison(5 * 4),
                                                                           poison(5 * 16))
    short = poison(20 << 20)                                             # 20 MB, an allocation of its own: an array that ends a row or a word past END is too short
    host = np.zeros((4096, 4), np.float32)
    torch.cuda.synchronize()
    S, M, A, B, I, T, P = (x.data_ptr() for x in (d_sh, d_maps, d_new_sh, d_new_maps, d_indices, d_state, d_positions))
    END = short.data_ptr() + (20 << 20)

    positions = lambda u=good, i=I, n=5, o=P, gr=grid: hip.volume_positions_list_device(gr, u, i, n, out=o)
    blend = lambda u=good, vm=vmap, i=I, n=5, a=A, b=B, s=S, m=M, st=T, gr=grid: hip.volume_blend_device(gr, vm, u, a, s, b, m, i, n, state=st)
    update = lambda u=good, vm=vmap, i=I, n=5, s=S, m=M, st=T, gr=grid, tt=t, qq=q: hip.volume_update_device(gr, tt, qq, vm, u, s, m, i, n, state=st)
    calls = (("flx_volume_positions_list_device", positions), ("flx_volume_blend_device", blend), ("flx_volume_update_device", update))
    refused = []
    for name, call in calls:
        refused += [
            (lambda call=call: call(u=None), name + ": the update is NULL"),
            (lambda call=call: call(u=update_of(float("nan"))), name + ": hysteresis is not one of 0 .. 1"),
            (lambda call=call: call(u=update_of(float("inf"))), name + ": hysteresis is not one of 0 .. 1"),
            (lambda call=call: call(u=update_of(-0.001)), name + ": hysteresis is not one of 0 .. 1"),
            (lambda call=call: call(u=update_of(1.001)), name + ": hysteresis is not one of 0 .. 1"),
            (lambda call=call: call(u=update_of(0.5, reserved=1)), name + ": the update's reserved word is not 0"),
            (lambda call=call: call(n=9), name + ": n_list is above the grid's probes"),
            (lambda call=call: call(i=0, u=update_of(0.5, 3, 0)), name + ": stride is 0 for a list of more than one entry"),
            (lambda call=call: call(i=0, u=update_of(0.5, 0, 2)), name + ": first \\+ \\(n_list - 1\\) \\* stride is not a probe of the grid"),
            (lambda call=call: call(i=0, u=update_of(0.5, 4, 1)), name + ": first \\+ \\(n_list - 1\\) \\* stride is not a probe of the grid"),
            (lambda call=call: call(i=0, u=update_of(0.5, 0, 0x40000000)), name + ": first \\+ \\(n_list - 1\\) \\* stride is not a probe of the grid"),      # (a 32-bit product is 0)
            (lambda call=call: call(i=I + 2), name + ": an array is misaligned"),
            (lambda call=call: call(i=host.ctypes.data), name + ": the indices are not n_list words of 4 bytes in memory of the context's device"),
            (lambda call=call: call(i=END - 5 * 4 + 4), name + ": the indices are not n_list words of 4 bytes in memory of the context's device"),      # one word past the allocation's end
            # the order: the update before the count, the count before the list, the siblings before all of them
            (lambda call=call: call(u=update_of(2.0, reserved=1), n=9), name + ": hysteresis is not one of 0 .. 1"),
            (lambda call=call: call(u=update_of(0.5, reserved=1), n=9), name + ": the update's reserved word is not 0"),
            (lambda call=call: call(i=0, n=9, u=update_of(0.5, 0, 0)), name + ": n_list is above the grid's probes"),
            (lambda call=call: call(gr=None, u=None), name + ": the grid is NULL"),
            (lambda call=call: call(gr=capi.VolumeGrid(count=(0, 1, 1)), u=None), name + ": a count of the grid is 0"),
        ]
    for name, call in calls[1:]:
        refused += [
            (lambda call=call: call(vm=None), name + ": maps are given without a map"),
            (lambda call=call: call(m=0), name + ": a map is given without its maps"),
            (lambda call=call: call(vm=capi.VolumeMap(17, 3), u=None), name + ": the map's size is not one of 1 .. 16"),
            (lambda call=call: call(vm=capi.VolumeMap(4, 9), u=None), name + ": the map's sharpness is above 8"),
            (lambda call=call: call(s=0), name + ": an array is NULL"),
            (lambda call=call: call(s=S + 8), name + ": an array is misaligned"),
            (lambda call=call: call(st=T + 1), name + ": an array is misaligned"),
            (lambda call=call: call(s=host.ctypes.data), name + ": the SH rows are not nx \\* ny \\* nz rows of 144 bytes in memory of the context's device"),
            (lambda call=call: call(s=END - 8 * 144 + 16), name + ": the SH rows are not nx \\* ny \\* nz rows of 144 bytes in memory of the context's device"),
            (lambda call=call: call(m=END - 8 * 256 + 16), name + ": the maps are not nx \\* ny \\* nz \\* size \\* size rows of 16 bytes in memory of the context's device"),
            (lambda call=call: call(st=host.ctypes.data), name + ": the states are not n_list words of 4 bytes in memory of the context's device"),
            (lambda call=call: call(st=END - 5 * 4 + 4), name + ": the states are not n_list words of 4 bytes in memory of the context's device"),
            (lambda call=call: call(st=I), name + ": the arrays overlap"),
            (lambda call=call: call(st=S + 16, n=4), name + ": the arrays overlap"),
            (lambda call=call: call(i=M + 1024), name + ": the arrays overlap"),
            (lambda call=call: call(m=S, vm=capi.VolumeMap(1, 3)), name + ": the arrays overlap"),
        ]
    refused += [
        (lambda: positions(o=0), "flx_volume_positions_list_device: an array is NULL"),
        (lambda: positions(o=P + 4), "flx_volume_positions_list_device: an array is misaligned"),
        (lambda: positions(o=END - 5 * 16 + 16), "flx_volume_positions_list_device: the positions are not n_list rows of 16 bytes in memory of the context's device"),
        (lambda: positions(o=S, i=S + 16), "flx_volume_positions_list_device: the arrays overlap"),
        (lambda: blend(a=0), "flx_volume_blend_device: an array is NULL"),
        (lambda: blend(b=0), "flx_volume_blend_device: a map is given without its maps"),
        (lambda: blend(vm=None, m=0), "flx_volume_blend_device: maps are given without a map"),
        (lambda: blend(a=END - 5 * 144 + 16), "flx_volume_blend_device: the new SH rows are not n_list rows of 144 bytes in memory of the context's device"),
        (lambda: blend(b=END - 5 * 256 + 16), "flx_volume_blend_device: the new maps are not n_list \\* size \\* size rows of 16 bytes in memory of the context's device"),
        (lambda: blend(a=S, n=4), "flx_volume_blend_device: the arrays overlap"),
        (lambda: blend(a=B, n=1), "flx_volume_blend_device: the arrays overlap"),
        (lambda: blend(b=M + 256, n=1), "flx_volume_blend_device: the arrays overlap"),
        (lambda: blend(b=A, vm=capi.VolumeMap(1, 3), n=4), "flx_volume_blend_device: the arrays overlap"),
        (lambda: blend(i=A + 16), "flx_volume_blend_device: the arrays overlap"),
        (lambda: blend(st=B + 64), "flx_volume_blend_device: the arrays overlap"),
        # the siblings of the whole path come first, in their words
        (lambda: update(tt=None, u=None), "flx_rays_trace_ordered: params is NULL"),
        (lambda: update(qq=None, u=None), "flx_probes_sh_device: the probe params are NULL"),
        (lambda: update(qq=capi.ProbeParams(face_size=0), gr=None), "flx_probes_sh_device: face_size is not one of 1 .. 256"),
        # the host variants: the same rules, and a list they can look at
        (lambda: hip.volume_positions_list(grid, update_of(2.0), n_list=3), "flx_volume_positions_list: hysteresis is not one of 0 .. 1"),
        (lambda: hip.volume_positions_list(grid, good, [1, 5, 1]), "flx_volume_positions_list: the list names a probe twice"),
        (lambda: hip.volume_blend(grid, vmap, good, np.zeros((3, 36), np.float32), sh, np.zeros((48, 4), np.float32), maps, [7, 2, 7]), "flx_volume_blend: the list names a probe twice"),
        (lambda: hip.volume_blend(grid, None, good, np.zeros((3, 36), np.float32), sh, None, maps, [7, 2, 1]), "flx_volume_blend: maps are given without a map"),
        (lambda: hip.volume_blend(grid, vmap, good, np.zeros((3, 36), np.float32), sh, None, None, [7, 2, 1]), "flx_volume_blend: a map is given without its maps"),
        (lambda: hip.volume_update(grid, t, q, vmap, good, sh, maps, [0, 0]), "flx_volume_update: the list names a probe twice"),
        (lambda: hip.volume_update(grid, t, q, vmap, None, sh, maps, [0, 1]), "flx_volume_update: the update is NULL"),
        (lambda: hip.volume_update(grid, t, q, vmap, update_of(0.5, 1, 1), sh, maps, n_list=8), "flx_volume_update: first \\+ \\(n_list - 1\\) \\* stride is not a probe of the grid"),
        (lambda: hip.volume_update(grid, t, q, vmap, good, sh[:7], maps, [0, 1]), "one SH row and size x size map rows per probe"),
    ]
    for call, words in refused:
        with pytest.raises((capi.FlexLightHipError, ValueError), match=r"(failed \(\d+\): .*(" + words + "))|(" + words + ")"):
            call()
    # a host list may repeat entries out of range: they are skipped
    assert hip.volume_blend(grid, vmap, good, np.zeros((3, 36), np.float32), sh, np.zeros((48, 4), np.float32), maps, [8, 2, 8])[2].tolist() == [SKIPPED, BLENDED, SKIPPED]
    before = (hip.last_volume_update(), before[1], before[2])
    hip.sync()
    for buffer in (d_sh, d_maps, d_new_sh, d_new_maps, d_indices, d_state, d_positions, short):
        assert bool((buffer == 0xA5).all())                              # nothing was written
    # no entries: FLX_OK and nothing enqueued, the rules that need no array looked at first
    hip.volume_positions_list_device(grid, good, 0, 0, out=0)
    hip.volume_blend_device(grid, vmap, good, 0, 0, B, M, 0, 0)
    hip.volume_blend_device(grid, None, good, 0, 0, None, None, None, 0)
    hip.volume_update_device(grid, t, q, vmap, good, 0, M, 0, 0)
    with pytest.raises(capi.FlexLightHipError, match="flx_volume_update_device: hysteresis is not one of 0 .. 1"):
        hip.volume_update_device(grid, t, q, vmap, update_of(-1.0), 0, M, 0, 0)
    with pytest.raises(capi.FlexLightHipError, match="flx_volume_blend_device: maps are given without a map"):
        hip.volume_blend_device(grid, None, good, 0, 0, 0, M, 0, 0)
    assert (hip.last_volume_update(), hip.last_probes(), hip.last_volume_map()) == before
    # the calls still work
    assert hip.volume_update(grid, t, q, vmap, good, sh, maps, n_list=8)[2].tolist() == [BLENDED] * 8
