"""Probe relocation across its seams (csrc/flx_volume_relocate.hip, include/flx_volume_relocate.h, the relocated lookup of csrc/flx_volume.hip): k_probe_relocate at
faces up to the largest the library accepts, with the three keys won at texels a narrow key, a spilling complement or a lost last trip would get wrong; the reduction
and the position rows of 32 769 probes of a 33 x 32 x 32 grid; the whole path on the Cornell scene over that grid — two launches of k_probe_rays inside one chunk,
nine chunks whose `first` reaches 32 768, trace slabs under them — against its parts and against the CPU chain; the natural chunk of 5 probes of face size 256, no
knob set; and the relocated lookup over the grid beyond one launch.  Every output goes into a poisoned buffer with spare rows behind it and is compared in all words,
bit for bit, with the CPU reference (tests/volume_relocate_ref, whose standing at these sizes test_volume_relocate_cpu.py checks) or with the calls a fused call is
made of."""
import time

import numpy as np
import pytest
import torch

import volume_util
from flexlight_hip import capi
from probe_util import reference as probe_reference
from surface_util import reference as surface_reference
from volume_relocate_util import (FLAVOURS, FREEZE, INACTIVE, LARGE, POISON, REJECTED, SPARE, assert_same_rows, assert_same_words, back, device_words, grid_of, map_of,
                                  placed_probe, placed_texels, placed_winners, planes_of, reference, relocate_of, rule_of, seam_planes, states_of, synthetic_maps,
                                  synthetic_probe, synthetic_sh)
from volume_update_util import update_of

pytestmark = pytest.mark.gpu

LAUNCH = 32768          # PROBE_LAUNCH of csrc/flx_probes.hip; the sibling kernels' cut
GRID = (33, 32, 32)     # 33 792 probes: test_probe_seams_gpu.py's grid
PROBES = 33792
ENTRIES = 32769
SEAM = slice(LAUNCH - 8, LAUNCH + 8)
FIELDS = capi.SURFACE_HIT | capi.SURFACE_NORMAL


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return reference(tmp_path_factory)


@pytest.fixture(scope="module")
def vref(tmp_path_factory):
    return volume_util.reference(tmp_path_factory)


def big_grid(normal_bias=0.0, visibility=True):
    """33 x 32 x 32; no spacing is a power of two"""
    return capi.VolumeGrid((0.1, -0.2, 0.3), (0.3, 0.7, 1.1), GRID, normal_bias, 0.05, capi.VOLUME_VISIBILITY if visibility else 0)


def pairwise_different(rows):
    rows = np.ascontiguousarray(rows)
    return len(np.unique(rows.view(np.uint32).reshape(len(rows), -1), axis=0)) == len(rows)


def poison_rows(rows, width=4):
    return np.full((rows, width), POISON, np.uint32)


# ---- 2. k_probe_relocate at large faces --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w, counts", LARGE)
def test_the_reduction_of_large_faces(hip, ref, w, counts):
    """Every second probe of a run is a placed one — its keys won at R - 1, in the last trip, on either side of 2^16 .. 2^18, a different texel for every probe of the
    run, under rule 1 or rule 2 with a move, where the winning texel's direction is the move — and the probes between them are ordinary flavours.  The run starts at
    first_probe != 0 of a 24-probe grid whose other rows keep their poison."""
    grid, rays = grid_of((3, 2, 4)), 6 * w * w
    cases, texels = placed_winners(w), placed_texels(w)
    high = texels[::-1]
    won = []
    for ci, n in enumerate(counts):
        first = 7 if n == 1 else 24 - n
        for flags in (0, FREEZE):
            relocate = relocate_of(flags=flags)
            rng = np.random.default_rng(1000 * w + 10 * n + flags)
            hits, normals, host = [], [], poison_rows(24).view(np.float32).copy()
            for k in range(n):
                if k % 2 == 0:
                    j = k // 2 + ci
                    s, side, is_hit, old = placed_probe(w, rng, relocate, cases[4 * texels.index(high[j % len(high)]) + (3 if flags else j % 3)])
                else:
                    s, side, is_hit, old = synthetic_probe(w, FLAVOURS[(k + w + n) % len(FLAVOURS)], rng, relocate)
                h, nn = planes_of(s, side, is_hit)
                hits.append(h), normals.append(nn)
                host[first + k] = old
                if not flags:
                    won += [key & 0xffffffff for key in ref.sums(w, h, nn)[2:] if key != 0xffffffffffffffff]
            hit, normal = np.concatenate(hits), np.concatenate(normals)
            want = ref.relocate(grid, relocate, w, hit, normal, host, first_probe=first)
            what = "w %d, %d probes from %d, flags %d" % (w, n, first, flags)
            if not flags:
                assert (want[first:first + n:2, :3] != host[first:first + n:2, :3]).any(axis=1).all(), what      # every placed probe moves: a wrong texel is a wrong row
            d_offsets = device_words(host, SPARE * 4)
            torch.cuda.synchronize()
            assert hip.probe_relocate_device(grid, relocate, device_words(hit, 0), device_words(normal, 0), n, w, d_offsets, first) is d_offsets
            got = back(hip, d_offsets, 24 * 4, 4)
            assert_same_words(got, want, what)
            outside = np.ones(24, bool)
            outside[first:first + n] = False
            assert (got[outside] == POISON).all()
            assert hip.last_volume_relocate() == {"probes": n, "face_size": w, "chunks": 0, "chunk": 0, "groups": (n + 3) // 4, "flags": flags, "first": first, "fused": 0}
            if flags:
                assert_same_words(got[first:first + n, :3], host[first:first + n, :3], "freeze")
            if (w, n, flags) == (64, 1, 0):
                assert_same_words(hip.probe_relocate(grid, relocate, hit, normal, n, w, host, first), want, "the host variant")
    # the reference's own winners reach where a kernel can lose them
    assert max(won) >= rays - 64 and (w < 128 or max(won) >= 65536) and (w < 256 or max(won) >= 262144), (w, max(won))
    assert len([t for t in won if t >= rays - 64]) >= 2 and min(won) < 64


# ---- 3. probe counts beyond 32 768 ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w, n, first", ((1, ENTRIES, 1023), (2, ENTRIES, 0)))
def test_the_reduction_of_32769_probes(hip, ref, w, n, first):
    """8 193 workgroups, the last with one wave; 32 769 + 1 023 ends at the grid's end.  ONE READING OF THE ISSUE: the sixteen rows around 32 768 cannot all be pairwise
    different after the call — see below —, so those that can be are, and the inputs are."""
    grid, relocate = big_grid(), relocate_of()
    hit, normal, old, _ = seam_planes(n, w, w, relocate)
    host = poison_rows(PROBES).view(np.float32).copy()
    host[first:first + n] = old
    want = ref.relocate(grid, relocate, w, hit, normal, host, first_probe=first)
    seam = slice(LAUNCH - 8, min(LAUNCH + 8, first + n))                     # (the rows of the run among the sixteen around 32 768)
    moved = (want[:, :3].view(np.uint32) != host[:, :3].view(np.uint32)).any(axis=1)
    assert moved[LAUNCH:first + n].sum() >= (first + n - LAUNCH) // 4 and moved[:LAUNCH].sum() > 8000
    # The rows around 32 768 are pairwise different on the way in, and on the way out but for the probes that go home: rule 3 with no front nearer than the way back
    # ("far", "no_hits": two flavours of six) ends exactly on the lattice point, by the definition, whatever the probe.
    home = (want[seam, :3] == 0).all(axis=1)
    rows = seam.stop - seam.start
    assert pairwise_different(old[seam.start - first:seam.stop - first]) and pairwise_different(want[seam][~home]) and (~home).sum() >= rows - 2 * ((rows + 5) // 6)
    states = states_of(want[first:first + n])
    assert set(rule_of(states).tolist()) == {1, 2, 3} and {int(s) & (INACTIVE | REJECTED) for s in states} == {0, INACTIVE, REJECTED, INACTIVE | REJECTED}
    d_offsets = device_words(host, SPARE * 4)
    torch.cuda.synchronize()
    assert hip.probe_relocate_device(grid, relocate, device_words(hit, 0), device_words(normal, 0), n, w, d_offsets, first) is d_offsets
    got = back(hip, d_offsets, PROBES * 4, 4)
    assert_same_words(got[seam], want[seam], "the rows around 32 768")
    assert_same_words(got, want, "%d probes of w = %d from %d" % (n, w, first))
    outside = np.ones(PROBES, bool)
    outside[first:first + n] = False
    assert (got[outside] == POISON).all()
    assert (got[LAUNCH:first + n] != host.view(np.uint32)[LAUNCH:first + n]).any(axis=1).all()          # rows from 32 768 on were changed: the state at least
    assert hip.last_volume_relocate() == {"probes": n, "face_size": w, "chunks": 0, "chunk": 0, "groups": 8193, "flags": 0, "first": first, "fused": 0}


def test_positions_with_offsets_of_a_grid_beyond_32768_probes(hip, ref):
    grid = big_grid()
    rng = np.random.default_rng(33)
    offsets = rng.uniform(0.01, 0.3, size=(PROBES, 4)).astype(np.float32) * rng.choice(np.array([-1.0, 1.0], np.float32), size=(PROBES, 4))
    offsets.view(np.uint32)[:, 3] = rng.integers(1, 16, size=PROBES)
    d_offsets = device_words(offsets, 0)

    def run(update, indices, n, what, host=False):
        want = ref.positions(grid, offsets, update, indices, n)
        out = device_words(poison_rows(len(want)), SPARE * 4)
        d_indices = device_words(indices, 0) if indices is not None else None
        torch.cuda.synchronize()
        assert hip.volume_positions_offset_device(grid, d_offsets, update, d_indices, n, out=out) is out
        assert_same_words(back(hip, out, len(want) * 4, 4), want, what)
        if host:
            assert_same_words(hip.volume_positions_offset(grid, offsets, update, indices, n), want, what + ", the host variant")
        return want

    whole = run(None, None, None, "the whole grid")
    assert pairwise_different(whole[:, :3]) and not (whole[:, :3] == ref.positions(grid, np.zeros_like(offsets))[:, :3]).all(axis=1).any()
    listed = rng.permutation(PROBES)[:ENTRIES].astype(np.uint32)             # a permutation's head, every 1000th entry out of range
    listed[::1000] = PROBES + np.arange(len(listed[::1000]), dtype=np.uint32)
    got = run(update_of(0.5), listed, None, "a list of 32 769 entries", host=True)
    assert_same_words(got, whole[np.where(listed < PROBES, listed, PROBES - 1)], "a skipped entry gets the last probe's row")
    assert listed[LAUNCH] < PROBES and (listed >= PROBES).sum() == 33 and (listed[listed < PROBES] > LAUNCH).sum() > 500      # the last entry names a probe; probes past 32 768 are named
    got = run(update_of(0.5, PROBES - ENTRIES, 1), None, ENTRIES, "first + j stride over the last 32 769 probes")
    assert_same_words(got, whole[PROBES - ENTRIES:], "first + j stride names those probes")


# ---- 4. the whole path across launches and chunks ----------------------------------------------------------------------------------------------------------------------------

# The 33 x 32 x 32 grid in the Cornell box (the room is -5 .. 5, the camera looks along +z).  Scaled into the hull of a frame's first hits as test_probe_seams_gpu.py's
# baked grid is, its last layer — the probes from 32 768 on — stands at z = 3, in free space behind the cuboids: every probe there is rule 3 and none moves (the CPU
# chain, with the room as the hull).  So origin and spacing are chosen: x from the left wall's 0.03 on (the first column is within min_front of it: rule 2, with a
# move), y from 0.4 above the floor, and z so that the last layer, z = 0.3, cuts through both cuboids (rule 1).  No spacing is a power of two.  min_front is
# test_volume_relocate_gpu.py's 0.3 scaled by the spacing's 0.2: with 0.3 itself every move is longer than limit spacing and nothing moves.
CORNELL_BIG = ((-4.97, -4.6, -4.35), (0.19, 0.2, 0.15))
NATURAL = 349525        # the probes of a natural chunk at face size 1: 2^21 / 6


def cornell_relocate(min_front, flags=0):
    return capi.VolumeRelocate(0.25, min_front, 20.0, 0.45, flags)


@pytest.fixture(scope="module")
def chain(tmp_path_factory, scenes, ref):
    """the CPU chain over the whole grid, two passes -> (scene, texture width, grid, relocation, the offset rows after each pass, the planes of each pass); what the
    test needs of the rows is asserted here, before the device is asked"""
    pref, sref = probe_reference(tmp_path_factory), surface_reference(tmp_path_factory)
    sc = scenes("cornell")
    tw = sc.frame_params(width=64, height=48, samples=1, max_reflections=1, use_filter=0).texture_width
    grid, relocate = capi.VolumeGrid(*CORNELL_BIG, GRID, normal_bias=0.05), cornell_relocate(0.06)
    offsets, rows, planes = np.zeros((PROBES, 4), np.float32), [], []
    for k in range(2):
        p = sref.rays(sc, pref.rays(ref.positions(grid, offsets), 1), tw)
        planes.append((p[0], p[3]))
        offsets = ref.relocate(grid, relocate, 1, p[0], p[3], offsets)
        rows.append(offsets)
    states = states_of(rows[0])
    for side in (slice(0, LAUNCH), slice(LAUNCH, PROBES)):                    # both sides of probe 32 768 hold all three rules and some INACTIVE rows
        assert set(rule_of(states[side]).tolist()) == {1, 2, 3} and 0 < (states[side] & INACTIVE != 0).sum() < PROBES // 10
        assert np.abs(rows[0][side, :3]).max() > 0
    assert (np.abs(rows[0][:, :3]).max(axis=1) > 0).sum() >= 100 and len(set(states[SEAM].tolist())) >= 3
    assert (rows[1] != rows[0]).any(axis=1).sum() >= 100 and (rows[1][LAUNCH:] != rows[0][LAUNCH:]).any()
    return sc, tw, grid, relocate, rows, planes


def device_parts(ctx, grid, relocate, tw, d_offsets):
    """the four parts one after the other, in place in d_offsets -> the two planes on the device"""
    d_positions = ctx.volume_positions_offset_device(grid, d_offsets)
    d_rays = ctx.probe_rays_device(d_positions, 1)
    planes = ctx.surface_rays_device(d_rays.view(-1, 8), FIELDS, tw)
    ctx.probe_relocate_device(grid, relocate, planes[0], planes[1], PROBES, 1, d_offsets)
    return planes


def test_the_whole_path_across_launches_and_chunks(hip, ref, chain):
    """Face size 1 over CORNELL_BIG — an origin and a spacing chosen, not scaled from a frame's hull: see the comment there — with min_front scaled to the spacing.
    The parts one after the other, the whole call in one chunk (two launches of k_probe_rays), in nine chunks of 4 096 and under trace slabs of 1 000 rays, a second
    pass from the first pass's rows, and the host variant: all 33 792 rows, and the rows at the seam and at the grid's end first, against the CPU chain."""
    sc, tw, grid, relocate, rows, cpu_planes = chain
    hip.update_scene(sc)
    zeros = np.zeros((PROBES, 4), np.float32)
    hip.set_probe_chunk(0)
    hip.set_trace_slab(0)
    d_parts = device_words(zeros, SPARE * 4)
    torch.cuda.synchronize()
    planes = device_parts(hip, grid, relocate, tw, d_parts)
    parts = back(hip, d_parts, PROBES * 4, 4)
    assert hip.last_volume_relocate() == {"probes": PROBES, "face_size": 1, "chunks": 0, "chunk": 0, "groups": 8448, "flags": 0, "first": 0, "fused": 0}
    host_planes = planes.cpu().numpy().view(np.uint32)
    assert_same_words(host_planes[0], cpu_planes[0][0], "the HIT plane against the CPU chain")
    assert_same_words(host_planes[1], cpu_planes[0][1], "the NORMAL plane against the CPU chain")
    assert_same_words(parts[SEAM], rows[0][SEAM], "the parts against the CPU chain, the sixteen rows at the seam")
    assert_same_words(parts[-16:], rows[0][-16:], "the parts against the CPU chain, the grid's last sixteen")
    assert_same_words(parts, rows[0], "the parts against the CPU chain")
    # the sixteen probes at the seam and the grid's last sixteen in a reduction of their own on their own planes
    for first in (LAUNCH - 8, PROBES - 16):
        own = device_words(zeros, SPARE * 4)
        torch.cuda.synchronize()
        hip.probe_relocate_device(grid, relocate, planes[0][first * 6:(first + 16) * 6].contiguous(), planes[1][first * 6:(first + 16) * 6].contiguous(), 16, 1, own, first)
        got = back(hip, own, PROBES * 4, 4)
        assert_same_words(got[first:first + 16], rows[0][first:first + 16], "sixteen probes from %d against the CPU chain" % first)
        assert (np.delete(got, np.s_[first:first + 16], axis=0) == 0).all()
    # the second pass of the parts, from the first pass's rows
    device_parts(hip, grid, relocate, tw, d_parts)
    parts2 = back(hip, d_parts, PROBES * 4, 4)
    assert_same_words(parts2, rows[1], "the second pass of the parts against the CPU chain")
    # the whole call: one chunk (two launches of k_probe_rays), nine chunks whose first reaches 32 768, and trace slabs of 1 000 rays under them
    for chunk, slab, chunks in ((0, 0, 1), (4096, 0, 9), (4096, 1000, 9)):
        hip.set_probe_chunk(chunk)
        hip.set_trace_slab(slab)
        try:
            m = PROBES - (chunks - 1) * (chunk or PROBES)
            for k, (start, want) in enumerate(((zeros, parts), (parts, parts2))):
                if k == 1 and slab:
                    continue
                what = "pass %d, chunk %d, slab %d" % (k, chunk, slab)
                d_offsets = device_words(start, SPARE * 4)
                torch.cuda.synchronize()
                assert hip.volume_relocate_device(grid, relocate, 1, d_offsets, tw) is d_offsets
                got = back(hip, d_offsets, PROBES * 4, 4)
                assert_same_words(got[SEAM], want[SEAM], what + ", the sixteen rows at the seam")
                assert_same_words(got[-16:], want[-16:], what + ", the grid's last sixteen")
                assert_same_words(got, want, what)
                assert hip.last_volume_relocate() == {"probes": PROBES, "face_size": 1, "chunks": chunks, "chunk": chunk or NATURAL, "groups": (m + 3) // 4, "flags": 0,
                                                      "first": 0, "fused": 1}
                last = hip.last_surface()
                assert last["fields"] == FIELDS and last["n"] == m * 6 and last["slab"] == (slab or 1 << 21), last
            if chunk and not slab:
                assert_same_words(hip.volume_relocate(grid, relocate, 1, zeros, tw), parts, "the host variant in chunks of 4096")
        finally:
            hip.set_probe_chunk(0)
            hip.set_trace_slab(0)


def test_a_chunk_whose_first_probe_is_beyond_16_bits(hip, ref, scenes, tmp_path_factory):
    """Beyond the issue's cases: 33 792 probes never put a chunk's `first` past 65 535, so a `d_offsets + first` kept in 16 bits passes everything above.  A 65 x 32 x
    32 grid in the same box (66 560 probes; the spacing in x and y narrower, the last layer still z = 0.3) in chunks of 4 096 has seventeen chunks, the last from
    probe 65 536 on, and in one chunk three launches of k_probe_rays.  All rows against the CPU chain."""
    pref, sref = probe_reference(tmp_path_factory), surface_reference(tmp_path_factory)
    sc = scenes("cornell")
    hip.update_scene(sc)
    tw = sc.frame_params(width=64, height=48, samples=1, max_reflections=1, use_filter=0).texture_width
    grid, relocate = capi.VolumeGrid((-4.97, -4.9, -4.35), (0.11, 0.13, 0.15), (65, 32, 32), normal_bias=0.05), cornell_relocate(0.06)
    probes, cut = 66560, 65536
    zeros = np.zeros((probes, 4), np.float32)
    p = sref.rays(sc, pref.rays(ref.positions(grid, zeros), 1), tw)
    want = ref.relocate(grid, relocate, 1, p[0], p[3], zeros)
    states = states_of(want)
    for side in (slice(0, cut), slice(cut, probes)):
        assert set(rule_of(states[side]).tolist()) == {1, 2, 3} and (np.abs(want[side, :3]).max(axis=1) > 0).sum() >= 40
    assert len(set(states[cut - 8:cut + 8].tolist())) >= 3
    for chunk, chunks, m in ((4096, 17, 1024), (0, 1, probes)):
        hip.set_probe_chunk(chunk)
        try:
            d_offsets = device_words(zeros, SPARE * 4)
            torch.cuda.synchronize()
            assert hip.volume_relocate_device(grid, relocate, 1, d_offsets, tw) is d_offsets
            got = back(hip, d_offsets, probes * 4, 4)
            assert_same_words(got[cut - 8:], want[cut - 8:], "chunk %d, the rows from the last chunk's seam on" % chunk)
            assert_same_words(got, want, "chunk %d" % chunk)
            assert hip.last_volume_relocate() == {"probes": probes, "face_size": 1, "chunks": chunks, "chunk": chunk or NATURAL, "groups": m // 4, "flags": 0, "first": 0, "fused": 1}
            assert hip.last_surface()["n"] == m * 6
        finally:
            hip.set_probe_chunk(0)


# ---- 5. the natural chunk --------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_natural_chunk(hip, ref, scenes):
    """six probes of face size 256: 2 359 296 rays, which the chunks cut at 5 probes = 1 966 080 rays; no knob is set.  A natural chunk is 2^21 rays by definition: the
    test cannot be smaller, and it is the one call plus its parts.  A line of six probes from the left wall of the Cornell box into the short cuboid, at the height
    and depth of test_volume_relocate_gpu.py's probe 18, which is probe 3 here: probe 0 stands 0.1 from the wall (rule 2), probes 3 and 4 inside the cuboid (rule 1),
    and probe 5 — the second chunk — in free space (rule 3), so a second chunk that reduced the first chunk's planes would give probe 0's row.  The parts' planes
    are the reduction's input on real first hits at the largest face."""
    w, n, rays = 256, 6, 393216
    sc = scenes("cornell")
    hip.update_scene(sc)
    tw = sc.frame_params(width=64, height=48, samples=1, max_reflections=1, use_filter=0).texture_width
    grid, relocate = capi.VolumeGrid((-4.9, -3.0, 0.3), (0.8, 1.0, 1.0), (6, 1, 1), normal_bias=0.05), cornell_relocate(0.3)
    zeros = np.zeros((n, 4), np.float32)
    hip.set_probe_chunk(0)
    hip.set_trace_slab(0)
    d_offsets = device_words(zeros, SPARE * 4)
    torch.cuda.synchronize()
    began = time.perf_counter()
    assert hip.volume_relocate_device(grid, relocate, w, d_offsets, tw) is d_offsets
    hip.sync()
    print("flx_volume_relocate_device, 6 probes of face size 256: %.1f ms" % (1e3 * (time.perf_counter() - began)))
    got = back(hip, d_offsets, n * 4, 4)
    ran, last = hip.last_volume_relocate(), hip.last_surface()
    d_parts = device_words(zeros, SPARE * 4)
    torch.cuda.synchronize()
    d_positions = hip.volume_positions_offset_device(grid, d_parts)
    d_rays = hip.probe_rays_device(d_positions, w)
    planes = hip.surface_rays_device(d_rays.view(-1, 8), FIELDS, tw)
    hip.probe_relocate_device(grid, relocate, planes[0], planes[1], n, w, d_parts)
    parts = back(hip, d_parts, n * 4, 4)
    assert_same_words(got, parts, "the whole call against its parts")
    assert ran == {"probes": 6, "face_size": 256, "chunks": 2, "chunk": 5, "groups": 1, "flags": 0, "first": 0, "fused": 1}
    assert last["n"] == rays and last["fields"] == FIELDS and last["slab"] == 1 << 21, last          # the second chunk's one probe
    host_planes = planes.cpu().numpy()
    del planes, d_rays
    want = ref.relocate(grid, relocate, w, host_planes[0], host_planes[1], zeros)
    assert_same_words(parts, want, "the parts' reduction against the reference over the parts' planes")
    states = states_of(want)
    assert (rule_of(states)[[3, 4]] == 1).all() and (states[[3, 4]] & INACTIVE).all() and rule_of(states).tolist()[0::5] == [2, 3]
    assert not states[4] & REJECTED and np.abs(want[4, :3]).max() > 0.3          # one of the two leaves the cuboid by its side
    assert np.abs(want[0, :3]).max() > 0 and (want[5] != want[0]).any()          # the second chunk's row is not the first chunk's first
    won = [key & 0xffffffff for p in range(n) for key in ref.sums(w, host_planes[0][p * rays:(p + 1) * rays], host_planes[1][p * rays:(p + 1) * rays])[2:]
           if key != 0xffffffffffffffff]
    assert max(won) >= 262144 and len(set(won)) >= 8, won                      # real first hits win far into the planes


# ---- 6. the relocated lookup over a grid beyond one launch --------------------------------------------------------------------------------------------------------------

def device_relocated(ctx, grid, d_sh, positions, normals, d_offsets, vmap=None, d_maps=None):
    n = len(positions)
    out = device_words(poison_rows(n), SPARE * 4)
    d_positions, d_normals = torch.from_numpy(positions).cuda(), torch.from_numpy(normals).cuda()
    torch.cuda.synchronize()
    assert ctx.volume_irradiance_relocated_device(grid, d_sh, d_positions, d_normals, d_offsets, vmap, d_maps, out=out) is out
    return back(ctx, out, n * 4, 4)


def test_the_relocated_lookup_over_a_grid_beyond_one_launch(hip, ref, vref):
    """test_probe_seams_gpu.py's lookup test with offsets: synthetic SH rows and map rows of size 2, offsets within 0.2 of the spacing, about a third of the probes
    INACTIVE with NaN rows; 2 000 points in the first cell, on cell faces all over the grid, and outside it"""
    n, vmap = 2000, map_of(2, 1)
    rng = np.random.default_rng(6)
    clean_sh, clean_maps = synthetic_sh(PROBES, 2), synthetic_maps(PROBES, 2, 2)
    sh, maps = clean_sh.copy(), clean_maps.copy()
    offsets = (rng.uniform(-0.2, 0.2, size=(PROBES, 4)) * np.array(list(big_grid().spacing) + [1.0])).astype(np.float32)
    dead = rng.random(PROBES) < 0.35
    offsets.view(np.uint32)[:, 3] = np.where(dead, INACTIVE | (1 << 1) | REJECTED, 3 << 1)
    sh[dead] = np.nan
    maps[np.repeat(dead, 4)] = np.nan
    d_sh, d_maps, d_offsets = torch.from_numpy(sh).cuda(), torch.from_numpy(maps).cuda(), torch.from_numpy(offsets).cuda()
    d_clean_sh, d_clean_maps, d_zero = torch.from_numpy(clean_sh).cuda(), torch.from_numpy(clean_maps).cuda(), torch.zeros((PROBES, 4), device="cuda")
    for visibility in (True, False):
        grid = big_grid(0.05, visibility)
        sets = [(kind,) + volume_util.point_set(grid, kind, n, 1000 * k + n) for k, kind in enumerate(("one_cell", "faces", "outside"))]
        if visibility:                                         # what the points reach, by the reference's own corners (they do not depend on the flag, rows or offsets)
            last_cell, highest, some_dead, all_live = np.zeros(3, bool), 0, 0, 0
            for _, positions, normals in sets:
                for k in range(n):
                    index = vref.corners(grid, clean_sh, positions[k], normals[k])[0]
                    base = int(index[0])
                    last_cell |= np.array([base % GRID[0], base // GRID[0] % GRID[1], base // (GRID[0] * GRID[1])]) == np.array(GRID) - 2
                    highest = max(highest, int(index.max()))
                    some_dead += int(dead[index].any())
                    all_live += int(not dead[index].any())
            assert last_cell.all() and highest > LAUNCH and some_dead > 1000 and all_live > 50, (last_cell, highest, some_dead, all_live)
        for kind, positions, normals in sets:
            for with_map in (False, True):
                mm, dm, hm, dcm = (vmap, d_maps, maps, d_clean_maps) if with_map else (None, None, None, None)
                what = "%s, visibility %d, map %d" % (kind, visibility, with_map)
                want = ref.lookup(grid, sh, offsets, positions, normals, mm, hm)
                assert not np.isnan(want).any() and (want[:, 3] > 0).sum() > n // 2, what          # no dead probe's NaN reaches a row
                assert_same_rows(device_relocated(hip, grid, d_sh, positions, normals, d_offsets, mm, dm).view(np.float32), want, what)
                last = hip.last_volume()
                assert (last["n"], last["groups"], last["probes"], last["flags"]) == (n, 8, PROBES, grid.flags), last
                # zero offsets and clean rows: the plain lookup of the same run
                d_positions, d_normals = torch.from_numpy(positions).cuda(), torch.from_numpy(normals).cuda()
                plain = (hip.volume_irradiance_map_device(grid, d_clean_sh, d_positions, d_normals, vmap, d_clean_maps) if with_map
                         else hip.volume_irradiance_device(grid, d_clean_sh, d_positions, d_normals))
                hip.sync()
                assert_same_rows(device_relocated(hip, grid, d_clean_sh, positions, normals, d_zero, mm, dcm).view(np.float32), plain.cpu().numpy(), what + ", zero offsets")
