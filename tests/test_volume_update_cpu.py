"""Volume updates without a GPU (include/flexlight_hip_debug.h, "volume updates"; include/flx_volume_update.h): the CPU reference the GPU tests compare against is
itself held against a float64 restatement written by hand and against the properties a hysteresis blend must have; the four states come in their order; the map rows
make their two exceptions; the calls are declared, exported and bound; the update structure has the C compiler's layout; and the argument rules that need no device
(csrc/flx_volume_update_args.h) hold in a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from volume_update_util import (BLENDED, FLAVOUR_STATE, GRIDS, HYSTERESES, KEPT, SKIPPED, TAKEN, assert_same_rows, assert_same_words, blend64, entries_of, grid_of, lists_of,
                                reference, synthetic_case, synthetic_maps, synthetic_sh, update_of)
from volume_util import reference as volume_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("flx_volume_positions_list_device", "flx_volume_positions_list", "flx_volume_blend_device", "flx_volume_blend", "flx_volume_update_device", "flx_volume_update",
         "flx_volume_blend_row_of", "flx_debug_last_volume_update")
ARGS_CASES = 252         # the cases tests/volume_update_args_main.cc runs
# float32 with one rounding per operation against the float64 restatement over the same inputs, relative to the larger of |old| and |new|: three roundings, each of
# at most 2^-24 of an intermediate that is at most 2 max(|old|, |new|).  The bound is the worst deviation measured on this test's own cases with a margin of 4x, as
# test_volume_map_cpu.py sets its bounds.
BLEND_BOUND = 4 * 2.03e-7            # observed 2.03e-07


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return reference(tmp_path_factory)


def test_the_update_structure_matches_the_c_compiler(tmp_path):
    from flexlight_hip import capi
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stdio.h>
#include <stddef.h>
#include "flexlight_hip_debug.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(struct flx_volume_update), offsetof(struct flx_volume_update, hysteresis), offsetof(struct flx_volume_update, first),
         offsetof(struct flx_volume_update, stride), offsetof(struct flx_volume_update, reserved));
  return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)]).decode().split()))
    u = capi.VolumeUpdate
    assert got == [C.sizeof(u), u.hysteresis.offset, u.first.offset, u.stride.offset, u.reserved.offset] == [16, 0, 4, 8, 12]
    q = capi.VolumeUpdate(0.5, 3, 8)
    assert (q.hysteresis, q.first, q.stride, q.reserved) == (0.5, 3, 8, 0)
    assert capi.UPDATE_STATES == ("blended", "taken", "kept", "skipped")


def test_finite_is_a_matter_of_the_exponent_bits(ref):
    for bits, finite in ((0x00000000, True), (0x80000000, True), (0x00000001, True), (0x7f7fffff, True), (0xff7fffff, True), (0x7f800000, False), (0xff800000, False),
                         (0x7f800001, False), (0x7fc00000, False), (0xffffffff, False), (0x7fffffff, False)):
        assert ref.finite(np.array([bits], np.uint32).view(np.float32)[0]) == finite, hex(bits)


def test_the_list_is_computed_in_64_bits(ref):
    assert ref.entry(update_of(0.5, 3, 8), 5) == 43
    assert ref.entry(update_of(0.5, 0xffffffff, 0xffffffff), 0xffffffff) == 0xffffffff + 0xffffffff * 0xffffffff
    assert ref.entry(update_of(0.5, 0, 0x80000000), 2) == 1 << 32              # (a 32-bit product is 0)
    assert ref.entry(update_of(0.5, 0xfffffff0, 0x10), 1) == 1 << 32           # (a 32-bit sum is 0)
    assert ref.entry(update_of(0.5, 3, 8), 1, indices=[9, 0xffffffff]) == 0xffffffff       # a list: first and stride are not read


def test_positions_are_the_grids_and_a_skipped_entry_gets_the_last_probes(ref, tmp_path_factory):
    plain = volume_reference(tmp_path_factory)
    for count in GRIDS:
        grid = grid_of(count)
        want = plain.positions(grid)
        assert_same_words(ref.positions(grid, update_of(0.5), n_list=grid.probes), want, "every probe, arithmetic")
        for name, indices, (first, stride), n in lists_of(grid.probes, 9):
            got = ref.positions(grid, update_of(0.5, first, stride), indices, n)
            entries = entries_of(indices, first, stride, n)
            assert_same_words(got, want[[e if e < grid.probes else grid.probes - 1 for e in entries]], name)
            assert (got[:, 3].view(np.uint32) == 0).all()


def test_the_four_states_in_their_order(ref):
    new, old = synthetic_sh(1, 1)[0], synthetic_sh(1, 2)[0]
    nan_new, inf_new = new.copy(), new.copy()
    nan_new[17], inf_new[35] = np.nan, np.inf
    zero, nan_old, inf_old, negative = np.zeros(36, np.float32), old.copy(), old.copy(), old.copy()
    nan_old[30], inf_old[3], negative[3] = np.nan, np.inf, -old[3]
    nan_word3 = old.copy()
    nan_word3[3] = np.nan
    assert ref.state(1, new, old, 0.5) == BLENDED and ref.state(1, new, old, 1.0) == BLENDED and ref.state(1, new, old, 1.0e-30) == BLENDED
    # each way of being taken
    for o, h in ((old, 0.0), (old, -0.0), (zero, 0.5), (nan_old, 0.5), (inf_old, 0.5), (negative, 0.5), (nan_word3, 1.0)):
        assert ref.state(1, new, o, h) == TAKEN
    # kept: any word of the new row, a NaN or an infinity of either sign
    for w in range(36):
        for bad in (np.nan, np.inf, -np.inf):
            poisoned = new.copy()
            poisoned[w] = bad
            assert ref.state(1, poisoned, old, 0.5) == KEPT, w
    # the order where two apply: skipped before kept, kept before taken (each way of being taken), taken before blended
    assert ref.state(0, nan_new, zero, 0.0) == SKIPPED and ref.state(0, new, old, 0.5) == SKIPPED
    for o, h in ((old, 0.0), (zero, 0.5), (nan_old, 0.5), (inf_old, 1.0)):
        assert ref.state(1, nan_new, o, h) == KEPT and ref.state(1, inf_new, o, h) == KEPT
    # ... and through the whole call: an entry out of range with a poisoned new row over a zeroed volume is skipped, and nothing is read or written
    grid = grid_of((2, 2, 2))
    sh = synthetic_sh(8, 3)
    got, _, state = ref.blend(grid, update_of(0.5), np.stack([nan_new, new, nan_new]), sh, indices=[8, 0xffffffff, 2])
    assert state.tolist() == [SKIPPED, SKIPPED, KEPT]
    assert_same_words(got, sh, "skipped and kept entries leave the volume alone")


def test_the_reference_against_float64_by_hand(ref):
    worst, cases = 0.0, 0
    for k, count in enumerate(GRIDS):
        grid = grid_of(count)
        for h in HYSTERESES + (0.25, 0.9990234375, 1.0e-3):
            for m in (0, 3):
                bins = m * m
                entries = list(range(grid.probes))
                sh, maps, new_sh, new_maps, flavours = synthetic_case(grid.probes, bins, entries, 10 * k + m)
                got_sh, got_maps, state = ref.blend(grid, update_of(h), new_sh, sh, new_maps, maps, n_list=grid.probes)
                for j, flavour in enumerate(flavours):
                    want_state = FLAVOUR_STATE[flavour] if h != 0.0 or FLAVOUR_STATE[flavour] == KEPT else TAKEN
                    assert state[j] == want_state, (flavour, h)
                    if state[j] == KEPT:
                        assert_same_rows(got_sh[j:j + 1], sh[j:j + 1], "kept")
                    elif state[j] == TAKEN:
                        assert_same_words(got_sh[j:j + 1], new_sh[j:j + 1], "taken")
                    else:
                        want = blend64(sh[j], new_sh[j], h)
                        scale = np.maximum(np.abs(sh[j]), np.abs(new_sh[j])).astype(np.float64)
                        some = scale > 0
                        worst = max(worst, float((np.abs(got_sh[j].astype(np.float64) - want)[some] / scale[some]).max()))
                        cases += int(some.sum())
                        if bins:
                            o, n, g = maps[j * bins:(j + 1) * bins], new_maps[j * bins:(j + 1) * bins], got_maps[j * bins:(j + 1) * bins]
                            both = np.isfinite(o).all(axis=1) & np.isfinite(n).all(axis=1)
                            want = blend64(o[both], n[both], h)
                            scale = np.maximum(np.abs(o[both]), np.abs(n[both])).astype(np.float64)
                            some = scale > 0
                            worst = max(worst, float((np.abs(g[both].astype(np.float64) - want)[some] / scale[some]).max()))
                            cases += int(some.sum())
    print("blend against float64: worst relative deviation %.3g over %d words" % (worst, cases))
    assert cases > 5000
    assert worst <= BLEND_BOUND, worst


def test_new_equal_to_old_keeps_its_bits_for_every_h(ref):
    rng = np.random.default_rng(6)
    words = np.concatenate([rng.normal(size=200) * np.exp2(rng.uniform(-120, 120, size=200)), [0.0, -0.0, 1.0e-45, -1.0e-45, 3.4e38, -3.4e38, 1.0, 12.566]]).astype(np.float32)
    for h in HYSTERESES:
        for w in words:
            got = ref.word(w, w, h)
            assert np.array([got]).view(np.uint32)[0] == np.array([w]).view(np.uint32)[0], (w, h)
    # ... a whole row with its map rows, through the call, whatever the state it ends in but KEPT-or-not makes no difference: the bits stay
    grid = grid_of((2, 2, 2))
    sh, maps = synthetic_sh(8, 5), synthetic_maps(8, 3, 5)
    sh[:, 20], maps[::5, 2] = -0.0, -0.0
    for h in HYSTERESES:
        got_sh, got_maps, state = ref.blend(grid, update_of(h), sh, sh, maps, maps, n_list=8)
        assert_same_rows(got_sh, sh, "h %g" % h)
        assert_same_rows(got_maps, maps, "h %g, maps" % h)
        assert (state == (TAKEN if h == 0.0 else BLENDED)).all()


def test_h_zero_is_the_new_bits_and_h_one_the_old(ref):
    grid = grid_of((3, 2, 4))
    sh, maps, new_sh, new_maps = synthetic_sh(24, 1), synthetic_maps(24, 3, 1), synthetic_sh(24, 2), synthetic_maps(24, 3, 2)
    maps[np.isnan(maps)], new_maps[np.isnan(new_maps)] = 1.0, 2.0
    got_sh, got_maps, state = ref.blend(grid, update_of(0.0), new_sh, sh, new_maps, maps, n_list=24)
    assert (state == TAKEN).all()
    assert_same_words(got_sh, new_sh, "h = 0")
    assert_same_words(got_maps, new_maps, "h = 0, maps")
    got_sh, got_maps, state = ref.blend(grid, update_of(1.0), new_sh, sh, new_maps, maps, n_list=24)
    assert (state == BLENDED).all()
    assert_same_words(got_sh, sh, "h = 1: old + (new - old) 0")
    assert_same_words(got_maps, maps, "h = 1, maps")


def test_repeated_blending_converges_monotonically(ref):
    grid = grid_of((2, 2, 2))
    start, target = synthetic_sh(8, 7), synthetic_sh(8, 8)
    for h in (0.5, 0.97):
        sh = start
        distance = np.abs(sh.astype(np.float64) - target)
        below = sh <= target
        for _ in range(1000 if h == 0.97 else 60):
            sh, _, state = ref.blend(grid, update_of(h), target, sh, n_list=8)
            assert (state == BLENDED).all()
            now = np.abs(sh.astype(np.float64) - target)
            assert (now <= distance).all() and ((sh <= target) == below)[now > 0].all()      # never further away, never across
            distance = now
        assert (distance <= 2.0e-5 * np.maximum(np.abs(target), 1.0e-3)).all()


def test_the_map_rows_exceptions(ref):
    old, new = np.array([0.5, 0.75, 1.5, 0.875], np.float32), np.array([0.25, 0.5, 1.25, 0.75], np.float32)
    half = np.array([0.375, 0.625, 1.375, 0.8125], np.float32)
    bad = [(w, v) for w in range(4) for v in (np.nan, np.inf, -np.inf)]
    assert ref.map_row(BLENDED, old, new, 0.5)[0] and np.array_equal(ref.map_row(BLENDED, old, new, 0.5)[1], half)
    assert np.array_equal(ref.map_row(TAKEN, old, new, 0.5)[1], new)
    for w, v in bad:
        poisoned_new, poisoned_old = new.copy(), old.copy()
        poisoned_new[w], poisoned_old[w] = v, v
        for state in (BLENDED, TAKEN):
            stored, row = ref.map_row(state, old, poisoned_new, 0.5)             # a new word that is not finite: the row keeps its old bits
            assert not stored and np.array_equal(row, old)
            stored, row = ref.map_row(state, poisoned_old, poisoned_new, 0.5)    # ... also where the old ones are no better
            assert not stored and np.array_equal(row.view(np.uint32), poisoned_old.view(np.uint32))
            stored, row = ref.map_row(state, poisoned_old, new, 0.5)             # an old word that is not finite: the new bits, also where the probe blends
            assert stored and np.array_equal(row, new)
    # ... and through the call: the flavour that holds both exceptions, and a kept probe whose map rows stay whatever they hold
    grid = grid_of((3, 2, 4))
    entries = list(range(24))
    for m in (2, 3, 8):
        bins = m * m
        sh, maps, new_sh, new_maps, flavours = synthetic_case(24, bins, entries, 0)
        got_sh, got_maps, state = ref.blend(grid, update_of(0.5), new_sh, sh, new_maps, maps, n_list=24)
        for j, flavour in enumerate(flavours):
            mine = slice(j * bins, (j + 1) * bins)
            if flavour == "blend_maps":
                assert state[j] == BLENDED
                assert_same_rows(got_maps[j * bins:j * bins + 1], maps[j * bins:j * bins + 1], "a NaN in the new row")
                assert_same_words(got_maps[(j + 1) * bins - 1:(j + 1) * bins], new_maps[(j + 1) * bins - 1:(j + 1) * bins], "an infinity in the old row")
                if 0 < bins // 2 < bins - 1:
                    at = j * bins + bins // 2
                    assert_same_rows(got_maps[at:at + 1], maps[at:at + 1], "both")
            if state[j] == KEPT:
                assert_same_rows(got_maps[mine], maps[mine], "a kept probe's maps")
                assert_same_rows(got_sh[j:j + 1], sh[j:j + 1], "a kept probe's row")


def test_the_calls_are_declared_exported_and_bound(ref):
    from flexlight_hip import capi
    header = open(os.path.join(ROOT, "include", "flexlight_hip_debug.h")).read()
    public = open(os.path.join(ROOT, "include", "flexlight_hip.h")).read()
    for name in CALLS:
        assert name in capi.EXPORTS and hasattr(capi.LIB, name) and name + "(" in header and name not in public, name
    for method in ("volume_positions_list", "volume_positions_list_device", "volume_blend", "volume_blend_device", "volume_update", "volume_update_device", "last_volume_update"):
        assert callable(getattr(capi.Context, method))
    # the library's host export is the reference's definition
    grid = grid_of((3, 2, 4))
    for h in HYSTERESES:
        sh, maps, new_sh, new_maps, _ = synthetic_case(24, 9, list(range(24)), 4)
        want_sh, want_maps, want_state = ref.blend(grid, update_of(h), new_sh, sh, new_maps, maps, n_list=24)
        for p in range(24):
            state, row, rows = capi.volume_blend_row_of(update_of(h), new_sh[p], sh[p], new_maps[p * 9:(p + 1) * 9], maps[p * 9:(p + 1) * 9])
            assert state == want_state[p]
            assert_same_rows(row.reshape(1, 36), want_sh[p:p + 1], "probe %d" % p)
            assert_same_rows(rows, want_maps[p * 9:(p + 1) * 9], "probe %d's maps" % p)
        state, row, rows = capi.volume_blend_row_of(update_of(h), new_sh[0], sh[0])
        assert rows is None and state == want_state[0]


def test_argument_rules_in_a_stand_alone_program_under_the_sanitizers(tmp_path):
    """every refusal of flx_volume_update_args.h and their order, the arithmetic list on either side of the grid's end and where a 32-bit product would wrap, every
    pairing of arrays: the header with a main of its own, built with -fsanitize=address,undefined, run directly"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is part of the image (the oracle is built with gcc)"
    exe = tmp_path / "volume_update_args"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "web-ray-tracer_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "volume_update_args_main.cc"), "-o", str(exe)])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) == ARGS_CASES
