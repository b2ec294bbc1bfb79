"""Volume updates across their seams (include/flexlight_hip_debug.h, "volume updates"): the blend and the positions of 32 769 entries of a 33 x 32 x 32 grid, m = 1 —
8 193 workgroups of k_volume_blend, the last one a single wave; 129 of k_volume_positions_list, the last one a single lane —, whose resident rows past 32 768 are
written.  NEITHER KERNEL'S LAUNCH IS CUT (n_list stays below 2^31 and both grids are one-dimensional), so there is no cut to cross but the 32 768 at which the sibling
kernels cut theirs: a library that cut there and lost the entry behind it, or that named a probe with 16 bits, fails here.  Synthetic rows against the CPU
reference's bits."""
import numpy as np
import pytest
import torch

from volume_update_util import (BLENDED, KEPT, POISON, SKIPPED, SPARE, TAKEN, assert_same_words, back, device_words, grid_of, map_of, reference, synthetic_maps, synthetic_sh,
                                update_of)

pytestmark = pytest.mark.gpu

GRID = (33, 32, 32)     # 33 792 probes: test_probe_seams_gpu.py's grid
ENTRIES = 32769


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return reference(tmp_path_factory)


@pytest.fixture(scope="module")
def rows():
    """-> (resident SH rows, resident map rows, new SH rows, new map rows) of the whole grid and of 32 769 entries, with every state among them: every 11th new row
    holds a NaN, every 13th resident row is zero-initialised"""
    probes = GRID[0] * GRID[1] * GRID[2]
    sh, maps, new_sh, new_maps = synthetic_sh(probes, 1), synthetic_maps(probes, 1, 1), synthetic_sh(ENTRIES, 2), synthetic_maps(ENTRIES, 1, 2)
    new_sh[::11, 9] = np.nan
    sh[::13], maps[::13] = 0.0, 0.0
    return sh, maps, new_sh, new_maps


@pytest.mark.parametrize("listed", (False, True))
def test_32769_entries(hip, ref, rows, listed):
    grid, vmap = grid_of(GRID), map_of(1, 5)
    probes = grid.probes
    sh, maps, new_sh, new_maps = rows
    if listed:                                           # a permutation's first 32 769 entries, every 1000th out of range
        indices = np.random.default_rng(3).permutation(probes)[:ENTRIES].astype(np.uint32)
        indices[::1000] = probes + np.arange(len(indices[::1000]), dtype=np.uint32)
        update = update_of(0.97)
    else:                                                # the last 32 769 probes: entry 32 768 names probe 33 791
        indices, update = None, update_of(0.97, probes - ENTRIES, 1)
    want_sh, want_maps, want_state = ref.blend(grid, update, new_sh, sh, new_maps, maps, indices, ENTRIES)
    assert set(want_state.tolist()) == ({BLENDED, TAKEN, KEPT, SKIPPED} if listed else {BLENDED, TAKEN, KEPT})
    d_sh, d_maps, d_state = device_words(sh, SPARE * 36), device_words(maps, SPARE * 4), device_words(np.full(ENTRIES, POISON, np.uint32), SPARE)
    d_indices = device_words(indices, 0) if listed else None
    torch.cuda.synchronize()
    hip.volume_blend_device(grid, vmap, update, device_words(new_sh, 0), d_sh, device_words(new_maps, 0), d_maps, d_indices, ENTRIES, state=d_state)
    got_sh = back(hip, d_sh, probes * 36, 36)
    assert_same_words(got_sh, want_sh, "32 769 entries")
    assert_same_words(back(hip, d_maps, probes * 4, 4), want_maps, "32 769 entries, maps")
    assert back(hip, d_state, ENTRIES, 1).reshape(-1).tolist() == want_state.tolist()
    changed = (got_sh != sh.view(np.uint32)).any(axis=1)
    assert changed[32768:].sum() > 500                   # resident rows past 32 768 are written
    assert hip.last_volume_update() == {"entries": ENTRIES, "groups": 8193, "size": 1, "listed": int(listed), "chunks": 0, "fused": 0}
    # the positions of the same list: the last entry is the one lane of the last workgroup
    want = ref.positions(grid, update, indices, ENTRIES)
    out = device_words(np.full((ENTRIES, 4), POISON, np.uint32), SPARE * 4)
    torch.cuda.synchronize()
    hip.volume_positions_list_device(grid, update, d_indices, ENTRIES, out=out)
    assert_same_words(back(hip, out, ENTRIES * 4, 4), want, "32 769 positions")
