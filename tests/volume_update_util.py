"""Helpers of the volume-update tests (test_volume_update_cpu.py, test_volume_update_gpu.py, test_volume_update_seams_gpu.py, test_volume_update_js_gpu.py): the CPU
reference built once per session, synthetic resident and new rows that hold every state and both map-row exceptions, the lists of the blend tests, and a float64
restatement of include/flx_volume_update.h's blend written by hand."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "volume_update_ref"))
import flx_volume_update_ref  # noqa: E402

from probe_util import SPARE, assert_same_words, finished, poisoned  # noqa: E402,F401
from volume_map_util import assert_same_rows, map_of, synthetic_maps  # noqa: E402,F401
from volume_util import grid_of, synthetic_sh  # noqa: E402,F401

BLENDED, TAKEN, KEPT, SKIPPED = 0, 1, 2, 3
GRIDS = ((1, 1, 1), (2, 2, 2), (3, 2, 4))
MAP_SIZES = (None, 1, 3, 8, 9, 16)            # no maps; 1, 9, 64, 81 and 256 rows a probe: under a wave, exactly one pass, a partial second pass, four passes
HYSTERESES = (0.0, 0.5, 0.97, 1.0)
POISON = 0xA5A5A5A5
# what an entry's rows are made to hold, entry j getting FLAVOURS[j % len]; the state each must end in where 0 < h (h == 0: every blend is a take)
FLAVOURS = ("blend", "new_nan", "old_zero", "old_nan", "new_inf", "old_inf", "same", "old_negative", "blend_maps")
FLAVOUR_STATE = {"blend": BLENDED, "new_nan": KEPT, "old_zero": TAKEN, "old_nan": TAKEN, "new_inf": KEPT, "old_inf": TAKEN, "same": BLENDED, "old_negative": TAKEN,
                 "blend_maps": BLENDED}

_ref = []


def reference(tmp_path_factory):
    """the CPU reference, built once per session"""
    if not _ref:
        _ref.append(flx_volume_update_ref.build(str(tmp_path_factory.mktemp("volume_update_ref"))))
    return _ref[0]


def update_of(hysteresis, first=0, stride=1, reserved=0):
    from flexlight_hip import capi
    return capi.VolumeUpdate(hysteresis, first, stride, reserved)


def lists_of(probes, n_list, seed=0):
    """the lists of the blend tests for a grid of `probes` probes, each of n_list entries (fewer where the grid has fewer probes) ->
    [(name, indices uint32 or None, (first, stride))]: ascending, reversed, with entries out of range, and arithmetic"""
    n = min(n_list, probes)
    rng = np.random.default_rng(seed)
    some = np.sort(rng.choice(probes, size=n, replace=False)).astype(np.uint32)
    out = [("ascending", some, (0, 1)), ("reversed", some[::-1].copy(), (0, 1))]
    beyond = some.copy()
    beyond[::2] = (probes, 0xffffffff, probes + 7, 0x80000000, probes)[: len(beyond[::2])] if n else []
    out.append(("out_of_range", beyond, (0, 1)))
    stride = max(1, (probes - 1) // max(1, n - 1)) if n > 1 else 1
    first = (probes - 1) - (n - 1) * stride if n else 0
    out.append(("arithmetic", None, (first, stride)))
    return [(name, idx, fs, n) for name, idx, fs in out]


def entries_of(indices, first, stride, n):
    """the probes a list names, as Python ints (64 bits and more)"""
    return [int(x) for x in indices] if indices is not None else [first + j * stride for j in range(n)]


def synthetic_case(probes, bins, entries, seed):
    """Resident rows of a volume and new rows of a list that hold every FLAVOUR.
    -> (sh float32 [probes, 36], maps float32 [probes * bins, 4] or None, new_sh float32 [n, 36], new_maps float32 [n * bins, 4] or None, flavours [n])
    The resident rows are synthetic_sh's and synthetic_maps' (finite but for a NaN mean in every seventh probe's map row 1); the new ones the same with another
    seed.  Then entry j is made its flavour, where it names a probe of the grid:
      blend         as they are
      new_nan       a NaN in word (5 j) % 36 of the new SH row
      old_zero      the resident SH row zero-initialised, map rows too
      old_nan       a NaN in word (7 j) % 36 of the resident SH row
      new_inf       an infinity in the new row's word 35 (which a baked row keeps at 0.0)
      old_inf       +infinity in the resident row's word 3: > 0 and not finite
      same          the new rows' bits equal the resident ones', with a -0.0 among them
      old_negative  the resident row's word 3 negative
      blend_maps    both map-row exceptions: map row 0 has a NaN in its NEW row, the last map row an infinity in its OLD row; row bins // 2, where it is neither,
                    has both"""
    n = len(entries)
    sh, new_sh = synthetic_sh(probes, seed), synthetic_sh(max(n, 1), seed + 100)[:n]
    maps = synthetic_maps(probes, int(round(bins ** 0.5)), seed) if bins else None
    new_maps = synthetic_maps(max(n, 1), int(round(bins ** 0.5)), seed + 100)[:n * bins] if bins else None
    flavours = []
    for j, p in enumerate(entries):
        flavour = FLAVOURS[(j + seed) % len(FLAVOURS)]
        flavours.append(flavour)
        if p >= probes:
            continue
        mine = slice(p * bins, (p + 1) * bins)
        if flavour == "new_nan":
            new_sh[j, (5 * j) % 36] = np.nan
        elif flavour == "old_zero":
            sh[p] = 0.0
            if bins:
                maps[mine] = 0.0
        elif flavour == "old_nan":
            sh[p, (7 * j) % 36] = np.nan
        elif flavour == "new_inf":
            new_sh[j, 35] = -np.inf
        elif flavour == "old_inf":
            sh[p, 3] = np.inf
        elif flavour == "same":
            sh[p, 20] = -0.0
            new_sh[j] = sh[p]
            if bins:
                new_maps[j * bins:(j + 1) * bins] = maps[mine]
        elif flavour == "old_negative":
            sh[p, 3] = -sh[p, 3]
        elif flavour == "blend_maps" and bins:
            new_maps[j * bins, 2] = np.nan
            maps[p * bins + bins - 1, 0] = np.inf
            if 0 < bins // 2 < bins - 1:
                new_maps[j * bins + bins // 2, 1] = np.inf
                maps[p * bins + bins // 2, 3] = np.nan
    return sh, maps, new_sh, new_maps, flavours


def device_words(words, spare_words):
    """a host array as uint32 words on the device with spare_words of poison behind it"""
    import torch
    words = np.ascontiguousarray(words).view(np.uint32).reshape(-1)
    return torch.from_numpy(np.concatenate([words, np.full(spare_words, POISON, np.uint32)]).view(np.int32)).cuda()


def back(ctx, tensor, words, width):
    """a device array after the call -> its first `words` words as uint32 [.., width]: the spare words behind them kept their poison"""
    ctx.sync()
    got = tensor.cpu().numpy().view(np.uint32).reshape(-1)
    assert (got[words:] == POISON).all()
    return got[:words].reshape(-1, width)


def blend64(old, new, h):
    """the blend of finite float32 words restated by hand in float64: old + (new - old) (1 - h), h the float32 the call is given"""
    old, new = np.asarray(old, np.float64), np.asarray(new, np.float64)
    return old + (new - old) * (1.0 - float(np.float32(h)))
