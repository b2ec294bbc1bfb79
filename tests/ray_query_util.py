"""Helpers of the ray query tests (test_ray_query_cpu.py, test_ray_query_gpu.py, test_ray_query_js_gpu.py): ray rows and hit rows as flx_rays_cast lays them out
(include/flexlight_hip_debug.h, "ray queries"), and the oracle's walks of a scene's rays, computed once per scene."""
import numpy as np

CLOSEST, OCCLUDED, COUNT = 1, 2, 4          # FLX_RAYS_*
EVERY_WHAT = (1, 2, 3, 5, 6, 7)


def pack_rays(rays7):
    """[n, 7] float32 (origin, direction, l), flx_debug_walk's rows -> [n, 8] float32 ray rows (origin, l, direction, a word nobody reads)"""
    rays7 = np.ascontiguousarray(rays7, np.float32).reshape(-1, 7)
    rows = np.zeros((rays7.shape[0], 8), np.float32)
    rows[:, 0:3], rows[:, 3], rows[:, 4:7] = rays7[:, 0:3], rays7[:, 6], rays7[:, 3:6]
    rows[:, 7] = np.float32(-123.0)
    return rows


def pack_hits(suv, entry, transform2, occluded, visits_closest, visits_shadow):
    """hit rows uint8 [n, 32] from the six columns"""
    n = len(entry)
    words = np.zeros((n, 8), np.uint32)
    words[:, 0:3] = np.ascontiguousarray(suv, np.float32).reshape(n, 3).view(np.uint32)
    words[:, 3] = np.asarray(entry, np.int32).view(np.uint32)
    words[:, 4] = np.asarray(transform2, np.int32).view(np.uint32)
    words[:, 5] = np.asarray(occluded, np.int32).view(np.uint32)
    words[:, 6] = np.asarray(visits_closest, np.uint32)
    words[:, 7] = np.asarray(visits_shadow, np.uint32)
    return words.view(np.uint8).reshape(n, 32)


def words_of(hits):
    """hit rows (uint8 [n, 32], numpy or torch) -> uint32 [n, 8]"""
    if not isinstance(hits, np.ndarray):
        hits = hits.detach().cpu().numpy()
    return np.ascontiguousarray(hits, np.uint8).reshape(-1, 32).view(np.uint32)


def expected_words(want_suv, want, what):
    """the hit rows a query with `what` must write, uint32 [n, 8], from the oracle's walks in test_walk_lds_gpu.oracle_walks' form (suv float32 [n, 3]; [n, 8]:
    -, -, -, 2 x transform, entry, closest-hit visits, shadowed, shadow visits): (s, u, v) as the oracle's bits where it hits; zeros and -1 at a miss and for a
    walk not asked for; visits only with COUNT"""
    n = want.shape[0]
    closest, occluded, count = bool(what & CLOSEST), bool(what & OCCLUDED), bool(what & COUNT)
    hit = (want[:, 4] != -1) & closest
    words = np.zeros((n, 8), np.uint32)
    words[hit, 0:3] = np.ascontiguousarray(want_suv, np.float32).view(np.uint32)[hit]
    words[:, 3] = np.where(hit, want[:, 4], -1).astype(np.int32).view(np.uint32)
    words[:, 4] = np.where(hit, want[:, 3], 0).astype(np.int32).view(np.uint32)
    if occluded:
        words[:, 5] = want[:, 6].astype(np.uint32)
    if count and closest:
        words[:, 6] = want[:, 5].astype(np.uint32)
    if count and occluded:
        words[:, 7] = want[:, 7].astype(np.uint32)
    return words


def same_rows(got, want, nan_equal=False):
    """bool per row: uint32 [n, 8] against uint32 [n, 8]; nan_equal: a NaN in s, u or v equals any NaN (the sign and payload of a NaN an invalid operation makes
    differ between the CPU's and the GPU's arithmetic: tests/intersect_edges_util.same_walks)"""
    same = got == want
    if nan_equal:
        nan = lambda b: (b & 0x7fffffff) > 0x7f800000
        same[:, 0:3] |= nan(got[:, 0:3]) & nan(want[:, 0:3])
    return same.all(axis=1)


def debug_walk_columns(hits):
    """hit rows -> flx_debug_walk's [n, 8] float32 (s, u, v, 2 x transform, entry, closest-hit visits, shadowed, shadow visits)"""
    w = words_of(hits)
    out = np.zeros((w.shape[0], 8), np.float32)
    out[:, 0:3] = w[:, 0:3].view(np.float32)
    out[:, 3], out[:, 4] = w[:, 4].view(np.int32), w[:, 3].view(np.int32)
    out[:, 5], out[:, 6], out[:, 7] = w[:, 6], w[:, 5].view(np.int32), w[:, 7]
    return out


_walks = {}


def scene_walks(oracle, entries, n_transforms):
    """(scene, rays [2160, 7], the oracle's suv, the oracle's [2160, 8]) of synth_scene.make_sized(entries, T): test_walk_lds_gpu's scenes, rays and oracle calls,
    made once per scene"""
    from test_walk_lds_gpu import make_rays, oracle_walks, sized
    key = (entries, n_transforms)
    if key not in _walks:
        sc = sized(entries, n_transforms)
        rays = make_rays(sc, set(), seed=entries + n_transforms)
        suv, want = oracle_walks(oracle, sc, rays)
        assert rays.shape[0] == 2160
        assert (want[:, 4] != -1).mean() > 0.3 and want[:, 6].mean() > 0.05, ((want[:, 4] != -1).mean(), want[:, 6].mean())      # the conditions on the inputs
        _walks[key] = (sc, rays, suv, want)
    return _walks[key]
