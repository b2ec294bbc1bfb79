"""Helpers of the flx_scene_upload_device tests: the rules by which flx_scene_upload refuses an entry array, restated in plain numpy, and the scenes both test
files use."""
import copy

import numpy as np

from scene_update_util import TRIANGLE, by_hand

TRANSFORM, SKIP, TYPE = 0, 1, 2
MESSAGES = (
    "flx_scene_upload: transform number out of range",
    "flx_scene_upload: AABB skip count leaves the entry array",
    "flx_scene_upload: entry type is not 0, 1 or 2",
)
POINTER_MESSAGE = "flx_scene_upload_device: the arrays are not in memory of the context's device, 16-byte aligned"
FAST_BOX_BOUND = np.float32(5.764607523034235e17)                   # 2^59


def offences(geometry):
    """THE TABLE k_derive_check implements: {entry * 4 + rule} of every (entry, rule) that offends, by the host loop's tests (flx_scene.hip: flx_scene_upload): a
    live entry's transform number must lie in [0, 2^20); a box's skip count must be >= 0 and keep entry + skip inside the array; an entry that is no box must
    be a terminator or a triangle.  NaN fails every comparison, as in C."""
    g = np.ascontiguousarray(geometry, np.float32).reshape(-1, 12)
    n = g.shape[0]
    entry = np.arange(n)
    kind, skip, transform = g[:, 10], g[:, 6].astype(np.float64), g[:, 9]
    with np.errstate(invalid="ignore"):
        live = ~(kind == 0)
        bad_transform = live & ~((transform >= 0) & (transform < 1048576))
        bad_skip = (kind == 1) & (~(skip >= 0) | (entry + skip >= n))
        bad_type = live & ~(kind == 1) & ~(kind == 2)
    keys = set()
    keys.update(entry[bad_transform] * 4 + TRANSFORM)
    keys.update(entry[bad_skip] * 4 + SKIP)
    keys.update(entry[bad_type] * 4 + TYPE)
    return keys


def refusal(geometry):
    """the message of the FIRST offending entry and, within it, of the first rule in the host's order — the least key — or None"""
    keys = offences(geometry)
    return MESSAGES[min(keys) % 4] if keys else None


POSITIONS = (0, 64, 255, "last")
REFUSAL_ENTRIES = 300


def offend(g, at, rule):
    """entry `at` of g made to break `rule` (and no rule before it)"""
    n = g.shape[0]
    if rule == TRANSFORM:
        assert g[at, 10] != 0
        g[at, 9] = -1.0 if at % 2 else 1048576.0
    elif rule == SKIP:
        g[at, 10], g[at, 6] = 1.0, float(n - at) if at % 2 == 0 else -1.0
    else:
        g[at, 10] = 3.0


def scene_of(base, geometry, attributes):
    """`base` (its transforms, lights, atlases, camera) with these entries; ids: the triangle entries, as the flatten lists them"""
    g = np.ascontiguousarray(geometry, np.float32).reshape(-1, 12)
    a = np.ascontiguousarray(attributes, np.float32).reshape(-1, 28)
    assert g.shape[0] == a.shape[0]
    sc = copy.copy(base)
    sc.arrays = dict(base.arrays, geometry=g.reshape(-1).copy(), attributes=a.reshape(-1).copy(), ids=np.flatnonzero(g[:, 10] == 2).astype(np.int32))
    return sc


def decoy(scene):
    """the scene with one triangle for its entries: what a context holds before the upload under test replaces it"""
    g = np.zeros((2, 12), np.float32)
    g[0, :9], g[0, 10] = TRIANGLE, 2
    return scene_of(scene, g, np.zeros((2, 28), np.float32))


def rows(scene):
    return scene.arrays["geometry"].reshape(-1, 12).copy(), scene.arrays["attributes"].reshape(-1, 28).copy()


def one_triangle():
    """a scene of ONE entry, unpadded"""
    sc = by_hand([("tri", TRIANGLE)])
    g, a = rows(sc)
    return scene_of(sc, g[:1], a[:1])


def shifted(k):
    return [v + 0.5 * k for v in TRIANGLE]


def terminator_in_the_middle():
    """box, triangle, TERMINATOR, triangle, triangle: live entries behind a terminator (no walk reaches them; both copies still hold them)"""
    sc = by_hand([("box", 1, None), ("tri", shifted(0)), ("tri", shifted(1)), ("tri", shifted(2)), ("tri", shifted(3))])
    g, a = rows(sc)
    g[2], a[2] = 0, 0
    return scene_of(sc, g[:5], a[:5])


def last_box_reaches_the_end():
    """three entries, unpadded: the box's second link leaves the array (WALK_END)"""
    sc = by_hand([("box", 2, None), ("tri", shifted(0)), ("tri", shifted(1))])
    g, a = rows(sc)
    return scene_of(sc, g[:3], a[:3])


def fractional_words(base):
    """a skip count of 2.5 and a transform number of 1.5 (`base`: a scene with at least two transforms): both are truncated"""
    sc = by_hand([("box", 3, None), ("box", 2, None), ("tri", shifted(0)), ("tri", shifted(1)), ("tri", shifted(2))])
    g, a = rows(sc)
    g[1, 6] = 2.5
    g[3, 9] = 1.5
    g[4, 9] = 1.0
    return scene_of(base, g, a)


def overlapping_boxes():
    """six entries, two boxes that overlap without nesting: box 0 covers entries 1 .. 3, box 2 covers 3 .. 5"""
    wide = [-20, -20, 0, 20, 20, 20]
    sc = by_hand([("box", 3, wide), ("tri", shifted(0)), ("box", 3, wide), ("tri", shifted(1)), ("tri", shifted(2)), ("tri", shifted(3))])
    g, a = rows(sc)
    g[0, :6] = g[2, :6] = wide                                      # (as given, whatever a re-flatten made of them)
    return scene_of(sc, g[:6], a[:6])
