"""Helpers of the flx_scene_splice_device tests: the rule of the splice and its refusals restated in plain numpy, the flatten's layout of a graph of static blocks
(modules/scene.js:190-316) to hold the rule against, and the scenes both test files use."""
import functools

import numpy as np

import synth_scene
from scene_update_util import reflatten, reflatten_by_rule
from scene_upload_device_util import scene_of
from tree_build_util import host_block, random_soup

NO_PARENT = 0xffffffff
PARENT, DIRECT, CUT, IDS = 0, 1, 2, 3
MESSAGES = (
    "flx_scene_splice_device: parent_entry is not a box in front of first_entry whose range holds the replaced rows",
    "flx_scene_splice_device: a box between parent_entry and first_entry reaches first_entry (parent_entry is not the direct parent)",
    "flx_scene_splice_device: a box among the replaced rows reaches beyond them",
    "flx_scene_splice_device: the resident id list is not non-decreasing",
)
NO_SCENE_MESSAGE = "flx_scene_splice_device before flx_scene_upload"
NOTHING_MESSAGE = "flx_scene_splice_device: n_old and n_new are both 0"
POINTER_MESSAGE = "flx_scene_splice_device: an array is not in memory of the context's device, 16-byte aligned, or too short"
BEYOND_MESSAGE = "flx_scene_splice_device: the replaced rows leave the scene (first_entry + n_old lies beyond its last entry)"
SIZE_MESSAGE = "flx_scene_splice_device: the scene would have no entry, or more than 2^24"
NAN_MESSAGE = "flx_scene_splice_device: the uploaded scene has a NaN vertex (its boxes cannot be refitted as the flatten makes them)"


def rows12(geometry):
    return np.ascontiguousarray(geometry, np.float32).reshape(-1, 12)


def end_of(geometry):
    """1 + the last entry whose word 10 is not 0: the reference's textureLength"""
    live = np.flatnonzero(rows12(geometry)[:, 10] != 0)
    return int(live[-1]) + 1 if live.size else 0


def padded(entries):
    return (entries + 255) // 256 * 256


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------------------

def splice_rule(geometry, attributes, ids, first, n_old, parent, block=None, block_ids=True):
    """THE RULE flx_scene_splice_device implements -> (geometry [padded, 12], attributes [padded, 28], ids).  block: (geometry [n, 12], attributes [n, 28], ids
    relative to the block's first entry) or None: a removal; block_ids False: the block's ids are not handed over."""
    g, a = rows12(geometry), np.ascontiguousarray(attributes, np.float32).reshape(-1, 28)
    ids = np.asarray(ids, np.int64)
    end = end_of(g)
    bg, ba, bi = (np.zeros((0, 12), np.float32), np.zeros((0, 28), np.float32), np.zeros(0, np.int64)) if block is None else block
    n_new = bg.shape[0]
    delta = n_new - n_old
    assert first + n_old <= end and 0 < end + delta <= 1 << 24
    n = padded(end + delta)
    og, oa = np.zeros((n, 12), np.float32), np.zeros((n, 28), np.float32)
    og[:end + delta] = np.concatenate([g[:first], bg, g[first + n_old:end]])
    oa[:end + delta] = np.concatenate([a[:first], ba, a[first + n_old:end]])
    if parent != NO_PARENT:                                         # the parent and every box that holds it: in whole numbers, then back to float
        for j in range(parent + 1):
            if g[j, 10] == 1 and (j == parent or j + int(g[j, 6]) >= parent):
                og[j, 6] = np.float32(int(g[j, 6]) + delta)
    og = reflatten_by_rule(og)                                      # flx_scene_update's refit, over the whole array
    new_ids = np.concatenate([ids[ids < first], (np.asarray(bi, np.int64) + first) if block_ids else np.zeros(0, np.int64), ids[ids >= first + n_old] + delta])
    return og, oa, new_ids.astype(np.int32)


def offences(geometry, ids, first, n_old, parent):
    """THE TABLE k_splice_check implements: {entry * 4 + rule} of everything that offends in the resident scene.  Rule 0: the parent is no box, or its range
    (parent, parent + skip] does not hold the replaced rows (an insertion: first > parent + skip + 1); a parent that does not lie in front of `first` offends at
    entry `first`.  1: a box in front of `first` (behind the parent; anywhere with NO_PARENT) reaches `first`.  2: a box among the replaced rows reaches beyond them.
    3: an id lies below the one in front of it; it offends at the entry it names, held inside the array."""
    g = rows12(geometry)
    n = g.shape[0]
    ids = np.asarray(ids, np.int64)
    last = first + n_old
    entry = np.arange(n)
    box = g[:, 10] == 1
    reach = entry + np.where(box, g[:, 6].astype(np.int64), 0)
    keys = set()
    if parent != NO_PARENT:
        if parent >= first:
            keys.add(first * 4 + PARENT)
        elif not box[parent] or (last - 1 > reach[parent] if n_old else first > reach[parent] + 1):
            keys.add(parent * 4 + PARENT)
    between = box & (entry < first) & ((entry > parent) if parent != NO_PARENT else True) & (reach >= first)
    keys.update(entry[between] * 4 + DIRECT)
    cut = box & (entry >= first) & (entry < last) & (reach >= last)
    keys.update(entry[cut] * 4 + CUT)
    falls = np.flatnonzero(ids[1:] < ids[:-1]) + 1
    keys.update(np.clip(ids[falls], 0, n - 1) * 4 + IDS)
    return {int(k) for k in keys}


def refusal(geometry, ids, first, n_old, parent):
    """the message of the FIRST offending entry and, within it, of its first rule — the least key — or None"""
    keys = offences(geometry, ids, first, n_old, parent)
    return MESSAGES[min(keys) % 4] if keys else None


# ---- the flatten's layout of a graph of static items ----------------------------------------------------------------------------------------------------

def flatten_graph(item):
    """generateArraysFromGraph over a graph whose leaves are static items — (geometry, attributes, relative ids) blocks — and whose lists are boxes: a box row
    (skip count = the rows beneath it, transform 0, attribute row of zeros), then its items; a static item's ids are offset by its first entry.  The boxes' six
    floats by the flatten's own recursion over the children (scene_update_util.reflatten).  -> (geometry, attributes [padded], ids, {name: (first, rows)})"""
    geo, att, ids, where = [], [], [], {}

    def fill(it):
        if isinstance(it, list):
            at = len(geo)
            geo.append(np.zeros(12, np.float32))
            att.append(np.zeros(28, np.float32))
            for child in it:
                fill(child)
            geo[at][6], geo[at][10] = len(geo) - at - 1, 1
            return
        name, (g, a, i) = it
        where[name] = (len(geo), g.shape[0])
        ids.extend(int(k) + len(geo) for k in i)
        geo.extend(np.array(g, np.float32))
        att.extend(np.array(a, np.float32))

    fill(item)
    n = len(geo)
    g, a = np.zeros((padded(n), 12), np.float32), np.zeros((padded(n), 28), np.float32)
    g[:n], a[:n] = np.array(geo), np.array(att)
    return reflatten(g), a, np.array(ids, np.int32), where


@functools.lru_cache(maxsize=None)
def mesh(n, seed):
    """the host builder's block of a seeded soup of n triangles, in view of synth_scene's camera"""
    block = host_block(random_soup(n, seed, centre=(0.0, 0.0, 8.0), extent=3.0, size=0.8))
    for x in block:
        x.setflags(write=False)
    return block


def triangles(n, seed):
    """a block of n bare triangle rows (no box): any row count"""
    g, a, _ = mesh(max(n, 5), seed)
    at = np.flatnonzero(g[:, 10] == 2)[:n]
    return g[at].copy(), a[at].copy(), np.arange(n, dtype=np.int32)


# ---- the scene of the GPU tests -------------------------------------------------------------------------------------------------------------------------

W, H = 64, 48


@functools.lru_cache(maxsize=None)
def base_scene():
    """synth_scene.make_sized(200, 1) with, appended inside its root box, W [ V [ A, B, C ], U [ D ] ], a mesh F and a single triangle E:
    -> (scene, {name: (first, rows)}, {box name: entry}).  B lies three boxes deep (V, W, the root), D is the only child of U, E is a tail of one row."""
    sized = synth_scene.make_sized(200, 1, seed=3, width=W, height=H)
    g, a = sized.arrays["geometry"].reshape(-1, 12), sized.arrays["attributes"].reshape(-1, 28)
    assert end_of(g) == 200 and g[0, 10] == 1 and g[0, 6] == 199
    inner = [("old", (g[1:200], a[1:200], np.flatnonzero(g[1:200, 10] == 2))),
             [[("A", mesh(40, 31)), ("B", mesh(23, 32)), ("C", mesh(9, 33))], [("D", mesh(14, 34))]], ("F", mesh(30, 35)), ("E", triangles(1, 36))]
    fg, fa, ids, where = flatten_graph(inner)
    scene = scene_of(sized, fg, fa)
    assert np.array_equal(scene.arrays["ids"], ids)
    w = 200
    v = w + 1
    u = where["D"][0] - 1
    assert fg[w, 10] == fg[v, 10] == fg[u, 10] == 1 and v + fg[v, 6] == u - 1 and fg[u, 6] == where["D"][1]
    return scene, where, {"root": 0, "W": w, "V": v, "U": u}


def with_arrays(scene, geometry, attributes, ids):
    """the scene with these entries and THIS id list"""
    sc = scene_of(scene, geometry, attributes)
    sc.arrays["ids"] = np.ascontiguousarray(ids, np.int32)
    return sc
