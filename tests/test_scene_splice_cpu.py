"""flx_scene_splice_device without a GPU: the rule of the splice, restated in numpy (scene_splice_util.splice_rule), held against the flatten itself — two graphs
of static blocks laid out as generateArraysFromGraph lays them out, the rule taking one into the other bit for bit —, the refusal table, and the exports."""
import os
import re

import numpy as np
import pytest

from scene_splice_util import (CUT, DIRECT, IDS, MESSAGES, NO_PARENT, PARENT, base_scene, end_of, flatten_graph, mesh, offences, refusal, splice_rule, triangles)
from scene_update_util import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

A, B, C, D = ("A", mesh(40, 31)), ("B", mesh(23, 32)), ("C", mesh(57, 33)), ("D", mesh(9, 34))


def assert_arrays_equal(got, want):
    for name, x, y in zip(("geometry", "attributes", "ids"), got, want):
        assert x.shape == y.shape, name
        if name == "ids":
            assert np.array_equal(x, y)
        else:
            bad = np.flatnonzero((bits(x) != bits(y)).reshape(x.shape[0], -1).any(axis=1))
            assert bad.size == 0, "%s: rows %s differ: %s vs %s" % (name, bad[:8], x[bad[0]], y[bad[0]])


# ---- the rule against the flatten ---------------------------------------------------------------------------------------------------------------------------

def test_a_replaced_block_gives_the_flatten_of_the_other_graph():
    g, a, ids, where = flatten_graph([A, B])
    first, rows = where["B"]
    assert_arrays_equal(splice_rule(g, a, ids, first, rows, 0, C[1]), flatten_graph([A, C])[:3])
    assert_arrays_equal(splice_rule(g, a, ids, *where["A"], 0, D[1]), flatten_graph([D, B])[:3])      # the first child, by a smaller one: the tail moves down


def test_a_removed_block_gives_the_flatten_without_it():
    g, a, ids, where = flatten_graph([A, B, C])
    assert_arrays_equal(splice_rule(g, a, ids, *where["B"], 0), flatten_graph([A, C])[:3])
    assert_arrays_equal(splice_rule(g, a, ids, *where["C"], 0), flatten_graph([A, B])[:3])


def test_a_block_appended_to_the_root_gives_the_flatten_with_it():
    g, a, ids, _ = flatten_graph([A, B])
    end = end_of(g)
    assert end == 1 + g[0, 6]
    assert_arrays_equal(splice_rule(g, a, ids, end, 0, 0, C[1]), flatten_graph([A, B, C])[:3])
    assert_arrays_equal(splice_rule(g, a, ids, 1, 0, 0, C[1]), flatten_graph([C, A, B])[:3])          # .. and in front of its first child


def test_two_boxes_deep_both_ancestors_grow():
    g, a, ids, where = flatten_graph([A, [B, D], C])
    want = flatten_graph([A, [B, C], C])
    inner = where["B"][0] - 1
    assert g[inner, 10] == 1 and g[inner, 6] == where["B"][1] + where["D"][1]
    got = splice_rule(g, a, ids, *where["D"], inner, C[1])
    assert_arrays_equal(got, want[:3])
    delta = C[1][0].shape[0] - D[1][0].shape[0]
    assert got[0][0, 6] == g[0, 6] + delta and got[0][inner, 6] == g[inner, 6] + delta
    assert got[0].shape[0] > g.shape[0]                              # (this one carries the array over a multiple of 256)


def test_at_top_level_no_box_grows():
    g, a, ids, _ = flatten_graph([A, B])
    end = end_of(g)
    og, oa, oids = splice_rule(g, a, ids, end, 0, NO_PARENT, D[1])
    assert og[0, 6] == g[0, 6] and (bits(og[:end]) == bits(g[:end])).all()
    assert (bits(og[end:end + D[1][0].shape[0]]) == bits(D[1][0])).all() and np.array_equal(oids, np.concatenate([ids, D[1][2] + end]))


def test_a_block_without_ids_and_an_emptied_parent():
    g, a, ids, where = flatten_graph([A, [D]])
    inner = where["D"][0] - 1
    og, _, oids = splice_rule(g, a, ids, *where["D"], inner)
    assert og[inner, 10] == 1 and og[inner, 6] == 0 and (bits(og[inner, :6]) == bits(g[inner, :6])).all()      # it stays, and keeps its six floats
    assert np.array_equal(oids, ids[ids < inner])
    _, _, oids = splice_rule(g, a, ids, 1, 0, 0, B[1], block_ids=False)
    assert np.array_equal(oids, np.concatenate([ids[:0], ids + B[1][0].shape[0]]))


# ---- the refusals ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nested():
    return flatten_graph([A, [B, [D]], C])


def test_a_proper_splice_offends_nothing(nested):
    g, _, ids, where = nested
    inner = where["B"][0] - 1
    assert offences(g, ids, *where["B"], inner) == set()
    assert offences(g, ids, inner, 1 + int(g[inner, 6]), 0) == set()                  # the inner box with everything in it
    assert offences(g, ids, end_of(g), 0, 0) == set() and offences(g, ids, end_of(g), 0, NO_PARENT) == set()
    assert offences(g, ids, 1, 0, 0) == set() and offences(g, ids, where["C"][0], 0, 0) == set()
    assert offences(g, ids, inner + 1 + int(g[inner, 6]), 0, inner) == set()         # appended to the inner box


def test_each_rule_names_its_entry(nested):
    g, _, ids, where = nested
    inner, innermost = where["B"][0] - 1, where["D"][0] - 1
    b, d, c = where["B"], where["D"], where["C"]
    # (a) the parent: a triangle; a box whose range ends in front of the rows; one that does not lie in front of them; an insertion beyond its end
    triangle = int(np.flatnonzero(g[:b[0], 10] == 2)[-1])
    assert min(offences(g, ids, *b, triangle)) == triangle * 4 + PARENT
    assert offences(g, ids, *c, inner) == {inner * 4 + PARENT}
    assert min(offences(g, ids, *b, c[0])) == b[0] * 4 + PARENT
    assert offences(g, ids, end_of(g), 0, inner) == {inner * 4 + PARENT}
    # (b) the root given for rows the inner box holds; no parent given for rows inside the root
    assert offences(g, ids, *d, inner) == {innermost * 4 + DIRECT}
    assert offences(g, ids, *b, 0) == {inner * 4 + DIRECT}
    assert offences(g, ids, *d, NO_PARENT) == {0 * 4 + DIRECT, inner * 4 + DIRECT, innermost * 4 + DIRECT}
    # (c) rows that begin with a box and end inside it
    cut = offences(g, ids, inner, 3, 0)                             # (the inner box, and B's own boxes behind it)
    assert min(cut) == inner * 4 + CUT and {k % 4 for k in cut} == {CUT}
    assert refusal(g, ids, b[0], b[1] - 1, inner) == MESSAGES[CUT]
    # (d) the ids
    swapped = ids.copy()
    swapped[[4, 5]] = swapped[[5, 4]]
    assert offences(g, swapped, *b, inner) == {int(ids[4]) * 4 + IDS}
    wild = ids.copy()
    wild[3] = -7
    assert min(offences(g, wild, *b, inner)) == 0 * 4 + IDS


def test_of_two_offenders_the_first_entry_and_its_first_rule_are_reported(nested):
    g, _, ids, where = nested
    inner, innermost = where["B"][0] - 1, where["D"][0] - 1
    # the root as the parent of rows [inner, inner + 3): the rows cut the inner box (c); with a triangle as the parent, that comes first (a)
    triangle = int(np.flatnonzero(g[:inner, 10] == 2)[0])
    keys = offences(g, ids, inner, 3, triangle)
    assert {triangle * 4 + PARENT, inner * 4 + CUT} <= keys and min(keys) == triangle * 4 + PARENT and refusal(g, ids, inner, 3, triangle) == MESSAGES[PARENT]
    # ids out of order at a late entry and a wrong parent at an early one; ids out of order at an early entry and a cut box at a late one
    late = ids.copy()
    late[[-1, -2]] = late[[-2, -1]]
    assert refusal(g, late, *where["D"], inner) == MESSAGES[DIRECT]
    early = ids.copy()
    early[[0, 1]] = early[[1, 0]]
    assert refusal(g, early, innermost, 2, inner) == MESSAGES[IDS]


def test_the_gpu_tests_scene_is_what_it_says():
    scene, where, box = base_scene()
    g = scene.arrays["geometry"].reshape(-1, 12)
    assert end_of(g) == where["E"][0] + 1 == 1 + g[0, 6]
    assert offences(g, scene.arrays["ids"], *where["B"], box["V"]) == set()
    assert offences(g, scene.arrays["ids"], *where["D"], box["U"]) == set()
    assert refusal(g, scene.arrays["ids"], *where["B"], box["W"]) == MESSAGES[DIRECT]


# ---- the exports ----------------------------------------------------------------------------------------------------------------------------------------------

def test_the_library_exports_and_the_headers_declare_it():
    from flexlight_hip import capi
    assert "flx_scene_splice_device" in capi.EXPORTS and hasattr(capi.LIB, "flx_scene_splice_device")
    assert hasattr(capi.Context, "splice_scene_device") and hasattr(capi.Context, "replace_mesh_device")
    assert capi.NO_PARENT == NO_PARENT
    with open(os.path.join(ROOT, "include", "flexlight_hip_debug.h")) as f:
        text = f.read()
    assert text.index("flx_status flx_tree_emit_device(") < text.index("flx_status flx_scene_splice_device(") < text.index("flx_status flx_debug_scene_read(")
    assert re.search(r"#define FLX_NO_PARENT 0xffffffffu", text)
    declaration = re.sub(r"/\*.*?\*/", "", text[text.index("flx_status flx_scene_splice_device("):].split(";")[0], flags=re.S)
    arguments = [x.strip() for x in declaration[declaration.index("(") + 1:declaration.rindex(")")].split(",")]
    assert arguments[0] == "flx_context *ctx" and len(arguments) == 1 + 9
    with open(os.path.join(ROOT, "include", "flexlight_hip.h")) as f:
        assert "flx_scene_splice_device" not in f.read()
