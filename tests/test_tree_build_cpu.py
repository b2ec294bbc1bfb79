"""flx_tree_build_device without a GPU: the level-by-level formulation its kernels implement (csrc/flx_build.hip) — stable ranges of a permutation, ranks from flag
scans, entry indices from the scan of the nodes' range starts — restated in numpy (tree_build_util.level_build) and held against the host builder
(flx_mesh_import_obj + flx_mesh_flatten) on every soup the GPU test runs and on a committed asset: the same kinds, skip counts, transform numbers, row order and
ids.  Also that the fixtures reach the branch they are named for, and where the two calls are declared and bound."""
import os
import re

import numpy as np
import pytest

from tree_build_util import (SOUPS, TRANSFORM_OF, asset_text_in_triangles, block_of_text, case, entry_of_face, face_order_rows, level_build, soup_of_obj)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_level_build_equals(block, soup, transform=0):
    g, _, ids = block
    kind, skip, face, tri = level_build(soup)
    assert kind.size == g.shape[0]
    assert np.array_equal(kind, g[:, 10].astype(np.int64))                                     # word 10
    boxes = kind == 1
    assert np.array_equal(skip[boxes], g[boxes, 6].astype(np.int64))                            # word 6
    assert (g[:, 9] == transform).all()                                                         # word 9: the device copies row 0's
    assert np.array_equal(np.flatnonzero(face >= 0)[np.argsort(face[face >= 0])], entry_of_face(block, soup))      # the row order
    assert np.array_equal(tri, ids)


@pytest.mark.parametrize("name", sorted(SOUPS))
def test_the_level_by_level_formulation_builds_the_hosts_tree(name):
    soup, block, _ = case(name)
    assert_level_build_equals(block, soup, TRANSFORM_OF.get(name, 0))


def test_the_level_by_level_formulation_builds_the_hosts_tree_of_an_asset():
    text = asset_text_in_triangles("sphere")
    soup = soup_of_obj(text)
    assert soup.shape[0] > 256
    block = block_of_text(text)
    assert block[2].size == soup.shape[0]
    assert_level_build_equals(block, soup)


def leaves(g):
    """(entry, triangles) of every box that holds triangles directly"""
    out = []
    for e in np.flatnonzero(g[:, 10] == 1):
        inside = g[e + 1:e + 1 + int(g[e, 6])]
        if (inside[:, 10] == 2).all():
            out.append((int(e), inside.shape[0]))
    return out


def test_the_fixtures_reach_their_branches():
    g = case("n1")[1][0]
    assert g[:, 10].tolist() == [1, 2]
    assert case("n4")[1][0][:, 10].tolist() == [1, 2, 2, 2, 2]
    assert (case("n5")[1][0][:, 10] == 1).sum() > 1                                             # the first split
    assert case("thin")[1][0][:, 10].tolist() == [1] + [2] * 20                                 # no axis has room: a leaf of more than 4
    g = case("flat_sheet")[1][0]
    assert (g[g[:, 10] == 1, 2] == 0.25).all() and (g[g[:, 10] == 1, 5] == 0.25).all()
    g = case("chain")[1][0]
    assert g[:3, 10].tolist() == [1, 1, 1] and g[0, 6] == g[1, 6] + 1 == g[2, 6] + 2            # boxes that share their range's start
    assert leaves(case("duplicates")[1][0])[-1][1] == 9
    g = case("axis_tie")[1][0]
    assert g[:, 10].tolist() == [1] + [1, 2, 2, 2, 2] * 2 and (g[g[:, 10] == 2][:4, 2] >= 1).all()      # split on z: the first bucket holds z >= the centre
    g = case("many_chains")[1][0]
    assert (g[:, 10] == 1).sum() > (g[:, 10] == 2).sum() + 64                                   # more nodes than the device's node arrays start with (flx_scene.hip: n + 64)
    g = case("depth_limit")[1][0]
    deep = [(e, k) for e, k in leaves(g) if k > 4]
    assert deep and all(g[e, 3] - g[e, 0] > 1 / 128 for e, k in deep)                           # ended by the depth limit, not by its width
    g = case("centre_ties")[1][0]
    assert g[1, 10] == 1 and g[1, 2] == 2.0                                                     # (z, the last axis) a triangle whose min is the centre went into the first bucket


def test_the_two_calls_are_declared_beside_flx_scene_upload_device_and_bound():
    from flexlight_hip import capi
    text = open(os.path.join(ROOT, "include", "flexlight_hip_debug.h")).read()
    assert text.index("flx_status flx_scene_upload_device(") < text.index("flx_status flx_tree_build_device(") < text.index("flx_status flx_tree_emit_device(")
    boundary = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flexlight_hip.h")).read(), flags=re.S)
    assert "flx_tree_" not in boundary
    for name, arguments in (("flx_tree_build_device", 5), ("flx_tree_emit_device", 6)):
        assert name in capi.EXPORTS and len(getattr(capi.LIB, name).argtypes) == arguments
    assert hasattr(capi.Context, "build_tree_device")


def test_face_order_rows_are_the_soup():
    soup, block, rows = case("n257")
    assert np.array_equal(rows[0][:, :9].reshape(-1, 3, 3), soup) and (rows[0][:, 10] == 2).all() and (rows[0][:, 9] == 5).all()
    assert rows[1].shape == (257, 28)
