"""CPU side of the box test's single-comparison form (csrc/flx_device.h: rayCuboidInterval<true>; DeviceScene::walk_thick_boxes):

- flx_scene_upload's scan for flat boxes, through flx_debug_boxes_thick (the library loads without a GPU): thick, flat per axis, min > max, NaN;
- the rows tests/test_box_single_gpu.py puts through the device land in every outcome of the form — surely hit, surely missed, not sure — and wherever the form,
  restated in numpy one float32 operation at a time, is sure, it says what the oracle's rayCuboid says: on the built rows and on every bounded row of the
  committed edge table."""
import gzip
import json
import os

import numpy as np
import pytest

from box_single_util import (OHI, bounded_rows, direction_rows, flat_rows, flattened, graze_rows, half_flat_scene, nan_corner_rows, on_face_rows,
                             oracle_ray_cuboid, short_l_rows, single_form_outcome, thick_numpy, thick_scene)
from flexlight_hip import capi

HERE = os.path.dirname(os.path.abspath(__file__))


def _box(mn, mx, skip=1.0):
    g = np.zeros(12, np.float32)
    g[0:3], g[3:6], g[6], g[10] = mn, mx, skip, 1
    return g


def _tri(v):
    g = np.zeros(12, np.float32)
    g[0:9], g[10] = v, 2
    return g


def test_thickness_of_an_entry_array():
    """every box row must have min < max on all three axes; triangle rows and terminators do not count"""
    tri = _tri([0, 0, 0, 0, 0, 0, 0, 0, 0])                              # (a degenerate triangle is no box)
    thick = [_box([-1, -2, -3], [1, 2, 3], 2), tri, tri, np.zeros(12, np.float32)]
    assert capi.boxes_thick(np.array(thick)) == 1
    assert capi.boxes_thick(np.array([tri, np.zeros(12, np.float32)])) == 1        # no box at all
    assert capi.boxes_thick(np.zeros((0, 12), np.float32)) == 1
    for axis in range(3):
        for position in (0, 2):                                        # the first and the last box of the array
            for what, (lo, hi), want in (("flat", (0.5, 0.5), 0), ("flat at zero", (0.0, 0.0), 0), ("zeros of both signs", (-0.0, 0.0), 0), ("min > max", (0.5, 0.25), 0),
                                         ("one step of room", (0.5, np.nextafter(np.float32(0.5), np.float32(1))), 1), ("NaN min", (np.nan, 1.0), 0),
                                         ("NaN max", (-1.0, np.nan), 0), ("infinite", (-np.inf, np.inf), 1), ("both +inf", (np.inf, np.inf), 0)):
                rows = [_box([-1, -2, -3], [1, 2, 3], 3), tri, _box([-1, -1, -1], [1, 1, 1], 1), tri]
                rows[position][axis], rows[position][3 + axis] = lo, hi
                g = np.array(rows)
                assert capi.boxes_thick(g) == want == thick_numpy(g), (axis, position, what)
    # a triangle's coordinates may be anything
    rows = [_box([-1, -2, -3], [1, 2, 3], 1), _tri([np.nan] * 9)]
    assert capi.boxes_thick(np.array(rows)) == 1
    # a kind that is no box (the upload refuses it elsewhere) is not looked at
    odd = _box([1, 1, 1], [0, 0, 0])
    odd[10] = 3
    assert capi.boxes_thick(np.array([odd])) == 1


def test_thickness_of_the_scenes_the_gpu_tests_use(scenes):
    g = scenes("dragon").arrays["geometry"]
    assert capi.boxes_thick(g) == 1 == thick_numpy(g)                    # the flagship scene: 28 803 boxes, none flat
    assert capi.boxes_thick(thick_scene().arrays["geometry"]) == 1
    half = half_flat_scene().arrays["geometry"].reshape(-1, 12)
    boxes = half[half[:, 10] == 1]
    flat = (boxes[:, 0:3] == boxes[:, 3:6]).any(axis=1)
    assert boxes.shape[0] == 13 and flat.sum() == 6 and not flat[0]       # half of the twelve leaves, two per axis; the root is thick
    assert [(boxes[flat][:, a] == boxes[flat][:, 3 + a]).sum() for a in range(3)] == [2, 2, 2]
    assert capi.boxes_thick(half) == 0
    sc, first, rows = flattened(thick_scene(), 5)
    assert capi.boxes_thick(sc.arrays["geometry"]) == 0 and first == 16 and rows.shape == (3, 12)


def test_the_built_rows_land_in_every_outcome_and_a_sure_answer_is_the_oracles(oracle):
    families = {"graze": graze_rows(), "flat": flat_rows(), "on_face": on_face_rows(), "short_l": short_l_rows(), "direction": direction_rows()}
    for name, (rows, classes) in families.items():
        assert len(rows) == len(classes) and np.all(np.abs(rows[:, 7:13]) <= OHI), name
        want = oracle_ray_cuboid(oracle, rows)
        outcome = np.array([single_form_outcome(r) for r in rows])
        for k in np.flatnonzero(outcome != "unsure"):
            assert (outcome[k] == "true") == bool(want[k]), (name, classes[k], rows[k].tolist())
        if name == "graze":
            # tmax - tmin of 0, 1, 2, 4 steps (at most 4 x 2^-23 = 0.5 x 2^-20 relative, and 0.375 x 2^-20 of rounding): inside the tolerance, never sure though the box
            # is hit or missed; 8 steps are 0.5 .. 1 x 2^-20, on the border, either; beyond 2^-20 on either side: sure
            for k, c in enumerate(classes):
                if ("_ulp" in c and "8_ulp" not in c) or "under_2^-20" in c:
                    assert outcome[k] == "unsure", c
                if "over_2^-20" in c or "over_2^-19" in c:
                    assert outcome[k] == ("true" if c.startswith("graze +") else "false"), c
            assert {"true", "false", "unsure"} <= set(outcome)
            assert any(outcome[k] == "true" for k, c in enumerate(classes) if c == "graze +over_2^-19")
            assert any(outcome[k] == "false" for k, c in enumerate(classes) if c == "graze -over_2^-19")
            assert 0 < want.sum() < len(want)
        if name == "flat":
            crossed = np.array(["crossed" in c and "long" in c for c in classes])
            assert want[crossed].all() and set(outcome[crossed]) == {"unsure"}        # a flat box that is hit always takes the exact quotients
            assert "false" in set(outcome[~crossed]) and not want[np.array(["missed" in c for c in classes])].any()
        if name == "short_l":
            below = np.array([float(np.float32(r[0])) < 2.0 ** -60 for r in rows])
            assert set(outcome[below]) == {"unsure"} and (outcome[~below] != "unsure").any()
        if name == "direction":
            assert (outcome == "unsure").sum() >= 60 and (outcome != "unsure").sum() >= 12      # (2^-60 and 2^60 themselves are in range)
    rows, classes = nan_corner_rows()
    assert len(rows) == 24 and all(np.isnan(r[7:13]).sum() == 1 for r in rows)


def test_on_the_edge_table_a_sure_answer_is_the_literal_one():
    """tests/golden/intersect_edge_kat.json.gz, every row whose box keeps the bound: where the single-comparison form is sure it gives the literal answer, and it is sure
    of most rows outside the band while every row of the classes made of flat boxes that are hit stays unsure"""
    kat = json.load(gzip.open(os.path.join(HERE, "golden", "intersect_edge_kat.json.gz"), "rt"))["ray_cuboid"]
    rows = np.array([r[0:13] for r in kat], np.uint32).view(np.float32)
    with np.errstate(invalid="ignore"):
        keep = np.all(np.abs(rows[:, 7:13]) <= OHI, axis=1)
    sure = wrong = 0
    per_class = {}
    for k in np.flatnonzero(keep):
        outcome = single_form_outcome(rows[k])
        stats = per_class.setdefault(kat[k][14], [0, 0])
        stats[1] += 1
        if outcome != "unsure":
            sure += 1
            stats[0] += 1
            wrong += (outcome == "true") != bool(kat[k][13])
    assert wrong == 0 and sure >= 500                                      # (the table is made of borders: most of its rows are not sure)
    assert per_class["outside_band"][0] >= 0.9 * per_class["outside_band"][1]
    flat_hit = [k for k in np.flatnonzero(keep) if kat[k][14] == "band_flat" and kat[k][13] == 1]
    assert flat_hit and all(single_form_outcome(rows[k]) == "unsure" for k in flat_hit)
