"""What a shade's result does not need, in the persistent frame kernels and the frame server (csrc/flx_frame_common.h: shade0_tile, shade_path; profiles/shade_needless.txt):

  * FLX_SHADE_COS_TABLE: cos((float)s) of the sample number from a table the context makes once (WavefrontBuffers::cosSample, WF_COS_SAMPLES = 64 entries) — a scalar
    load at bounce 0, where s is the loop's counter, a vector load by the lane's s at the later bounces; a sample number beyond the table computes;
  * FLX_SHADE_FIRST_LIGHT: in a scene of ONE light the reservoir's first draw is not made; whether the light is taken is an f32 range check
    (include/flx_reservoir_first.h, held against the literal comparison by tests/test_reservoir_first_cpu.py), with the sine behind a branch where the weight is +inf;
  * FLX_FRAME_ANGLE_TABLE: the frame kernel of whole frames (the front inside, unstamped: here the COUNTED frames of front_inside) reads DeviceScene::angle_tan.

What may go wrong, and the smallest frames on which it would: samples 1, 3 and 8 (table entries 0, 2 and 7; 3: item_pixel's division), 65 samples on one screen tile (one
more than the table holds); max_reflections 1 (bounce 0 alone) and 4 (shade_path's vector load, records rewritten); one light, one light of strength 0, no light, two
lights, two lights of which the first has strength 0 (in the last two the rule must be off: the draw feeds the second light); random_seed 11 500 — the sine's argument
of the draw's .x is below 2^20 and that of its .y above: .y is NaN and the light is NOT taken — and 20 000, all NaN; a light of strength 1e30, whose weight overflows to
+inf: the branch that takes the sine (the frame itself stays finite there, largest value 4.7e27, no non-finite value: the test tells the overflow from the frame's
magnitude, see test_the_frames_hold_what_the_cases_need).  The table follows an upload of the transforms and an update of the vertices.  Every frame is the oracle's bit for bit, counted
and uncounted, with the oracle's work counters, through the three fronts of tests/test_fold_order_gpu.py and through the frame server."""
import copy
import functools

import numpy as np
import pytest

import synth_scene
from scene_update_util import moved, rows_for_update

pytestmark = pytest.mark.gpu

COUNTERS = ("closest_visits", "shadow_visits", "shades", "closest_walks", "shadow_walks")
FRONTS = {"front_outside": 0, "front_inside": 2, "front_kernel": 3}
ORGANISATION = {"front_outside": 2, "front_inside": 3, "front_kernel": 2}
SCENE_SEED = 29                     # tests/test_fold_order_gpu.py's: 28.8 % of its bounce-0 paths go on, a third of its screen tiles see past the scene

#        name                    scene            width height samples max_reflections random_seed
CASES = {"one_s1_b1":            ("one",            64, 48, 1, 1, 0.0),
         "one_s1_b4":            ("one",            64, 48, 1, 4, 0.0),
         "one_s3_b1":            ("one",            64, 48, 3, 1, 0.0),
         "one_s3_b4":            ("one",            64, 48, 3, 4, 0.0),
         "one_s8_b1":            ("one",            64, 48, 8, 1, 0.0),
         "one_s8_b4":            ("one",            64, 48, 8, 4, 0.0),
         "beyond_the_table":     ("one",             8,  8, 65, 2, 0.0),
         "one_dark":             ("one_dark",       64, 48, 2, 4, 0.0),
         "no_light":             ("none",           64, 48, 2, 4, 0.0),
         "two_lights":           ("two",            64, 48, 2, 4, 0.0),
         "two_first_dark":       ("two_first_dark", 64, 48, 2, 4, 0.0),
         "seed_ordinary":        ("one",            64, 48, 2, 4, 7.0),
         "seed_y_nan":           ("one",            64, 48, 2, 4, 11500.0),
         "seed_all_nan":         ("one",            64, 48, 2, 4, 20000.0),
         "weight_overflows":     ("hot",            64, 48, 2, 4, 0.0)}


def config(hip, front):
    hip.set_pipeline(3)
    hip.set_wavefront_organisation(2)
    hip.set_frame_front(front)


def restore(hip):
    hip.set_pipeline(0)
    hip.set_wavefront_organisation(0)
    hip.set_frame_front(1)


def with_lights(base, lights):
    sc = copy.copy(base)
    sc.arrays = dict(base.arrays, lights=np.ascontiguousarray(lights, np.float32).reshape(-1))
    return sc


@functools.lru_cache(maxsize=None)
def scene(kind):
    if kind == "two":
        return synth_scene.make(seed=SCENE_SEED, n_objects=3, tris_per_object=40, n_transforms=3, n_lights=2)
    one = synth_scene.make(seed=SCENE_SEED, n_objects=3, tris_per_object=40, n_transforms=3, n_lights=1)      # (the same triangles: the lights are drawn last)
    if kind == "one":
        return one
    lights = np.array(one.arrays["lights"], np.float32).reshape(-1, 6).copy()
    if kind == "one_dark":
        lights[0, 3] = 0.0
        return with_lights(one, lights)
    if kind == "none":
        return with_lights(one, np.zeros((0, 6), np.float32))
    if kind == "hot":
        lights[0, 3] = 1e30                                  # strength / (1 + distance)^2 is ~1e27 anywhere in the scene: the colour's squares overflow, its length is +inf
        return with_lights(one, lights)
    if kind == "two_first_dark":
        two = np.array(scene("two").arrays["lights"], np.float32).reshape(-1, 6).copy()
        two[0, 3] = 0.0
        return with_lights(scene("two"), two)
    raise KeyError(kind)


def frame_params(name):
    kind, w, h, s, b, seed = CASES[name]
    p = scene(kind).frame_params(width=w, height=h, samples=s, max_reflections=b, use_filter=0)
    p.random_seed = seed
    return p


_oracle_frames = {}


def oracle_frame(oracle, name):
    if name not in _oracle_frames:
        want, cnt, _ = oracle.render(scene(CASES[name][0]), frame_params(name))
        _oracle_frames[name] = (want, cnt)
    return _oracle_frames[name]


# ---- the cases are what they are meant to be (the oracle alone) ------------------------------------------------------------------------------------------

def test_the_frames_hold_what_the_cases_need(oracle):
    assert [len(scene(k).arrays["lights"]) // 6 for k in ("one", "one_dark", "none", "two", "two_first_dark", "hot")] == [1, 1, 0, 2, 2, 1]
    ordinary, cnt = oracle_frame(oracle, "seed_ordinary")
    hot, hot_cnt = oracle_frame(oracle, "weight_overflows")
    # The weight is length(colorForLight): +inf as soon as a component's square overflows, |component| > 2^64 = 1.8e19.  The frame itself stays FINITE at strength
    # 1e30 (its largest value is 4.7e27: forwardTrace's radiance factor is bounded by its BIAS floors to a few thousand, far from the 3.4e8 an overflow of the colour
    # would take), so "the frame holds non-finite values" cannot tell whether the branch runs.  What can: a pixel is the mean over its samples of at most four
    # bounces' colour x importancy x originalColor, both factors <= 1 — a pixel above 4 x 2^64 holds a shade whose colour has a component above 2^64, whose weight is +inf.
    overflowed = int((hot[..., :3] > 4.0 * 2.0 ** 64).any(axis=2).sum())
    print("non-finite values: ordinary", int((~np.isfinite(ordinary)).sum()), "weight overflows", int((~np.isfinite(hot)).sum()),
          "| largest value: ordinary", float(ordinary[..., :3].max()), "weight overflows", float(np.nanmax(hot[..., :3])), "| pixels that hold a shade of weight +inf:", overflowed)
    assert np.isfinite(ordinary).all() and ordinary[..., :3].max() < 2.0 ** 32      # the ordinary case: no weight of +inf anywhere (no component near 2^64) ...
    assert overflowed > 100                                    # ... and here the rule's slow branch runs in more than a hundred pixels, or this case exercises nothing
    assert hot_cnt["shadow_walks"] > 100
    # the seeds: with .y a NaN the light is never taken, no path walks a shadow ray, and the frame differs from the ordinary seed's
    for name in ("seed_y_nan", "seed_all_nan"):
        f, c = oracle_frame(oracle, name)
        assert c["shadow_walks"] == 0 and c["shades"] > 0, name
    assert cnt["shadow_walks"] > 1000
    _, dark = oracle_frame(oracle, "one_dark")
    _, none = oracle_frame(oracle, "no_light")
    assert dark["shadow_walks"] == 0 and none["shadow_walks"] == 0 and dark["closest_walks"] > 0 and none["closest_walks"] > 0
    _, two = oracle_frame(oracle, "two_lights")
    _, first_dark = oracle_frame(oracle, "two_first_dark")
    assert two["shadow_walks"] > 1000 and first_dark["shadow_walks"] > 1000
    _, four = oracle_frame(oracle, "one_s8_b4")
    _, one = oracle_frame(oracle, "one_s8_b1")
    assert one["shades"] == 8 * one["primary_hits"] and four["shades"] > one["shades"]      # later bounces are shaded: shade_path runs
    _, beyond = oracle_frame(oracle, "beyond_the_table")
    assert 0 < beyond["primary_hits"] <= 64 and beyond["shades"] > 65 * beyond["primary_hits"]


# ---- the frames -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("front_name", list(FRONTS))
@pytest.mark.parametrize("name", list(CASES))
def test_frames_equal_the_oracle_counted_and_uncounted(hip, oracle, name, front_name):
    sc = scene(CASES[name][0])
    want, want_cnt = oracle_frame(oracle, name)
    hip.update_scene(sc)
    p = frame_params(name)
    try:
        config(hip, FRONTS[front_name])
        counted, cnt, _ = hip.render(p, counters=True)           # (front_inside: k_wf_frame<true, true>, unstamped — the per-triangle table)
        info, organisation = hip.last_walk_lds(), hip.last_organisation()
        plain = hip.render(p)[0]                                 # (uncounted and thin: with the front inside, this is k_wf_frame_stamped)
        organisation_plain = hip.last_organisation()
    finally:
        restore(hip)
    assert organisation == organisation_plain == ORGANISATION[front_name] and info["kind"] == organisation, (organisation, organisation_plain, info)
    assert np.array_equal(counted, want, equal_nan=True)
    assert {k: cnt[k] for k in COUNTERS} == {k: want_cnt[k] for k in COUNTERS}
    assert np.array_equal(plain.view(np.uint32), counted.view(np.uint32))


@pytest.mark.parametrize("name", ["one_s3_b4", "one_s8_b4", "seed_y_nan", "weight_overflows", "two_lights", "no_light"])
def test_served_frames_equal_the_oracle(hip, oracle, name):
    """the same shading in k_wf_server: frames through the frame server, three in flight"""
    sc = scene(CASES[name][0])
    want, _ = oracle_frame(oracle, name)
    hip.update_scene(sc)
    hip.set_frame_chain(3)
    hip.set_frame_lanes(3)
    p = frame_params(name)
    try:
        assert hip.frame_server_takes(p)
        hip.frame_begin(p)                                       # (the frame that follows update_scene itself goes to the lanes)
        hip.frame_end()
        got, kinds = [], []
        for _ in range(4):
            if hip.frames_in_flight() == 3:
                got.append(hip.frame_end()[0].copy())
            hip.frame_begin(p)
            kinds.append(hip.last_chained())
        while hip.frames_in_flight():
            got.append(hip.frame_end()[0].copy())
        assert kinds == [3] * 4, kinds
        assert hip.last_walk_lds()["kind"] == 4
        for f in got:
            assert np.array_equal(f, want, equal_nan=True)
    finally:
        hip.set_frame_lanes(2)
        hip.set_frame_chain(2)


# ---- the per-triangle table in the frame kernel -----------------------------------------------------------------------------------------------------------

def turned(sc, angle, scale):
    """the scene's second transform turned about y and scaled (std140 columns of the matrix and of its inverse)"""
    rot = np.array(sc.arrays["rotation"], np.float32).copy().reshape(-1, 2, 12)
    c, s_ = np.cos(angle), np.sin(angle)
    R = np.array([[c, 0, s_], [0, 1, 0], [-s_, 0, c]], np.float64) * scale
    Ri = np.linalg.inv(R)
    for m, M in ((0, R), (1, Ri)):
        for col in range(3):
            rot[1, m, 4 * col:4 * col + 3] = M[:, col]
    return rot.reshape(-1)


def test_the_table_follows_transforms_and_vertices_in_the_frame_kernel(hip, oracle):
    """a frame; flx_transforms_upload with a changed rotation, a frame; a vertex update (flx_scene_update), a frame: each is the oracle's for the arrays as they then
    stand, with the table and without it"""
    sc = scene("one")
    p = frame_params("one_s3_b4")
    hip.update_scene(sc)
    frames = []
    try:
        config(hip, FRONTS["front_inside"])

        def both():
            hip.set_angle_table(True)
            a, ca, _ = hip.render(p, counters=True)              # counted: the unstamped kernel, which reads the table
            assert hip.last_organisation() == 3
            hip.set_angle_table(False)
            b, cb, _ = hip.render(p, counters=True)
            hip.set_angle_table(True)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and ca == cb
            return a, ca

        got, cnt = both()
        want, want_cnt = oracle.render(sc, p)[:2]
        assert np.array_equal(got, want, equal_nan=True) and {k: cnt[k] for k in COUNTERS} == {k: want_cnt[k] for k in COUNTERS}
        frames.append(got)

        rotation = turned(sc, 0.4, 0.7)
        hip.update_transforms(rotation, sc.arrays["shift"])
        sc_turned = copy.copy(sc)
        sc_turned.arrays = dict(sc.arrays, rotation=rotation)
        got, cnt = both()
        want, want_cnt = oracle.render(sc_turned, p)[:2]
        assert np.array_equal(got, want, equal_nan=True) and {k: cnt[k] for k in COUNTERS} == {k: want_cnt[k] for k in COUNTERS}
        frames.append(got)

        sc_moved = moved(sc_turned, 5)                           # every triangle's vertices and normals, the boxes re-flattened
        n = sc_moved.arrays["geometry"].size // 12
        rows, attrs = rows_for_update(sc_moved, 0, n)
        hip.update_scene_rows(0, rows, attrs)
        got, cnt = both()
        want, want_cnt = oracle.render(sc_moved, p)[:2]
        assert np.array_equal(got, want, equal_nan=True) and {k: cnt[k] for k in COUNTERS} == {k: want_cnt[k] for k in COUNTERS}
        frames.append(got)
        assert not np.array_equal(frames[0], frames[1], equal_nan=True) and not np.array_equal(frames[1], frames[2], equal_nan=True)
    finally:
        hip.set_angle_table(True)
        restore(hip)
        hip.update_scene(sc)


def test_the_server_with_changing_transforms_equals_the_oracle(hip, oracle):
    """transforms uploaded before every frame: the server's launch for a scene that moves (a version of the transforms per frame in flight) computes the terms — one
    table cannot follow them — and every frame is the oracle's for its own arrays"""
    sc = scene("one")
    p = frame_params("one_s3_b4")
    hip.update_scene(sc)
    hip.set_frame_chain(3)
    hip.set_frame_lanes(3)
    N = 6
    rotations = [turned(sc, 0.1 * f, 1.0 + 0.05 * f) for f in range(N)]
    try:
        assert hip.frame_server_takes(p)
        hip.frame_begin(p)
        hip.frame_end()
        got, kinds, moving = [], [], []
        for f in range(N):
            if hip.frames_in_flight() == 3:
                got.append(hip.frame_end()[0].copy())
            hip.update_transforms(rotations[f], sc.arrays["shift"])
            hip.frame_begin(p)
            kinds.append(hip.last_chained())
            moving.append(hip.server_moving())
        while hip.frames_in_flight():
            got.append(hip.frame_end()[0].copy())
        assert kinds == [3] * N, kinds
        assert moving[-1], moving                                  # the launch for a scene that moves took over
        for f in range(N):
            at = copy.copy(sc)
            at.arrays = dict(sc.arrays, rotation=rotations[f])
            assert np.array_equal(got[f], oracle.render(at, p)[0], equal_nan=True), f
    finally:
        hip.update_transforms(sc.arrays["rotation"], sc.arrays["shift"])
        hip.set_frame_lanes(2)
        hip.set_frame_chain(2)
