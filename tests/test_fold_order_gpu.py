"""A walk lane's fold (FLX_WALK_LANE_FOLD_FETCH / FLX_WALK_LANE_FOLD_WITH, csrc/flx_frame_common.h; FLX_WF_FOLD_EARLY).  In the persistent frame kernels and the frame
server a compact bounce-0 path that goes on gets the first words of its full record from the lane that walked it, not from memory a second time, and the loads a fold
starts with have one site for either form of record, the compact form's constants put in afterwards.  What may go wrong with that, and the smallest frames on which it would:

  * max_reflections 1: every compact path ends in its fold, no full record is ever written;
  * max_reflections 2: compact -> full record (from the lane), then ONE plain fold reads that record back; max_reflections 4: records rewritten by the shade waves;
  * the stamped kernels (the front of the frame outside the frame kernel, or inside it in an uncounted thin frame): the time a path came in sits above the flags in the
    lane, and the record must get the flags alone — the shade waves and the next install read them;
  * lanes that reach the fold without a walk: lights of strength 0 and max_reflections 1 give P_DONE at install;
  * dead items and live paths in one wave: the camera sees past the scene in a third of the screen tiles;
  * samples 3: the per-pixel part of a compact record through item_tile's division, not its shift;
  * 8 x 8 at 1 spp: blocks that fold with nothing to refill;  64 x 48 at 2 spp: blocks that fold and refill from both rings.

Both sides of the fold's `goes on` branch are taken in the same waves: see FOLD_SEED.  Every frame is the oracle's bit for bit, and the work counters are the oracle's."""
import copy
import functools

import numpy as np
import pytest

import synth_scene

pytestmark = pytest.mark.gpu

COUNTERS = ("closest_visits", "shadow_visits", "shades", "closest_walks", "shadow_walks")
FRONTS = {"front_outside": 0, "front_inside": 2, "front_kernel": 3}
ORGANISATION = {"front_outside": 2, "front_inside": 3, "front_kernel": 2}      # flx_last_organisation: 2 k_wf_frame<., false> — always stamped —, 3 the front inside
# chosen on the CPU, with the oracle alone, among seeds 0 .. 59: of the bounce-0 paths of the 64 x 48 frame at 2 spp, 28.8 % go on (went_on_share: 0.288), and 17 of its 48
# screen tiles hold pixels with and without a primary hit
FOLD_SEED = 29

#        name              width height samples max_reflections
CASES = {"ends_in_fold":   (64, 48, 2, 1),
         "one_plain_fold": (64, 48, 2, 2),
         "four_bounces":   (64, 48, 2, 4),
         "no_walk":        (64, 48, 2, 1),
         "three_samples":  (64, 48, 3, 3),
         "one_tile":       (8, 8, 1, 3)}


def config(hip, front):
    hip.set_pipeline(3)
    hip.set_wavefront_organisation(2)
    hip.set_frame_front(front)


def restore(hip):
    hip.set_pipeline(0)
    hip.set_wavefront_organisation(0)
    hip.set_frame_front(1)


@functools.lru_cache(maxsize=None)
def fold_scene():
    return synth_scene.make(seed=FOLD_SEED, n_objects=3, tris_per_object=40, n_transforms=3, n_lights=2)


@functools.lru_cache(maxsize=None)
def dark_scene():
    """the same scene with lights of strength 0: no path needs a shadow walk"""
    base = fold_scene()
    sc = copy.copy(base)
    lights = np.array(base.arrays["lights"], np.float32).reshape(-1, 6).copy()
    lights[:, 3] = 0.0
    sc.arrays = dict(base.arrays, lights=lights.reshape(-1))
    return sc


def scene_of(name):
    return dark_scene() if name == "no_walk" else fold_scene()


def frame_params(name):
    w, h, s, b = CASES[name]
    return scene_of(name).frame_params(width=w, height=h, samples=s, max_reflections=b, use_filter=0)


_oracle_frames = {}


def oracle_frame(oracle, name):
    if name not in _oracle_frames:
        want, cnt, _ = oracle.render(scene_of(name), frame_params(name))
        _oracle_frames[name] = (want, cnt)
    return _oracle_frames[name]


def went_on_share(cnt, samples):
    """of the bounce-0 paths of a frame of max_reflections 2, the share that was shaded a second time"""
    first = samples * cnt["primary_hits"]
    return (cnt["shades"] - first) / first


# ---- the scenes are what they are meant to be (CPU side of the GPU cases) --------------------------------------------------------------------------------

def test_the_frames_hold_what_the_cases_need(oracle):
    want, cnt = oracle_frame(oracle, "one_plain_fold")
    share = went_on_share(cnt, 2)
    print("bounce-0 paths that go on:", share)
    assert 0.2 <= share <= 0.8
    hit = want[..., 3].reshape(6, 8, 8, 8).transpose(0, 2, 1, 3).reshape(48, 64) != 0      # [screen tile][pixel]: a wave's 64 fresh paths
    mixed = int(((hit.sum(1) > 0) & (hit.sum(1) < 64)).sum())
    print("screen tiles with and without a primary hit:", mixed)
    assert mixed >= 8
    _, ends = oracle_frame(oracle, "ends_in_fold")
    assert ends["shades"] == 2 * ends["primary_hits"] and ends["shadow_walks"] > 1000       # one shading per path: every path ends in its first fold
    _, dark = oracle_frame(oracle, "no_walk")
    assert dark["shadow_walks"] == 0 and dark["closest_walks"] == 0 and dark["shades"] == 2 * dark["primary_hits"] > 0
    _, four = oracle_frame(oracle, "four_bounces")
    assert four["shades"] > cnt["shades"]                                                  # paths shaded a third time: records the shade waves rewrote
    _, tile = oracle_frame(oracle, "one_tile")
    assert 0 < tile["primary_hits"] <= 64


# ---- the frames -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("front_name", list(FRONTS))
@pytest.mark.parametrize("name", list(CASES))
def test_frames_equal_the_oracle_counted_and_uncounted(hip, oracle, name, front_name):
    sc = scene_of(name)
    want, want_cnt = oracle_frame(oracle, name)
    hip.update_scene(sc)
    p = frame_params(name)
    try:
        config(hip, FRONTS[front_name])
        counted, cnt, _ = hip.render(p, counters=True)
        info, organisation = hip.last_walk_lds(), hip.last_organisation()
        plain = hip.render(p)[0]                                 # (uncounted and thin: with the front inside, this is k_wf_frame_stamped)
        organisation_plain = hip.last_organisation()
    finally:
        restore(hip)
    # the frame kernel rendered both, from compact bounce-0 records (it has no other form of them); organisation 2 is the kernel that stamps every path
    assert organisation == organisation_plain == ORGANISATION[front_name] and info["kind"] == organisation, (organisation, organisation_plain, info)
    assert np.array_equal(counted, want, equal_nan=True)
    assert {k: cnt[k] for k in COUNTERS} == {k: want_cnt[k] for k in COUNTERS}
    assert np.array_equal(plain.view(np.uint32), counted.view(np.uint32))


@pytest.mark.parametrize("name", ["one_plain_fold", "four_bounces"])
def test_served_frames_equal_the_oracle(hip, oracle, name):
    """the same fold in k_wf_server: frames through the frame server, three in flight"""
    sc = scene_of(name)
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
