"""The CPU side of test_server_moving_gpu.py (the frame server's moving scenes; tests/server_moving_util.py): with the oracle alone, no device.

  * No wrong frame can hide: a frame rendered with another frame's transforms and lights differs from the right one in a quarter of its lit pixels at the least,
    so a stale version or a wrong post cannot pass for the frame.  These are conditions on the INPUTS (the scene's seed, the steps of the sequence), met by what
    server_moving_util.py commits.
  * The posts have the sizes the GPU cases rely on, and the limit is where they put it.
  * classify() names a stale version, a neighbouring post and a mix for what they are."""
import os

import numpy as np
import pytest

import server_moving_util as u

FRAMES = 13                     # the longest sequence of the GPU cases (4 x 3 + 1); the arrays of frames 0 and 1 are the scene's own


def _index(f):
    return f if f >= 2 else -1


@pytest.mark.parametrize("L", [0, 1, 2])
@pytest.mark.parametrize("T", [1, 2, 4])
def test_no_wrong_frame_can_hide(oracle, T, L):
    """64 x 48: every frame f has a primary hit in a quarter of its pixels, and with the arrays of any other frame g (its own view and seed) it differs in a quarter
    of those; for L = 0 through the transforms alone"""
    worst, least = 1.0, 1.0
    for f in range(FRAMES):
        want = u.oracle_frame(oracle, T, L, u.WIDE, _index(f), _index(f), f)
        hit = want[..., 3] != 0
        least = min(least, hit.mean())
        assert hit.mean() >= 0.25, (f, hit.mean())
        for g in range(FRAMES):
            if _index(g) == _index(f):
                continue
            other = u.oracle_frame(oracle, T, L, u.WIDE, _index(g), _index(g), f)
            share = u.differing(want, other)[hit].mean()
            worst = min(worst, share)
            assert share >= 0.25, (f, g, share)
    print("T %d, L %d: primary hits in %.3f of the pixels at the least, a wrong frame differs in %.3f of them at the least" % (T, L, least, worst))


@pytest.mark.parametrize("T,L,n", [(1, 1, 13), (2, 1, 13), (2, 160, 9), (2, 161, 9)])
def test_no_wrong_frame_can_hide_in_one_tile(oracle, T, L, n):
    """8 x 8 (at 160 and 161 lights: the only frame there is): eight differing pixels at the least"""
    worst = 64
    for f in range(n):
        want = u.oracle_frame(oracle, T, L, u.TILE, _index(f), _index(f), f)
        assert want.shape == (8, 8, 4)
        for g in range(n):
            if _index(g) != _index(f):
                count = int(u.differing(want, u.oracle_frame(oracle, T, L, u.TILE, _index(g), _index(g), f)).sum())
                worst = min(worst, count)
                assert count >= 8, (f, g, count)
    print("T %d, L %d: a wrong frame differs in %d of 64 pixels at the least" % (T, L, worst))


def test_transforms_alone_and_lights_alone_show(oracle):
    """the sequences of test_what_is_uploaded: the transforms of another frame under a frame's own lights, and the other way round, each change a quarter of the lit pixels"""
    T, L = 4, 2
    for f in range(2, 9):
        want = u.oracle_frame(oracle, T, L, u.WIDE, f, f, f)
        hit = want[..., 3] != 0
        for g in (-1, f - 1, f + 1, f + 20):
            assert u.differing(want, u.oracle_frame(oracle, T, L, u.WIDE, g, f, f))[hit].mean() >= 0.25, (f, g, "transforms")
            assert u.differing(want, u.oracle_frame(oracle, T, L, u.WIDE, f, g, f))[hit].mean() >= 0.25, (f, g, "lights")


def test_the_sequences_move_everything():
    """every transform is turned and shifted, every light moved by about a scene radius and its strength scaled by 1 + 0.5 (k % 3); index -1 is the scene's own"""
    T, L = 4, 2
    sc = u.scene(T, L)
    rot0, sh0, lt0 = u.arrays(T, L, -1)
    assert rot0 is sc.arrays["rotation"] and sh0 is sc.arrays["shift"] and lt0 is sc.arrays["lights"]
    assert lt0.size == 6 * L and (lt0.reshape(-1, 6)[:, 3] > 0).all()
    for k in range(13):
        rot, sh, lt = u.arrays(T, L, k)
        r, r0 = rot.reshape(T, 2, 12), rot0.reshape(T, 2, 12)
        for t in range(T):
            assert np.abs(r[t, 0] - r0[t, 0]).max() > 0.1 and np.abs(r[t, 1] - r0[t, 1]).max() > 0.1, (k, t)
            m = np.stack([r[t, 0, 0:3], r[t, 0, 4:7], r[t, 0, 8:11]]).astype(np.float64)
            mi = np.stack([r[t, 1, 0:3], r[t, 1, 4:7], r[t, 1, 8:11]]).astype(np.float64)
            assert np.abs(m @ mi - np.eye(3)).max() < 1e-5, (k, t)                          # the inverse with it
            assert np.linalg.norm(sh.reshape(T, 8)[t, 0:3] - sh0.reshape(T, 8)[t, 0:3]) > 0.25, (k, t)
            assert np.array_equal(sh.reshape(T, 8)[t, 4:7], -sh.reshape(T, 8)[t, 0:3])
        moved = np.linalg.norm(lt.reshape(L, 6)[:, 0:3] - lt0.reshape(L, 6)[:, 0:3], axis=1)
        assert (moved > 0.9 * u.RADIUS).all() and (moved < 1.1 * u.RADIUS).all(), (k, moved)
        assert np.allclose(lt.reshape(L, 6)[:, 3], lt0.reshape(L, 6)[:, 3] * (1.0 + 0.5 * (k % 3)))
    for L in (0, 160, 161):
        assert u.arrays(2, L, 3)[2].size == 6 * L and (u.base_lights(L)[:, 3] > 0).all()


def test_blob_sizes_and_the_limit():
    want = {(1, 0): 32, (1, 1): 38, (2, 0): 64, (2, 1): 70, (4, 2): 140, (2, 160): 1024, (2, 161): 1030}
    for (T, L), words in want.items():
        assert u.blob_words(T, L) == 32 * T + 6 * L == words, (T, L)
        rot, sh, lt = u.arrays(T, L, 2)
        assert rot.size + sh.size + lt.size == words, (T, L)                                 # what server_post copies behind the view
    limit = u.source_constant("flx_server.h", "SV_BLOB_WORDS")
    assert limit == 1024
    assert u.blob_words(2, 160) == limit and u.blob_words(2, 161) > limit
    # the copy loops run `for (t = lane; t < blobWords; t += 64)`: half a trip, a trip and a few lanes, one trip, sixteen trips, and past the limit
    assert [w % 64 for w in (32, 38, 64, 70, 140, 1024)] == [32, 38, 0, 6, 12, 0] and 1024 // 64 == 16
    assert u.source_constant("flx_server.hip", "FLX_SERVER_RELAY_GROUPS") >= 2
    with open(os.path.join(u.CSRC, "flx_server.h")) as fh:
        assert "return n_transforms * 32u + n_lights * 6u;" in fh.read()                     # server_blob_words, as blob_words restates it


def test_classify_names_what_a_wrong_frame_shows(oracle):
    T, L, depth = 2, 1, 3
    seq = u.Sequence(oracle, T, L, u.WIDE, depth)
    assert seq.n == 13 and seq.holds[:3] == [(-1, -1), (-1, -1), (2, 2)] and seq.first_moved() == 2
    f = 7
    seq.slots[f] = 1
    right = seq.want(f)
    assert "the frame is right" in u.classify(right, f, seq)
    stale = u.classify(seq.frame(f - depth, f), f, seq)                      # frame 7 with the arrays of frame 4, the slot's occupant before
    assert "STALE VERSION: the arrays of frame 4" in stale and "WRONG POST" not in stale and "slot 1 of 3" in stale, stale
    before = u.classify(seq.frame(f - 1, f), f, seq)
    assert "WRONG POST: the arrays of frame 6, the one before" in before and "STALE" not in before, before
    after = u.classify(seq.frame(f + 1, f), f, seq)
    assert "WRONG POST: the arrays of frame 8, the one after" in after and "STALE" not in after, after
    far = u.classify(seq.frame(11, f), f, seq)
    assert "the arrays of frame [11]" in far and "STALE" not in far and "WRONG POST" not in far, far
    # a frame swapped with its neighbour — the view and the seed are frame 6's too: no frame of frame 7's view
    swapped = u.classify(seq.want(f - 1), f, seq)
    assert "none of these (a mix)" in swapped, swapped
    # the upper half of the stale frame, the lower half of the right one
    mix = np.array(right)
    mix[:24] = seq.frame(f - depth, f)[:24]
    line = u.classify(mix, f, seq)
    assert "none of these (a mix): rows 0 .. 23" in line and "STALE" not in line, line
    count = int(u.differing(mix, right).sum())
    assert ("%d of 3072 pixels differ" % count) in line and count >= 0.25 * 0.25 * 3072
    # depth 2 in a sequence whose frames 0 and 1 share the scene's own arrays: frame 3's stale version is frame 1's, frame 2's neighbour before is frame 1's
    two = u.Sequence(oracle, T, L, u.WIDE, 2)
    assert "STALE VERSION: the arrays of frame 1" in u.classify(two.frame(1, 3), 3, two)
    both = u.classify(two.frame(0, 2), 2, two)                               # frames 0 and 1 hold the same arrays: stale and the post before
    assert "STALE VERSION: the arrays of frame 0" in both and "WRONG POST: the arrays of frame 1" in both, both


def test_the_driver_s_sequences(oracle):
    """holds follows the uploads in order: the last of two counts, an array that is not uploaded stays"""
    ups = [[], [], [(u.TRANSFORMS, 2)], [(u.LIGHTS, 3)], [(u.BOTH, 24), (u.BOTH, 4)], [(u.BOTH, 4)], []]
    seq = u.Sequence(oracle, 4, 2, u.WIDE, 2, ups=ups, n=7)
    assert seq.holds == [(-1, -1), (-1, -1), (2, -1), (2, 3), (4, 4), (4, 4), (4, 4)] and seq.first_moved() == 2
    assert u.same(seq.frame(5, 6), seq.frame(4, 6)) and not u.same(seq.frame(3, 6), seq.frame(4, 6))
