"""The oracle's temporal pass against the generated shader's text at every history depth and under motion (tests/temporal_util.py), without a GPU.

The literal is first held against the committed table (tests/golden/temporal_kat.json.gz, written by the scalar, depth-4 transcription of
tests/analysis/make_temporal_kat.py); then flx_oracle_render_sequence and flx_oracle_render_sequence_frames are held against the literal driven by the
oracle's own per-frame G-buffers (flx_oracle_trace): the two differ only where oracle/flx_oracle_filter.c's temporal_pass and ring rotation differ from the text.
The motion runs assert, from the literal's masks, that they do decide the id comparison (temporal_util.Coverage)."""
import ctypes as C

import numpy as np
import pytest

from temporal_util import (Coverage, TemporalRing, copy_params, effective_depth, far_frames, fetch, literal_run, motion_frames, only_w_tells, quantise, still_frames,
                           temporal_literal, temporal_params)
from test_oracle_kat import _temporal_kat_cases, assert_filter_kat, temporal_kat_expectations

W, H = 48, 32
DEPTHS = [1, 2, 3, 4, 5, 6, 8, 9, 13, 16, 0, 17, -1]
STILL = [("dragon", n, 0) for n in DEPTHS] + [("theater", 6, 0), ("theater", 16, 0), ("dragon", 6, 1)]
MOTION = [(name, n) for name in ("theater", "dragon") for n in (4, 6, 16)]


def oracle_gbuffers(oracle, sc, frames):
    return [oracle.trace(sc, q) for q in frames]


def test_quantise_is_the_rgba8_store():
    x = np.array([np.nan, -1.0, -0.0, 0.0, 1e-9, 0.5 / 255, 0.49999 / 255, 1.5 / 255, 0.5, 254.5 / 255, 0.9999999, 1.0, 7.0, np.inf, -np.inf], np.float32)
    want = [0, 0, 0, 0, 0, 1, 0, 2, 128, 255, 255, 255, 255, 255, 0]
    want[5] = int(np.float32(np.float32(x[5] * np.float32(255)) + np.float32(0.5)))          # the two roundings decide the ties, as in Tex.store
    want[7] = int(np.float32(np.float32(x[7] * np.float32(255)) + np.float32(0.5)))
    want[9] = int(np.float32(np.float32(x[9] * np.float32(255)) + np.float32(0.5)))
    assert quantise(x.reshape(1, -1, 1)).reshape(-1).tolist() == want
    every = np.arange(256, dtype=np.uint8).reshape(1, 64, 4)
    assert np.array_equal(quantise(fetch(every)), every)                  # k / 255 stores as k


def test_effective_depth():
    assert [effective_depth(n) for n in (-1, 0, 1, 4, 15, 16, 17, 20, 1000)] == [4, 4, 1, 4, 15, 16, 16, 16, 16]


def test_ring_rotates_backwards_and_a_depth_of_one_has_no_history():
    ring = TemporalRing(3, 1, 1)
    for f in range(5):
        ring.push({n: np.full((1, 1, 4), (f + 1) / 255.0, np.float32) for n in ("color", "color_ip", "location_id", "original_id")})
        assert [int(pl[0, 0, 0]) for pl in ring.c] == [v if v > 0 else 0 for v in (f + 1, f, f - 1)]
        assert ring.filled == min(f, 2)
    one = TemporalRing(1, 1, 2)
    one.push({n: np.zeros((1, 2, 4), np.float32) for n in ("color", "color_ip", "location_id", "original_id")})
    out, masks = temporal_literal(one, 0, 0)
    assert masks.id.shape == (0, 1, 2) and (masks.counter == 1).all()     # no group at all: not even a stand-in for the zero id


@pytest.mark.parametrize("k", range(2))
def test_literal_equals_the_committed_table(oracle, scenes, k):
    case = _temporal_kat_cases()[k]
    sc, p, want = temporal_kat_expectations(case, scenes)
    p.temporal_samples = 4
    got = literal_run(4, oracle_gbuffers(oracle, sc, still_frames(p, want.shape[0])), case["hdr"])
    for f in range(want.shape[0]):
        assert_filter_kat(np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f]), case["hdr"], "literal, sequence %d frame %d" % (k, f))


@pytest.mark.parametrize("name,n,hdr", STILL, ids=["%s_n%d_hdr%d" % c for c in STILL])
def test_oracle_sequence_equals_the_literal_at_every_depth(oracle, scenes, name, n, hdr):
    sc = scenes(name)
    p = temporal_params(sc, W, H, n, hdr=hdr)
    depth = effective_depth(n)
    frames = still_frames(p)
    assert len(frames) == depth + 3
    got = oracle.render_sequence(sc, p, len(frames))
    want = literal_run(depth, oracle_gbuffers(oracle, sc, frames), hdr)
    assert np.array_equal(got[0], got[-1]) == (depth == 1)                 # (the history does change the frame; a depth of 1 has none, and one seed)
    for f in range(len(frames)):
        assert_filter_kat(np.ascontiguousarray(got[f]), want[f], hdr, "%s depth %d frame %d" % (name, n, f))


def oracle_filter(oracle, p, planes_u8):
    """flx_oracle_filter over five RGBA8 planes"""
    from flexlight_hip.scene_io import GBuffers
    planes = [np.ascontiguousarray(fetch(pl)) for pl in planes_u8]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    gb = GBuffers(fp(planes[0]), fp(planes[1]), fp(planes[2]), fp(planes[3]), fp(planes[4]), None)
    out = np.zeros((p.height, p.width, 4), np.float32)
    assert oracle.lib().flx_oracle_filter(C.byref(p), C.byref(gb), fp(out), 0) == 0
    return out


@pytest.mark.parametrize("moving", [0, 1])
def test_oracle_filter_sequence_reads_the_planes_the_literal_writes(oracle, scenes, moving):
    """use_filter = 1, depth 5: the frame is the chain over the literal's two planes and the stored original colour, id and original id of the frame"""
    sc = scenes("dragon")
    p = temporal_params(sc, W, H, 5, use_filter=1)
    frames = motion_frames(p) if moving else still_frames(p)
    got = oracle.render_sequence_frames(sc, frames) if moving else oracle.render_sequence(sc, p, len(frames))
    gbs = oracle_gbuffers(oracle, sc, frames)
    planes = literal_run(5, gbs, 0, use_filter=1)
    for f, (gb, (dColor, dIp)) in enumerate(zip(gbs, planes)):
        want = oracle_filter(oracle, frames[f], [dColor, dIp, quantise(gb["original_color"]), quantise(gb["id"]), quantise(gb["original_id"])])
        assert_filter_kat(np.ascontiguousarray(got[f]), want, 0, "filter frame %d" % f)
    assert not np.array_equal(planes[0][0], planes[-1][0])


@pytest.mark.parametrize("name,n", MOTION, ids=["%s_n%d" % c for c in MOTION])
def test_oracle_sequence_equals_the_literal_under_motion(oracle, scenes, name, n):
    sc = scenes(name)
    p = temporal_params(sc, W, H, n)
    frames = motion_frames(p, n + 4)
    got = oracle.render_sequence_frames(sc, frames)
    cov = Coverage(n)
    want = literal_run(n, oracle_gbuffers(oracle, sc, frames), 0, coverage=cov)
    print(name, cov.figures())
    cov.check(uncovered=name == "theater")
    for f in range(len(frames)):
        assert_filter_kat(np.ascontiguousarray(got[f]), want[f], 0, "%s depth %d frame %d" % (name, n, f))


def test_oracle_sequence_equals_the_literal_where_only_w_tells_a_pixel_from_a_zero_texel(oracle, scenes):
    """cornell from far away: a quarter of the covered pixels store the location id (0, 0, 0, 1 / 255) — equal to an empty slot's or a stand-in's zero texel in
    three of four bytes — beside uncovered pixels, which do equal it"""
    sc = scenes("cornell")
    n = 6
    frames = far_frames(sc, temporal_params(sc, W, H, n))
    gbs = oracle_gbuffers(oracle, sc, frames)
    w_only = only_w_tells(gbs[0])
    assert w_only.sum() >= 100 and (quantise(gbs[0]["location_id"]) == 0).all(axis=-1).sum() >= 100
    got = oracle.render_sequence_frames(sc, frames)
    cov = Coverage(n)
    want = literal_run(n, gbs, 0, coverage=cov)
    assert cov.uncovered_stand_in >= 100 and set(range(1, n + 1)) <= cov.counters, cov.figures()
    assert (want[0][w_only][:, :3] > 0).any()                              # (divided by a counter of 1: nothing else matched)
    for f in range(len(frames)):
        assert_filter_kat(np.ascontiguousarray(got[f]), want[f], 0, "far cornell frame %d" % f)


def test_render_sequence_frames_takes_the_frames_as_given(oracle, scenes):
    sc = scenes("dragon")
    p = temporal_params(sc, W, H, 3)
    # with the seeds f % N it is render_sequence
    assert np.array_equal(oracle.render_sequence_frames(sc, still_frames(p, 5)), oracle.render_sequence(sc, p, 5), equal_nan=True)
    # a seed of the caller's is kept
    other = still_frames(p, 5)
    other[1].random_seed = 7.0
    assert not np.array_equal(oracle.render_sequence_frames(sc, other)[1], oracle.render_sequence(sc, p, 5)[1])
    # frames that do not belong to one run are refused
    for kw in ({"width": W + 8}, {"height": H + 8}, {"temporal_samples": 4}, {"use_filter": 1}, {"is_temporal": 0}):
        bad = still_frames(p, 3)
        bad[2] = copy_params(bad[2], **kw)
        with pytest.raises(RuntimeError):
            oracle.render_sequence_frames(sc, bad)


def test_trace_keeps_the_seed_that_render_overwrites(oracle, scenes):
    """flx_oracle.render of a temporal frame is a run of one frame, seed 0: trace is the source of frame f's G-buffers"""
    sc = scenes("dragon")
    p = copy_params(temporal_params(sc, W, H, 4), random_seed=2.0)
    traced = oracle.trace(sc, p)
    rendered = oracle.render(sc, p, gbuffers=True)[2]
    seed0 = oracle.trace(sc, copy_params(p, random_seed=0.0))
    assert all(np.array_equal(rendered[k], seed0[k], equal_nan=True) for k in traced)
    assert not np.array_equal(traced["color"], seed0["color"])
