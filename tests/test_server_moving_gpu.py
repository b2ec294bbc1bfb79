"""The frame server's moving scenes (csrc/flx_server.hip: k_wf_server<VER = true, .>) at every slot re-use and blob size.  A scene that moves sends its transforms and
lights with every frame: the host copies them behind the view (flx_api.hip: server_post), up to FLX_SERVER_RELAY_GROUPS workgroups pass the post on in device memory,
every workgroup copies it into its own version of the slot (global memory for the shading, LDS for the walk waves' inverse transforms: sAvail), and tryRotate hands
the slot to the frame `depth` later.  What may go wrong there, and the cases that would show it:

  1  the three 64-lane copy loops at posts of 32, 38, 64, 70 and 140 words: half a trip, a trip and six lanes, one whole trip, three trips; no lights at all;
  2  the limit of a post: 1024 words are served, 1030 go to the lanes — and come back;
  3  1, 15, 16, 17 and all workgroups: the only workgroup relays to itself, every workgroup relays, one sees nothing but the relay's copy;
  4  frames of one screen tile: every workgroup but one fetches the view only to rotate, the shortest time between a version's last read and its overwrite;
  5  the host's pacing: batches of `depth`, one frame at a time, flx_sync in the loop, a host that pauses (steady: the cases of 1);
  6  what is uploaded: transforms alone, lights alone, in turn, twice before a frame, the same arrays again;
  7  the device's arrays after the launch: flx_rays_cast with such frames in flight;
  8  RGBA8 frames.

Every sequence has 4 x depth + 1 frames — its launch starts at frame 2, so every slot is re-used three times at the least —, every frame is compared bit for bit
(NaN equal to NaN) with the CPU oracle's frame of its own arrays, which shares no code with the server or with flx_dyn_flush; a wrong frame is classified (a stale
version, a neighbour's post, a mix: server_moving_util.classify).  test_server_moving_cpu.py shows on the CPU that a frame with the arrays of another differs in a
quarter of its lit pixels (eight of the 64 of one tile) at the least.

What the cases found when they were written (profiles/server_moving_tests.txt): with 4 transforms and three slots a frame never completed — sAvail could set "the view
is here" across a rotation, and the workgroup went through the slot twice —, and every frame of less than 16 KB stalled a launch on all CUs for two seconds, its copy to
the host being a kernel of the runtime's (cases 2, 4 and 8 at 6 .. 10 s each, the rotation count of case 4 short).  Both are fixed; the file takes about 3 s."""
import time

import numpy as np
import pytest

import server_moving_util as u
from flexlight_hip import capi

pytestmark = pytest.mark.gpu

_started = time.perf_counter()
RELAY = u.source_constant("flx_server.hip", "FLX_SERVER_RELAY_GROUPS")
SIZES = [(1, 0), (1, 1), (2, 0), (2, 1), (4, 2)]
TWO = [(1, 1), (4, 2)]


def ids(v):
    return "T%d-L%d" % v if isinstance(v, tuple) else None


def launch_groups(hip, asked):
    """workgroups of the server's launch (flx_api.hip, server_post: cusWalk)"""
    cus = hip.device_info()[1]
    reserved = u.source_constant("flx_api.hip", "FLX_SERVER_RESERVED_CUS")
    walk = cus - reserved if cus > 4 * reserved else cus
    return asked if asked and asked < walk else walk


def served_and_right(hip, seq, got, kinds, flags):
    """every frame went to the server, the launch took the arrays per frame from the first changed upload on, every frame is the oracle's"""
    assert kinds == [3] * seq.n, kinds
    first = seq.first_moved()
    assert flags[first:] == [True] * (seq.n - first) and not any(flags[:first]), flags
    info = hip.last_walk_lds()
    assert (info["kind"], info["n_transforms"]) == (4, seq.T), info
    wrong = u.wrong_frames(got, seq)
    assert not wrong, "\n".join(wrong)


def test_the_scenes_are_the_smallest_the_server_takes(hip):
    """128 entries and the terminator: 129 walk entries; a scene of one entry fewer is not taken (test_server_gpu.py::test_frames_the_server_does_not_take)"""
    import synth_scene
    assert RELAY >= 2                                                        # (read from the source: the group counts of case 3 stand around it)
    hip.set_frame_chain(3)
    try:
        for T, L in SIZES:
            sc = u.scene(T, L)
            hip.update_scene(sc)
            assert hip.last_walk_lds()["walk_entries"] == u.ENTRIES + 1
            assert hip.frame_server_takes(u.params(T, L, u.WIDE, 0)) and hip.frame_server_takes(u.params(T, L, u.TILE, 0)), (T, L)
        small = synth_scene.make_sized(u.ENTRIES - 1, 1, seed=1)
        hip.update_scene(small)
        assert not hip.frame_server_takes(small.frame_params(use_filter=0))
    finally:
        hip.set_frame_chain(2)


# ---- 1. blob sizes ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("size", SIZES, ids=ids)
def test_blob_sizes(hip, oracle, size, depth):
    T, L = size
    seq = u.Sequence(oracle, T, L, u.WIDE, depth)
    with u.knobs(hip, seq):
        got, kinds, flags = u.run(hip, seq)
        served_and_right(hip, seq, got, kinds, flags)


# ---- 2. the limit -------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [2, 3])
def test_a_post_of_exactly_the_limit_is_served(hip, oracle, depth):
    """2 transforms and 160 lights: 1024 words, sixteen whole trips of the copy loops.  In the default mode (flx_set_frame_chain(2)) a frame that follows an upload
    stays with the server only while the arrays fit a post"""
    seq = u.Sequence(oracle, 2, 160, u.TILE, depth)
    assert u.blob_words(2, 160) == u.source_constant("flx_server.h", "SV_BLOB_WORDS")
    with u.knobs(hip, seq, chain=2):
        got, kinds, flags = u.run(hip, seq)
        served_and_right(hip, seq, got, kinds, flags)


@pytest.mark.parametrize("depth", [2, 3])
def test_a_post_past_the_limit_goes_to_the_lanes_and_comes_back(hip, oracle, depth):
    """one light more: 1030 words.  No launch takes them per frame; in the default mode every frame that follows a changed upload goes to the lanes
    (flx_api.hip, frame_begin: `Where they do not fit a post ...`) — flx_last_chained says 0 there — and is right.  With 160 lights again the server serves"""
    seq = u.Sequence(oracle, 2, 161, u.TILE, depth)
    assert u.blob_words(2, 161) > u.source_constant("flx_server.h", "SV_BLOB_WORDS")
    with u.knobs(hip, seq, chain=2):
        got, kinds, flags = u.run(hip, seq)
        assert flags == [False] * seq.n, flags
        assert kinds == [3, 3] + [0] * (seq.n - 2), kinds                    # (frames 0 and 1 follow no upload)
        wrong = u.wrong_frames(got, seq)
        assert not wrong, "\n".join(wrong)
        back = u.Sequence(oracle, 2, 160, u.TILE, depth)                     # the same scene but for its lights
        assert np.array_equal(u.scene(2, 160).arrays["geometry"], u.scene(2, 161).arrays["geometry"])
        back.restore(hip)                                                    # 160 lights: another count is another scene, and one that has moved already
        got, kinds, flags = u.run(hip, back)
        assert kinds == [3] * back.n, kinds
        assert flags[2:] == [True] * (back.n - 2), flags
        wrong = u.wrong_frames(got, back)
        assert not wrong, "\n".join(wrong)


# ---- 3. groups around the relay ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("size", TWO, ids=ids)
@pytest.mark.parametrize("groups", [1, RELAY - 1, RELAY, RELAY + 1, 0], ids=lambda g: "groups%d" % g)
def test_groups_around_the_relay(hip, oracle, groups, size, depth):
    T, L = size
    seq = u.Sequence(oracle, T, L, u.WIDE, depth)
    assert launch_groups(hip, RELAY + 1) == RELAY + 1                        # (the device has more workgroups than relay: one of 17 sees only the relay's copy)
    with u.knobs(hip, seq, groups=groups):
        got, kinds, flags = u.run(hip, seq, before_drain=hip.sync)
        served_and_right(hip, seq, got, kinds, flags)
        stats = hip.server_stats()
        assert stats["frames"] == seq.n - 2, stats                           # ONE launch from the first changed upload on
        assert stats["rotations"] == launch_groups(hip, groups) * (seq.n - 2), stats


# ---- 4. one screen tile -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("groups", [0, RELAY + 1], ids=lambda g: "groups%d" % g)
@pytest.mark.parametrize("size", [(1, 1), (2, 1)], ids=ids)
def test_frames_of_one_screen_tile(hip, oracle, size, groups, depth):
    """8 x 8 at one sample: one workgroup makes the tile, every other one has nothing of the frame and rotates as soon as it has the view.  flx_get_server_stats
    counts the rotations (SVS_ROTATIONS): every workgroup rotated for every frame"""
    T, L = size
    seq = u.Sequence(oracle, T, L, u.TILE, depth)
    with u.knobs(hip, seq, groups=groups):
        got, kinds, flags = u.run(hip, seq, before_drain=hip.sync)           # (flx_sync: the launch has ended, its counters are final)
        served_and_right(hip, seq, got, kinds, flags)
        stats = hip.server_stats()
        n_groups = launch_groups(hip, groups)
        assert n_groups > 1
        assert stats["frames"] == seq.n - 2 and stats["tiles"] == seq.n - 2, stats
        assert stats["rotations"] == n_groups * (seq.n - 2), (stats, n_groups)


# ---- 5. pacing ----------------------------------------------------------------------------------------------------------------------------------------------------

def paced(oracle, T, L, depth, pacing):
    if pacing == u.BATCHES:                                                  # begin `depth` frames, end them all, upload, repeat: the frames of a batch share their arrays
        n = 4 * depth + 1
        ups = [[(u.BOTH, f)] if f >= depth and f % depth == 0 else [] for f in range(n)]
        return u.Sequence(oracle, T, L, u.WIDE, depth, ups=ups)
    return u.Sequence(oracle, T, L, u.WIDE, depth)


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("size", TWO, ids=ids)
@pytest.mark.parametrize("pacing", [u.BATCHES, u.SINGLE, u.SYNCED, u.PAUSED])
def test_pacing(hip, oracle, pacing, size, depth):
    """(steady, with the same scenes and depths: test_blob_sizes.)  No pause comes near the launch's idle exit of 2 s (test_server_gpu.py::
    test_a_host_that_pauses_loses_nothing has that)"""
    T, L = size
    seq = paced(oracle, T, L, depth, pacing)
    with u.knobs(hip, seq):
        got, kinds, flags = u.run(hip, seq, pacing=pacing)
        served_and_right(hip, seq, got, kinds, flags)
        if pacing == u.SINGLE:
            assert seq.slots == [0] * seq.n, seq.slots                       # every launch starts on an empty loop
        elif pacing == u.BATCHES:
            assert seq.slots == [f % depth for f in range(seq.n)], seq.slots
        if pacing in (u.BATCHES, u.SINGLE):
            assert all(not before and not after for _, before, after in seq.around), seq.around      # (the loop ran empty: no launch beside the uploads)
        elif pacing == u.PAUSED:
            assert all(before and after for f, before, after in seq.around if f > 2), seq.around     # the launch goes on over the uploads and the pauses


# ---- 6. what is uploaded ----------------------------------------------------------------------------------------------------------------------------------------

N6 = 9
UPLOADS = {
    "transforms_alone": [[(u.TRANSFORMS, f)] if f >= 2 else [] for f in range(N6)],
    "lights_alone": [[(u.LIGHTS, f)] if f >= 2 else [] for f in range(N6)],
    "in_turn": [[(u.TRANSFORMS if f % 2 == 0 else u.LIGHTS, f)] if f >= 2 else [] for f in range(N6)],
    "twice": [[(u.BOTH, f + 20), (u.BOTH, f)] if f >= 2 else [] for f in range(N6)],
    "the_same_again": [[(u.BOTH, f - f % 2)] if f >= 2 else [] for f in range(N6)],
}


@pytest.mark.parametrize("name", list(UPLOADS))
def test_what_is_uploaded(hip, oracle, name):
    """4 transforms, 2 lights, two frames in flight.  Two uploads before one frame: the last one counts.  The arrays the context holds already, uploaded again in front
    of every second frame: nothing changes, the launch goes on, flx_server_moving keeps its value"""
    seq = u.Sequence(oracle, 4, 2, u.WIDE, 2, ups=UPLOADS[name])
    assert seq.n == N6
    if name == "the_same_again":
        assert [seq.holds[f] == seq.holds[f - 1] for f in range(3, N6)] == [True, False] * 3
    with u.knobs(hip, seq):
        got, kinds, flags = u.run(hip, seq, before_drain=hip.sync)
        served_and_right(hip, seq, got, kinds, flags)
        assert hip.server_stats()["frames"] == N6 - 2                        # ONE launch served every frame from the first changed upload on
        # no launch takes the arrays per frame before the first changed upload; the one that does goes on over every later upload, changed or not
        assert all((before, after) == ((True, True) if f > 2 else (False, False)) for f, before, after in seq.around), seq.around


# ---- 7. after the launch ----------------------------------------------------------------------------------------------------------------------------------------

def primary_rays(oracle, sc, p, n=256):
    """n of the frame's primary rays (flx_oracle_primary's directions) as flx_rays_cast takes them: origin, l, direction, a word nobody reads"""
    import ctypes as C
    from flexlight_hip.scene_io import FrameParams, SceneView
    F3 = C.c_float * 3
    lib = oracle.lib()
    lib.flx_oracle_primary.argtypes = [C.POINTER(SceneView), C.POINTER(FrameParams), C.c_uint32, C.c_uint32, F3, C.POINTER(C.c_int), C.POINTER(C.c_int), F3]
    lib.flx_oracle_primary.restype = None
    view = sc.view()
    rays = np.zeros((n, 8), np.float32)
    for k in range(n):
        px, py = 2 + 4 * (k % 16), 1 + 3 * (k // 16)
        assert px < p.width and py < p.height
        suv, d, ti, tri = F3(), F3(), C.c_int(), C.c_int()
        lib.flx_oracle_primary(C.byref(view), C.byref(p), px, py, suv, C.byref(ti), C.byref(tri), d)
        rays[k] = [p.camera[0], p.camera[1], p.camera[2], 25.0, d[0], d[1], d[2], 0.0]
    return rays


def test_the_device_s_arrays_follow_after_the_launch(hip, oracle):
    """2 transforms, 1 light, three frames in flight: five moving frames in flight or taken, then — the loop still running — flx_rays_cast, which reads the DEVICE's
    transforms: they followed the host's copies (flx_dyn_flush) if the hit rows are those of a fresh context that was given the scene with the last arrays.  The
    frames still in flight are right when they are taken afterwards"""
    T, L, depth = 2, 1, 3
    seq = u.Sequence(oracle, T, L, u.WIDE, depth, ups=[[(u.BOTH, f + 2)] for f in range(5)], n=5)
    last = u.scene_with(T, L, *seq.holds[4])
    rays = primary_rays(oracle, last, seq.params(4))
    with u.knobs(hip, seq):
        hip.cast_rays(rays)                                  # (the call's staging buffers grow here, not beside the launch)
        got, kinds, flags = [], [], []
        for f in range(seq.n):
            if hip.frames_in_flight() == depth:
                got.append(hip.frame_end()[0].copy())
            seq.upload(hip, *seq.ups[f][0])
            hip.frame_begin(seq.params(f))
            kinds.append(hip.last_chained())
            flags.append(hip.server_moving())
        assert kinds == [3] * 5 and flags == [True] * 5, (kinds, flags)
        assert hip.frames_in_flight() == 3
        hits = hip.cast_rays(rays)
        assert hip.frames_in_flight() == 3
        while hip.frames_in_flight():
            got.append(hip.frame_end()[0].copy())
        fresh = capi.Context(0)
        try:
            fresh.update_scene(last)
            want_hits = fresh.cast_rays(rays)
        finally:
            fresh.close()
        words, want_words = hits.view(np.uint32).reshape(-1, 8), want_hits.view(np.uint32).reshape(-1, 8)
        assert (want_words[:, 3].view(np.int32) >= 0).mean() > 0.25              # (the rays hit the scene)
        assert np.array_equal(words, want_words), "%d of %d hit rows differ" % (int((words != want_words).any(1).sum()), len(words))
        first = capi.Context(0)                                                  # ... and NOT those of the scene's own arrays: the rays can tell
        try:
            first.update_scene(u.scene(T, L))
            assert (first.cast_rays(rays).view(np.uint32).reshape(-1, 8) != want_words).any(1).mean() > 0.25
        finally:
            first.close()
        wrong = u.wrong_frames(got, seq)
        assert not wrong, "\n".join(wrong)


# ---- 8. eight-bit frames ----------------------------------------------------------------------------------------------------------------------------------------

def test_rgba8_frames(hip, oracle):
    """frames begun as FLX_FRAME_RGBA8: the server's workgroups quantise the tiles they resolve; the bytes are flx_present's of the oracle's frame
    (oracle.present: the rule of test_server_gpu.py's RGBA8 frames)"""
    seq = u.Sequence(oracle, 1, 1, u.WIDE, 2)
    with u.knobs(hip, seq):
        got, kinds, flags = u.run(hip, seq, rgba8=True)
        assert kinds == [3] * seq.n and flags[2:] == [True] * (seq.n - 2), (kinds, flags)
        assert all(g.dtype == np.uint8 and g.shape == (48, 64, 4) for g in got)
        wrong = u.wrong_frames(got, seq, present=oracle.present)
        assert not wrong, "\n".join(wrong)
        assert not u.same(oracle.present(seq.want(5)), oracle.present(seq.frame(3, 5)))      # (the bytes can tell a stale version)


def test_the_time_this_file_took():
    """(last: the oracle's frames dominate and are shared between the cases)"""
    seconds, frames = u.oracle_spent()
    print("test_server_moving_gpu.py: %.1f s in all, %.1f s of them in the oracle for %d frames" % (time.perf_counter() - _started, seconds, frames))
