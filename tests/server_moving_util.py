"""Moving scenes for the frame server's tests (test_server_moving_cpu.py, test_server_moving_gpu.py): scenes of T transforms and L lights whose post
(ServerMail::blob, csrc/flx_server.h) has a chosen number of words, sequences of transforms and lights that change a frame in most of its pixels from one frame to
the next, the oracle's frames of them — the yardstick: it shares no code with the server or with flx_dyn_flush —, a driver for the frame loop in several
pacings, and classify(), which says WHAT a wrong frame shows.

A sequence names its arrays by an index k: k = -1 the scene's own arrays, k >= 0 the arrays made for frame k (arrays(T, L, k)).  A frame is (transforms of index a,
lights of index b, the view and the seed of frame f): Sequence.holds[f] = (a, b)."""
import copy
import functools
import os
import re
import time

import numpy as np

import synth_scene

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "web-ray-tracer_amd", "csrc")

ENTRIES = 128                   # the smallest scene the frame server takes: 129 walk entries with the terminator (test_the_scenes_are_the_smallest_the_server_takes)
SEED = 7                        # chosen on the CPU (test_server_moving_cpu.py: no wrong frame can hide)
CENTRE = np.array([0.0, 0.0, 10.0])          # of synth_scene.make_sized's volume (x -9 .. 9, y -7 .. 7, z 0 .. 20): the scene's radius is about 10
RADIUS = 10.0
WANDER = 3.0                    # radius of the circle a transform's shift goes round, beside its turn and its drift
GROW = 2.0                      # the objects' triangles, against make_sized's
TURN = 0.74                     # rad per frame: 8.5 steps to a whole turn, so no two of 13 frames come nearer than 0.37 rad (at 0.7 rad, frames nine apart would be 0.017 rad apart)
AXES = np.array([[0.15, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0]])      # transform t turns about AXES[t] (0: the floor stays a floor)
WIDE, TILE = "wide", "tile"
#         width height samples max_reflections
SHAPES = {WIDE: (64, 48, 2, 3),              # 48 screen tiles
          TILE: (8, 8, 1, 3)}                # one screen tile: every workgroup but one holds nothing of the frame
MANY = (8, 8, 1, 2)                          # the cases of 160 and 161 lights: the oracle stays within about a second a frame


def blob_words(n_transforms, n_lights):
    """server_blob_words (csrc/flx_server.h), restated: 2 x 3 float4 of rotation and 2 float4 of shift per transform, 6 floats per light"""
    return 32 * n_transforms + 6 * n_lights


def source_constant(path, name):
    """the integer a source file gives `name`: `#define NAME 16` or `constexpr uint32_t NAME = 1024;`"""
    with open(os.path.join(CSRC, path)) as fh:
        text = fh.read()
    m = re.search(r"#define\s+%s\s+(\d+)" % name, text) or re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)" % name, text)
    assert m, "%s: no %s" % (path, name)
    return int(m.group(1))


def shape_of(L, shape):
    return MANY if L >= 100 else SHAPES[shape]


def base_lights(L):
    """L lights on a spiral over the upper half of a sphere of 1.4 scene radii about the scene's centre, strengths 150 .. 500 (fewer per light where there are many)"""
    lights = np.zeros((L, 6), np.float32)
    for i in range(L):
        z = 0.15 + 0.8 * ((i * 0.618034) % 1.0)
        a = 2.399963 * i + 0.5
        r = np.sqrt(1.0 - z * z)
        lights[i, 0:3] = CENTRE + 1.4 * RADIUS * np.array([r * np.cos(a), z, r * np.sin(a)])
        lights[i, 3] = (150.0 + 350.0 * ((i * 0.381966) % 1.0)) * (1.0 if L <= 2 else 8.0 / L)
        lights[i, 4] = 0.4 if i % 2 else 0.0
    return lights


@functools.lru_cache(maxsize=None)
def scene(T, L):
    """make_sized's scene of ENTRIES entries and T transforms at 64 x 48, its lights replaced by base_lights(L)"""
    sc = synth_scene.make_sized(ENTRIES, T, seed=SEED + 100 * T, width=64, height=48)
    # The objects' triangles GROW about their centres (make_sized's leave most of the view to its floor, which has one colour wherever it is), the boxes follow
    # by make_sized's rule: the bounds of the triangles behind a box, in their own spaces.  Most pixels then show a triangle that moves with its transform.
    g = np.array(sc.arrays["geometry"], np.float32).reshape(-1, 12).copy()
    for i in range(3, ENTRIES):                              # (entry 0: the root box, 1 and 2: the floor)
        if g[i, 10] == 2:
            v = g[i, :9].reshape(3, 3).astype(np.float64)
            g[i, :9] = (v.mean(0) + GROW * (v - v.mean(0))).reshape(-1)
    for i in range(ENTRIES - 1, -1, -1):
        if g[i, 10] == 1:
            span = g[i + 1:i + 1 + int(g[i, 6])]
            v = span[span[:, 10] == 2][:, :9].reshape(-1, 3)
            g[i, 0:3], g[i, 3:6] = v.min(0), v.max(0)
    sc.arrays = dict(sc.arrays, geometry=g.reshape(-1), lights=base_lights(L).reshape(-1))
    sc.meta = dict(sc.meta, lights=L)
    for a in sc.arrays.values():
        a.setflags(write=False)
    return sc


def _turn(axis, angle):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


@functools.lru_cache(maxsize=None)
def arrays(T, L, k):
    """-> (rotation, shift, lights) of index k.  k = -1: the scene's own.  Otherwise EVERY transform t is turned by TURN x (k + 1) about AXES[t] through the scene's
    centre (the rotation and its inverse as test_walk_lds_gpu._turned forms them; the shift takes the centre's part of the turn, and a step of its own on top), every
    light is moved by a scene radius in a direction of its own and of the frame's, its strength scaled by 1 + 0.5 (k % 3)."""
    sc = scene(T, L)
    if k < 0:
        return sc.arrays["rotation"], sc.arrays["shift"], sc.arrays["lights"]
    r = np.array(sc.arrays["rotation"], np.float32).reshape(-1, 24).copy()
    sh = np.array(sc.arrays["shift"], np.float32).reshape(-1, 8).copy()
    for t in range(T):
        turn = _turn(AXES[t % len(AXES)], TURN * (k + 1))
        m = turn @ np.stack([r[t, 0:3], r[t, 4:7], r[t, 8:11]]).astype(np.float64)
        mi = np.linalg.inv(m)
        for j in range(3):
            r[t, 4 * j:4 * j + 3] = m[j]
            r[t, 12 + 4 * j:12 + 4 * j + 3] = mi[j]
        pos = turn @ (sh[t, 0:3].astype(np.float64) - CENTRE) + CENTRE                     # world = turn (m local + pos - centre) + centre
        pos += 0.25 * (k + 1) * np.array([np.cos(1.9 * t), 0.0 if t == 0 else 0.5, np.sin(1.9 * t)])
        pos += WANDER * np.array([np.cos(2.3 * k + t), 0.4 * np.sin(1.7 * k + t), np.sin(2.3 * k + t)])      # (TURN x 9 is a whole turn and a hundredth: the shifts of frames nine apart differ by more)
        sh[t, 0:3] = pos
        sh[t, 4:7] = -sh[t, 0:3]
    lt = np.array(sc.arrays["lights"], np.float32).reshape(-1, 6).copy()
    for i in range(L):
        a = 2.4 * k + 1.7 * i
        lt[i, 0:3] += np.float32(RADIUS) * np.array([np.cos(a), 0.3 * np.sin(1.3 * k + i), np.sin(a)], np.float32)
        lt[i, 3] *= np.float32(1.0 + 0.5 * (k % 3))
    out = (r.reshape(-1), sh.reshape(-1), lt.reshape(-1))
    for a in out:
        a.setflags(write=False)
    return out


def scene_with(T, L, a, b):
    """the scene with the transforms of index a and the lights of index b"""
    sc = copy.copy(scene(T, L))
    rot, sh, _ = arrays(T, L, a)
    sc.arrays = dict(sc.arrays, rotation=rot, shift=sh, lights=arrays(T, L, b)[2])
    return sc


def params(T, L, shape, f):
    """frame f's view: the camera 0.05 f further along x, random_seed f % 3"""
    w, h, s, b = shape_of(L, shape)
    p = scene(T, L).frame_params(width=w, height=h, samples=s, max_reflections=b, use_filter=0)
    p.camera[0] += 0.05 * f
    p.random_seed = float(f % 3)
    return p


_frames = {}
_spent = [0.0, 0]               # seconds in the oracle, frames it rendered


def oracle_frame(oracle, T, L, shape, a, b, f):
    """the oracle's frame with the transforms of index a, the lights of index b and frame f's view and seed; rendered once, shared, never written"""
    key = (T, L, shape_of(L, shape), a, b if L else -1, f)
    if key not in _frames:
        t0 = time.perf_counter()
        want = oracle.render(scene_with(T, L, a, b), params(T, L, shape, f))[0]
        _spent[0] += time.perf_counter() - t0
        _spent[1] += 1
        want.setflags(write=False)
        _frames[key] = want
    return _frames[key]


def oracle_spent():
    return tuple(_spent)


def differing(a, b):
    """[rows, width] bool: the pixels whose four words differ (NaN equal to NaN of the same bits)"""
    return (np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(-1)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


# ---- sequences ------------------------------------------------------------------------------------------------------------------------------------------------

BOTH, TRANSFORMS, LIGHTS = "both", "transforms", "lights"


class Sequence:
    """N frames of scene(T, L) in `shape`, `depth` frames in flight.  ups[f]: the uploads in front of frame f, [(what, k)] in order; holds[f] = (a, b): the indices of
    the transforms and lights frame f must therefore show.  slots[f]: the slot of the launch frame f was in (the driver fills it in)."""

    def __init__(self, oracle, T, L, shape, depth, ups=None, n=None):
        self.oracle, self.T, self.L, self.shape, self.depth = oracle, T, L, shape, depth
        self.n = n if n is not None else 4 * depth + 1          # every slot of a launch that starts at frame 2 is re-used three times at the least
        if ups is None:                                          # the transforms, and the lights where there are any, in front of every frame from frame 2 on
            ups = [[(BOTH, f)] if f >= 2 else [] for f in range(self.n)]
        assert len(ups) == self.n
        self.ups = ups
        self.holds, a, b = [], -1, -1
        for f in range(self.n):
            for what, k in ups[f]:
                if what in (BOTH, TRANSFORMS):
                    a = k
                if what in (BOTH, LIGHTS):
                    b = k
            self.holds.append((a, b))
        self.slots = [None] * self.n

    def params(self, f):
        return params(self.T, self.L, self.shape, f)

    def frame(self, g, f):
        """the oracle's frame of frame g's arrays with frame f's view and seed"""
        a, b = self.holds[g]
        return oracle_frame(self.oracle, self.T, self.L, self.shape, a, b, f)

    def want(self, f):
        return self.frame(f, f)

    def first_moved(self):
        """the first frame in front of which arrays go up that differ from the ones in force"""
        for f in range(self.n):
            if self.holds[f] != (self.holds[f - 1] if f else (-1, -1)):
                return f
        return self.n

    def upload(self, hip, what, k):
        rot, sh, lt = arrays(self.T, self.L, k)
        if what in (BOTH, TRANSFORMS):
            hip.update_transforms(rot, sh)
        if what in (BOTH, LIGHTS) and self.L:
            hip.update_primary_light_sources(lt)

    def restore(self, hip):
        self.upload(hip, BOTH, -1)


def classify(got, f, wants):
    """What does the wrong frame f show?  `wants`: the Sequence (its holds, depth and slots; its frame(g, f) renders the alternatives — only now, when a frame has
    failed).  -> one line for the assertion's message: the count of differing pixels, the slot, and whether the frame is bit for bit the one of the arrays of frame
    f - depth (the slot's occupant before: a STALE VERSION), of frame f - 1 or f + 1 (the WRONG POST), each with frame f's own view and seed, or none of these."""
    want = wants.want(f)
    if got.shape != want.shape:
        return "frame %d: shape %s, not %s" % (f, got.shape, want.shape)
    diff = differing(got, want)
    slot = wants.slots[f] if wants.slots[f] is not None else f % wants.depth
    head = "frame %d (slot %d of %d; transforms %d, lights %d): %d of %d pixels differ from the oracle's" % (
        (f, slot, wants.depth) + tuple(wants.holds[f]) + (int(diff.sum()), diff.size))
    if not diff.any():
        return head + " — the frame is right"
    names = ((f - wants.depth, "a STALE VERSION: the arrays of frame %d, the slot's occupant before"),
             (f - 1, "the WRONG POST: the arrays of frame %d, the one before"),
             (f + 1, "the WRONG POST: the arrays of frame %d, the one after"))
    found = []
    for g, text in names:
        if 0 <= g < wants.n and wants.holds[g] != wants.holds[f] and same(got, wants.frame(g, f)):
            found.append(text % g)
    if found:
        return head + "; it is bit for bit " + " and ".join(found) + " (with its own view and seed)"
    others = [g for g in range(wants.n) if wants.holds[g] != wants.holds[f] and same(got, wants.frame(g, f))]
    if others:
        return head + "; it is bit for bit the frame of the arrays of frame %s (with its own view and seed)" % others
    rows = np.flatnonzero(diff.any(1))
    cols = np.flatnonzero(diff.any(0))
    return head + "; none of these (a mix): rows %d .. %d, columns %d .. %d, %d of the %d screen tiles" % (
        rows[0], rows[-1], cols[0], cols[-1], len({(y // 8, x // 8) for y, x in zip(*np.nonzero(diff))}), ((diff.shape[0] + 7) // 8) * ((diff.shape[1] + 7) // 8))


# ---- the frame loop ---------------------------------------------------------------------------------------------------------------------------------------------

STEADY, BATCHES, SINGLE, SYNCED, PAUSED = "steady", "batches", "single", "synced", "paused"


def run(hip, seq, pacing=STEADY, rgba8=False, before_drain=None):
    """The frames of `seq` through the frame loop.  STEADY: end the oldest when `depth` are in flight, upload, begin; BATCHES: begin `depth`, end them all; SINGLE:
    begin and end one at a time; SYNCED: steady, flx_sync after every second begin; PAUSED: steady, 50 ms of host pause in front of the uploads.
    before_drain(): called after the last begin, with the last frames still in flight.  seq.around: (f, server_moving() before, after) of every upload.
    -> (frames, last_chained() after every begin, server_moving() after every begin); seq.slots is filled in (flx_api.hip, server_post: a launch that starts
    on an empty loop starts in slot 0, every other one goes on counting)"""
    got, kinds, flags = [], [], []
    next_slot, seq.around = 0, []

    def end():
        got.append(hip.frame_end()[0].copy())
    for f in range(seq.n):
        if pacing == BATCHES:
            if f % seq.depth == 0:
                while hip.frames_in_flight():
                    end()
        elif pacing == SINGLE:
            while hip.frames_in_flight():
                end()
        elif hip.frames_in_flight() == seq.depth:
            end()
        if pacing == PAUSED and seq.ups[f]:
            time.sleep(0.05)
        for what, k in seq.ups[f]:
            before = hip.server_moving()
            seq.upload(hip, what, k)
            seq.around.append((f, before, hip.server_moving()))
        empty = hip.frames_in_flight() == 0
        hip.frame_begin(seq.params(f), rgba8=rgba8)
        kinds.append(hip.last_chained())
        flags.append(hip.server_moving())
        if kinds[-1] == 3:
            seq.slots[f] = 0 if empty else next_slot
            next_slot = (seq.slots[f] + 1) % seq.depth
        if pacing == SYNCED and f % 2 == 1:
            hip.sync()
    if before_drain:
        before_drain()
    while hip.frames_in_flight():
        end()
    return got, kinds, flags


def wrong_frames(got, seq, present=None):
    """-> [classify's line for every frame that is not the oracle's bit for bit (present: the oracle's quantisation, for RGBA8 frames)]"""
    lines = []
    for f in range(seq.n):
        want = seq.want(f)
        if present is not None:
            if not same(got[f], present(want)):
                lines.append("frame %d: %d of %d RGBA8 pixels differ from the oracle's" % (f, int((got[f] != present(want)).any(-1).sum()), want.shape[0] * want.shape[1]))
        elif not same(got[f], want):
            lines.append(classify(got[f], f, seq))
    return lines


class knobs:
    """the frame loop's knobs for a case, every one of them put back afterwards, and the scene's own transforms and lights with them"""

    def __init__(self, hip, seq, chain=3, groups=0):
        self.hip, self.seq, self.chain, self.groups = hip, seq, chain, groups

    def __enter__(self):
        hip, seq = self.hip, self.seq
        hip.update_scene(scene(seq.T, seq.L))
        hip.set_server_groups(self.groups)
        hip.set_server_moving_scenes(1)
        hip.set_frame_chain(self.chain)
        hip.set_frame_lanes(seq.depth)
        hip.frame_begin(seq.params(0))                       # (the frame that follows update_scene itself goes to the lanes)
        hip.frame_end()
        return self

    def __exit__(self, *exc):
        hip = self.hip
        try:
            while hip.frames_in_flight():
                hip.frame_end()
        finally:
            hip.set_server_groups(0)
            hip.set_frame_lanes(2)
            hip.set_frame_chain(2)
            hip.set_server_moving_scenes(1)
            self.seq.restore(hip)
        return False
