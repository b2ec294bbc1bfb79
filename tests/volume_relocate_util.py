"""Helpers of the probe-relocation tests (test_volume_relocate_cpu.py, test_volume_relocate_gpu.py, test_volume_relocate_seams_gpu.py): the CPU reference built once per
session, synthetic HIT and NORMAL planes that hold every rule, ties across and within lanes, empties and poison, planes of large faces whose winning texels the caller
places, planes of tens of thousands of probes made without a loop over probes, a float64 restatement of include/flx_volume_relocate.h's reduction and move
written by hand, and an analytic room — an axis-aligned box seen from inside with a solid box in it — whose ray distances and front/back verdicts are computed in
numpy."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "volume_relocate_ref"))
import flx_volume_relocate_ref  # noqa: E402

import probe_util  # noqa: E402
from probe_util import SPARE, assert_same_words, finished, poisoned  # noqa: E402,F401
from volume_map_util import assert_same_rows, map_of, synthetic_maps  # noqa: E402,F401
from volume_util import ORIGIN, SPACING, grid_of, synthetic_sh  # noqa: E402,F401

INACTIVE, REJECTED = 1, 8
FREEZE = 1
POISON = 0xA5A5A5A5
FACES = (1, 2, 3, 4, 5, 8, 11, 16)            # R = 6, 24, 54 (lanes without a texel), 96, 150, 384, 726, 1536
PROBE_COUNTS = (1, 3, 4, 5, 9)                # the last workgroup part full
# what a probe's planes are made to hold, probe i getting FLAVOURS[(i + seed) % len]
FLAVOURS = ("inside", "near_wall", "open", "near_corner", "no_hits", "all_back", "all_grazing", "poison_s", "ties", "far", "inside_far", "old_nan")

_ref = []
_quadrature = {}


def quadrature64(face_size):
    """probe_util.quadrature64, kept per face size: the generators and relocate64 ask for it once a probe, and at face size 256 it is 393 216 rows"""
    if face_size not in _quadrature:
        _quadrature[face_size] = probe_util.quadrature64(face_size)
    return _quadrature[face_size]


def reference(tmp_path_factory):
    """the CPU reference, built once per session"""
    if not _ref:
        _ref.append(flx_volume_relocate_ref.build(str(tmp_path_factory.mktemp("volume_relocate_ref"))))
    return _ref[0]


def relocate_of(back_share=0.26, min_front=0.25, reach=4.0, limit=0.45, flags=0, reserved=0):
    from flexlight_hip import capi
    return capi.VolumeRelocate(back_share, min_front, reach, limit, flags, reserved)


def states_of(offsets):
    return np.ascontiguousarray(offsets, np.float32).reshape(-1, 4)[:, 3].copy().view(np.uint32)


def rule_of(states):
    return (np.asarray(states, np.uint32) >> 1) & 3


def planes_of(s, side, hit):
    """s float [n], side float [n] (the NORMAL plane's word 3), hit bool [n] -> (HIT plane, NORMAL plane) float32 [n, 4]; a miss row is zeros with -1 in word 3"""
    n = len(s)
    rng = np.random.default_rng(n)
    h, nn = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    h[:, 0] = s
    h[:, 1:3] = rng.uniform(0.0, 1.0, size=(n, 2))           # u, v: not read
    h.view(np.uint32)[:, 3] = rng.integers(0, 1000, size=n)
    nn[:, 0:3] = rng.normal(size=(n, 3))                     # the normal itself: not read
    nn[:, 3] = side
    h[~hit] = 0.0
    h.view(np.uint32)[~hit, 3] = 0xffffffff
    nn[~hit] = 0.0
    return h, nn


def synthetic_probe(face_size, flavour, rng, relocate):
    """one probe's (s, side, hit, old offset float32 [4]) of a FLAVOUR.  Distances are multiples of 1/64 away from min_front and reach by at least 1/128, so that the
    float64 restatement finds no threshold close; "ties" quantises them to 1/4 so that many texels share the least and the greatest."""
    rays = 6 * face_size * face_size
    d, _, _ = quadrature64(face_size)
    mf = float(relocate.min_front)
    grid64 = lambda lo, hi: (np.floor(rng.uniform(lo, hi, size=rays) * 64.0) + 0.5) / 64.0      # noqa: E731
    s = grid64(mf + 0.05, 3.0)
    side = -np.ones(rays)
    hit = rng.random(rays) < 0.8
    old = np.zeros(4, np.float32)
    old.view(np.uint32)[3] = rng.integers(0, 16)              # an earlier state: not read
    if flavour == "inside":              # most texels see back faces, close by
        side = np.where(rng.random(rays) < 0.7, 1.0, -1.0)
        s = grid64(0.01, 0.2)
        old[:3] = rng.uniform(-0.05, 0.05, size=3)
    elif flavour == "inside_far":        # ... whose closest back face is beyond every limit: rejected
        side = np.where(rng.random(rays) < 0.9, 1.0, -1.0)
        s = grid64(2.0, 3.0)
    elif flavour == "near_wall":         # a wall at -x within min_front, the room open at +x: the farthest front lies across from the closest (their dot is < 0)
        near, across = d[:, 0] < -0.6, d[:, 0] > 0.6
        s = np.where(near, grid64(0.01, mf - 0.02), np.where(across, grid64(mf + 0.2, mf + 0.25), grid64(mf + 0.05, mf + 0.15)))
        hit = hit | near | across
    elif flavour == "near_corner":       # everything near, the closest and the farthest front both on the +z face: their dot is 1, 2/3 or 1/3 at w = 2, never the 1/2
        top = d[:, 2] > 0.6              # two texels of neighbouring faces can have — rule 2 with no move where it is above 1/2
        low = rng.random(rays) < 0.5
        s = np.where(top, np.where(low, grid64(0.01, 0.05), grid64(mf - 0.07, mf - 0.02)), grid64(0.08, mf - 0.1))
        hit = hit | top
    elif flavour == "open":              # nothing near, a displaced probe
        old[:3] = rng.uniform(-0.3, 0.3, size=3)
    elif flavour == "far":               # nothing within reach
        s = grid64(float(relocate.reach) + 0.1, float(relocate.reach) + 3.0)
        old[:3] = rng.uniform(-0.1, 0.1, size=3)
    elif flavour == "no_hits":
        hit[:] = False
        old[:3] = rng.uniform(-0.2, 0.2, size=3)
    elif flavour == "all_back":
        side[:] = 1.0
        hit[:] = True
        s = grid64(0.01, 0.3)
    elif flavour == "all_grazing":
        side = rng.choice(np.array([0.0, -0.0, np.nan]), size=rays)
        hit[:] = True
    elif flavour == "poison_s":          # NaN, negative and infinite distances among good ones, front and back
        side = np.where(rng.random(rays) < 0.3, 1.0, -1.0)
        bad = rng.choice(np.array([np.nan, -1.0, -np.inf, np.inf, -0.0]), size=rays)
        s = np.where(rng.random(rays) < 0.5, bad, s)
    elif flavour == "ties":
        s = np.floor(rng.uniform(mf + 0.3, 2.0, size=rays) * 4.0) / 4.0 + 1.0 / 128.0
        side = np.where(rng.random(rays) < 0.2, 1.0, -1.0)
        old[:3] = rng.uniform(-0.2, 0.2, size=3)
    elif flavour == "old_nan":
        old[int(rng.integers(0, 3))] = np.nan
    else:
        raise ValueError(flavour)
    return s, side, hit, old


def synthetic_case(n_probes, face_size, seed, relocate):
    """-> (HIT plane float32 [n R, 4], NORMAL plane float32 [n R, 4], old offset rows float32 [n, 4], flavours [n])"""
    rng = np.random.default_rng(1000 * seed + face_size)
    hits, normals, olds, flavours = [], [], [], []
    for i in range(n_probes):
        flavour = FLAVOURS[(i + seed) % len(FLAVOURS)]
        s, side, hit, old = synthetic_probe(face_size, flavour, rng, relocate)
        h, nn = planes_of(s, side, hit)
        hits.append(h), normals.append(nn), olds.append(old), flavours.append(flavour)
    return np.concatenate(hits), np.concatenate(normals), np.stack(olds), flavours


# ---- placed winners: large faces (test_volume_relocate_cpu.py, test_volume_relocate_seams_gpu.py) ---------------------------------------------------------------
# synthetic_probe's distances are quantised to 1/64, so among the 2 400 .. 393 216 texels of a large face the extreme is always tied and the lowest t wins early: no
# winning texel of those inputs is above R / 6.  Here the caller names the texels that win.

LARGE = ((20, (1, 5)), (32, (1, 5)), (48, (1, 5)), (64, (1, 5)), (128, (1, 5)), (256, (1, 3)))      # test_probe_seams_gpu.py's LARGE_SUMS and its reasoning, from 20 on
KEYS = ("cb", "cf", "ff")                      # the closest back, the closest front, the farthest front


def placed_texels(face_size):
    """the texels at which a key can go wrong, those that exist for R = 6 w w: the first trip's ends and the second's start, the last trip's first texel and R - 1 (the
    last texel that has a lane in the last trip: lane 31 at w = 20), either side of 2^16, 2^17 and 2^18, and 393 215"""
    rays = 6 * face_size * face_size
    named = (0, 63, 64, rays - 1, (rays - 1) // 64 * 64, 65535, 65536, 131071, 131072, 262143, 262144, 393215)
    return sorted({t for t in named if t < rays})


def placed_distances(relocate, rule):
    """the distances placed_probe gives the three winners under that rule -> {"cb", "cf", "ff"}: float64 on the 1/64 grid, (k + 0.5) / 64.
      1  the backs are 0.6 of the texels, the closest 1.5 / 64 away; the fronts lie beyond min_front
      2  the backs are 0.1 of the texels; every front is nearer than min_front, the farthest of them 3.5 / 64 short of it: the step is that distance
      3  the backs are 0.1 of the texels; the closest front is 2.5 / 64 beyond min_front, which is the way back a displaced probe is allowed"""
    mfk = float(relocate.min_front) * 64.0
    assert mfk.is_integer() and (float(relocate.reach) * 64.0).is_integer() and 10 <= mfk <= 100 and float(relocate.reach) >= 3.0      # every grid value is 1/128 away from both
    mfk = int(mfk)
    k = {1: (1, mfk + 3, 191), 2: (1, 2, mfk - 4), 3: (1, mfk + 2, 191)}[rule]
    return {name: (kk + 0.5) / 64.0 for name, kk in zip(KEYS, k)}


def placed_probe(face_size, rng, relocate, winners):
    """one probe's (s, side, hit, old offset float32 [4]) whose three keys are won where the caller says.  winners: {"rule": 1, 2 or 3, "cb", "cf", "ff": the winning
    texels (three different ones), "ties": {key: texels above the winner that share its distance and its side}}.  Every other ranked distance is strictly worse than
    its winner's; about a fifth of the other texels are misses.  Rule 2 moves or not by the two texels the caller picked: their float64 dot is at least 0.05 away
    from 0.5, asserted here.  The old offset is small enough for the move to be accepted on volume_util's grid at limit 0.45."""
    rays = 6 * face_size * face_size
    rule, ties = winners["rule"], winners.get("ties", {})
    placed = placed_distances(relocate, rule)
    k = {name: int(placed[name] * 64.0) for name in KEYS}
    cb, cf, ff = (winners[name] for name in KEYS)
    assert len({cb, cf, ff}) == 3 and max(cb, cf, ff) < rays
    back = rng.random(rays) < (0.6 if rule == 1 else 0.1)
    assert 0.1 + 0.05 < float(relocate.back_share) < 0.6 * 0.8 - 0.1            # (a fifth of either share are misses)
    hit = rng.random(rays) < 0.8
    ks = np.where(back, rng.integers(k["cb"] + 1, 13, size=rays), rng.integers(k["cf"] + 1, k["ff"], size=rays))      # strictly between the winners
    for name in KEYS:
        members = [winners[name]] + list(ties.get(name, ()))
        assert all(winners[name] < t < rays for t in members[1:])
        ks[members], back[members], hit[members] = k[name], name == "cb", True
    assert (ks[[cb, cf, ff]] == [k[name] for name in KEYS]).all()          # (no tie overwrote another key's winner)
    if rule == 2:
        d, _, _ = quadrature64(face_size)
        dot = float(d[cf] @ d[ff])
        assert abs(dot - 0.5) >= 0.05 and (dot <= 0.5) == bool(winners["move"]), (cf, ff, dot)
    old = np.zeros(4, np.float32)
    old[:3] = rng.uniform(-0.1, 0.1, size=3) if rule == 3 else rng.uniform(-0.01, 0.01, size=3)
    old.view(np.uint32)[3] = rng.integers(0, 16)
    return (ks + 0.5) / 64.0, np.where(back, 1.0, -1.0), hit, old


def _partner(face_size, t, move, taken):
    """a texel whose direction's dot with texel t's is <= 0.45 (move) or >= 0.55 (no move): a named texel where one will do, else one from the middle of those that do"""
    d, _, _ = quadrature64(face_size)
    dots = d @ d[t]
    good = (dots <= 0.45) if move else (dots >= 0.55)
    good[list(taken)] = False
    for other in placed_texels(face_size):
        if good[other]:
            return other
    found = np.flatnonzero(good)
    return int(found[len(found) // 2])


def placed_winners(face_size):
    """the placed cases of a face size -> a list of placed_probe's winners, each with "key" (which of KEYS the case is about) and "texel" (where it is won).  Every
    texel of placed_texels wins the closest back under rule 1 (its direction is the move's), the closest front and the farthest front under rule 2 with a move (both
    directions are read), and a fourth time, by its place in the list: the closest or the farthest front, under rule 2 without a move or under rule 3.  The other two
    keys are won at named texels too where the rule allows.  Each winner is tied with the texels 1, 64 and 197 above it that exist and are free: another lane, the
    same lane's next trip, another lane three trips on."""
    rays = 6 * face_size * face_size
    texels = placed_texels(face_size)
    cases = []
    for i, t in enumerate(texels):
        others = [x for x in texels[i + 1:] + texels[:i]]
        for key, rule, move in (("cb", 1, None), ("cf", 2, True), ("ff", 2, True), (("cf", 2, False), ("cf", 3, None), ("ff", 2, False), ("ff", 3, None))[i % 4]):
            w = {"rule": rule, "move": move, "key": key, "texel": t, key: t}
            if rule == 2:
                w["ff" if key == "cf" else "cf"] = _partner(face_size, t, move, {t})
            for name in KEYS:
                if name not in w:
                    w[name] = next(x for x in others if x not in [w.get(n) for n in KEYS])
            taken = {w[name] for name in KEYS}
            w["ties"] = {}
            for name in KEYS:
                w["ties"][name] = [x for x in (w[name] + 1, w[name] + 64, w[name] + 197) if x < rays and x not in taken]
                taken.update(w["ties"][name])
            cases.append(w)
    return cases


FLAVOURS_SEAM = ("inside", "near_wall", "open", "far", "no_hits", "all_back")


def seam_planes(n_probes, face_size, seed, relocate=None):
    """synthetic_case for tens of thousands of probes of a small face, without a loop over probes: probe i's flavour is FLAVOURS_SEAM[(i + seed) % 6].
    -> (HIT plane float32 [n R, 4], NORMAL plane float32 [n R, 4], old offset rows float32 [n, 4], flavour index [n]).  The flavours are synthetic_probe's, but for
    "open", whose closest front leaves a displaced probe less than the whole way back, and for an old offset within 0.02 where synthetic_probe's is zero: no two old
    rows are alike, and no two probes' planes are but those of probes without a hit (asserted)."""
    rays = 6 * face_size * face_size
    relocate = relocate or relocate_of()
    rng = np.random.default_rng(100000 * seed + 100 * face_size + n_probes % 97)
    d, _, _ = quadrature64(face_size)
    mf, reach = float(relocate.min_front), float(relocate.reach)
    flavour = ((np.arange(n_probes) + seed) % len(FLAVOURS_SEAM))[:, None]
    is_ = lambda name: flavour == FLAVOURS_SEAM.index(name)                                                         # noqa: E731
    grid64 = lambda lo, hi: (np.floor(rng.uniform(lo, hi, size=(n_probes, rays)) * 64.0) + 0.5) / 64.0      # noqa: E731
    near, across = (d[:, 0] < -0.6)[None, :], (d[:, 0] > 0.6)[None, :]
    s = grid64(mf + 0.05, 3.0)
    s = np.where(is_("inside"), grid64(0.01, 0.2), s)
    s = np.where(is_("near_wall"), np.where(near, grid64(0.01, mf - 0.02), np.where(across, grid64(mf + 0.2, mf + 0.25), grid64(mf + 0.05, mf + 0.15))), s)
    s = np.where(is_("open"), grid64(mf + 0.02, mf + 0.12), s)
    s = np.where(is_("far"), grid64(reach + 0.1, reach + 3.0), s)
    s = np.where(is_("all_back"), grid64(0.01, 0.3), s)
    side = np.where(is_("inside") & (rng.random((n_probes, rays)) < 0.7) | is_("all_back"), 1.0, -1.0)
    hit = rng.random((n_probes, rays)) < 0.8
    hit = (hit | is_("all_back") | (is_("near_wall") & (near | across))) & ~is_("no_hits")
    width = np.select([is_("inside"), is_("open"), is_("far"), is_("no_hits")], [0.05, 0.3, 0.1, 0.2], 0.02)
    old = np.zeros((n_probes, 4), np.float32)
    old[:, :3] = rng.uniform(-1.0, 1.0, size=(n_probes, 3)) * width
    old.view(np.uint32)[:, 3] = rng.integers(16, 32, size=n_probes)          # an earlier state that no call writes: every row of a run changes
    h, nn = planes_of(s.reshape(-1), side.reshape(-1), hit.reshape(-1))
    assert len(np.unique(old.view(np.uint32)[:, :3], axis=0)) == n_probes
    seen = hit.any(axis=1)
    both = np.concatenate([h.view(np.uint32).reshape(n_probes, -1), nn.view(np.uint32).reshape(n_probes, -1)], axis=1)[seen]
    assert len(np.unique(both, axis=0)) == len(both)
    return h, nn, old, flavour[:, 0]


def relocate64(grid, relocate, face_size, hit, normal, old):
    """The reduction and the move of include/flexlight_hip_debug.h ("probe relocation") restated by hand in float64 over the same float32 inputs, one probe.
    -> (new offset float64 [3], state, margin): margin is the least relative distance of a comparison's two sides over the thresholds that decided the rule, the
    acceptance and the state (inf where none was asked)"""
    rays = 6 * face_size * face_size
    d, _, _ = quadrature64(face_size)
    hit, normal = np.asarray(hit, np.float32).reshape(rays, 4), np.asarray(normal, np.float32).reshape(rays, 4)
    is_hit = hit.view(np.uint32)[:, 3] != 0xffffffff
    s = hit[:, 0].astype(np.float64)
    side = normal[:, 3].astype(np.float64)
    with np.errstate(invalid="ignore"):
        back, front, ranks = is_hit & (side > 0), is_hit & (side < 0), s >= 0
    s = np.where(s == 0.0, 0.0, s)
    margin = [np.inf]

    def close(a, b):
        scale = max(abs(a), abs(b))
        if scale > 0 and np.isfinite(scale):
            margin[0] = min(margin[0], abs(a - b) / scale)

    def least(mask, sign):
        cand = np.flatnonzero(mask & ranks)
        if cand.size == 0:
            return None
        t = cand[np.argmin(sign * s[cand])]             # (the first of equals: the lowest t)
        return float(s[t]), int(t)

    B, R = int(back.sum()), rays
    bs, mf, reach, limit = float(relocate.back_share), float(relocate.min_front), float(relocate.reach), float(relocate.limit)
    inside = B > bs * R
    close(float(B), bs * R)
    cb, cf, ff = least(back, 1.0), least(front, 1.0), least(front, -1.0)
    o = np.asarray(old, np.float32)[:3].astype(np.float64)
    moved = o.copy()
    if inside and cb is not None:
        rule = 1
        moved = o + d[cb[1]] * (cb[0] + mf * 0.5)
    elif cf is not None and cf[0] < mf:
        rule = 2
        dot = float(d[cf[1]] @ d[ff[1]])
        close(dot, 0.5)
        if dot <= 0.5:
            moved = o + d[ff[1]] * min(ff[0], mf)
    else:
        rule = 3
        if cf is not None:
            close(cf[0], mf)
        length = float(np.sqrt((o * o).sum()))
        m = min(cf[0] - mf, length) if cf is not None else length
        if length > 0:
            moved = o - (o / length) * m
    spacing = np.array(list(grid.spacing), np.float64)
    accepted = bool(np.isfinite(moved).all())
    if accepted:
        for a in range(3):
            close(abs(moved[a]), limit * spacing[a])
        accepted = bool((np.abs(moved) <= limit * spacing).all())
    lit = cf is not None and cf[0] <= reach
    if cf is not None:
        close(cf[0], reach)
    state = (INACTIVE if inside or not lit else 0) | (rule << 1) | (0 if accepted else REJECTED)
    keep = not accepted or (int(relocate.flags) & FREEZE)
    return (o if keep else moved), state, margin[0]


# ---- the analytic room -----------------------------------------------------------------------------------------------------------------------------------

ROOM = (np.array([-2.0, -2.0, -2.0]), np.array([2.0, 2.0, 2.0]))            # seen from inside


def _slab(origin, d, lo, hi):
    """ray against an axis-aligned box in float64 -> (t_enter, t_exit) per ray; no hit where t_enter > t_exit"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - origin) / d, (hi - origin) / d
    near, far = np.minimum(t0, t1), np.maximum(t0, t1)
    near, far = np.where(np.isnan(near), -np.inf, near), np.where(np.isnan(far), np.inf, far)
    return near.max(axis=1), far.min(axis=1)


def room_planes(position, face_size, solid):
    """The HIT and NORMAL planes a probe at `position` sees in ROOM with the solid box `solid` = (lo, hi) in it.  From inside the solid box the first hit is the box's
    inner side, a BACK face (+1); outside it the box's near side or the room's wall, FRONT faces (-1)."""
    d, _, _ = quadrature64(face_size)
    position = np.asarray(position, np.float64)
    rays = len(d)
    enter, leave = _slab(position, d, solid[0], solid[1])
    _, wall = _slab(position, d, ROOM[0], ROOM[1])
    in_solid = bool(((position > solid[0]) & (position < solid[1])).all())
    if in_solid:
        s, side = leave, np.ones(rays)
    else:
        box = (enter <= leave) & (enter > 0)
        s, side = np.where(box, enter, wall), -np.ones(rays)
    return planes_of(s.astype(np.float32), side, np.ones(rays, bool))


def room_iterate(ref, grid, relocate, face_size, solid, probe, offset, passes):
    """`passes` passes of the reference over the one probe `probe` of the grid, then a frozen one -> (offsets after each pass float32 [passes + 1, 4], back shares
    seen by each pass [passes + 1])"""
    from flexlight_hip import capi
    lattice = ref.positions(grid, np.zeros((grid.probes, 4), np.float32))[probe, :3].astype(np.float64)
    offsets = np.zeros((grid.probes, 4), np.float32)
    offsets[probe] = offset
    rows, shares = [], []
    for k in range(passes + 1):
        h, nn = room_planes(lattice + offsets[probe, :3].astype(np.float64), face_size, solid)
        shares.append(float((nn[:, 3] > 0).mean()))
        r = relocate if k < passes else capi.VolumeRelocate(relocate.back_share, relocate.min_front, relocate.reach, relocate.limit, FREEZE)
        offsets = ref.relocate(grid, r, face_size, h, nn, offsets, first_probe=probe)
        rows.append(offsets[probe].copy())
    return np.stack(rows), shares


def device_words(words, spare_words):
    """a host array as uint32 words on the device with spare_words of poison behind it"""
    import torch
    words = np.ascontiguousarray(words).view(np.uint32).reshape(-1)
    return torch.from_numpy(np.concatenate([words, np.full(spare_words, POISON, np.uint32)]).view(np.int32)).cuda()


def back(ctx, tensor, words, width):
    """a device array after the call -> its first `words` words as uint32 [.., width]: the spare words behind them kept their poison"""
    ctx.sync()
    got = tensor.cpu().numpy().view(np.uint32).reshape(-1)
    assert (got[words:] == POISON).all()
    return got[:words].reshape(-1, width)
