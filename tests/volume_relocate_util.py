"""Helpers of the probe-relocation tests (test_volume_relocate_cpu.py, test_volume_relocate_gpu.py): the CPU reference built once per session, synthetic HIT and
NORMAL planes that hold every rule, ties across and within lanes, empties and poison, a float64 restatement of include/flx_volume_relocate.h's reduction and move
written by hand, and an analytic room — an axis-aligned box seen from inside with a solid box in it — whose ray distances and front/back verdicts are computed in
numpy."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "volume_relocate_ref"))
import flx_volume_relocate_ref  # noqa: E402

from probe_util import SPARE, assert_same_words, finished, poisoned, quadrature64  # noqa: E402,F401
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
