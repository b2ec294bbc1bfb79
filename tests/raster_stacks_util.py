"""Hand-made layer stacks for the rasterizer's one-walk depth test (k_raster, flx_raster.hip): scenes whose every pixel has a fragment list chosen on
purpose, an emulation of the loop head of k_raster's wave (which trips it makes, when it stops walking in lockstep), and the case list that
tests/test_raster_stacks_cpu.py checks for what it reaches and tests/test_raster_stacks_gpu.py runs on the GPU.  TEST INFRASTRUCTURE ONLY.

A scene is a flat entry list padded to 256 rows; the camera sits at the origin and looks along +z with an identity view matrix, so that the ray of the
pixel with centre (nx, ny) in [-1, 1]^2 meets the plane z = c at (nx c, ny c, c).  Entry order is draw order."""
import collections
import os
import re

import numpy as np

from flexlight_hip.scene_io import FrameParams, Scene

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "web-ray-tracer_amd", "csrc")

PALETTE = [(1.0, 1.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.25, 0.5, 1.0), (1.0, 1.0, 0.0), (0.0, 1.0, 1.0), (1.0, 0.5, 0.25), (0.5, 0.25, 1.0)]


# -- entries --------------------------------------------------------------------------------------------------------------------------
def tri(verts, tpo=0.0, albedo=(1.0, 1.0, 1.0), emissive=0.5, normal=(0.0, 0.0, -1.0), tpo_tex=-1.0, flip=False):
    """one triangle entry: nine vertex floats, material.tpo.x (alpha = 1 - tpo / 2), albedo, emissive value, a flat normal; tpo_tex >= 0: tpo from the
    atlas texel instead of the attribute; flip: the other winding (the same coverage: nothing is culled; a shadow ray meets only one facing)"""
    geo = np.zeros(12, np.float32)
    v = np.asarray(verts, np.float32).reshape(3, 3)
    geo[0:9] = (v[[0, 2, 1]] if flip else v).reshape(-1)
    geo[10] = 2
    att = np.zeros(28, np.float32)
    att[0:9] = list(normal) * 3
    att[15:18] = [-1, -1, tpo_tex]
    att[18:21] = albedo
    att[21:24] = [1, 0, emissive]
    att[24:27] = [tpo, 0, 1]
    return ("tri", geo, att)


def layer(z, tpo=0.0, albedo=(1.0, 1.0, 1.0), emissive=0.5, cover="full", edge=0.0, **kw):
    """one large triangle at constant z.  cover: 'full', or the half plane 'left' / 'right' / 'top' / 'bottom' whose edge runs through the pixel centres
    with nx = edge (left, right) or ny = edge (top, bottom; ny counts upwards): edge = 0 is the image centre"""
    e = edge * z
    verts = {"full": [-100, -100, z, 300, -100, z, -100, 300, z],
             "right": [e, -100, z, e + 300, -100, z, e, 300, z],
             "left": [e, -100, z, e - 300, -100, z, e, 300, z],
             "top": [-100, e, z, 300, e, z, -100, e + 300, z],
             "bottom": [-100, e, z, 300, e, z, -100, e - 300, z]}[cover]
    return tri(verts, tpo, albedo, emissive, **kw)


def patch(z, x0, y0, x1, y1, **kw):
    """a small right triangle at constant z over the pixel centres with nx >= x0, ny >= y0 and (nx - x0) / (x1 - x0) + (ny - y0) / (y1 - y0) <= 1"""
    return tri([x0 * z, y0 * z, z, x1 * z, y0 * z, z, x0 * z, y1 * z, z], **kw)


def box(children):
    """a box row in front of its children's rows, with their bounds and their number of rows as its skip count"""
    return ("box", list(children))


def _flatten(entries, geo, att):
    lo = hi = None
    for e in entries:
        if e[0] == "tri":
            geo.append(e[1]); att.append(e[2])
            v = e[1][0:9].reshape(3, 3)
            clo, chi = v.min(0), v.max(0)
        else:
            at = len(geo)
            geo.append(None); att.append(np.zeros(28, np.float32))
            clo, chi = _flatten(e[1], geo, att)
            g = np.zeros(12, np.float32)
            g[0:3], g[3:6] = clo, chi
            g[6] = len(geo) - at - 1
            g[10] = 1
            geo[at] = g
        lo = clo if lo is None else np.minimum(lo, clo)
        hi = chi if hi is None else np.maximum(hi, chi)
    return lo, hi


def stack_scene(entries, width, height, lights=(), tpo_texel=None, hdr=0):
    """entries in draw order -> (Scene, FrameParams): 256 rows, one identity transform, 1 x 1 atlases (tpo_texel: the tpo atlas' texel's first byte),
    lights [[x, y, z, strength], ...], no ambient light"""
    geo, att = [], []
    _flatten(entries, geo, att)
    assert 0 < len(geo) < 256
    geometry = np.zeros((256, 12), np.float32)
    attributes = np.zeros((256, 28), np.float32)
    geometry[:len(geo)] = np.stack(geo)
    attributes[:len(att)] = np.stack(att)
    rotation = np.zeros(24, np.float32)
    for r in range(3):
        rotation[4 * r + r] = rotation[12 + 4 * r + r] = 1
    lt = np.zeros((len(lights), 6), np.float32)
    for k, l in enumerate(lights):
        lt[k, 0:4] = l
    tex = np.zeros(4, np.uint8)
    if tpo_texel is not None:
        tex[0] = tpo_texel
    meta = {"atlas": {"albedo": [1, 1], "pbr": [1, 1], "tpo": [1, 1]}}
    arrays = {"geometry": geometry.reshape(-1), "attributes": attributes.reshape(-1),
              "ids": np.flatnonzero(geometry[:, 10] == 2).astype(np.int32),
              "rotation": rotation, "shift": np.zeros(8, np.float32), "lights": lt.reshape(-1),
              "atlasAlbedo": np.zeros(4, np.uint8), "atlasPbr": np.zeros(4, np.uint8), "atlasTpo": tex}
    p = FrameParams()
    p.width, p.height = width, height
    p.view_matrix[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]              # camera at the origin looking along +z
    p.samples, p.hdr, p.texture_width = 1, hdr, 1
    return Scene(meta, arrays), p


def two_layer_scene(near_first):
    """Two large triangles facing the camera at depths 5 (near) and 10 (far), both translucent (tpo.x = 1: alpha 0.5), emissive 0.5, no
    lights, no ambient; near: albedo (1, 1, 1), far: albedo (1, 0, 0).  Entry order = draw order."""
    layers = [layer(5, 1, (1, 1, 1)), layer(10, 1, (1, 0, 0))]
    return stack_scene(layers if near_first else layers[::-1], 5, 3)


# -- the wave of k_raster ---------------------------------------------------------------------------------------------------------------
def lock_min():
    """FLX_PRIMARY_LOCK_MIN as the library is built: flx_device.h's default, which the Makefile must not override"""
    text = open(os.path.join(CSRC, "flx_device.h")).read()
    found = re.findall(r"^#define\s+FLX_PRIMARY_LOCK_MIN\s+(\d+)", text, re.M)
    assert len(found) == 1, found
    assert "FLX_PRIMARY_LOCK_MIN" not in open(os.path.join(CSRC, "Makefile")).read()
    return int(found[0])


def tile_lanes(width, height, tile):
    """tile8_pixel (flx_kernel_util.h): the 64 lanes of 8 x 8 tile `tile` (row-major) -> [(px, image row from the top) or None outside the image]"""
    tiles_x = (width + 7) >> 3
    tx, ty = tile % tiles_x, tile // tiles_x
    lanes = []
    for lane in range(64):
        px, row = (tx << 3) + (lane & 7), (ty << 3) + (lane >> 3)
        lanes.append((px, row) if px < width and row < height else None)
    return lanes


Schedule = collections.namedtuple("Schedule", "alone_from trips")


def wave_schedule(visits, lock_min):
    """The loop head of k_raster for one wave.  visits: per lane the entries its walk fetches in order (terminator included; empty for a lane outside the
    image, which starts ended).  While the wave is not alone a trip serves the least next entry over the lanes, `mine` = the lanes whose next entry that
    is; thin <- thin + 1 when fewer than lock_min lanes are mine, else 0; once thin >= 2 the wave is alone and every further trip serves every unfinished
    lane.  (The kernel walks the forward-ordered copy, whose indices are the live entries' ranks and whose terminator comes last: the same order.)
    -> Schedule(alone_from: the number (from 1) of the first trip made alone, None if the wave never goes alone; trips: per trip the lanes served)"""
    assert len(visits) == 64
    pos = [0] * 64
    thin, alone, alone_from, trips = 0, False, None, []
    while True:
        live = [l for l in range(64) if pos[l] < len(visits[l])]
        if not live:
            break
        if not alone:
            i = min(visits[l][pos[l]] for l in live)
            mine = [l for l in live if visits[l][pos[l]] == i]
            thin = thin + 1 if len(mine) < lock_min else 0
            if thin >= 2:
                alone, alone_from = True, len(trips) + 2
        else:
            mine = live
        trips.append(tuple(mine))
        for l in mine:
            pos[l] += 1
    return Schedule(alone_from, trips)


# -- what a frame's pixels are made of --------------------------------------------------------------------------------------------------
Pixel = collections.namedtuple("Pixel", "entries colours opaque pattern")


def clamp01(x):
    return np.float32(0) if not x > 0 else (np.float32(1) if x >= 1 else np.float32(x))


def pixel_fragments(ref, view, p, px, row):
    """pixel (px, image row from the top) -> Pixel: its fragments' entries in draw order, each one's renderColor (ref.fragment), whether its clamped alpha
    is 1, and the O / T pattern"""
    frags = ref.fragments(view, p, px, p.height - 1 - row)
    colours = [ref.fragment(view, p, ti, entry, suv)[0] for suv, ti, entry in frags]
    opaque = [bool(clamp01(c[3]) == 1) for c in colours]
    return Pixel([f[2] for f in frags], colours, opaque, "".join("O" if o else "T" for o in opaque))


def frame_pixels(ref, sc, p):
    view = sc.view()
    return {(px, row): pixel_fragments(ref, view, p, px, row) for row in range(p.height) for px in range(p.width)}


def literal_pixel(ref, pixel, upto=None):
    """every fragment blended in draw order over the clear colour, with no shortcut -> the RGBA8 buffer's values k / 255"""
    dst = np.zeros(4, np.float32)
    for c in pixel.colours[:upto]:
        dst = ref.blend(c, dst)
    return dst


def shades_of(pixel):
    """what the counters count: the fragments from the last opaque one on"""
    n = len(pixel.pattern)
    return n - max(pixel.pattern.rfind("O"), 0) if n else 0


def pattern_table(pixels):
    """pattern -> number of pixels ('none': no fragment)"""
    return dict(collections.Counter(px.pattern or "none" for px in pixels.values()))


LaneState = collections.namedtuple("LaneState", "fragments pending colour last_shaded_while_others_walk")


def wave_states(ref, sc, p, tile=0, lock=None):
    """-> (Schedule, [LaneState or None per lane]): for every lane inside the image its state when the wave goes alone (or at the end if it never does) —
    the fragments it has met, whether one is pending, whether its blended colour is non-zero — and whether its last fragment is shaded on a trip that
    still serves other lanes"""
    view = sc.view()
    lanes = tile_lanes(p.width, p.height, tile)
    visits = [ref.visits(view, p, l[0], p.height - 1 - l[1]) if l else [] for l in lanes]
    sched = wave_schedule(visits, lock_min() if lock is None else lock)
    before = len(sched.trips) if sched.alone_from is None else sched.alone_from - 1
    states = []
    for lane, l in enumerate(lanes):
        if l is None:
            states.append(None)
            continue
        served = [t for t, trip in enumerate(sched.trips) if lane in trip]
        seen = set(visits[lane][:sum(1 for t in served if t < before)])
        pixel = pixel_fragments(ref, view, p, l[0], l[1])
        met = [k for k, e in enumerate(pixel.entries) if e in seen]
        colour = False
        if met:                                                     # (in lockstep every lane fetches the terminator on one trip: the last of `met` is still pending)
            first = max("".join(pixel.pattern[k] for k in met).rfind("O"), 0)
            dst = np.zeros(4, np.float32)
            for k in met[first:-1]:
                dst = ref.blend(pixel.colours[k], dst)
            colour = bool(dst.any())
        states.append(LaneState(len(met), bool(met), colour, served[-1] + 1 < len(sched.trips)))
    return sched, states


# -- the cases ------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "id group entries width height lights tpo_texel")
O, T = 0.0, 1.0


def flat(zs_tpos, **kw):
    """full-cover layers [(z, tpo.x)] in draw order, coloured from the palette"""
    return [layer(z, t, PALETTE[k % len(PALETTE)], **kw) for k, (z, t) in enumerate(zs_tpos)]


def _with_cover(entries, cover):
    """the same stack with its full-cover layers over one half of the image (either winding); other entries stay"""
    out = []
    for kind, geo, att in entries:
        z = float(geo[2])
        g = geo.copy()
        for flip in (False, True):
            if np.array_equal(geo, layer(z, flip=flip)[1]):
                g = layer(z, cover=cover, flip=flip)[1]
        out.append((kind, g, att))
    return out


def _two_tiles(a, b):
    """16 x 8: stack a over the left tile, stack b over the right one, their entries drawn in turn"""
    a, b = _with_cover(a, "left"), _with_cover(b, "right")
    out = []
    for k in range(max(len(a), len(b))):
        out += a[k:k + 1] + b[k:k + 1]
    return out


def _flat_cases(group, named, lights=(), tpo_texel=None):
    """a flat (full-cover) stack at 8 x 8 (lockstep throughout), 3 x 3 (alone from the third trip) and 16 x 8 with the next stack of the group over the
    right tile"""
    out = []
    for k, (name, entries) in enumerate(named):
        other = named[(k + 1) % len(named)][1] if len(named) > 1 else entries[::-1]
        out.append(Case("%s-%s-8x8" % (group, name), group, entries, 8, 8, lights, tpo_texel))
        out.append(Case("%s-%s-3x3" % (group, name), group, entries, 3, 3, lights, tpo_texel))
        out.append(Case("%s-%s-16x8" % (group, name), group, _two_tiles(entries, other), 16, 8, lights, tpo_texel))
    return out


def all_patterns():
    return [format(m, "0%db" % n).replace("0", "O").replace("1", "T") for n in range(1, 5) for m in range(1 << n)]


def pattern_stack(pattern, failing_after_each=False):
    """four or more full-cover layers whose fragment list is `pattern`: one passing layer per letter, each nearer than the one before; the rest fail the
    depth test — drawn last to make four, or (failing_after_each) one after every passing layer, farther than it and of the other opacity"""
    zs = []
    for k, ch in enumerate(pattern):
        zs.append((10.0 - k, O if ch == "O" else T))
        if failing_after_each:
            zs.append((10.5 - k, T if ch == "O" else O))
    if not failing_after_each:
        zs += [(20.0 + k, O if k % 2 else T) for k in range(4 - len(pattern))]
    return flat(zs)


def mixed_tile():
    """seven patterns in one 8 x 8 wave: four bands of two columns each (edges at nx = -0.5, 0, 0.5) times the upper and the lower half.
    Upper half, left to right: T, OT, OTT, OTTO; lower half: none, O, OT, OTO."""
    return [layer(10, O, PALETTE[0], cover="right", edge=-0.5), layer(9, T, PALETTE[1], cover="right"), layer(8, T, PALETTE[2], cover="top"),
            layer(7, O, PALETTE[3], cover="right", edge=0.5)]


MIXED_WANT = {"T", "OT", "OTT", "OTTO", "none", "O", "OTO"}


def switch_stack(b_first, patches=3, wide=False):
    """[layers A][a box][layers B].  A: opaque over the right three quarters, translucent over the right half — lanes with no fragment, with a pending
    fragment and a zero colour, and with a pending fragment over a non-zero colour.  The box: `patches` small triangles over the upper right quadrant's
    nine inner pixels (wide: over 25 pixels).  B: two or three layers, the first opaque or translucent (b_first)."""
    x1 = 0.72
    x0 = -0.45 if wide else 0.05
    kids = [patch(8.0 - 0.1 * k, x0, x0, x1 + (0.25 if wide else 0), x1 + (0.25 if wide else 0), tpo=(T, O, T)[k % 3], albedo=PALETTE[4 + k]) for k in range(patches)]
    a = [layer(10, O, PALETTE[0], cover="right", edge=-0.5), layer(9, T, PALETTE[1], cover="right")]
    if b_first == "O":
        b = [layer(7, O, PALETTE[2]), layer(6, T, PALETTE[3], cover="top")]
    else:
        b = [layer(7, T, PALETTE[2]), layer(6, T, PALETTE[3], cover="top"), layer(5, O, PALETTE[7], cover="left")]
    return a + [box(kids)] + b


ALPHA_TPO = [("zero", 0.0), ("minus-zero", -0.0), ("2^-25", 2.0 ** -25), ("2^-24", 2.0 ** -24), ("2^-23", 2.0 ** -23), ("one", 1.0), ("two", 2.0),
             ("three", 3.0), ("minus-one", -1.0), ("nan", float("nan")), ("inf", float("inf"))]


def alpha_stack(tpo, tpo_tex=-1.0):
    """the boundary value as the near layer over a translucent red far layer"""
    return [layer(10, T, (1, 0, 0)), layer(5, tpo, (1, 1, 1), tpo_tex=tpo_tex)]


def tilted(slope=0.3):
    """a layer z = 0.5 + slope x: the pixel with centre nx meets it at view depth 0.5 / (1 - slope nx), at the near plane where nx = 0"""
    z = lambda x: 0.5 + slope * x
    return tri([-100, -100, z(-100), 300, -100, z(300), -100, 300, z(-100)], O, PALETTE[3])


BELOW_HALF, ABOVE_HALF = float(np.nextafter(np.float32(0.5), np.float32(0))), float(np.nextafter(np.float32(0.5), np.float32(1)))

LIGHTS = ([3.0, 4.0, -5.0, 300.0], [4.0, 4.0, -5.0, 0.0])


def shadow_stack():
    """A light behind the camera at (3, 4, -5), a zero-strength one beside it, and an opaque caster between the light and the layers, behind the near
    plane (no pixel sees it), that shadows the layers' points with x >= -0.5: the pixels right of the centre.  Two translucent layers, the far one shaded
    when the near one comes to lie over it, the near one as the last fragment; their winding is the one that a shadow ray towards the light does not
    meet (moellerTrumboreCull), so that neither shadows the other."""
    return [layer(10, T, (0.6, 0.5, 0.4), emissive=0.1, flip=True), layer(9, T, (0.3, 0.6, 0.5), emissive=0.1, flip=True),
            tri([2.3, -8, -2, 12, -8, -2, 2.3, 12, -2], O, PALETTE[2])]


def _cases():
    out = []
    pats = all_patterns()
    out += _flat_cases("pattern", [(pt, pattern_stack(pt)) for pt in pats])
    out += _flat_cases("failing", [(pt, pattern_stack(pt, True)) for pt in pats])
    out += [Case("mixed-8x8", "mixed", mixed_tile(), 8, 8, (), None), Case("mixed-3x3", "mixed", mixed_tile(), 3, 3, (), None),
            Case("mixed-16x8", "mixed", mixed_tile(), 16, 8, (), None)]
    for b in "OT":
        out += [Case("switch-B%s-3" % b, "switch", switch_stack(b, 3), 8, 8, (), None),
                Case("switch-B%s-2" % b, "switch", switch_stack(b, 2), 8, 8, (), None),
                Case("control-wide-B%s" % b, "control", switch_stack(b, 3, wide=True), 8, 8, (), None),
                Case("control-single-B%s" % b, "control", switch_stack(b, 1), 8, 8, (), None)]
    out += _flat_cases("alpha", [(name, alpha_stack(v)) for name, v in ALPHA_TPO])
    for byte in (0, 1):
        out += _flat_cases("alpha-texel%d" % byte, [("near", alpha_stack(7.0, tpo_tex=0.0))], tpo_texel=byte)
    for name, first in (("first-white", 0), ("first-red", 1)):
        twins = [layer(7, O, PALETTE[0]), layer(7, O, PALETTE[1])]
        out += _flat_cases("coplanar", [(name, twins if first == 0 else twins[::-1])])
    for name, z in (("half", 0.5), ("below", BELOW_HALF), ("above", ABOVE_HALF)):
        st = [layer(z, O, PALETTE[3])]
        out += [Case("near-%s-9x9" % name, "near", st, 9, 9, (), None), Case("near-%s-8x8" % name, "near", st, 8, 8, (), None)]
    out += [Case("near-tilted-9x9", "near", [tilted()], 9, 9, (), None), Case("near-tilted-8x8", "near", [layer(3, T, PALETTE[1]), tilted()], 8, 8, (), None)]
    out += _flat_cases("shadow", [("TT", shadow_stack())], lights=LIGHTS)
    out += [Case("shadow-mixed-8x8", "shadow", [layer(11, O, (0.5, 0.5, 0.6), emissive=0.1, cover="top", flip=True)] + shadow_stack(), 8, 8, LIGHTS, None)]
    out += _flat_cases("saturate", [("emissive", flat([(10, O), (9, T), (8, T)], emissive=3.0)), ("alpha-halves", flat([(10 - k, 1.0) for k in range(4)])),
                                    ("alpha-quarters", flat([(10 - k, 1.5) for k in range(4)], emissive=0.2))])
    assert len({c.id for c in out}) == len(out)
    return out


CASES = _cases()
CASE = {c.id: c for c in CASES}


def case_scene(case, hdr=0):
    return stack_scene(case.entries, case.width, case.height, case.lights, case.tpo_texel, hdr)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(hip, ref, sc, p, what):
    """the scene `sc` is uploaded: k_raster's frame and counters equal the reference's bit for bit, and so does the frame of the kernel without counters"""
    want, want_cnt = ref.render(sc, p)
    got, cnt = hip.raster_render(p, counters=True)
    bad = np.argwhere((bits(got) != bits(want)).any(axis=-1))
    assert bad.size == 0, "%s: %d pixels differ, first %s: got %s want %s" % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    assert cnt == want_cnt, "%s: counters %s vs %s" % (what, cnt, want_cnt)
    plain, none = hip.raster_render(p, counters=False)             # the kernel without counting code: the same image
    assert none is None
    assert np.array_equal(bits(plain), bits(want)), what
    return got, cnt
