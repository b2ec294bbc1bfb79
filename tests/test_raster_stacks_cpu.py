"""The hand-made layer stacks of tests/raster_stacks_util.py without a GPU: every case reaches the class of pixels and of wave schedules it is there
for, and the CPU reference (tests/raster_ref) is right on it — its shortcut (shade from the last opaque fragment on) against the literal draw (every
fragment shaded and blended in order) and against hand-computed bytes.  tests/test_raster_stacks_gpu.py runs the same cases through k_raster."""
import itertools
import os
import sys

import numpy as np
import pytest

import raster_stacks_util as u

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "raster_ref"))
import flx_raster_ref  # noqa: E402

GROUPS = sorted({c.group for c in u.CASES})
FLAT_GROUPS = ["pattern", "failing", "alpha", "alpha-texel0", "alpha-texel1", "coplanar", "shadow", "saturate"]


@pytest.fixture(scope="module")
def ref(oracle, tmp_path_factory):
    return flx_raster_ref.build(str(tmp_path_factory.mktemp("raster_ref")))


@pytest.fixture(scope="module")
def frames(ref):
    """case id -> (scene, params, {(px, row): Pixel}, reference frame, reference counters), computed once"""
    cache = {}

    def get(cid):
        if cid not in cache:
            sc, p = u.case_scene(u.CASE[cid])
            cache[cid] = (sc, p, u.frame_pixels(ref, sc, p)) + ref.render(sc, p)
        return cache[cid]
    return get


def table(frames, cid):
    return u.pattern_table(frames(cid)[2])


def byte_frame(img):
    k = np.rint(img * 255.0)
    assert np.array_equal(k.astype(np.float32) / np.float32(255), img)
    return k.astype(np.int64)


# -- the wave emulation itself ----------------------------------------------------------------------------------------------------------
def test_wave_schedule_follows_the_loop_head():
    full = [[0, 1, 2]] * 64
    assert u.wave_schedule(full, 12) == u.Schedule(None, [tuple(range(64))] * 3)
    nine = [[0, 1, 2, 3]] * 9 + [[]] * 55                               # lanes outside the image start ended
    s = u.wave_schedule(nine, 12)
    assert s.alone_from == 3 and s.trips == [tuple(range(9))] * 4
    assert u.wave_schedule(nine, 9).alone_from is None                   # "fewer than": nine lanes are not thin at 9
    # a box at 1 over entries 2, 3 that lanes 0 .. 4 enter: two thin trips, then every lane is served at once
    v = [[0, 1, 2, 3, 4, 5] if l < 5 else [0, 1, 4, 5] for l in range(64)]
    s = u.wave_schedule(v, 12)
    assert s.alone_from == 5 and [len(t) for t in s.trips] == [64, 64, 5, 5, 64, 64]
    # one entry under the box: thin goes to 1 and back to 0
    v = [[0, 1, 2, 3, 4] if l < 5 else [0, 1, 3, 4] for l in range(64)]
    s = u.wave_schedule(v, 12)
    assert s.alone_from is None and [len(t) for t in s.trips] == [64, 64, 5, 64, 64]
    # alone, the lanes no longer wait for each other: the 59 are a trip ahead and end first
    v = [[0, 1, 2, 3, 4, 5, 6] if l < 5 else [0, 1, 5, 6] for l in range(64)]
    s = u.wave_schedule(v, 12)
    assert s.alone_from == 5 and [len(t) for t in s.trips] == [64, 64, 5, 5, 64, 64, 5]


def test_tile_lanes_are_tile8_pixel():
    lanes = u.tile_lanes(16, 8, 1)
    assert lanes[0] == (8, 0) and lanes[7] == (15, 0) and lanes[8] == (8, 1) and lanes[63] == (15, 7)
    lanes = u.tile_lanes(9, 9, 3)
    assert lanes[0] == (8, 8) and lanes.count(None) == 63
    assert u.lock_min() >= 2


# -- patterns ---------------------------------------------------------------------------------------------------------------------------
def test_four_layers_in_every_order_and_opacity_make_exactly_the_thirty_patterns(ref):
    """24 draw orders x 16 opacity masks of four full-cover layers: a layer passes iff it is nearer than all layers drawn before it"""
    seen = set()
    for order in itertools.permutations(range(4)):
        for mask in range(16):
            zs = [(10.0 - rank, u.T if mask >> rank & 1 else u.O) for rank in order]
            sc, p = u.stack_scene(u.flat(zs), 1, 1)
            got = u.pixel_fragments(ref, sc.view(), p, 0, 0).pattern
            want, nearest = "", 1e9
            for z, t in zs:
                if z < nearest:
                    nearest, want = z, want + ("T" if t else "O")
            assert got == want, (order, mask)
            seen.add(got)
    assert seen == set(u.all_patterns()) and len(seen) == 30


@pytest.mark.parametrize("kind", ["pattern", "failing"])
def test_every_pattern_case_reaches_its_pattern(frames, kind):
    pats = u.all_patterns()
    assert len(pats) == 30
    for k, pt in enumerate(pats):
        assert table(frames, "%s-%s-8x8" % (kind, pt)) == {pt: 64}
        assert table(frames, "%s-%s-3x3" % (kind, pt)) == {pt: 9}
        pixels = frames("%s-%s-16x8" % (kind, pt))[2]
        other = pats[(k + 1) % 30]
        assert all(px.pattern == (pt if x < 8 else other) for (x, _), px in pixels.items()), pt
        n = len(u.CASE["%s-%s-8x8" % (kind, pt)].entries)
        assert n == (2 * len(pt) if kind == "failing" else 4)           # (failing: a farther layer after every passing one)


def test_mixed_tile_holds_seven_patterns_in_one_wave(ref, frames):
    t = table(frames, "mixed-8x8")
    assert set(t) == u.MIXED_WANT and len(t) >= 6 and "none" in t
    sc, p = frames("mixed-8x8")[:2]
    assert u.wave_states(ref, sc, p)[0].alone_from is None
    assert len(table(frames, "mixed-3x3")) >= 6


# -- modes ------------------------------------------------------------------------------------------------------------------------------
def test_flat_stacks_walk_in_lockstep_at_8x8_and_alone_from_the_third_trip_at_3x3(ref):
    for c in u.CASES:
        if c.group not in FLAT_GROUPS:
            continue
        sc, p = u.case_scene(c)
        view = sc.view()
        for tile in range((p.width + 7) // 8):
            lanes = u.tile_lanes(p.width, p.height, tile)
            s = u.wave_schedule([ref.visits(view, p, l[0], p.height - 1 - l[1]) if l else [] for l in lanes], u.lock_min())
            assert s.alone_from == (3 if p.width == 3 else None), c.id
            assert all(len(t) == (9 if p.width == 3 else 64) for t in s.trips), c.id


def box_row(case):
    g = u.case_scene(case)[0].arrays["geometry"].reshape(-1, 12)
    rows = np.flatnonzero(g[:, 10] == 1)
    assert len(rows) == 1
    return int(rows[0]), int(g[rows[0], 6])


@pytest.mark.parametrize("cid", ["switch-BO-3", "switch-BO-2", "switch-BT-3", "switch-BT-2"])
def test_switch_cases_go_alone_inside_the_box(ref, frames, cid):
    sc, p, pixels = frames(cid)[:3]
    at, skip = box_row(u.CASE[cid])
    assert skip >= 2
    s, states = u.wave_states(ref, sc, p)
    view = sc.view()
    visits = [ref.visits(view, p, l[0], p.height - 1 - l[1]) for l in u.tile_lanes(8, 8, 0)]
    inside = [l for l in range(64) if at + 1 in visits[l]]
    assert 1 <= len(inside) < u.lock_min(), inside                       # the box's bounds are hit by 1 .. 11 pixel rays
    assert s.alone_from == at + 4                                        # trips 1 .. at + 1: the rows up to the box; at + 2, at + 3: two thin trips
    assert s.trips[at + 1] == s.trips[at + 2] == tuple(inside)           # ... which serve the box's first two triangles
    assert any(st.pending and st.colour for st in states) and any(st.pending and not st.colour for st in states)
    assert any(st.fragments == 0 for st in states)
    assert any(st.pending and st.colour for l, st in enumerate(states) if l in inside)
    first_b = at + 1 + skip
    later = [sum(1 for e in px.entries if e >= first_b) for px in pixels.values()]
    assert min(later) >= 1                                               # layers B still produce fragments, on every lane
    b0 = {px.pattern[px.entries.index(first_b)] for px in pixels.values()}
    assert b0 == {cid[8]}                                                # B starts with O / with T
    whiles = {st.last_shaded_while_others_walk for st in states}
    assert whiles == ({True, False} if skip == 3 else {False})           # three triangles: the 9 lanes end a trip after the others


@pytest.mark.parametrize("cid", ["control-wide-BO", "control-wide-BT", "control-single-BO", "control-single-BT"])
def test_controls_stay_in_lockstep(ref, frames, cid):
    sc, p = frames(cid)[:2]
    at, skip = box_row(u.CASE[cid])
    s, _ = u.wave_states(ref, sc, p)
    assert s.alone_from is None
    under = [len(t) for t in s.trips[at + 1:at + 1 + skip]]
    if "wide" in cid:
        assert skip == 3 and all(n >= u.lock_min() for n in under), under
    else:
        assert skip == 1 and 1 <= under[0] < u.lock_min() and len(s.trips[at + 2]) == 64      # thin goes to 1 and back to 0
    # A and B are the switch cases' own
    twin = u.CASE["switch-B%s-3" % cid[-1]].entries
    mine = u.CASE[cid].entries
    same = lambda a, b: all(np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]) for x, y in zip(a, b)) and len(a) == len(b)
    assert same(mine[:2], twin[:2]) and same(mine[3:], twin[3:])


# -- the literal draw -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_literal_draw_equals_the_reference_frame(ref, frames, group):
    """every fragment shaded (ref.fragment) and blended (ref.blend) in draw order, with no shortcut: the bytes of ref.render; and the reference's shades
    are the fragments from the last opaque one on"""
    n = 0
    for c in u.CASES:
        if c.group != group:
            continue
        sc, p, pixels, img, cnt = frames(c.id)
        for (px, row), pixel in pixels.items():
            lit = u.literal_pixel(ref, pixel)
            assert np.array_equal(u.bits(lit), u.bits(img[row, px])), (c.id, px, row, pixel.pattern, lit, img[row, px])
        assert cnt["shades"] == sum(u.shades_of(px) for px in pixels.values()), c.id
        assert cnt["primary_hits"] == sum(1 for px in pixels.values() if px.pattern), c.id
        n += 1
    assert n > 0


@pytest.mark.parametrize("cid,want", [("pattern-OT-8x8", (255, 64, 64, 255)), ("pattern-TO-8x8", (128, 0, 0, 255)), ("pattern-OTO-8x8", (0, 128, 0, 255)),
                                      ("failing-TO-3x3", (0, 128, 0, 255)), ("pattern-O-3x3", (128, 128, 128, 255)), ("pattern-T-8x8", (191, 191, 191, 128))])
def test_hand_computed_stacks(frames, cid, want):
    """Layer k has the palette's colour k (white, red, green), emissive 0.5, no light.  Opaque (tpo.x = 0): colour 0.5 albedo, alpha 1.  Translucent
    (tpo.x = 1): finalColor = 0.5 albedo, translucencyFactor = min(1 + 0.5 - 1, 1) = 0.5, colour mix(albedo^2, finalColor, 0.5) = 0.75 albedo, alpha 0.5.
    O: Q(0.5) = 128.  T: Q(0.75) = 191, Q(0.5) = 128.  OT: red (0.75, 0, 0, 0.5) over white (128, 128, 128, 255): Q(0.75 + 0.5 * 128 / 255) = 255,
    Q(0.5 * 128 / 255) = floor(64 + 0.5) = 64, alpha Q(0.5 + 1) = 255.  TO: opaque red (0.5, 0, 0, 1) replaces what is under it.  OTO: opaque green.
    failing-TO: the layers that pass are 0 (white, T) and 2 (green, O); 1 (red, O) and 3 lie farther than the one before them and fail."""
    img = frames(cid)[3]
    assert np.array_equal(byte_frame(img), np.broadcast_to(np.array(want), img.shape)), byte_frame(img)[0, 0]


def test_an_opaque_fragment_hides_every_buffer_value(ref):
    """what both shortcuts rest on (and why k_raster's colour reset at an opaque fragment cannot show in a frame: without it the blend gives the same
    bytes): with clamped alpha 1 the blend's result is the same over each of the 256 values a channel can hold"""
    for src in ([0.5, 0.25, 1.0, 1.0], [3.0, -1.0, np.nan, 1.0], [0.1, 0.2, 0.3, 1.0 + 2.0 ** -23], [0.7, 0.0, 1e-9, 7.0], [0.3, 0.6, 0.9, np.inf]):
        over_clear = ref.blend(np.array(src, np.float32), np.zeros(4, np.float32))
        assert over_clear[3] == 1
        for k in range(256):
            dst = np.full(4, np.float32(k) / np.float32(255), np.float32)
            assert np.array_equal(u.bits(ref.blend(np.array(src, np.float32), dst)), u.bits(over_clear)), (src, k)


# -- alpha at the opaque / translucent boundary -----------------------------------------------------------------------------------------
ALPHA_WANT = {"zero": "TO", "minus-zero": "TO", "2^-25": "TO", "2^-24": "TO", "minus-one": "TO", "2^-23": "TT", "one": "TT", "two": "TT", "three": "TT",
              "nan": "TT", "inf": "TT"}


def test_alpha_boundaries(frames):
    """1 - tpo.x / 2 rounds to 1 up to tpo.x = 2^-24 and is 1 - 2^-24 at 2^-23: TO with one shade per pixel, TT with two — and the same bytes, so only
    the counters tell them apart; NaN and inf give alpha 0"""
    assert set(ALPHA_WANT) == {n for n, _ in u.ALPHA_TPO}
    for name, pat in ALPHA_WANT.items():
        sc, p, pixels, img, cnt = frames("alpha-%s-8x8" % name)
        assert u.pattern_table(pixels) == {pat: 64}, name
        assert cnt["shades"] == 64 * (1 if pat == "TO" else 2), name
        assert cnt["atlas_texels"] == 0
    assert np.array_equal(u.bits(frames("alpha-2^-23-8x8")[3]), u.bits(frames("alpha-2^-24-8x8")[3]))
    assert np.array_equal(u.bits(frames("alpha-2^-23-8x8")[3]), u.bits(frames("alpha-zero-8x8")[3]))
    for name in ("nan", "inf", "two", "three"):
        near = frames("alpha-%s-8x8" % name)[2][(3, 3)].colours[1]
        assert u.clamp01(near[3]) == 0, (name, near)
    assert np.isnan(frames("alpha-nan-8x8")[2][(3, 3)].colours[1][3])


def test_alpha_boundary_from_a_tpo_atlas_texel(frames):
    """byte 0: tpo.x = 0, opaque; byte 1: tpo.x = 1 / 255, alpha below 1 (the attribute, 7, would give alpha 0 either way)"""
    for byte, pat, shades in ((0, "TO", 64), (1, "TT", 128)):
        sc, p, pixels, img, cnt = frames("alpha-texel%d-near-8x8" % byte)
        assert u.pattern_table(pixels) == {pat: 64}
        assert cnt["shades"] == shades and cnt["atlas_texels"] == 64      # the near layer's tpo texel, once per shade of it
    assert np.array_equal(byte_frame(frames("alpha-texel0-near-8x8")[3]), byte_frame(frames("alpha-texel1-near-8x8")[3]))


# -- depth ties and the near plane ------------------------------------------------------------------------------------------------------
def test_coplanar_twins_the_earlier_keeps_every_pixel(frames):
    for cid, want in (("coplanar-first-white", (128, 128, 128, 255)), ("coplanar-first-red", (128, 0, 0, 255))):
        for size in ("8x8", "3x3"):
            sc, p, pixels, img, cnt = frames("%s-%s" % (cid, size))
            assert all(px.entries == [0] for px in pixels.values())
            assert np.array_equal(byte_frame(img), np.broadcast_to(np.array(want), img.shape))


def test_near_plane_at_exactly_half(frames):
    """view depth s d.z against 0.5 in float32: at z = 0.5 the product rounds below 0.5 on 12 of 81 pixels, at the float below 0.5 it reaches 0.5 on 4"""
    for cid, covered in (("near-half-9x9", 69), ("near-below-9x9", 4), ("near-above-9x9", 81)):
        t = table(frames, cid)
        assert t.get("O", 0) == covered and t.get("none", 0) == 81 - covered, (cid, t)
    for cid in ("near-half-9x9", "near-below-9x9", "near-half-8x8", "near-below-8x8", "near-tilted-9x9", "near-tilted-8x8"):
        t = table(frames, cid)
        assert len(t) == 2 and min(t.values()) >= 4, (cid, t)               # both outcomes occur in the frame
    pixels = frames("near-tilted-9x9")[2]
    assert all(bool(px.pattern) == (x >= 4) for (x, _), px in pixels.items())      # the plane crosses the near plane at the centre column


# -- light and shadow -------------------------------------------------------------------------------------------------------------------
def test_shadowed_and_lit_fragments_in_both_shade_positions(frames):
    sc, p, pixels, img, cnt = frames("shadow-TT-8x8")
    assert cnt["shadow_walks"] == cnt["shades"] == 128                    # one walk per shade: the zero-strength light has none
    lit, dark = pixels[(1, 3)], pixels[(6, 3)]
    for k in (0, 1):                                                      # 0: shaded when the near layer comes to lie over it; 1: the last fragment
        assert (lit.colours[k][:3] != dark.colours[k][:3]).any(), (k, lit.colours[k], dark.colours[k])
    b = byte_frame(img)
    assert (b[:, :4, :3] != b[:, 4:, :3]).any(axis=-1).all(), b[3]
    sc, p, pixels, img, cnt = frames("shadow-mixed-8x8")
    assert u.pattern_table(pixels) == {"OTT": 32, "TT": 32} and cnt["shadow_walks"] == 160
    b = byte_frame(img)
    assert (b[:, :4, :3] != b[:, 4:, :3]).any(axis=-1).all(), b[3]


# -- saturation -------------------------------------------------------------------------------------------------------------------------
def test_saturation(ref, frames):
    b = byte_frame(frames("saturate-emissive-8x8")[3])
    assert b.max() == 255 and frames("saturate-emissive-8x8")[2][(0, 0)].colours[0].max() > 1.0
    for cid, alpha in (("saturate-alpha-halves-8x8", 128), ("saturate-alpha-quarters-8x8", 64)):
        sc, p, pixels, img, cnt = frames(cid)
        px = pixels[(2, 5)]
        assert px.pattern == "TTTT"
        assert [int(np.rint(255 * u.literal_pixel(ref, px, n)[3])) for n in range(1, 5)] == [min(255, alpha * n) for n in range(1, 5)]
        assert 4 * alpha > 255 and (byte_frame(img)[..., 3] == 255).all()
