"""The denoise chain from the reference's text alone, over whole planes at once, and a generator of plane sets that put its claims to the test.

filter_literal is the three filter shaders (shaders/pathtracer_first_filter.glsl:18-123, pathtracer_second_filter.glsl:17-79, pathtracer_final_filter.glsl:11-71) and
the host's pass schedule (modules/pathtracerWGL2.js:462-550 with firstPasses = secondPasses = 3), every GLSL operation one float32 operation in the text's order (a vec4
expression component by component).  It is the vectorised form of tests/analysis/make_filter_kat.py's per-texel chain and keeps that script's pins: render targets are
RGBA8 (a store is 0 for not (x > 0), 255 for x >= 1, else int(f32(f32(x * 255) + 0.5)); texelFetch gives byte / 255), texelFetch outside the texture gives zeros, the
first filter's renderColorIp starts as zeros, IdRenderTexture[2] and [3] attach nothing.  tanh and pow are correctly rounded from 50-digit arithmetic, cached by the
argument's bit pattern.  Nothing here is taken from oracle/ or from the library: the tests hold both against it.

Planes are uint8 [H, W, 4] with rows top-down; inside, the passes index [y, x] with y counting from the bottom like gl_FragCoord (the tap order and the vote depend on
it).  Everything a pass records in its masks is turned back to rows top-down, so that a 16 x 16 tile of the kernels is [16 ty : 16 ty + 16, 16 tx : 16 tx + 16] of a mask.

make_planes is the seeded generator of adversarial plane sets: regions of a few ids and original ids so that taps pass, pixel noise from small palettes so that
neighbours differ, hand-placed patches for the conditions tests/test_filter_tiles_gpu.py asserts (coverage), colour bytes over 0 .. 255.
"""
import functools
from decimal import Decimal, getcontext

import numpy as np

f32 = np.float32
INV_256 = f32(0.00390625)

STENCIL1 = ((-1, 0), (0, -1), (0, 1), (1, 0))
STENCIL3_37 = ((-3, -1), (-3, 0), (-3, 1),
               (-2, -2), (-2, -1), (-2, 0), (-2, 1), (-2, 2),
               (-1, -3), (-1, -2), (-1, -1), (-1, 0), (-1, 1), (-1, 2), (-1, 3),
               (0, -3), (0, -2), (0, -1), (0, 0), (0, 1), (0, 2), (0, 3),
               (1, -3), (1, -2), (1, -1), (1, 0), (1, 1), (1, 2), (1, 3),
               (2, -2), (2, -1), (2, 0), (2, 1), (2, 2),
               (3, -1), (3, 0), (3, 1))
STENCIL3_36 = tuple(s for s in STENCIL3_37 if s != (0, 0))

# ---- tanh and pow: correctly rounded, cached by bit pattern ----------------------------------------------------------------------------------------------------------
_TANH, _POW = {}, {}


def _rnd(d):
    """Decimal -> nearest float32 (through the correctly rounded double of its 50 digits: make_filter_kat.py's rnd)"""
    return f32(np.float64(str(d)))


def _by_bits(x, table, fn):
    x = np.ascontiguousarray(x, f32)
    u, inv = np.unique(x.view(np.uint32), return_inverse=True)
    vals = np.empty(u.size, f32)
    for i, b in enumerate(u.tolist()):
        if b not in table:
            table[b] = fn(np.array([b], np.uint32).view(f32)[0])
        vals[i] = table[b]
    return vals[inv.reshape(-1)].reshape(x.shape)


def _tanh1(x):
    getcontext().prec = 50
    e2 = (2 * Decimal(float(x))).exp()
    return _rnd((e2 - 1) / (e2 + 1))


def _pow1(x, y):                                                           # x >= 0 here
    if np.isnan(x) or np.isinf(x): return x
    if x == 0: return f32(0)
    getcontext().prec = 50
    return _rnd((Decimal(float(x)).ln() * Decimal(float(y))).exp())


def tanh_f32(x):
    return _by_bits(x, _TANH, _tanh1)


def pow_f32(x, y):
    """pow(x, y) for one float32 exponent y"""
    y = f32(y)
    return _by_bits(x, _POW.setdefault(float(y), {}), lambda v: _pow1(v, y))


# ---- RGBA8 ---------------------------------------------------------------------------------------------------------------------------------------------------------
def quantise(v):
    """float32 [..., 4] -> the bytes an RGBA8 render target stores (make_filter_kat.py's Tex.store)"""
    x = np.asarray(v, f32)
    low, high = ~(x > 0), x >= 1                                           # (NaN: not > 0)
    with np.errstate(all="ignore"):
        q = (np.where(low | high, f32(0), x) * f32(255) + f32(0.5)).astype(f32)
    return np.where(low, 0, np.where(high, 255, q.astype(np.int32))).astype(np.uint8)


def fetch(q):
    """texelFetch of RGBA8 bytes"""
    return q.astype(f32) / f32(255)


def gather(p, cx, cy):
    """texelFetch(p, ivec2(cx, cy)) for coordinate planes, as bytes: zeros outside the texture -> (uint8 [H, W, 4], inside [H, W])"""
    H, W = p.shape[:2]
    inside = (cx >= 0) & (cy >= 0) & (cx < W) & (cy < H)
    q = p[np.clip(cy, 0, H - 1), np.clip(cx, 0, W - 1)]
    return np.where(inside[..., None], q, 0).astype(np.uint8), inside


def eq3(a, b): return (a[..., :3] == b[..., :3]).all(axis=-1)
def eq4(a, b): return (a == b).all(axis=-1)
def fmax(x, y): return np.where(x < y, y, x)                              # GLSL max(x, y): y if x < y else x
def fmin(x, y): return np.where(y < x, y, x)
def mod1(x): return x - f32(1.0) * np.floor(x / f32(1.0))                 # mod(x, 1.0) = x - 1.0 * floor(x / 1.0)
def rows(a): return np.ascontiguousarray(np.asarray(a)[..., ::-1, :])     # [..., y_gl, x] -> [..., row, x]


def first_offsets(ocw):
    """ivec2(stencil3[i] * (1.0 + w) * (1.0 + w) * 3.5) for float32 w of any shape -> int32 [37, 2, ...]"""
    k = f32(1.0) + np.asarray(ocw, f32)
    return np.array([[(((f32(s[c]) * k) * k) * f32(3.5)).astype(np.int32) for c in (0, 1)] for s in STENCIL3_37])


def scale_offsets(stencil, f):
    """ivec2(stencil3[i] * f) for float32 f of any shape -> int32 [len(stencil), 2, ...]"""
    f = np.asarray(f, f32)
    return np.array([[(f32(s[c]) * f).astype(np.int32) for c in (0, 1)] for s in stencil])


def second_scale(ocw, oidw, tanh=tanh_f32):
    return f32(1.0) + f32(2.0) * tanh((np.asarray(ocw, f32) + np.asarray(oidw, f32) * f32(4.0)).astype(f32))


def final_scale(ocw, oidw, tanh=tanh_f32):
    return f32(0.7) + f32(2.0) * tanh((np.asarray(ocw, f32) + np.asarray(oidw, f32) * f32(4.0)).astype(f32))


# ---- the three shaders -------------------------------------------------------------------------------------------------------------------------------------------------
def first_filter(R, Ip, O, Id, OId):
    """-> (renderColor, renderColorIp, renderId as float32 [H, W, 4], masks)"""
    H, W = R.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    centerColor, centerColorIp, centerOColor, centerId, centerOId = fetch(R), fetch(Ip), fetch(O), fetch(Id), fetch(OId)
    centerIdw = (centerId[..., 3] * f32(255.0)).astype(np.int32)
    centerLightNum, centerShadow = centerIdw // 2, centerIdw % 2
    gate = (centerOId[..., 3] != 0.0) & (centerColorIp[..., 3] != 0.0)
    ids = [fetch(gather(Id, xx + s[0], yy + s[1])[0]) for s in STENCIL1]
    oIds = [fetch(gather(OId, xx + s[0], yy + s[1])[0]) for s in STENCIL1]
    ipws = [fetch(gather(Ip, xx + s[0], yy + s[1])[0])[..., 3] for s in STENCIL1]
    vote = []
    for i in range(4):
        v = 1 + (eq3(ids[i], centerId) & eq4(oIds[i], centerOId)).astype(np.int32)
        for j in range(i + 1, 4):
            v = v + (eq3(ids[i], ids[j]) & eq4(oIds[i], oIds[j])).astype(np.int32)
        vote.append(np.where(ipws[i] == 0.0, v, 0))
    maxVote, idNumber = vote[0].copy(), np.zeros((H, W), np.int32)
    tie, loser = np.zeros((H, W), bool), np.zeros((H, W), np.int32)
    for i in range(1, 4):
        take = vote[i] >= maxVote
        tie = np.where(take, vote[i] == maxVote, tie)
        loser = np.where(take, idNumber, loser)
        maxVote, idNumber = np.where(take, vote[i], maxVote), np.where(take, i, idNumber)
    idsA = np.stack(ids)
    chosen = np.take_along_axis(idsA, idNumber[None, ..., None], axis=0)[0]
    lost = np.take_along_axis(idsA, loser[None, ..., None], axis=0)[0]
    renderId = np.where(gate[..., None], chosen, centerId)
    ipw = np.where(gate, fmax(f32(1.0) - np.sign(maxVote.astype(f32)), f32(0.0)), f32(0.0)).astype(f32)      # renderColorIp.w, zero where the shader leaves it unwritten (pinned)
    taps = centerOColor[..., 3] != 0.0
    color, count = np.zeros((H, W, 4), f32), np.zeros((H, W), f32)
    off = first_offsets(centerOColor[..., 3])
    rec = {k: [] for k in ("cx", "crow", "inside", "branch", "passed", "id3", "oid3", "oid4", "light")}
    for i in range(37):
        cx, cy = xx + off[i, 0], yy + off[i, 1]
        bId, inside = gather(Id, cx, cy)
        ident, originalId = fetch(bId), fetch(gather(OId, cx, cy)[0])
        idW = (ident[..., 3] * f32(255.0)).astype(np.int32)
        lightNum, shadow = idW // 2, idW % 2
        nextColor, nextColorIp = fetch(gather(R, cx, cy)[0]), fetch(gather(Ip, cx, cy)[0])
        id3, oid3, oid4 = eq3(centerId, ident), eq3(centerOId, originalId), eq4(centerOId, originalId)
        light = (centerLightNum != lightNum) | (centerShadow == shadow)
        passed = taps & id3 & oid4 & light
        color = np.where(passed[..., None], color + (nextColor + nextColorIp * f32(256.0)), color)
        count = np.where(passed, count + f32(1.0), count)
        branch = np.where(~taps, 0, np.where(passed, 1, np.where(~id3, 2, np.where(~oid4, 3, 4)))).astype(np.int8)      # 1 summed; rejected by 2 the id, 3 the original id, 4 the (light number, shadow) clause alone; 0 the texel has no taps
        for k, v in (("cx", cx), ("crow", H - 1 - cy), ("inside", inside), ("branch", branch), ("passed", passed), ("id3", id3), ("oid3", oid3), ("oid4", oid4), ("light", light)):
            rec[k].append(v)
    color = np.where(taps[..., None], color, centerColor)
    count = np.where(taps, count, f32(1.0))
    with np.errstate(all="ignore"):
        invCount = f32(1.0) / count
        sg = np.sign(centerColor[..., 3])
        c3 = color[..., :3] * invCount[..., None]
        renderColor = sg[..., None] * np.concatenate([mod1(c3), centerColor[..., 3:4]], axis=-1)
        renderColorIp = sg[..., None] * np.concatenate([np.floor(c3) * INV_256, ipw[..., None]], axis=-1)
    assert renderColor.dtype == f32 and renderColorIp.dtype == f32 and count.dtype == f32
    masks = {k: rows(np.array(v)) for k, v in rec.items()}
    masks.update(kind="first", taps=rows(taps), ocw=rows(O[..., 3]), gate=rows(gate), idNumber=rows(idNumber), maxVote=rows(maxVote), tie=rows(tie),
                 tie_unequal=rows(gate & tie & (chosen != lost).any(axis=-1)), ipw=rows(ipw), covered=rows(R[..., 3] != 0))
    return renderColor, renderColorIp, renderId, masks


def second_filter(R, Ip, O, Id, OId):
    """-> (renderColor, renderColorIp, renderOriginalColor as float32 [H, W, 4], masks)"""
    H, W = R.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    centerColor, centerColorIp, centerOColor, centerId, centerOId = fetch(R), fetch(Ip), fetch(O), fetch(Id), fetch(OId)
    zero = np.zeros((H, W, 1), f32)
    color = centerColor + np.concatenate([centerColorIp[..., :3], zero], axis=-1) * f32(256.0)
    oColor = centerOColor.copy()
    ipw = centerColorIp[..., 3].copy()
    count, oCount = np.full((H, W), f32(1.0)), np.full((H, W), f32(1.0))
    off = scale_offsets(STENCIL3_36, second_scale(centerOColor[..., 3], centerOId[..., 3]))
    rec = {k: [] for k in ("cx", "crow", "inside", "branch", "minOIdW", "maxIpW", "id3", "id4", "admit")}
    for i in range(36):
        cx, cy = xx + off[i, 0], yy + off[i, 1]
        bId, inside = gather(Id, cx, cy)
        bOId, bIp = gather(OId, cx, cy)[0], gather(Ip, cx, cy)[0]
        ident, nextOId, nextColor, nextColorIp, nextOColor = fetch(bId), fetch(bOId), fetch(gather(R, cx, cy)[0]), fetch(bIp), fetch(gather(O, cx, cy)[0])
        oid3 = eq3(centerOId, nextOId)
        near = fmin(centerOId[..., 3], nextOId[..., 3]) > f32(0.1)
        admit = eq4(ident, centerId) | (fmax(nextColorIp[..., 3], centerColorIp[..., 3]) >= f32(0.1))
        both = oid3 & near & admit
        only = oid3 & ~both & eq3(ident, centerId)
        add = nextColor + np.concatenate([nextColorIp[..., :3], zero], axis=-1) * f32(256.0)
        color = np.where((both | only)[..., None], color + add, color)
        count = np.where(both | only, count + f32(1.0), count)
        ipw = np.where(both, ipw + nextColorIp[..., 3], ipw)
        oColor = np.where(both[..., None], oColor + nextOColor, oColor)
        oCount = np.where(both, oCount + f32(1.0), oCount)
        branch = np.where(both, 1, np.where(only, 2, np.where(oid3, 3, 0))).astype(np.int8)       # 1 both sums, 2 colour only, 3 nothing though the original ids agree, 0 they do not
        for k, v in (("cx", cx), ("crow", H - 1 - cy), ("inside", inside), ("branch", branch), ("minOIdW", np.minimum(OId[..., 3], bOId[..., 3])),
                     ("maxIpW", np.maximum(Ip[..., 3], bIp[..., 3])), ("id3", eq3(ident, centerId)), ("id4", eq4(ident, centerId)), ("admit", admit)):
            rec[k].append(v)
    with np.errstate(all="ignore"):
        invCount = f32(1.0) / count
        w = centerColor[..., 3:4]
        c3 = color[..., :3] * invCount[..., None]
        renderColor = w * np.concatenate([mod1(c3), (color[..., 3] * invCount)[..., None]], axis=-1)
        renderColorIp = w * np.concatenate([np.floor(c3) * INV_256, ipw[..., None]], axis=-1)
        renderOriginalColor = (w * oColor) / oCount[..., None]
    assert renderColor.dtype == f32 and renderColorIp.dtype == f32 and renderOriginalColor.dtype == f32
    masks = {k: rows(np.array(v)) for k, v in rec.items()}
    masks.update(kind="second", covered=rows(R[..., 3] != 0), reach=rows(np.abs(off).max(axis=(0, 1))))
    return renderColor, renderColorIp, renderOriginalColor, masks


def final_filter(R, Ip, O, Id, OId, hdr):
    """-> (outColor float32 [H, W, 4], masks)"""
    H, W = R.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    centerColor, centerColorIp, centerOColor, centerId, centerOId = fetch(R), fetch(Ip), fetch(O), fetch(Id), fetch(OId)
    color, oColor = np.zeros((H, W, 4), f32), np.zeros((H, W, 4), f32)
    count, oCount = np.zeros((H, W), f32), np.zeros((H, W), f32)
    off = scale_offsets(STENCIL3_37, final_scale(centerOColor[..., 3], centerOId[..., 3]))
    rec = {k: [] for k in ("cx", "crow", "inside", "branch", "blur", "id3", "oid3", "counted", "minOIdW", "maxIpW")}
    for i in range(37):
        cx, cy = xx + off[i, 0], yy + off[i, 1]
        bId, inside = gather(Id, cx, cy)
        bOId, bIp = gather(OId, cx, cy)[0], gather(Ip, cx, cy)[0]
        ident, nextOId, nextColor, nextColorIp, nextOColor = fetch(bId), fetch(bOId), fetch(gather(R, cx, cy)[0]), fetch(bIp), fetch(gather(O, cx, cy)[0])
        blurTranslucent = (fmax(nextColorIp[..., 3], centerColorIp[..., 3]) != 0.0) & (fmin(centerOId[..., 3], nextOId[..., 3]) > 0.0)
        oid3, id3 = eq3(centerOId, nextOId), eq3(centerId, ident)
        m = blurTranslucent & oid3
        oColor = np.where(m[..., None], oColor + nextOColor, oColor)
        oCount = np.where(m, oCount + f32(1.0), oCount)
        m = (blurTranslucent | id3) & oid3
        color = np.where(m[..., None], color + (nextColor + nextColorIp * f32(255.0)), color)
        count = np.where(m, count + f32(1.0), count)
        branch = np.where(blurTranslucent & oid3, 1, np.where(m, 2, 0)).astype(np.int8)      # 1 both sums, 2 the colour sum only (by the id's equality), 0 nothing
        for k, v in (("cx", cx), ("crow", H - 1 - cy), ("inside", inside), ("branch", branch), ("blur", blurTranslucent), ("id3", id3), ("oid3", oid3), ("counted", m),
                     ("minOIdW", np.minimum(OId[..., 3], bOId[..., 3])), ("maxIpW", np.maximum(Ip[..., 3], bIp[..., 3]))):
            rec[k].append(v)
    with np.errstate(all="ignore"):
        fc = color[..., :3] / count[..., None]
        fc = fc * np.where((oCount == 0.0)[..., None], centerOColor[..., :3], oColor[..., :3] / oCount[..., None])
        if hdr == 1:
            fc = fc / (fc + f32(1.0))
            inv_gamma = f32(1.0) / f32(0.8)
            fc = pow_f32((f32(4.0) * fc).astype(f32), inv_gamma) / f32(4.0) * f32(1.3)
    assert fc.dtype == f32
    lit = centerColor[..., 3] > 0.0
    out = np.where(lit[..., None], np.concatenate([fc, np.ones((H, W, 1), f32)], axis=-1), f32(0.0)).astype(f32)
    masks = {k: rows(np.array(v)) for k, v in rec.items()}
    masks.update(kind="final", covered=rows(lit), oCount0=rows(oCount == 0.0), reach=rows(np.abs(off).max(axis=(0, 1))))
    return out, masks


# ---- the pass schedule -------------------------------------------------------------------------------------------------------------------------------------------------
def filter_literal(planes, hdr, firstPasses=3, secondPasses=3):
    """planes: R0, Ip0, O0, Id0, OId as uint8 [H, W, 4], rows top-down -> (the final filter's float32 [H, W, 4], rows top-down; the masks of the 6 + 1 passes in order).
    modules/pathtracerWGL2.js:462-550, the statements that touch textures."""
    gl = [np.ascontiguousarray(np.asarray(p, np.uint8)[::-1]) for p in planes]
    H, W = gl[0].shape[:2]
    blank = lambda: np.zeros((H, W, 4), np.uint8)
    RenderTexture = [gl[0], blank(), blank(), blank()]
    IpRenderTexture = [gl[1], blank(), blank(), blank()]
    OriginalRenderTexture = [gl[2], blank()]
    IdRenderTexture = [gl[3], blank()]
    OriginalIdRenderTexture = gl[4]
    PostProgram = [first_filter, first_filter, second_filter, second_filter]
    masks = []
    n = nId = nOriginal = 0
    for i in range(firstPasses + secondPasses):
        np_ = (i % 2) ^ 1
        npOriginal = int(np.fmod(i - firstPasses, 2)) ^ 1                 # JavaScript's % keeps the sign of the dividend: (-3 % 2) = -1, (-1) ^ 1 = -2
        if firstPasses <= i: np_ += 2
        third = None                                                       # which list and slot the third attachment is, if any
        if firstPasses <= i - 2: third = (OriginalRenderTexture, npOriginal)
        elif np_ < len(IdRenderTexture): third = (IdRenderTexture, np_)    # IdRenderTexture[2], [3] are undefined: nothing attached
        assert np_ != n and (third is None or third[1] != (nOriginal if third[0] is OriginalRenderTexture else nId))      # no attachment is also bound as a source
        a, b, c, m = PostProgram[n](RenderTexture[n], IpRenderTexture[n], OriginalRenderTexture[nOriginal], IdRenderTexture[nId], OriginalIdRenderTexture)
        RenderTexture[np_], IpRenderTexture[np_] = quantise(a), quantise(b)      # gl.clear, then every texel is written
        if third is not None: third[0][third[1]] = quantise(c)
        m["pass"] = i
        masks.append(m)
        n = np_
        if firstPasses <= i: nOriginal = npOriginal
        else: nId = np_
    index = 2 + (firstPasses + secondPasses) % 2
    indexId, indexOriginal = firstPasses % 2, secondPasses % 2
    out, m = final_filter(RenderTexture[index], IpRenderTexture[index], OriginalRenderTexture[indexOriginal], IdRenderTexture[indexId], OriginalIdRenderTexture, hdr)
    m["pass"] = firstPasses + secondPasses
    masks.append(m)
    return np.ascontiguousarray(out[::-1]), masks


# ---- adversarial plane sets ---------------------------------------------------------------------------------------------------------------------------------------------
MAIN = (93, 87)          # 6 x 6 tiles of 16 with a ragged last column (13) and row (7); 3 x 11 first-filter workgroups of 32 x 8; room for first-filter taps 42 texels away on all four sides
SHAPES = (MAIN, (1, 1), (1, 40), (40, 1), (15, 17), (16, 16), (17, 15), (32, 8), (31, 7), (33, 9), (64, 16))
CASES = tuple((W, H, 11 + k, (k + 1) % 2 if k else 0) for k, (W, H) in enumerate(SHAPES)) + ((MAIN[0], MAIN[1], 11, 1),)      # (W, H, seed, hdr): the main case at both hdr, the others alternating
EXCLUDED_PAIRS = ()      # (OColor.w, OId.w) byte pairs at which flx_math.h's tanh moves a tap (test_filter_literal_cpu.py's table): none

# where the main case's hand-placed patches lie (rows top-down)
UNCOVERED_TILE = (2, 0)                  # (tx, ty): every R.w zero, every other byte non-zero
ONE_COVERED_TILE, ONE_COVERED_AT = (4, 0), (70, 9)          # (x, row) of its one covered texel
ONE_UNCOVERED_TILE, ONE_UNCOVERED_AT = (4, 3), (69, 53)
FAR_TEXEL = (46, 43)                     # OColor.w = 255: all 37 first-filter taps, 14 texels apart, inside the image and of the centre's ids
BLOCK = (6, 22, 42, 58)                  # x0, row0, x1, row1: one original id at w = 255 (second- and final-filter taps 8 texels away), around the interior tile (1, 2)
BLOB = (10, 26, 38, 54)                  # translucent (Ip.w != 0) inside BLOCK: four first-filter passes leave its core
INTERIOR_TILE = (1, 2)
LONE = ((60, 30, 25), (60, 62, 26), (80, 40, 25), (80, 70, 26))      # (x, row, R.w): the centre of a translucent diamond of radius 4 — the one texel that is still translucent when the second filter starts


def make_planes(W, H, seed):
    """-> [R, Ip, O, Id, OId] uint8 [H, W, 4], rows top-down"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    pick = lambda palette, p=None: rng.choice(np.array(palette, np.uint8), size=(H, W), p=p)
    noisy = lambda share: rng.random((H, W)) < share
    # regions of four "objects": slanted bands, ~11 texels wide
    region = ((xx + yy // 3) // 11 + 2 * (yy // 19)) % 4
    ids = rng.integers(1, 256, (4, 3)).astype(np.uint8)
    oids = rng.integers(1, 256, (4, 3)).astype(np.uint8)
    idw_of, oidw_of = np.array([0, 2, 3, 5], np.uint8), np.array([200, 64, 255, 30], np.uint8)
    R, Ip, O, Id, OId = (np.zeros((H, W, 4), np.uint8) for _ in range(5))
    R[..., :3] = rng.integers(0, 256, (H, W, 3))
    R[..., 3] = np.where(noisy(0.12), pick([25, 26, 13, 128, 5, 2, 1]), 255)
    R[..., 3] = np.where(noisy(0.04), 0, R[..., 3])                                   # lone uncovered texels
    Ip[..., :3] = np.where(noisy(0.1)[..., None], rng.integers(0, 256, (H, W, 3)), rng.integers(0, 3, (H, W, 3)))
    Ip[..., 3] = np.where(noisy(0.08), pick([1, 25, 26, 40, 255]), 0)
    O[..., :3] = rng.integers(0, 256, (H, W, 3))
    O[..., 3] = np.where(noisy(0.45), rng.integers(1, 256, (H, W)), 0)
    r_id = np.where(noisy(0.06), (region + 1) % 4, region)                            # pixel noise: a neighbour of another object
    r_oid = np.where(noisy(0.06), (region + 2) % 4, region)
    Id[..., :3], OId[..., :3] = ids[r_id], oids[r_oid]
    Id[..., 3] = np.where(noisy(0.25), pick([0, 1, 2, 3, 4, 5]), idw_of[region])
    OId[..., 3] = np.where(noisy(0.2), pick([0, 25, 26, 27, 64, 255]), oidw_of[region])
    if W >= 24 and H >= 7:                                                            # a translucent band: wide enough to keep a core where the height allows it
        band = (xx >= W // 3) & (xx < W // 3 + 12)
        Ip[..., 3] = np.where(band & ~noisy(0.03), pick([40, 255, 25, 26, 1]), Ip[..., 3])
        OId[..., 3] = np.where(band & (OId[..., 3] == 0) & ~noisy(0.1), 27, OId[..., 3])
    if (W, H) != MAIN:
        return [R, Ip, O, Id, OId]
    planes = [R, Ip, O, Id, OId]
    # BLOCK: one object, original id at w = 255 with a little 0 / 25 / 26 noise; its ids with noise in w and in xyz
    x0, r0, x1, r1 = BLOCK
    blk = (xx >= x0) & (xx < x1) & (yy >= r0) & (yy < r1)
    OId[blk, :3] = oids[0]
    OId[..., 3] = np.where(blk, np.where(noisy(0.1), pick([0, 25, 26]), 255), OId[..., 3])
    Id[blk, :3] = ids[0]
    Id[..., :3] = np.where((blk & noisy(0.08))[..., None], ids[1], Id[..., :3])
    Id[..., 3] = np.where(blk, np.where(noisy(0.15), pick([1, 2, 3]), 0), Id[..., 3])
    R[..., 3] = np.where(blk & (R[..., 3] == 0), 255, R[..., 3])
    O[..., 3] = np.where(blk & noisy(0.5), 0, O[..., 3])
    bx0, br0, bx1, br1 = BLOB
    blob = (xx >= bx0) & (xx < bx1) & (yy >= br0) & (yy < br1)
    Ip[..., 3] = np.where(blob, pick([40, 255, 25, 26, 1]), np.where(blk, 0, Ip[..., 3]))
    OId[..., 3] = np.where(blob & (OId[..., 3] == 0), 26, OId[..., 3])
    for hx, hr in ((17, 33), (30, 45)):                                               # two holes in the blob
        Ip[hr, hx, 3] = 0
    tx, ty = INTERIOR_TILE
    for cx, cr in ((16 * tx, 16 * ty), (16 * tx + 15, 16 * ty), (16 * tx, 16 * ty + 15), (16 * tx + 15, 16 * ty + 15)):      # the tile's corners and what they tap: no noise
        for dx in (-8, 0, 8):
            for dr in (-8, 0, 8):
                OId[cr + dr, cx + dx], Id[cr + dr, cx + dx], R[cr + dr, cx + dx, 3] = list(oids[0]) + [255], list(ids[0]) + [0], 255
    # lone translucent texels: diamonds of radius 4, covered, with an original id whose w is not zero
    for lx, lr, rw in LONE:
        dia = (np.abs(xx - lx) + np.abs(yy - lr)) <= 4
        near = (np.abs(xx - lx) <= 9) & (np.abs(yy - lr) <= 9)
        Ip[..., 3] = np.where(dia, 255, np.where(near, 0, Ip[..., 3]))
        OId[near, :3] = oids[1]
        OId[..., 3] = np.where(near, 64, OId[..., 3])
        Id[near, :3] = ids[1]
        Id[..., 3] = np.where(near, (xx % 2) * 2, Id[..., 3])
        R[..., 3] = np.where(near, 255, R[..., 3])
        R[lr, lx, 3] = rw
        O[..., 3] = np.where(near, np.where((xx + yy) % 2 == 0, 255, 0), O[..., 3])
    # the far first-filter texel: its 37 taps, 14 texels apart, are its own object
    fx, fr = FAR_TEXEL
    O[fr, fx, 3] = 255
    for sx, sy in STENCIL3_37:
        Id[fr + 14 * sy, fx + 14 * sx], OId[fr + 14 * sy, fx + 14 * sx] = list(ids[3]) + [2], list(oids[3]) + [77]
        R[fr + 14 * sy, fx + 14 * sx, 3] = 255
    # whole tiles
    tx, ty = UNCOVERED_TILE
    t = (slice(16 * ty, 16 * ty + 16), slice(16 * tx, 16 * tx + 16))
    for p in planes:
        p[t] = np.maximum(p[t], 1)
    R[t + (3,)] = 0
    tx, ty = ONE_COVERED_TILE
    R[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16, 3] = 0
    R[ONE_COVERED_AT[1], ONE_COVERED_AT[0], 3] = 255
    tx, ty = ONE_UNCOVERED_TILE
    t = R[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16, 3]
    t[t == 0] = 255
    R[ONE_UNCOVERED_AT[1], ONE_UNCOVERED_AT[0], 3] = 0
    for sl in ((slice(18, 22), slice(0, 3)), (slice(H - 3, H), slice(W - 3, W))):     # all-zero id and original id, as outside the image: first-filter taps out there pass
        Id[sl], OId[sl], O[sl + (3,)] = 0, 0, 200
        R[sl + (3,)] = 255
    for k, v in enumerate((1, 254, 255)):                                             # OColor.w bytes the first filter must meet
        O[70 + k, 50, 3] = v
    return planes


@functools.lru_cache(maxsize=None)
def literal_case(W, H, seed, hdr):
    """-> (planes, the literal's frame, its masks): computed once per case and shared by the tests (read only)"""
    planes = make_planes(W, H, seed)
    out, masks = filter_literal(planes, hdr)
    for a in planes + [out]:
        a.setflags(write=False)
    return planes, out, masks


def pack_planes(planes):
    """five uint8 [H, W, 4] planes -> uint32 [5, H, W], R in the low byte: what flx_filter_planes_device reads"""
    return np.stack([np.ascontiguousarray(p).view(np.uint32)[..., 0] for p in planes])


def tile_of(mask2d, tx, ty):
    return mask2d[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16]


def coverage(planes, masks):
    """what a plane set asks of the chain, counted from the literal's masks -> {condition: count}; the tests assert every one > 0 on the main case"""
    R = planes[0]
    H, W = R.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    c = {}
    first = [m for m in masks if m["kind"] == "first"]
    second = [m for m in masks if m["kind"] == "second"]
    final = masks[-1]
    n = lambda a: int(np.count_nonzero(a))
    # first filter
    m = first[0]
    t = m["taps"] & m["covered"]
    c["first: all 37 taps inside at OColor.w = 255"] = n(t & (m["ocw"] == 255) & m["inside"].all(axis=0))
    far = t & (m["ocw"] == 255) & m["inside"].all(axis=0)
    for name, sel in (("left", m["cx"] - xx == -42), ("right", m["cx"] - xx == 42), ("above", m["crow"] - yy == -42), ("below", m["crow"] - yy == 42)):
        c["first: a passed tap 42 texels away, " + name] = n(far & (sel & m["passed"]).any(axis=0))
    for name, sel in (("left", m["cx"] < 0), ("right", m["cx"] >= W), ("above", m["crow"] < 0), ("below", m["crow"] >= H)):
        c["first: taps outside the image, " + name] = n(t & sel.any(axis=0))
    c["first: a tap outside the image that passes"] = sum(n(f["covered"] & ~f["inside"] & f["passed"]) for f in first)
    bytes_ = set(np.unique(m["ocw"][t]).tolist())
    c["first: 32 distinct OColor.w bytes among texels with taps"] = int(len(bytes_) >= 32)
    for k in (1, 254, 255):
        c["first: OColor.w = %d among texels with taps" % k] = int(k in bytes_)
    c["first: texels with OColor.w = 0"] = n(~m["taps"] & m["covered"])
    c["first: a tap rejected by the (light number, shadow) clause alone"] = sum(n(f["taps"] & f["covered"] & (f["inside"] & f["id3"] & f["oid4"] & ~f["light"])) for f in first)
    c["first: a tap rejected by the original id's w alone"] = sum(n(f["taps"] & f["covered"] & (f["inside"] & f["id3"] & f["light"] & f["oid3"] & ~f["oid4"])) for f in first)
    for k in range(4):
        c["first: idNumber %d chosen" % k] = sum(n(f["gate"] & (f["idNumber"] == k)) for f in first)
    c["first: a tie between neighbours of unequal id won by the later one"] = sum(n(f["tie_unequal"]) for f in first)
    c["first: a tie at a vote above zero, unequal ids"] = sum(n(f["tie_unequal"] & (f["maxVote"] > 0)) for f in first)
    c["first: renderColorIp.w = 1"] = sum(n(f["gate"] & f["covered"] & (f["ipw"] == 1)) for f in first)
    c["first: renderColorIp.w = 0 after the vote"] = sum(n(f["gate"] & f["covered"] & (f["ipw"] == 0)) for f in first)
    # second filter
    for name, b in (("both sums", 1), ("colour only", 2), ("nothing", 3)):
        c["second: a tap that takes " + name] = sum(n(s["covered"] & (s["branch"] == b)) for s in second)
    for k in (25, 26):
        c["second: a tap decided by min OId.w = %d" % k] = sum(n(s["covered"] & (s["branch"] != 0) & (s["minOIdW"] == k) & s["admit"]) for s in second)
        c["second: a tap with unequal ids decided by max Ip.w = %d" % k] = sum(n(s["covered"] & (s["branch"] != 0) & (s["minOIdW"] >= 26) & ~s["id4"] & (s["maxIpW"] == k)) for s in second)
    c["second: a tap whose id equals the centre's in three bytes but not in w"] = sum(n(s["covered"] & (s["branch"] == 2) & (s["minOIdW"] >= 26) & (s["maxIpW"] < 26) & s["id3"] & ~s["id4"]) for s in second)
    # final filter
    c["final: oCount == 0"] = n(final["covered"] & final["oCount0"])
    c["final: oCount != 0"] = n(final["covered"] & ~final["oCount0"])
    c["final: blurTranslucent true over unequal ids"] = n(final["covered"] & final["blur"] & final["oid3"] & ~final["id3"])
    c["final: a tap that only the id equality admits"] = n(final["covered"] & ~final["blur"] & final["oid3"] & final["id3"])
    c["final: a tap that only min OId.w = 0 keeps from blurring"] = n(final["covered"] & final["oid3"] & (final["maxIpW"] != 0) & (final["minOIdW"] == 0))
    c["final: a tap that only max Ip.w = 0 keeps from blurring"] = n(final["covered"] & final["oid3"] & (final["maxIpW"] == 0) & (final["minOIdW"] != 0) & ~final["id3"])
    # tiles of the second and the final filter
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    for m in second + [final]:
        used = m["covered"] & ((m["branch"] == 1) | (m["branch"] == 2) if m["kind"] == "second" else m["counted"])
        what = "%s (pass %d): " % (m["kind"], m["pass"])
        good = 0
        for ty in range(1, tiles_y - 1):
            for tx in range(1, tiles_x - 1):
                if 16 * tx + 32 > W or 16 * ty + 32 > H: continue                     # (its eight neighbours are whole tiles)
                inT = (xx // 16 == tx) & (yy // 16 == ty)
                u = used & inT
                lands = {(int(a), int(b)) for a, b in zip((m["cx"][u] // 16 - tx).tolist(), (m["crow"][u] // 16 - ty).tolist())}
                corner = inT & ((xx % 16 == 0) | (xx % 16 == 15)) & ((yy % 16 == 0) | (yy % 16 == 15))
                reach8 = (used & corner & (np.maximum(np.abs(m["cx"] - xx), np.abs(m["crow"] - yy)) == 8)).any()
                good += int(len(lands - {(0, 0)}) == 8 and bool(reach8) and int(m["reach"].max()) == 8)
        c[what + "an interior tile whose used taps land in all eight neighbours, 8 texels away from a corner"] = good
        for name, sel in (("left", m["cx"] < 0), ("right", m["cx"] >= W), ("above", m["crow"] < 0), ("below", m["crow"] >= H)):
            c[what + "taps beyond the image, " + name] = n(m["covered"] & sel)
    # tiles of the input planes
    rest = np.concatenate([R[..., :3]] + list(planes[1:]), axis=-1)
    zero_tile = one_cov = one_unc = 0
    for ty in range(H // 16):
        for tx in range(W // 16):
            cov = tile_of(R[..., 3] != 0, tx, ty)
            zero_tile += int(not cov.any() and bool((tile_of(rest, tx, ty) != 0).all()))
            one_cov += int(cov.sum() == 1)
            one_unc += int(cov.sum() == 255)
    c["tiles: a 16 x 16 tile with every R.w zero and every other byte non-zero"] = zero_tile
    c["tiles: a tile with exactly one covered texel"] = one_cov
    c["tiles: a tile with exactly one uncovered texel"] = one_unc
    c["planes: colour bytes take every value 0 .. 255"] = int(all(len(np.unique(p[..., :3])) == 256 for p in (planes[0], planes[2])))
    return c
