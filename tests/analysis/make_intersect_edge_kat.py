#!/usr/bin/env python3
"""Adversarial known answers for the intersection routines: rows placed on the float borders of the predicates, where the device's shortcuts (one product per
quotient with a 2^-21 margin, Markstein's corrected quotients, v_rcp_f32 + one FMA, the branch-free acceptance rule) could differ from the shader's arithmetic.

Answers come from tests/analysis/make_intersect_kat.py's moeller_trumbore, moeller_trumbore_cull and ray_cuboid (the shader text, one float32 operation per
operation; not through oracle/ nor include/flx_math.h).  Rows whose min / max see a NaN are KEPT, answered with pinned_nan=True (min / max are their defining
comparisons, the oracle's pin) and flagged.  Every float32 quotient a row's answer used is verified against the correctly rounded quotient from exact rational
arithmetic (fractions.Fraction).

The device's DECISION STRUCTURE (csrc/flx_device.h: reciprocalOfDir's fastDiv, rayCuboidRecip's aOk, rayCuboidInterval's sure and its boolean from the raw
products) is replayed here in float32 only to COUNT rows per path — never to produce an answer — and the file is not written unless the counts of CONDITIONS hold.

Writes tests/golden/intersect_edge_kat.json.gz:
    ray_cuboid             [l, origin 3, dir 3, min 3, max 3 | hit | class | 1 if a NaN reached min / max]
    moeller_trumbore       [tri 9, origin 3, dir 3, l | s, u, v | class]
    moeller_trumbore_cull  [tri 9, origin 3, dir 3, l | hit | class]          (the same inputs, row by row)
floats as float32 bit patterns.   usage: make_intersect_edge_kat.py [--check]"""
import gzip, json, os, struct, sys
from fractions import Fraction
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_intersect_kat import f32, bits, BIAS, sub, dot, cross, moeller_trumbore, moeller_trumbore_cull, ray_cuboid      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "intersect_edge_kat.json.gz")
POW32 = f32(4294967296.0)
P2 = lambda e: f32(2.0 ** e)
FLT_MAX = f32(3.4028234663852886e38)
INF, NAN = f32(np.inf), f32(np.nan)
DENORM = f32(1e-40)
LO, HI, OHI = P2(-60), P2(60), P2(59)           # reciprocalOfDir's range of the direction and of the origin (and of flx_scene_upload's box coordinates)
D21 = 2.0 ** -21                                # rayCuboidInterval's margin


def unbits(w):
    return f32(struct.unpack("<f", struct.pack("<I", int(w) & 0xffffffff))[0])


def step(x, n):
    """x moved by n float32 neighbours (n > 0: towards +inf)"""
    b = bits(x)
    k = -(b & 0x7fffffff) if b >> 31 else b
    k += int(n)
    return unbits((0x80000000 | -k) if k < 0 else k)


def ulps(x, y):
    """signed distance y - x in float32 neighbours"""
    o = lambda b: -(b & 0x7fffffff) if b >> 31 else b
    return o(bits(y)) - o(bits(x))


# ---- exact arithmetic ------------------------------------------------------------------------------------------------------------------------------

def rn32(x):
    """the float32 nearest to the rational x, ties to even, denormals and overflow as IEEE 754 has them (the sign of a zero result is the caller's)"""
    if x == 0: return f32(0.0)
    s, x = (-1, -x) if x < 0 else (1, x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x: e -= 1
    e = max(e, -126)
    q = x / Fraction(2) ** (e - 23)
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1): n += 1
    v = Fraction(n) * Fraction(2) ** (e - 23)
    if v >= Fraction(2) ** 128: return f32(s * np.inf)
    return f32(s * float(v))


QUOTIENTS = [0, 0]          # verified against exact arithmetic / special operands (IEEE's rules for them are numpy's)


def check_quotient(a, d):
    a, d = f32(a), f32(d)
    with np.errstate(all="ignore"):
        q = f32(a / d)
    if np.isfinite(a) and np.isfinite(d) and d != 0:
        want = rn32(Fraction(float(a)) / Fraction(float(d)))
        assert float(want) == float(q) and (q != 0 or want == 0), (a, d, q, want)          # (value and sign; a zero quotient's sign is the operands')
        assert q != 0 or bool(np.signbit(q)) == (bool(np.signbit(a)) != bool(np.signbit(d))), (a, d, q)
        QUOTIENTS[0] += 1
    else:
        QUOTIENTS[1] += 1
    return q


def fma32(x, y, z):
    """RN(x * y + z) from exact rational arithmetic"""
    return rn32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))


def corrected_quotient(a, d, corrections=2):
    """csrc/flx_device.h's divByRecip in exact arithmetic (finite operands): used to CHOOSE operands on which its preconditions matter, and to count them"""
    y = f32(f32(1) / d)
    q = f32(a * y)
    for _ in range(corrections):
        q = fma32(fma32(-q, d, a), y, q)
    return q


# ---- the device's decision structure, replayed to COUNT rows per path (never an answer) -----------------------------------------------------------------

def fmaD(x, sign):
    """RN(x + sign * |x| * 2^-21): the product is exact in float64, and so is the sum (45 significant bits)"""
    with np.errstate(all="ignore"):
        return f32(np.float64(x) + sign * abs(np.float64(x)) * D21)


def box_paths(r, flag=1):
    """(fastDiv, sure, aOk, boolean from the raw products) of a ray_cuboid row as csrc/flx_device.h decides them with walk_fast_boxes = flag"""
    v = [unbits(w) for w in r[:13]]
    l, o, d, mn, mx = v[0], v[1:4], v[4:7], v[7:10], v[10:13]
    fast = bool(flag) and all(LO <= abs(x) <= HI for x in d) and all(abs(x) <= OHI for x in o)
    with np.errstate(all="ignore"):
        a = [f32(mn[k] - o[k]) for k in range(3)] + [f32(mx[k] - o[k]) for k in range(3)]
        aok = all((bits(x) & 0x7fffffff) == 0 or (bits(x) & 0x7fffffff) >= 0x2b800000 for x in a)
        y = [f32(f32(1) / x) for x in d]
        q0 = [f32(a[k] * y[k]) for k in range(3)]
        q1 = [f32(a[3 + k] * y[k]) for k in range(3)]
        fmin = lambda p, q: q if (np.isnan(p) or q < p) else p           # (NaN operands: any lane of the test that sees one is not sure)
        fmax = lambda p, q: q if (np.isnan(p) or q > p) else p
        n = [fmin(q0[k], q1[k]) for k in range(3)]
        f = [fmax(q0[k], q1[k]) for k in range(3)]
        nyz, nxz, nxy = fmax(n[1], n[2]), fmax(n[0], n[2]), fmax(n[0], n[1])
        tmin, tmax = fmax(nxy, n[2]), fmin(fmin(f[0], f[1]), f[2])
        cx = fmaD(f[0], -1) >= fmaD(nyz, 1)
        cy = fmaD(f[1], -1) >= fmaD(nxz, 1)
        cz = fmaD(f[2], -1) >= fmaD(nxy, 1)
        sure_true = bool(cx and cy and cz and fmaD(tmax, -1) >= BIAS and fmaD(tmin, 1) < l)
        sure_false = bool(fmaD(tmax, 1) < fmax(fmaD(tmin, -1), BIAS) or fmaD(tmin, -1) >= l)
        sure = bool(fast and l >= LO and (sure_true or sure_false))
        raw = int(bool(tmax >= fmax(tmin, BIAS) and tmin < l))
    return fast, sure, aok, raw


def box_corrected_bool(r, corrections=2):
    """rayCuboidRecip's fast branch (every quotient through divByRecip) taken regardless of aOk, in exact arithmetic: to count the rows that need aOk"""
    v = [unbits(w) for w in r[:13]]
    l, o, d, mn, mx = v[0], v[1:4], v[4:7], v[7:10], v[10:13]
    v0 = [corrected_quotient(f32(mn[k] - o[k]), d[k], corrections) for k in range(3)]
    v1 = [corrected_quotient(f32(mx[k] - o[k]), d[k], corrections) for k in range(3)]
    tmin = max(min(v0[k], v1[k]) for k in range(3))
    tmax = min(max(v0[k], v1[k]) for k in range(3))
    return int(bool(tmax >= max(tmin, BIAS) and tmin < l))


def hard_quotients(rng, n):
    """(a, d) whose quotient lies within 2^-24 of a neighbour's distance of the midpoint of two floats — the operands on which a faithful quotient is hardest to round:
    with D the 24-bit significand of d, (2k + 1) D = +-1 (mod 2^25) makes a = ((2k + 1) D -+ 1) / 2^25 an integer and a / d = (2k + 1) / 2^25 -+ 1 / (2^25 D)"""
    out = []
    while len(out) < n:
        Dm = int(rng.integers(2 ** 23, 2 ** 24)) | 1
        rho = int(rng.choice([-1, 1]))
        k2 = (rho * pow(Dm, -1, 2 ** 25)) % (2 ** 25)
        A = (k2 * Dm - rho) >> 25
        if k2 < 2 ** 24 or not (2 ** 23 <= A < 2 ** 24): continue
        out.append((f32(f32(A) * P2(-22)), f32(f32(Dm) * P2(-23))))
    return out


def box_gap(r):
    """relative distance of the closer of the two comparisons that decide the literal boolean (tmax against max(tmin, BIAS), tmin against l)"""
    v = [unbits(w) for w in r[:13]]
    l, o, d, mn, mx = v[0], v[1:4], v[4:7], v[7:10], v[10:13]
    with np.errstate(all="ignore"):
        v0 = [np.float64(f32(f32(mn[k] - o[k]) / d[k])) for k in range(3)]
        v1 = [np.float64(f32(f32(mx[k] - o[k]) / d[k])) for k in range(3)]
        tmin = max(min(v0[k], v1[k]) for k in range(3))
        tmax = min(max(v0[k], v1[k]) for k in range(3))
        rel = lambda p, q: abs(p - q) / max(abs(p), abs(q)) if max(abs(p), abs(q)) > 0 else 0.0
        return min(rel(tmax, max(tmin, np.float64(BIAS))), rel(tmin, np.float64(l)))


def tri_values(r):
    """the literal routine's intermediates (det, u, v, u + v, s) of a triangle row: for the search and for the counts"""
    v = [unbits(w) for w in r[:16]]
    t, origin, d = [v[0:3], v[3:6], v[6:9]], v[9:12], v[12:15]
    with np.errstate(all="ignore"):
        edge1, edge2 = sub(t[1], t[0]), sub(t[2], t[0])
        pvec = cross(d, edge2)
        det = dot(edge1, pvec)
        inv_det = f32(f32(1) / det)
        tvec = sub(origin, t[0])
        u = f32(dot(tvec, pvec) * inv_det)
        qvec = cross(tvec, edge1)
        vv = f32(dot(d, qvec) * inv_det)
        s = f32(dot(edge2, qvec) * inv_det)
        return {"det": det, "u": u, "v": vv, "uv": f32(u + vv), "s": s}


# ---- box rows ------------------------------------------------------------------------------------------------------------------------------------------

class Boxes:
    def __init__(self, rng):
        self.rng, self.rows = rng, []

    def add(self, cls, l, o, d, mn, mx, perm=True):
        l, o, d, mn, mx = f32(l), [f32(x) for x in o], [f32(x) for x in d], [f32(x) for x in mn], [f32(x) for x in mx]
        if perm:
            p = self.rng.permutation(3)
            o, d, mn, mx = [o[k] for k in p], [d[k] for k in p], [mn[k] for k in p], [mx[k] for k in p]
        with np.errstate(all="ignore"):
            for k in range(3):
                check_quotient(f32(mn[k] - o[k]), d[k]); check_quotient(f32(mx[k] - o[k]), d[k])
        nan = ray_cuboid(l, o, d, mn, mx) is None
        hit = ray_cuboid(l, o, d, mn, mx, pinned_nan=True)
        self.rows.append([bits(l)] + [bits(x) for x in o + d + mn + mx] + [hit, cls, int(nan)])

    def pairs(self, n, inexact):
        """(a, d, R = RN(a / d)) with a, d > 0 random; inexact: only pairs whose product RN(a * RN(1 / d)) is NOT the quotient"""
        out = []
        while len(out) < n:
            a = f32(self.rng.uniform(0.5, 8.0)); d = f32(2.0 ** self.rng.uniform(-2.0, 2.0))
            R = f32(a / d)
            if inexact and f32(a * f32(f32(1) / d)) == R: continue
            out.append((a, d, R))
        return out

    def slab(self, a, d, near, sign):
        """the x planes and direction that put the quotient a / d (both > 0) on the near (or far) side of the slab; sign -1 mirrors the axis"""
        W = f32(4.0 * float(a) + 3.0)
        lo, hi = (a, f32(a + W)) if near else (f32(a - W), a)
        return (lo, hi, d) if sign > 0 else (f32(-hi), f32(-lo), f32(-d))

    def partner(self, value, near, sign, k):
        """the y planes and direction 2^k (an exact quotient) that put `value` on the near (far) side, the other plane far away"""
        s = P2(k)
        lo, hi = (f32(value * s), f32(1000.0 * s)) if near else (f32(-10.0 * s), f32(value * s))
        return (lo, hi, s) if sign > 0 else (f32(-hi), f32(-lo), f32(-s))

    def wide(self):
        s = P2(int(self.rng.integers(-3, 4)))
        return f32(-10.0 * s), f32(1000.0 * s), s

    def js(self, i, close, far):
        return close if i % 4 else close + far

    def margin_and_outside(self):
        rng = self.rng
        sg = lambda: 1 if rng.random() < 0.5 else -1
        for i, (a, d, R) in enumerate(self.pairs(170, True)):
            for j in self.js(i, [-1, 0, 1], [-4, -3, -2, 2, 3, 4]):
                # tmax against tmin: another axis' plane AT the quotient, moved by j neighbours (edge and corner grazing); even i: its far plane against this near one
                xl, xh, xd = self.slab(a, d, i % 2 == 0, sg())
                yl, yh, yd = self.partner(step(R, j), i % 2 == 1, sg(), int(rng.integers(-3, 4)))
                zl, zh, zd = self.wide()
                self.add("margin_tmax_tmin", 1e9, [0, 0, 0], [xd, yd, zd], [xl, yl, zl], [xh, yh, zh])
        for i, (a, d, R) in enumerate(self.pairs(170, True)):
            for j in self.js(i, [-1, 0, 1], [-4, -3, -2, 2, 3, 4]):
                xl, xh, xd = self.slab(a, d, True, sg())
                yl, yh, yd = self.wide(); zl, zh, zd = self.wide()
                self.add("margin_tmin_l", step(R, j), [0, 0, 0], [xd, yd, zd], [xl, yl, zl], [xh, yh, zh])
        # tmax against BIAS: the far plane's quotient within 4 neighbours of 2^-16, the origin inside the box on every axis
        found = 0
        while found < 240:
            d = f32(2.0 ** rng.uniform(-2.0, 2.0))
            a0 = f32(BIAS * d)
            cand = [(j, step(a0, j)) for j in range(-4, 5)]
            turn = [j for j, a in cand if (f32(a / d) >= BIAS) != (f32(a * f32(f32(1) / d)) >= BIAS)]
            if not turn: continue
            found += 1
            for j, a in cand:
                if j in turn or abs(j - turn[0]) == 1 or found % 4 == 0:
                    xl, xh, xd = self.slab(a, d, False, sg())
                    yl, yh, yd = self.wide(); zl, zh, zd = self.wide()
                    self.add("margin_tmax_bias", 1e9, [0, 0, 0], [xd, yd, zd], [xl, yl, zl], [xh, yh, zh])
        # just outside the band: the same three constructions 10 .. 31 neighbours apart (2^-21 relative is 4 .. 8 neighbours, 2^-19 is 16 .. 32)
        # (these rows hold the interval test's OWN answer where it is sure closest to the band: a sureTrue / sureFalse mix-up or a margin of the wrong sign fails them.  A
        # margin that is merely smaller does not: a product is never more than one neighbour from the quotient — checked below on the table and on 20 M random pairs when
        # this was written — so even 2^-23 |x|, one to two neighbours, brackets it; no row of any table can tell 2^-23 from 2^-21)
        for i, (a, d, R) in enumerate(self.pairs(210, False)):
            for j in (int(rng.integers(17, 32)) * sg(), int(rng.integers(10, 16)) * sg()):
                kind = i % 3
                if kind == 0:
                    xl, xh, xd = self.slab(a, d, i % 2 == 0, sg())
                    yl, yh, yd = self.partner(step(R, j), i % 2 == 1, sg(), int(rng.integers(-3, 4)))
                    l = 1e9
                elif kind == 1:
                    xl, xh, xd = self.slab(a, d, True, sg())
                    yl, yh, yd = self.wide()
                    l = step(R, j)
                else:
                    xl, xh, xd = self.slab(step(f32(BIAS * d), j), d, False, sg())
                    yl, yh, yd = self.wide()
                    l = 1e9
                zl, zh, zd = self.wide()
                self.add("outside_band", l, [0, 0, 0], [xd, yd, zd], [xl, yl, zl], [xh, yh, zh])

    def band(self):
        rng = self.rng
        sg = lambda: 1 if rng.random() < 0.5 else -1
        rd = lambda: f32(2.0 ** rng.uniform(-2.0, 2.0))
        # two inexact quotients within a few neighbours of each other: the fallback's exact quotients decide
        for i, (a, d, R) in enumerate(self.pairs(260, False)):
            dy = rd()
            j = int(rng.integers(-6, 7))
            ay = step(f32(R * dy), j)
            xl, xh, xd = self.slab(a, d, i % 2 == 0, sg())
            W = f32(4.0 * float(ay) + 3.0)
            yl, yh = (f32(ay - W), ay) if i % 2 == 0 else (ay, f32(ay + W))
            s = sg()
            if s < 0: yl, yh, dy = f32(-yh), f32(-yl), f32(-dy)
            zl, zh, zd = self.wide()
            self.add("band_graze", rng.choice([1e9, 4294967296.0]), [0, 0, 0], [xd, dy, zd], [xl, yl, zl], [xh, yh, zh])
        # near-midpoint quotients (hard_quotients): the exact quotient is all but a tie between two floats, so a corrected quotient that is only faithful rounds it
        # either way; another axis' plane at the quotient itself and at its two neighbours
        for i, (a, d) in enumerate(hard_quotients(rng, 60)):
            R = f32(a / d)
            assert corrected_quotient(a, d, 1) == R          # (one correction already rounds these correctly: y = RN(1 / d) and a faithful first product, Markstein's theorem)
            for j in (-1, 0, 1):
                xl, xh, xd = self.slab(a, d, i % 2 == 0, sg())
                yl, yh, yd = self.partner(step(R, j), i % 2 == 1, sg(), int(rng.integers(-3, 4)))
                zl, zh, zd = self.wide()
                self.add("band_midpoint", 1e9, [0, 0, 0], [xd, yd, zd], [xl, yl, zl], [xh, yh, zh])
        # flat boxes (mn == mx on one axis) met in their plane: the x slab's far plane at the plane's quotient, moved by j: hit in the plane / missed beside it
        for i in range(200):
            p, dy, dx = f32(rng.uniform(0.5, 8.0)), rd(), rd()
            Ry = f32(p / dy)
            ax = step(f32(Ry * dx), int(rng.integers(-5, 6)))
            xl, xh, xd = self.slab(ax, dx, False, sg())
            zl, zh, zd = self.wide()
            o_y = f32(0.0)
            if i % 4 == 0:                         # the same plane from an origin off zero: a = RN(p' - o) is whatever the subtraction gives
                o_y = f32(rng.normal()); p = f32(p + o_y)
            self.add("band_flat", 1e9, [0, o_y, 0], [xd, dy, zd], [xl, p, zl], [xh, p, zh])
        # the origin ON a plane: a == 0 exactly.  A flat box there is missed (tmax = 0 < BIAS); a box with the origin on its near plane decides by its other planes
        for i in range(120):
            p, dy, dx = f32(rng.normal(0.0, 3.0)), f32(rd() * sg()), rd()
            zl, zh, zd = self.wide()
            if i % 3 == 0:
                xl, xh, xd = self.wide()
                self.add("band_origin_on_flat", 1e9, [0, p, 0], [xd, dy, zd], [xl, p, zl], [xh, p, zh])
            else:
                h = f32(rng.uniform(0.5, 4.0))
                yl, yh = (p, f32(p + h)) if dy > 0 else (f32(p - h), p)
                xl, xh, xd = self.slab(step(f32(BIAS * dx), int(rng.integers(-4, 5))), dx, False, sg())      # and the x slab ends around BIAS
                self.add("band_origin_on_plane", 1e9, [0, p, 0], [xd, dy, zd], [xl, yl, zl], [xh, yh, zh])

    def a_ok(self):
        """|a| below 2^-40 (the corrected quotients' residuals would leave the normal range: rayCuboidRecip divides), and |a| at 2^-40 and its neighbours.
        Only tmin against l can depend on a quotient this small (tmax must reach BIAS), so l sits at the quotient, moved by j."""
        rng = self.rng
        sg = lambda: 1 if rng.random() < 0.5 else -1
        for i in range(280):
            if i < 160:
                cls = "aok_small"
                a = unbits(int(rng.integers(1, 0x2b800000)))                  # log-uniform over 0 < a < 2^-40, denormals included
                if i % 4 == 0: a = unbits(int(rng.integers(1, 0x00800000)))   # denormal
            else:
                cls = "aok_border"
                a = step(P2(-40), (i % 3) - 1)
            d = f32(2.0 ** (rng.uniform(-20.0, 60.0) if i % 2 else rng.uniform(-2.0, 2.0)))      # (quotients down to the denormals and to zero)
            with np.errstate(all="ignore"):
                R = f32(a / d)
            s = sg()
            hi = f32(OHI * f32(rng.uniform(0.5, 1.0)))                         # the far plane far enough for tmax >= BIAS at every d
            xl, xh, xd = (a, hi, d) if s > 0 else (f32(-hi), f32(-a), f32(-d))
            yl, yh, yd = self.wide(); zl, zh, zd = self.wide()
            l = step(R, int(rng.integers(-2, 3))) if i % 5 else f32(1e9)
            self.add(cls, l, [0, 0, 0], [xd, yd, zd], [xl, yl, zl], [xh, yh, zh])

    def aok_residual(self):
        """|a| so small (denormal, or below 2^-118) that the corrected quotients' residual leaves the normal range and divByRecip would NOT give RN(a / d): operands are
        kept only where the exact replay of divByRecip differs from the quotient, and l goes between the two values (and one neighbour to either side)"""
        rng = self.rng
        kept = 0
        while kept < 120:
            a = unbits(int(rng.integers(1, 0x00800000))) if rng.random() < 0.4 else unbits(int(rng.integers(0x00800000, 0x05000000)))
            d = f32(2.0 ** rng.uniform(-2.0, 2.0))
            with np.errstate(all="ignore"):
                R, qm = f32(a / d), corrected_quotient(a, d)
            if qm == R or R == 0: continue
            kept += 1
            hi = f32(OHI * f32(rng.uniform(0.5, 1.0)))
            for l in (max(R, qm), step(max(R, qm), 1), min(R, qm)):
                s = 1 if rng.random() < 0.5 else -1
                xl, xh, xd = (a, hi, d) if s > 0 else (f32(-hi), f32(-a), f32(-d))
                yl, yh, yd = self.wide(); zl, zh, zd = self.wide()
                self.add("aok_residual", l, [0, 0, 0], [xd, yd, zd], [xl, yl, zl], [xh, yh, zh])

    def generic(self, geom=1.0, dirs=1.0, inside=None, aimed=None):
        rng = self.rng
        c = rng.normal(0.0, 1.5, 3) * geom
        h = (np.abs(rng.normal(0.0, 1.0, 3)) + 0.05) * geom
        mn, mx = np.clip(c - h, -float(OHI), float(OHI)), np.clip(c + h, -float(OHI), float(OHI))
        if inside is None: inside = rng.random() < 0.5
        o = mn + rng.random(3) * (mx - mn) if inside else np.clip(rng.normal(0.0, 3.0, 3) * geom, -float(OHI), float(OHI))
        if aimed is None: aimed = rng.random() < 0.6
        if not inside and aimed:                                               # aimed through the box
            d = (mn + rng.random(3) * (mx - mn)) - o
            d = d / max(np.linalg.norm(d), 1e-300) * dirs
        else:
            d = rng.normal(0.0, 1.0, 3) * dirs
        return [f32(x) for x in o], [f32(x) for x in d], [f32(x) for x in mn], [f32(x) for x in mx]

    def borders(self):
        rng = self.rng
        sg = lambda: 1.0 if rng.random() < 0.5 else -1.0
        N = 36
        for name, base in (("dir_2^-60", LO), ("dir_2^60", HI)):
            for j in (-1, 0, 1):
                for i in range(N):
                    val = step(base, j)
                    if base == LO:
                        o, d, mn, mx = self.generic(1.0, 1.0)
                        d = [f32(float(LO) * rng.uniform(1.0, 4.0) * sg()) for _ in range(3)]
                        l = rng.choice([np.inf, 1e9, 2.0 ** 62])
                    else:
                        o, d, mn, mx = self.generic(2.0 ** 57, 1.0)
                        d = [f32(float(HI) * rng.uniform(0.25, 1.0) * np.sign(float(x) or 1.0)) for x in d]
                        l = rng.choice([np.inf, 1e9, 1.0])
                    k = int(rng.integers(0, 3))
                    d[k] = f32(float(val) * np.sign(float(d[k]) or 1.0))
                    self.add("%s%+d" % (name, j), l, o, d, mn, mx, perm=False)
        for name, val in (("dir_+0", f32(0.0)), ("dir_-0", f32(-0.0)), ("dir_denormal", DENORM), ("dir_+inf", INF), ("dir_-inf", f32(-np.inf)), ("dir_nan", NAN)):
            for i in range(N):
                o, d, mn, mx = self.generic()
                k = int(rng.integers(0, 3))
                d[k] = f32(val * f32(sg())) if name == "dir_denormal" else val
                if i % 6 == 0: d[(k + 1) % 3] = val                            # two such components
                if i % 4 == 1: o[k] = mn[k] if rng.random() < 0.5 else mx[k]   # the origin on one of the axis' planes: 0 / 0, 0 / inf
                self.add(name, rng.choice([1e9, 4294967296.0, 2.0]), o, d, mn, mx, perm=False)
        for j in (-1, 0, 1):
            for i in range(N):
                o, d, mn, mx = self.generic(2.0 ** 57, 1.0, inside=False)
                k = int(rng.integers(0, 3))
                s = sg()
                o[k] = f32(float(step(OHI, j)) * s)
                mn[k], mx[k] = sorted([f32(s * 2.0 ** 58 * rng.uniform(0.5, 1.0)), f32(s * float(OHI) * (1.0 if i % 2 else rng.uniform(0.6, 1.0)))])
                if i % 3:                                                      # aimed at the box from there
                    t = np.array([float(mn[q]) + rng.random() * (float(mx[q]) - float(mn[q])) for q in range(3)]) - np.array([float(x) for x in o])
                    d = [f32(x) for x in t / np.linalg.norm(t)]
                self.add("origin_2^59%+d" % j, rng.choice([np.inf, 2.0 ** 60, 2.0 ** 58]), o, d, mn, mx, perm=False)
        for name, val in (("l_2^-60-1", step(LO, -1)), ("l_2^-60+0", LO), ("l_2^-60+1", step(LO, 1)), ("l_pow32", POW32), ("l_+inf", INF), ("l_nan", NAN),
                          ("l_zero", f32(0.0)), ("l_negative", None)):
            for i in range(N):
                far = name in ("l_pow32", "l_+inf") and i % 2 == 0
                o, d, mn, mx = self.generic(2.0 ** 33 if far else 1.0, inside=(i % 3 != 0) and not far, aimed=(i % 4 != 0) if far else None)      # (distances around 2^32 for l = 2^32)
                self.add(name, f32(-abs(rng.normal(0.0, 2.0)) * (1e-3 if i % 2 else 1.0) - 1e-6) if val is None else val, o, d, mn, mx, perm=False)

    def unbounded(self):
        """a box coordinate beyond 2^59: flx_scene_upload clears walk_fast_boxes for such a scene, and these rows are run with the flag off"""
        rng = self.rng
        sg = lambda: 1.0 if rng.random() < 0.5 else -1.0
        big = [step(OHI, 1), P2(60), P2(61), P2(100), P2(120), FLT_MAX, INF]
        for i in range(150):
            o, d, mn, mx = self.generic()
            k = int(rng.integers(0, 3))
            v = big[i % len(big)]
            kind = i % 5
            if kind == 0: mx[k] = v                                            # a far floor: one plane beyond the bound
            elif kind == 1: mn[k] = f32(-v)
            elif kind == 2: mn[k], mx[k] = f32(-v), v
            elif kind == 3:                                                    # a quotient that overflows: the corrected quotients would make inf - inf of it
                mx[k] = v; d[k] = f32(2.0 ** rng.uniform(-60.0, -20.0) * sg())
            else:                                                              # everything huge, quotients of ordinary size: no reciprocal of such a direction is exact
                scale = 2.0 ** rng.uniform(110.0, 126.0)
                o, d, mn, mx = self.generic(inside=(i % 2 == 0))
                o, d, mn, mx = [[f32(float(x) * scale) for x in vec] for vec in (o, d, mn, mx)]
            self.add("unbounded", rng.choice([1e9, 4294967296.0, np.inf]), o, d, mn, mx, perm=False)
        # one direction component beyond 2^126 (its reciprocal is denormal: no v_rcp_f32 + one FMA gives it) over a slab of that size, so that its quotients are
        # ordinary; the other axes ordinary: rows that only a test that ignores the range of the direction gets wrong
        for i in range(80):
            dx = f32(2.0 ** rng.uniform(126.0, 127.99) * sg())
            t0, t1 = sorted([rng.uniform(-2.0, 6.0), rng.uniform(-2.0, 6.0)])
            xs = sorted([f32(t0 * float(dx)), f32(t1 * float(dx))])
            o, d, mn, mx = self.generic(inside=True)
            d[0], o[0], mn[0], mx[0] = dx, f32(0), xs[0], xs[1]
            self.add("unbounded_huge_dir", rng.choice([1e9, 4294967296.0, np.inf]), o, d, mn, mx)


# ---- triangle rows ---------------------------------------------------------------------------------------------------------------------------------------

class Triangles:
    """Triangles in the plane z = 0 of a cyclically permuted frame: a = 0, b = (ex, 0, 0), c = (0, ey, 0), so that det = -ex ey d_z, u ~ (o_x - o_z d_x / d_z) / ex,
    v ~ (o_y - o_z d_y / d_z) / ey and s = -o_z / d_z each follow ONE input at that input's own float resolution; the search moves that input neighbour by neighbour
    until the literal routine's intermediate is within two neighbours of the border.  (A triangle in general position rounds det, u, v on a grid thousands of
    neighbours wide around these borders: its rows cannot be aimed.)"""

    def __init__(self, rng):
        self.rng, self.rows = rng, []                   # rows: (16 input words, class)

    def base(self, dz=None, oblique=True):
        rng = self.rng
        ex, ey = f32(rng.uniform(0.5, 4.0)), f32(rng.uniform(0.5, 4.0))
        pu, pv = rng.dirichlet([1.0, 1.0, 1.0])[:2]
        dz = f32(-rng.uniform(0.3, 1.0)) if dz is None else f32(dz)              # negative: the front face (det > 0)
        dx, dy = (f32(rng.normal(0.0, 0.4)), f32(rng.normal(0.0, 0.4))) if oblique else (f32(0), f32(0))
        s0 = rng.uniform(0.5, 3.0)
        o = [f32(pu * float(ex) - s0 * float(dx)), f32(pv * float(ey) - s0 * float(dy)), f32(-s0 * float(dz))]
        return {"ex": ex, "ey": ey, "o": o, "d": [dx, dy, dz], "l": f32(1e9)}

    def words(self, g, rot):
        z = f32(0)
        pts = [[z, z, z], [g["ex"], z, z], [z, g["ey"], z], g["o"], g["d"]]
        pts = [[p[(k + rot) % 3] for k in range(3)] for p in pts]                  # a cyclic permutation of the axes keeps cross and dot
        return [bits(x) for p in pts for x in p] + [bits(g["l"])]

    def aim(self, cls, key, target, var, count, make, offsets=(-2, -1, 0, 1, 2), per_offset=None):
        """rows whose intermediate `key` is within `offsets` neighbours of `target`, found by bisecting input `var` (("o", k), ("d", k) or "ex") and scanning its neighbours"""
        got = {j: 0 for j in offsets}
        per_offset = per_offset or -(-count // len(offsets))
        tries = 0
        while min(got.values()) < per_offset and tries < 40 * count:
            tries += 1
            g = make()
            rot = int(self.rng.integers(0, 3))

            def setv(x):
                if var == "ex": g["ex"] = x
                else: g[var[0]][var[1]] = x

            def val(x):
                setv(x)
                return tri_values(self.words(g, rot))[key]
            x0 = g["ex"] if var == "ex" else g[var[0]][var[1]]
            lo_x, hi_x = step(x0, -2 ** 22), step(x0, 2 ** 22)                     # the start is near the border: a quarter of a binade to either side brackets it
            vl, vh = val(lo_x), val(hi_x)
            if not (np.isfinite(vl) and np.isfinite(vh)) or (vl < target) == (vh < target): continue
            a, b = 0, 2 ** 23
            while b - a > 1:
                m = (a + b) // 2
                if (val(step(lo_x, m)) < target) == (vl < target): a = m
                else: b = m
            for n in range(a - 6, a + 8):
                x = step(lo_x, n)
                j = ulps(target, val(x))
                if j in got and got[j] < per_offset:
                    got[j] += 1
                    setv(x)
                    self.rows.append((self.words(g, rot), "%s%+d" % (cls, j)))
        return got

    def build(self):
        rng = self.rng
        sg = lambda: 1.0 if rng.random() < 0.5 else -1.0
        one = f32(1)

        def near_det(target):                     # d_z starts where -ex ey d_z is the target; the hit point stays inside the triangle
            def make():
                g = self.base(dz=-1.0)
                g["d"][2] = f32(-float(target) / (float(g["ex"]) * float(g["ey"])) * rng.uniform(0.98, 1.02))
                g["o"][2] = f32(-rng.uniform(0.5, 3.0) * float(g["d"][2]))
                g["o"][0], g["o"][1] = f32(float(g["o"][0]) * 0.5), f32(float(g["o"][1]) * 0.5)
                g["d"][0], g["d"][1] = f32(float(g["d"][0]) * 2.0 ** -18), f32(float(g["d"][1]) * 2.0 ** -18)
                return g
            return make
        self.aim("det_+bias", "det", BIAS, ("d", 2), 60, near_det(BIAS))
        self.aim("det_-bias", "det", f32(-BIAS), ("d", 2), 60, near_det(-BIAS))

        def huge_det(sign):                       # ex ey |d_z| around 2^60, everything else scaled along: u, v, s stay ordinary
            def make():
                g = self.base(oblique=False)
                sc = 2.0 ** 20
                g["ex"], g["ey"] = f32(float(g["ex"]) * sc), f32(float(g["ey"]) * sc)
                g["d"][2] = f32(-sign * float(HI) / (float(g["ex"]) * float(g["ey"])) * rng.uniform(0.98, 1.02))
                s0 = rng.uniform(0.5, 3.0)
                pu, pv = rng.dirichlet([1.0, 1.0, 1.0])[:2]
                g["o"] = [f32(pu * float(g["ex"])), f32(pv * float(g["ey"])), f32(-s0 * float(g["d"][2]))]
                return g
            return make
        self.aim("det_+2^60", "det", HI, ("d", 2), 45, huge_det(1.0), offsets=(-1, 0, 1))
        self.aim("det_-2^60", "det", f32(-HI), ("d", 2), 45, huge_det(-1.0), offsets=(-1, 0, 1))

        def coord(k, frac, oblique):              # o_k starts where u (k = 0) or v (k = 1) is `frac`
            def make():
                g = self.base(oblique=oblique)
                e = float(g["ex"] if k == 0 else g["ey"])
                s0 = -float(g["o"][2]) / float(g["d"][2])
                g["o"][k] = f32((frac * rng.uniform(0.99, 1.01)) * e - s0 * float(g["d"][k]))
                return g
            return make
        for k, name in ((0, "u"), (1, "v")):
            self.aim(name + "_bias", name, BIAS, ("o", k), 40, coord(k, float(BIAS), False))
            self.aim(name + "_bias_oblique", name, BIAS, ("o", k), 10, coord(k, float(BIAS), True), per_offset=1)
            self.aim(name + "_one", name, one, ("o", k), 40, coord(k, 1.0, False))
            self.aim(name + "_one_oblique", name, one, ("o", k), 10, coord(k, 1.0, True), per_offset=1)

        def uv_sum(oblique):
            def make():
                g = self.base(oblique=oblique)
                s0 = -float(g["o"][2]) / float(g["d"][2])
                u = rng.uniform(0.05, 0.9)
                g["o"][0] = f32(u * float(g["ex"]) - s0 * float(g["d"][0]))
                g["o"][1] = f32((1.0 - u) * rng.uniform(0.99, 1.01) * float(g["ey"]) - s0 * float(g["d"][1]))
                return g
            return make
        self.aim("uv_one", "uv", one, ("o", 1), 40, uv_sum(False))
        self.aim("uv_one_oblique", "uv", one, ("o", 1), 10, uv_sum(True), per_offset=1)

        def s_bias():
            g = self.base()
            g["o"][2] = f32(-float(BIAS) * float(g["d"][2]) * rng.uniform(0.99, 1.01))
            s0 = float(BIAS)
            pu, pv = rng.dirichlet([1.0, 1.0, 1.0])[:2]
            g["o"][0], g["o"][1] = f32(pu * float(g["ex"]) - s0 * float(g["d"][0])), f32(pv * float(g["ey"]) - s0 * float(g["d"][1]))
            return g
        self.aim("s_bias", "s", BIAS, ("o", 2), 45, s_bias)

        for i in range(60):                       # s at l: l is the literal s, moved by j; front and back faces
            g = self.base(dz=rng.uniform(0.3, 1.0) * (1.0 if i % 3 == 0 else -1.0))
            rot = int(rng.integers(0, 3))
            s = tri_values(self.words(g, rot))["s"]
            j = i % 5 - 2
            g["l"] = step(s, j)
            self.rows.append((self.words(g, rot), "s_at_l%+d" % j))
        for i in range(330):                      # non-finite cases
            g = self.base(dz=rng.uniform(0.3, 1.0) * (1.0 if i % 3 == 0 else -1.0))
            rot = int(rng.integers(0, 3))
            kind = i % 6
            if kind == 0: g["l"] = INF; cls = "l_inf"
            elif kind == 1: g["l"] = NAN; cls = "l_nan"
            elif kind == 2:                       # det = +-inf: the direction overflows the products
                g["d"] = [f32(float(x) * 2.0 ** 126) for x in g["d"]]; g["ex"] = f32(float(g["ex"]) * 2.0 ** 3); cls = "det_inf"
            elif kind == 3:                       # det NaN: a NaN direction component (i % 12 == 3: all of them)
                g["d"][int(rng.integers(0, 3))] = NAN
                if i % 12 == 3: g["d"] = [NAN, NAN, NAN]
                cls = "det_nan"
            elif kind == 4:                       # s NaN under a finite det: an infinite origin coordinate times a zero edge coordinate
                g["o"][int(rng.integers(0, 3))] = f32(np.inf * sg()); cls = "s_nan"
            else:
                g["o"][int(rng.integers(0, 3))] = f32(np.inf * sg()); g["l"] = NAN; cls = "s_nan_l_nan"
            self.rows.append((self.words(g, rot), cls))
        for i in range(45):                       # |det| far beyond 2^60 (up to 2^127): 1 / det is denormal, no reciprocal instruction with one correction gives it
            g = self.base(oblique=False)
            sc = 2.0 ** rng.uniform(50.0, 63.4)
            g["ex"], g["ey"] = f32(float(g["ex"]) * sc), f32(float(g["ey"]) * sc)
            pu, pv = rng.dirichlet([1.0, 1.0, 1.0])[:2]
            g["o"] = [f32(pu * float(g["ex"])), f32(pv * float(g["ey"])), f32(-rng.uniform(0.5, 3.0) * float(g["d"][2]))]
            if i % 3 == 0: g["d"][2] = f32(-g["d"][2]); g["o"][2] = f32(-g["o"][2])
            self.rows.append((self.words(g, int(rng.integers(0, 3))), "det_huge"))
        for i in range(45):                       # s == 0: the origin in the triangle's plane.  A HIT with s == 0 cannot exist: fragment:138 rejects s <= BIAS and
            g = self.base()                       # fragment:157 requires s > BIAS before anything is returned; the rows pin that 0 (and -0) are misses of both rules
            g["o"][2] = f32(0.0) if i % 2 else f32(-0.0)
            if i % 5 == 0: g["l"] = f32(0.0)
            self.rows.append((self.words(g, int(rng.integers(0, 3))), "s_zero"))


def tri_tables(rows):
    mt, cull = [], []
    for w, cls in rows:
        v = [unbits(x) for x in w]
        t, origin, d, l = [v[0:3], v[3:6], v[6:9]], v[9:12], v[12:15], v[15]
        check_quotient(f32(1), tri_values(w)["det"])
        mt.append(list(w) + [bits(x) for x in moeller_trumbore(t, origin, d, l)] + [cls])
        cull.append(list(w) + [moeller_trumbore_cull(t, origin, d, l), cls])
    return mt, cull


# ---- the conditions on the table ------------------------------------------------------------------------------------------------------------------------

BORDER_ITEMS = ["dir_2^-60-1", "dir_2^-60+0", "dir_2^-60+1", "dir_2^60-1", "dir_2^60+0", "dir_2^60+1", "dir_+0", "dir_-0", "dir_denormal", "dir_+inf", "dir_-inf",
                "dir_nan", "origin_2^59-1", "origin_2^59+0", "origin_2^59+1", "l_2^-60-1", "l_2^-60+0", "l_2^-60+1", "l_pow32", "l_+inf", "l_nan", "l_zero", "l_negative"]
# border items whose rows can only miss: tmin < l has no true side when l is NaN; every finite a over an infinite direction component is 0, so tmax <= 0 < BIAS
ONE_ANSWER = {"l_nan", "dir_+inf", "dir_-inf"}
TRI_ITEMS = {name: 40 for name in ("det_+bias", "det_-bias", "det_+2^60", "det_-2^60", "det_inf", "det_nan", "det_huge", "u_bias", "u_one", "v_bias", "v_one", "uv_one", "s_bias",
                                   "s_at_l", "s_nan", "s_nan_l_nan", "l_inf", "l_nan", "s_zero")}
# rows per offset (in float32 neighbours) of the items that are aimed at a border: every offset of the issue's range is present, none carries the item alone
OFFSET_ITEMS = [(name, (-2, -1, 0, 1, 2), 8) for name in ("det_+bias", "det_-bias", "u_bias", "u_one", "v_bias", "v_one", "uv_one", "s_bias", "s_at_l")] + \
               [("det_+2^60", (-1, 0, 1), 12), ("det_-2^60", (-1, 0, 1), 12)]
# items on which the two-sided and the culling rule can disagree: back faces (det_-bias, det_-2^60, and the back-facing rows of s_at_l, l_inf), NaN s and NaN det
# (no comparison with a NaN rejects in the two-sided rule, none accepts in the culling one), NaN l.  s == l itself cannot: !(s > l) and (s <= l) agree for ordered s, l.
TRI_DIFFER = ["det_-bias", "det_-2^60", "det_nan", "s_nan", "s_nan_l_nan", "l_nan", "s_at_l"]


def tri_item(cls):
    for name in sorted(TRI_ITEMS, key=len, reverse=True):
        if cls == name or (cls.startswith(name) and cls[len(name)] in "+-_"): return name
    raise KeyError(cls)


def counts(data):
    """per class and per path; the conditions of the table are asserted on these (here before the file is written, and by tests/test_intersect_edges_cpu.py)"""
    c = {"box_class": {}, "tri_class": {}, "tri_differ": {}}
    way = {"margin_tmax_tmin": [0, 0], "margin_tmin_l": [0, 0], "margin_tmax_bias": [0, 0]}
    band = [0, 0]
    flat = {"band_flat": [0, 0], "band_origin_on_flat": [0, 0], "band_origin_on_plane": [0, 0]}
    outside = small = border = unbounded = nan_rows = fallback_total = 0
    flat_unsure, residual, huge_dir, midpoint, far_products = [0, 0], [0, 0], [0, 0], [0, 0], 0
    items = {k: [0, 0] for k in BORDER_ITEMS}
    for r in data["ray_cuboid"]:
        cls, hit = r[14], r[13]
        c["box_class"][cls] = c["box_class"].get(cls, 0) + 1
        nan_rows += r[15]
        fast, sure, aok, raw = box_paths(r)
        fallback_total += fast and not sure
        if cls in way and fast and raw != hit: way[cls][hit] += 1
        if fast:
            v = [unbits(w) for w in r[:13]]
            with np.errstate(all="ignore"):
                for k in range(3):
                    for plane in (v[7 + k], v[10 + k]):
                        a_, d_ = f32(plane - v[1 + k]), v[4 + k]
                        R_, q_ = f32(a_ / d_), f32(a_ * f32(f32(1) / d_))
                        if abs(R_) >= P2(-100): far_products = max(far_products, abs(ulps(R_, q_)))
        if cls.startswith("band_") and fast and not sure: band[hit] += 1
        if cls in flat: flat[cls][hit] += 1
        if cls == "band_flat" and fast and not sure: flat_unsure[hit] += 1
        if cls == "aok_residual" and fast and not sure and not aok and box_corrected_bool(r) != hit: residual[hit] += 1
        if cls == "band_midpoint" and fast and not sure and aok: midpoint[hit] += 1
        if cls == "unbounded_huge_dir": huge_dir[hit] += 1
        if cls == "outside_band" and sure and 2.0 ** -21 < box_gap(r) < 2.0 ** -19: outside += 1
        if cls.startswith("aok_"):
            a = []
            v = [unbits(w) for w in r[:13]]
            with np.errstate(all="ignore"):
                a = [abs(f32(v[7 + k] - v[1 + k])) for k in range(3)] + [abs(f32(v[10 + k] - v[1 + k])) for k in range(3)]
            if cls == "aok_small" and fast and not aok and any(0 < x < P2(-40) for x in a): small += 1
            if cls == "aok_border" and fast and any(abs(ulps(P2(-40), x)) <= 1 for x in a): border += 1
        if cls in items: items[cls][hit] += 1
        if cls.startswith("unbounded") and any(not (abs(unbits(w)) <= OHI) for w in r[7:13]): unbounded += 1
    c.update(far_products=far_products)
    c.update(flat_unsure=flat_unsure, aok_residual=residual, huge_dir=huge_dir, midpoint=midpoint)
    c.update(margin=way, band=band, flat=flat, outside=outside, aok_small=small, aok_border=border, border_items=items, unbounded=unbounded, box_nan_rows=nan_rows,
             fallback_rows=fallback_total)
    for m, k in zip(data["moeller_trumbore"], data["moeller_trumbore_cull"]):
        assert m[:16] == k[:16] and m[19] == k[17]
        item = tri_item(m[19])
        c["tri_class"][item] = c["tri_class"].get(item, 0) + 1
        c.setdefault("tri_exact", {})[m[19]] = c.get("tri_exact", {}).get(m[19], 0) + 1
        if (m[16:19] != [0, 0, 0]) != bool(k[16]): c["tri_differ"][item] = c["tri_differ"].get(item, 0) + 1
    c["tri_hits"] = sum(1 for m in data["moeller_trumbore"] if m[16:19] != [0, 0, 0])
    c["cull_hits"] = sum(k[16] for k in data["moeller_trumbore_cull"])
    return c


def check_conditions(c):
    for name, (n0, n1) in c["margin"].items():
        assert n0 >= 50 and n1 >= 50, ("margin: rows whose raw-product boolean differs from the answer, per way and answer", name, n0, n1)
    assert sum(a + b for a, b in c["margin"].values()) >= 300, c["margin"]
    assert sum(c["band"]) >= 300 and min(c["band"]) >= 50, ("band: fastDiv and not sure", c["band"])
    assert sum(c["flat"]["band_flat"]) >= 100 and min(c["flat_unsure"]) >= 30, (c["flat"], c["flat_unsure"])          # hit in the plane and missed beside it, the fallback deciding
    assert min(c["aok_residual"]) >= 40, ("rows whose answer differs from the corrected quotients' boolean (aOk must send them to the division)", c["aok_residual"])
    assert min(c["midpoint"]) >= 40, ("near-midpoint quotients on the fallback", c["midpoint"])
    assert min(c["huge_dir"]) >= 20, c["huge_dir"]
    assert c["far_products"] == 1, ("under fastDiv a product RN(a * RN(1 / d)) is the quotient or its neighbour", c["far_products"])
    assert c["flat"]["band_origin_on_flat"][0] >= 30 and min(c["flat"]["band_origin_on_plane"]) >= 10, c["flat"]
    assert c["outside"] >= 200, ("sure rows 2^-21 .. 2^-19 from the border", c["outside"])
    assert c["aok_small"] >= 100 and c["aok_border"] >= 100, (c["aok_small"], c["aok_border"])
    for name, (n0, n1) in c["border_items"].items():
        assert n0 + n1 >= 30, (name, n0, n1)
        assert name in ONE_ANSWER or min(n0, n1) >= 8, ("both answers", name, n0, n1)
    assert c["unbounded"] >= 100, c["unbounded"]
    for name, need in TRI_ITEMS.items():
        assert c["tri_class"].get(name, 0) >= need, (name, c["tri_class"].get(name, 0))
    for name, offsets, floor in OFFSET_ITEMS:
        for j in offsets:
            assert c["tri_exact"].get("%s%+d" % (name, j), 0) >= floor, ("rows per offset", name, j, c["tri_exact"].get("%s%+d" % (name, j), 0))
    for name in TRI_DIFFER:
        assert c["tri_differ"].get(name, 0) >= 10, ("rows on which the two rules differ", name, c["tri_differ"].get(name, 0))


def rows():
    rng = np.random.default_rng(20261016)
    b = Boxes(rng)
    b.margin_and_outside(); b.band(); b.a_ok(); b.aok_residual(); b.borders(); b.unbounded()
    t = Triangles(rng)
    t.build()
    mt, cull = tri_tables(t.rows)
    return {"ray_cuboid": b.rows, "moeller_trumbore": mt, "moeller_trumbore_cull": cull}


def report(c):
    print("rayCuboid rows per class:", json.dumps(c["box_class"], sort_keys=True))
    print("  margin (fastDiv, raw-product boolean != answer) [answer 0, answer 1]:", c["margin"])
    print("  band (fastDiv, not sure) [answer 0, answer 1]:", c["band"], " flat boxes:", c["flat"], " all rows on the fallback under fastDiv:", c["fallback_rows"])
    print("  just outside the band (sure, 2^-21 .. 2^-19):", c["outside"], " aOk false with 0 < |a| < 2^-40:", c["aok_small"], " |a| at 2^-40 +- 1:", c["aok_border"])
    print("  range borders [answer 0, answer 1]:", json.dumps(c["border_items"], sort_keys=True))
    print("  flat boxes on the fallback [0, 1]:", c["flat_unsure"], " aOk rows that divByRecip would answer wrongly [0, 1]:", c["aok_residual"], " near-midpoint rows on the fallback:",
          c["midpoint"], " direction beyond 2^126 over a slab of that size [0, 1]:", c["huge_dir"])
    print("  largest distance of a product from its quotient under fastDiv, in neighbours:", c["far_products"])
    print("  unbounded:", c["unbounded"], " rows with a NaN in min / max (pinned):", c["box_nan_rows"])
    print("triangle rows per item:", json.dumps(c["tri_class"], sort_keys=True), " hits:", c["tri_hits"], " cull hits:", c["cull_hits"])
    print("  rows on which the two rules differ:", json.dumps(c["tri_differ"], sort_keys=True))
    print("quotients verified against exact rational arithmetic: %d (and %d with a special operand)" % tuple(QUOTIENTS))


if __name__ == "__main__":
    data = rows()
    c = counts(data)
    report(c)
    check_conditions(c)
    if "--check" in sys.argv:
        assert json.load(gzip.open(OUT, "rt")) == data, "tests/golden/intersect_edge_kat.json.gz is not what this script writes"
        print("matches", OUT)
    else:
        with gzip.GzipFile(OUT, "wb", mtime=0) as fh:
            fh.write(json.dumps(data, separators=(",", ":")).encode())
        assert os.path.getsize(OUT) < 512 * 1024
        print("wrote", OUT, os.path.getsize(OUT), "bytes")
