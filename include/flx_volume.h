/*
 * flx_volume.h — probe volumes, exactly defined (include/flexlight_hip_debug.h, "probe volumes": flx_volume_positions, flx_volume_bake, flx_volume_irradiance,
 * flx_rays_irradiance, flx_frame_irradiance, flx_volume_irradiance_of).
 *
 * A volume is a regular grid of light probes (flx_volume_grid) and one SH row per probe (flx_probe.h's 144 bytes).  This file defines, in float32 with ONE
 * OPERATION PER ROUNDING (every product, sum, quotient and root is its own statement or parenthesis; compiled with -ffp-contract=off like everything that shares
 * flx_math.h): the position of a probe, and THE LOOKUP — the irradiance the grid gives a surface point with a normal: the eight probes around the point, weighted
 * trilinearly, against back faces and by the visibility moments of their rows, each probe's irradiance being flx_probe_irradiance_of's — THAT FUNCTION AND
 * flx_probe_basis ARE CALLED, not restated.  The kernels (web-ray-tracer_amd/csrc/flx_volume.hip: k_volume_positions, k_volume_irradiance) and the CPU reference of
 * the tests (tests/volume_ref/flx_volume_ref.c) compile THIS text.  Plain C99, also valid C++ / HIP.  A numerical definition, not a renderer.
 *
 * THE MOMENTS ARE THOSE OF THE WHOLE SPHERE, NOT OF A DIRECTION.  A row's words 7, 11 and 15 are sums over every texel that hit: their quotients are the mean and
 * the mean square of the distance to whatever the probe sees, all around.  The visibility weight is Chebyshev's bound on "a surface as far as this point lies in
 * front of the probe" under that one distribution, so it is ISOTROPIC: it dims a probe for points further away than its surroundings on average, whatever lies
 * between the two.  It keeps light from leaking through walls where probes sit close to them and it darkens open rooms seen from a corner; the directional
 * (octahedral) visibility map per probe that cures both is flx_volume_map.h's, read by calls of its own beside these.  FLX_VOLUME_VISIBILITY is a flag so that a
 * caller can turn the test off, isotropic or directional.
 */
#ifndef FLX_VOLUME_H
#define FLX_VOLUME_H

#include "flx_probe.h"

#define FLX_VOLUME_BACK_FLOOR 0.2f      /* what the back-face weight keeps of a probe straight behind the surface */

/* probes of a grid: nx ny nz (below 2^31 for an accepted grid: csrc/flx_volume_args.h) */
FLX_HD uint32_t flx_volume_probes(const flx_volume_grid *g) { return g->count[0] * g->count[1] * g->count[2]; }

/* the index of probe (ix, iy, iz): p = (iz ny + iy) nx + ix */
FLX_HD uint32_t flx_volume_index(const flx_volume_grid *g, uint32_t ix, uint32_t iy, uint32_t iz) { return (iz * g->count[1] + iy) * g->count[0] + ix; }

/* the position of probe i along axis a: origin + (float)i spacing — one product, then one sum */
FLX_HD float flx_volume_axis(const flx_volume_grid *g, int a, uint32_t i) {
  const float step = (float)i * g->spacing[a];
  return g->origin[a] + step;
}

/* the position row of probe p (flx_probes_sh's input: word 3 is 0.0f) */
FLX_HD void flx_volume_position(const flx_volume_grid *g, uint32_t p, float row[4]) {
  const uint32_t ix = p % g->count[0], rest = p / g->count[0];
  const uint32_t iy = rest % g->count[1], iz = rest / g->count[1];
  row[0] = flx_volume_axis(g, 0, ix); row[1] = flx_volume_axis(g, 1, iy); row[2] = flx_volume_axis(g, 2, iz); row[3] = 0.0f;
}

/* A surface row is A MISS where word 3 of its position is 0.0f (-0.0f is; a NaN is not): its irradiance row is four 0.0f and no probe is read. */
FLX_HD int flx_volume_miss(const float position[4]) { return position[3] == 0.0f; }

/* What the eight corners of a point share: the sample point x' = n normal_bias + x (the product first), the base index i and the fraction f per axis.
 *   g = (x' - origin) / spacing; g = (g >= 0) ? g : 0 — A NaN BECOMES 0 —; g = (g <= (float)(count - 1)) ? g : (float)(count - 1);
 *   i = min((uint32_t)g, count - 2) where count >= 2, else 0; f = g - (float)i.
 * No index ever leaves the grid: the corners are at min(i + k, count - 1).  ((float)(count - 1) may round up where count > 2^24: i is cut to count - 2 all the same.) */
typedef struct flx_volume_cell { float x[3], f[3]; uint32_t i[3]; } flx_volume_cell;

FLX_HD flx_volume_cell flx_volume_cell_of(const flx_volume_grid *g, const float position[4], const float n[3]) {
  flx_volume_cell c;
  for (int a = 0; a < 3; a++) {
    const float lift = n[a] * g->normal_bias;
    const float x = lift + position[a];
    const float off = x - g->origin[a];
    const float last = (float)(g->count[a] - 1u);
    float q = off / g->spacing[a];
    q = (q >= 0.0f) ? q : 0.0f;
    q = (q <= last) ? q : last;
    const uint32_t whole = (uint32_t)q;
    const uint32_t most = g->count[a] >= 2u ? g->count[a] - 2u : 0u;
    const uint32_t i = whole < most ? whole : most;
    c.x[a] = x;
    c.i[a] = i;
    c.f[a] = q - (float)i;
  }
  return c;
}

/* the probe at corner k = kx + 2 ky + 4 kz of a cell: min(i_a + k_a, count_a - 1) per axis */
FLX_HD uint32_t flx_volume_corner_axis(const flx_volume_grid *g, const flx_volume_cell *c, int a, uint32_t k) {
  const uint32_t i = c->i[a] + ((k >> a) & 1u), last = g->count[a] - 1u;
  return i < last ? i : last;
}

FLX_HD uint32_t flx_volume_corner(const flx_volume_grid *g, const flx_volume_cell *c, uint32_t k) {
  return flx_volume_index(g, flx_volume_corner_axis(g, c, 0, k), flx_volume_corner_axis(g, c, 1, k), flx_volume_corner_axis(g, c, 2, k));
}

/* The weight of corner k, whose probe's row is sh: w = (t wb) wv.
 *   t  = (tx ty) tz, t_a = k_a ? f_a : 1 - f_a: the trilinear weight.
 *   wb = c c + 0.2, c = ((dir . n) + 1) 0.5: d = probe - x' per axis (the probe's position by flx_volume_axis), dist = sqrt((dx dx + dy dy) + dz dz),
 *        dir = d / dist — three quotients —, zero where dist == 0; dir . n = (dirx nx + diry ny) + dirz nz.
 *   wv = 1 unless the grid's FLX_VOLUME_VISIBILITY is set and sh[7] > 0.  Then mean = sh[11] / sh[7], mean2 = sh[15] / sh[7], var = |mean2 - mean mean| (the
 *        product first); where dist > mean: delta = dist - mean, den = var + delta delta, ch = den > 0 ? var / den : 0, wv = flx_max((ch ch) ch, floor) — a NaN
 *        cube stays a NaN —; otherwise wv = 1. */
/* the first part of the weight, which a directional map (flx_volume_map.h) shares: -> t wb; *dist_out and dir_out: dist and dir as defined above */
FLX_HD float flx_volume_weight_base(const flx_volume_grid *g, const flx_volume_cell *c, uint32_t k, const float n[3], float *dist_out, float dir_out[3]) {
  float t[3], d[3];
  for (int a = 0; a < 3; a++) {
    t[a] = ((k >> a) & 1u) ? c->f[a] : 1.0f - c->f[a];
    d[a] = flx_volume_axis(g, a, flx_volume_corner_axis(g, c, a, k)) - c->x[a];
  }
  const float txy = t[0] * t[1];
  const float tri = txy * t[2];
  const float xx = d[0] * d[0], yy = d[1] * d[1], zz = d[2] * d[2];
  const float xxyy = xx + yy;
  const float dist = flx_sqrt(xxyy + zz);
  const int apart = dist != 0.0f;                         /* (a NaN distance is apart, and carries its NaN on) */
  const float dir0 = apart ? d[0] / dist : 0.0f, dir1 = apart ? d[1] / dist : 0.0f, dir2 = apart ? d[2] / dist : 0.0f;
  const float p0 = dir0 * n[0], p1 = dir1 * n[1], p2 = dir2 * n[2];
  const float p01 = p0 + p1;
  const float cosine = p01 + p2;
  const float half = (cosine + 1.0f) * 0.5f;
  const float half2 = half * half;
  const float wb = half2 + FLX_VOLUME_BACK_FLOOR;
  *dist_out = dist;
  dir_out[0] = dir0; dir_out[1] = dir1; dir_out[2] = dir2;
  return tri * wb;
}

/* the second part: wv of the moments' quotients mean and mean2 for a point dist away — Chebyshev's bound, cubed, kept above floor; 1 where dist > mean does not hold */
FLX_HD float flx_volume_visibility(float mean, float mean2, float dist, float floor) {
  const float mm = mean * mean;
  const float var = flx_abs(mean2 - mm);
  float wv = 1.0f;
  if (dist > mean) {
    const float delta = dist - mean;
    const float dd = delta * delta;
    const float den = var + dd;
    const float ch = den > 0.0f ? var / den : 0.0f;
    const float ch2 = ch * ch;
    wv = flx_max(ch2 * ch, floor);
  }
  return wv;
}

FLX_HD float flx_volume_weight(const flx_volume_grid *g, const flx_volume_cell *c, uint32_t k, const float n[3], const float sh[36]) {
  float dist, dir[3];
  const float tb = flx_volume_weight_base(g, c, k, n, &dist, dir);
  float wv = 1.0f;
  if ((g->flags & FLX_VOLUME_VISIBILITY) != 0u && sh[7] > 0.0f) {
    const float mean = sh[11] / sh[7], mean2 = sh[15] / sh[7];
    wv = flx_volume_visibility(mean, mean2, dist, g->floor);
  }
  return tb * wv;
}

/* THE SAME TWO PARTS FOR A PROBE THAT DOES NOT STAND ON THE LATTICE (flx_volume_relocate.h: the lattice point plus an offset).  flx_volume_weight_base_at is
 * flx_volume_weight_base's text with the probe's position given as `at`, and flx_volume_weight_of is flx_volume_weight's second half; with at_a = flx_volume_axis of
 * the corner they give the functions above bit for bit (tests/test_volume_relocate_cpu.py holds them to it).  They stand beside the originals, which do not call
 * them, so that the plain lookups' compiled code stays what it was: a change to either pair is a change to both. */
FLX_HD float flx_volume_weight_base_at(const flx_volume_cell *c, uint32_t k, const float n[3], const float at[3], float *dist_out, float dir_out[3]) {
  float t[3], d[3];
  for (int a = 0; a < 3; a++) {
    t[a] = ((k >> a) & 1u) ? c->f[a] : 1.0f - c->f[a];
    d[a] = at[a] - c->x[a];
  }
  const float txy = t[0] * t[1];
  const float tri = txy * t[2];
  const float xx = d[0] * d[0], yy = d[1] * d[1], zz = d[2] * d[2];
  const float xxyy = xx + yy;
  const float dist = flx_sqrt(xxyy + zz);
  const int apart = dist != 0.0f;
  const float dir0 = apart ? d[0] / dist : 0.0f, dir1 = apart ? d[1] / dist : 0.0f, dir2 = apart ? d[2] / dist : 0.0f;
  const float p0 = dir0 * n[0], p1 = dir1 * n[1], p2 = dir2 * n[2];
  const float p01 = p0 + p1;
  const float cosine = p01 + p2;
  const float half = (cosine + 1.0f) * 0.5f;
  const float half2 = half * half;
  const float wb = half2 + FLX_VOLUME_BACK_FLOOR;
  *dist_out = dist;
  dir_out[0] = dir0; dir_out[1] = dir1; dir_out[2] = dir2;
  return tri * wb;
}

FLX_HD float flx_volume_weight_of(const flx_volume_grid *g, float tb, float dist, const float sh[36]) {
  float wv = 1.0f;
  if ((g->flags & FLX_VOLUME_VISIBILITY) != 0u && sh[7] > 0.0f) {
    const float mean = sh[11] / sh[7], mean2 = sh[15] / sh[7];
    wv = flx_volume_visibility(mean, mean2, dist, g->floor);
  }
  return tb * wv;
}

/* THE ORDER OF THE SUMS: W and S_c start at 0.0f; corner k = 0 .. 7 in ascending order adds w_k to W and w_k E_k,c (the product first) to S_c, E_k =
 * flx_probe_irradiance_of(row_k, n) — also where the corner's trilinear weight is 0: there is one path.  sums: W, S_0, S_1, S_2. */
FLX_HD void flx_volume_add(float sums[4], float w, const float sh[36], const float n[3]) {
  float e[3];
  flx_probe_irradiance_of(sh, n, e);
  const float s0 = w * e[0], s1 = w * e[1], s2 = w * e[2];
  sums[0] = sums[0] + w;
  sums[1] = sums[1] + s0; sums[2] = sums[2] + s1; sums[3] = sums[3] + s2;
}

/* The irradiance row of the four sums: (S_0 / W, S_1 / W, S_2 / W, W); four 0.0f where W <= 0.  (W > 0 and W <= 0 part the numbers; A NaN W IS NEITHER and takes
 * the quotients: a NaN anywhere gives some NaN, whose payload is not defined.) */
FLX_HD void flx_volume_row(const float sums[4], float out[4]) {
  const int none = sums[0] <= 0.0f;
  out[0] = none ? 0.0f : sums[1] / sums[0];
  out[1] = none ? 0.0f : sums[2] / sums[0];
  out[2] = none ? 0.0f : sums[3] / sums[0];
  out[3] = none ? 0.0f : sums[0];
}

/* The lookup as one function over SH rows in memory (rows: flx_volume_probes(g) rows of 36 floats).  position: a FLX_SURFACE_POSITION row (x, y, z, hit);
 * normal: a FLX_SURFACE_NORMAL row, USED AS GIVEN, not normalised (word 3 is ignored).  The library exports it as flx_volume_irradiance_of. */
FLX_HD void flx_volume_lookup(const flx_volume_grid *g, const float *rows, const float position[4], const float normal[4], float out[4]) {
  float sums[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
  if (flx_volume_miss(position)) { out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f; out[3] = 0.0f; return; }
  const flx_volume_cell c = flx_volume_cell_of(g, position, normal);
  for (uint32_t k = 0; k < 8u; k++) {
    const float *sh = rows + (size_t)flx_volume_corner(g, &c, k) * FLX_PROBE_SH_WORDS;
    flx_volume_add(sums, flx_volume_weight(g, &c, k, normal, sh), sh, normal);
  }
  flx_volume_row(sums, out);
}

#endif /* FLX_VOLUME_H */
