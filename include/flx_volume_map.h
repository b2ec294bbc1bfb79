/*
 * flx_volume_map.h — directional visibility for probe volumes, exactly defined (include/flexlight_hip_debug.h, "directional visibility": flx_probe_map,
 * flx_probes_sh_map, flx_volume_bake_map, flx_volume_irradiance_map, flx_rays_irradiance_map, flx_frame_irradiance_map, flx_volume_irradiance_map_of).
 *
 * Every probe gets a small OCTAHEDRAL MAP of filtered distance moments: m x m bins over the octahedral square, each a row of four floats — the filter's weight
 * over the texels that hit, that weight times the first-hit distance, times its square, and the weight over all texels.  The map is reduced from the same radiance
 * rows as the probe's SH row (flx_probe.h), and the lookup (flx_volume.h) reads the bin that faces the sample point IN PLACE OF the SH row's whole-sphere moments
 * (words 7, 11 and 15): a wall on one side of a probe no longer decides what the probe may light on its other sides.  This file defines, in float32 with ONE
 * OPERATION PER ROUNDING (compiled with -ffp-contract=off like everything that shares flx_math.h): a bin's centre and direction, the bin of a direction, the four
 * terms a cube texel adds to a bin, the directional weight of a corner and the lookup.  flx_camera_ndc, flx_probe_texel, flx_probe_ray_at, flx_probe_weight and
 * flx_volume.h's pieces ARE CALLED, not restated.  The kernels (web-ray-tracer_amd/csrc/flx_volume_map.hip: k_probe_map; flx_volume.hip: k_volume_irradiance_map) and the CPU
 * reference of the tests (tests/volume_map_ref/flx_volume_map_ref.c) compile THIS text.  THE ORDER OF THE SUMS is flx_probe.h's and is written out above
 * flx_volume_map_terms below.  Plain C99, also valid C++ / HIP.  A numerical definition, not a renderer.
 *
 * LEFT OUT: bilinear taps between bins (the lookup reads the nearest bin only, so the weight steps where a direction crosses a bin's edge); borders around a map;
 * maps for groups of GPUs.  (Hysteresis between bakes is flx_volume_update.h's, probe relocation flx_volume_relocate.h's.)  Sizes 1 .. 3 are accepted because they are where the kernels can go wrong, not because
 * they are useful.
 */
#ifndef FLX_VOLUME_MAP_H
#define FLX_VOLUME_MAP_H

#include "flx_volume.h"

#define FLX_VOLUME_MAP_MAX_SIZE 16u        /* the largest m */
#define FLX_VOLUME_MAP_MAX_SHARPNESS 8u    /* the largest k: the filter's exponent is 2^8 */
#define FLX_VOLUME_MAP_ROW_WORDS 4u        /* a bin's row: one float4 */

/* bins of a probe's map */
FLX_HD uint32_t flx_volume_map_bins(const flx_volume_map *map) { return map->size * map->size; }

/* sgn(a) = (a >= 0) ? 1 : -1, applied to b as an exact product: b or -b */
FLX_HD float flx_volume_map_signed(float b, float a) { return (a >= 0.0f) ? b : -b; }

/* the lower half of the octahedron folded over: x = (1 - |v|) sgn(u), y = (1 - |u|) sgn(v) */
FLX_HD void flx_volume_map_fold(float u, float v, float *x, float *y) {
  const float ru = 1.0f - flx_abs(u), rv = 1.0f - flx_abs(v);
  *x = flx_volume_map_signed(rv, u);
  *y = flx_volume_map_signed(ru, v);
}

/* DECODE: the direction of the point (u, v) of the square.  z = (1 - |u|) - |v|; where z < 0 the fold, otherwise x = u and y = v; l = sqrt((x x + y y) + z z); three
 * quotients by l. */
FLX_HD void flx_volume_map_decode(float u, float v, float dir[3]) {
  const float ru = 1.0f - flx_abs(u);
  const float z = ru - flx_abs(v);
  float x = u, y = v;
  if (z < 0.0f) flx_volume_map_fold(u, v, &x, &y);
  const float xx = x * x, yy = y * y, zz = z * z;
  const float xxyy = xx + yy;
  const float l = flx_sqrt(xxyy + zz);
  dir[0] = x / l; dir[1] = y / l; dir[2] = z / l;
}

/* the direction of bin b = by m + bx: the decode of its centre, u = flx_camera_ndc(bx, m, 0), v = flx_camera_ndc(by, m, 0) */
FLX_HD void flx_volume_map_bin_direction(uint32_t m, uint32_t b, float dir[3]) {
  const uint32_t by = b / m, bx = b - by * m;
  flx_volume_map_decode(flx_camera_ndc(bx, m, 0.0f), flx_camera_ndc(by, m, 0.0f), dir);
}

/* one axis of the encode: g = ((p + 1) 0.5) (float)m; g = (g >= 0) ? g : 0 — A NaN BECOMES 0 —; min((uint32_t)g, m - 1).  (p is in [-1, 1] or a NaN: g <= m.) */
FLX_HD uint32_t flx_volume_map_axis(float p, uint32_t m) {
  const float half = (p + 1.0f) * 0.5f;
  float g = half * (float)m;
  g = (g >= 0.0f) ? g : 0.0f;
  const uint32_t i = (uint32_t)g;
  return i < m - 1u ? i : m - 1u;
}

/* ENCODE: the bin of the direction (x, y, z), which need not be of unit length.  l1 = (|x| + |y|) + |z|; where not l1 > 0 (zero or a NaN) the bin is 0; px = x / l1,
 * py = y / l1; where z < 0 the fold on (px, py); the bin is by m + bx of the two axes.  No index leaves the map. */
FLX_HD uint32_t flx_volume_map_bin(uint32_t m, float x, float y, float z) {
  const float axy = flx_abs(x) + flx_abs(y);
  const float l1 = axy + flx_abs(z);
  if (!(l1 > 0.0f)) return 0u;
  float px = x / l1, py = y / l1;
  if (z < 0.0f) { const float u = px, v = py; flx_volume_map_fold(u, v, &px, &py); }
  return flx_volume_map_axis(py, m) * m + flx_volume_map_axis(px, m);
}

/* What cube texel t of a probe gives every bin: its direction and d_omega — flx_probe_texel_terms' calls, no other —, and of its radiance row whether it hit
 * (word 3 != 0.0f, flx_probe_terms' rule) and the first-hit distance s (word 4). */
typedef struct flx_volume_map_texel { float d[3], dw, s; int hit; } flx_volume_map_texel;

FLX_HD flx_volume_map_texel flx_volume_map_texel_of(const flx_probe_grid *g, uint32_t t, float word3, float word4) {
  const float zero[3] = { 0.0f, 0.0f, 0.0f };
  uint32_t face, row, px;
  flx_volume_map_texel x;
  flx_probe_texel(g, t, &face, &row, &px);
  const flx_camera_row r = flx_probe_ray_at(zero, g, t, face, row, px);
  x.d[0] = r.dx; x.d[1] = r.dy; x.d[2] = r.dz;
  x.dw = flx_probe_weight(g, row, px);
  x.hit = word3 != 0.0f;
  x.s = word4;
  return x;
}

/* THE ORDER OF THE FOUR SUMS OF A BIN is flx_probe.h's, word for word (no function here computes it; the reference writes it out as loops, the kernel as lanes):
 *   There are 64 slots.  Slot j adds the terms of its texels t = j, j + 64, j + 128, .. in ascending order onto 0.0f; a slot that owns no texel stays 0.0f.
 *   Then, for off = 1, 2, 4, 8, 16, 32 in that order, every slot becomes v[j] + v[j ^ off].  A sum that meets a NaN is some NaN; its payload is not defined.
 * The bin's row is the four sums in the order of the terms.
 *
 * THE TERMS of texel x for the bin whose direction is b, with the sharpness k: c = (dx bx + dy by) + dz bz; c = (c > 0) ? c : 0; c squared k times (the exponent
 * 2^k); g = d_omega c.  term[0] = g over hits, term[1] = g s over hits, term[2] = g (s s) over hits, term[3] = g; a miss gives 0.0f to the first three. */
FLX_HD void flx_volume_map_terms(const flx_volume_map_texel *x, const float b[3], uint32_t k, float term[4]) {
  const float p0 = x->d[0] * b[0], p1 = x->d[1] * b[1], p2 = x->d[2] * b[2];
  const float p01 = p0 + p1;
  float c = p01 + p2;
  c = (c > 0.0f) ? c : 0.0f;
  for (uint32_t i = 0; i < k; i++) c = c * c;
  const float g = x->dw * c;
  const float ss = x->s * x->s;
  const float gs = g * x->s, gss = g * ss;
  term[0] = x->hit ? g : 0.0f;
  term[1] = x->hit ? gs : 0.0f;
  term[2] = x->hit ? gss : 0.0f;
  term[3] = g;
}

/* The bin a corner's probe is asked for: dir points from the sample point to the probe (flx_volume_weight_base), the map is looked up with (-dir0, -dir1, -dir2) —
 * the negation is exact —, the nearest bin. */
FLX_HD uint32_t flx_volume_map_corner_bin(const flx_volume_map *map, const float dir[3]) { return flx_volume_map_bin(map->size, -dir[0], -dir[1], -dir[2]); }

/* THE DIRECTIONAL WEIGHT of a corner whose base weight is tb = t wb and whose bin's row is q: w = tb wv.  q stands in for the SH row's words 7, 11 and 15: wv = 1
 * unless the grid's FLX_VOLUME_VISIBILITY is set and q[0] > 0 — a bin that nothing hit leaves the probe fully visible in that direction —; then mean = q[1] / q[0],
 * mean2 = q[2] / q[0] and flx_volume_visibility, the Chebyshev text the isotropic weight uses. */
FLX_HD float flx_volume_map_weight(const flx_volume_grid *g, float tb, float dist, const float q[4]) {
  float wv = 1.0f;
  if ((g->flags & FLX_VOLUME_VISIBILITY) != 0u && q[0] > 0.0f) {
    const float mean = q[1] / q[0], mean2 = q[2] / q[0];
    wv = flx_volume_visibility(mean, mean2, dist, g->floor);
  }
  return tb * wv;
}

/* The lookup with maps as one function over rows in memory (rows: flx_volume_probes(g) SH rows of 36 floats; maps: as many times m m rows of 4 floats, probe p's
 * from row p m m).  Everything but the weight is flx_volume_lookup's: the miss rule, the cell, the corners, the order of W and S, flx_volume_row.  The library
 * exports it as flx_volume_irradiance_map_of. */
FLX_HD void flx_volume_map_lookup(const flx_volume_grid *g, const flx_volume_map *map, const float *rows, const float *maps, const float position[4], const float normal[4],
                                  float out[4]) {
  float sums[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
  if (flx_volume_miss(position)) { out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f; out[3] = 0.0f; return; }
  const flx_volume_cell c = flx_volume_cell_of(g, position, normal);
  const uint32_t bins = flx_volume_map_bins(map);
  for (uint32_t k = 0; k < 8u; k++) {
    const uint32_t p = flx_volume_corner(g, &c, k);
    const float *sh = rows + (size_t)p * FLX_PROBE_SH_WORDS;
    float dist, dir[3];
    const float tb = flx_volume_weight_base(g, &c, k, normal, &dist, dir);
    const float *q = maps + ((size_t)p * bins + flx_volume_map_corner_bin(map, dir)) * FLX_VOLUME_MAP_ROW_WORDS;
    flx_volume_add(sums, flx_volume_map_weight(g, tb, dist, q), sh, normal);
  }
  flx_volume_row(sums, out);
}

#endif /* FLX_VOLUME_MAP_H */
