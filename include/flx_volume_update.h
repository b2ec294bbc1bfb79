/*
 * flx_volume_update.h — a probe volume updated over time, exactly defined (include/flexlight_hip_debug.h, "volume updates": flx_volume_positions_list,
 * flx_volume_blend, flx_volume_update, flx_volume_blend_row_of).
 *
 * A volume that lives over many frames is not re-baked whole.  Each frame a LIST of its probes is retraced with a new random_seed and the new rows are blended
 * into the resident ones with a hysteresis h: old + (new - old) (1 - h).  Every sum of an SH row (flx_probe.h) and of a map row (flx_volume_map.h) is linear in
 * the radiance rows, so blending the sums is blending the moments, and the lookup's text needs no change.  This file defines, in float32 with ONE OPERATION PER
 * ROUNDING (compiled with -ffp-contract=off like everything that shares flx_math.h): the probe an entry of the list names, the position row the entry is traced
 * from, THE STATE of an entry — blended, taken, kept, skipped —, the blend of a word, and what a map row does under its probe's state.  flx_volume_position IS
 * CALLED, not restated.  The kernels (web-ray-tracer_amd/csrc/flx_volume_update.hip: k_volume_positions_list, k_volume_blend) and the CPU reference of the tests
 * (tests/volume_update_ref/flx_volume_update_ref.c) compile THIS text.  Plain C99, also valid C++ / HIP.  A numerical definition, not a renderer.
 *
 * A POISONED NEW ROW IS REJECTED.  About one ray in 100 000 of a path tracer is a NaN, and one NaN texel makes a probe's whole SH row NaNs (flx_probe.h: a sum that
 * meets a NaN is some NaN).  An entry whose new SH row holds a word that is not finite leaves its probe as it was; a resident row that is not finite, or that was
 * never baked, is replaced and not blended.  "Finite" is a matter of bits: the exponent bits are not all ones.
 *
 * OVERFLOW IS LEFT AS IEEE GIVES IT: the difference of two finite words of opposite sign may be an infinity, its product with g = 0 a NaN, and the sum is then
 * what the operations give.  The next update finds the word not finite and takes the new row.
 *
 * LEFT OUT: a hysteresis per probe that adapts to how much the probe's surroundings changed, updates for groups of GPUs.  (Probe relocation is flx_volume_relocate.h's:
 * flx_volume_update_relocated traces the listed probes from their offset positions and blends as this file says.)
 *
 * (struct flx_volume_update has no typedef: the call that runs the whole path bears the same name, and a function and a structure tag may share one in C and
 * in C++ alike.)
 */
#ifndef FLX_VOLUME_UPDATE_H
#define FLX_VOLUME_UPDATE_H

#include "flx_volume_map.h"

#define FLX_VOLUME_UPDATE_BLENDED 0u      /* every word is old + ((new - old) g) */
#define FLX_VOLUME_UPDATE_TAKEN 1u        /* the new row's bits are copied */
#define FLX_VOLUME_UPDATE_KEPT 2u         /* the new SH row is poisoned: the probe keeps its SH row and all its map rows */
#define FLX_VOLUME_UPDATE_SKIPPED 3u      /* the entry names no probe of the grid: nothing of the volume is read or written */

/* finite: the exponent bits are not all ones (neither an infinity nor a NaN) */
FLX_HD int flx_volume_update_finite(float x) { return (flx_f2u(x) & 0x7f800000u) != 0x7f800000u; }

/* the four words of a float4, and the 36 of an SH row */
FLX_HD int flx_volume_update_finite4(const float v[4]) {
  return flx_volume_update_finite(v[0]) & flx_volume_update_finite(v[1]) & flx_volume_update_finite(v[2]) & flx_volume_update_finite(v[3]);
}

FLX_HD int flx_volume_update_finite_row(const float row[FLX_PROBE_SH_WORDS]) {
  int ok = 1;
  for (uint32_t i = 0; i < FLX_PROBE_SH_WORDS; i += 4u) ok &= flx_volume_update_finite4(row + i);
  return ok;
}

/* THE LIST.  Entry j names the probe indices[j] where a list is given, otherwise first + j stride, COMPUTED IN 64 BITS: a rotating subset (first = frame % stride)
 * runs with no list made anywhere, and no product wraps back into the grid. */
FLX_HD uint64_t flx_volume_update_arithmetic(const struct flx_volume_update *u, uint32_t j) { return (uint64_t)u->first + (uint64_t)j * (uint64_t)u->stride; }

FLX_HD uint64_t flx_volume_update_entry(const struct flx_volume_update *u, const uint32_t *indices, uint32_t j) {
  return indices ? (uint64_t)indices[j] : flx_volume_update_arithmetic(u, j);
}

/* whether an entry names a probe of the grid; one that does not is SKIPPED */
FLX_HD int flx_volume_update_in_grid(const flx_volume_grid *g, uint64_t index) { return index < (uint64_t)flx_volume_probes(g); }

/* THE POSITION ROW an entry is traced from: flx_volume_position of its probe.  A skipped entry gets the position of probe nx ny nz - 1, so that the trace has
 * something inside the grid to work on; the blend ignores its rows.  No index leaves the grid. */
FLX_HD void flx_volume_update_position(const flx_volume_grid *g, uint64_t index, float row[4]) {
  const uint32_t probes = flx_volume_probes(g);
  flx_volume_position(g, flx_volume_update_in_grid(g, index) ? (uint32_t)index : probes - 1u, row);
}

/* THE STATE of an entry, the rules tried in this order:
 *   3 SKIPPED  the index is not below nx ny nz.
 *   2 KEPT     any of the 36 words of the NEW SH row is not finite.
 *   1 TAKEN    h == 0; or the OLD row's word 3 (the sum of d_omega over all texels) is not > 0 — never baked, zero-initialised, or a NaN —; or any old word is
 *              not finite.
 *   0 BLENDED  otherwise.
 * new_finite, old_finite: flx_volume_update_finite_row of the two rows; old_word3: the old row's word 3. */
FLX_HD uint32_t flx_volume_update_state(int in_grid, int new_finite, int old_finite, float old_word3, float h) {
  if (!in_grid) return FLX_VOLUME_UPDATE_SKIPPED;
  if (!new_finite) return FLX_VOLUME_UPDATE_KEPT;
  if (h == 0.0f || !(old_word3 > 0.0f) || !old_finite) return FLX_VOLUME_UPDATE_TAKEN;
  return FLX_VOLUME_UPDATE_BLENDED;
}

/* g = 1 - h, computed once per call */
FLX_HD float flx_volume_update_gain(float h) { return 1.0f - h; }

/* THE BLEND of a word: old + ((new - old) g) — the difference, the product, the sum.  A word whose new bits equal its old ones keeps them: the three operations
 * give that too (the difference is 0.0f), but for -0.0f, which the sum would turn into 0.0f; so a row whose new bits equal its old ones keeps them for every h. */
FLX_HD float flx_volume_update_word(float old, float nw, float g) {
  const float d = nw - old;
  const float dg = d * g;
  const float sum = old + dg;
  return flx_f2u(nw) == flx_f2u(old) ? old : sum;
}

FLX_HD void flx_volume_update_blend4(const float old[4], const float nw[4], float g, float out[4]) {
  out[0] = flx_volume_update_word(old[0], nw[0], g); out[1] = flx_volume_update_word(old[1], nw[1], g);
  out[2] = flx_volume_update_word(old[2], nw[2], g); out[3] = flx_volume_update_word(old[3], nw[3], g);
}

/* four words of an SH row under its probe's state, BLENDED or TAKEN (a KEPT or SKIPPED entry writes nothing) */
FLX_HD void flx_volume_update_sh4(uint32_t state, const float old[4], const float nw[4], float g, float out[4]) {
  if (state == FLX_VOLUME_UPDATE_TAKEN) { out[0] = nw[0]; out[1] = nw[1]; out[2] = nw[2]; out[3] = nw[3]; return; }
  flx_volume_update_blend4(old, nw, g, out);
}

/* A MAP ROW follows its probe's state, BLENDED or TAKEN, with two exceptions of its own: a row with a NEW word that is not finite keeps its old bits (-> 0, and
 * out is the old row); where the probe blends, a row with an OLD word that is not finite takes the new bits.  -> whether the row changes hands (1: store out). */
FLX_HD int flx_volume_update_map_row(uint32_t state, const float old[4], const float nw[4], float g, float out[4]) {
  if (!flx_volume_update_finite4(nw)) { out[0] = old[0]; out[1] = old[1]; out[2] = old[2]; out[3] = old[3]; return 0; }
  flx_volume_update_sh4(flx_volume_update_finite4(old) ? state : FLX_VOLUME_UPDATE_TAKEN, old, nw, g, out);
  return 1;
}

/* One probe as one function over rows in memory: its resident SH row sh (36 floats) and its bins resident map rows maps (4 floats each; bins may be 0), the
 * entry's new rows beside them; the resident rows are updated in place.  -> the state (never SKIPPED: the caller has found the probe).  The library exports it
 * as flx_volume_blend_row_of. */
FLX_HD uint32_t flx_volume_update_probe(const struct flx_volume_update *u, uint32_t bins, const float *new_sh, const float *new_maps, float *sh, float *maps) {
  const uint32_t state = flx_volume_update_state(1, flx_volume_update_finite_row(new_sh), flx_volume_update_finite_row(sh), sh[3], u->hysteresis);
  const float g = flx_volume_update_gain(u->hysteresis);
  if (state == FLX_VOLUME_UPDATE_KEPT) return state;
  for (uint32_t i = 0; i < FLX_PROBE_SH_WORDS; i += 4u) {
    float out[4];
    flx_volume_update_sh4(state, sh + i, new_sh + i, g, out);
    sh[i] = out[0]; sh[i + 1u] = out[1]; sh[i + 2u] = out[2]; sh[i + 3u] = out[3];
  }
  for (uint32_t b = 0; b < bins; b++) {
    float out[4];
    float *row = maps + (size_t)b * FLX_VOLUME_MAP_ROW_WORDS;
    if (flx_volume_update_map_row(state, row, new_maps + (size_t)b * FLX_VOLUME_MAP_ROW_WORDS, g, out)) { row[0] = out[0]; row[1] = out[1]; row[2] = out[2]; row[3] = out[3]; }
  }
  return state;
}

#endif /* FLX_VOLUME_UPDATE_H */
