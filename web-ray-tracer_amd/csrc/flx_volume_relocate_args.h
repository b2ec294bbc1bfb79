/* flx_volume_relocate_args.h — what the probe-relocation calls (csrc/flx_volume_relocate.hip: flx_probe_relocate, flx_volume_positions_offset, flx_volume_relocate and
 * their _device forms; csrc/flx_volume.hip: the relocated lookups) decide about the relocation, the range of probes and their arrays before they ask the device
 * anything: plain C++, no HIP, so that a stand-alone program can hold it under the sanitizers (tests/volume_relocate_args_main.cc), in the manner of
 * flx_volume_update_args.h, whose array rules are used as they stand.  What the siblings decide — the scene, the grid, the map, the update — is theirs and is
 * asked first. */
#ifndef FLX_VOLUME_RELOCATE_ARGS_H
#define FLX_VOLUME_RELOCATE_ARGS_H

#include <stdint.h>

#include "flexlight_hip_debug.h"
#include "flx_probe_args.h"
#include "flx_volume_update_args.h"

#define FLX_VOLUME_RELOCATE_ROW_BYTES 16u          /* an offset row, a row of the HIT plane, a row of the NORMAL plane */
#define FLX_VOLUME_RELOCATE_WAVE_PROBES 4u         /* probes a workgroup of k_probe_relocate reduces: four waves, a probe each */
#define FLX_VOLUME_RELOCATE_THREADS 256u

enum flx_volume_relocate_refusal {
  FLX_VOLUME_RELOCATE_ARGS_OK = 0,
  FLX_VOLUME_RELOCATE_NULL,            /* no flx_volume_relocate */
  FLX_VOLUME_RELOCATE_BACK_SHARE,      /* not finite or outside [0, 1] */
  FLX_VOLUME_RELOCATE_MIN_FRONT,       /* negative or not finite */
  FLX_VOLUME_RELOCATE_REACH,           /* not > 0 or not finite */
  FLX_VOLUME_RELOCATE_LIMIT,           /* not finite or outside [0, 0.5] */
  FLX_VOLUME_RELOCATE_FLAGS,           /* a bit beyond FLX_VOLUME_RELOCATE_FREEZE */
  FLX_VOLUME_RELOCATE_RESERVED,        /* the reserved word is not 0 */
  FLX_VOLUME_RELOCATE_FACE_SIZE,       /* 0 or above 256 */
  FLX_VOLUME_RELOCATE_RANGE,           /* first_probe + n_probes beyond the grid */
  FLX_VOLUME_RELOCATE_ROWS             /* n_probes * 6 w w is 2^32 or more */
};

/* the relocation, in the order the header lists the refusals */
static inline enum flx_volume_relocate_refusal flx_volume_relocate_check(const struct flx_volume_relocate *r) {
  if (!r) return FLX_VOLUME_RELOCATE_NULL;
  if (!flx_probe_finite(r->back_share) || r->back_share < 0.0f || r->back_share > 1.0f) return FLX_VOLUME_RELOCATE_BACK_SHARE;
  if (!flx_probe_finite(r->min_front) || r->min_front < 0.0f) return FLX_VOLUME_RELOCATE_MIN_FRONT;
  if (!flx_probe_finite(r->reach) || !(r->reach > 0.0f)) return FLX_VOLUME_RELOCATE_REACH;
  if (!flx_probe_finite(r->limit) || r->limit < 0.0f || r->limit > 0.5f) return FLX_VOLUME_RELOCATE_LIMIT;
  if ((r->flags & ~FLX_VOLUME_RELOCATE_FREEZE) != 0u) return FLX_VOLUME_RELOCATE_FLAGS;
  if (r->reserved != 0u) return FLX_VOLUME_RELOCATE_RESERVED;
  return FLX_VOLUME_RELOCATE_ARGS_OK;
}

/* the face size and the probes first_probe .. first_probe + n_probes - 1 of a grid of `probes`: the end in 64 bits (both terms are below 2^32), the rows of a
 * plane in 64 bits; *rows <- n_probes * 6 w w of an accepted range */
static inline enum flx_volume_relocate_refusal flx_volume_relocate_range_check(uint32_t face_size, uint32_t first_probe, uint32_t n_probes, uint32_t probes, uint32_t *rows) {
  if (flx_probe_face_check(face_size) != FLX_PROBE_ARGS_OK) return FLX_VOLUME_RELOCATE_FACE_SIZE;
  if ((uint64_t)first_probe + (uint64_t)n_probes > (uint64_t)probes) return FLX_VOLUME_RELOCATE_RANGE;
  if (flx_probe_count_check(n_probes, face_size, rows) != FLX_PROBE_ARGS_OK) return FLX_VOLUME_RELOCATE_ROWS;
  return FLX_VOLUME_RELOCATE_ARGS_OK;
}

/* the bytes of n offset rows or plane rows */
static inline uint64_t flx_volume_relocate_row_bytes(uint32_t n) { return (uint64_t)n * FLX_VOLUME_RELOCATE_ROW_BYTES; }

/* probes of a chunk of flx_volume_relocate_device: flx_probes_sh_device's, max(1, 2^21 / R), lowered by flx_debug_set_probe_chunk */
static inline uint32_t flx_volume_relocate_chunk(uint32_t face_size, uint32_t ceiling) { return flx_probe_chunk(face_size, ceiling); }

/* workgroups of k_probe_relocate for n probes, four a workgroup, and of k_volume_positions_offset, 256 entries a workgroup (n below 2^31: neither wraps) */
static inline uint32_t flx_volume_relocate_groups(uint32_t n) { return n / FLX_VOLUME_RELOCATE_WAVE_PROBES + (n % FLX_VOLUME_RELOCATE_WAVE_PROBES != 0u ? 1u : 0u); }
static inline uint32_t flx_volume_relocate_position_groups(uint32_t n) { return n / FLX_VOLUME_RELOCATE_THREADS + (n % FLX_VOLUME_RELOCATE_THREADS != 0u ? 1u : 0u); }

#endif
