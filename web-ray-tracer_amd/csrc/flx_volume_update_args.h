/* flx_volume_update_args.h — what the volume-update calls (csrc/flx_volume_update.hip: flx_volume_positions_list, flx_volume_blend, flx_volume_update and their
 * _device forms) decide about the update, the list and their arrays before they ask the device anything: plain C++, no HIP, so that a stand-alone program can hold
 * it under the sanitizers (tests/volume_update_args_main.cc), in the manner of flx_volume_map_args.h.  What the siblings decide — the scene, the trace and probe
 * params, the grid, the map — is theirs and is asked first. */
#ifndef FLX_VOLUME_UPDATE_ARGS_H
#define FLX_VOLUME_UPDATE_ARGS_H

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "flexlight_hip_debug.h"
#include "flx_probe_args.h"      /* flx_probe_finite; FLX_PROBE_POSITION_BYTES, FLX_PROBE_SH_BYTES */
#include "flx_range_args.h"
#include "flx_volume_map_args.h"

#define FLX_VOLUME_UPDATE_WORD_BYTES 4u           /* an index of the list, a state */
#define FLX_VOLUME_UPDATE_MAX_ARRAYS 6            /* the blend's: indices, new SH rows, new map rows, SH rows, map rows, states */
#define FLX_VOLUME_UPDATE_WAVE_ENTRIES 4u         /* entries a workgroup of k_volume_blend blends: four waves, an entry each */
#define FLX_VOLUME_UPDATE_THREADS 256u

enum flx_volume_update_refusal {
  FLX_VOLUME_UPDATE_ARGS_OK = 0,
  FLX_VOLUME_UPDATE_NULL,            /* no flx_volume_update */
  FLX_VOLUME_UPDATE_HYSTERESIS,      /* h not finite or outside [0, 1] */
  FLX_VOLUME_UPDATE_RESERVED,        /* the reserved word is not 0 */
  FLX_VOLUME_UPDATE_COUNT,           /* n_list above the grid's probes */
  FLX_VOLUME_UPDATE_STRIDE,          /* the arithmetic list: stride 0 with more than one entry */
  FLX_VOLUME_UPDATE_END,             /* the arithmetic list: its last entry is not a probe of the grid */
  FLX_VOLUME_UPDATE_MAPS_ALONE,      /* maps without a map */
  FLX_VOLUME_UPDATE_MAP_ALONE,       /* a map without maps */
  FLX_VOLUME_UPDATE_ARRAY_NULL,      /* a NULL array */
  FLX_VOLUME_UPDATE_MISALIGNED,      /* an array off its alignment */
  FLX_VOLUME_UPDATE_WRAPS,           /* an array's end leaves 64 bits */
  FLX_VOLUME_UPDATE_OVERLAP,         /* two arrays of a call share a byte */
  FLX_VOLUME_UPDATE_DUPLICATE        /* a host list names a probe of the grid twice */
};

/* the update and the list of n_list entries for a grid of `probes` probes (accepted: 1 .. 2^31 - 1), in the order the header lists the refusals.  has_list: a
 * list is given, and first and stride are not read.  The arithmetic list's last entry is first + (n_list - 1) stride in 64 bits: both factors are below 2^32, the
 * product below 2^64 - 2^33, and the sum cannot wrap. */
static inline enum flx_volume_update_refusal flx_volume_update_check(const struct flx_volume_update *u, int has_list, uint32_t n_list, uint32_t probes) {
  if (!u) return FLX_VOLUME_UPDATE_NULL;
  if (!flx_probe_finite(u->hysteresis) || u->hysteresis < 0.0f || u->hysteresis > 1.0f) return FLX_VOLUME_UPDATE_HYSTERESIS;
  if (u->reserved != 0u) return FLX_VOLUME_UPDATE_RESERVED;
  if (n_list > probes) return FLX_VOLUME_UPDATE_COUNT;
  if (!has_list && n_list > 0u) {
    if (u->stride == 0u && n_list > 1u) return FLX_VOLUME_UPDATE_STRIDE;
    const uint64_t last = (uint64_t)u->first + (uint64_t)(n_list - 1u) * (uint64_t)u->stride;
    if (last >= (uint64_t)probes) return FLX_VOLUME_UPDATE_END;
  }
  return FLX_VOLUME_UPDATE_ARGS_OK;
}

/* the map and the maps arrays of a call go together (has_maps: any maps array of the call is given; all_maps: every one is) */
static inline enum flx_volume_update_refusal flx_volume_update_pairing(int has_map, int has_maps, int all_maps) {
  if (!has_map && has_maps) return FLX_VOLUME_UPDATE_MAPS_ALONE;
  if (has_map && !all_maps) return FLX_VOLUME_UPDATE_MAP_ALONE;
  return FLX_VOLUME_UPDATE_ARGS_OK;
}

/* the bytes of a list's indices or states, of n entries' or probes' SH rows, of so many map rows */
static inline uint64_t flx_volume_update_word_bytes(uint32_t n) { return (uint64_t)n * FLX_VOLUME_UPDATE_WORD_BYTES; }
static inline uint64_t flx_volume_update_sh_bytes(uint32_t n) { return (uint64_t)n * FLX_PROBE_SH_BYTES; }
static inline uint64_t flx_volume_update_position_bytes(uint32_t n) { return (uint64_t)n * FLX_PROBE_POSITION_BYTES; }

/* an array of a call: where it lies, its bytes (> 0), its alignment (4 or 16) and whether the call may go without it (then a NULL address is no array) */
struct flx_update_array { uint64_t address, bytes; uint32_t align; int optional; };

static inline int flx_update_array_absent(const flx_update_array &a) { return a.optional && a.address == 0u; }

/* the k <= 6 arrays of a call: none NULL that must be there, none off its alignment, none leaving 64 bits, no two sharing a byte — in that order */
static inline enum flx_volume_update_refusal flx_volume_update_arrays_check(const flx_update_array *a, int k) {
  for (int i = 0; i < k; i++)
    if (a[i].address == 0u && !a[i].optional) return FLX_VOLUME_UPDATE_ARRAY_NULL;
  for (int i = 0; i < k; i++)
    if (!flx_update_array_absent(a[i]) && (a[i].address & (uint64_t)(a[i].align - 1u)) != 0u) return FLX_VOLUME_UPDATE_MISALIGNED;
  for (int i = 0; i < k; i++)
    if (!flx_update_array_absent(a[i]) && flx_range_wraps(a[i].address, a[i].bytes)) return FLX_VOLUME_UPDATE_WRAPS;
  for (int i = 0; i < k; i++)
    for (int j = i + 1; j < k; j++)
      if (!flx_update_array_absent(a[i]) && !flx_update_array_absent(a[j]) && flx_ranges_overlap(a[i].address, a[i].bytes, a[j].address, a[j].bytes)) return FLX_VOLUME_UPDATE_OVERLAP;
  return FLX_VOLUME_UPDATE_ARGS_OK;
}

/* a list in host memory: whether two entries name the same probe of the grid (entries out of range are skipped by the kernel and may repeat) */
static inline int flx_volume_update_duplicate(const uint32_t *indices, uint32_t n_list, uint32_t probes) {
  std::vector<uint32_t> seen;
  seen.reserve(n_list);
  for (uint32_t j = 0; j < n_list; j++)
    if (indices[j] < probes) seen.push_back(indices[j]);
  std::sort(seen.begin(), seen.end());
  return std::adjacent_find(seen.begin(), seen.end()) != seen.end();
}

/* workgroups of k_volume_blend for n_list entries, four a workgroup, and of k_volume_positions_list, 256 a workgroup (n_list below 2^31: neither wraps, and both
 * fit a one-dimensional grid) */
static inline uint32_t flx_volume_update_blend_groups(uint32_t n_list) { return n_list / FLX_VOLUME_UPDATE_WAVE_ENTRIES + (n_list % FLX_VOLUME_UPDATE_WAVE_ENTRIES != 0u ? 1u : 0u); }
static inline uint32_t flx_volume_update_position_groups(uint32_t n_list) { return n_list / FLX_VOLUME_UPDATE_THREADS + (n_list % FLX_VOLUME_UPDATE_THREADS != 0u ? 1u : 0u); }

#endif
