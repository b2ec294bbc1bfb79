/* flx_gather_args.h — what flx_rays_trace_gather[_device] (csrc/flx_rays_gather.hip) decide about a flx_gather_volume beyond the checks the trace calls and the
 * volume calls already have (flx_query_args.h, flx_volume_args.h, flx_volume_map_args.h): plain C++, no HIP, so that a stand-alone program can hold it under the
 * sanitizers (tests/gather_args_main.cc), in the manner of flx_volume_args.h; the range arithmetic is flx_range_args.h's. */
#ifndef FLX_GATHER_ARGS_H
#define FLX_GATHER_ARGS_H

#include <stdint.h>

#include "flexlight_hip_debug.h"
#include "flx_probe_args.h"      /* flx_probe_finite */
#include "flx_query_args.h"      /* flx_trace_slab_rays */
#include "flx_range_args.h"

#define FLX_GATHER_RECORD_FLOAT4 4u       /* a path record: four float4 a (ray, sample) — include/flx_gather.h */
#define FLX_GATHER_SLOTS 5u               /* 16-byte slots of scratch a (ray, sample): the record and the slot the resolve reads */
#define FLX_GATHER_THREADS 256u
#define FLX_GATHER_MAX_ARRAYS 3           /* SH rows, maps, offsets */
#define FLX_GATHER_HAS_MAP 1u             /* flx_debug_last_gather's flags */
#define FLX_GATHER_HAS_OFFSETS 2u

enum flx_gather_refusal {
  FLX_GATHER_ARGS_OK = 0,
  FLX_GATHER_VOLUME_NULL,            /* no flx_gather_volume */
  FLX_GATHER_GAIN,                   /* gain negative or not finite */
  FLX_GATHER_RESERVED,               /* the reserved word is not 0 */
  FLX_GATHER_MAP_PAIR,               /* map without maps, or maps without map */
  FLX_GATHER_OVERLAP                 /* an array of the volume shares a byte with the rays or the radiance */
};

/* the words of a flx_gather_volume that are this call's own, in the order the header lists the refusals (the grid, the map and the arrays have checkers of their own) */
static inline enum flx_gather_refusal flx_gather_volume_check(int have_volume, float gain, uint32_t reserved, int have_map, int have_maps) {
  if (!have_volume) return FLX_GATHER_VOLUME_NULL;
  if (!flx_probe_finite(gain) || gain < 0.0f) return FLX_GATHER_GAIN;
  if (reserved != 0u) return FLX_GATHER_RESERVED;
  if ((have_map != 0) != (have_maps != 0)) return FLX_GATHER_MAP_PAIR;
  return FLX_GATHER_ARGS_OK;
}

/* the k <= 3 arrays of the volume (addresses as integers, none NULL, none wrapping: their own checks came first) against the n > 0 rows of 32 bytes of the rays and of
 * the radiance (neither wrapping: the trace's check came first) */
static inline enum flx_gather_refusal flx_gather_arrays_check(const uint64_t *address, const uint64_t *bytes, int k, uint64_t rays, uint64_t radiance, uint32_t n) {
  const uint64_t rows = (uint64_t)n * FLX_RAY_ROW_BYTES;
  for (int i = 0; i < k; i++)
    if (flx_ranges_overlap(address[i], bytes[i], rays, rows) || flx_ranges_overlap(address[i], bytes[i], radiance, rows)) return FLX_GATHER_OVERLAP;
  return FLX_GATHER_ARGS_OK;
}

/* The slot count flx_trace_slab_rays is asked with: five 16-byte slots a (ray, sample), so that records plus slots stay under the traced batches' 256 MB; it
 * saturates where 5 samples leaves 32 bits (the slab is 64 rays then either way). */
static inline uint32_t flx_gather_slab_slots(uint32_t samples) { return samples > UINT32_MAX / FLX_GATHER_SLOTS ? UINT32_MAX : samples * FLX_GATHER_SLOTS; }
static inline uint32_t flx_gather_slab_rays(uint32_t samples, uint32_t ceiling) { return flx_trace_slab_rays(flx_gather_slab_slots(samples), ceiling); }

/* workgroups of k_gather_ambient for a slab's records (rays x samples, which the host keeps below 2^32: see flx_rays_gather.hip): 256 lanes each */
static inline uint32_t flx_gather_groups(uint64_t records) { return (uint32_t)((records + (FLX_GATHER_THREADS - 1u)) / FLX_GATHER_THREADS); }

#endif
