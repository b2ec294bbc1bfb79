/* flx_query_args.h — what flx_rays_cast_device decides about its arguments before it asks the device anything: plain C++, no HIP, so that a stand-alone program
 * can hold it under the sanitizers (tests/ray_query_args_main.cc). */
#ifndef FLX_QUERY_ARGS_H
#define FLX_QUERY_ARGS_H

#include <stdint.h>

#include "flx_range_args.h"      /* the range arithmetic, and FLX_RAY_ROW_BYTES: a ray row and a hit row alike */

enum flx_query_refusal {
  FLX_QUERY_ARGS_OK = 0,
  FLX_QUERY_WHAT_NONE,               /* neither FLX_RAYS_CLOSEST nor FLX_RAYS_OCCLUDED */
  FLX_QUERY_WHAT_UNKNOWN,            /* a bit beyond FLX_RAYS_COUNT */
  FLX_QUERY_NULL,                    /* a NULL array */
  FLX_QUERY_WRAPS,                   /* an array of n rows would end beyond the address space */
  FLX_QUERY_OVERLAP                  /* the rays' bytes and the hits' bytes overlap */
};

/* rays, hits: the two addresses as integers; n > 0 rows of 32 bytes each (n * 32 in 64 bits: a uint32_t n cannot overflow it; address + bytes can) */
static inline enum flx_query_refusal flx_query_args_check(uint64_t rays, uint64_t hits, uint32_t n, uint32_t what) {
  if ((what & ~7u) != 0u) return FLX_QUERY_WHAT_UNKNOWN;
  if ((what & 3u) == 0u) return FLX_QUERY_WHAT_NONE;
  if (rays == 0u || hits == 0u) return FLX_QUERY_NULL;
  const uint64_t bytes = (uint64_t)n * FLX_RAY_ROW_BYTES;
  if (flx_range_wraps(rays, bytes) || flx_range_wraps(hits, bytes)) return FLX_QUERY_WRAPS;
  if (flx_ranges_overlap(rays, bytes, hits, bytes)) return FLX_QUERY_OVERLAP;
  return FLX_QUERY_ARGS_OK;
}

/* flx_rays_trace_device's arguments (csrc/flx_rays_trace.hip; tests/rays_trace_args_main.cc holds this under the sanitizers): the params first, then — for n > 0 only,
 * as n == 0 enqueues nothing and looks at no array — the two arrays of n rows of 32 bytes */
enum flx_trace_refusal {
  FLX_TRACE_ARGS_OK = 0,
  FLX_TRACE_PARAMS_NULL,             /* no params */
  FLX_TRACE_SAMPLES,                 /* samples < 1 */
  FLX_TRACE_REFLECTIONS,             /* max_reflections < 0 */
  FLX_TRACE_TEXTURE_WIDTH,           /* texture_width < 1 */
  FLX_TRACE_NULL,                    /* a NULL array */
  FLX_TRACE_WRAPS,                   /* an array of n rows would end beyond the address space */
  FLX_TRACE_OVERLAP                  /* the rays' bytes and the radiance's bytes overlap */
};

static inline enum flx_trace_refusal flx_trace_args_check(int have_params, int32_t samples, int32_t max_reflections, int32_t texture_width, uint64_t rays, uint64_t radiance,
                                                          uint32_t n) {
  if (!have_params) return FLX_TRACE_PARAMS_NULL;
  if (samples < 1) return FLX_TRACE_SAMPLES;
  if (max_reflections < 0) return FLX_TRACE_REFLECTIONS;
  if (texture_width < 1) return FLX_TRACE_TEXTURE_WIDTH;
  if (n == 0u) return FLX_TRACE_ARGS_OK;
  if (rays == 0u || radiance == 0u) return FLX_TRACE_NULL;
  const uint64_t bytes = (uint64_t)n * FLX_RAY_ROW_BYTES;
  if (flx_range_wraps(rays, bytes) || flx_range_wraps(radiance, bytes)) return FLX_TRACE_WRAPS;
  if (flx_ranges_overlap(rays, bytes, radiance, bytes)) return FLX_TRACE_OVERLAP;
  return FLX_TRACE_ARGS_OK;
}

/* Rays of a slab of a traced batch: the scratch holds samples slots of 16 bytes a ray, so a slab has at most 2^24 slots (256 MB) and 2^21 rays, whole blocks of 64
 * rays, and at least one block whatever the sample count.  ceiling > 0 (flx_debug_set_trace_slab): at most so many rays, any number from 1 on. */
#define FLX_TRACE_SLAB_SLOTS (1u << 24)
#define FLX_TRACE_SLAB_RAYS (1u << 21)
static inline uint32_t flx_trace_slab_rays(uint32_t samples, uint32_t ceiling) {
  uint32_t rays = (FLX_TRACE_SLAB_SLOTS / (samples ? samples : 1u)) & ~63u;
  if (rays > FLX_TRACE_SLAB_RAYS) rays = FLX_TRACE_SLAB_RAYS;
  if (rays < 64u) rays = 64u;
  if (ceiling != 0u && ceiling < rays) rays = ceiling;
  return rays;
}

#endif
