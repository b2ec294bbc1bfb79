/* flx_query_args.h — what flx_rays_cast_device decides about its arguments before it asks the device anything: plain C++, no HIP, so that a stand-alone program
 * can hold it under the sanitizers (tests/ray_query_args_main.cc). */
#ifndef FLX_QUERY_ARGS_H
#define FLX_QUERY_ARGS_H

#include <stdint.h>

#define FLX_QUERY_ROW_BYTES 32u      /* a ray row and a hit row alike: 8 words */

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
  const uint64_t bytes = (uint64_t)n * FLX_QUERY_ROW_BYTES;
  if (rays > UINT64_MAX - bytes || hits > UINT64_MAX - bytes) return FLX_QUERY_WRAPS;
  if (rays < hits + bytes && hits < rays + bytes) return FLX_QUERY_OVERLAP;
  return FLX_QUERY_ARGS_OK;
}

#endif
