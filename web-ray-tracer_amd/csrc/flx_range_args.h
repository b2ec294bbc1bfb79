/* flx_range_args.h — the byte-range arithmetic of the ray-batch calls' args headers (flx_query_args.h, flx_surface_args.h, flx_ray_planes_args.h) and the row every
 * one of them reads its rays from: plain C++, no HIP, as they are. */
#ifndef FLX_RANGE_ARGS_H
#define FLX_RANGE_ARGS_H

#include <stdint.h>

#define FLX_RAY_ROW_BYTES 32u        /* a ray row (and a hit row, a radiance row): 8 words */

/* address + bytes leaves 64 bits (a product of a uint32_t n and a row's bytes cannot: only the sum can) */
static inline int flx_range_wraps(uint64_t a, uint64_t bytes) { return a > UINT64_MAX - bytes; }

/* [a, a + a_bytes) and [b, b + b_bytes) share a byte (neither end wraps: checked first) */
static inline int flx_ranges_overlap(uint64_t a, uint64_t a_bytes, uint64_t b, uint64_t b_bytes) { return a < b + b_bytes && b < a + a_bytes; }

#endif
