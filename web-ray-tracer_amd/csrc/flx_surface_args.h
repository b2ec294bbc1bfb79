/* flx_surface_args.h — what flx_rays_surface_device and flx_frame_surface_device decide about their arguments before they ask the device anything (csrc/flx_surface.hip):
 * plain C++, no HIP, so that a stand-alone program can hold it under the sanitizers (tests/surface_args_main.cc), in the manner of flx_query_args.h.  The range arithmetic is flx_range_args.h's. */
#ifndef FLX_SURFACE_ARGS_H
#define FLX_SURFACE_ARGS_H

#include <stdint.h>

#include "flx_range_args.h"

#define FLX_SURFACE_ROW_BYTES 16u    /* a row of a plane: 4 words (a ray row: FLX_RAY_ROW_BYTES) */
#define FLX_SURFACE_FIELDS_ALL 255u  /* FLX_SURFACE_HIT .. FLX_SURFACE_TPO */

enum flx_surface_refusal {
  FLX_SURFACE_ARGS_OK = 0,
  FLX_SURFACE_FIELDS_NONE,           /* fields is 0 */
  FLX_SURFACE_FIELDS_UNKNOWN,        /* a bit above FLX_SURFACE_TPO */
  FLX_SURFACE_TEXTURE_WIDTH,         /* texture_width < 1 */
  FLX_SURFACE_PARAMS_NULL,           /* a frame: no params */
  FLX_SURFACE_SIZE,                  /* a frame: width or height is 0 */
  FLX_SURFACE_TILE,                  /* a frame: the tile policy does not name the whole frame */
  FLX_SURFACE_PIXELS,                /* a frame: more than 2^32 - 1 pixels */
  FLX_SURFACE_NULL,                  /* a NULL array */
  FLX_SURFACE_WRAPS,                 /* the planes' bytes, or an array's end, leave 64 bits */
  FLX_SURFACE_OVERLAP                /* the rays' bytes and the planes' bytes overlap */
};

/* planes a call writes: the bits of fields (a value that passed flx_surface_fields_check: at most 8) */
static inline uint32_t flx_surface_planes(uint32_t fields) {
  uint32_t planes = 0;
  for (; fields != 0u; fields &= fields - 1u) planes++;
  return planes;
}

/* index of plane `bit` (one bit of fields) among the planes of `fields`: the planes follow each other in bit order */
static inline uint32_t flx_surface_plane_index(uint32_t fields, uint32_t bit) { return flx_surface_planes(fields & (bit - 1u)); }

/* what both kinds of call say first, for any n */
static inline enum flx_surface_refusal flx_surface_fields_check(uint32_t fields, int32_t texture_width) {
  if (fields == 0u) return FLX_SURFACE_FIELDS_NONE;
  if ((fields & ~FLX_SURFACE_FIELDS_ALL) != 0u) return FLX_SURFACE_FIELDS_UNKNOWN;
  if (texture_width < 1) return FLX_SURFACE_TEXTURE_WIDTH;
  return FLX_SURFACE_ARGS_OK;
}

/* a frame's params: the size and the tile policy, which must name the whole frame (0/0/0 or x/0/1) */
static inline enum flx_surface_refusal flx_surface_frame_check(int have_params, uint32_t width, uint32_t height, uint32_t tile_rows, uint32_t tile_index,
                                                               uint32_t tile_count) {
  if (!have_params) return FLX_SURFACE_PARAMS_NULL;
  if (width == 0u || height == 0u) return FLX_SURFACE_SIZE;
  const int whole = (tile_rows == 0u && tile_index == 0u && tile_count == 0u) || (tile_index == 0u && tile_count == 1u);
  if (!whole) return FLX_SURFACE_TILE;
  if ((uint64_t)width * height > 0xffffffffull) return FLX_SURFACE_PIXELS;
  return FLX_SURFACE_ARGS_OK;
}

/* The arrays of a call over n > 0 items: rays (n rows of 32 bytes; a frame has none: have_rays 0 and `rays` is not looked at) and out, popcount(fields) planes of n
 * rows of 16 bytes.  *out_bytes <- the planes' bytes where they fit 64 bits. */
static inline enum flx_surface_refusal flx_surface_arrays_check(int have_rays, uint64_t rays, uint64_t out, uint32_t n, uint32_t fields, uint64_t *out_bytes) {
  if ((have_rays && rays == 0u) || out == 0u) return FLX_SURFACE_NULL;
  const uint64_t plane = (uint64_t)n * FLX_SURFACE_ROW_BYTES, planes = flx_surface_planes(fields);      /* n * 16 * 8 < 2^39: the product itself cannot leave 64 bits, address + bytes can */
  const uint64_t bytes = plane * planes, ray_bytes = (uint64_t)n * FLX_RAY_ROW_BYTES;
  if (out_bytes) *out_bytes = bytes;
  if (flx_range_wraps(out, bytes) || (have_rays && flx_range_wraps(rays, ray_bytes))) return FLX_SURFACE_WRAPS;
  if (have_rays && flx_ranges_overlap(rays, ray_bytes, out, bytes)) return FLX_SURFACE_OVERLAP;
  return FLX_SURFACE_ARGS_OK;
}

#endif
