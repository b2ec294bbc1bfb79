/* flx_ray_planes_args.h — what flx_rays_planes_device and flx_rays_image_device decide about their arguments before they ask the device anything
 * (csrc/flx_rays_planes.hip): plain C++, no HIP, so that a stand-alone program can hold it under the sanitizers (tests/ray_planes_args_main.cc), in the manner of
 * flx_surface_args.h; the range arithmetic is flx_range_args.h's.  The params are flx_rays_trace's and are checked by its rule (flx_query_args.h: flx_trace_args_check with n = 0). */
#ifndef FLX_RAY_PLANES_ARGS_H
#define FLX_RAY_PLANES_ARGS_H

#include <stdint.h>

#include "flx_range_args.h"

#define FLX_RAY_PLANES 5u             /* renderColor, renderColorIp, renderOriginalColor, renderId, renderOriginalId: flx_render_planes_device's order */
#define FLX_RAY_PLANES_ROW8 4u        /* a row of a byte plane: one RGBA8 texel */
#define FLX_RAY_PLANES_ROW32 16u      /* a row of a float plane, and a pixel of a ray image: a float4 */

enum flx_ray_planes_refusal {
  FLX_RAY_PLANES_ARGS_OK = 0,
  FLX_RAY_PLANES_NONE,               /* planes: both plane pointers are NULL */
  FLX_RAY_PLANES_SIZE,               /* an image: width or height is 0 */
  FLX_RAY_PLANES_PIXELS,             /* an image: width * height is 2^32 or more */
  FLX_RAY_PLANES_NULL,               /* the rays, or an image's output, are NULL */
  FLX_RAY_PLANES_WRAPS,              /* an array's end leaves 64 bits */
  FLX_RAY_PLANES_OVERLAP_RAYS,       /* an output's bytes overlap the rays' */
  FLX_RAY_PLANES_OVERLAP_OUT         /* planes: the two outputs' bytes overlap */
};

/* flx_ranges_overlap under the name this header gave it first */
static inline int flx_ray_planes_overlap(uint64_t a, uint64_t a_bytes, uint64_t b, uint64_t b_bytes) { return flx_ranges_overlap(a, a_bytes, b, b_bytes); }

/* The arrays of flx_rays_planes_device over n > 0 rays: rays (n rows of 32 bytes), planes8 (5 n rows of 4 bytes, or 0: not asked for), planes32 (5 n rows of 16
 * bytes, or 0).  5 * 16 * n < 2^39: a product cannot leave 64 bits, address + bytes can. */
static inline enum flx_ray_planes_refusal flx_ray_planes_arrays_check(uint64_t rays, uint64_t planes8, uint64_t planes32, uint32_t n) {
  if (planes8 == 0u && planes32 == 0u) return FLX_RAY_PLANES_NONE;
  if (rays == 0u) return FLX_RAY_PLANES_NULL;
  const uint64_t ray_bytes = (uint64_t)n * FLX_RAY_ROW_BYTES;
  const uint64_t bytes8 = (uint64_t)n * FLX_RAY_PLANES * FLX_RAY_PLANES_ROW8, bytes32 = (uint64_t)n * FLX_RAY_PLANES * FLX_RAY_PLANES_ROW32;
  if (flx_range_wraps(rays, ray_bytes) || (planes8 != 0u && flx_range_wraps(planes8, bytes8)) || (planes32 != 0u && flx_range_wraps(planes32, bytes32))) return FLX_RAY_PLANES_WRAPS;
  if (planes8 != 0u && flx_ranges_overlap(rays, ray_bytes, planes8, bytes8)) return FLX_RAY_PLANES_OVERLAP_RAYS;
  if (planes32 != 0u && flx_ranges_overlap(rays, ray_bytes, planes32, bytes32)) return FLX_RAY_PLANES_OVERLAP_RAYS;
  if (planes8 != 0u && planes32 != 0u && flx_ranges_overlap(planes8, bytes8, planes32, bytes32)) return FLX_RAY_PLANES_OVERLAP_OUT;
  return FLX_RAY_PLANES_ARGS_OK;
}

/* a ray image's size, looked at for any width and height: *n <- width * height where that is a ray count */
static inline enum flx_ray_planes_refusal flx_ray_image_size_check(uint32_t width, uint32_t height, uint32_t *n) {
  if (width == 0u || height == 0u) return FLX_RAY_PLANES_SIZE;
  const uint64_t pixels = (uint64_t)width * height;
  if (pixels > 0xffffffffull) return FLX_RAY_PLANES_PIXELS;
  if (n) *n = (uint32_t)pixels;
  return FLX_RAY_PLANES_ARGS_OK;
}

/* The arrays of flx_rays_image_device: rays (n rows of 32 bytes) and out (n float4), n = width * height > 0 */
static inline enum flx_ray_planes_refusal flx_ray_image_arrays_check(uint64_t rays, uint64_t out, uint32_t n) {
  if (rays == 0u || out == 0u) return FLX_RAY_PLANES_NULL;
  const uint64_t ray_bytes = (uint64_t)n * FLX_RAY_ROW_BYTES, out_bytes = (uint64_t)n * FLX_RAY_PLANES_ROW32;
  if (flx_range_wraps(rays, ray_bytes) || flx_range_wraps(out, out_bytes)) return FLX_RAY_PLANES_WRAPS;
  if (flx_ranges_overlap(rays, ray_bytes, out, out_bytes)) return FLX_RAY_PLANES_OVERLAP_RAYS;
  return FLX_RAY_PLANES_ARGS_OK;
}

#endif
