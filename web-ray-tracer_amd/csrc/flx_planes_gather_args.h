/* flx_planes_gather_args.h — what the ray-image calls that take a volume (flx_rays_planes_gather[_device], flx_rays_image[_temporal]_gather[_device],
 * flx_camera_image[_temporal]_gather[_device]; csrc/flx_rays_planes_gather.hip) decide about it without a device, beyond the checks their siblings and the gathered
 * batches already have (flx_ray_planes_args.h, flx_gather_args.h): plain C++, no HIP, so that a stand-alone program can hold it under the sanitizers
 * (tests/planes_gather_args_main.cc), in the manner of flx_gather_args.h; the range arithmetic is flx_range_args.h's. */
#ifndef FLX_PLANES_GATHER_ARGS_H
#define FLX_PLANES_GATHER_ARGS_H

#include <stdint.h>

#include "flx_gather_args.h"          /* flx_gather_volume_check, FLX_GATHER_HAS_MAP, FLX_GATHER_HAS_OFFSETS, FLX_GATHER_MAX_ARRAYS */
#include "flx_ray_planes_args.h"
#include "flx_range_args.h"

#define FLX_PLANES_GATHER_CALL_ARRAYS 3      /* the most arrays of a call beside the volume's: rays, planes8, planes32 */
#define FLX_PLANES_GATHER_SLAB_SLOTS 1u      /* 16-byte slots of scratch a ray beyond its hit rows count for: the planes calls' own, one — the lookup runs inline */

/* the arrays of a call that the volume's must not share a byte with: where each lies */
struct flx_planes_gather_array { uint64_t address, bytes; };

/* flx_rays_planes_gather_device's over n rays (planes8, planes32: 0 where not asked for) -> how many of `out` are filled */
static inline int flx_planes_gather_planes_arrays(uint64_t rays, uint64_t planes8, uint64_t planes32, uint32_t n, struct flx_planes_gather_array out[FLX_PLANES_GATHER_CALL_ARRAYS]) {
  int k = 0;
  if (rays != 0u) { out[k].address = rays; out[k].bytes = (uint64_t)n * FLX_RAY_ROW_BYTES; k++; }
  if (planes8 != 0u) { out[k].address = planes8; out[k].bytes = (uint64_t)n * FLX_RAY_PLANES * FLX_RAY_PLANES_ROW8; k++; }
  if (planes32 != 0u) { out[k].address = planes32; out[k].bytes = (uint64_t)n * FLX_RAY_PLANES * FLX_RAY_PLANES_ROW32; k++; }
  return k;
}

/* an image call's over n = width * height rays: the rays (0: the context makes them, a camera call) and the image */
static inline int flx_planes_gather_image_arrays(uint64_t rays, uint64_t image, uint32_t n, struct flx_planes_gather_array out[FLX_PLANES_GATHER_CALL_ARRAYS]) {
  int k = 0;
  if (rays != 0u) { out[k].address = rays; out[k].bytes = (uint64_t)n * FLX_RAY_ROW_BYTES; k++; }
  if (image != 0u) { out[k].address = image; out[k].bytes = (uint64_t)n * FLX_RAY_PLANES_ROW32; k++; }
  return k;
}

/* the k <= 3 arrays of the volume (none NULL, none wrapping: their own checks came first) against the kc arrays of the call (none wrapping: the sibling's check came
 * first): FLX_GATHER_OVERLAP where two share a byte */
static inline enum flx_gather_refusal flx_planes_gather_overlap_check(const uint64_t *address, const uint64_t *bytes, int k, const struct flx_planes_gather_array *call, int kc) {
  for (int i = 0; i < k; i++)
    for (int j = 0; j < kc; j++)
      if (flx_ranges_overlap(address[i], bytes[i], call[j].address, call[j].bytes)) return FLX_GATHER_OVERLAP;
  return FLX_GATHER_ARGS_OK;
}

/* flx_debug_last_planes_gather's word 4 */
static inline uint32_t flx_planes_gather_flags(int has_map, int has_offsets) { return (has_map ? FLX_GATHER_HAS_MAP : 0u) | (has_offsets ? FLX_GATHER_HAS_OFFSETS : 0u); }

/* the rays of a full slab: the planes calls' rule, one slot a ray — 2^21 rays, so that a 1080p image is one slab */
static inline uint32_t flx_planes_gather_slab_rays(uint32_t ceiling) { return flx_trace_slab_rays(FLX_PLANES_GATHER_SLAB_SLOTS, ceiling); }

#endif
