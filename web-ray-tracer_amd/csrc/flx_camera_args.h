/* flx_camera_args.h — what flx_camera_rays[_device] and flx_camera_image[_temporal][_device] decide about their arguments before they ask the device anything
 * (csrc/flx_camera.hip): plain C++, no HIP, so that a stand-alone program can hold it under the sanitizers (tests/camera_args_main.cc), in the manner of
 * flx_ray_planes_args.h; the range arithmetic is flx_range_args.h's.  The image calls' params, temporal and output are checked by flx_rays_image's rules. */
#ifndef FLX_CAMERA_ARGS_H
#define FLX_CAMERA_ARGS_H

#include <stdint.h>

#include "flexlight_hip_debug.h"
#include "flx_range_args.h"

enum flx_camera_refusal {
  FLX_CAMERA_ARGS_OK = 0,
  FLX_CAMERA_NONE,                   /* cameras is NULL or n_cameras is 0 */
  FLX_CAMERA_SIZE,                   /* width or height is 0 */
  FLX_CAMERA_RAYS,                   /* n_cameras * width * height is 2^32 or more */
  FLX_CAMERA_REGION_EMPTY,           /* a region of no pixels */
  FLX_CAMERA_REGION_OUTSIDE,         /* a region that leaves the image */
  FLX_CAMERA_PROJECTION,             /* none of the five */
  FLX_CAMERA_FACE,                   /* outside 0 .. 5 */
  FLX_CAMERA_NOT_FINITE,             /* a NaN or an infinity in position, basis, extent or jitter */
  FLX_CAMERA_JITTER,                 /* outside [-0.5, 0.5] */
  FLX_CAMERA_EXTENT,                 /* <= 0 where the projection reads it */
  FLX_CAMERA_OUT_NULL,               /* no output */
  FLX_CAMERA_OUT_WRAPS               /* the output's end leaves 64 bits */
};

/* what a call writes: the pixels [x0, x0 + w) x [y0, y0 + h) of every camera's image, w * h rows a camera, `rays` rows in all */
struct flx_camera_span { uint32_t x0, y0, w, h, rays; };

/* The batch: cameras given (have: the pointer is not NULL), the image's size, the region (NULL: the whole image).  *span is written where the batch is accepted
 * and left alone otherwise. */
static inline enum flx_camera_refusal flx_camera_batch_check(int have, uint32_t n_cameras, uint32_t width, uint32_t height, const uint32_t *region, struct flx_camera_span *span) {
  if (!have || n_cameras == 0u) return FLX_CAMERA_NONE;
  if (width == 0u || height == 0u) return FLX_CAMERA_SIZE;
  const uint64_t pixels = (uint64_t)width * height;      /* < 2^64 */
  if (pixels > 0xffffffffull || pixels * n_cameras > 0xffffffffull) return FLX_CAMERA_RAYS;      /* (pixels < 2^32 and n_cameras < 2^32: the product stays in 64 bits) */
  struct flx_camera_span s = { 0u, 0u, width, height, 0u };
  if (region) {
    if (region[2] == 0u || region[3] == 0u) return FLX_CAMERA_REGION_EMPTY;
    /* x0 + w <= width without a sum that could wrap */
    if (region[0] >= width || region[2] > width - region[0] || region[1] >= height || region[3] > height - region[1]) return FLX_CAMERA_REGION_OUTSIDE;
    s.x0 = region[0]; s.y0 = region[1]; s.w = region[2]; s.h = region[3];
  }
  s.rays = (uint32_t)((uint64_t)s.w * s.h * n_cameras);      /* <= pixels * n_cameras */
  if (span) *span = s;
  return FLX_CAMERA_ARGS_OK;
}

static inline int flx_camera_finite(float x) { return x - x == 0.0f; }      /* (inf - inf and NaN - NaN are NaN) */

/* one camera, in the order the header lists the refusals */
static inline enum flx_camera_refusal flx_camera_check(const flx_camera *c) {
  if (c->projection < FLX_CAMERA_PINHOLE || c->projection > FLX_CAMERA_CUBE_FACE) return FLX_CAMERA_PROJECTION;
  if (c->face < 0 || c->face > 5) return FLX_CAMERA_FACE;
  int finite = 1;
  for (int k = 0; k < 3; k++) finite &= flx_camera_finite(c->position[k]);
  for (int k = 0; k < 9; k++) finite &= flx_camera_finite(c->basis[k]);
  for (int k = 0; k < 2; k++) finite &= flx_camera_finite(c->extent[k]) & flx_camera_finite(c->jitter[k]);
  if (!finite) return FLX_CAMERA_NOT_FINITE;
  for (int k = 0; k < 2; k++) if (c->jitter[k] < -0.5f || c->jitter[k] > 0.5f) return FLX_CAMERA_JITTER;
  const int reads0 = c->projection == FLX_CAMERA_PANORAMA || c->projection == FLX_CAMERA_FISHEYE || c->projection == FLX_CAMERA_ORTHOGRAPHIC;
  const int reads1 = c->projection == FLX_CAMERA_PANORAMA || c->projection == FLX_CAMERA_ORTHOGRAPHIC;
  if ((reads0 && c->extent[0] <= 0.0f) || (reads1 && c->extent[1] <= 0.0f)) return FLX_CAMERA_EXTENT;
  return FLX_CAMERA_ARGS_OK;
}

/* every camera of an accepted batch: the first refusal, *which <- its camera */
static inline enum flx_camera_refusal flx_cameras_check(const flx_camera *cameras, uint32_t n_cameras, uint32_t *which) {
  for (uint32_t c = 0; c < n_cameras; c++) {
    const enum flx_camera_refusal why = flx_camera_check(cameras + c);
    if (why != FLX_CAMERA_ARGS_OK) { if (which) *which = c; return why; }
  }
  return FLX_CAMERA_ARGS_OK;
}

/* the output of `rays` > 0 rows of 32 bytes (rays * 32 < 2^37: the product cannot leave 64 bits, address + bytes can) */
static inline enum flx_camera_refusal flx_camera_out_check(uint64_t out, uint32_t rays) {
  if (out == 0u) return FLX_CAMERA_OUT_NULL;
  if (flx_range_wraps(out, (uint64_t)rays * FLX_RAY_ROW_BYTES)) return FLX_CAMERA_OUT_WRAPS;
  return FLX_CAMERA_ARGS_OK;
}

#endif
