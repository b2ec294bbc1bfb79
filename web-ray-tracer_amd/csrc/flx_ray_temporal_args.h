/* flx_ray_temporal_args.h — what flx_rays_image_temporal[_device] and flx_rays_history_reset decide about their arguments and about a history's key before they ask
 * the device anything (csrc/flx_rays_planes.hip): plain C++, no HIP, so that a stand-alone program can hold it under the sanitizers
 * (tests/rays_temporal_args_main.cc), in the manner of flx_ray_planes_args.h.  The scene, the params, the size and the arrays are checked by flx_rays_image's rules
 * (flx_ray_planes_args.h). */
#ifndef FLX_RAY_TEMPORAL_ARGS_H
#define FLX_RAY_TEMPORAL_ARGS_H

#include <stdint.h>

#define FLX_RAY_TEMPORAL_HISTORIES 8   /* FLX_RAY_HISTORIES of the header */
#define FLX_RAY_TEMPORAL_RINGS 4u      /* colour, colour integer part, location id, original id: the frames' rings (flx_context.h: d_ring) */
#define FLX_RAY_TEMPORAL_DEEPEST 16    /* slots of the deepest history: flx_frame_params' ceiling */

enum flx_ray_temporal_refusal {
  FLX_RAY_TEMPORAL_ARGS_OK = 0,
  FLX_RAY_TEMPORAL_NULL,               /* temporal is NULL */
  FLX_RAY_TEMPORAL_HISTORY,            /* history is outside 0 .. FLX_RAY_HISTORIES - 1 */
  FLX_RAY_TEMPORAL_USE_FILTER,         /* use_filter is neither 0 nor 1 */
  FLX_RAY_TEMPORAL_HDR,                /* hdr is neither 0 nor 1 */
  FLX_RAY_TEMPORAL_RESET               /* flx_rays_history_reset: history is below -1 or above FLX_RAY_HISTORIES - 1 */
};

/* the depth N of a history: flx_frame_params' rule for temporal_samples */
static inline int flx_ray_temporal_depth(int32_t temporal_samples) { return temporal_samples <= 0 ? 4 : (temporal_samples > FLX_RAY_TEMPORAL_DEEPEST ? FLX_RAY_TEMPORAL_DEEPEST : temporal_samples); }

/* the fields of a flx_ray_temporal (have: the pointer is not NULL), looked at in the order the header lists the refusals */
static inline enum flx_ray_temporal_refusal flx_ray_temporal_check(int have, int32_t history, int32_t use_filter, int32_t hdr) {
  if (!have) return FLX_RAY_TEMPORAL_NULL;
  if (history < 0 || history >= FLX_RAY_TEMPORAL_HISTORIES) return FLX_RAY_TEMPORAL_HISTORY;
  if (use_filter != 0 && use_filter != 1) return FLX_RAY_TEMPORAL_USE_FILTER;
  if (hdr != 0 && hdr != 1) return FLX_RAY_TEMPORAL_HDR;
  return FLX_RAY_TEMPORAL_ARGS_OK;
}

/* flx_rays_history_reset's argument: -1 names all histories */
static inline enum flx_ray_temporal_refusal flx_ray_history_reset_check(int history) {
  return history < -1 || history >= FLX_RAY_TEMPORAL_HISTORIES ? FLX_RAY_TEMPORAL_RESET : FLX_RAY_TEMPORAL_ARGS_OK;
}

/* A history's key and ring position.  n == 0: no history (never used, reset, or an allocation that failed half way). */
struct flx_ray_history_state { uint32_t width, height; int n, head; };

/* the call continues the history: same size and depth */
static inline int flx_ray_history_continues(const struct flx_ray_history_state *h, uint32_t width, uint32_t height, int n) {
  return h->n != 0 && h->n == n && h->width == width && h->height == height;
}
/* the state after an accepted call: a history that does not continue starts afresh at head 0 (its planes zero), then the ring rotates — TempTexture.unshift(
 * TempTexture.pop()): the oldest slot becomes the head */
static inline struct flx_ray_history_state flx_ray_history_advance(struct flx_ray_history_state h, uint32_t width, uint32_t height, int n) {
  if (!flx_ray_history_continues(&h, width, height, n)) { h.width = width; h.height = height; h.n = n; h.head = 0; }
  h.head = (h.head + n - 1) % n;
  return h;
}
/* the ring slot that holds the frame `age` calls old (0: the head), 0 <= age < n */
static inline uint32_t flx_ray_history_slot(const struct flx_ray_history_state *h, int age) { return (uint32_t)((h->head + age) % h->n); }
/* texels of a history: four rings back to back, each n planes of width * height (width * height < 2^32, n <= 16: no overflow of 64 bits).  Ring j's slot s starts
 * at texel (j * n + s) * width * height. */
static inline uint64_t flx_ray_history_texels(uint32_t width, uint32_t height, int n) { return (uint64_t)width * height * (uint64_t)n * FLX_RAY_TEMPORAL_RINGS; }

#endif
