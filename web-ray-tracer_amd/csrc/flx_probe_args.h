/* flx_probe_args.h — what flx_probe_rays[_device], flx_probe_reduce[_device] and flx_probes_sh[_device] decide about their arguments before they ask the device
 * anything (csrc/flx_probes.hip): plain C++, no HIP, so that a stand-alone program can hold it under the sanitizers (tests/probe_args_main.cc), in the manner of
 * flx_camera_args.h; the range arithmetic is flx_range_args.h's.  The trace params and the scene of flx_probes_sh are checked by flx_rays_trace's rules. */
#ifndef FLX_PROBE_ARGS_H
#define FLX_PROBE_ARGS_H

#include <stdint.h>

#include "flexlight_hip_debug.h"
#include "flx_query_args.h"      /* FLX_TRACE_SLAB_RAYS: the most rays of a trace slab, hence of a chunk of probes */
#include "flx_range_args.h"
#include "flx_ray_order_args.h"  /* flx_order_bits_known */

#define FLX_PROBE_FACE_MAX 256u        /* include/flx_probe.h: FLX_PROBE_MAX_FACE */
#define FLX_PROBE_POSITION_BYTES 16u   /* a position row: x, y, z and a word that is ignored */
#define FLX_PROBE_SH_BYTES 144u        /* an SH row: nine float4 */

enum flx_probe_refusal {
  FLX_PROBE_ARGS_OK = 0,
  FLX_PROBE_PARAMS_NULL,             /* no flx_probe_params */
  FLX_PROBE_FACE_SIZE,               /* 0 or above 256 */
  FLX_PROBE_ORDER,                   /* a bit beyond FLX_TRACE_ORDER_HITS */
  FLX_PROBE_NOT_FINITE,              /* a NaN or an infinity in sky or reserved */
  FLX_PROBE_RAYS,                    /* n_probes * 6 w w is 2^32 or more */
  FLX_PROBE_NULL,                    /* a NULL array */
  FLX_PROBE_WRAPS,                   /* an array's end leaves 64 bits */
  FLX_PROBE_OVERLAP                  /* the two arrays share a byte */
};

static inline int flx_probe_finite(float x) { return x - x == 0.0f; }      /* (inf - inf and NaN - NaN are NaN) */

static inline enum flx_probe_refusal flx_probe_face_check(uint32_t face_size) {
  return face_size == 0u || face_size > FLX_PROBE_FACE_MAX ? FLX_PROBE_FACE_SIZE : FLX_PROBE_ARGS_OK;
}

/* rays of a probe of an accepted face size: 6 .. 393 216 */
static inline uint32_t flx_probe_rays_of(uint32_t face_size) { return 6u * face_size * face_size; }

/* a flx_probe_params, in the order the header lists the refusals (have: the pointer is not NULL; the fields are looked at only then) */
static inline enum flx_probe_refusal flx_probe_params_check(int have, uint32_t face_size, uint32_t order, const float *sky, float reserved) {
  if (!have) return FLX_PROBE_PARAMS_NULL;
  if (flx_probe_face_check(face_size) != FLX_PROBE_ARGS_OK) return FLX_PROBE_FACE_SIZE;
  if (!flx_order_bits_known(order)) return FLX_PROBE_ORDER;
  if (!(flx_probe_finite(sky[0]) & flx_probe_finite(sky[1]) & flx_probe_finite(sky[2]) & flx_probe_finite(reserved))) return FLX_PROBE_NOT_FINITE;
  return FLX_PROBE_ARGS_OK;
}

/* the ray and reduce calls write or read n_probes * R rows in one piece: *rays <- that count where it is below 2^32 (R < 2^19 and n_probes < 2^32: the product
 * stays in 64 bits) */
static inline enum flx_probe_refusal flx_probe_count_check(uint32_t n_probes, uint32_t face_size, uint32_t *rays) {
  const uint64_t all = (uint64_t)n_probes * flx_probe_rays_of(face_size);
  if (all > 0xffffffffull) return FLX_PROBE_RAYS;
  if (rays) *rays = (uint32_t)all;
  return FLX_PROBE_ARGS_OK;
}

/* two arrays of a call (addresses as integers, bytes > 0 each: no product of a uint32_t count and a row's bytes leaves 64 bits, address + bytes can) */
static inline enum flx_probe_refusal flx_probe_arrays_check(uint64_t a, uint64_t a_bytes, uint64_t b, uint64_t b_bytes) {
  if (a == 0u || b == 0u) return FLX_PROBE_NULL;
  if (flx_range_wraps(a, a_bytes) || flx_range_wraps(b, b_bytes)) return FLX_PROBE_WRAPS;
  if (flx_ranges_overlap(a, a_bytes, b, b_bytes)) return FLX_PROBE_OVERLAP;
  return FLX_PROBE_ARGS_OK;
}

/* Probes of a chunk of flx_probes_sh_device: as many as a trace slab's 2^21 rays hold, at least one (w = 256 gives 5: 5 x 393 216 <= 2^21); ceiling > 0
 * (flx_debug_set_probe_chunk): at most so many.  A chunk's rays, chunk * R, are at most 2^21: the context's two buffers end at 2^21 x 32 bytes each. */
static inline uint32_t flx_probe_chunk(uint32_t face_size, uint32_t ceiling) {
  uint32_t probes = FLX_TRACE_SLAB_RAYS / flx_probe_rays_of(face_size);
  if (probes < 1u) probes = 1u;
  if (ceiling != 0u && ceiling < probes) probes = ceiling;
  return probes;
}

static inline uint32_t flx_probe_chunks(uint32_t n_probes, uint32_t chunk) { return n_probes / chunk + (n_probes % chunk != 0u ? 1u : 0u); }

/* workgroups of k_probe_sh for n probes: four waves, a probe each (n / 4 + 1 cannot wrap) */
static inline uint32_t flx_probe_reduce_groups(uint32_t n_probes) { return n_probes / 4u + (n_probes % 4u != 0u ? 1u : 0u); }

#endif
