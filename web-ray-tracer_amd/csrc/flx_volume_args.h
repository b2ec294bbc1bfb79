/* flx_volume_args.h — what the probe-volume calls (csrc/flx_volume.hip: flx_volume_positions, flx_volume_bake, flx_volume_irradiance, flx_rays_irradiance,
 * flx_frame_irradiance and their _device forms) decide about their arguments before they ask the device anything: plain C++, no HIP, so that a stand-alone program
 * can hold it under the sanitizers (tests/volume_args_main.cc), in the manner of flx_probe_args.h; the range arithmetic is flx_range_args.h's.  The scene, the
 * trace and probe params and the surface rows are checked by the calls they belong to. */
#ifndef FLX_VOLUME_ARGS_H
#define FLX_VOLUME_ARGS_H

#include <stdint.h>

#include "flexlight_hip_debug.h"
#include "flx_probe_args.h"      /* flx_probe_finite; FLX_PROBE_POSITION_BYTES, FLX_PROBE_SH_BYTES: a volume's position rows and SH rows are the probes' */
#include "flx_range_args.h"

#define FLX_VOLUME_ROW_BYTES 16u         /* a surface row (position, normal) and an irradiance row */
#define FLX_VOLUME_MAX_PROBES 0x7fffffffu      /* nx ny nz stays below 2^31 */
#define FLX_VOLUME_THREADS 256u
#define FLX_VOLUME_MAX_ARRAYS 4

enum flx_volume_refusal {
  FLX_VOLUME_ARGS_OK = 0,
  FLX_VOLUME_GRID_NULL,              /* no flx_volume_grid */
  FLX_VOLUME_COUNT_ZERO,             /* a count of 0 */
  FLX_VOLUME_PROBES,                 /* nx ny nz is 2^31 or more */
  FLX_VOLUME_NOT_FINITE,             /* a NaN or an infinity in origin or spacing */
  FLX_VOLUME_SPACING,                /* a spacing <= 0 */
  FLX_VOLUME_BIAS,                   /* normal_bias negative or not finite */
  FLX_VOLUME_FLOOR,                  /* floor outside [0, 1] or not finite */
  FLX_VOLUME_FLAGS,                  /* a bit beyond FLX_VOLUME_VISIBILITY */
  FLX_VOLUME_RESERVED,               /* the reserved word is not 0 */
  FLX_VOLUME_NULL,                   /* a NULL array */
  FLX_VOLUME_WRAPS,                  /* an array's end leaves 64 bits */
  FLX_VOLUME_OVERLAP                 /* two arrays of a call share a byte */
};

/* nx ny nz without overflow: every count is below 2^32, so nx ny stays in 64 bits; only where that is below 2^31 is it multiplied again, and stays below 2^63.
 * -> 0 where the product is 2^31 or more (no count is 0: checked first) */
static inline int flx_volume_probe_count(const uint32_t count[3], uint32_t *probes) {
  const uint64_t xy = (uint64_t)count[0] * count[1];
  if (xy > FLX_VOLUME_MAX_PROBES) return 0;
  const uint64_t xyz = xy * count[2];
  if (xyz > FLX_VOLUME_MAX_PROBES) return 0;
  if (probes) *probes = (uint32_t)xyz;
  return 1;
}

/* a flx_volume_grid, in the order the header lists the refusals; *probes <- nx ny nz of an accepted grid */
static inline enum flx_volume_refusal flx_volume_grid_check(const flx_volume_grid *g, uint32_t *probes) {
  if (!g) return FLX_VOLUME_GRID_NULL;
  if (g->count[0] == 0u || g->count[1] == 0u || g->count[2] == 0u) return FLX_VOLUME_COUNT_ZERO;
  if (!flx_volume_probe_count(g->count, probes)) return FLX_VOLUME_PROBES;
  for (int a = 0; a < 3; a++)
    if (!(flx_probe_finite(g->origin[a]) & flx_probe_finite(g->spacing[a]))) return FLX_VOLUME_NOT_FINITE;
  for (int a = 0; a < 3; a++)
    if (!(g->spacing[a] > 0.0f)) return FLX_VOLUME_SPACING;
  if (!flx_probe_finite(g->normal_bias) || g->normal_bias < 0.0f) return FLX_VOLUME_BIAS;
  if (!flx_probe_finite(g->floor) || g->floor < 0.0f || g->floor > 1.0f) return FLX_VOLUME_FLOOR;
  if ((g->flags & ~FLX_VOLUME_VISIBILITY) != 0u) return FLX_VOLUME_FLAGS;
  if (g->reserved != 0u) return FLX_VOLUME_RESERVED;
  return FLX_VOLUME_ARGS_OK;
}

/* the bytes of the grid's position rows, of its SH rows, and of a plane of n surface or irradiance rows (a uint32_t count times a row's bytes stays in 64 bits) */
static inline uint64_t flx_volume_position_bytes(uint32_t probes) { return (uint64_t)probes * FLX_PROBE_POSITION_BYTES; }
static inline uint64_t flx_volume_sh_bytes(uint32_t probes) { return (uint64_t)probes * FLX_PROBE_SH_BYTES; }
static inline uint64_t flx_volume_plane_bytes(uint32_t n) { return (uint64_t)n * FLX_VOLUME_ROW_BYTES; }

/* the k <= 4 arrays of a call (addresses as integers, bytes > 0 each): none NULL, none leaving 64 bits, no two sharing a byte — in that order */
static inline enum flx_volume_refusal flx_volume_arrays_check(const uint64_t *address, const uint64_t *bytes, int k) {
  for (int i = 0; i < k; i++)
    if (address[i] == 0u) return FLX_VOLUME_NULL;
  for (int i = 0; i < k; i++)
    if (flx_range_wraps(address[i], bytes[i])) return FLX_VOLUME_WRAPS;
  for (int i = 0; i < k; i++)
    for (int j = i + 1; j < k; j++)
      if (flx_ranges_overlap(address[i], bytes[i], address[j], bytes[j])) return FLX_VOLUME_OVERLAP;
  return FLX_VOLUME_ARGS_OK;
}

/* workgroups of k_volume_positions / k_volume_irradiance for n lanes' worth of work: 256 a workgroup (n / 256 + 1 cannot wrap) */
static inline uint32_t flx_volume_groups(uint32_t n) { return n / FLX_VOLUME_THREADS + (n % FLX_VOLUME_THREADS != 0u ? 1u : 0u); }

#endif
