/* flx_volume_map_args.h — what the directional-visibility calls (csrc/flx_volume_map.hip: flx_probe_map, flx_probes_sh_map, flx_volume_bake_map,
 * flx_volume_irradiance_map, flx_rays_irradiance_map, flx_frame_irradiance_map and their _device forms) decide about the map and the maps array before they ask the
 * device anything: plain C++, no HIP, so that a stand-alone program can hold it under the sanitizers (tests/volume_map_args_main.cc), in the manner of
 * flx_volume_args.h.  What the siblings decide — the grid, the probe params, their own arrays — is theirs and is asked first. */
#ifndef FLX_VOLUME_MAP_ARGS_H
#define FLX_VOLUME_MAP_ARGS_H

#include <stdint.h>

#include "flexlight_hip_debug.h"
#include "flx_range_args.h"

#define FLX_VOLUME_MAP_SIZE_MAX 16u               /* include/flx_volume_map.h: FLX_VOLUME_MAP_MAX_SIZE */
#define FLX_VOLUME_MAP_SHARPNESS_MAX 8u           /* FLX_VOLUME_MAP_MAX_SHARPNESS */
#define FLX_VOLUME_MAP_ROW_BYTES 16u              /* a bin's row: one float4 */
#define FLX_VOLUME_MAP_MAX_ROWS 0x7fffffffu       /* n_probes m m stays below 2^31: a maps array ends below 2^35 bytes */
#define FLX_VOLUME_MAP_MAX_ARRAYS 5               /* the lookup's four arrays and the maps */
#define FLX_VOLUME_MAP_LAUNCH 32768u              /* probes a launch of k_probe_map names with its grid's y */
#define FLX_VOLUME_MAP_GROUP_BINS 16u             /* bins a workgroup of k_probe_map reduces: four waves, four bins each */

enum flx_volume_map_refusal {
  FLX_VOLUME_MAP_ARGS_OK = 0,
  FLX_VOLUME_MAP_NULL,               /* no flx_volume_map */
  FLX_VOLUME_MAP_SIZE,               /* 0 or above 16 */
  FLX_VOLUME_MAP_SHARPNESS,          /* above 8 */
  FLX_VOLUME_MAP_RESERVED,           /* a reserved word is not 0 */
  FLX_VOLUME_MAP_ROWS,               /* n_probes m m is 2^31 or more */
  FLX_VOLUME_MAPS_NULL,              /* a NULL maps array */
  FLX_VOLUME_MAPS_WRAPS,             /* the maps array's end leaves 64 bits */
  FLX_VOLUME_MAPS_OVERLAP            /* the maps array shares a byte with another array of the call */
};

/* a flx_volume_map, in the order the header lists the refusals */
static inline enum flx_volume_map_refusal flx_volume_map_check(const flx_volume_map *map) {
  if (!map) return FLX_VOLUME_MAP_NULL;
  if (map->size == 0u || map->size > FLX_VOLUME_MAP_SIZE_MAX) return FLX_VOLUME_MAP_SIZE;
  if (map->sharpness > FLX_VOLUME_MAP_SHARPNESS_MAX) return FLX_VOLUME_MAP_SHARPNESS;
  if (map->reserved[0] != 0u || map->reserved[1] != 0u) return FLX_VOLUME_MAP_RESERVED;
  return FLX_VOLUME_MAP_ARGS_OK;
}

/* the rows of n_probes maps of an accepted size (m m <= 256 and n_probes < 2^32: the product stays in 64 bits): *rows <- the count where it is below 2^31 */
static inline enum flx_volume_map_refusal flx_volume_map_rows_check(uint32_t n_probes, uint32_t size, uint32_t *rows) {
  const uint64_t all = (uint64_t)n_probes * (size * size);
  if (all > FLX_VOLUME_MAP_MAX_ROWS) return FLX_VOLUME_MAP_ROWS;
  if (rows) *rows = (uint32_t)all;
  return FLX_VOLUME_MAP_ARGS_OK;
}

static inline uint64_t flx_volume_map_bytes(uint32_t rows) { return (uint64_t)rows * FLX_VOLUME_MAP_ROW_BYTES; }

/* the maps array against the k <= 4 other arrays of its call, which their own check has accepted (addresses as integers, bytes > 0 each): there, inside 64 bits,
 * apart from every other — in that order */
static inline enum flx_volume_map_refusal flx_volume_maps_check(uint64_t maps, uint64_t maps_bytes, const uint64_t *address, const uint64_t *bytes, int k) {
  if (maps == 0u) return FLX_VOLUME_MAPS_NULL;
  if (flx_range_wraps(maps, maps_bytes)) return FLX_VOLUME_MAPS_WRAPS;
  for (int i = 0; i < k; i++)
    if (flx_ranges_overlap(maps, maps_bytes, address[i], bytes[i])) return FLX_VOLUME_MAPS_OVERLAP;
  return FLX_VOLUME_MAP_ARGS_OK;
}

/* k_probe_map's grid: x the groups of 16 bins of a map (1 .. 16), y the probes of a launch (at most 32 768); launches for n probes */
static inline uint32_t flx_volume_map_bin_groups(uint32_t size) { return (size * size + FLX_VOLUME_MAP_GROUP_BINS - 1u) / FLX_VOLUME_MAP_GROUP_BINS; }
static inline uint32_t flx_volume_map_launches(uint32_t n_probes) { return n_probes / FLX_VOLUME_MAP_LAUNCH + (n_probes % FLX_VOLUME_MAP_LAUNCH != 0u ? 1u : 0u); }

#endif
