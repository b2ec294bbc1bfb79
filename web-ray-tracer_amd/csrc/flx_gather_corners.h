/* flx_gather_corners.h — the volume lookup of one surface point as a device function: the corner loop flx_volume.hip's volume_irradiance and flx_rays_gather.hip's
 * k_gather_ambient run, statement for statement, for a kernel that looks a volume up in the middle of other work (flx_rays_planes_gather.hip).  Those two files keep
 * their copies.  The functions it calls are the definitions of include/flx_volume.h, flx_volume_map.h and flx_volume_relocate.h; the result has the bits of
 * include/flx_gather.h's flx_gather_lookup over the same rows.  HIP only. */
#ifndef FLX_GATHER_CORNERS_H
#define FLX_GATHER_CORNERS_H

#include <hip/hip_runtime.h>

#include "flx_gather.h"

namespace flx {

/* the SH row of probe p, nine 16-byte loads (flx_volume.hip's load_sh) */
__device__ __forceinline__ void corners_load_sh(const float4 *__restrict__ sh, uint32_t p, float row[FLX_PROBE_SH_WORDS]) {
  const float4 *r = sh + (size_t)p * 9u;
#pragma unroll
  for (uint32_t i = 0; i < 9u; i++) {
    const float4 v = r[i];
    row[4u * i] = v.x; row[4u * i + 1u] = v.y; row[4u * i + 2u] = v.z; row[4u * i + 3u] = v.w;
  }
}

/* e <- (E_r, E_g, E_b, W) of position (x, 1.0f) and normal.  maps and map are not read without MAP, offsets not without OFFSETS.  NOT unrolled, a row at a time
 * (flx_volume.hip's volume_irradiance says why); the offset row is read before any SH or map row, an inactive corner reads nothing. */
template <bool MAP, bool OFFSETS>
__device__ __forceinline__ void gather_corners(const float4 *__restrict__ sh, const float4 *__restrict__ maps, const float4 *__restrict__ offsets, const flx_volume_grid &g,
                                               const flx_volume_map &map, const float position[4], const float normal[3], float e[4]) {
  const flx_volume_cell c = flx_volume_cell_of(&g, position, normal);
  float sums[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll 1
  for (uint32_t k = 0; k < 8u; k++) {
    float row[FLX_PROBE_SH_WORDS];
    const uint32_t p = flx_volume_corner(&g, &c, k);
    if constexpr (OFFSETS) {
      const float4 o = offsets[p];
      const float offset[4] = { o.x, o.y, o.z, o.w };
      if (flx_volume_relocate_inactive(offset)) continue;
      corners_load_sh(sh, p, row);
      float dist, dir[3];
      const float tb = flx_volume_relocate_corner(&g, &c, k, normal, offset, &dist, dir);
      if constexpr (MAP) {
        const float4 bin = maps[(size_t)p * flx_volume_map_bins(&map) + flx_volume_map_corner_bin(&map, dir)];
        const float q[4] = { bin.x, bin.y, bin.z, bin.w };
        flx_volume_add(sums, flx_volume_map_weight(&g, tb, dist, q), row, normal);
      } else {
        flx_volume_add(sums, flx_volume_weight_of(&g, tb, dist, row), row, normal);
      }
      continue;
    }
    corners_load_sh(sh, p, row);
    if constexpr (MAP) {
      float dist, dir[3];
      const float tb = flx_volume_weight_base(&g, &c, k, normal, &dist, dir);
      const float4 bin = maps[(size_t)p * flx_volume_map_bins(&map) + flx_volume_map_corner_bin(&map, dir)];      /* (below 2^31 rows: the calls' check) */
      const float q[4] = { bin.x, bin.y, bin.z, bin.w };
      flx_volume_add(sums, flx_volume_map_weight(&g, tb, dist, q), row, normal);
    } else {
      flx_volume_add(sums, flx_volume_weight(&g, &c, k, normal, row), row, normal);
    }
  }
  flx_volume_row(sums, e);
}

}  // namespace flx

#endif
