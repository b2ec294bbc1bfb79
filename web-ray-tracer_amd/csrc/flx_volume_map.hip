/* flx_volume_map.hip — directional visibility on the device: the reduction of radiance rows to octahedral moment maps (include/flexlight_hip_debug.h, "directional
 * visibility": flx_probe_map[_device], flx_debug_last_volume_map) and what the other files' map calls share (flx_volume_map_host.h).  The arithmetic is
 * include/flx_volume_map.h's, the text the tests' CPU reference compiles too: map rows are defined bit for bit.  The fused calls are flx_probes.hip's chunk loop and
 * flx_volume.hip's bake; the lookup with maps is flx_volume.hip's k_volume_irradiance, instantiated with a map.
 *
 * k_probe_map: m m outputs a probe, each a sum over all R = 6 w w texels, where k_probe_sh has one output row a probe.  A WORKGROUP IS ONE PROBE AND 16 BINS: the
 * grid's y names the probe, its x the group of 16 bins; each of the four waves owns four bins, and THE 64 SLOTS OF THE SUMS ARE ITS LANES, as in k_probe_sh.
 *   What a texel gives every bin — direction, d_omega, hit, s: 24 bytes — is made ONCE per workgroup and staged in LDS, in tiles of 1024 texels (24 KB; a multiple
 *   of 64, so that lane j meets the texels j, j + 64, .. of every tile in ascending order): all 256 threads read the tile's radiance rows as 16-byte loads (a wave's
 *   load covers 2 KB without a gap), recompute direction and weight from t with the header and store six words, structure of arrays, so that a wave's 64 lanes read
 *   64 consecutive words.  Then every wave walks the tile for its four bins: six LDS reads a texel feed four bins' sixteen sums, which stay in registers across the
 *   tiles.  w <= 13 is one tile; w = 16 two; w = 256 is 384.
 *   The six steps of the xor tree are six __shfl_xor per sum, in the header's order; lane 0 stores the wave's rows, 16 bytes each.
 *   A wave whose bins lie past m m (the last group; three of four waves where m = 1) still stages and still meets both barriers of every tile: it leaves after the
 *   last one, where nothing waits for it.  A lane without a texel (R < 64) keeps its zeros; a bin past the end within a wave is computed and not stored.
 * No atomics, no scratch (make resources). */
#include <string>

#include "flx_rays_host.h"
#include "flx_probe_args.h"
#include "flx_volume_map.h"
#include "flx_volume_map_host.h"

namespace flx {

constexpr uint32_t MAP_THREADS = 256u;
constexpr uint32_t MAP_TILE = 1024u;            /* texels staged at a time */
constexpr uint32_t MAP_WAVE_BINS = 4u;          /* bins a wave reduces: FLX_VOLUME_MAP_GROUP_BINS / 4 */
static_assert(MAP_TILE % FLX_PROBE_SLOTS == 0u, "a tile keeps every texel in its slot");
static_assert(MAP_WAVE_BINS * (MAP_THREADS / 64u) == FLX_VOLUME_MAP_GROUP_BINS, "a workgroup's bins");

/* radiance: the launch's first probe's rows, g.rays rows of two float4 a probe; maps: its first probe's rows, m m float4 a probe.  blockIdx.y < 32 768. */
__global__ __launch_bounds__(MAP_THREADS) void k_probe_map(const float4 *__restrict__ radiance, float4 *__restrict__ maps, flx_probe_grid g, uint32_t m, uint32_t sharpness) {
  __shared__ float s_d0[MAP_TILE], s_d1[MAP_TILE], s_d2[MAP_TILE], s_dw[MAP_TILE], s_s[MAP_TILE];
  __shared__ uint32_t s_hit[MAP_TILE];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t bins = m * m;
  const uint32_t first_bin = blockIdx.x * FLX_VOLUME_MAP_GROUP_BINS + (threadIdx.x >> 6) * MAP_WAVE_BINS;      /* (wave-uniform; below 256 + 16) */
  const bool works = first_bin < bins;
  const float4 *rows = radiance + (size_t)blockIdx.y * g.rays * 2u;
  float b[MAP_WAVE_BINS][3], sum[MAP_WAVE_BINS][4];
#pragma unroll
  for (uint32_t q = 0; q < MAP_WAVE_BINS; q++) {
    const uint32_t bin = first_bin + q < bins ? first_bin + q : 0u;      /* (a bin past the end: computed as bin 0, never stored) */
    flx_volume_map_bin_direction(m, bin, b[q]);
    sum[q][0] = 0.0f; sum[q][1] = 0.0f; sum[q][2] = 0.0f; sum[q][3] = 0.0f;
  }
  for (uint32_t base = 0; base < g.rays; base += MAP_TILE) {
    const uint32_t count = g.rays - base < MAP_TILE ? g.rays - base : MAP_TILE;
    for (uint32_t i = threadIdx.x; i < count; i += MAP_THREADS) {
      const uint32_t t = base + i;
      const float4 r0 = rows[(size_t)t * 2u], r1 = rows[(size_t)t * 2u + 1u];
      const flx_volume_map_texel x = flx_volume_map_texel_of(&g, t, r0.w, r1.x);
      s_d0[i] = x.d[0]; s_d1[i] = x.d[1]; s_d2[i] = x.d[2]; s_dw[i] = x.dw; s_s[i] = x.s; s_hit[i] = x.hit ? 1u : 0u;
    }
    __syncthreads();
    if (works) {
      for (uint32_t i = lane; i < count; i += FLX_PROBE_SLOTS) {
        flx_volume_map_texel x;
        x.d[0] = s_d0[i]; x.d[1] = s_d1[i]; x.d[2] = s_d2[i]; x.dw = s_dw[i]; x.s = s_s[i]; x.hit = s_hit[i] != 0u;
#pragma unroll
        for (uint32_t q = 0; q < MAP_WAVE_BINS; q++) {
          float term[4];
          flx_volume_map_terms(&x, b[q], sharpness, term);
          sum[q][0] = sum[q][0] + term[0]; sum[q][1] = sum[q][1] + term[1]; sum[q][2] = sum[q][2] + term[2]; sum[q][3] = sum[q][3] + term[3];
        }
      }
    }
    __syncthreads();      /* (the next tile overwrites what the slowest wave still reads) */
  }
  if (!works) return;      /* the whole wave, behind the last barrier */
  /* all 64 lanes are here; v[j] + v[j ^ off], off = 1, 2, 4, 8, 16, 32 */
#pragma unroll
  for (uint32_t off = 1u; off < FLX_PROBE_SLOTS; off <<= 1) {
#pragma unroll
    for (uint32_t q = 0; q < MAP_WAVE_BINS; q++) {
#pragma unroll
      for (uint32_t k = 0; k < 4u; k++) sum[q][k] = sum[q][k] + __shfl_xor(sum[q][k], (int)off, 64);
    }
  }
  if (lane != 0u) return;
  float4 *o = maps + (size_t)blockIdx.y * bins;
#pragma unroll
  for (uint32_t q = 0; q < MAP_WAVE_BINS; q++)
    if (first_bin + q < bins) o[first_bin + q] = make_float4(sum[q][0], sum[q][1], sum[q][2], sum[q][3]);
}

}  // namespace flx

using namespace flx;

static flx_status fail(flx_context *ctx, flx_status code, const std::string &msg) { return flx_fail(ctx, code, msg.c_str()); }

/* a refusal of flx_volume_map_args.h in words */
static flx_status map_refusal(flx_context *ctx, enum flx_volume_map_refusal why, const char *call) {
  const char *what = "";
  switch (why) {
    case FLX_VOLUME_MAP_ARGS_OK: return FLX_OK;
    case FLX_VOLUME_MAP_NULL: what = "the map is NULL"; break;
    case FLX_VOLUME_MAP_SIZE: what = "the map's size is not one of 1 .. 16"; break;
    case FLX_VOLUME_MAP_SHARPNESS: what = "the map's sharpness is above 8"; break;
    case FLX_VOLUME_MAP_RESERVED: what = "a reserved word of the map is not 0"; break;
    case FLX_VOLUME_MAP_ROWS: what = "the maps have 2^31 rows or more"; break;
    case FLX_VOLUME_MAPS_NULL: what = "the maps array is NULL"; break;
    case FLX_VOLUME_MAPS_WRAPS: what = "the maps array leaves the address space"; break;
    case FLX_VOLUME_MAPS_OVERLAP: what = "the maps overlap another array"; break;
  }
  return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": " + what);
}

flx_status flx_volume_map_refused(flx_context *ctx, const flx_volume_map *map, uint32_t n_probes, uint32_t *rows, const char *call) {
  const enum flx_volume_map_refusal why = flx_volume_map_check(map);
  return map_refusal(ctx, why != FLX_VOLUME_MAP_ARGS_OK ? why : flx_volume_map_rows_check(n_probes, map->size, rows), call);
}

flx_status flx_volume_maps_refused(flx_context *ctx, const void *d_maps, uint32_t rows, const flx_map_other *others, int k, const char *call) {
  uint64_t address[FLX_VOLUME_MAP_MAX_ARRAYS], bytes[FLX_VOLUME_MAP_MAX_ARRAYS];
  for (int i = 0; i < k; i++) { address[i] = (uint64_t)(uintptr_t)others[i].p; bytes[i] = others[i].bytes; }
  const enum flx_volume_map_refusal why = flx_volume_maps_check((uint64_t)(uintptr_t)d_maps, flx_volume_map_bytes(rows), address, bytes, k);
  if (why != FLX_VOLUME_MAP_ARGS_OK && why != FLX_VOLUME_MAPS_OVERLAP) return map_refusal(ctx, why, call);      /* (overlap: said after the pointer is known to be the device's) */
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  if (!flx_rows_on_device(ctx, d_maps, (size_t)flx_volume_map_bytes(rows)))
    return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": the maps are not n_probes * size * size rows of 16 bytes in memory of the context's device, 16-byte aligned");
  return map_refusal(ctx, why, call);
}

flx_status flx_probe_map_enqueue(flx_context *ctx, const float4 *d_radiance, uint32_t n, const flx_probe_grid &g, const flx_volume_map &map, float4 *d_maps, uint32_t all) {
  const uint32_t bin_groups = flx_volume_map_bin_groups(map.size), bins = map.size * map.size;
  uint32_t launches = 0, groups = 0;
  for (uint32_t first = 0; first < n; first += FLX_VOLUME_MAP_LAUNCH) {
    const uint32_t m = n - first < FLX_VOLUME_MAP_LAUNCH ? n - first : FLX_VOLUME_MAP_LAUNCH;
    hipLaunchKernelGGL(k_probe_map, dim3(bin_groups, m), dim3(MAP_THREADS), 0, ctx->stream, d_radiance + (size_t)first * g.rays * 2u, d_maps + (size_t)first * bins, g, map.size,
                       map.sharpness);
    FLX_HIP(ctx, hipGetLastError());
    groups = bin_groups * m;
    launches++;
    if (n - first <= FLX_VOLUME_MAP_LAUNCH) break;          /* (first + 32 768 could wrap) */
  }
  flx_context::VolumeMapLaunch ran;
  ran.probes = all; ran.size = map.size; ran.sharpness = map.sharpness; ran.launches = launches; ran.groups = groups; ran.face_size = g.w;
  ctx->last_volume_map = ran;
  return FLX_OK;
}

static flx_status probe_count_refused(flx_context *ctx, uint32_t n_probes, uint32_t face_size, uint32_t *rays, const char *call) {
  if (flx_probe_face_check(face_size) != FLX_PROBE_ARGS_OK) return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": face_size is not one of 1 .. 256");
  if (flx_probe_count_check(n_probes, face_size, rays) != FLX_PROBE_ARGS_OK)
    return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": n_probes * 6 * face_size * face_size is 2^32 or more");
  return FLX_OK;
}

extern "C" flx_status flx_probe_map_device(flx_context *ctx, const void *d_radiance, uint32_t n_probes, uint32_t face_size, const flx_volume_map *map, void *d_maps,
                                           void *producer_stream) {
  static const char *const call = "flx_probe_map_device";
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t rays = 0, rows = 0;
  flx_status s = probe_count_refused(ctx, n_probes, face_size, &rays, call);
  if (s || (s = flx_volume_map_refused(ctx, map, n_probes, &rows, call)) || n_probes == 0u) return s;
  const uint64_t radiance_bytes = (uint64_t)rays * FLX_RAY_ROW_BYTES;
  if (!d_radiance) return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": an array is NULL");
  if (flx_range_wraps((uint64_t)(uintptr_t)d_radiance, radiance_bytes)) return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": an array leaves the address space");
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  if (!flx_rows_on_device(ctx, d_radiance, (size_t)radiance_bytes))
    return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": the radiance is not n_probes * 6 * face_size * face_size rows in memory of the context's device, 16-byte aligned");
  const flx_map_other others[1] = { { d_radiance, radiance_bytes } };
  if ((s = flx_volume_maps_refused(ctx, d_maps, rows, others, 1, call))) return s;
  if ((s = flx_server_stop(ctx)) || (s = flx_wait_for_producer(ctx, producer_stream))) return s;
  return flx_probe_map_enqueue(ctx, (const float4 *)d_radiance, n_probes, flx_probe_grid_of(face_size), *map, (float4 *)d_maps, n_probes);
}

extern "C" flx_status flx_probe_map(flx_context *ctx, const void *radiance, uint32_t n_probes, uint32_t face_size, const flx_volume_map *map, float *maps) {
  static const char *const call = "flx_probe_map";
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t rays = 0, rows = 0;
  flx_status s = probe_count_refused(ctx, n_probes, face_size, &rays, call);
  if (s || (s = flx_volume_map_refused(ctx, map, n_probes, &rows, call)) || n_probes == 0u) return s;
  if (!radiance) return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": an array is NULL");
  if (!maps) return map_refusal(ctx, FLX_VOLUME_MAPS_NULL, call);
  /* the radiance rows go up where a ray batch's rays go: rows of 32 bytes both */
  return flx_rays_from_host(ctx, (const float *)radiance, rays,
                            [&]() { return flx_probe_map_device(ctx, ctx->d_query_rays.get(), n_probes, face_size, map, ctx->d_volume_maps.get(), nullptr); },
                            flx_down(&ctx->d_volume_maps, (size_t)rows, maps));
}

extern "C" flx_status flx_debug_last_volume_map(flx_context *ctx, uint32_t out[8]) {
  if (!ctx || !out) return FLX_ERR_INVALID;
  const flx_context::VolumeMapLaunch &v = ctx->last_volume_map;
  out[0] = v.probes; out[1] = v.size; out[2] = v.sharpness; out[3] = v.launches; out[4] = v.groups; out[5] = v.face_size; out[6] = 0u; out[7] = 0u;
  return FLX_OK;
}
