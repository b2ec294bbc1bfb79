/* flx_volume.hip — probe volumes on the device (include/flexlight_hip_debug.h, "probe volumes": flx_volume_positions[_device], flx_volume_bake[_device],
 * flx_volume_irradiance[_device], flx_rays_irradiance[_device], flx_frame_irradiance[_device], flx_volume_irradiance_of).  The arithmetic is include/flx_volume.h's,
 * the text the tests' CPU reference compiles too: position rows and irradiance rows are defined bit for bit.
 *
 * k_volume_positions: ONE LANE PER PROBE; a lane writes its 16-byte row, consecutive lanes consecutive rows.  No loads.
 *
 * k_volume_irradiance: ONE LANE PER POINT, 256 threads.  A lane reads its position row and its normal row as one 16-byte load each and writes its irradiance row as
 * one 16-byte store: a wave moves 1 KiB contiguous per plane.  A miss writes its zeros and leaves before any probe is read.  The eight SH rows of a point are nine
 * float4 loads each into registers, a row at a time; the header's functions run on them corner by corner in ascending k.  flx_probe_irradiance_of is called per
 * corner as the header says; it is inlined and the basis of the normal, which does not depend on the corner, is computed once per point by the compiler's common
 * subexpression elimination (the ISA has one set of the basis' products).
 *   THERE IS NO SECOND PATH FOR COHERENT WAVES.  A variant that compared every lane's base index with the first lane's (readfirstlane, a ballot) and, where all
 *   agreed, read the eight rows through wave-uniform addresses as scalar loads was built and measured on the dragon at 1080p: 0.088 ms against this gather's 0.094,
 *   the two runs' ranges overlapping (profiles/volume.txt).  It was deleted as the issue of its keeping was set: faster only if outside the spread.
 * No LDS, no atomics, no scratch (make resources).
 *   k_volume_irradiance_map is the same body instantiated with a map (include/flx_volume_map.h, "directional visibility"): per corner the encode of the direction
 *   from the probe to the point and one 16-byte gather of that bin's row, whose moments stand in for the SH row's words 7, 11 and 15.  The instantiation without a
 *   map is the code it was.  Every lookup call and its _map sibling are one implementation (irradiance_run, rays_run, frame_run), which the plain calls enter with no
 *   maps; the map's own refusals (flx_volume_map_host.h) are asked after the siblings'.
 *
 * flx_volume_bake_device is k_volume_positions into ctx->d_volume_positions and flx_probes_sh_device from there: there is no second probe path.
 * flx_rays_irradiance_device and flx_frame_irradiance_device are flx_rays_surface_device / flx_frame_surface_device, as they stand, into ctx->d_volume_surface
 * (a position plane and a normal plane) and k_volume_irradiance behind them on the context's stream; a ray batch goes slab by slab (flx_trace_slab_rays at one slot a
 * ray), so the buffer ends at 2^21 x 32 bytes.  The host-memory calls are the ray-batch calls' shared path (flx_rays_host.h). */
#include <string>

#include "flx_context.h"
#include "flx_query_args.h"
#include "flx_rays_host.h"
#include "flx_volume_args.h"
#include "flx_volume_map.h"
#include "flx_volume_map_host.h"
#include "flx_volume_relocate.h"

namespace flx {

constexpr uint32_t VOLUME_THREADS = FLX_VOLUME_THREADS;

/* positions: n = flx_volume_probes(&g) rows */
__global__ __launch_bounds__(VOLUME_THREADS) void k_volume_positions(float4 *__restrict__ positions, flx_volume_grid g, uint32_t n) {
  const uint32_t p = blockIdx.x * VOLUME_THREADS + threadIdx.x;      /* (blockIdx.x <= (n - 1) / 256 and n < 2^31: no wrap) */
  if (p >= n) return;
  float row[4];
  flx_volume_position(&g, p, row);
  positions[p] = make_float4(row[0], row[1], row[2], row[3]);
}

/* the SH row of probe p, nine 16-byte loads (of which the compiler keeps the words the header reads) */
__device__ __forceinline__ void load_sh(const float4 *__restrict__ sh, uint32_t p, float row[FLX_PROBE_SH_WORDS]) {
  const float4 *r = sh + (size_t)p * 9u;
#pragma unroll
  for (uint32_t i = 0; i < 9u; i++) {
    const float4 v = r[i];
    row[4u * i] = v.x; row[4u * i + 1u] = v.y; row[4u * i + 2u] = v.z; row[4u * i + 3u] = v.w;
  }
}

/* sh: the grid's rows; positions, normals, out: n rows each.  MAP: the directional weight (include/flx_volume_map.h) — per corner the encode and one 16-byte gather
 * of the bin's row from maps (m m rows a probe), in place of the row's words 7, 11 and 15; without it the body is what it was, and maps and map are not read. */
/* OFFSETS: the lookup with offsets (include/flx_volume_relocate.h) — per corner one 16-byte load of the probe's offset row BEFORE any SH or map row is read; an
 * inactive corner is left there, and the others' probes stand at the lattice point plus the offset.  Without it the body is what it was, and offsets is not read. */
template <bool MAP, bool OFFSETS = false>
__device__ __forceinline__ void volume_irradiance(const float4 *__restrict__ sh, const float4 *__restrict__ maps, const float4 *__restrict__ positions,
                                                  const float4 *__restrict__ normals, float4 *__restrict__ out, const flx_volume_grid &g, const flx_volume_map &map, uint32_t n,
                                                  const float4 *__restrict__ offsets = nullptr) {
  const uint32_t r = blockIdx.x * VOLUME_THREADS + threadIdx.x;      /* (n / 256 + 1 workgroups: no wrap) */
  if (r >= n) return;
  const float4 x = positions[r];
  const float position[4] = { x.x, x.y, x.z, x.w };
  if (flx_volume_miss(position)) { out[r] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); return; }
  const float4 nn = normals[r];
  const float normal[3] = { nn.x, nn.y, nn.z };
  const flx_volume_cell c = flx_volume_cell_of(&g, position, normal);
  float sums[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
  /* (not unrolled: unrolled, the compiler hoists all 72 loads and keeps 288 values live — 251 VGPRs and one wave a SIMD; a row at a time it is 71 VGPRs and seven) */
#pragma unroll 1
  for (uint32_t k = 0; k < 8u; k++) {
    float row[FLX_PROBE_SH_WORDS];
    const uint32_t p = flx_volume_corner(&g, &c, k);
    if constexpr (OFFSETS) {
      const float4 o = offsets[p];
      const float offset[4] = { o.x, o.y, o.z, o.w };
      if (flx_volume_relocate_inactive(offset)) continue;
      load_sh(sh, p, row);
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
    load_sh(sh, p, row);
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
  float e[4];
  flx_volume_row(sums, e);
  out[r] = make_float4(e[0], e[1], e[2], e[3]);
}

__global__ __launch_bounds__(VOLUME_THREADS) void k_volume_irradiance(const float4 *__restrict__ sh, const float4 *__restrict__ positions, const float4 *__restrict__ normals,
                                                                      float4 *__restrict__ out, flx_volume_grid g, uint32_t n) {
  const flx_volume_map none = { 0u, 0u, { 0u, 0u } };
  volume_irradiance<false>(sh, nullptr, positions, normals, out, g, none, n);
}

__global__ __launch_bounds__(VOLUME_THREADS) void k_volume_irradiance_map(const float4 *__restrict__ sh, const float4 *__restrict__ maps, const float4 *__restrict__ positions,
                                                                          const float4 *__restrict__ normals, float4 *__restrict__ out, flx_volume_grid g, flx_volume_map map,
                                                                          uint32_t n) {
  volume_irradiance<true>(sh, maps, positions, normals, out, g, map, n);
}

__global__ __launch_bounds__(VOLUME_THREADS) void k_volume_irradiance_relocated(const float4 *__restrict__ sh, const float4 *__restrict__ offsets, const float4 *__restrict__ positions,
                                                                                const float4 *__restrict__ normals, float4 *__restrict__ out, flx_volume_grid g, uint32_t n) {
  const flx_volume_map none = { 0u, 0u, { 0u, 0u } };
  volume_irradiance<false, true>(sh, nullptr, positions, normals, out, g, none, n, offsets);
}

__global__ __launch_bounds__(VOLUME_THREADS) void k_volume_irradiance_map_relocated(const float4 *__restrict__ sh, const float4 *__restrict__ maps, const float4 *__restrict__ offsets,
                                                                                    const float4 *__restrict__ positions, const float4 *__restrict__ normals, float4 *__restrict__ out,
                                                                                    flx_volume_grid g, flx_volume_map map, uint32_t n) {
  volume_irradiance<true, true>(sh, maps, positions, normals, out, g, map, n, offsets);
}

}  // namespace flx

using namespace flx;

/* ---- the calls ------------------------------------------------------------------------------------------------------------------------------------- */

static flx_status fail(flx_context *ctx, flx_status code, const std::string &msg) { return flx_fail(ctx, code, msg.c_str()); }

/* a refusal of flx_volume_args.h in words */
static flx_status volume_refusal(flx_context *ctx, enum flx_volume_refusal why, const char *call) {
  const char *what = "";
  switch (why) {
    case FLX_VOLUME_ARGS_OK: return FLX_OK;
    case FLX_VOLUME_GRID_NULL: what = "the grid is NULL"; break;
    case FLX_VOLUME_COUNT_ZERO: what = "a count of the grid is 0"; break;
    case FLX_VOLUME_PROBES: what = "the grid has 2^31 probes or more"; break;
    case FLX_VOLUME_NOT_FINITE: what = "origin or spacing holds a value that is not finite"; break;
    case FLX_VOLUME_SPACING: what = "a spacing is not greater than 0"; break;
    case FLX_VOLUME_BIAS: what = "normal_bias is negative or not finite"; break;
    case FLX_VOLUME_FLOOR: what = "floor is not one of 0 .. 1"; break;
    case FLX_VOLUME_FLAGS: what = "flags has a bit beyond FLX_VOLUME_VISIBILITY"; break;
    case FLX_VOLUME_RESERVED: what = "reserved is not 0"; break;
    case FLX_VOLUME_NULL: what = "an array is NULL"; break;
    case FLX_VOLUME_WRAPS: what = "an array leaves the address space"; break;
    case FLX_VOLUME_OVERLAP: what = "the arrays overlap"; break;
  }
  return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": " + what);
}

/* the same for the files whose calls take a grid beside their own arguments (flx_volume_update.hip) */
flx_status flx_volume_grid_refused(flx_context *ctx, const flx_volume_grid *grid, uint32_t *probes, const char *call) { return volume_refusal(ctx, flx_volume_grid_check(grid, probes), call); }

/* an array of a device call: what it is, for the message */
struct VolumeArray { const void *p; uint64_t bytes; const char *what; };

/* the maps of a call: none (the plain calls), or the map and its rows on the device (the _map calls; either may be NULL, which is refused) */
struct VolumeMaps { const flx_volume_map *map = nullptr; const void *d_maps = nullptr; bool has = false; const void *d_offsets = nullptr; bool relocated = false; };
static VolumeMaps with_maps(const flx_volume_map *map, const void *d_maps) {
  VolumeMaps maps;
  maps.map = map; maps.d_maps = d_maps; maps.has = true;
  return maps;
}
/* the same for a relocated call: the map and its rows where either is given (both NULL: the whole-sphere moments), and the offset rows */
static VolumeMaps with_offsets(const flx_volume_map *map, const void *d_maps, const void *d_offsets) {
  VolumeMaps maps = (map || d_maps) ? with_maps(map, d_maps) : VolumeMaps();
  maps.d_offsets = d_offsets; maps.relocated = true;
  return maps;
}

/* The k arrays of a device call: there, inside 64 bits, memory of the context's device, and apart — in that order. */
static flx_status arrays_refused(flx_context *ctx, const VolumeArray *arrays, int k, const char *call) {
  uint64_t address[FLX_VOLUME_MAX_ARRAYS], bytes[FLX_VOLUME_MAX_ARRAYS];
  for (int i = 0; i < k; i++) { address[i] = (uint64_t)(uintptr_t)arrays[i].p; bytes[i] = arrays[i].bytes; }
  const enum flx_volume_refusal why = flx_volume_arrays_check(address, bytes, k);
  if (why != FLX_VOLUME_ARGS_OK && why != FLX_VOLUME_OVERLAP) return volume_refusal(ctx, why, call);      /* (overlap: said after the pointers are known to be the device's) */
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  for (int i = 0; i < k; i++)
    if (!flx_rows_on_device(ctx, arrays[i].p, (size_t)arrays[i].bytes))
      return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": " + arrays[i].what + " in memory of the context's device, 16-byte aligned");
  return volume_refusal(ctx, why, call);
}

/* what a map call asks after its sibling's own refusals: the map and its rows for the grid's probes ... */
static flx_status maps_params_refused(flx_context *ctx, const VolumeMaps &maps, uint32_t probes, uint32_t *rows, const char *call) {
  return maps.has ? flx_volume_map_refused(ctx, maps.map, probes, rows, call) : FLX_OK;
}

/* ... and, behind the sibling's arrays, the maps array against them */
static flx_status maps_array_refused(flx_context *ctx, const VolumeMaps &maps, uint32_t rows, const VolumeArray *arrays, int k, const char *call) {
  if (!maps.has) return FLX_OK;
  flx_map_other others[FLX_VOLUME_MAX_ARRAYS];
  for (int i = 0; i < k; i++) others[i] = { arrays[i].p, arrays[i].bytes };
  return flx_volume_maps_refused(ctx, maps.d_maps, rows, others, k, call);
}

/* ... and, behind both, a relocated call's offset rows against them and the maps */
static flx_status offsets_array_refused(flx_context *ctx, const VolumeMaps &maps, uint32_t probes, uint32_t rows, const VolumeArray *arrays, int k, const char *call) {
  if (!maps.relocated) return FLX_OK;
  const void *others[FLX_VOLUME_MAX_ARRAYS + 1];
  uint64_t bytes[FLX_VOLUME_MAX_ARRAYS + 1];
  for (int i = 0; i < k; i++) { others[i] = arrays[i].p; bytes[i] = arrays[i].bytes; }
  if (maps.has) { others[k] = maps.d_maps; bytes[k] = flx_volume_map_bytes(rows); k++; }
  return flx_volume_offsets_refused(ctx, maps.d_offsets, probes, others, bytes, k, call);
}

static flx_status positions_enqueue(flx_context *ctx, const flx_volume_grid &g, uint32_t probes, float4 *d_positions) {
  hipLaunchKernelGGL(k_volume_positions, dim3(flx_volume_groups(probes)), dim3(VOLUME_THREADS), 0, ctx->stream, d_positions, g, probes);
  FLX_HIP(ctx, hipGetLastError());
  return FLX_OK;
}

static flx_status lookup_enqueue(flx_context *ctx, const flx_volume_grid &g, const float4 *d_sh, const float4 *d_positions, const float4 *d_normals, uint32_t n, float4 *d_out,
                                 const VolumeMaps &maps) {
  if (maps.relocated && maps.has)
    hipLaunchKernelGGL(k_volume_irradiance_map_relocated, dim3(flx_volume_groups(n)), dim3(VOLUME_THREADS), 0, ctx->stream, d_sh, (const float4 *)maps.d_maps,
                       (const float4 *)maps.d_offsets, d_positions, d_normals, d_out, g, *maps.map, n);
  else if (maps.relocated)
    hipLaunchKernelGGL(k_volume_irradiance_relocated, dim3(flx_volume_groups(n)), dim3(VOLUME_THREADS), 0, ctx->stream, d_sh, (const float4 *)maps.d_offsets, d_positions, d_normals,
                       d_out, g, n);
  else if (maps.has)
    hipLaunchKernelGGL(k_volume_irradiance_map, dim3(flx_volume_groups(n)), dim3(VOLUME_THREADS), 0, ctx->stream, d_sh, (const float4 *)maps.d_maps, d_positions, d_normals, d_out, g,
                       *maps.map, n);
  else
    hipLaunchKernelGGL(k_volume_irradiance, dim3(flx_volume_groups(n)), dim3(VOLUME_THREADS), 0, ctx->stream, d_sh, d_positions, d_normals, d_out, g, n);
  FLX_HIP(ctx, hipGetLastError());
  return FLX_OK;
}

static void lookup_ran(flx_context *ctx, const flx_volume_grid &g, uint32_t probes, uint32_t n, uint32_t slabs, uint32_t slab, uint32_t source, uint32_t groups) {
  flx_context::VolumeLaunch ran;
  ran.n = n; ran.slabs = slabs; ran.slab = slab; ran.probes = probes; ran.flags = g.flags; ran.source = source; ran.groups = groups;
  ctx->last_volume = ran;
}

extern "C" flx_status flx_volume_positions_device(flx_context *ctx, const flx_volume_grid *grid, void *d_positions, void *producer_stream) {
  static const char *const call = "flx_volume_positions_device";
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t probes = 0;
  flx_status s = volume_refusal(ctx, flx_volume_grid_check(grid, &probes), call);
  if (s) return s;
  const VolumeArray arrays[1] = { { d_positions, flx_volume_position_bytes(probes), "the positions are not nx * ny * nz rows of 16 bytes" } };
  if ((s = arrays_refused(ctx, arrays, 1, call))) return s;
  if ((s = flx_server_stop(ctx)) || (s = flx_wait_for_producer(ctx, producer_stream))) return s;
  return positions_enqueue(ctx, *grid, probes, (float4 *)d_positions);
}

extern "C" flx_status flx_volume_positions(flx_context *ctx, const flx_volume_grid *grid, float *positions) {
  static const char *const call = "flx_volume_positions";
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t probes = 0;
  flx_status s = volume_refusal(ctx, flx_volume_grid_check(grid, &probes), call);
  if (s) return s;
  if (!positions) return volume_refusal(ctx, FLX_VOLUME_NULL, call);
  return flx_rays_from_host(ctx, nullptr, 0u, [&]() { return flx_volume_positions_device(ctx, grid, ctx->d_query_hits.get(), nullptr); },
                            flx_down(&ctx->d_query_hits, (size_t)probes, positions));
}

/* what both bake calls refuse before they look at an array: the scene, the trace params and the probe params, asked of flx_probes_sh_device in its words (no
 * probes: it looks at them and at nothing else, and enqueues nothing), then the grid */
static flx_status bake_refused(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, uint32_t *probes, const char *call) {
  flx_status s = flx_probes_sh_device(ctx, trace, params, nullptr, 0u, nullptr, nullptr);
  return s ? s : volume_refusal(ctx, flx_volume_grid_check(grid, probes), call);
}

/* flx_volume_bake_device and flx_volume_bake_map_device: one implementation; d_maps: where the maps go (maps.has) */
static flx_status bake_run(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, void *d_sh, const VolumeMaps &maps,
                           void *d_maps, void *producer_stream, const char *call) {
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t probes = 0, rows = 0;
  flx_status s = bake_refused(ctx, trace, params, grid, &probes, call);
  if (s || (s = maps_params_refused(ctx, maps, probes, &rows, call))) return s;
  const VolumeArray arrays[1] = { { d_sh, flx_volume_sh_bytes(probes), "the SH rows are not nx * ny * nz rows of 144 bytes" } };
  if ((s = arrays_refused(ctx, arrays, 1, call)) || (s = maps_array_refused(ctx, maps, rows, arrays, 1, call))) return s;
  if ((s = flx_server_stop(ctx))) return s;
  if ((s = flx_grow(ctx, flx_need(&ctx->d_volume_positions, (size_t)probes)))) return s;
  if ((s = flx_wait_for_producer(ctx, producer_stream))) return s;
  if ((s = positions_enqueue(ctx, *grid, probes, ctx->d_volume_positions.get()))) return s;
  return maps.has ? flx_probes_sh_map_device(ctx, trace, params, maps.map, ctx->d_volume_positions.get(), probes, d_sh, d_maps, nullptr)
                  : flx_probes_sh_device(ctx, trace, params, ctx->d_volume_positions.get(), probes, d_sh, nullptr);
}

extern "C" flx_status flx_volume_bake_device(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, void *d_sh,
                                             void *producer_stream) {
  return bake_run(ctx, trace, params, grid, d_sh, VolumeMaps(), nullptr, producer_stream, "flx_volume_bake_device");
}

extern "C" flx_status flx_volume_bake_map_device(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, const flx_volume_map *map,
                                                 void *d_sh, void *d_maps, void *producer_stream) {
  return bake_run(ctx, trace, params, grid, d_sh, with_maps(map, d_maps), d_maps, producer_stream, "flx_volume_bake_map_device");
}

extern "C" flx_status flx_volume_bake_map(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, const flx_volume_map *map,
                                          float *sh, float *maps) {
  static const char *const call = "flx_volume_bake_map";
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t probes = 0, rows = 0;
  flx_status s = bake_refused(ctx, trace, params, grid, &probes, call);
  if (s || (s = flx_volume_map_refused(ctx, map, probes, &rows, call))) return s;
  if (!sh) return volume_refusal(ctx, FLX_VOLUME_NULL, call);
  if (!maps) return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": the maps array is NULL");
  return flx_rays_from_host(ctx, nullptr, 0u, [&]() { return flx_volume_bake_map_device(ctx, trace, params, grid, map, ctx->d_query_hits.get(), ctx->d_volume_maps.get(), nullptr); },
                            flx_down(&ctx->d_query_hits, (size_t)probes * 9u, sh), flx_down(&ctx->d_volume_maps, (size_t)rows, maps));
}

extern "C" flx_status flx_volume_bake(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, float *sh) {
  static const char *const call = "flx_volume_bake";
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t probes = 0;
  flx_status s = bake_refused(ctx, trace, params, grid, &probes, call);
  if (s) return s;
  if (!sh) return volume_refusal(ctx, FLX_VOLUME_NULL, call);
  return flx_rays_from_host(ctx, nullptr, 0u, [&]() { return flx_volume_bake_device(ctx, trace, params, grid, ctx->d_query_hits.get(), nullptr); },
                            flx_down(&ctx->d_query_hits, (size_t)probes * 9u, sh));
}

/* THE LOOKUPS: each _device call and its _map sibling are one implementation, `maps` telling them apart. */
static flx_status irradiance_run(flx_context *ctx, const flx_volume_grid *grid, const void *d_sh, const void *d_positions, const void *d_normals, uint32_t n, void *d_out,
                                 const VolumeMaps &maps, void *producer_stream, const char *call) {
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t probes = 0, rows = 0;
  flx_status s = volume_refusal(ctx, flx_volume_grid_check(grid, &probes), call);
  if (s || (s = maps_params_refused(ctx, maps, probes, &rows, call)) || n == 0u) return s;
  const VolumeArray arrays[4] = { { d_sh, flx_volume_sh_bytes(probes), "the SH rows are not nx * ny * nz rows of 144 bytes" },
                                  { d_positions, flx_volume_plane_bytes(n), "the positions are not n rows of 16 bytes" },
                                  { d_normals, flx_volume_plane_bytes(n), "the normals are not n rows of 16 bytes" },
                                  { d_out, flx_volume_plane_bytes(n), "the irradiance rows are not n rows of 16 bytes" } };
  if ((s = arrays_refused(ctx, arrays, 4, call)) || (s = maps_array_refused(ctx, maps, rows, arrays, 4, call)) || (s = offsets_array_refused(ctx, maps, probes, rows, arrays, 4, call))) return s;
  if ((s = flx_server_stop(ctx)) || (s = flx_wait_for_producer(ctx, producer_stream))) return s;
  if ((s = lookup_enqueue(ctx, *grid, (const float4 *)d_sh, (const float4 *)d_positions, (const float4 *)d_normals, n, (float4 *)d_out, maps))) return s;
  lookup_ran(ctx, *grid, probes, n, 1u, n, 0u, flx_volume_groups(n));
  return FLX_OK;
}

extern "C" flx_status flx_volume_irradiance_device(flx_context *ctx, const flx_volume_grid *grid, const void *d_sh, const void *d_positions, const void *d_normals, uint32_t n,
                                                   void *d_out, void *producer_stream) {
  return irradiance_run(ctx, grid, d_sh, d_positions, d_normals, n, d_out, VolumeMaps(), producer_stream, "flx_volume_irradiance_device");
}

extern "C" flx_status flx_volume_irradiance_map_device(flx_context *ctx, const flx_volume_grid *grid, const void *d_sh, const void *d_positions, const void *d_normals, uint32_t n,
                                                       void *d_out, const flx_volume_map *map, const void *d_maps, void *producer_stream) {
  return irradiance_run(ctx, grid, d_sh, d_positions, d_normals, n, d_out, with_maps(map, d_maps), producer_stream, "flx_volume_irradiance_map_device");
}

/* the SH rows of a host variant into ctx->d_volume_sh, on the context's stream */
static flx_status sh_up(flx_context *ctx, const float *sh, uint32_t probes) {
  flx_status s = flx_grow(ctx, flx_need(&ctx->d_volume_sh, (size_t)probes * 9u));
  if (s) return s;
  FLX_HIP(ctx, hipMemcpyAsync(ctx->d_volume_sh.get(), sh, (size_t)flx_volume_sh_bytes(probes), hipMemcpyHostToDevice, ctx->stream));
  return FLX_OK;
}

/* the map rows of a host variant into ctx->d_volume_maps, on the context's stream; -> the call's maps on the device (none where the call has none) */
static flx_status maps_up(flx_context *ctx, const flx_volume_map *map, const float *maps, uint32_t rows, VolumeMaps *up) {
  *up = VolumeMaps();
  if (!map) return FLX_OK;
  flx_status s = flx_grow(ctx, flx_need(&ctx->d_volume_maps, (size_t)rows));
  if (s) return s;
  FLX_HIP(ctx, hipMemcpyAsync(ctx->d_volume_maps.get(), maps, (size_t)flx_volume_map_bytes(rows), hipMemcpyHostToDevice, ctx->stream));
  *up = with_maps(map, ctx->d_volume_maps.get());
  return FLX_OK;
}

/* the offset rows of a relocated host variant into ctx->d_relocate_offsets, on the context's stream; *up becomes the relocated call's (offsets NULL: *up is left) */
static flx_status offsets_up(flx_context *ctx, const float *offsets, uint32_t probes, VolumeMaps *up) {
  if (!offsets) return FLX_OK;
  flx_status s = flx_grow(ctx, flx_need(&ctx->d_relocate_offsets, (size_t)probes));
  if (s) return s;
  FLX_HIP(ctx, hipMemcpyAsync(ctx->d_relocate_offsets.get(), offsets, (size_t)probes * 16u, hipMemcpyHostToDevice, ctx->stream));
  up->d_offsets = ctx->d_relocate_offsets.get(); up->relocated = true;
  return FLX_OK;
}

/* what a host map call refuses behind its sibling's grid: the map, its rows, a NULL maps array (has_map: the call is a _map call) */
static flx_status host_maps_refused(flx_context *ctx, bool has_map, const flx_volume_map *map, const float *maps, uint32_t probes, uint32_t *rows, const char *call) {
  if (!has_map) return FLX_OK;
  const flx_status s = flx_volume_map_refused(ctx, map, probes, rows, call);
  if (s) return s;
  return maps ? FLX_OK : fail(ctx, FLX_ERR_INVALID, std::string(call) + ": the maps array is NULL");
}

/* (relocated: the call takes offset rows, which must be there; the device call's name follows) */
static flx_status irradiance_host(flx_context *ctx, const flx_volume_grid *grid, const float *sh, const float *positions, const float *normals, uint32_t n, float *out, bool has_map,
                                  const flx_volume_map *map, const float *maps, const char *call, bool relocated = false, const float *offsets = nullptr) {
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t probes = 0, rows = 0;
  flx_status s = volume_refusal(ctx, flx_volume_grid_check(grid, &probes), call);
  if (s || (has_map && (s = flx_volume_map_refused(ctx, map, probes, &rows, call))) || n == 0u) return s;
  if (!sh || !positions || !normals || !out || (relocated && !offsets)) return volume_refusal(ctx, FLX_VOLUME_NULL, call);
  if ((s = host_maps_refused(ctx, has_map, map, maps, probes, &rows, call))) return s;
  /* the two planes go up where a ray batch's rays go, one behind the other: n rows of 32 bytes are 2 n rows of 16 */
  return flx_rays_from_host(ctx, nullptr, 0u, [&]() -> flx_status {
    VolumeMaps dm;
    flx_status up = sh_up(ctx, sh, probes);
    if (up || (up = maps_up(ctx, has_map ? map : nullptr, maps, rows, &dm)) || (up = offsets_up(ctx, offsets, probes, &dm)) ||
        (up = flx_grow(ctx, flx_need(&ctx->d_query_rays, (size_t)n * 2u))))
      return up;
    float4 *planes = ctx->d_query_rays.get();
    FLX_HIP(ctx, hipMemcpyAsync(planes, positions, (size_t)flx_volume_plane_bytes(n), hipMemcpyHostToDevice, ctx->stream));
    FLX_HIP(ctx, hipMemcpyAsync(planes + n, normals, (size_t)flx_volume_plane_bytes(n), hipMemcpyHostToDevice, ctx->stream));
    return irradiance_run(ctx, grid, ctx->d_volume_sh.get(), planes, planes + n, n, ctx->d_query_hits.get(), dm, nullptr,
                          relocated ? "flx_volume_irradiance_relocated_device" : has_map ? "flx_volume_irradiance_map_device" : "flx_volume_irradiance_device");
  }, flx_down(&ctx->d_query_hits, (size_t)n, out));
}

extern "C" flx_status flx_volume_irradiance(flx_context *ctx, const flx_volume_grid *grid, const float *sh, const float *positions, const float *normals, uint32_t n, float *out) {
  return irradiance_host(ctx, grid, sh, positions, normals, n, out, false, nullptr, nullptr, "flx_volume_irradiance");
}

extern "C" flx_status flx_volume_irradiance_map(flx_context *ctx, const flx_volume_grid *grid, const float *sh, const float *positions, const float *normals, uint32_t n, float *out,
                                                const flx_volume_map *map, const float *maps) {
  return irradiance_host(ctx, grid, sh, positions, normals, n, out, true, map, maps, "flx_volume_irradiance_map");
}

static flx_status rays_run(flx_context *ctx, int32_t texture_width, const flx_volume_grid *grid, const void *d_sh, const void *d_rays, uint32_t n, void *d_out, const VolumeMaps &maps,
                           void *producer_stream, const char *call) {
  static const uint32_t fields = FLX_SURFACE_POSITION | FLX_SURFACE_NORMAL;
  if (!ctx) return FLX_ERR_INVALID;
  /* the scene and texture_width in the surface call's words (n = 0: it looks at them and at nothing else), then the grid */
  uint32_t probes = 0, rows = 0;
  flx_status s = flx_rays_surface_device(ctx, texture_width, nullptr, 0u, fields, nullptr, nullptr);
  if (s || (s = volume_refusal(ctx, flx_volume_grid_check(grid, &probes), call)) || (s = maps_params_refused(ctx, maps, probes, &rows, call)) || n == 0u) return s;
  const VolumeArray arrays[3] = { { d_sh, flx_volume_sh_bytes(probes), "the SH rows are not nx * ny * nz rows of 144 bytes" },
                                  { d_rays, (uint64_t)n * FLX_RAY_ROW_BYTES, "the rays are not n rows of 32 bytes" },
                                  { d_out, flx_volume_plane_bytes(n), "the irradiance rows are not n rows of 16 bytes" } };
  if ((s = arrays_refused(ctx, arrays, 3, call)) || (s = maps_array_refused(ctx, maps, rows, arrays, 3, call)) || (s = offsets_array_refused(ctx, maps, probes, rows, arrays, 3, call))) return s;
  if ((s = flx_server_stop(ctx))) return s;
  const uint32_t slab = flx_trace_slab_rays(1u, ctx->trace_slab), most = n < slab ? n : slab;
  if ((s = flx_grow(ctx, flx_need(&ctx->d_volume_surface, (size_t)most * 2u)))) return s;
  if ((s = flx_wait_for_producer(ctx, producer_stream))) return s;
  uint32_t slabs = 0, groups = 0;
  for (uint64_t first = 0; first < n; first += slab) {
    const uint32_t m = (uint32_t)(n - first < slab ? n - first : slab);
    float4 *planes = ctx->d_volume_surface.get();
    if ((s = flx_rays_surface_device(ctx, texture_width, (const float4 *)d_rays + first * 2u, m, fields, planes, nullptr))) return s;
    if ((s = lookup_enqueue(ctx, *grid, (const float4 *)d_sh, planes, planes + m, m, (float4 *)d_out + first, maps))) return s;
    groups = flx_volume_groups(m);
    slabs++;
  }
  lookup_ran(ctx, *grid, probes, n, slabs, slab, 1u, groups);
  return FLX_OK;
}

extern "C" flx_status flx_rays_irradiance_device(flx_context *ctx, int32_t texture_width, const flx_volume_grid *grid, const void *d_sh, const void *d_rays, uint32_t n, void *d_out,
                                                 void *producer_stream) {
  return rays_run(ctx, texture_width, grid, d_sh, d_rays, n, d_out, VolumeMaps(), producer_stream, "flx_rays_irradiance_device");
}

extern "C" flx_status flx_rays_irradiance_map_device(flx_context *ctx, int32_t texture_width, const flx_volume_grid *grid, const void *d_sh, const void *d_rays, uint32_t n, void *d_out,
                                                     const flx_volume_map *map, const void *d_maps, void *producer_stream) {
  return rays_run(ctx, texture_width, grid, d_sh, d_rays, n, d_out, with_maps(map, d_maps), producer_stream, "flx_rays_irradiance_map_device");
}

static flx_status rays_host(flx_context *ctx, int32_t texture_width, const flx_volume_grid *grid, const float *sh, const float *rays, uint32_t n, float *out, bool has_map,
                            const flx_volume_map *map, const float *maps, const char *call, bool relocated = false, const float *offsets = nullptr) {
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t probes = 0, rows = 0;
  flx_status s = flx_rays_surface_device(ctx, texture_width, nullptr, 0u, FLX_SURFACE_POSITION | FLX_SURFACE_NORMAL, nullptr, nullptr);
  if (s || (s = volume_refusal(ctx, flx_volume_grid_check(grid, &probes), call)) || (has_map && (s = flx_volume_map_refused(ctx, map, probes, &rows, call))) || n == 0u) return s;
  if (!sh || !rays || !out || (relocated && !offsets)) return volume_refusal(ctx, FLX_VOLUME_NULL, call);
  if ((s = host_maps_refused(ctx, has_map, map, maps, probes, &rows, call))) return s;
  return flx_rays_from_host(ctx, rays, n, [&]() -> flx_status {
    VolumeMaps dm;
    flx_status up = sh_up(ctx, sh, probes);
    if (up || (up = maps_up(ctx, has_map ? map : nullptr, maps, rows, &dm)) || (up = offsets_up(ctx, offsets, probes, &dm))) return up;
    return rays_run(ctx, texture_width, grid, ctx->d_volume_sh.get(), ctx->d_query_rays.get(), n, ctx->d_query_hits.get(), dm, nullptr,
                    relocated ? "flx_rays_irradiance_relocated_device" : has_map ? "flx_rays_irradiance_map_device" : "flx_rays_irradiance_device");
  }, flx_down(&ctx->d_query_hits, (size_t)n, out));
}

extern "C" flx_status flx_rays_irradiance(flx_context *ctx, int32_t texture_width, const flx_volume_grid *grid, const float *sh, const float *rays, uint32_t n, float *out) {
  return rays_host(ctx, texture_width, grid, sh, rays, n, out, false, nullptr, nullptr, "flx_rays_irradiance");
}

extern "C" flx_status flx_rays_irradiance_map(flx_context *ctx, int32_t texture_width, const flx_volume_grid *grid, const float *sh, const float *rays, uint32_t n, float *out,
                                              const flx_volume_map *map, const float *maps) {
  return rays_host(ctx, texture_width, grid, sh, rays, n, out, true, map, maps, "flx_rays_irradiance_map");
}

/* what both frame calls refuse before they look at an array: the scene and the frame params in the surface call's words, then the grid */
static flx_status frame_refused(flx_context *ctx, const flx_frame_params *params, const flx_volume_grid *grid, uint32_t *probes, const char *call) {
  const flx_status s = flx_frame_surface_refused(ctx, params, FLX_SURFACE_POSITION | FLX_SURFACE_NORMAL, "flx_frame_surface_device");
  return s ? s : volume_refusal(ctx, flx_volume_grid_check(grid, probes), call);
}

static flx_status frame_run(flx_context *ctx, const flx_frame_params *params, const flx_volume_grid *grid, const void *d_sh, void *d_out, const VolumeMaps &maps, const char *call) {
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t probes = 0, rows = 0;
  flx_status s = frame_refused(ctx, params, grid, &probes, call);
  if (s || (s = maps_params_refused(ctx, maps, probes, &rows, call))) return s;
  const uint32_t n = params->width * params->height;          /* (fits: the surface call's check) */
  const VolumeArray arrays[2] = { { d_sh, flx_volume_sh_bytes(probes), "the SH rows are not nx * ny * nz rows of 144 bytes" },
                                  { d_out, flx_volume_plane_bytes(n), "the irradiance rows are not width * height rows of 16 bytes" } };
  if ((s = arrays_refused(ctx, arrays, 2, call)) || (s = maps_array_refused(ctx, maps, rows, arrays, 2, call)) || (s = offsets_array_refused(ctx, maps, probes, rows, arrays, 2, call))) return s;
  if ((s = flx_server_stop(ctx))) return s;
  if ((s = flx_grow(ctx, flx_need(&ctx->d_volume_surface, (size_t)n * 2u)))) return s;
  float4 *planes = ctx->d_volume_surface.get();
  if ((s = flx_frame_surface_device(ctx, params, FLX_SURFACE_POSITION | FLX_SURFACE_NORMAL, planes))) return s;
  if ((s = lookup_enqueue(ctx, *grid, (const float4 *)d_sh, planes, planes + n, n, (float4 *)d_out, maps))) return s;
  lookup_ran(ctx, *grid, probes, n, 1u, n, 2u, flx_volume_groups(n));
  return FLX_OK;
}

extern "C" flx_status flx_frame_irradiance_device(flx_context *ctx, const flx_frame_params *params, const flx_volume_grid *grid, const void *d_sh, void *d_out) {
  return frame_run(ctx, params, grid, d_sh, d_out, VolumeMaps(), "flx_frame_irradiance_device");
}

extern "C" flx_status flx_frame_irradiance_map_device(flx_context *ctx, const flx_frame_params *params, const flx_volume_grid *grid, const void *d_sh, void *d_out,
                                                      const flx_volume_map *map, const void *d_maps) {
  return frame_run(ctx, params, grid, d_sh, d_out, with_maps(map, d_maps), "flx_frame_irradiance_map_device");
}

static flx_status frame_host(flx_context *ctx, const flx_frame_params *params, const flx_volume_grid *grid, const float *sh, float *out, bool has_map, const flx_volume_map *map,
                             const float *maps, const char *call, bool relocated = false, const float *offsets = nullptr) {
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t probes = 0, rows = 0;
  flx_status s = frame_refused(ctx, params, grid, &probes, call);
  if (s) return s;
  if (!sh || !out || (relocated && !offsets)) return volume_refusal(ctx, FLX_VOLUME_NULL, call);
  if ((s = host_maps_refused(ctx, has_map, map, maps, probes, &rows, call))) return s;
  return flx_rays_from_host(ctx, nullptr, 0u, [&]() -> flx_status {
    VolumeMaps dm;
    flx_status up = sh_up(ctx, sh, probes);
    if (up || (up = maps_up(ctx, has_map ? map : nullptr, maps, rows, &dm)) || (up = offsets_up(ctx, offsets, probes, &dm))) return up;
    return frame_run(ctx, params, grid, ctx->d_volume_sh.get(), ctx->d_query_hits.get(), dm,
                     relocated ? "flx_frame_irradiance_relocated_device" : has_map ? "flx_frame_irradiance_map_device" : "flx_frame_irradiance_device");
  }, flx_down(&ctx->d_query_hits, (size_t)params->width * params->height, out));
}

extern "C" flx_status flx_frame_irradiance(flx_context *ctx, const flx_frame_params *params, const flx_volume_grid *grid, const float *sh, float *out) {
  return frame_host(ctx, params, grid, sh, out, false, nullptr, nullptr, "flx_frame_irradiance");
}

extern "C" flx_status flx_frame_irradiance_map(flx_context *ctx, const flx_frame_params *params, const flx_volume_grid *grid, const float *sh, float *out, const flx_volume_map *map,
                                               const float *maps) {
  return frame_host(ctx, params, grid, sh, out, true, map, maps, "flx_frame_irradiance_map");
}

/* THE RELOCATED LOOKUPS: the same implementations once more, entered with offset rows (and with a map where either of map and maps is given). */
extern "C" flx_status flx_volume_irradiance_relocated_device(flx_context *ctx, const flx_volume_grid *grid, const void *d_sh, const void *d_positions, const void *d_normals, uint32_t n,
                                                             void *d_out, const flx_volume_map *map, const void *d_maps, const void *d_offsets, void *producer_stream) {
  return irradiance_run(ctx, grid, d_sh, d_positions, d_normals, n, d_out, with_offsets(map, d_maps, d_offsets), producer_stream, "flx_volume_irradiance_relocated_device");
}

extern "C" flx_status flx_volume_irradiance_relocated(flx_context *ctx, const flx_volume_grid *grid, const float *sh, const float *positions, const float *normals, uint32_t n, float *out,
                                                      const flx_volume_map *map, const float *maps, const float *offsets) {
  return irradiance_host(ctx, grid, sh, positions, normals, n, out, map || maps, map, maps, "flx_volume_irradiance_relocated", true, offsets);
}

extern "C" flx_status flx_rays_irradiance_relocated_device(flx_context *ctx, int32_t texture_width, const flx_volume_grid *grid, const void *d_sh, const void *d_rays, uint32_t n,
                                                           void *d_out, const flx_volume_map *map, const void *d_maps, const void *d_offsets, void *producer_stream) {
  return rays_run(ctx, texture_width, grid, d_sh, d_rays, n, d_out, with_offsets(map, d_maps, d_offsets), producer_stream, "flx_rays_irradiance_relocated_device");
}

extern "C" flx_status flx_rays_irradiance_relocated(flx_context *ctx, int32_t texture_width, const flx_volume_grid *grid, const float *sh, const float *rays, uint32_t n, float *out,
                                                    const flx_volume_map *map, const float *maps, const float *offsets) {
  return rays_host(ctx, texture_width, grid, sh, rays, n, out, map || maps, map, maps, "flx_rays_irradiance_relocated", true, offsets);
}

extern "C" flx_status flx_frame_irradiance_relocated_device(flx_context *ctx, const flx_frame_params *params, const flx_volume_grid *grid, const void *d_sh, void *d_out,
                                                            const flx_volume_map *map, const void *d_maps, const void *d_offsets) {
  return frame_run(ctx, params, grid, d_sh, d_out, with_offsets(map, d_maps, d_offsets), "flx_frame_irradiance_relocated_device");
}

extern "C" flx_status flx_frame_irradiance_relocated(flx_context *ctx, const flx_frame_params *params, const flx_volume_grid *grid, const float *sh, float *out, const flx_volume_map *map,
                                                     const float *maps, const float *offsets) {
  return frame_host(ctx, params, grid, sh, out, map || maps, map, maps, "flx_frame_irradiance_relocated", true, offsets);
}

extern "C" void flx_volume_irradiance_relocated_of(const flx_volume_grid *grid, const flx_volume_map *map, const float *sh_rows, const float *map_rows, const float *offset_rows,
                                                   const float position[4], const float normal[4], float out[4]) {
  flx_volume_relocate_lookup(grid, map, sh_rows, map_rows, offset_rows, position, normal, out);
}

extern "C" void flx_volume_irradiance_of(const flx_volume_grid *grid, const float *sh_rows, const float position[4], const float normal[4], float out[4]) {
  flx_volume_lookup(grid, sh_rows, position, normal, out);
}

extern "C" void flx_volume_irradiance_map_of(const flx_volume_grid *grid, const flx_volume_map *map, const float *sh_rows, const float *map_rows, const float position[4],
                                             const float normal[4], float out[4]) {
  flx_volume_map_lookup(grid, map, sh_rows, map_rows, position, normal, out);
}

extern "C" flx_status flx_debug_last_volume(flx_context *ctx, uint32_t out[8]) {
  if (!ctx || !out) return FLX_ERR_INVALID;
  const flx_context::VolumeLaunch &v = ctx->last_volume;
  out[0] = v.n; out[1] = v.slabs; out[2] = v.slab; out[3] = v.probes; out[4] = v.flags; out[5] = v.source; out[6] = v.groups; out[7] = 0u;
  return FLX_OK;
}
