/* flx_probes.hip — light probes on the device (include/flexlight_hip_debug.h, "light probes": flx_probe_rays[_device], flx_probe_reduce[_device],
 * flx_probes_sh[_device], flx_probe_irradiance).  The arithmetic is include/flx_probe.h's, the text the tests' CPU reference compiles too: ray rows and SH rows are
 * defined bit for bit.
 *
 * k_probe_rays: ONE LANE PER RAY, k_camera_rays' shape.  The grid's y names the probe, whose position is one uniform 16-byte load; a lane writes its 32-byte row as
 * two 16-byte vector stores, consecutive lanes consecutive rows.  Where w w is a multiple of 256 a workgroup lies within one face and the cube-face switch is a
 * scalar branch; elsewhere the face is the lane's own and the switch becomes selects.  No loads but the position either way.
 *
 * k_probe_sh: ONE WAVE PER PROBE, four probes a workgroup; THE 64 SLOTS OF flx_probe.h's SUMS ARE THE LANES.  Lane j reads the radiance rows of its texels j, j + 64,
 * .. as two 16-byte loads (a wave's load covers 2 KB without a gap; of the second half only the distance is used and the compiler narrows that load), recomputes direction and weight from t with the header — no ray row is read —, adds the 31 terms
 * onto its 31 registers in ascending t, and the six steps of the xor tree are six __shfl_xor per sum, in the header's order.  Lane 0 stores the row.  No LDS, no
 * atomics, no scratch (make resources).  A wave without a probe (the last workgroup) leaves at once; a lane without a texel (R < 64) keeps its zeros.
 *
 * flx_probes_sh_device cuts the probes into chunks of at most 2^21 rays and runs, per chunk and on the context's stream, k_probe_rays into ctx->d_probe_rays,
 * flx_rays_trace_ordered_device from there into ctx->d_probe_radiance — there is no second trace implementation — and k_probe_sh into the chunk's rows of the
 * output.  flx_probes_sh_map_device is the same loop — the same function — with k_probe_map (flx_volume_map.hip) enqueued beside k_probe_sh on each chunk's radiance.
 * The host-memory calls are the ray-batch calls' shared path (flx_rays_host.h). */
#include <string>

#include "flx_context.h"
#include "flx_probe.h"
#include "flx_probe_args.h"
#include "flx_rays_host.h"
#include "flx_volume_map_host.h"

namespace flx {

constexpr uint32_t PROBE_THREADS = 256u;
constexpr uint32_t PROBE_LAUNCH = 32768u;            /* probes a launch of k_probe_rays names with its grid's y */

/* positions: the launch's first probe's row; rays: its first ray row.  t = blockIdx.x * 256 + threadIdx.x < 2^19 + 256.  face_uniform: w w is a multiple of 256. */
__global__ __launch_bounds__(PROBE_THREADS) void k_probe_rays(const float4 *__restrict__ positions, float4 *__restrict__ rays, flx_probe_grid g, uint32_t face_uniform) {
  const uint32_t t = blockIdx.x * PROBE_THREADS + threadIdx.x;
  if (t >= g.rays) return;
  const float4 p = positions[blockIdx.y];
  const float position[3] = { p.x, p.y, p.z };
  uint32_t face, row, px;
  flx_probe_texel(&g, t, &face, &row, &px);
  if (face_uniform) face = (uint32_t)__builtin_amdgcn_readfirstlane((int)face);
  const flx_camera_row r = flx_probe_ray_at(position, &g, t, face, row, px);
  float4 *o = rays + ((size_t)blockIdx.y * g.rays + t) * 2u;
  o[0] = make_float4(r.ox, r.oy, r.oz, r.noise_x);
  o[1] = make_float4(r.dx, r.dy, r.dz, r.noise_y);
}

/* radiance: n_probes * g.rays rows of two float4; sh: n_probes rows of nine float4 */
__global__ __launch_bounds__(PROBE_THREADS) void k_probe_sh(const float4 *__restrict__ radiance, float4 *__restrict__ sh, flx_probe_grid g, float sky0, float sky1, float sky2,
                                                            uint32_t n_probes) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t probe = blockIdx.x * 4u + (threadIdx.x >> 6);      /* (blockIdx.x <= (n_probes - 1) / 4: no wrap) */
  if (probe >= n_probes) return;                                      /* the whole wave: nothing below waits for another wave */
  const float sky[3] = { sky0, sky1, sky2 };
  const float4 *rows = radiance + (size_t)probe * g.rays * 2u;
  float sum[FLX_PROBE_SUMS];
#pragma unroll
  for (uint32_t k = 0; k < FLX_PROBE_SUMS; k++) sum[k] = 0.0f;
  for (uint32_t t = lane; t < g.rays; t += FLX_PROBE_SLOTS) {
    const float4 a = rows[(size_t)t * 2u], b = rows[(size_t)t * 2u + 1u];
    const float row0[4] = { a.x, a.y, a.z, a.w }, row1[4] = { b.x, b.y, b.z, b.w };
    float term[FLX_PROBE_SUMS];
    flx_probe_texel_terms(&g, t, row0, row1, sky, term);
#pragma unroll
    for (uint32_t k = 0; k < FLX_PROBE_SUMS; k++) sum[k] = sum[k] + term[k];
  }
  /* all 64 lanes are here again; v[j] + v[j ^ off], off = 1, 2, 4, 8, 16, 32 */
#pragma unroll
  for (uint32_t off = 1u; off < FLX_PROBE_SLOTS; off <<= 1) {
#pragma unroll
    for (uint32_t k = 0; k < FLX_PROBE_SUMS; k++) sum[k] = sum[k] + __shfl_xor(sum[k], (int)off, 64);
  }
  if (lane != 0u) return;
  float row[FLX_PROBE_SH_WORDS];
  flx_probe_pack(sum, row);
  float4 *o = sh + (size_t)probe * 9u;
#pragma unroll
  for (uint32_t i = 0; i < 9u; i++) o[i] = make_float4(row[4u * i], row[4u * i + 1u], row[4u * i + 2u], row[4u * i + 3u]);
}

}  // namespace flx

using namespace flx;

/* ---- the calls ------------------------------------------------------------------------------------------------------------------------------------- */

static flx_status fail(flx_context *ctx, flx_status code, const std::string &msg) { return flx_fail(ctx, code, msg.c_str()); }

/* a refusal of flx_probe_args.h in words */
static flx_status probe_refusal(flx_context *ctx, enum flx_probe_refusal why, const char *call) {
  const char *what = "";
  switch (why) {
    case FLX_PROBE_ARGS_OK: return FLX_OK;
    case FLX_PROBE_PARAMS_NULL: what = "the probe params are NULL"; break;
    case FLX_PROBE_FACE_SIZE: what = "face_size is not one of 1 .. 256"; break;
    case FLX_PROBE_ORDER: what = "order has a bit beyond FLX_TRACE_ORDER_HITS"; break;
    case FLX_PROBE_NOT_FINITE: what = "sky or reserved holds a value that is not finite"; break;
    case FLX_PROBE_RAYS: what = "n_probes * 6 * face_size * face_size is 2^32 or more"; break;
    case FLX_PROBE_NULL: what = "an array is NULL"; break;
    case FLX_PROBE_WRAPS: what = "an array leaves the address space"; break;
    case FLX_PROBE_OVERLAP: what = "the arrays overlap"; break;
  }
  return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": " + what);
}

static enum flx_probe_refusal params_check(const flx_probe_params *p) {
  return flx_probe_params_check(p != nullptr, p ? p->face_size : 0u, p ? p->order : 0u, p ? p->sky : nullptr, p ? p->reserved : 0.0f);
}

/* Two arrays of a device call: there, inside 64 bits, memory of the context's device, and apart — in that order.  a_what, b_what: what the arrays are, for the
 * message. */
static flx_status arrays_refused(flx_context *ctx, const void *a, uint64_t a_bytes, const char *a_what, const void *b, uint64_t b_bytes, const char *b_what, const char *call) {
  const enum flx_probe_refusal why = flx_probe_arrays_check((uint64_t)(uintptr_t)a, a_bytes, (uint64_t)(uintptr_t)b, b_bytes);
  if (why != FLX_PROBE_ARGS_OK && why != FLX_PROBE_OVERLAP) return probe_refusal(ctx, why, call);      /* (overlap: said after the pointers are known to be the device's) */
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  if (!flx_rows_on_device(ctx, a, (size_t)a_bytes)) return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": " + a_what + " in memory of the context's device, 16-byte aligned");
  if (!flx_rows_on_device(ctx, b, (size_t)b_bytes)) return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": " + b_what + " in memory of the context's device, 16-byte aligned");
  return probe_refusal(ctx, why, call);
}

/* the launches of k_probe_rays for n probes, PROBE_LAUNCH of them a launch */
static flx_status rays_enqueue(flx_context *ctx, const float4 *d_positions, uint32_t n, const flx_probe_grid &g, float4 *d_rays) {
  const uint32_t groups = (g.rays + PROBE_THREADS - 1u) / PROBE_THREADS;
  const uint32_t face_uniform = (g.w * g.w) % PROBE_THREADS == 0u ? 1u : 0u;
  for (uint32_t first = 0; first < n; first += PROBE_LAUNCH) {
    const uint32_t m = n - first < PROBE_LAUNCH ? n - first : PROBE_LAUNCH;
    hipLaunchKernelGGL(k_probe_rays, dim3(groups, m), dim3(PROBE_THREADS), 0, ctx->stream, d_positions + first, d_rays + (size_t)first * g.rays * 2u, g, face_uniform);
    FLX_HIP(ctx, hipGetLastError());
  }
  return FLX_OK;
}

static flx_status reduce_enqueue(flx_context *ctx, const float4 *d_radiance, uint32_t n, const flx_probe_grid &g, const float sky[3], float4 *d_sh) {
  hipLaunchKernelGGL(k_probe_sh, dim3(flx_probe_reduce_groups(n)), dim3(PROBE_THREADS), 0, ctx->stream, d_radiance, d_sh, g, sky[0], sky[1], sky[2], n);
  FLX_HIP(ctx, hipGetLastError());
  return FLX_OK;
}

extern "C" flx_status flx_probe_rays_device(flx_context *ctx, const void *d_positions, uint32_t n_probes, uint32_t face_size, void *d_rays, void *producer_stream) {
  static const char *const call = "flx_probe_rays_device";
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t rays = 0;
  flx_status s = probe_refusal(ctx, flx_probe_face_check(face_size), call);
  if (s || (s = probe_refusal(ctx, flx_probe_count_check(n_probes, face_size, &rays), call)) || n_probes == 0u) return s;
  if ((s = arrays_refused(ctx, d_positions, (uint64_t)n_probes * FLX_PROBE_POSITION_BYTES, "the positions are not n_probes rows of 16 bytes", d_rays,
                          (uint64_t)rays * FLX_RAY_ROW_BYTES, "the rays are not n_probes * 6 * face_size * face_size rows", call)))
    return s;
  if ((s = flx_server_stop(ctx)) || (s = flx_wait_for_producer(ctx, producer_stream))) return s;
  return rays_enqueue(ctx, (const float4 *)d_positions, n_probes, flx_probe_grid_of(face_size), (float4 *)d_rays);
}

/* the positions of a host variant into ctx->d_probe_positions, on the context's stream */
static flx_status positions_up(flx_context *ctx, const float *positions, uint32_t n) {
  flx_status s = flx_grow(ctx, flx_need(&ctx->d_probe_positions, n));
  if (s) return s;
  FLX_HIP(ctx, hipMemcpyAsync(ctx->d_probe_positions.get(), positions, (size_t)n * FLX_PROBE_POSITION_BYTES, hipMemcpyHostToDevice, ctx->stream));
  return FLX_OK;
}

extern "C" flx_status flx_probe_rays(flx_context *ctx, const float *positions, uint32_t n_probes, uint32_t face_size, float *rays) {
  static const char *const call = "flx_probe_rays";
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t count = 0;
  flx_status s = probe_refusal(ctx, flx_probe_face_check(face_size), call);
  if (s || (s = probe_refusal(ctx, flx_probe_count_check(n_probes, face_size, &count), call)) || n_probes == 0u) return s;
  if (!positions || !rays) return probe_refusal(ctx, FLX_PROBE_NULL, call);
  return flx_rays_from_host(ctx, nullptr, 0u, [&]() {
    flx_status up = positions_up(ctx, positions, n_probes);
    return up ? up : flx_probe_rays_device(ctx, ctx->d_probe_positions.get(), n_probes, face_size, ctx->d_query_hits.get(), nullptr);
  }, flx_down(&ctx->d_query_hits, (size_t)count * 2u, rays));
}

extern "C" flx_status flx_probe_reduce_device(flx_context *ctx, const void *d_radiance, uint32_t n_probes, const flx_probe_params *params, void *d_sh, void *producer_stream) {
  static const char *const call = "flx_probe_reduce_device";
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t rays = 0;
  flx_status s = probe_refusal(ctx, params_check(params), call);
  if (s || (s = probe_refusal(ctx, flx_probe_count_check(n_probes, params->face_size, &rays), call)) || n_probes == 0u) return s;
  if ((s = arrays_refused(ctx, d_radiance, (uint64_t)rays * FLX_RAY_ROW_BYTES, "the radiance is not n_probes * 6 * face_size * face_size rows", d_sh,
                          (uint64_t)n_probes * FLX_PROBE_SH_BYTES, "the SH rows are not n_probes rows of 144 bytes", call)))
    return s;
  if ((s = flx_server_stop(ctx)) || (s = flx_wait_for_producer(ctx, producer_stream))) return s;
  return reduce_enqueue(ctx, (const float4 *)d_radiance, n_probes, flx_probe_grid_of(params->face_size), params->sky, (float4 *)d_sh);
}

extern "C" flx_status flx_probe_reduce(flx_context *ctx, const void *radiance, uint32_t n_probes, const flx_probe_params *params, float *sh) {
  static const char *const call = "flx_probe_reduce";
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t rays = 0;
  flx_status s = probe_refusal(ctx, params_check(params), call);
  if (s || (s = probe_refusal(ctx, flx_probe_count_check(n_probes, params->face_size, &rays), call)) || n_probes == 0u) return s;
  if (!radiance || !sh) return probe_refusal(ctx, FLX_PROBE_NULL, call);
  /* the radiance rows go up where a ray batch's rays go: rows of 32 bytes both */
  return flx_rays_from_host(ctx, (const float *)radiance, rays, [&]() { return flx_probe_reduce_device(ctx, ctx->d_query_rays.get(), n_probes, params, ctx->d_query_hits.get(), nullptr); },
                            flx_down(&ctx->d_query_hits, (size_t)n_probes * 9u, sh));
}

/* what both flx_probes_sh calls refuse before they look at an array: the scene and the trace params, asked of the trace call in its words (n = 0: it looks at
 * them and at nothing else, and enqueues nothing), then the probe params */
static flx_status probes_refused(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const char *call) {
  flx_status s = flx_rays_trace_ordered_device(ctx, trace, nullptr, nullptr, 0u, 0u, nullptr);
  return s ? s : probe_refusal(ctx, params_check(params), call);
}

/* flx_probes_sh_device and flx_probes_sh_map_device: ONE LOOP.  has_map: k_probe_map is enqueued beside k_probe_sh on each chunk's radiance (flx_volume_map.hip),
 * into the chunk's rows of d_maps; the map's refusals are asked after the siblings' own. */
static flx_status probes_sh_run(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, bool has_map, const flx_volume_map *map, const void *d_positions,
                                uint32_t n_probes, void *d_sh, void *d_maps, void *producer_stream, const char *call) {
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t map_rows = 0;
  flx_status s = probes_refused(ctx, trace, params, call);
  if (s || (has_map && (s = flx_volume_map_refused(ctx, map, n_probes, &map_rows, call))) || n_probes == 0u) return s;
  if ((s = arrays_refused(ctx, d_positions, (uint64_t)n_probes * FLX_PROBE_POSITION_BYTES, "the positions are not n_probes rows of 16 bytes", d_sh,
                          (uint64_t)n_probes * FLX_PROBE_SH_BYTES, "the SH rows are not n_probes rows of 144 bytes", call)))
    return s;
  if (has_map) {
    const flx_map_other others[2] = { { d_positions, (uint64_t)n_probes * FLX_PROBE_POSITION_BYTES }, { d_sh, (uint64_t)n_probes * FLX_PROBE_SH_BYTES } };
    if ((s = flx_volume_maps_refused(ctx, d_maps, map_rows, others, 2, call))) return s;
  }
  const flx_probe_grid g = flx_probe_grid_of(params->face_size);
  const uint32_t chunk = flx_probe_chunk(params->face_size, ctx->probe_chunk);
  const uint32_t most = n_probes < chunk ? n_probes : chunk;
  if ((s = flx_server_stop(ctx))) return s;
  /* (an earlier call's chunk may still read the buffers that are about to go: flx_grow waits first) */
  if ((s = flx_grow(ctx, flx_need(&ctx->d_probe_rays, (size_t)most * g.rays * 2u), flx_need(&ctx->d_probe_radiance, (size_t)most * g.rays * 2u)))) return s;
  if ((s = flx_wait_for_producer(ctx, producer_stream))) return s;
  uint32_t chunks = 0, groups = 0;
  for (uint32_t first = 0; first < n_probes; first += chunk) {
    const uint32_t m = n_probes - first < chunk ? n_probes - first : chunk;
    if ((s = rays_enqueue(ctx, (const float4 *)d_positions + first, m, g, ctx->d_probe_rays.get()))) return s;
    if ((s = flx_rays_trace_ordered_device(ctx, trace, ctx->d_probe_rays.get(), ctx->d_probe_radiance.get(), m * g.rays, params->order, nullptr))) return s;
    if ((s = reduce_enqueue(ctx, ctx->d_probe_radiance.get(), m, g, params->sky, (float4 *)d_sh + (size_t)first * 9u))) return s;
    if (has_map && (s = flx_probe_map_enqueue(ctx, ctx->d_probe_radiance.get(), m, g, *map, (float4 *)d_maps + (size_t)first * (map->size * map->size), n_probes))) return s;
    groups = flx_probe_reduce_groups(m);
    chunks++;
    if (n_probes - first <= chunk) break;                   /* (first + chunk could wrap) */
  }
  flx_context::ProbeLaunch ran;
  ran.chunks = chunks; ran.chunk = chunk; ran.face_size = params->face_size; ran.n = n_probes; ran.order = params->order; ran.rays = g.rays; ran.reduce_groups = groups;
  ctx->last_probes = ran;
  return FLX_OK;
}

extern "C" flx_status flx_probes_sh_device(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const void *d_positions, uint32_t n_probes, void *d_sh,
                                           void *producer_stream) {
  return probes_sh_run(ctx, trace, params, false, nullptr, d_positions, n_probes, d_sh, nullptr, producer_stream, "flx_probes_sh_device");
}

extern "C" flx_status flx_probes_sh_map_device(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_map *map, const void *d_positions,
                                               uint32_t n_probes, void *d_sh, void *d_maps, void *producer_stream) {
  return probes_sh_run(ctx, trace, params, true, map, d_positions, n_probes, d_sh, d_maps, producer_stream, "flx_probes_sh_map_device");
}

extern "C" flx_status flx_probes_sh_map(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_map *map, const float *positions,
                                        uint32_t n_probes, float *sh, float *maps) {
  static const char *const call = "flx_probes_sh_map";
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t map_rows = 0;
  flx_status s = probes_refused(ctx, trace, params, call);
  if (s || (s = flx_volume_map_refused(ctx, map, n_probes, &map_rows, call)) || n_probes == 0u) return s;
  if (!positions || !sh) return probe_refusal(ctx, FLX_PROBE_NULL, call);
  if (!maps) return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": the maps array is NULL");
  return flx_rays_from_host(ctx, nullptr, 0u, [&]() {
    flx_status up = positions_up(ctx, positions, n_probes);
    return up ? up : flx_probes_sh_map_device(ctx, trace, params, map, ctx->d_probe_positions.get(), n_probes, ctx->d_query_hits.get(), ctx->d_volume_maps.get(), nullptr);
  }, flx_down(&ctx->d_query_hits, (size_t)n_probes * 9u, sh), flx_down(&ctx->d_volume_maps, (size_t)map_rows, maps));
}

extern "C" flx_status flx_probes_sh(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const float *positions, uint32_t n_probes, float *sh) {
  static const char *const call = "flx_probes_sh";
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = probes_refused(ctx, trace, params, call);
  if (s || n_probes == 0u) return s;
  if (!positions || !sh) return probe_refusal(ctx, FLX_PROBE_NULL, call);
  return flx_rays_from_host(ctx, nullptr, 0u, [&]() {
    flx_status up = positions_up(ctx, positions, n_probes);
    return up ? up : flx_probes_sh_device(ctx, trace, params, ctx->d_probe_positions.get(), n_probes, ctx->d_query_hits.get(), nullptr);
  }, flx_down(&ctx->d_query_hits, (size_t)n_probes * 9u, sh));
}

extern "C" void flx_probe_irradiance(const float sh[36], const float n[3], float out[3]) { flx_probe_irradiance_of(sh, n, out); }

extern "C" flx_status flx_debug_set_probe_chunk(flx_context *ctx, uint32_t probes) {
  if (!ctx) return FLX_ERR_INVALID;
  ctx->probe_chunk = probes;
  return FLX_OK;
}

extern "C" flx_status flx_debug_last_probes(flx_context *ctx, uint32_t out[8]) {
  if (!ctx || !out) return FLX_ERR_INVALID;
  const flx_context::ProbeLaunch &p = ctx->last_probes;
  out[0] = p.chunks; out[1] = p.chunk; out[2] = p.face_size; out[3] = p.n; out[4] = p.order; out[5] = p.rays; out[6] = p.reduce_groups; out[7] = 0u;
  return FLX_OK;
}
