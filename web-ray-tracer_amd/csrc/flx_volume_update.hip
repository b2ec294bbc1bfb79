/* flx_volume_update.hip — probe volumes updated over time (include/flexlight_hip_debug.h, "volume updates": flx_volume_positions_list[_device],
 * flx_volume_blend[_device], flx_volume_update[_device], flx_volume_blend_row_of, flx_debug_last_volume_update).  The arithmetic is include/flx_volume_update.h's,
 * the text the tests' CPU reference compiles too: position rows, blended rows and states are defined bit for bit.
 *
 * k_volume_positions_list: ONE LANE PER ENTRY; a lane reads its index as one 4-byte load where a list is given — none otherwise: first + j stride in 64 bits — and
 * writes its 16-byte row, consecutive lanes consecutive rows.
 *
 * k_volume_blend: ONE WAVE PER ENTRY, four entries a workgroup (k_probe_sh's shape).  The entry, hence the probe, is wave-uniform (readfirstlane): the index is one
 * scalar load and every branch on the state is a scalar branch.  Lanes 0 .. 8 hold the nine float4 of the new and of the old SH row, one 16-byte load each; the
 * other lanes hold zeros, which are finite.  THE STATE is one ballot over "my new words are finite", one over "my old words are finite", and lane 0's old word 3.
 * A skipped entry leaves before any row is read; a kept one after its two rows.  Lanes 0 .. 8 store the SH row, 16 bytes each.  The map rows go lane j at rows j,
 * j + 64, ..: one pass for m <= 8, four at m = 16, two 16-byte loads and at most one 16-byte store a row (a row that keeps its bits is not stored).  Lane 0 stores the
 * state word where a state array is given.  It is a memory kernel: 288 + 32 m m bytes read and 144 + 16 m m written an entry.  No LDS, no atomics, no scratch
 * (make resources).  A wave without an entry (the last workgroup) leaves at once.
 *   THE LAUNCHES ARE NOT CUT: n_list is at most nx ny nz < 2^31, so ceil(n_list / 4) workgroups and ceil(n_list / 256) fit a one-dimensional grid.
 *   A PROBE NAMED TWICE by a list in device memory is blended by two waves in no order: one of the possible results, torn rows included.
 *
 * flx_volume_update_device is k_volume_positions_list into ctx->d_update_positions, flx_probes_sh_device (or flx_probes_sh_map_device) AS IT STANDS from there into
 * ctx->d_update_sh (and ctx->d_update_maps) — there is no second probe path — and k_volume_blend behind them on the context's stream.  The host-memory calls are the
 * ray-batch calls' shared path (flx_rays_host.h). */
#include <string>

#include "flx_context.h"
#include "flx_rays_host.h"
#include "flx_volume_args.h"
#include "flx_volume_map_host.h"
#include "flx_volume_update.h"
#include "flx_volume_update_args.h"

namespace flx {

constexpr uint32_t UPDATE_THREADS = FLX_VOLUME_UPDATE_THREADS;
static_assert(UPDATE_THREADS / 64u == FLX_VOLUME_UPDATE_WAVE_ENTRIES, "a wave an entry");

/* indices: n_list words, or nullptr for the arithmetic list; positions: n_list rows */
__global__ __launch_bounds__(UPDATE_THREADS) void k_volume_positions_list(const uint32_t *__restrict__ indices, float4 *__restrict__ positions, flx_volume_grid g,
                                                                          struct flx_volume_update u, uint32_t n_list) {
  const uint32_t j = blockIdx.x * UPDATE_THREADS + threadIdx.x;      /* (blockIdx.x <= (n_list - 1) / 256 and n_list < 2^31: no wrap) */
  if (j >= n_list) return;
  float row[4];
  flx_volume_update_position(&g, flx_volume_update_entry(&u, indices, j), row);
  positions[j] = make_float4(row[0], row[1], row[2], row[3]);
}

/* indices: as above; new_sh: n_list rows of nine float4; new_maps: n_list * bins rows; sh, maps: the grid's resident rows; state: n_list words, or nullptr.
 * bins == 0: no maps, and neither maps array is read. */
__global__ __launch_bounds__(UPDATE_THREADS) void k_volume_blend(const uint32_t *__restrict__ indices, const float4 *__restrict__ new_sh, const float4 *__restrict__ new_maps,
                                                                 float4 *__restrict__ sh, float4 *__restrict__ maps, uint32_t *__restrict__ state, flx_volume_grid g,
                                                                 struct flx_volume_update u, uint32_t bins, uint32_t n_list) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * FLX_VOLUME_UPDATE_WAVE_ENTRIES + (threadIdx.x >> 6)));      /* (blockIdx.x <= (n_list - 1) / 4: no wrap) */
  if (j >= n_list) return;                                            /* the whole wave: nothing below waits for another wave */
  const uint64_t index = flx_volume_update_entry(&u, indices, j);
  if (!flx_volume_update_in_grid(&g, index)) {
    if (state != nullptr && lane == 0u) state[j] = FLX_VOLUME_UPDATE_SKIPPED;
    return;
  }
  const uint32_t p = (uint32_t)index;
  float4 *row = sh + (size_t)p * 9u;
  float nw[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, old[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
  if (lane < 9u) {
    const float4 a = new_sh[(size_t)j * 9u + lane], b = row[lane];
    nw[0] = a.x; nw[1] = a.y; nw[2] = a.z; nw[3] = a.w;
    old[0] = b.x; old[1] = b.y; old[2] = b.z; old[3] = b.w;
  }
  /* all 64 lanes are here again */
  const int new_finite = __ballot(flx_volume_update_finite4(nw)) == ~0ull;
  const int old_finite = __ballot(flx_volume_update_finite4(old)) == ~0ull;
  const float old_word3 = flx_u2f((uint32_t)__builtin_amdgcn_readfirstlane((int)flx_f2u(old[3])));      /* lane 0's: word 3 of the row */
  const uint32_t s = flx_volume_update_state(1, new_finite, old_finite, old_word3, u.hysteresis);
  if (state != nullptr && lane == 0u) state[j] = s;
  if (s == FLX_VOLUME_UPDATE_KEPT) return;
  const float gain = flx_volume_update_gain(u.hysteresis);
  if (lane < 9u) {
    float out[4];
    flx_volume_update_sh4(s, old, nw, gain, out);
    row[lane] = make_float4(out[0], out[1], out[2], out[3]);
  }
  const float4 *fresh = new_maps + (size_t)j * bins;                  /* (below 2^31 rows each: the calls' check) */
  float4 *resident = maps + (size_t)p * bins;
  for (uint32_t r = lane; r < bins; r += 64u) {
    const float4 a = fresh[r], b = resident[r];
    const float n4[4] = { a.x, a.y, a.z, a.w }, o4[4] = { b.x, b.y, b.z, b.w };
    float out[4];
    if (flx_volume_update_map_row(s, o4, n4, gain, out)) resident[r] = make_float4(out[0], out[1], out[2], out[3]);
  }
}

}  // namespace flx

using namespace flx;

/* ---- the calls ------------------------------------------------------------------------------------------------------------------------------------- */

static flx_status fail(flx_context *ctx, flx_status code, const std::string &msg) { return flx_fail(ctx, code, msg.c_str()); }

/* a refusal of flx_volume_update_args.h in words */
static flx_status update_refusal(flx_context *ctx, enum flx_volume_update_refusal why, const char *call) {
  const char *what = "";
  switch (why) {
    case FLX_VOLUME_UPDATE_ARGS_OK: return FLX_OK;
    case FLX_VOLUME_UPDATE_NULL: what = "the update is NULL"; break;
    case FLX_VOLUME_UPDATE_HYSTERESIS: what = "hysteresis is not one of 0 .. 1"; break;
    case FLX_VOLUME_UPDATE_RESERVED: what = "the update's reserved word is not 0"; break;
    case FLX_VOLUME_UPDATE_COUNT: what = "n_list is above the grid's probes"; break;
    case FLX_VOLUME_UPDATE_STRIDE: what = "stride is 0 for a list of more than one entry"; break;
    case FLX_VOLUME_UPDATE_END: what = "first + (n_list - 1) * stride is not a probe of the grid"; break;
    case FLX_VOLUME_UPDATE_MAPS_ALONE: what = "maps are given without a map"; break;
    case FLX_VOLUME_UPDATE_MAP_ALONE: what = "a map is given without its maps"; break;
    case FLX_VOLUME_UPDATE_ARRAY_NULL: what = "an array is NULL"; break;
    case FLX_VOLUME_UPDATE_MISALIGNED: what = "an array is misaligned (16 bytes; 4 for indices and states)"; break;
    case FLX_VOLUME_UPDATE_WRAPS: what = "an array leaves the address space"; break;
    case FLX_VOLUME_UPDATE_OVERLAP: what = "the arrays overlap"; break;
    case FLX_VOLUME_UPDATE_DUPLICATE: what = "the list names a probe twice"; break;
  }
  return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": " + what);
}

/* an array of a device call: where it lies and what it is, for the message */
struct UpdateArray { const void *p; uint64_t bytes; uint32_t align; bool optional; const char *what; };

/* The k arrays of a device call: there, aligned, inside 64 bits, memory of the context's device, and apart — in that order. */
static flx_status arrays_refused(flx_context *ctx, const UpdateArray *arrays, int k, const char *call) {
  flx_update_array a[FLX_VOLUME_UPDATE_MAX_ARRAYS];
  for (int i = 0; i < k; i++) a[i] = { (uint64_t)(uintptr_t)arrays[i].p, arrays[i].bytes, arrays[i].align, arrays[i].optional ? 1 : 0 };
  const enum flx_volume_update_refusal why = flx_volume_update_arrays_check(a, k);
  if (why != FLX_VOLUME_UPDATE_ARGS_OK && why != FLX_VOLUME_UPDATE_OVERLAP) return update_refusal(ctx, why, call);      /* (overlap: said after the pointers are known to be the device's) */
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  for (int i = 0; i < k; i++) {
    if (flx_update_array_absent(a[i])) continue;
    const bool there = arrays[i].align == 16u ? flx_rows_on_device(ctx, arrays[i].p, (size_t)arrays[i].bytes) : flx_words_on_device(ctx, arrays[i].p, (size_t)arrays[i].bytes);
    if (!there) return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": " + arrays[i].what + " in memory of the context's device");
  }
  return update_refusal(ctx, why, call);
}

/* What every call decides before it looks at an array: the grid, the map where one is given, then the update and the list.  *probes, *bins (0 without a map),
 * *new_rows (n_list bins) and *rows (nx ny nz bins) of an accepted call. */
struct UpdateShape { uint32_t probes = 0, bins = 0, new_rows = 0, rows = 0; };
static flx_status shape_refused(flx_context *ctx, const flx_volume_grid *grid, const flx_volume_map *map, const struct flx_volume_update *update, bool has_list, uint32_t n_list,
                                UpdateShape *shape, const char *call) {
  flx_status s = flx_volume_grid_refused(ctx, grid, &shape->probes, call);
  if (s || (map && (s = flx_volume_map_refused(ctx, map, shape->probes, &shape->rows, call)))) return s;
  if ((s = update_refusal(ctx, flx_volume_update_check(update, has_list ? 1 : 0, n_list, shape->probes), call))) return s;
  shape->bins = map ? map->size * map->size : 0u;
  shape->new_rows = n_list * shape->bins;                              /* (n_list <= probes: at most `rows`) */
  return FLX_OK;
}

static void update_ran(flx_context *ctx, uint32_t n_list, const flx_volume_map *map, bool has_list, uint32_t chunks, uint32_t fused) {
  flx_context::VolumeUpdateLaunch ran;
  ran.entries = n_list; ran.groups = flx_volume_update_blend_groups(n_list); ran.size = map ? map->size : 0u; ran.listed = has_list ? 1u : 0u; ran.chunks = chunks; ran.fused = fused;
  ctx->last_volume_update = ran;
}

static flx_status positions_enqueue(flx_context *ctx, const flx_volume_grid &g, const struct flx_volume_update &u, const void *d_indices, uint32_t n_list, float4 *d_positions) {
  hipLaunchKernelGGL(k_volume_positions_list, dim3(flx_volume_update_position_groups(n_list)), dim3(UPDATE_THREADS), 0, ctx->stream, (const uint32_t *)d_indices, d_positions, g, u, n_list);
  FLX_HIP(ctx, hipGetLastError());
  return FLX_OK;
}

static flx_status blend_enqueue(flx_context *ctx, const flx_volume_grid &g, const struct flx_volume_update &u, uint32_t bins, const void *d_indices, uint32_t n_list, const void *d_new_sh,
                                const void *d_new_maps, void *d_sh, void *d_maps, void *d_state) {
  hipLaunchKernelGGL(k_volume_blend, dim3(flx_volume_update_blend_groups(n_list)), dim3(UPDATE_THREADS), 0, ctx->stream, (const uint32_t *)d_indices, (const float4 *)d_new_sh,
                     (const float4 *)d_new_maps, (float4 *)d_sh, (float4 *)d_maps, (uint32_t *)d_state, g, u, bins, n_list);
  FLX_HIP(ctx, hipGetLastError());
  return FLX_OK;
}

static const char *const INDICES_WHAT = "the indices are not n_list words of 4 bytes";
static const char *const STATE_WHAT = "the states are not n_list words of 4 bytes";
static const char *const SH_WHAT = "the SH rows are not nx * ny * nz rows of 144 bytes";
static const char *const MAPS_WHAT = "the maps are not nx * ny * nz * size * size rows of 16 bytes";

extern "C" flx_status flx_volume_positions_list_device(flx_context *ctx, const flx_volume_grid *grid, const struct flx_volume_update *update, const void *d_indices, uint32_t n_list,
                                                       void *d_positions, void *producer_stream) {
  static const char *const call = "flx_volume_positions_list_device";
  if (!ctx) return FLX_ERR_INVALID;
  UpdateShape shape;
  flx_status s = shape_refused(ctx, grid, nullptr, update, d_indices != nullptr, n_list, &shape, call);
  if (s || n_list == 0u) return s;
  const UpdateArray arrays[2] = { { d_indices, flx_volume_update_word_bytes(n_list), 4u, true, INDICES_WHAT },
                                  { d_positions, flx_volume_update_position_bytes(n_list), 16u, false, "the positions are not n_list rows of 16 bytes" } };
  if ((s = arrays_refused(ctx, arrays, 2, call))) return s;
  if ((s = flx_server_stop(ctx)) || (s = flx_wait_for_producer(ctx, producer_stream))) return s;
  return positions_enqueue(ctx, *grid, *update, d_indices, n_list, (float4 *)d_positions);
}

/* what the host variants ask of a list they can look at, behind the update's own rules */
static flx_status host_list_refused(flx_context *ctx, const uint32_t *indices, uint32_t n_list, uint32_t probes, const char *call) {
  return indices && flx_volume_update_duplicate(indices, n_list, probes) ? update_refusal(ctx, FLX_VOLUME_UPDATE_DUPLICATE, call) : FLX_OK;
}

/* the list of a host variant into ctx->d_update_indices, on the context's stream; -> the list on the device (nullptr for the arithmetic one) */
static flx_status indices_up(flx_context *ctx, const uint32_t *indices, uint32_t n_list, const void **d_indices) {
  *d_indices = nullptr;
  if (!indices) return FLX_OK;
  flx_status s = flx_grow(ctx, flx_need(&ctx->d_update_indices, (size_t)n_list));
  if (s) return s;
  FLX_HIP(ctx, hipMemcpyAsync(ctx->d_update_indices.get(), indices, (size_t)flx_volume_update_word_bytes(n_list), hipMemcpyHostToDevice, ctx->stream));
  *d_indices = ctx->d_update_indices.get();
  return FLX_OK;
}

extern "C" flx_status flx_volume_positions_list(flx_context *ctx, const flx_volume_grid *grid, const struct flx_volume_update *update, const uint32_t *indices, uint32_t n_list,
                                                float *positions) {
  static const char *const call = "flx_volume_positions_list";
  if (!ctx) return FLX_ERR_INVALID;
  UpdateShape shape;
  flx_status s = shape_refused(ctx, grid, nullptr, update, indices != nullptr, n_list, &shape, call);
  if (s || n_list == 0u) return s;
  if (!positions) return update_refusal(ctx, FLX_VOLUME_UPDATE_ARRAY_NULL, call);
  if ((s = host_list_refused(ctx, indices, n_list, shape.probes, call))) return s;
  return flx_rays_from_host(ctx, nullptr, 0u, [&]() -> flx_status {
    const void *d_indices = nullptr;
    flx_status up = indices_up(ctx, indices, n_list, &d_indices);
    return up ? up : flx_volume_positions_list_device(ctx, grid, update, d_indices, n_list, ctx->d_query_hits.get(), nullptr);
  }, flx_down(&ctx->d_query_hits, (size_t)n_list, positions));
}

extern "C" flx_status flx_volume_blend_device(flx_context *ctx, const flx_volume_grid *grid, const flx_volume_map *map, const struct flx_volume_update *update, const void *d_indices,
                                              uint32_t n_list, const void *d_new_sh, const void *d_new_maps, void *d_sh, void *d_maps, void *d_state, void *producer_stream) {
  static const char *const call = "flx_volume_blend_device";
  if (!ctx) return FLX_ERR_INVALID;
  UpdateShape shape;
  flx_status s = shape_refused(ctx, grid, map, update, d_indices != nullptr, n_list, &shape, call);
  if (s || (s = update_refusal(ctx, flx_volume_update_pairing(map != nullptr, d_new_maps != nullptr || d_maps != nullptr, d_new_maps != nullptr && d_maps != nullptr), call)) || n_list == 0u)
    return s;
  const bool no_map = map == nullptr;
  const UpdateArray arrays[6] = { { d_indices, flx_volume_update_word_bytes(n_list), 4u, true, INDICES_WHAT },
                                  { d_new_sh, flx_volume_update_sh_bytes(n_list), 16u, false, "the new SH rows are not n_list rows of 144 bytes" },
                                  { d_new_maps, flx_volume_map_bytes(shape.new_rows), 16u, no_map, "the new maps are not n_list * size * size rows of 16 bytes" },
                                  { d_sh, flx_volume_update_sh_bytes(shape.probes), 16u, false, SH_WHAT },
                                  { d_maps, flx_volume_map_bytes(shape.rows), 16u, no_map, MAPS_WHAT },
                                  { d_state, flx_volume_update_word_bytes(n_list), 4u, true, STATE_WHAT } };
  if ((s = arrays_refused(ctx, arrays, 6, call))) return s;
  if ((s = flx_server_stop(ctx)) || (s = flx_wait_for_producer(ctx, producer_stream))) return s;
  if ((s = blend_enqueue(ctx, *grid, *update, shape.bins, d_indices, n_list, d_new_sh, d_new_maps, d_sh, d_maps, d_state))) return s;
  update_ran(ctx, n_list, map, d_indices != nullptr, 0u, 0u);
  return FLX_OK;
}

/* the resident rows of a host variant into ctx->d_volume_sh and ctx->d_volume_maps, on the context's stream */
static flx_status resident_up(flx_context *ctx, const float *sh, const float *maps, const UpdateShape &shape) {
  flx_status s = flx_grow(ctx, flx_need(&ctx->d_volume_sh, (size_t)shape.probes * 9u), flx_need(maps ? &ctx->d_volume_maps : nullptr, (size_t)shape.rows));
  if (s) return s;
  FLX_HIP(ctx, hipMemcpyAsync(ctx->d_volume_sh.get(), sh, (size_t)flx_volume_update_sh_bytes(shape.probes), hipMemcpyHostToDevice, ctx->stream));
  if (maps) FLX_HIP(ctx, hipMemcpyAsync(ctx->d_volume_maps.get(), maps, (size_t)flx_volume_map_bytes(shape.rows), hipMemcpyHostToDevice, ctx->stream));
  return FLX_OK;
}

extern "C" flx_status flx_volume_blend(flx_context *ctx, const flx_volume_grid *grid, const flx_volume_map *map, const struct flx_volume_update *update, const uint32_t *indices,
                                       uint32_t n_list, const float *new_sh, const float *new_maps, float *sh, float *maps, uint32_t *state) {
  static const char *const call = "flx_volume_blend";
  if (!ctx) return FLX_ERR_INVALID;
  UpdateShape shape;
  flx_status s = shape_refused(ctx, grid, map, update, indices != nullptr, n_list, &shape, call);
  if (s || (s = update_refusal(ctx, flx_volume_update_pairing(map != nullptr, new_maps != nullptr || maps != nullptr, new_maps != nullptr && maps != nullptr), call)) || n_list == 0u)
    return s;
  if (!new_sh || !sh) return update_refusal(ctx, FLX_VOLUME_UPDATE_ARRAY_NULL, call);
  if ((s = host_list_refused(ctx, indices, n_list, shape.probes, call))) return s;
  return flx_rays_from_host(ctx, nullptr, 0u, [&]() -> flx_status {
    const void *d_indices = nullptr;
    flx_status up = indices_up(ctx, indices, n_list, &d_indices);
    if (up || (up = resident_up(ctx, sh, maps, shape))) return up;
    if ((up = flx_grow(ctx, flx_need(&ctx->d_update_sh, (size_t)n_list * 9u), flx_need(map ? &ctx->d_update_maps : nullptr, (size_t)shape.new_rows)))) return up;
    FLX_HIP(ctx, hipMemcpyAsync(ctx->d_update_sh.get(), new_sh, (size_t)flx_volume_update_sh_bytes(n_list), hipMemcpyHostToDevice, ctx->stream));
    if (map) FLX_HIP(ctx, hipMemcpyAsync(ctx->d_update_maps.get(), new_maps, (size_t)flx_volume_map_bytes(shape.new_rows), hipMemcpyHostToDevice, ctx->stream));
    return flx_volume_blend_device(ctx, grid, map, update, d_indices, n_list, ctx->d_update_sh.get(), map ? ctx->d_update_maps.get() : nullptr, ctx->d_volume_sh.get(),
                                   map ? ctx->d_volume_maps.get() : nullptr, state ? ctx->d_update_state.get() : nullptr, nullptr);
  }, flx_down(&ctx->d_volume_sh, (size_t)shape.probes * 9u, sh), flx_down(&ctx->d_volume_maps, (size_t)shape.rows, map ? maps : nullptr),
     flx_down(&ctx->d_update_state, (size_t)n_list, state));
}

/* what both update calls refuse before they look at the update: the scene, the trace params and the probe params, asked of flx_probes_sh_device in its words (no
 * probes: it looks at them and at nothing else, and enqueues nothing) */
static flx_status bake_refused(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params) {
  return flx_probes_sh_device(ctx, trace, params, nullptr, 0u, nullptr, nullptr);
}

/* everything flx_volume_update_device refuses, in its order (n_list == 0: FLX_OK before the arrays are looked at) */
static flx_status update_args_refused(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, const flx_volume_map *map,
                                      const struct flx_volume_update *update, const void *d_indices, uint32_t n_list, void *d_sh, void *d_maps, void *d_state, UpdateShape *shape,
                                      const char *call) {
  flx_status s = bake_refused(ctx, trace, params);
  if (s || (s = shape_refused(ctx, grid, map, update, d_indices != nullptr, n_list, shape, call))) return s;
  if ((s = update_refusal(ctx, flx_volume_update_pairing(map != nullptr, d_maps != nullptr, d_maps != nullptr), call)) || n_list == 0u) return s;
  const bool no_map = map == nullptr;
  const UpdateArray arrays[4] = { { d_indices, flx_volume_update_word_bytes(n_list), 4u, true, INDICES_WHAT },
                                  { d_sh, flx_volume_update_sh_bytes(shape->probes), 16u, false, SH_WHAT },
                                  { d_maps, flx_volume_map_bytes(shape->rows), 16u, no_map, MAPS_WHAT },
                                  { d_state, flx_volume_update_word_bytes(n_list), 4u, true, STATE_WHAT } };
  return arrays_refused(ctx, arrays, 4, call);
}

/* the same for flx_volume_update_relocated_device (flx_volume_relocate.hip), under its own name; *probes and *new_rows (n_list m m; 0 without a map) of an accepted call */
flx_status flx_volume_update_args_refused(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, const flx_volume_map *map,
                                          const struct flx_volume_update *update, const void *d_indices, uint32_t n_list, void *d_sh, void *d_maps, void *d_state, uint32_t *probes,
                                          uint32_t *new_rows, const char *call) {
  UpdateShape shape;
  const flx_status s = update_args_refused(ctx, trace, params, grid, map, update, d_indices, n_list, d_sh, d_maps, d_state, &shape, call);
  *probes = shape.probes; *new_rows = shape.new_rows;
  return s;
}

/* the update and the list alone, in this file's words (flx_volume_positions_offset_device takes a list) */
flx_status flx_volume_update_list_refused(flx_context *ctx, const struct flx_volume_update *update, bool has_list, uint32_t n_list, uint32_t probes, const char *call) {
  return update_refusal(ctx, flx_volume_update_check(update, has_list ? 1 : 0, n_list, probes), call);
}

extern "C" flx_status flx_volume_update_device(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, const flx_volume_map *map,
                                               const struct flx_volume_update *update, const void *d_indices, uint32_t n_list, void *d_sh, void *d_maps, void *d_state,
                                               void *producer_stream) {
  static const char *const call = "flx_volume_update_device";
  if (!ctx) return FLX_ERR_INVALID;
  UpdateShape shape;
  flx_status s = update_args_refused(ctx, trace, params, grid, map, update, d_indices, n_list, d_sh, d_maps, d_state, &shape, call);
  if (s || n_list == 0u) return s;
  if ((s = flx_server_stop(ctx))) return s;
  /* (an earlier update's blend may still read the buffers that are about to go: flx_grow waits first) */
  if ((s = flx_grow(ctx, flx_need(&ctx->d_update_positions, (size_t)n_list), flx_need(&ctx->d_update_sh, (size_t)n_list * 9u),
                    flx_need(map ? &ctx->d_update_maps : nullptr, (size_t)shape.new_rows))))
    return s;
  if ((s = flx_wait_for_producer(ctx, producer_stream))) return s;
  if ((s = positions_enqueue(ctx, *grid, *update, d_indices, n_list, ctx->d_update_positions.get()))) return s;
  s = map ? flx_probes_sh_map_device(ctx, trace, params, map, ctx->d_update_positions.get(), n_list, ctx->d_update_sh.get(), ctx->d_update_maps.get(), nullptr)
          : flx_probes_sh_device(ctx, trace, params, ctx->d_update_positions.get(), n_list, ctx->d_update_sh.get(), nullptr);
  if (s) return s;
  if ((s = blend_enqueue(ctx, *grid, *update, shape.bins, d_indices, n_list, ctx->d_update_sh.get(), map ? ctx->d_update_maps.get() : nullptr, d_sh, d_maps, d_state))) return s;
  update_ran(ctx, n_list, map, d_indices != nullptr, ctx->last_probes.chunks, 1u);
  return FLX_OK;
}

extern "C" flx_status flx_volume_update(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, const flx_volume_map *map,
                                        const struct flx_volume_update *update, const uint32_t *indices, uint32_t n_list, float *sh, float *maps, uint32_t *state) {
  static const char *const call = "flx_volume_update";
  if (!ctx) return FLX_ERR_INVALID;
  UpdateShape shape;
  flx_status s = bake_refused(ctx, trace, params);
  if (s || (s = shape_refused(ctx, grid, map, update, indices != nullptr, n_list, &shape, call))) return s;
  if ((s = update_refusal(ctx, flx_volume_update_pairing(map != nullptr, maps != nullptr, maps != nullptr), call)) || n_list == 0u) return s;
  if (!sh) return update_refusal(ctx, FLX_VOLUME_UPDATE_ARRAY_NULL, call);
  if ((s = host_list_refused(ctx, indices, n_list, shape.probes, call))) return s;
  return flx_rays_from_host(ctx, nullptr, 0u, [&]() -> flx_status {
    const void *d_indices = nullptr;
    flx_status up = indices_up(ctx, indices, n_list, &d_indices);
    if (up || (up = resident_up(ctx, sh, maps, shape))) return up;
    return flx_volume_update_device(ctx, trace, params, grid, map, update, d_indices, n_list, ctx->d_volume_sh.get(), map ? ctx->d_volume_maps.get() : nullptr,
                                    state ? ctx->d_update_state.get() : nullptr, nullptr);
  }, flx_down(&ctx->d_volume_sh, (size_t)shape.probes * 9u, sh), flx_down(&ctx->d_volume_maps, (size_t)shape.rows, map ? maps : nullptr),
     flx_down(&ctx->d_update_state, (size_t)n_list, state));
}

extern "C" uint32_t flx_volume_blend_row_of(const struct flx_volume_update *update, uint32_t bins, const float new_sh[36], const float *new_maps, float sh[36], float *maps) {
  return flx_volume_update_probe(update, bins, new_sh, new_maps, sh, maps);
}

extern "C" flx_status flx_debug_last_volume_update(flx_context *ctx, uint32_t out[8]) {
  if (!ctx || !out) return FLX_ERR_INVALID;
  const flx_context::VolumeUpdateLaunch &v = ctx->last_volume_update;
  out[0] = v.entries; out[1] = v.groups; out[2] = v.size; out[3] = v.listed; out[4] = v.chunks; out[5] = v.fused; out[6] = 0u; out[7] = 0u;
  return FLX_OK;
}
