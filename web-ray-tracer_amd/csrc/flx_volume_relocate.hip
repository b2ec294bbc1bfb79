/* flx_volume_relocate.hip — probe relocation and classification (include/flexlight_hip_debug.h, "probe relocation": flx_probe_relocate[_device],
 * flx_volume_positions_offset[_device], flx_volume_relocate[_device], flx_volume_bake_relocated[_device], flx_volume_update_relocated[_device],
 * flx_volume_relocate_row_of, flx_debug_last_volume_relocate; the relocated lookups are flx_volume.hip's).  The arithmetic is include/flx_volume_relocate.h's, the
 * text the tests' CPU reference compiles too: offset rows, states and position rows are defined bit for bit.
 *
 * k_probe_relocate: ONE WAVE PER PROBE, four probes a workgroup (k_probe_sh's shape); the 64 lanes are slots.  Lane j reads the HIT row and the NORMAL row of its
 * texels j, j + 64, .. — the planes are contiguous: a wave's 64 rows are 1 KiB of each — and keeps two counters and three 64-bit keys in registers.  Six xor-shuffle
 * steps join the lanes: the counts by integer add, the keys by unsigned minimum (the header's keys turn "least s, lowest t" and "greatest s, lowest t" into that), so
 * no order of the steps matters.  Lane 0 reads the old offset row, computes the move and the state and stores one float4.  A wave without a probe (the last
 * workgroup) leaves at once; a lane without a texel (R < 64) keeps empty keys.  No LDS, no atomics, no scratch (make resources).
 *
 * k_volume_positions_offset: ONE LANE PER ENTRY, the whole grid or a list (indices, or first + j stride in 64 bits) in one kernel; a lane reads its probe's offset
 * row and writes its 16-byte position row.
 *   THE LAUNCHES ARE NOT CUT: n is at most nx ny nz < 2^31, so ceil(n / 4) and ceil(n / 256) workgroups fit a one-dimensional grid.
 *
 * flx_volume_relocate_device cuts the probes into flx_probes_sh_device's chunks and runs, per chunk and on the context's stream, k_volume_positions_offset into
 * ctx->d_relocate_positions, flx_probe_rays_device from there into ctx->d_probe_rays, flx_rays_surface_device AS IT STANDS (FLX_SURFACE_HIT | FLX_SURFACE_NORMAL)
 * into ctx->d_relocate_planes, and k_probe_relocate onto the chunk's rows of the offsets.  A probe's position depends on its own offset row alone, so the chunks do
 * not see each other.  flx_volume_bake_relocated_device and flx_volume_update_relocated_device are compositions of calls that exist.  The host-memory calls are the
 * ray-batch calls' shared path (flx_rays_host.h). */
#include <string>

#include "flx_context.h"
#include "flx_rays_host.h"
#include "flx_volume_args.h"
#include "flx_volume_map_host.h"
#include "flx_volume_relocate.h"
#include "flx_volume_relocate_args.h"

namespace flx {

constexpr uint32_t RELOCATE_THREADS = FLX_VOLUME_RELOCATE_THREADS;
static_assert(RELOCATE_THREADS / 64u == FLX_VOLUME_RELOCATE_WAVE_PROBES, "a wave a probe");

/* hit, normal: n_probes * pg.rays rows each; offsets: the row of the first of the n_probes probes */
__global__ __launch_bounds__(RELOCATE_THREADS) void k_probe_relocate(const float4 *__restrict__ hit, const float4 *__restrict__ normal, float4 *__restrict__ offsets,
                                                                     flx_volume_grid g, struct flx_volume_relocate u, flx_probe_grid pg, uint32_t n_probes) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t probe = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * FLX_VOLUME_RELOCATE_WAVE_PROBES + (threadIdx.x >> 6)));      /* (blockIdx.x <= (n_probes - 1) / 4: no wrap) */
  if (probe >= n_probes) return;                                      /* the whole wave: nothing below waits for another wave */
  const float4 *h = hit + (size_t)probe * pg.rays, *nn = normal + (size_t)probe * pg.rays;      /* (n_probes * R < 2^32 rows: the calls' check) */
  flx_volume_relocate_sums r = flx_volume_relocate_empty();
  for (uint32_t t = lane; t < pg.rays; t += 64u) {
    const float4 a = h[t], b = nn[t];
    const float hit_row[4] = { a.x, a.y, a.z, a.w }, normal_row[4] = { b.x, b.y, b.z, b.w };
    flx_volume_relocate_texel(&r, t, hit_row, normal_row);
  }
  /* all 64 lanes are here again */
#pragma unroll
  for (uint32_t off = 1u; off < 64u; off <<= 1) {
    flx_volume_relocate_sums o;
    o.hits = (uint32_t)__shfl_xor((int)r.hits, (int)off, 64);
    o.backs = (uint32_t)__shfl_xor((int)r.backs, (int)off, 64);
    o.closest_back = (uint64_t)__shfl_xor((unsigned long long)r.closest_back, (int)off, 64);
    o.closest_front = (uint64_t)__shfl_xor((unsigned long long)r.closest_front, (int)off, 64);
    o.farthest_front = (uint64_t)__shfl_xor((unsigned long long)r.farthest_front, (int)off, 64);
    r = flx_volume_relocate_join(r, o);
  }
  if (lane != 0u) return;
  const float4 was = offsets[probe];
  const float old[4] = { was.x, was.y, was.z, was.w };
  float out[4];
  flx_volume_relocate_move(&g, &u, &pg, &r, old, out);
  offsets[probe] = make_float4(out[0], out[1], out[2], out[3]);
}

/* offsets: the grid's rows; indices: n words, or nullptr; listed 0: entry j is probe j (the whole grid); positions: n rows */
__global__ __launch_bounds__(RELOCATE_THREADS) void k_volume_positions_offset(const float4 *__restrict__ offsets, const uint32_t *__restrict__ indices, float4 *__restrict__ positions,
                                                                              flx_volume_grid g, struct flx_volume_update u, uint32_t listed, uint32_t n) {
  const uint32_t j = blockIdx.x * RELOCATE_THREADS + threadIdx.x;      /* (blockIdx.x <= (n - 1) / 256 and n < 2^31: no wrap) */
  if (j >= n) return;
  const uint64_t index = listed ? flx_volume_update_entry(&u, indices, j) : (uint64_t)j;
  float row[4];
  flx_volume_relocate_position(&g, (const float *)offsets, index, row);
  positions[j] = make_float4(row[0], row[1], row[2], row[3]);
}

}  // namespace flx

using namespace flx;

/* ---- the calls ------------------------------------------------------------------------------------------------------------------------------------- */

static flx_status fail(flx_context *ctx, flx_status code, const std::string &msg) { return flx_fail(ctx, code, msg.c_str()); }

/* a refusal of flx_volume_relocate_args.h in words */
static flx_status relocate_refusal(flx_context *ctx, enum flx_volume_relocate_refusal why, const char *call) {
  const char *what = "";
  switch (why) {
    case FLX_VOLUME_RELOCATE_ARGS_OK: return FLX_OK;
    case FLX_VOLUME_RELOCATE_NULL: what = "the relocation is NULL"; break;
    case FLX_VOLUME_RELOCATE_BACK_SHARE: what = "back_share is not one of 0 .. 1"; break;
    case FLX_VOLUME_RELOCATE_MIN_FRONT: what = "min_front is negative or not finite"; break;
    case FLX_VOLUME_RELOCATE_REACH: what = "reach is not greater than 0 or not finite"; break;
    case FLX_VOLUME_RELOCATE_LIMIT: what = "limit is not one of 0 .. 0.5"; break;
    case FLX_VOLUME_RELOCATE_FLAGS: what = "flags has a bit beyond FLX_VOLUME_RELOCATE_FREEZE"; break;
    case FLX_VOLUME_RELOCATE_RESERVED: what = "the relocation's reserved word is not 0"; break;
    case FLX_VOLUME_RELOCATE_FACE_SIZE: what = "face_size is not one of 1 .. 256"; break;
    case FLX_VOLUME_RELOCATE_RANGE: what = "first_probe + n_probes is beyond the grid's probes"; break;
    case FLX_VOLUME_RELOCATE_ROWS: what = "n_probes * 6 * face_size * face_size is 2^32 or more"; break;
  }
  return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": " + what);
}

/* an array's own refusals (flx_volume_update_args.h's rules, used as they stand) in words */
static flx_status array_refusal(flx_context *ctx, enum flx_volume_update_refusal why, const char *call) {
  const char *what = "";
  switch (why) {
    case FLX_VOLUME_UPDATE_ARRAY_NULL: what = "an array is NULL"; break;
    case FLX_VOLUME_UPDATE_MISALIGNED: what = "an array is misaligned (16 bytes; 4 for indices and states)"; break;
    case FLX_VOLUME_UPDATE_WRAPS: what = "an array leaves the address space"; break;
    case FLX_VOLUME_UPDATE_OVERLAP: what = "the arrays overlap"; break;
    default: return FLX_OK;
  }
  return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": " + what);
}

struct RelocateArray { const void *p; uint64_t bytes; uint32_t align; bool optional; const char *what; };
constexpr int RELOCATE_MAX_ARRAYS = FLX_VOLUME_UPDATE_MAX_ARRAYS;      /* (no call here has more than three) */

/* The k arrays of a device call: there, aligned, inside 64 bits, memory of the context's device, and apart — in that order. */
static flx_status arrays_refused(flx_context *ctx, const RelocateArray *arrays, int k, const char *call) {
  flx_update_array a[RELOCATE_MAX_ARRAYS];
  for (int i = 0; i < k; i++) a[i] = { (uint64_t)(uintptr_t)arrays[i].p, arrays[i].bytes, arrays[i].align, arrays[i].optional ? 1 : 0 };
  const enum flx_volume_update_refusal why = flx_volume_update_arrays_check(a, k);
  if (why != FLX_VOLUME_UPDATE_ARGS_OK && why != FLX_VOLUME_UPDATE_OVERLAP) return array_refusal(ctx, why, call);      /* (overlap: said after the pointers are known to be the device's) */
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  for (int i = 0; i < k; i++) {
    if (flx_update_array_absent(a[i])) continue;
    const bool there = arrays[i].align == 16u ? flx_rows_on_device(ctx, arrays[i].p, (size_t)arrays[i].bytes) : flx_words_on_device(ctx, arrays[i].p, (size_t)arrays[i].bytes);
    if (!there) return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": " + arrays[i].what + " in memory of the context's device");
  }
  return array_refusal(ctx, why, call);
}

static const char *const OFFSETS_WHAT = "the offsets are not nx * ny * nz rows of 16 bytes";

/* the offset rows of a relocated lookup (flx_volume.hip) against the call's other arrays, which their own checks have accepted */
flx_status flx_volume_offsets_refused(flx_context *ctx, const void *d_offsets, uint32_t probes, const void *const *others, const uint64_t *other_bytes, int k, const char *call) {
  const RelocateArray own[1] = { { d_offsets, flx_volume_relocate_row_bytes(probes), 16u, false, OFFSETS_WHAT } };
  flx_status s = arrays_refused(ctx, own, 1, call);
  if (s) return s;
  for (int i = 0; i < k; i++)
    if (flx_ranges_overlap((uint64_t)(uintptr_t)d_offsets, own[0].bytes, (uint64_t)(uintptr_t)others[i], other_bytes[i])) return array_refusal(ctx, FLX_VOLUME_UPDATE_OVERLAP, call);
  return FLX_OK;
}

static flx_status reduce_enqueue(flx_context *ctx, const flx_volume_grid &g, const struct flx_volume_relocate &u, const flx_probe_grid &pg, const float4 *d_hit, const float4 *d_normal,
                                 uint32_t n_probes, float4 *d_first_row) {
  hipLaunchKernelGGL(k_probe_relocate, dim3(flx_volume_relocate_groups(n_probes)), dim3(RELOCATE_THREADS), 0, ctx->stream, d_hit, d_normal, d_first_row, g, u, pg, n_probes);
  FLX_HIP(ctx, hipGetLastError());
  return FLX_OK;
}

static flx_status positions_enqueue(flx_context *ctx, const flx_volume_grid &g, const float4 *d_offsets, const struct flx_volume_update *update, const void *d_indices, uint32_t n,
                                    float4 *d_positions) {
  const struct flx_volume_update none = { 0.0f, 0u, 1u, 0u };
  hipLaunchKernelGGL(k_volume_positions_offset, dim3(flx_volume_relocate_position_groups(n)), dim3(RELOCATE_THREADS), 0, ctx->stream, d_offsets, (const uint32_t *)d_indices, d_positions,
                     g, update ? *update : none, update ? 1u : 0u, n);
  FLX_HIP(ctx, hipGetLastError());
  return FLX_OK;
}

static void relocate_ran(flx_context *ctx, uint32_t probes, uint32_t face_size, uint32_t chunks, uint32_t chunk, uint32_t groups, uint32_t flags, uint32_t first, uint32_t fused) {
  flx_context::VolumeRelocateLaunch ran;
  ran.probes = probes; ran.face_size = face_size; ran.chunks = chunks; ran.chunk = chunk; ran.groups = groups; ran.flags = flags; ran.first = first; ran.fused = fused;
  ctx->last_volume_relocate = ran;
}

/* what both reduction calls decide before they look at an array: the grid, then the relocation, then the range */
static flx_status reduce_refused(flx_context *ctx, const flx_volume_grid *grid, const struct flx_volume_relocate *relocate, uint32_t n_probes, uint32_t face_size, uint32_t first_probe,
                                 uint32_t *probes, uint32_t *rows, const char *call) {
  flx_status s = flx_volume_grid_refused(ctx, grid, probes, call);
  if (s || (s = relocate_refusal(ctx, flx_volume_relocate_check(relocate), call))) return s;
  return relocate_refusal(ctx, flx_volume_relocate_range_check(face_size, first_probe, n_probes, *probes, rows), call);
}

extern "C" flx_status flx_probe_relocate_device(flx_context *ctx, const flx_volume_grid *grid, const struct flx_volume_relocate *relocate, const void *d_hit, const void *d_normal,
                                                uint32_t n_probes, uint32_t face_size, uint32_t first_probe, void *d_offsets, void *producer_stream) {
  static const char *const call = "flx_probe_relocate_device";
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t probes = 0, rows = 0;
  flx_status s = reduce_refused(ctx, grid, relocate, n_probes, face_size, first_probe, &probes, &rows, call);
  if (s || n_probes == 0u) return s;
  const RelocateArray arrays[3] = { { d_hit, flx_volume_relocate_row_bytes(rows), 16u, false, "the HIT plane is not n_probes * 6 * face_size * face_size rows of 16 bytes" },
                                    { d_normal, flx_volume_relocate_row_bytes(rows), 16u, false, "the NORMAL plane is not n_probes * 6 * face_size * face_size rows of 16 bytes" },
                                    { d_offsets, flx_volume_relocate_row_bytes(probes), 16u, false, OFFSETS_WHAT } };
  if ((s = arrays_refused(ctx, arrays, 3, call))) return s;
  if ((s = flx_server_stop(ctx)) || (s = flx_wait_for_producer(ctx, producer_stream))) return s;
  if ((s = reduce_enqueue(ctx, *grid, *relocate, flx_probe_grid_of(face_size), (const float4 *)d_hit, (const float4 *)d_normal, n_probes, (float4 *)d_offsets + first_probe))) return s;
  relocate_ran(ctx, n_probes, face_size, 0u, 0u, flx_volume_relocate_groups(n_probes), relocate->flags, first_probe, 0u);
  return FLX_OK;
}

/* the offset rows of a host variant into ctx->d_relocate_offsets, on the context's stream */
static flx_status offsets_up(flx_context *ctx, const float *offsets, uint32_t probes) {
  flx_status s = flx_grow(ctx, flx_need(&ctx->d_relocate_offsets, (size_t)probes));
  if (s) return s;
  FLX_HIP(ctx, hipMemcpyAsync(ctx->d_relocate_offsets.get(), offsets, (size_t)flx_volume_relocate_row_bytes(probes), hipMemcpyHostToDevice, ctx->stream));
  return FLX_OK;
}

extern "C" flx_status flx_probe_relocate(flx_context *ctx, const flx_volume_grid *grid, const struct flx_volume_relocate *relocate, const void *hit, const void *normal, uint32_t n_probes,
                                         uint32_t face_size, uint32_t first_probe, float *offsets) {
  static const char *const call = "flx_probe_relocate";
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t probes = 0, rows = 0;
  flx_status s = reduce_refused(ctx, grid, relocate, n_probes, face_size, first_probe, &probes, &rows, call);
  if (s || n_probes == 0u) return s;
  if (!hit || !normal || !offsets) return array_refusal(ctx, FLX_VOLUME_UPDATE_ARRAY_NULL, call);
  return flx_rays_from_host(ctx, nullptr, 0u, [&]() -> flx_status {
    flx_status up = offsets_up(ctx, offsets, probes);
    if (up || (up = flx_grow(ctx, flx_need(&ctx->d_relocate_planes, (size_t)rows * 2u)))) return up;
    float4 *planes = ctx->d_relocate_planes.get();
    FLX_HIP(ctx, hipMemcpyAsync(planes, hit, (size_t)flx_volume_relocate_row_bytes(rows), hipMemcpyHostToDevice, ctx->stream));
    FLX_HIP(ctx, hipMemcpyAsync(planes + rows, normal, (size_t)flx_volume_relocate_row_bytes(rows), hipMemcpyHostToDevice, ctx->stream));
    return flx_probe_relocate_device(ctx, grid, relocate, planes, planes + rows, n_probes, face_size, first_probe, ctx->d_relocate_offsets.get(), nullptr);
  }, flx_down(&ctx->d_relocate_offsets, (size_t)probes, offsets));
}

/* what both position calls decide before they look at an array: the grid, then the list in the update calls' words.  update NULL: the whole grid. */
static flx_status positions_refused(flx_context *ctx, const flx_volume_grid *grid, const struct flx_volume_update *update, bool has_list, uint32_t n, uint32_t *probes, const char *call) {
  flx_status s = flx_volume_grid_refused(ctx, grid, probes, call);
  if (s) return s;
  if (update) return flx_volume_update_list_refused(ctx, update, has_list, n, *probes, call);
  if (has_list) return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": indices are given without an update");
  if (n != 0u && n != *probes) return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": n is not nx * ny * nz for the whole grid");
  return FLX_OK;
}

extern "C" flx_status flx_volume_positions_offset_device(flx_context *ctx, const flx_volume_grid *grid, const void *d_offsets, const struct flx_volume_update *update, const void *d_indices,
                                                         uint32_t n, void *d_positions, void *producer_stream) {
  static const char *const call = "flx_volume_positions_offset_device";
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t probes = 0;
  flx_status s = positions_refused(ctx, grid, update, d_indices != nullptr, n, &probes, call);
  if (s || n == 0u) return s;
  const RelocateArray arrays[3] = { { d_offsets, flx_volume_relocate_row_bytes(probes), 16u, false, OFFSETS_WHAT },
                                    { d_indices, flx_volume_update_word_bytes(n), 4u, true, "the indices are not n words of 4 bytes" },
                                    { d_positions, flx_volume_relocate_row_bytes(n), 16u, false, "the positions are not n rows of 16 bytes" } };
  if ((s = arrays_refused(ctx, arrays, 3, call))) return s;
  if ((s = flx_server_stop(ctx)) || (s = flx_wait_for_producer(ctx, producer_stream))) return s;
  return positions_enqueue(ctx, *grid, (const float4 *)d_offsets, update, d_indices, n, (float4 *)d_positions);
}

/* the list of a host variant into ctx->d_update_indices, on the context's stream; -> the list on the device (nullptr for none) */
static flx_status indices_up(flx_context *ctx, const uint32_t *indices, uint32_t n, const void **d_indices) {
  *d_indices = nullptr;
  if (!indices) return FLX_OK;
  flx_status s = flx_grow(ctx, flx_need(&ctx->d_update_indices, (size_t)n));
  if (s) return s;
  FLX_HIP(ctx, hipMemcpyAsync(ctx->d_update_indices.get(), indices, (size_t)flx_volume_update_word_bytes(n), hipMemcpyHostToDevice, ctx->stream));
  *d_indices = ctx->d_update_indices.get();
  return FLX_OK;
}

extern "C" flx_status flx_volume_positions_offset(flx_context *ctx, const flx_volume_grid *grid, const float *offsets, const struct flx_volume_update *update, const uint32_t *indices,
                                                  uint32_t n, float *positions) {
  static const char *const call = "flx_volume_positions_offset";
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t probes = 0;
  flx_status s = positions_refused(ctx, grid, update, indices != nullptr, n, &probes, call);
  if (s || n == 0u) return s;
  if (!offsets || !positions) return array_refusal(ctx, FLX_VOLUME_UPDATE_ARRAY_NULL, call);
  return flx_rays_from_host(ctx, nullptr, 0u, [&]() -> flx_status {
    const void *d_indices = nullptr;
    flx_status up = offsets_up(ctx, offsets, probes);
    if (up || (up = indices_up(ctx, indices, n, &d_indices))) return up;
    return flx_volume_positions_offset_device(ctx, grid, ctx->d_relocate_offsets.get(), update, d_indices, n, ctx->d_query_hits.get(), nullptr);
  }, flx_down(&ctx->d_query_hits, (size_t)n, positions));
}

static const uint32_t RELOCATE_FIELDS = FLX_SURFACE_HIT | FLX_SURFACE_NORMAL;

/* what both whole-path calls decide before they look at the offsets: the scene and texture_width in the surface call's words (n = 0: it looks at them and at nothing
 * else), the grid, the relocation, the face size */
static flx_status relocate_refused(flx_context *ctx, int32_t texture_width, const flx_volume_grid *grid, const struct flx_volume_relocate *relocate, uint32_t face_size, uint32_t *probes,
                                   const char *call) {
  flx_status s = flx_rays_surface_device(ctx, texture_width, nullptr, 0u, RELOCATE_FIELDS, nullptr, nullptr);
  if (s || (s = flx_volume_grid_refused(ctx, grid, probes, call)) || (s = relocate_refusal(ctx, flx_volume_relocate_check(relocate), call))) return s;
  return relocate_refusal(ctx, flx_volume_relocate_range_check(face_size, 0u, 0u, *probes, nullptr), call);      /* (the chunks' rows are below 2^32 by their size) */
}

extern "C" flx_status flx_volume_relocate_device(flx_context *ctx, int32_t texture_width, const flx_volume_grid *grid, const struct flx_volume_relocate *relocate, uint32_t face_size,
                                                 void *d_offsets, void *producer_stream) {
  static const char *const call = "flx_volume_relocate_device";
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t probes = 0;
  flx_status s = relocate_refused(ctx, texture_width, grid, relocate, face_size, &probes, call);
  if (s) return s;
  const RelocateArray arrays[1] = { { d_offsets, flx_volume_relocate_row_bytes(probes), 16u, false, OFFSETS_WHAT } };
  if ((s = arrays_refused(ctx, arrays, 1, call))) return s;
  const flx_probe_grid pg = flx_probe_grid_of(face_size);
  const uint32_t chunk = flx_volume_relocate_chunk(face_size, ctx->probe_chunk);
  const uint32_t most = probes < chunk ? probes : chunk;
  if ((s = flx_server_stop(ctx))) return s;
  /* (an earlier call's chunk may still read the buffers that are about to go: flx_grow waits first) */
  if ((s = flx_grow(ctx, flx_need(&ctx->d_relocate_positions, (size_t)most), flx_need(&ctx->d_probe_rays, (size_t)most * pg.rays * 2u),
                    flx_need(&ctx->d_relocate_planes, (size_t)most * pg.rays * 2u))))
    return s;
  if ((s = flx_wait_for_producer(ctx, producer_stream))) return s;
  uint32_t chunks = 0, groups = 0;
  for (uint32_t first = 0; first < probes; first += chunk) {
    const uint32_t m = probes - first < chunk ? probes - first : chunk;
    const uint32_t rows = m * pg.rays;                        /* (at most 2^21, or one probe's 393 216) */
    const struct flx_volume_update range = { 0.0f, first, 1u, 0u };
    float4 *planes = ctx->d_relocate_planes.get();
    if ((s = positions_enqueue(ctx, *grid, (const float4 *)d_offsets, &range, nullptr, m, ctx->d_relocate_positions.get()))) return s;
    if ((s = flx_probe_rays_device(ctx, ctx->d_relocate_positions.get(), m, face_size, ctx->d_probe_rays.get(), nullptr))) return s;
    if ((s = flx_rays_surface_device(ctx, texture_width, ctx->d_probe_rays.get(), rows, RELOCATE_FIELDS, planes, nullptr))) return s;
    if ((s = reduce_enqueue(ctx, *grid, *relocate, pg, planes, planes + rows, m, (float4 *)d_offsets + first))) return s;
    groups = flx_volume_relocate_groups(m);
    chunks++;
    if (probes - first <= chunk) break;                       /* (first + chunk could wrap) */
  }
  relocate_ran(ctx, probes, face_size, chunks, chunk, groups, relocate->flags, 0u, 1u);
  return FLX_OK;
}

extern "C" flx_status flx_volume_relocate(flx_context *ctx, int32_t texture_width, const flx_volume_grid *grid, const struct flx_volume_relocate *relocate, uint32_t face_size,
                                          float *offsets) {
  static const char *const call = "flx_volume_relocate";
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t probes = 0;
  flx_status s = relocate_refused(ctx, texture_width, grid, relocate, face_size, &probes, call);
  if (s) return s;
  if (!offsets) return array_refusal(ctx, FLX_VOLUME_UPDATE_ARRAY_NULL, call);
  return flx_rays_from_host(ctx, nullptr, 0u, [&]() -> flx_status {
    flx_status up = offsets_up(ctx, offsets, probes);
    return up ? up : flx_volume_relocate_device(ctx, texture_width, grid, relocate, face_size, ctx->d_relocate_offsets.get(), nullptr);
  }, flx_down(&ctx->d_relocate_offsets, (size_t)probes, offsets));
}

/* what both relocated bakes decide before they look at an array: the scene, the trace params and the probe params in flx_probes_sh_device's words, the grid, the map
 * where one is given, the pairing of map and maps */
static flx_status bake_refused(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, const flx_volume_map *map, bool has_maps,
                               uint32_t *probes, uint32_t *rows, const char *call) {
  flx_status s = flx_probes_sh_device(ctx, trace, params, nullptr, 0u, nullptr, nullptr);
  if (s || (s = flx_volume_grid_refused(ctx, grid, probes, call)) || (map && (s = flx_volume_map_refused(ctx, map, *probes, rows, call)))) return s;
  if (!map && has_maps) return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": maps are given without a map");
  if (map && !has_maps) return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": a map is given without its maps");
  return FLX_OK;
}

extern "C" flx_status flx_volume_bake_relocated_device(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, const flx_volume_map *map,
                                                       const void *d_offsets, void *d_sh, void *d_maps, void *producer_stream) {
  static const char *const call = "flx_volume_bake_relocated_device";
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t probes = 0, rows = 0;
  flx_status s = bake_refused(ctx, trace, params, grid, map, d_maps != nullptr, &probes, &rows, call);
  if (s) return s;
  const RelocateArray arrays[3] = { { d_offsets, flx_volume_relocate_row_bytes(probes), 16u, false, OFFSETS_WHAT },
                                    { d_sh, flx_volume_update_sh_bytes(probes), 16u, false, "the SH rows are not nx * ny * nz rows of 144 bytes" },
                                    { d_maps, flx_volume_map_bytes(rows), 16u, map == nullptr, "the maps are not nx * ny * nz * size * size rows of 16 bytes" } };
  if ((s = arrays_refused(ctx, arrays, 3, call))) return s;
  if ((s = flx_server_stop(ctx))) return s;
  if ((s = flx_grow(ctx, flx_need(&ctx->d_volume_positions, (size_t)probes)))) return s;
  if ((s = flx_volume_positions_offset_device(ctx, grid, d_offsets, nullptr, nullptr, probes, ctx->d_volume_positions.get(), producer_stream))) return s;
  return map ? flx_probes_sh_map_device(ctx, trace, params, map, ctx->d_volume_positions.get(), probes, d_sh, d_maps, nullptr)
             : flx_probes_sh_device(ctx, trace, params, ctx->d_volume_positions.get(), probes, d_sh, nullptr);
}

extern "C" flx_status flx_volume_bake_relocated(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, const flx_volume_map *map,
                                                const float *offsets, float *sh, float *maps) {
  static const char *const call = "flx_volume_bake_relocated";
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t probes = 0, rows = 0;
  flx_status s = bake_refused(ctx, trace, params, grid, map, maps != nullptr, &probes, &rows, call);
  if (s) return s;
  if (!offsets || !sh) return array_refusal(ctx, FLX_VOLUME_UPDATE_ARRAY_NULL, call);
  return flx_rays_from_host(ctx, nullptr, 0u, [&]() -> flx_status {
    flx_status up = offsets_up(ctx, offsets, probes);
    return up ? up : flx_volume_bake_relocated_device(ctx, trace, params, grid, map, ctx->d_relocate_offsets.get(), ctx->d_query_hits.get(), map ? ctx->d_volume_maps.get() : nullptr, nullptr);
  }, flx_down(&ctx->d_query_hits, (size_t)probes * 9u, sh), flx_down(&ctx->d_volume_maps, (size_t)rows, map ? maps : nullptr));
}

extern "C" flx_status flx_volume_update_relocated_device(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, const flx_volume_map *map,
                                                         const struct flx_volume_update *update, const void *d_indices, uint32_t n_list, const void *d_offsets, void *d_sh, void *d_maps,
                                                         void *d_state, void *producer_stream) {
  static const char *const call = "flx_volume_update_relocated_device";
  if (!ctx) return FLX_ERR_INVALID;
  uint32_t probes = 0, new_rows = 0;
  flx_status s = flx_volume_update_args_refused(ctx, trace, params, grid, map, update, d_indices, n_list, d_sh, d_maps, d_state, &probes, &new_rows, call);
  if (s || n_list == 0u) return s;
  const void *others[4] = { d_indices, d_sh, d_maps, d_state };
  const uint64_t bytes[4] = { d_indices ? flx_volume_update_word_bytes(n_list) : 0u, flx_volume_update_sh_bytes(probes), d_maps ? flx_volume_map_bytes(probes * (map->size * map->size)) : 0u,
                              d_state ? flx_volume_update_word_bytes(n_list) : 0u };
  if ((s = flx_volume_offsets_refused(ctx, d_offsets, probes, others, bytes, 4, call))) return s;
  if ((s = flx_server_stop(ctx))) return s;
  /* (an earlier update's blend may still read the buffers that are about to go: flx_grow waits first) */
  if ((s = flx_grow(ctx, flx_need(&ctx->d_update_positions, (size_t)n_list), flx_need(&ctx->d_update_sh, (size_t)n_list * 9u), flx_need(map ? &ctx->d_update_maps : nullptr, (size_t)new_rows))))
    return s;
  if ((s = flx_volume_positions_offset_device(ctx, grid, d_offsets, update, d_indices, n_list, ctx->d_update_positions.get(), producer_stream))) return s;
  s = map ? flx_probes_sh_map_device(ctx, trace, params, map, ctx->d_update_positions.get(), n_list, ctx->d_update_sh.get(), ctx->d_update_maps.get(), nullptr)
          : flx_probes_sh_device(ctx, trace, params, ctx->d_update_positions.get(), n_list, ctx->d_update_sh.get(), nullptr);
  if (s) return s;
  return flx_volume_blend_device(ctx, grid, map, update, d_indices, n_list, ctx->d_update_sh.get(), map ? ctx->d_update_maps.get() : nullptr, d_sh, d_maps, d_state, nullptr);
}

extern "C" flx_status flx_volume_update_relocated(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, const flx_volume_map *map,
                                                  const struct flx_volume_update *update, const uint32_t *indices, uint32_t n_list, const float *offsets, float *sh, float *maps,
                                                  uint32_t *state) {
  static const char *const call = "flx_volume_update_relocated";
  if (!ctx) return FLX_ERR_INVALID;
  /* the rules that need no array, asked of the device call with no entries under this name's sibling; then the arrays of the host */
  uint32_t probes = 0, new_rows = 0;
  flx_status s = flx_volume_update_args_refused(ctx, trace, params, grid, map, update, indices ? (const void *)indices : nullptr, 0u, nullptr, maps, nullptr, &probes, &new_rows, call);
  if (s || (s = flx_volume_update_list_refused(ctx, update, indices != nullptr, n_list, probes, call)) || n_list == 0u) return s;
  if (!offsets || !sh) return array_refusal(ctx, FLX_VOLUME_UPDATE_ARRAY_NULL, call);
  if (indices && flx_volume_update_duplicate(indices, n_list, probes)) return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": the list names a probe twice");
  const uint32_t rows = map ? probes * (map->size * map->size) : 0u;
  return flx_rays_from_host(ctx, nullptr, 0u, [&]() -> flx_status {
    const void *d_indices = nullptr;
    flx_status up = offsets_up(ctx, offsets, probes);
    if (up || (up = indices_up(ctx, indices, n_list, &d_indices))) return up;
    if ((up = flx_grow(ctx, flx_need(&ctx->d_volume_sh, (size_t)probes * 9u), flx_need(map ? &ctx->d_volume_maps : nullptr, (size_t)rows)))) return up;
    FLX_HIP(ctx, hipMemcpyAsync(ctx->d_volume_sh.get(), sh, (size_t)flx_volume_update_sh_bytes(probes), hipMemcpyHostToDevice, ctx->stream));
    if (map) FLX_HIP(ctx, hipMemcpyAsync(ctx->d_volume_maps.get(), maps, (size_t)flx_volume_map_bytes(rows), hipMemcpyHostToDevice, ctx->stream));
    return flx_volume_update_relocated_device(ctx, trace, params, grid, map, update, d_indices, n_list, ctx->d_relocate_offsets.get(), ctx->d_volume_sh.get(),
                                              map ? ctx->d_volume_maps.get() : nullptr, state ? ctx->d_update_state.get() : nullptr, nullptr);
  }, flx_down(&ctx->d_volume_sh, (size_t)probes * 9u, sh), flx_down(&ctx->d_volume_maps, (size_t)rows, map ? maps : nullptr), flx_down(&ctx->d_update_state, (size_t)n_list, state));
}

extern "C" void flx_volume_relocate_row_of(const flx_volume_grid *grid, const struct flx_volume_relocate *relocate, uint32_t face_size, const float *hit, const float *normal,
                                           float offset[4]) {
  flx_volume_relocate_probe(grid, relocate, face_size, hit, normal, offset);
}

extern "C" flx_status flx_debug_last_volume_relocate(flx_context *ctx, uint32_t out[8]) {
  if (!ctx || !out) return FLX_ERR_INVALID;
  const flx_context::VolumeRelocateLaunch &v = ctx->last_volume_relocate;
  out[0] = v.probes; out[1] = v.face_size; out[2] = v.chunks; out[3] = v.chunk; out[4] = v.groups; out[5] = v.flags; out[6] = v.first; out[7] = v.fused;
  return FLX_OK;
}
