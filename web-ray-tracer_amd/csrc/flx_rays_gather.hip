/* flx_rays_gather.hip — radiance along a caller's rays with the ambient term taken from a probe volume (include/flexlight_hip_debug.h, "ray batches with a volume":
 * flx_rays_trace_gather, flx_rays_trace_gather_device).  The definition is include/flx_gather.h's: a path of flx_rays_trace that ends in finalColor +
 * importancyFactor * A, A the volume's irradiance at the path's last point times the caller's gain, the params' ambient where the volume has nothing to say.
 *
 * THE LOOKUP IS DEFERRED, NOT INLINED.  k_rays_paths (flx_rays_trace.hip) is built for four waves per SIMD — 128 registers — and holds a whole path per lane; the
 * lookup alone takes 71 registers corner by corner (flx_volume.hip), and lanes finish at different trips, so an inlined lookup would run under a sparse mask in the
 * most register-hungry kernel of the file.  Instead a slab takes three launches behind its first hits (and, in first-hit order, its sort):
 *   1. k_rays_paths_gather<LOCK, ORDERED>: k_rays_paths' refill, item numbering, chunking and loop guard, to the statement.  A trip is the pieces bounce() is made of
 *      (flx_device.h: shadeSurface + shadeSample — what bounceShade calls —, walkBounce, bounceFinish), called one by one so that the iteration's SurfaceCtx, and with
 *      it the smooth normal facing the ray, is still there when the path ends.  A finished path writes its PATH RECORD, four float4 per (ray, sample):
 *        finalColor + the bounce iterations it shaded, as bits | importancyFactor + whether it has a last point (1.0f / 0.0f) | x, 1.0f (0.0f: no point) | n, 0.0f
 *      as PLANES, plane * slots + sample * n + ray (slots = samples * n), so that the lanes of a wave that finish together store next to each other and the next
 *      kernel's loads are contiguous.  x is the path's ray origin, which the walk leaves alone; n lives from the shading to the end of the same trip, across the walk:
 *      three registers (make resources; profiles/rays_gather.txt).  The last sample's path also writes its originalColor, as k_rays_paths does.
 *   2. k_gather_ambient<MAP, OFFSETS>: ONE LANE PER RECORD, dense, 256 threads.  A record of a ray without a first hit was never written and is never read: the hit row
 *      says so.  Four 16-byte loads, flx_volume.hip's corner loop — NOT unrolled: a row at a time; the offset row read before any SH or map row, an inactive corner
 *      reading nothing — over the functions of flx_volume.h, flx_volume_map.h and flx_volume_relocate.h, then flx_gather.h's value and sum, and one 16-byte store into
 *      the slot k_rays_resolve reads: r g b and the bounce iterations.
 *   3. k_rays_resolve (flx_rays_trace.hip), as it stands: the sum over samples in sample order, the scale, originalColor, the radiance row.
 * The scratch — hit rows, slots, originalColor per ray are the traced batches' own buffers; the records a buffer of this file's — is the context's, grown behind
 * flx_grow's one wait and never shrunk.  A slab is flx_trace_slab_rays asked with FIVE slots a sample (flx_gather_args.h): records plus slots stay under the traced
 * batches' 256 MB.  The host side around the launches is the ray-batch calls' shared path (flx_query.hip, flx_rays_host.h). */
#include <cstring>
#include <string>

#define FLX_ANGLE_TABLE 1                  /* as flx_rays_trace.hip: the paths kernel reads the shading's per-triangle table (flx_device.h: one definition per translation unit) */
#include "flx_context.h"
#include "flx_gather.h"
#include "flx_gather_args.h"
#include "flx_kernel_util.h"
#include "flx_query_args.h"
#include "flx_ray_order_args.h"
#include "flx_rays_host.h"
#include "flx_volume_args.h"
#include "flx_volume_map_host.h"

using namespace flx;

namespace flx {

constexpr uint32_t GATHER_CHUNK_UNITS = 4;              /* k_rays_paths' TRACE_CHUNK_UNITS */
constexpr uint32_t GATHER_WAVES = 4;                    /* waves per SIMD the paths kernel is built for: k_rays_paths' */
constexpr uint32_t GATHER_THREADS = FLX_GATHER_THREADS;

struct GatherArgs { DeviceScene sc; DeviceFrame fr; };
static_assert(sizeof(GatherArgs) + 64 <= 4096, "the paths kernel's arguments fit a 4 KB kernarg segment");

/* flx_rays_trace.hip's, used as it stands (its slots are k_gather_ambient's here) */
__global__ void k_rays_resolve(const float4 *__restrict__ hits, const float4 *__restrict__ slots, const float4 *__restrict__ lastOriginal, float4 *__restrict__ out, uint32_t n,
                               int samples);

/* k_rays_paths with a record where it has a slot.  records: FLX_GATHER_RECORD_PLANES planes of S * n float4. */
template <bool LOCK, bool ORDERED = false>
__global__ __launch_bounds__(256, GATHER_WAVES) void k_rays_paths_gather(GatherArgs ta, const float4 *__restrict__ rays, const float4 *__restrict__ hits, float4 *__restrict__ records,
                                                                         float4 *__restrict__ lastOriginal, uint32_t *__restrict__ queue, uint32_t n, uint32_t units,
                                                                         const uint32_t *__restrict__ order) {
  const DeviceScene &sc = ta.sc;
  const DeviceFrame &fr = ta.fr;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t S = (uint32_t)fr.samples;
  const size_t plane = (size_t)S * n;
  f3 origin = F3(0.0f, 0.0f, 0.0f);           /* of the lane's ray: lightTrace's `camera` */
  WorkCounters cnt = {};
  bool alive = false;
  PathState p;
  PixelState ps;
  int bounceIdx = 0;
  float cosSampleN = 0.0f;
  uint32_t rayIdx = 0, sampleIdx = 0;
  uint32_t chunkUnit = 0, chunkNext = 0, chunkEnd = 0;      /* wave-uniform: the chunk's first unit, items of it handed out, its items */
  bool itemsLeft = true;                                    /* wave-uniform */
  auto finishPath = [&](bool hasPoint, f3 normal) {         /* the record in place of fragment:598 + what main() needs from the last sample */
    const size_t at = (size_t)sampleIdx * n + rayIdx;
    const float flag = hasPoint ? 1.0f : 0.0f;
    records[at] = make_float4(p.finalColor.x, p.finalColor.y, p.finalColor.z, __uint_as_float((uint32_t)bounceIdx));
    records[plane + at] = make_float4(p.importancyFactor.x, p.importancyFactor.y, p.importancyFactor.z, flag);
    records[2u * plane + at] = make_float4(p.ray.origin.x, p.ray.origin.y, p.ray.origin.z, flag);
    records[3u * plane + at] = make_float4(normal.x, normal.y, normal.z, 0.0f);
    if (sampleIdx == S - 1u) lastOriginal[rayIdx] = make_float4(ps.originalColor.x, ps.originalColor.y, ps.originalColor.z, 1.0f);
  };

  for (;;) {
    /* -- refill: dead lanes draw new items until the wave is full or the queue is dry ------------ */
    for (;;) {
      const unsigned long long idle = __ballot(!alive);
      if (idle == 0ull) break;
      if (chunkNext == chunkEnd) {
        if (!itemsLeft) break;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(queue, GATHER_CHUNK_UNITS);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= units) { itemsLeft = false; break; }
        chunkUnit = base;
        chunkNext = 0;
        chunkEnd = (units - base > GATHER_CHUNK_UNITS ? GATHER_CHUNK_UNITS : units - base) * 64u;
      }
      const uint32_t nIdle = (uint32_t)__popcll(idle);
      const uint32_t avail = chunkEnd - chunkNext;
      const uint32_t take = nIdle < avail ? nIdle : avail;
      const uint32_t rank = lane_rank(idle);
      if (!alive && rank < take) {
        const uint32_t j = chunkNext + rank, unit = chunkUnit + (j >> 6);      /* unit = block * S + sample: < units, which the host keeps below 2^32 */
        const uint32_t block = unit / S, s = unit - block * S;
        const uint32_t at = block * 64u + (j & 63u);                           /* block < 2^26: no overflow */
        if (at < n) {
          const uint32_t named = ORDERED ? order[at] : at;
          const uint32_t r = named < n ? named : n - 1u;                       /* (an order is a permutation of 0 .. n - 1: the bound holds whatever the order says) */
          const float4 h = hits[(size_t)r * 2u];
          const int tri = __float_as_int(h.w);
          if (tri != -1) {
            const float4 q0 = rays[(size_t)r * 2u], q1 = rays[(size_t)r * 2u + 1u];
            origin = F3(q0.x, q0.y, q0.z);
            ps.ndc_x = q0.w; ps.ndc_y = q1.w;
            ps.seed = fr.view[0].random_seed;
            ps.firstRayLength = 1.0f; ps.glassFilter = 0.0f; ps.originalRMEx = 0.0f; ps.originalTPOx = 0.0f;
            ps.renderId.x = ps.renderId.y = ps.renderId.z = ps.renderId.w = 0.0f;
            ps.renderOriginalId = ps.renderId;
            ps.originalColor = F3(1.0f, 1.0f, 1.0f);
            p.dontFilter = true;
            p.finalColor = F3(0.0f, 0.0f, 0.0f);
            p.importancyFactor = F3(1.0f, 1.0f, 1.0f);
            p.ray.origin = origin; p.ray.dir = F3(q1.x, q1.y, q1.z);      /* as given: rayTracer does not normalise it, lightTrace steps along it by s */
            p.lastHitPoint = origin;
            p.hit.suv = F3(h.x, h.y, h.z);
            p.hit.triangleId = tri;
            p.hit.transformId = __float_as_int(hits[(size_t)r * 2u + 1u].x);
            cosSampleN = flx_cos((float)s);
            bounceIdx = 0;
            rayIdx = r; sampleIdx = s;
            /* loop guard of fragment:475 before the first bounce (fails only for bounces = 0 or minImportancy > 1): such a path has no last point */
            alive = fr.max_reflections > 0 && length(p.importancyFactor * ps.originalColor) >= fr.min_importancy * SQRT3;
            if (!alive) finishPath(false, F3(0.0f, 0.0f, 0.0f));
          }
        }
      }
      chunkNext += take;
    }
    if (__ballot(alive) == 0ull) break;

    /* -- one bounce for every live lane (fragment:475-596): bounce<false, LOCK>() piece by piece, the surface kept ------ */
    if (alive) {
      ShadeOut so;
      SurfaceCtx sf;
      shadeSurface<false>(sc, fr, p.hit, p.ray, p.lastHitPoint, sf, cnt);
      shadeSample<false>(sc, fr, sf, ps, p, origin, cosSampleN, bounceIdx, so);
      const f3 facing = sf.smoothNormal;
      bool shadowed;
      walkBounce<false, LOCK>(sc, so.needShadow, nextBounceRuns(fr, bounceIdx, p.importancyFactor, ps.originalColor), so.shadowRay, so.shadowLen, p.ray, shadowed, p.hit, cnt);
      bounceFinish(ps, p, so, shadowed);
      bool cont = p.hit.triangleId != -1;
      if (cont) p.lastHitPoint = p.ray.origin;
      bounceIdx++;
      if (cont) cont = bounceIdx < fr.max_reflections && length(p.importancyFactor * ps.originalColor) >= fr.min_importancy * SQRT3;
      if (!cont) { finishPath(true, facing); alive = false; }
    }
  }
}

/* the SH row of probe p, nine 16-byte loads (flx_volume.hip's load_sh) */
__device__ __forceinline__ void gather_load_sh(const float4 *__restrict__ sh, uint32_t p, float row[FLX_PROBE_SH_WORDS]) {
  const float4 *r = sh + (size_t)p * 9u;
#pragma unroll
  for (uint32_t i = 0; i < 9u; i++) {
    const float4 v = r[i];
    row[4u * i] = v.x; row[4u * i + 1u] = v.y; row[4u * i + 2u] = v.z; row[4u * i + 3u] = v.w;
  }
}

/* records: four planes of `count` = samples * n float4; slots: count float4, slot sample * n + ray.  n: the slab's rays.  The volume's arrays as flx_volume.hip's
 * kernels take them; maps and map are not read without MAP, offsets not without OFFSETS. */
template <bool MAP, bool OFFSETS>
__global__ __launch_bounds__(GATHER_THREADS) void k_gather_ambient(const float4 *__restrict__ hits, const float4 *__restrict__ records, float4 *__restrict__ slots,
                                                                   const float4 *__restrict__ sh, const float4 *__restrict__ maps, const float4 *__restrict__ offsets,
                                                                   flx_volume_grid g, flx_volume_map map, flx_trace_params params, float gain, uint32_t n, uint64_t count) {
  const uint64_t at = (uint64_t)blockIdx.x * GATHER_THREADS + threadIdx.x;      /* (at most count / 256 + 1 workgroups: no wrap) */
  if (at >= count) return;
  const uint32_t r = (uint32_t)(at % n);
  if (__float_as_int(hits[(size_t)r * 2u].w) == -1) return;                      /* a ray without a first hit: no path wrote this record, the resolve reads no slot of it */
  const float4 c0 = records[at], c1 = records[count + at], x = records[2u * count + at], nn = records[3u * count + at];
  const int hasPoint = c1.w != 0.0f;
  float e[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
  if (hasPoint) {
    const float position[4] = { x.x, x.y, x.z, 1.0f };
    const float normal[3] = { nn.x, nn.y, nn.z };
    const flx_volume_cell c = flx_volume_cell_of(&g, position, normal);
    float sums[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    /* (not unrolled, a row at a time: flx_volume.hip's volume_irradiance says why) */
#pragma unroll 1
    for (uint32_t k = 0; k < 8u; k++) {
      float row[FLX_PROBE_SH_WORDS];
      const uint32_t p = flx_volume_corner(&g, &c, k);
      if constexpr (OFFSETS) {
        const float4 o = offsets[p];
        const float offset[4] = { o.x, o.y, o.z, o.w };
        if (flx_volume_relocate_inactive(offset)) continue;
        gather_load_sh(sh, p, row);
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
      gather_load_sh(sh, p, row);
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
  float a[3], value[3];
  const float finalColor[3] = { c0.x, c0.y, c0.z }, importancy[3] = { c1.x, c1.y, c1.z };
  flx_gather_ambient(&params, gain, hasPoint, e, a);
  flx_gather_path_value(finalColor, importancy, a, value);
  slots[at] = make_float4(value[0], value[1], value[2], c0.w);
}

}  // namespace flx

/* ---- the calls ------------------------------------------------------------------------------------------------------------------------------------- */

static const char *const CALL = "flx_rays_trace_gather";
static const char *const DEVICE_CALL = "flx_rays_trace_gather_device";
static const char *const SH_WHAT = "the SH rows are not nx * ny * nz rows of 144 bytes";

static flx_status fail(flx_context *ctx, flx_status code, const std::string &msg) { return flx_fail(ctx, code, msg.c_str()); }

/* a refusal of flx_gather_args.h in words */
static flx_status gather_refusal(flx_context *ctx, enum flx_gather_refusal why, const char *call) {
  const char *what = "";
  switch (why) {
    case FLX_GATHER_ARGS_OK: return FLX_OK;
    case FLX_GATHER_VOLUME_NULL: what = "the volume is NULL"; break;
    case FLX_GATHER_GAIN: what = "gain is negative or not finite"; break;
    case FLX_GATHER_RESERVED: what = "the volume's reserved word is not 0"; break;
    case FLX_GATHER_MAP_PAIR: what = "map and maps are not both given or both NULL"; break;
    case FLX_GATHER_OVERLAP: what = "an array of the volume overlaps the rays or the radiance"; break;
  }
  return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": " + what);
}

/* what both calls refuse before they look at an array: the scene, the params, a bit of `order` that is none of FLX_TRACE_ORDER_HITS */
static flx_status params_refused(flx_context *ctx, const flx_trace_params *params, uint32_t order) {
  flx_status s = flx_trace_params_refused(ctx, params, CALL);
  if (s) return s;
  if (!flx_order_bits_known(order)) return fail(ctx, FLX_ERR_INVALID, std::string(CALL) + ": order has a bit beyond FLX_TRACE_ORDER_HITS");
  return FLX_OK;
}

/* the volume's words that need no array: the grid and the map in the volume calls' words (a map only where one is given), under `call`; *probes and *rows of an
 * accepted volume (rows 0 without a map) */
static flx_status volume_params_refused(flx_context *ctx, const flx_gather_volume *volume, uint32_t *probes, uint32_t *rows, const char *call) {
  flx_status s = flx_volume_grid_refused(ctx, volume->grid, probes, call);
  if (s) return s;
  *rows = 0u;
  return volume->map ? flx_volume_map_refused(ctx, volume->map, *probes, rows, call) : FLX_OK;
}

static flx_status gather_device(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume, const void *d_rays, void *d_radiance, uint32_t n, uint32_t order,
                                void *producer_stream) {
  const std::string device_call = DEVICE_CALL;
  /* 1. the trace call's arrays, in its words */
  const enum flx_trace_refusal arrays = flx_trace_args_check(1, params->samples, params->max_reflections, params->texture_width, (uint64_t)(uintptr_t)d_rays,
                                                             (uint64_t)(uintptr_t)d_radiance, n);
  switch (arrays) {
    case FLX_TRACE_ARGS_OK: case FLX_TRACE_OVERLAP: break;      /* (overlap: said after the pointers are known to be the device's) */
    case FLX_TRACE_NULL: return fail(ctx, FLX_ERR_INVALID, device_call + ": an array is NULL");
    default: return fail(ctx, FLX_ERR_INVALID, device_call + ": n rows of 32 bytes leave the address space");
  }
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  const size_t bytes = (size_t)n * FLX_RAY_ROW_BYTES;
  if (!flx_rows_on_device(ctx, d_rays, bytes))
    return fail(ctx, FLX_ERR_INVALID, device_call + ": the rays are not n rows in memory of the context's device, 16-byte aligned");
  if (!flx_rows_on_device(ctx, d_radiance, bytes))
    return fail(ctx, FLX_ERR_INVALID, device_call + ": the radiance is not n rows in memory of the context's device, 16-byte aligned");
  if (arrays == FLX_TRACE_OVERLAP)
    return fail(ctx, FLX_ERR_INVALID, device_call + ": the rays and the radiance overlap");
  /* 2. the volume calls' own: the grid, the map, the arrays — the SH rows, then the maps against them, then the offsets against both */
  if (!volume) return gather_refusal(ctx, FLX_GATHER_VOLUME_NULL, DEVICE_CALL);
  uint32_t probes = 0, rows = 0;
  flx_status s = volume_params_refused(ctx, volume, &probes, &rows, DEVICE_CALL);
  if (s) return s;
  const bool has_map = volume->map && volume->maps, relocated = volume->offsets != nullptr;
  uint64_t address[FLX_GATHER_MAX_ARRAYS], lengths[FLX_GATHER_MAX_ARRAYS];
  const void *others[FLX_GATHER_MAX_ARRAYS];
  int k = 0;
  {
    const uint64_t sh_address = (uint64_t)(uintptr_t)volume->sh, sh_bytes = flx_volume_sh_bytes(probes);
    const enum flx_volume_refusal why = flx_volume_arrays_check(&sh_address, &sh_bytes, 1);
    if (why == FLX_VOLUME_NULL) return fail(ctx, FLX_ERR_INVALID, device_call + ": an array is NULL");
    if (why != FLX_VOLUME_ARGS_OK) return fail(ctx, FLX_ERR_INVALID, device_call + ": an array leaves the address space");
    if (!flx_rows_on_device(ctx, volume->sh, (size_t)sh_bytes)) return fail(ctx, FLX_ERR_INVALID, device_call + ": " + SH_WHAT + " in memory of the context's device, 16-byte aligned");
    address[k] = sh_address; lengths[k] = sh_bytes; others[k] = volume->sh; k++;
  }
  if (has_map) {
    const flx_map_other sh_rows[1] = { { volume->sh, lengths[0] } };
    if ((s = flx_volume_maps_refused(ctx, volume->maps, rows, sh_rows, 1, DEVICE_CALL))) return s;
    address[k] = (uint64_t)(uintptr_t)volume->maps; lengths[k] = flx_volume_map_bytes(rows); others[k] = volume->maps; k++;
  }
  if (relocated) {
    if ((s = flx_volume_offsets_refused(ctx, volume->offsets, probes, others, lengths, k, DEVICE_CALL))) return s;
    address[k] = (uint64_t)(uintptr_t)volume->offsets; lengths[k] = (uint64_t)probes * 16u; others[k] = volume->offsets; k++;
  }
  /* 3. this call's own */
  enum flx_gather_refusal own = flx_gather_volume_check(1, volume->gain, volume->reserved, volume->map != nullptr, volume->maps != nullptr);
  if (own == FLX_GATHER_ARGS_OK) own = flx_gather_arrays_check(address, lengths, k, (uint64_t)(uintptr_t)d_rays, (uint64_t)(uintptr_t)d_radiance, n);
  if (own != FLX_GATHER_ARGS_OK) return gather_refusal(ctx, own, DEVICE_CALL);

  GatherArgs ta;
  if ((s = flx_make_scene(ctx, ta.sc))) return s;           /* (refuses a scene that names a transform not uploaded) */
  if ((s = flx_server_stop(ctx))) return s;                 /* as flx_render_device: the frame server's launch ends after the frames posted to it */
  flx_trace_frame(params, ta.fr, 0, 0);                     /* no filter, no temporal */
  const uint32_t S = (uint32_t)params->samples;
  const bool ordered = order != 0u;
  flx_ray_slabs cut(ctx, flx_gather_slab_slots(S), n);      /* five slots a sample: the record's four and the resolve's */
  /* the traced batches' scratch and the records; the sort's is asked for by an ordered batch alone — one growth, one wait */
  if ((s = flx_grow(ctx, flx_need(&ctx->d_trace_hits, (size_t)cut.most * 2u), flx_need(&ctx->d_trace_slots, (size_t)cut.most * S), flx_need(&ctx->d_trace_last, cut.most),
                    flx_need(&ctx->d_gather_records, (size_t)cut.most * S * FLX_GATHER_RECORD_FLOAT4), flx_need(&ctx->d_trace_ctl, 4),
                    flx_need(ordered ? &ctx->d_order_keys[0] : nullptr, flx_order_room(cut.most)), flx_need(ordered ? &ctx->d_order_keys[1] : nullptr, flx_order_room(cut.most)),
                    flx_need(ordered ? &ctx->d_order_pos[0] : nullptr, flx_order_room(cut.most)), flx_need(ordered ? &ctx->d_order_pos[1] : nullptr, flx_order_room(cut.most)),
                    flx_need(ordered ? &ctx->d_order_counts : nullptr, flx_order_table_room(cut.most)), flx_need(ordered ? &ctx->d_order_ctl : nullptr, 16))))
    return s;
  if ((s = flx_wait_for_producer(ctx, producer_stream))) return s;
  if ((s = flx_angle_table(ctx, ta.sc))) return s;          /* the shading's per-triangle table: FLX_ANGLE_TABLE above makes this file's shadeSurface read it */
  const bool lock = FLX_LOCKSTEP && ta.sc.lock_entries != 0u;
  const uint32_t cus = (uint32_t)ctx->prop.multiProcessorCount;
  const flx_volume_grid grid = *volume->grid;
  const flx_volume_map none = { 0u, 0u, { 0u, 0u } };
  const flx_volume_map map = has_map ? *volume->map : none;
  const float4 *d_sh = (const float4 *)volume->sh, *d_maps = (const float4 *)volume->maps, *d_offsets = (const float4 *)volume->offsets;
  const flx_trace_params tp = *params;
  const float gain = volume->gain;
  uint32_t blocks = 0, lookup_groups = 0, sort_groups = 0;
  /* a slab's launches behind its first hits; of d_trace_ctl's words [2] is the paths kernel's unit cursor */
  s = flx_rays_slabs(ctx, ta.sc, d_rays, n, cut, DEVICE_CALL, [&](uint64_t first, uint32_t m, const float4 *rays) -> flx_status {
    float4 *out = (float4 *)d_radiance + first * 2u;
    flx_status so;
    if (ordered && (so = flx_slab_order(ctx, rays, ctx->d_trace_hits.get(), m, &sort_groups))) return so;
    const uint32_t *by = ctx->d_order_pos[0].get();          /* (the unordered kernels do not read it) */
    /* the persistent grid is k_rays_paths': enough workgroups to fill every CU at the kernel's occupancy, no more than the items fill; flx_debug_set_query_groups sets it too */
    const uint32_t units = ((m + 63u) >> 6) * S;
    const uint32_t full = (units + 3u) / 4u;
    blocks = ctx->query_groups ? ctx->query_groups : (full < cus * 8u ? full : cus * 8u);
    uint32_t *queue = ctx->d_trace_ctl.get() + 2;
    float4 *hits = ctx->d_trace_hits.get(), *records = ctx->d_gather_records.get(), *slots = ctx->d_trace_slots.get(), *last = ctx->d_trace_last.get();
    if (ordered) {
      if (lock) hipLaunchKernelGGL((k_rays_paths_gather<true, true>), dim3(blocks), dim3(256), 0, ctx->stream, ta, rays, hits, records, last, queue, m, units, by);
      else hipLaunchKernelGGL((k_rays_paths_gather<false, true>), dim3(blocks), dim3(256), 0, ctx->stream, ta, rays, hits, records, last, queue, m, units, by);
    } else {
      if (lock) hipLaunchKernelGGL((k_rays_paths_gather<true, false>), dim3(blocks), dim3(256), 0, ctx->stream, ta, rays, hits, records, last, queue, m, units, by);
      else hipLaunchKernelGGL((k_rays_paths_gather<false, false>), dim3(blocks), dim3(256), 0, ctx->stream, ta, rays, hits, records, last, queue, m, units, by);
    }
    FLX_HIP(ctx, hipGetLastError());
    const uint64_t count = (uint64_t)m * S;                   /* (below 2^32 wherever the records fit a device's memory; the kernel counts in 64 bits all the same) */
    lookup_groups = flx_gather_groups(count);
    if (has_map && relocated) hipLaunchKernelGGL((k_gather_ambient<true, true>), dim3(lookup_groups), dim3(GATHER_THREADS), 0, ctx->stream, hits, records, slots, d_sh, d_maps, d_offsets, grid, map, tp, gain, m, count);
    else if (relocated) hipLaunchKernelGGL((k_gather_ambient<false, true>), dim3(lookup_groups), dim3(GATHER_THREADS), 0, ctx->stream, hits, records, slots, d_sh, d_maps, d_offsets, grid, map, tp, gain, m, count);
    else if (has_map) hipLaunchKernelGGL((k_gather_ambient<true, false>), dim3(lookup_groups), dim3(GATHER_THREADS), 0, ctx->stream, hits, records, slots, d_sh, d_maps, d_offsets, grid, map, tp, gain, m, count);
    else hipLaunchKernelGGL((k_gather_ambient<false, false>), dim3(lookup_groups), dim3(GATHER_THREADS), 0, ctx->stream, hits, records, slots, d_sh, d_maps, d_offsets, grid, map, tp, gain, m, count);
    FLX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_rays_resolve, dim3((m + 255u) / 256u), dim3(256), 0, ctx->stream, hits, slots, last, out, m, params->samples);
    FLX_HIP(ctx, hipGetLastError());
    return FLX_OK;
  });
  if (s) return s;
  flx_context::GatherLaunch ran;
  ran.n = n; ran.slabs = cut.slabs; ran.slab = cut.slab; ran.path_groups = blocks; ran.lookup_groups = lookup_groups;
  ran.flags = (has_map ? FLX_GATHER_HAS_MAP : 0u) | (relocated ? FLX_GATHER_HAS_OFFSETS : 0u); ran.order = ordered ? 1u : 0u;
  ctx->last_gather = ran;
  return FLX_OK;
}

extern "C" flx_status flx_rays_trace_gather_device(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume, const void *d_rays, void *d_radiance, uint32_t n,
                                                   uint32_t order, void *producer_stream) {
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = params_refused(ctx, params, order);
  if (s || n == 0) return s;
  return gather_device(ctx, params, volume, d_rays, d_radiance, n, order, producer_stream);
}

extern "C" flx_status flx_rays_trace_gather(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume, const float *rays, void *radiance, uint32_t n,
                                            uint32_t order) {
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = params_refused(ctx, params, order);
  if (s || n == 0) return s;
  if (!rays || !radiance) return fail(ctx, FLX_ERR_INVALID, std::string(CALL) + ": an array is NULL");
  /* what needs no device array, under this call's name: the volume, its grid and map, its host arrays, its own words */
  if (!volume) return gather_refusal(ctx, FLX_GATHER_VOLUME_NULL, CALL);
  uint32_t probes = 0, rows = 0;
  if ((s = volume_params_refused(ctx, volume, &probes, &rows, CALL))) return s;
  if (!volume->sh) return fail(ctx, FLX_ERR_INVALID, std::string(CALL) + ": an array is NULL");
  if ((s = gather_refusal(ctx, flx_gather_volume_check(1, volume->gain, volume->reserved, volume->map != nullptr, volume->maps != nullptr), CALL))) return s;
  return flx_rays_from_host(ctx, rays, n, [&]() -> flx_status {
    /* the volume's rows go up where the volume calls' host variants put them (flx_volume.hip), on the context's stream */
    flx_status up = flx_grow(ctx, flx_need(&ctx->d_volume_sh, (size_t)probes * 9u), flx_need(volume->map ? &ctx->d_volume_maps : nullptr, (size_t)rows),
                             flx_need(volume->offsets ? &ctx->d_relocate_offsets : nullptr, (size_t)probes));
    if (up) return up;
    flx_gather_volume dv = *volume;
    FLX_HIP(ctx, hipMemcpyAsync(ctx->d_volume_sh.get(), volume->sh, (size_t)flx_volume_sh_bytes(probes), hipMemcpyHostToDevice, ctx->stream));
    dv.sh = ctx->d_volume_sh.get();
    if (volume->map) {
      FLX_HIP(ctx, hipMemcpyAsync(ctx->d_volume_maps.get(), volume->maps, (size_t)flx_volume_map_bytes(rows), hipMemcpyHostToDevice, ctx->stream));
      dv.maps = ctx->d_volume_maps.get();
    }
    if (volume->offsets) {
      FLX_HIP(ctx, hipMemcpyAsync(ctx->d_relocate_offsets.get(), volume->offsets, (size_t)probes * 16u, hipMemcpyHostToDevice, ctx->stream));
      dv.offsets = ctx->d_relocate_offsets.get();
    }
    return flx_rays_trace_gather_device(ctx, params, &dv, ctx->d_query_rays, ctx->d_query_hits, n, order, nullptr);
  }, flx_down(&ctx->d_query_hits, (size_t)n * 2u, radiance));
}

extern "C" flx_status flx_debug_last_gather(flx_context *ctx, uint32_t out[8]) {
  if (!ctx || !out) return FLX_ERR_INVALID;
  const flx_context::GatherLaunch &t = ctx->last_gather;
  out[0] = t.n; out[1] = t.slabs; out[2] = t.slab; out[3] = t.path_groups; out[4] = t.lookup_groups; out[5] = t.flags; out[6] = t.order; out[7] = FLX_GATHER_RECORD_BYTES;
  return FLX_OK;
}
