/* flx_rays_trace.hip — radiance along a caller's rays (include/flexlight_hip_debug.h, "ray queries": flx_rays_trace, flx_rays_trace_device, and the same in
 * first-hit order: flx_rays_trace_ordered, flx_rays_trace_ordered_device).
 *
 * What a frame computes for a pixel without filter and without temporal (fragment:601-632), computed for a ray of the caller's own: hit = rayTracer(origin,
 * direction); the samples' lightTrace(hit, direction, origin, cos(float(s)), max_reflections) added in sample order, averaged, times the originalColor the last
 * sample left.  The ray's origin stands where a frame has its camera, the row's two noise coordinates where a frame has the pixel's NDC.
 *
 * The structure is pipeline 2's (flx_kernels.hip: k_primary -> k_paths -> k_resolve) with rows where it has pixels:
 *   1. first hits: k_ray_query as it stands (flx_query.hip, what = FLX_RAYS_CLOSEST) into hit rows the context owns — a hit row's first float4 is k_paths'
 *      (s, u, v, triangle), word 4 the hit's 2 x transform;
 *   2. k_rays_paths<LOCK>: persistent waves refilled as k_paths refills them.  A work item is (ray, sample); items are numbered [block of 64 consecutive rays]
 *      [sample][lane], so that the 64 items a wave draws together are one sample of 64 neighbouring rays: the coherence the caller gave survives.  Every loop trip
 *      is one bounce<false, LOCK>() — one whole iteration of lightTrace, flx_device.h — for every live lane; the loop guard is tested before the first bounce.  A
 *      finished path writes finalColor + importancyFactor * ambient to its own slot (w: the bounce iterations it shaded, as bits), the last sample's path also
 *      its originalColor.  bounce() is given a DeviceFrame of one view that holds the params' seed and ambient;
 *   3. k_rays_resolve: a thread per ray adds the slots in sample order, scales, multiplies by originalColor, adds the bounce counts and writes the radiance row
 *      with two float4 stores.
 * The scratch (hit rows, rays x samples slots, an originalColor per ray) is the context's, grown and never shrunk.  The host cuts a batch into SLABS of rays so
 * that the scratch has a ceiling: flx_trace_slab_rays (flx_query_args.h) — at most 2^24 slots (256 MB) and 2^21 rays a slab, at least 64 rays.  A slab's three
 * launches follow each other on the context's stream, the cursors zeroed in stream order in front of them.  The paths kernel's cursor counts UNITS of 64 items
 * (a block of rays x a sample), of which a slab has fewer than 2^31 + 2^18 whatever n and the sample count: any n a uint32_t holds works at any sample count the
 * memory holds a slab of.  The host waits for nothing — but where the scratch must grow, for the work that may still use it.
 * IN FIRST-HIT ORDER (FLX_TRACE_ORDER_HITS) a slab has its bounds, keys and sort (flx_rays_order.hip) between 1 and 2, and k_rays_paths<LOCK, true> takes the item at
 * position block * 64 + lane for ray order[position]: the 64 items a wave draws together are then 64 rays whose first hits are neighbours in the scene, whatever
 * order the caller's rays came in.  Slots, lastOriginal and the resolve are indexed by the ray's own number, so the rows need no scatter and arrive in the caller's
 * order, bit for bit the unordered call's: a row depends on nothing but its ray row and the scene.
 * The host side around the launches — the params' refusal and the frame bounce() is given, the growth, the producer wait, the slab loop and its first hits, the
 * host-memory call — is the ray-batch calls' shared path (flx_query.hip, flx_rays_host.h). */
#include <cstring>
#include <string>

#define FLX_ANGLE_TABLE 1                  /* k_rays_paths reads the shading's per-triangle table (flx_device.h: one definition per translation unit), as k_paths does at the same four waves per SIMD */
#include "flx_context.h"
#include "flx_kernel_util.h"
#include "flx_query_args.h"
#include "flx_ray_order_args.h"
#include "flx_rays_host.h"

using namespace flx;

namespace flx {

constexpr uint32_t TRACE_CHUNK_UNITS = 4;               /* units a wave draws with one atomic, a unit = the 64 items of one (block of rays, sample): 256 items, k_paths' PATH_CHUNK */
constexpr uint32_t TRACE_WAVES = 4;                    /* waves per SIMD the paths kernel is built for (FLX_PATHS_WAVES: 128 registers) */

struct TraceArgs { DeviceScene sc; DeviceFrame fr; };
static_assert(sizeof(TraceArgs) + 64 <= 4096, "the paths kernel's arguments fit a 4 KB kernarg segment");

/* ORDERED: the item at position block * 64 + (j & 63) names ray order[position] — a slab in first-hit order (flx_rays_order.hip): the 64 items a wave draws
 * together start their paths in one corner of the scene whatever order the caller's rays came in.  Slots, lastOriginal and the resolve stay indexed by the ray's
 * own number: the rows arrive in the caller's order with no scatter pass.  `order` is not read otherwise. */
template <bool LOCK, bool ORDERED = false>
__global__ __launch_bounds__(256, TRACE_WAVES) void k_rays_paths(TraceArgs ta, const float4 *__restrict__ rays, const float4 *__restrict__ hits, float4 *__restrict__ slots,
                                                                 float4 *__restrict__ lastOriginal, uint32_t *__restrict__ queue, uint32_t n, uint32_t units,
                                                                 const uint32_t *__restrict__ order) {
  const DeviceScene &sc = ta.sc;
  const DeviceFrame &fr = ta.fr;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t S = (uint32_t)fr.samples;
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
  auto finishPath = [&]() {                                 /* fragment:598 + what main() needs from the last sample */
    const f3 r = p.finalColor + p.importancyFactor * frame_ambient(fr, 0);
    slots[(size_t)sampleIdx * n + rayIdx] = make_float4(r.x, r.y, r.z, __uint_as_float((uint32_t)bounceIdx));
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
        if (lane == 0) base = atomicAdd(queue, TRACE_CHUNK_UNITS);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= units) { itemsLeft = false; break; }
        chunkUnit = base;
        chunkNext = 0;
        chunkEnd = (units - base > TRACE_CHUNK_UNITS ? TRACE_CHUNK_UNITS : units - base) * 64u;
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
            /* loop guard of fragment:475 before the first bounce (fails only for bounces = 0 or minImportancy > 1) */
            alive = fr.max_reflections > 0 && length(p.importancyFactor * ps.originalColor) >= fr.min_importancy * SQRT3;
            if (!alive) finishPath();
          }
        }
      }
      chunkNext += take;
    }
    if (__ballot(alive) == 0ull) break;

    /* -- one bounce for every live lane (fragment:475-596) ------------------------------------------ */
    if (alive) {
      bool cont = bounce<false, LOCK>(sc, fr, ps, p, origin, cosSampleN, bounceIdx, cnt);
      bounceIdx++;
      if (cont) cont = bounceIdx < fr.max_reflections && length(p.importancyFactor * ps.originalColor) >= fr.min_importancy * SQRT3;
      if (!cont) { finishPath(); alive = false; }
    }
  }
}

/* fragment:608-632 for a ray (flx_kernel_util.h: resolve_pixel), and the row: r g b, 1.0 | s, entry, 2 x transform, bounce iterations — a miss: zeros, entry -1 */
__global__ __launch_bounds__(256) void k_rays_resolve(const float4 *__restrict__ hits, const float4 *__restrict__ slots, const float4 *__restrict__ lastOriginal,
                                                      float4 *__restrict__ out, uint32_t n, int samples) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  const float4 h0 = hits[(size_t)r * 2u], h1 = hits[(size_t)r * 2u + 1u];
  float4 o0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), o1 = make_float4(0.0f, __int_as_float(-1), 0.0f, 0.0f);
  if (__float_as_int(h0.w) != -1) {
    f3 finalColor = F3(0.0f, 0.0f, 0.0f);
    uint32_t shades = 0;
    for (int s = 0; s < samples; s++) {
      const float4 c = slots[(size_t)s * n + r];
      finalColor = finalColor + F3(c.x, c.y, c.z);
      shades += __float_as_uint(c.w);
    }
    const float invSamples = 1.0f / (float)samples;
    finalColor = finalColor * invSamples;
    const float4 oc = lastOriginal[r];
    finalColor = finalColor * F3(oc.x, oc.y, oc.z);
    o0 = make_float4(finalColor.x, finalColor.y, finalColor.z, 1.0f);
    o1 = make_float4(h0.x, h0.w, h1.x, __uint_as_float(shades));
  }
  out[(size_t)r * 2u] = o0;
  out[(size_t)r * 2u + 1u] = o1;
}

}  // namespace flx

/* ---- the calls ------------------------------------------------------------------------------------------------------------------------------------- */

static flx_status fail(flx_context *ctx, flx_status code, const std::string &msg) { return flx_fail(ctx, code, msg.c_str()); }

/* One traced batch, behind both device calls: `call` is flx_rays_trace or flx_rays_trace_ordered, the name every message begins with (the device call's with
 * _device behind it).  order: 0, or FLX_TRACE_ORDER_HITS — per slab bounds, keys and the sort (flx_rays_order.hip) between the first hits and the paths kernel,
 * which then takes its rays through the order. */
static flx_status trace_device(flx_context *ctx, const flx_trace_params *params, const void *d_rays, void *d_radiance, uint32_t n, uint32_t order, void *producer_stream,
                               const char *call) {
  const std::string device_call = std::string(call) + "_device";
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
  flx_status s;
  TraceArgs ta;
  if ((s = flx_make_scene(ctx, ta.sc))) return s;           /* (refuses a scene that names a transform not uploaded) */
  if ((s = flx_server_stop(ctx))) return s;                 /* as flx_render_device: the frame server's launch ends after the frames posted to it */
  flx_trace_frame(params, ta.fr, 0, 0);                     /* no filter, no temporal */
  const uint32_t S = (uint32_t)params->samples;
  const bool ordered = order != 0u;
  flx_ray_slabs cut(ctx, S, n);
  /* the sort's scratch is asked for by an ordered batch alone, in the same growth and behind its one wait */
  if ((s = flx_grow(ctx, flx_need(&ctx->d_trace_hits, (size_t)cut.most * 2u), flx_need(&ctx->d_trace_slots, (size_t)cut.most * S), flx_need(&ctx->d_trace_last, cut.most),
                    flx_need(&ctx->d_trace_ctl, 4), flx_need(ordered ? &ctx->d_order_keys[0] : nullptr, flx_order_room(cut.most)),
                    flx_need(ordered ? &ctx->d_order_keys[1] : nullptr, flx_order_room(cut.most)), flx_need(ordered ? &ctx->d_order_pos[0] : nullptr, flx_order_room(cut.most)),
                    flx_need(ordered ? &ctx->d_order_pos[1] : nullptr, flx_order_room(cut.most)), flx_need(ordered ? &ctx->d_order_counts : nullptr, flx_order_table_room(cut.most)),
                    flx_need(ordered ? &ctx->d_order_ctl : nullptr, 16))))
    return s;
  if ((s = flx_wait_for_producer(ctx, producer_stream))) return s;
  if ((s = flx_angle_table(ctx, ta.sc))) return s;          /* the shading's per-triangle table, made again first where the scene or the transforms changed: FLX_ANGLE_TABLE above makes this file's bounce() read it */
  const bool lock = FLX_LOCKSTEP && ta.sc.lock_entries != 0u;
  const uint32_t cus = (uint32_t)ctx->prop.multiProcessorCount;
  uint32_t blocks = 0, sort_groups = 0;
  /* a slab's launches behind its first hits; of d_trace_ctl's words [2] is the paths kernel's unit cursor */
  s = flx_rays_slabs(ctx, ta.sc, d_rays, n, cut, device_call.c_str(), [&](uint64_t first, uint32_t m, const float4 *rays) -> flx_status {
    float4 *out = (float4 *)d_radiance + first * 2u;
    flx_status so;
    if (ordered && (so = flx_slab_order(ctx, rays, ctx->d_trace_hits.get(), m, &sort_groups))) return so;
    const uint32_t *by = ctx->d_order_pos[0].get();          /* (the unordered kernels do not read it) */
    /* persistent grid: enough workgroups to fill every CU at the kernel's occupancy, no more than the items fill; flx_debug_set_query_groups sets it too.  An
     * ordered slab launches as many: its dead rays sit at the end of the order, where a unit of them costs a wave 64 loads of a hit row's entry */
    const uint32_t units = ((m + 63u) >> 6) * S;              /* (block of 64 rays, sample) pairs: below 2^31 + 2^18 by flx_trace_slab_rays' rule; four fill a workgroup */
    const uint32_t full = (units + 3u) / 4u;
    blocks = ctx->query_groups ? ctx->query_groups : (full < cus * 8u ? full : cus * 8u);
    uint32_t *queue = ctx->d_trace_ctl.get() + 2;
    if (ordered) {
      if (lock) hipLaunchKernelGGL((k_rays_paths<true, true>), dim3(blocks), dim3(256), 0, ctx->stream, ta, rays, ctx->d_trace_hits.get(), ctx->d_trace_slots.get(), ctx->d_trace_last.get(), queue, m, units, by);
      else hipLaunchKernelGGL((k_rays_paths<false, true>), dim3(blocks), dim3(256), 0, ctx->stream, ta, rays, ctx->d_trace_hits.get(), ctx->d_trace_slots.get(), ctx->d_trace_last.get(), queue, m, units, by);
    } else {
      if (lock) hipLaunchKernelGGL((k_rays_paths<true, false>), dim3(blocks), dim3(256), 0, ctx->stream, ta, rays, ctx->d_trace_hits.get(), ctx->d_trace_slots.get(), ctx->d_trace_last.get(), queue, m, units, by);
      else hipLaunchKernelGGL((k_rays_paths<false, false>), dim3(blocks), dim3(256), 0, ctx->stream, ta, rays, ctx->d_trace_hits.get(), ctx->d_trace_slots.get(), ctx->d_trace_last.get(), queue, m, units, by);
    }
    FLX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_rays_resolve, dim3((m + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->d_trace_hits.get(), ctx->d_trace_slots.get(), ctx->d_trace_last.get(), out, m, params->samples);
    FLX_HIP(ctx, hipGetLastError());
    return FLX_OK;
  });
  if (s) return s;
  flx_context::TraceLaunch ran;
  ran.n = n; ran.samples = S; ran.slab = cut.slab; ran.lock = lock ? 1u : 0u;
  ran.slabs = cut.slabs; ran.path_groups = blocks; ran.query_groups = cut.query.groups;
  ctx->last_trace_rays = ran;
  flx_context::OrderLaunch sorted;
  sorted.ordered = ordered ? 1u : 0u; sorted.groups = sort_groups; sorted.passes = ordered ? 4u : 0u; sorted.n = n;
  ctx->last_ray_order = sorted;
  return FLX_OK;
}

extern "C" flx_status flx_rays_trace_device(flx_context *ctx, const flx_trace_params *params, const void *d_rays, void *d_radiance, uint32_t n, void *producer_stream) {
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = flx_trace_params_refused(ctx, params, "flx_rays_trace");      /* (both entry points say flx_rays_trace: here) */
  if (s || n == 0) return s;
  return trace_device(ctx, params, d_rays, d_radiance, n, 0u, producer_stream, "flx_rays_trace");
}

extern "C" flx_status flx_rays_trace(flx_context *ctx, const flx_trace_params *params, const float *rays, void *radiance, uint32_t n) {
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = flx_trace_params_refused(ctx, params, "flx_rays_trace");      /* (both entry points say flx_rays_trace: here) */
  if (s || n == 0) return s;
  if (!rays || !radiance) return fail(ctx, FLX_ERR_INVALID, "flx_rays_trace: an array is NULL");
  return flx_rays_from_host(ctx, rays, n, [&]() { return flx_rays_trace_device(ctx, params, ctx->d_query_rays, ctx->d_query_hits, n, nullptr); },
                            flx_down(&ctx->d_query_hits, (size_t)n * 2u, radiance));
}

/* what both ordered calls refuse before they look at an array: the scene, the params, then a bit of `order` that is none of FLX_TRACE_ORDER_HITS */
static flx_status ordered_refused(flx_context *ctx, const flx_trace_params *params, uint32_t order) {
  flx_status s = flx_trace_params_refused(ctx, params, "flx_rays_trace_ordered");
  if (s) return s;
  if (!flx_order_bits_known(order)) return fail(ctx, FLX_ERR_INVALID, "flx_rays_trace_ordered: order has a bit beyond FLX_TRACE_ORDER_HITS");
  return FLX_OK;
}

extern "C" flx_status flx_rays_trace_ordered_device(flx_context *ctx, const flx_trace_params *params, const void *d_rays, void *d_radiance, uint32_t n, uint32_t order,
                                                    void *producer_stream) {
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = ordered_refused(ctx, params, order);
  if (s || n == 0) return s;
  return trace_device(ctx, params, d_rays, d_radiance, n, order, producer_stream, "flx_rays_trace_ordered");
}

extern "C" flx_status flx_rays_trace_ordered(flx_context *ctx, const flx_trace_params *params, const float *rays, void *radiance, uint32_t n, uint32_t order) {
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = ordered_refused(ctx, params, order);
  if (s || n == 0) return s;
  if (!rays || !radiance) return fail(ctx, FLX_ERR_INVALID, "flx_rays_trace_ordered: an array is NULL");
  return flx_rays_from_host(ctx, rays, n, [&]() { return flx_rays_trace_ordered_device(ctx, params, ctx->d_query_rays, ctx->d_query_hits, n, order, nullptr); },
                            flx_down(&ctx->d_query_hits, (size_t)n * 2u, radiance));
}

extern "C" flx_status flx_debug_set_trace_slab(flx_context *ctx, uint32_t rays) {
  if (!ctx) return FLX_ERR_INVALID;
  ctx->trace_slab = rays;
  return FLX_OK;
}

extern "C" flx_status flx_debug_last_trace(flx_context *ctx, uint32_t out[8]) {
  if (!ctx || !out) return FLX_ERR_INVALID;
  const flx_context::TraceLaunch &t = ctx->last_trace_rays;
  out[0] = t.slabs; out[1] = t.slab; out[2] = t.path_groups; out[3] = t.lock; out[4] = t.n; out[5] = t.samples; out[6] = t.query_groups; out[7] = TRACE_CHUNK_UNITS * 64u;
  return FLX_OK;
}
