/* flx_rays_planes.hip — the denoise chain's five render targets for a caller's rays, and a ray IMAGE traced and denoised (include/flexlight_hip_debug.h, "ray
 * queries": flx_rays_planes[_device], flx_rays_image[_device]).
 *
 * What a frame computes for a pixel with use_filter = 1 and is_temporal = 0 (fragment:601-646), computed for a ray of the caller's own: hit = rayTracer(origin,
 * direction); the shader's globals (firstRayLength, glassFilter, originalRMEx, originalTPOx, renderId; fragment:83-89) initialised once; the samples'
 * lightTrace(hit, direction, origin, cos(float(s)), max_reflections) run IN ORDER ON THAT ONE STATE and added, averaged; then the five targets as fragment_main's
 * filter branch writes them.  The ray's origin stands where a frame has its camera, the row's two noise coordinates where a frame has the pixel's NDC.
 *
 * Because the globals carry from sample to sample, k_rays_paths (flx_rays_trace.hip), whose work items are (ray, sample) pairs, cannot make these planes.  Per slab:
 *   1. first hits: k_ray_query as it stands (flx_query.hip, what = FLX_RAYS_CLOSEST) into the traced batches' hit rows;
 *   2. k_rays_planes<LOCK>: persistent waves; a wave draws a block of 64 CONSECUTIVE rays with one atomic (the caller's coherence survives, as in k_rays_paths), and
 *      A LANE OWNS ONE RAY FOR ALL OF ITS SAMPLES: PixelState stays in registers from the first sample to the stores.  The body is k_trace_pixels' (flx_kernels.hip)
 *      with the hit row where that kernel has its primary walk: the surface at the first hit is shaded once (shadeSurface) and reused by every sample's first bounce
 *      (bounceOn) — all samples share the first hit —, then the inner loop: the guard tested before every bounce, one bounce<false, LOCK>() a trip.  A ray stores
 *      its row of every plane asked for: one 16-byte store per float plane, one 4-byte store per byte plane; plane p starts at row p * n, so the lanes of a block
 *      write contiguous runs.  A miss stores zeros.  A wave finishes its 64 rays together and then draws the next block.
 * Measured against the alternative, on the MI355X (profiles/rays_planes.txt): a form in which a lane went on to its next sample as soon as a path ended and free
 * lanes drew new rays mid-wave once 24 (FLX_WF_BATCH) or 40 of them were free was 20 - 35 % slower than the same form finishing its rays together, and that one
 * 3 - 9 % slower than this body; 5 and 6 waves per SIMD for the build without the lockstep copy (80 - 96 registers, more scratch) lost to 4 as well.
 * bounce() is given a DeviceFrame of one view that holds the params' seed and ambient (flx_query.hip: flx_trace_frame).  The batch is cut into slabs of at most 2^21 rays
 * (flx_trace_slab_rays at one slot a ray); the scratch is hit rows only.  The host waits for nothing — but where the scratch must grow, for the work that may
 * still use it.  The params' refusal, the growth, the producer wait, the slab loop and its first hits and the host-memory calls are the ray-batch calls' shared path
 * (flx_query.hip, flx_rays_host.h).
 *
 * A ray image is those planes (RGBA8) into memory the context owns, then the chain exactly as flx_filter_planes_device launches it.
 *
 * A ray image OVER TIME (flx_rays_image_temporal[_device], "ray images over time") is the same launches with the kernel's temporal instantiations, which run the
 * reference's temporal pass over one of the context's ray-image histories in the lane that owns the ray, then the chain where use_filter == 1. */
#include <cstring>
#include <string>
#include <type_traits>

/* as flx_kernels.hip, whose k_trace_pixels this kernel restates: it shades inline between walks, where the table form of the sin / cos polynomial measures faster
 * (the same floats; here 16.50 against 16.69 ms on the dragon's 1080p rays), and reads the shading's per-triangle table (flx_device.h: one definition per
 * translation unit) */
#define FLX_SINCOS_TABLE 1
#define FLX_ANGLE_TABLE 1
#include "flx_context.h"
#include "flx_kernel_util.h"
#include "flx_query_args.h"
#include "flx_ray_planes_args.h"
#include "flx_ray_temporal_args.h"
#include "flx_rays_host.h"
#include "flx_rays_planes_gather.h"
#include "flx_texel.h"

using namespace flx;

namespace flx {

constexpr uint32_t RAY_PLANES_BLOCK = 64u;             /* consecutive rays a wave draws with one atomic: a ray per lane */
constexpr uint32_t RAY_PLANES_WAVES = 4;               /* waves per SIMD both builds are allocated for: 128 registers + 296 B of scratch a lane (profiles/rays_planes.txt) */

struct RayPlanesArgs { DeviceScene sc; DeviceFrame fr; };
/* What the temporal instantiations are given beside the planes': the history's four rings (colour, colour integer part, location id, original id) — back to back in
 * one allocation, each `depth` planes of `stride` texels —, pointing AT THE SLAB'S FIRST RAY as the outputs do, so that rings[(j * depth + s) * stride + r] is ring j's
 * texel of the ray's index in the image in slot s; packed: the slot that takes the new frame | depth << 8 | hdr << 16.  (One pointer and one word: with four
 * pointers and three words held in scalar registers across the bounces the kernel needed 4 - 16 B more scratch a lane than the planes kernel;
 * profiles/rays_temporal.txt.)  The planes kernel proper is given nothing. */
struct RayTemporalArgs { uint32_t *rings; uint32_t packed; };
enum RayPlanesMode { RAY_PLANES = 0, RAY_TEMPORAL_CANVAS = 1, RAY_TEMPORAL_FILTER = 2 };
struct RayNoArgs {};
template <int MODE> using RayModeArgs = typename std::conditional<MODE != RAY_PLANES, RayTemporalArgs, RayNoArgs>::type;
static_assert(sizeof(RayPlanesArgs) + sizeof(RayTemporalArgs) + 64 <= 4096, "the planes kernel's arguments fit a 4 KB kernarg segment");

/* m: rays of the slab (rays, hits and both outputs point at its first); stride: rows of a plane, the call's n.
 * MODE RAY_TEMPORAL_CANVAS / RAY_TEMPORAL_FILTER (flx_rays_image_temporal_device): fragment_main with is_temporal == 1 and use_filter 0 / 1 (fr.use_filter says the same to bounce()), then the temporal pass of k_temporal_frame
 * (flx_filter.hip) IN THE LANE THAT OWNS THE RAY: it packs its six rows, stores the four texels of the ring's head, reads its own index in the older slots and
 * averages (temporal_texel, flx_texel.h: the pass works on unpack(pack(x)) of the new frame's values).  With the filter the five RGBA8 inputs of the chain go to
 * planes8 as the planes kernel lays them out; without it the canvas colour goes to planes32[r], one float4 a ray.  No float G-buffer, no second pass. */
template <bool LOCK, int MODE>
__global__ __launch_bounds__(256, RAY_PLANES_WAVES) void k_rays_planes(RayPlanesArgs ra, const float4 *__restrict__ rays, const float4 *__restrict__ hits, uint32_t *__restrict__ planes8,
                                                                      float4 *__restrict__ planes32, uint32_t *__restrict__ queue, uint32_t m, size_t stride, RayModeArgs<MODE> th) {
  constexpr bool TEMPORAL = MODE != RAY_PLANES;
  const DeviceScene &sc = ra.sc;
  const DeviceFrame &fr = ra.fr;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t blocks = (m + RAY_PLANES_BLOCK - 1u) / RAY_PLANES_BLOCK;
  /* fragment:475's guard before a sample's first bounce: importancyFactor and originalColor are (1, 1, 1) there for every sample (k_trace_pixels: firstBounce) */
  const bool firstBounce = fr.max_reflections > 0 && length(F3(1.0f, 1.0f, 1.0f) * F3(1.0f, 1.0f, 1.0f)) >= fr.min_importancy * SQRT3;
  WorkCounters cnt = {};
  for (;;) {
    uint32_t b = 0;
    if (lane == 0) b = atomicAdd(queue, 1u);
    b = __builtin_amdgcn_readfirstlane(b);
    if (b >= blocks) break;
    const uint32_t r = b * RAY_PLANES_BLOCK + lane;      /* b < blocks <= 2^15: no overflow */
    if (r < m) {
      float4 color = make_float4(0.f, 0.f, 0.f, 0.f), colorIp = color, origColor = color, rid = color, roid = color;      /* a miss: an uncovered pixel, fragment_main writes nothing */
      uint32_t qc = 0u, qip = 0u, qo = 0u, qrid = 0u, qoid = 0u, qid = 0u;      /* the temporal instantiation's six rows as stored, renderLocationId the sixth */
      const float4 h0 = hits[(size_t)r * 2u];
      Hit hit0;
      hit0.suv = F3(h0.x, h0.y, h0.z);
      hit0.triangleId = __float_as_int(h0.w);
      hit0.transformId = 0;
      if (hit0.triangleId != -1) {
        hit0.transformId = __float_as_int(hits[(size_t)r * 2u + 1u].x);
        const float4 q0 = rays[(size_t)r * 2u], q1 = rays[(size_t)r * 2u + 1u];
        const f3 origin = F3(q0.x, q0.y, q0.z);          /* lightTrace's `camera` */
        const f3 dir0 = F3(q1.x, q1.y, q1.z);            /* as given: rayTracer does not normalise it, lightTrace steps along it by s */
        Ray pr; pr.origin = origin; pr.dir = dir0;
        PixelState ps;
        ps.ndc_x = q0.w; ps.ndc_y = q1.w;
        ps.seed = fr.view[0].random_seed;
        ps.firstRayLength = 1.0f; ps.glassFilter = 0.0f; ps.originalRMEx = 0.0f; ps.originalTPOx = 0.0f;
        ps.originalColor = F3(0.0f, 0.0f, 0.0f);
        ps.renderId.x = ps.renderId.y = ps.renderId.z = ps.renderId.w = 0.0f;
        ps.renderOriginalId = ps.renderId;
        f3 finalColor = F3(0.0f, 0.0f, 0.0f);
        /* every sample's first bounce lands on the first hit: what its shading knows before it draws a random number is computed once (k_trace_pixels) */
        SurfaceCtx sf0;
        WorkCounters sfCnt = {};
        if (firstBounce) shadeSurface<false>(sc, fr, hit0, pr, origin, sf0, sfCnt);
        for (int s = 0; s < fr.samples; s++) {
          float cosSampleN = flx_cos((float)s);
          PathState p;
          p.dontFilter = true;
          p.finalColor = F3(0.0f, 0.0f, 0.0f);
          p.importancyFactor = F3(1.0f, 1.0f, 1.0f);
          ps.originalColor = F3(1.0f, 1.0f, 1.0f);
          p.ray.origin = origin; p.ray.dir = dir0;
          p.lastHitPoint = origin;
          p.hit = hit0;
          bool alive = firstBounce;
          if (firstBounce) alive = bounceOn<false, LOCK>(sc, fr, sf0, ps, p, origin, cosSampleN, 0, cnt);
          for (int i = 1; alive && i < fr.max_reflections && length(p.importancyFactor * ps.originalColor) >= fr.min_importancy * SQRT3; i++) {
            if (!bounce<false, LOCK>(sc, fr, ps, p, origin, cosSampleN, i, cnt)) break;
          }
          finalColor = finalColor + (p.finalColor + p.importancyFactor * frame_ambient(fr, 0));
        }
        /* fragment:614-646, the filter branch */
        const float invSamples = 1.0f / (float)fr.samples;
        finalColor = finalColor * invSamples;
        float ipW = ps.glassFilter;
        if constexpr (TEMPORAL) {
          if (MODE == RAY_TEMPORAL_CANVAS) { finalColor = finalColor * ps.originalColor; ipW = 1.0f; }      /* fragment:632-636, is_temporal == 1 */
        }
        color = make_float4(flx_fract(finalColor.x), flx_fract(finalColor.y), flx_fract(finalColor.z), 1.0f);
        colorIp = make_float4(flx_floor(finalColor.x) * INV_256, flx_floor(finalColor.y) * INV_256, flx_floor(finalColor.z) * INV_256, ipW);
        origColor = make_float4(ps.originalColor.x, ps.originalColor.y, ps.originalColor.z, flx_min(ps.originalRMEx, ps.firstRayLength) + INV_255);
        rid = make_float4(ps.renderId.x, ps.renderId.y, ps.renderId.z, ps.renderId.w + INV_255);
        roid = make_float4(0.0f, 0.0f, 0.0f, ps.originalTPOx + INV_255);
        if constexpr (TEMPORAL) {
          qc = pack_rgba8(color.x, color.y, color.z, color.w); qip = pack_rgba8(colorIp.x, colorIp.y, colorIp.z, colorIp.w);
          qo = pack_rgba8(origColor.x, origColor.y, origColor.z, origColor.w); qrid = pack_rgba8(rid.x, rid.y, rid.z, rid.w); qoid = pack_rgba8(roid.x, roid.y, roid.z, roid.w);
          /* fragment:640-642 as k_trace_pixels writes it: relativePosition in object space, the origin in world space */
          /* the hit row is fetched again, through an index the compiler cannot see through: kept from the first fetch, u, v and the entry would hold three registers
           * through the last sample's bounces, where the kernel has none to spare (the planes kernel lets them go after that sample's first bounce) */
          uint32_t again = r;
          asm volatile("" : "+v"(again));
          const float4 h1 = hits[(size_t)again * 2u];
          const int entry = __float_as_int(h1.w);
          const float4 g0 = sc.geometry[3 * entry], g1 = sc.geometry[3 * entry + 1], g2 = sc.geometry[3 * entry + 2];
          const float w0 = 1.0f - h1.y - h1.z;
          const f3 rel = (F3(g0.x, g0.y, g0.z) * w0 + F3(g0.w, g1.x, g1.y) * h1.y) + F3(g1.z, g1.w, g2.x) * h1.z;
          const float div = 2.0f * distance(rel, origin);
          qid = pack_rgba8(flx_mod(rel.x, div) / div, flx_mod(rel.y, div) / div, flx_mod(rel.z, div) / div, INV_255);
        }
      }
      if constexpr (TEMPORAL) {
        const uint32_t th_head = th.packed & 255u, th_depth = (th.packed >> 8) & 255u;
        const int th_hdr = (int)(th.packed >> 16);
        const size_t ringT = (size_t)th_depth * stride;      /* texels of a ring */
        uint32_t *const ring_0 = th.rings, *const ring_1 = ring_0 + ringT, *const ring_2 = ring_1 + ringT, *const ring_3 = ring_2 + ringT;
        const size_t head = (size_t)th_head * stride + r;
        ring_0[head] = qc; ring_1[head] = qip; ring_2[head] = qid; ring_3[head] = qoid;
        if (MODE == RAY_TEMPORAL_FILTER) {     /* the three targets the pass hands on as they are */
          uint32_t *o = planes8 + r;
          o[2u * stride] = qo;
          o[3u * stride] = qrid;
          o[4u * stride] = qoid;
        }
        f3 avg; float glassFilter, centerW;
        temporal_texel(qc, qip, qid, qoid, (int)th_depth, [&](int k, uint32_t &c, uint32_t &ip, uint32_t &id, uint32_t &oid) {
          uint32_t slot = th_head + (uint32_t)k;             /* head, k < depth */
          if (slot >= th_depth) slot -= th_depth;
          const size_t at = (size_t)slot * stride + r;
          c = ring_0[at]; ip = ring_1[at]; id = ring_2[at]; oid = ring_3[at];
        }, avg, glassFilter, centerW);
        if (MODE == RAY_TEMPORAL_FILTER) {
          uint32_t *o = planes8 + r;
          o[0] = temporal_color_texel(avg, centerW);
          o[stride] = temporal_ip_texel(avg, glassFilter);
        } else {
          planes32[r] = temporal_canvas(avg, centerW, th_hdr);
        }
        continue;
      }
      if (planes32) {
        float4 *o = planes32 + r;
        o[0] = color; o[stride] = colorIp; o[2u * stride] = origColor; o[3u * stride] = rid; o[4u * stride] = roid;
      }
      if (planes8) {
        uint32_t *o = planes8 + r;
        o[0] = pack_rgba8(color.x, color.y, color.z, color.w);
        o[stride] = pack_rgba8(colorIp.x, colorIp.y, colorIp.z, colorIp.w);
        o[2u * stride] = pack_rgba8(origColor.x, origColor.y, origColor.z, origColor.w);
        o[3u * stride] = pack_rgba8(rid.x, rid.y, rid.z, rid.w);
        o[4u * stride] = pack_rgba8(roid.x, roid.y, roid.z, roid.w);
      }
    }
  }
}

}  // namespace flx

/* ---- the calls ------------------------------------------------------------------------------------------------------------------------------------- */

static flx_status fail(flx_context *ctx, flx_status code, const char *msg) { return flx_fail(ctx, code, msg); }
static flx_status fail(flx_context *ctx, flx_status code, const std::string &msg) { return flx_fail(ctx, code, msg.c_str()); }

/* a refusal of flx_ray_planes_args.h in words */
static flx_status planes_refusal(flx_context *ctx, enum flx_ray_planes_refusal why, const char *call) {
  const char *what = "";
  switch (why) {
    case FLX_RAY_PLANES_ARGS_OK: return FLX_OK;
    case FLX_RAY_PLANES_NONE: what = "planes8 and planes32 are both NULL: no plane is asked for"; break;
    case FLX_RAY_PLANES_SIZE: what = "width or height is 0"; break;
    case FLX_RAY_PLANES_PIXELS: what = "width * height is 2^32 or more"; break;
    case FLX_RAY_PLANES_NULL: what = "an array is NULL"; break;
    case FLX_RAY_PLANES_WRAPS: what = "the rows leave the address space"; break;
    case FLX_RAY_PLANES_OVERLAP_RAYS: what = "the rays and an output overlap"; break;
    case FLX_RAY_PLANES_OVERLAP_OUT: what = "planes8 and planes32 overlap"; break;
  }
  return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": " + what);
}

template <bool LOCK, int MODE>
static void planes_launch(uint32_t groups, hipStream_t stream, const RayPlanesArgs &ra, const float4 *rays, const float4 *hits, uint32_t *out8, float4 *out32, uint32_t *queue, uint32_t m,
                          size_t stride, const RayModeArgs<MODE> &th) {
  hipLaunchKernelGGL((k_rays_planes<LOCK, MODE>), dim3(groups), dim3(256), 0, stream, ra, rays, hits, out8, out32, queue, m, stride, th);
}

/* A temporal image's history, keyed and rotated for an accepted call (everything that can refuse it is behind): a history of another size or depth starts afresh,
 * zero planes and head 0, as a resize does for frames; then the oldest slot becomes the head.  width * height = the call's n. */
static flx_status history_advance(flx_context *ctx, flx_context::RayHistory &h, uint32_t width, uint32_t height, int depth) {
  if (!flx_ray_history_continues(&h.at, width, height, depth)) {
    const size_t texels = (size_t)flx_ray_history_texels(width, height, depth);
    FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));          /* (an earlier image may still use the rings that are about to go) */
    h.at.n = 0;                                               /* (re)allocation in progress: a failure below leaves no key to match */
    flx_status s;
    if ((s = h.rings.release(ctx)) || (s = h.rings.ensure(ctx, texels))) return s;
    FLX_HIP(ctx, hipMemsetAsync(h.rings, 0, texels * sizeof(uint32_t), ctx->stream));
  }
  h.at = flx_ray_history_advance(h.at, width, height, depth);
  return FLX_OK;
}

/* The slabs' launches, the arguments accepted: the five planes of n > 0 rays into d_planes8 and / or d_planes32.  With `temporal` (and the image's width): the
 * temporal instantiation over that history, the chain's five inputs into d_planes8 (use_filter == 1) or the canvas colours into d_planes32, float4[n].  With `volume`
 * ("ray images with a volume"), accepted: the same launches of k_rays_planes_gather (flx_rays_planes_gather.hip) */
static flx_status planes_enqueue(flx_context *ctx, const flx_trace_params *params, const void *d_rays, uint32_t n, void *d_planes8, void *d_planes32, void *producer_stream,
                                 const char *call, const flx_ray_temporal *temporal = nullptr, uint32_t width = 0u, const flx_planes_volume *volume = nullptr) {
  flx_status s;
  RayPlanesArgs ra;
  if ((s = flx_make_scene(ctx, ra.sc))) return s;           /* (refuses a scene that names a transform not uploaded) */
  if ((s = flx_server_stop(ctx))) return s;                 /* as flx_render_device: the frame server's launch ends after the frames posted to it */
  flx_trace_frame(params, ra.fr, temporal ? temporal->use_filter : 1, temporal ? 1 : 0);
  flx_ray_slabs cut(ctx, 1u, n);
  if ((s = flx_grow(ctx, flx_need(&ctx->d_trace_hits, (size_t)cut.most * 2u), flx_need(&ctx->d_trace_ctl, 4)))) return s;
  if ((s = flx_wait_for_producer(ctx, producer_stream))) return s;
  if ((s = flx_angle_table(ctx, ra.sc))) return s;          /* the shading's per-triangle table, made again first where the scene or the transforms changed */
  const bool lock = FLX_LOCKSTEP && ra.sc.lock_entries != 0u;
  const uint32_t cus = (uint32_t)ctx->prop.multiProcessorCount;
  flx_context::RayHistory *history = nullptr;
  if (temporal) {
    history = &ctx->ray_history[temporal->history];
    if ((s = history_advance(ctx, *history, width, n / width, flx_ray_temporal_depth(temporal->temporal_samples)))) return s;
  }
  uint32_t groups = 0;
  /* a slab's launch behind its first hits; of d_trace_ctl's words [2] is the planes kernel's block cursor */
  s = flx_rays_slabs(ctx, ra.sc, d_rays, n, cut, call, [&](uint64_t first, uint32_t m, const float4 *rays) -> flx_status {
    uint32_t *out8 = d_planes8 ? (uint32_t *)d_planes8 + first : nullptr;
    float4 *out32 = d_planes32 ? (float4 *)d_planes32 + first : nullptr;
    /* persistent grid: enough workgroups to fill every CU at the kernel's occupancy, no more than the blocks of rays fill; flx_debug_set_query_groups sets it too */
    const uint32_t full = (((m + RAY_PLANES_BLOCK - 1u) / RAY_PLANES_BLOCK) + 3u) / 4u;
    groups = ctx->query_groups ? ctx->query_groups : (full < cus * 8u ? full : cus * 8u);
    uint32_t *queue = ctx->d_trace_ctl.get() + 2;
    const float4 *hits = ctx->d_trace_hits.get();
    if (volume) {
      const int mode = !history ? RAY_PLANES : temporal->use_filter == 1 ? RAY_TEMPORAL_FILTER : RAY_TEMPORAL_CANVAS;
      uint32_t *rings = history ? history->rings.get() + first : nullptr;      /* as th below */
      const uint32_t packed = history ? (uint32_t)history->at.head | ((uint32_t)history->at.n << 8) | ((uint32_t)temporal->hdr << 16) : 0u;
      return flx_planes_gather_launch(ctx, lock, mode, groups, ra.sc, ra.fr, rays, hits, out8, out32, queue, m, (size_t)n, rings, packed, *volume);
    }
    if (history) {
      RayTemporalArgs th;
      th.rings = history->rings.get() + first;              /* the ray's index in the IMAGE: first + its index in the slab */
      th.packed = (uint32_t)history->at.head | ((uint32_t)history->at.n << 8) | ((uint32_t)temporal->hdr << 16);
      if (temporal->use_filter == 1) {
        if (lock) planes_launch<true, RAY_TEMPORAL_FILTER>(groups, ctx->stream, ra, rays, hits, out8, out32, queue, m, (size_t)n, th);
        else planes_launch<false, RAY_TEMPORAL_FILTER>(groups, ctx->stream, ra, rays, hits, out8, out32, queue, m, (size_t)n, th);
      } else {
        if (lock) planes_launch<true, RAY_TEMPORAL_CANVAS>(groups, ctx->stream, ra, rays, hits, out8, out32, queue, m, (size_t)n, th);
        else planes_launch<false, RAY_TEMPORAL_CANVAS>(groups, ctx->stream, ra, rays, hits, out8, out32, queue, m, (size_t)n, th);
      }
    } else {
      if (lock) planes_launch<true, RAY_PLANES>(groups, ctx->stream, ra, rays, hits, out8, out32, queue, m, (size_t)n, RayNoArgs());
      else planes_launch<false, RAY_PLANES>(groups, ctx->stream, ra, rays, hits, out8, out32, queue, m, (size_t)n, RayNoArgs());
    }
    FLX_HIP(ctx, hipGetLastError());
    return FLX_OK;
  });
  if (s) return s;
  if (volume) flx_planes_gather_ran(ctx, n, cut.slabs, cut.slab);
  if (history) {
    flx_context::RayTemporalLaunch &t = ctx->last_ray_temporal;
    t.slabs = cut.slabs; t.slab = cut.slab; t.depth = (uint32_t)history->at.n; t.history = (uint32_t)temporal->history; t.n = n; t.samples = (uint32_t)params->samples;
    t.head = (uint32_t)history->at.head; t.fused = 1u;      /* the temporal pass ran inside the planes kernel */
    return FLX_OK;
  }
  flx_context::RayPlanesLaunch ran;
  ran.n = n; ran.samples = (uint32_t)params->samples; ran.slab = cut.slab; ran.lock = lock ? 1u : 0u;
  ran.slabs = cut.slabs; ran.groups = groups; ran.query_groups = cut.query.groups;
  ctx->last_ray_planes = ran;
  return FLX_OK;
}

/* flx_rays_planes_device, and with `gather` flx_rays_planes_gather_device: the volume's refusals behind the arrays', its overlap with them last */
static flx_status planes_device(flx_context *ctx, const flx_trace_params *params, bool gather, const flx_gather_volume *volume, const void *d_rays, uint32_t n, void *d_planes8,
                                void *d_planes32, void *producer_stream, const char *call) {
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = flx_trace_params_refused(ctx, params, call);
  if (s || n == 0) return s;
  const enum flx_ray_planes_refusal arrays = flx_ray_planes_arrays_check((uint64_t)(uintptr_t)d_rays, (uint64_t)(uintptr_t)d_planes8, (uint64_t)(uintptr_t)d_planes32, n);
  const bool overlap = arrays == FLX_RAY_PLANES_OVERLAP_RAYS || arrays == FLX_RAY_PLANES_OVERLAP_OUT;      /* (said after the pointers are known to be the device's) */
  if (arrays != FLX_RAY_PLANES_ARGS_OK && !overlap) return planes_refusal(ctx, arrays, call);
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  if (!flx_rows_on_device(ctx, d_rays, (size_t)n * FLX_RAY_ROW_BYTES))
    return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": the rays are not n rows in memory of the context's device, 16-byte aligned");
  if (d_planes8 && !flx_rows_on_device(ctx, d_planes8, (size_t)n * FLX_RAY_PLANES * FLX_RAY_PLANES_ROW8))
    return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": planes8 is not 5 n texels in memory of the context's device, 16-byte aligned");
  if (d_planes32 && !flx_rows_on_device(ctx, d_planes32, (size_t)n * FLX_RAY_PLANES * FLX_RAY_PLANES_ROW32))
    return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": planes32 is not 5 n rows in memory of the context's device, 16-byte aligned");
  if (overlap) return planes_refusal(ctx, arrays, call);
  if (!gather) return planes_enqueue(ctx, params, d_rays, n, d_planes8, d_planes32, producer_stream, call);
  flx_planes_gather_array mine[FLX_PLANES_GATHER_CALL_ARRAYS];
  const int kc = flx_planes_gather_planes_arrays((uint64_t)(uintptr_t)d_rays, (uint64_t)(uintptr_t)d_planes8, (uint64_t)(uintptr_t)d_planes32, n, mine);
  flx_planes_volume pv;
  if ((s = flx_planes_gather_volume_refused(ctx, volume, mine, kc, call, &pv))) return s;
  return planes_enqueue(ctx, params, d_rays, n, d_planes8, d_planes32, producer_stream, call, nullptr, 0u, &pv);
}

extern "C" flx_status flx_rays_planes_device(flx_context *ctx, const flx_trace_params *params, const void *d_rays, uint32_t n, void *d_planes8, void *d_planes32,
                                             void *producer_stream) {
  return planes_device(ctx, params, false, nullptr, d_rays, n, d_planes8, d_planes32, producer_stream, "flx_rays_planes_device");
}

extern "C" flx_status flx_rays_planes_gather_device(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume, const void *d_rays, uint32_t n,
                                                    void *d_planes8, void *d_planes32, void *producer_stream) {
  return planes_device(ctx, params, true, volume, d_rays, n, d_planes8, d_planes32, producer_stream, "flx_rays_planes_gather_device");
}

/* flx_rays_planes, and with `gather` flx_rays_planes_gather: host rays and planes, the volume's arrays on the device */
static flx_status planes_host(flx_context *ctx, const flx_trace_params *params, bool gather, const flx_gather_volume *volume, const float *rays, uint32_t n, void *planes8,
                              void *planes32, const char *call) {
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = flx_trace_params_refused(ctx, params, call);
  if (s || n == 0) return s;
  if (!planes8 && !planes32) return planes_refusal(ctx, FLX_RAY_PLANES_NONE, call);
  if (!rays) return planes_refusal(ctx, FLX_RAY_PLANES_NULL, call);
  const size_t rows = (size_t)n * FLX_RAY_PLANES;
  if (gather && (s = flx_planes_gather_volume_refused(ctx, volume, nullptr, 0, call, nullptr))) return s;      /* (before anything is staged) */
  return flx_rays_from_host(ctx, rays, n, [&]() {
    void *d8 = planes8 ? ctx->d_ray_planes.get() : nullptr, *d32 = planes32 ? ctx->d_query_hits.get() : nullptr;
    return gather ? planes_device(ctx, params, true, volume, ctx->d_query_rays, n, d8, d32, nullptr, call)
                  : flx_rays_planes_device(ctx, params, ctx->d_query_rays, n, d8, d32, nullptr);
  }, flx_down(&ctx->d_ray_planes, rows, planes8), flx_down(&ctx->d_query_hits, rows, planes32));
}

extern "C" flx_status flx_rays_planes(flx_context *ctx, const flx_trace_params *params, const float *rays, uint32_t n, void *planes8, void *planes32) {
  return planes_host(ctx, params, false, nullptr, rays, n, planes8, planes32, "flx_rays_planes");
}

extern "C" flx_status flx_rays_planes_gather(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume, const float *rays, uint32_t n, void *planes8,
                                             void *planes32) {
  return planes_host(ctx, params, true, volume, rays, n, planes8, planes32, "flx_rays_planes_gather");
}

/* Both image calls behind their own refusals: the arrays of n = width * height rays, the planes, the chain.  temporal NULL: flx_rays_image_device, which has its hdr
 * beside the params; else the image over that history, the hdr the history's. */
static flx_status image_enqueue(flx_context *ctx, const flx_trace_params *params, const flx_ray_temporal *temporal, int hdr, const void *d_rays, uint32_t width, uint32_t height,
                                uint32_t n, void *d_out_rgba, void *producer_stream, const char *call, bool gather = false, const flx_gather_volume *gather_volume = nullptr) {
  const enum flx_ray_planes_refusal arrays = flx_ray_image_arrays_check((uint64_t)(uintptr_t)d_rays, (uint64_t)(uintptr_t)d_out_rgba, n);
  if (arrays != FLX_RAY_PLANES_ARGS_OK && arrays != FLX_RAY_PLANES_OVERLAP_RAYS) return planes_refusal(ctx, arrays, call);
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  if (!flx_rows_on_device(ctx, d_rays, (size_t)n * FLX_RAY_ROW_BYTES))
    return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": the rays are not width * height rows in memory of the context's device, 16-byte aligned");
  if (!flx_rows_on_device(ctx, d_out_rgba, (size_t)n * FLX_RAY_PLANES_ROW32))
    return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": the image is not width * height float4 in memory of the context's device, 16-byte aligned");
  if (arrays == FLX_RAY_PLANES_OVERLAP_RAYS) return planes_refusal(ctx, arrays, call);
  flx_status s;
  flx_planes_volume pv;
  const flx_planes_volume *volume = nullptr;      /* "ray images with a volume": the volume's refusals behind the arrays', its overlap with them last */
  if (gather) {
    flx_planes_gather_array mine[FLX_PLANES_GATHER_CALL_ARRAYS];
    const int kc = flx_planes_gather_image_arrays((uint64_t)(uintptr_t)d_rays, (uint64_t)(uintptr_t)d_out_rgba, n, mine);
    if ((s = flx_planes_gather_volume_refused(ctx, gather_volume, mine, kc, call, &pv))) return s;
    volume = &pv;
  }
  if (temporal && temporal->use_filter != 1)      /* the canvas colour of the temporal pass, straight from the kernel */
    return planes_enqueue(ctx, params, d_rays, n, nullptr, d_out_rgba, producer_stream, call, temporal, width, volume);
  if ((s = flx_grow(ctx, flx_need(&ctx->d_ray_planes, (size_t)n * FLX_RAY_PLANES)))) return s;      /* (an earlier image's chain may still read the planes that are about to go) */
  if ((s = planes_enqueue(ctx, params, d_rays, n, ctx->d_ray_planes.get(), nullptr, producer_stream, call, temporal, width, volume))) return s;
  /* the chain reads width, height and hdr of a frame's params, nothing of a camera: frame-0 texture state, as flx_filter_planes_device starts it (with a history:
   * dColor, dIp, dOColor, dId and dOId feed it as for a ray image) */
  flx_frame_params image;
  memset(&image, 0, sizeof image);
  image.width = width; image.height = height; image.hdr = hdr;
  return flx_filter_planes_enqueue(ctx, &image, ctx->d_ray_planes.get(), d_out_rgba, true);
}

static flx_status image_device(flx_context *ctx, const flx_trace_params *params, bool gather, const flx_gather_volume *volume, int hdr, const void *d_rays, uint32_t width,
                               uint32_t height, void *d_out_rgba, void *producer_stream, const char *call) {
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = flx_trace_params_refused(ctx, params, call);
  if (s) return s;
  uint32_t n = 0;
  if ((s = planes_refusal(ctx, flx_ray_image_size_check(width, height, &n), call))) return s;
  return image_enqueue(ctx, params, nullptr, hdr, d_rays, width, height, n, d_out_rgba, producer_stream, call, gather, volume);
}

extern "C" flx_status flx_rays_image_device(flx_context *ctx, const flx_trace_params *params, int hdr, const void *d_rays, uint32_t width, uint32_t height, void *d_out_rgba,
                                            void *producer_stream) {
  return image_device(ctx, params, false, nullptr, hdr, d_rays, width, height, d_out_rgba, producer_stream, "flx_rays_image_device");
}

extern "C" flx_status flx_rays_image_gather_device(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume, int hdr, const void *d_rays, uint32_t width,
                                                   uint32_t height, void *d_out_rgba, void *producer_stream) {
  return image_device(ctx, params, true, volume, hdr, d_rays, width, height, d_out_rgba, producer_stream, "flx_rays_image_gather_device");
}

static flx_status image_host(flx_context *ctx, const flx_trace_params *params, bool gather, const flx_gather_volume *volume, int hdr, const float *rays, uint32_t width,
                             uint32_t height, float *out_rgba, const char *call) {
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = flx_trace_params_refused(ctx, params, call);
  if (s) return s;
  uint32_t n = 0;
  if ((s = planes_refusal(ctx, flx_ray_image_size_check(width, height, &n), call))) return s;
  if (!rays || !out_rgba) return planes_refusal(ctx, FLX_RAY_PLANES_NULL, call);
  if (gather && (s = flx_planes_gather_volume_refused(ctx, volume, nullptr, 0, call, nullptr))) return s;      /* (before anything is staged) */
  return flx_rays_from_host(ctx, rays, n, [&]() { return image_device(ctx, params, gather, volume, hdr, ctx->d_query_rays, width, height, ctx->d_query_hits, nullptr, call); },
                            flx_down(&ctx->d_query_hits, n, out_rgba));
}

extern "C" flx_status flx_rays_image(flx_context *ctx, const flx_trace_params *params, int hdr, const float *rays, uint32_t width, uint32_t height, float *out_rgba) {
  return image_host(ctx, params, false, nullptr, hdr, rays, width, height, out_rgba, "flx_rays_image");
}

extern "C" flx_status flx_rays_image_gather(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume, int hdr, const float *rays, uint32_t width,
                                            uint32_t height, float *out_rgba) {
  return image_host(ctx, params, true, volume, hdr, rays, width, height, out_rgba, "flx_rays_image_gather");
}

/* a refusal of flx_ray_temporal_args.h in words */
static flx_status temporal_refusal(flx_context *ctx, enum flx_ray_temporal_refusal why, const char *call) {
  const char *what = "";
  switch (why) {
    case FLX_RAY_TEMPORAL_ARGS_OK: return FLX_OK;
    case FLX_RAY_TEMPORAL_NULL: what = "temporal is NULL"; break;
    case FLX_RAY_TEMPORAL_HISTORY: what = "history is not one of 0 .. 7"; break;
    case FLX_RAY_TEMPORAL_USE_FILTER: what = "use_filter is neither 0 nor 1"; break;
    case FLX_RAY_TEMPORAL_HDR: what = "hdr is neither 0 nor 1"; break;
    case FLX_RAY_TEMPORAL_RESET: what = "history is not one of -1 .. 7"; break;
  }
  return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": " + what);
}
static_assert(FLX_RAY_HISTORIES == FLX_RAY_TEMPORAL_HISTORIES, "the header's histories are the context's");

static flx_status temporal_device(flx_context *ctx, const flx_trace_params *params, bool gather, const flx_gather_volume *volume, const flx_ray_temporal *temporal,
                                  const void *d_rays, uint32_t width, uint32_t height, void *d_out_rgba, void *producer_stream, const char *call) {
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = flx_trace_params_refused(ctx, params, call);
  if (s) return s;
  uint32_t n = 0;
  if ((s = planes_refusal(ctx, flx_ray_image_size_check(width, height, &n), call))) return s;
  if ((s = temporal_refusal(ctx, flx_ray_temporal_check(temporal != nullptr, temporal ? temporal->history : 0, temporal ? temporal->use_filter : 0, temporal ? temporal->hdr : 0), call)))
    return s;
  return image_enqueue(ctx, params, temporal, temporal->hdr, d_rays, width, height, n, d_out_rgba, producer_stream, call, gather, volume);
}

extern "C" flx_status flx_rays_image_temporal_device(flx_context *ctx, const flx_trace_params *params, const flx_ray_temporal *temporal, const void *d_rays, uint32_t width,
                                                     uint32_t height, void *d_out_rgba, void *producer_stream) {
  return temporal_device(ctx, params, false, nullptr, temporal, d_rays, width, height, d_out_rgba, producer_stream, "flx_rays_image_temporal_device");
}

extern "C" flx_status flx_rays_image_temporal_gather_device(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume, const flx_ray_temporal *temporal,
                                                            const void *d_rays, uint32_t width, uint32_t height, void *d_out_rgba, void *producer_stream) {
  return temporal_device(ctx, params, true, volume, temporal, d_rays, width, height, d_out_rgba, producer_stream, "flx_rays_image_temporal_gather_device");
}

static flx_status temporal_host(flx_context *ctx, const flx_trace_params *params, bool gather, const flx_gather_volume *volume, const flx_ray_temporal *temporal, const float *rays,
                                uint32_t width, uint32_t height, float *out_rgba, const char *call) {
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = flx_trace_params_refused(ctx, params, call);
  if (s) return s;
  uint32_t n = 0;
  if ((s = planes_refusal(ctx, flx_ray_image_size_check(width, height, &n), call))) return s;
  if ((s = temporal_refusal(ctx, flx_ray_temporal_check(temporal != nullptr, temporal ? temporal->history : 0, temporal ? temporal->use_filter : 0, temporal ? temporal->hdr : 0), call)))
    return s;
  if (!rays || !out_rgba) return planes_refusal(ctx, FLX_RAY_PLANES_NULL, call);
  if (gather && (s = flx_planes_gather_volume_refused(ctx, volume, nullptr, 0, call, nullptr))) return s;      /* (before anything is staged) */
  return flx_rays_from_host(ctx, rays, n, [&]() { return temporal_device(ctx, params, gather, volume, temporal, ctx->d_query_rays, width, height, ctx->d_query_hits, nullptr, call); },
                            flx_down(&ctx->d_query_hits, n, out_rgba));
}

extern "C" flx_status flx_rays_image_temporal(flx_context *ctx, const flx_trace_params *params, const flx_ray_temporal *temporal, const float *rays, uint32_t width, uint32_t height,
                                              float *out_rgba) {
  return temporal_host(ctx, params, false, nullptr, temporal, rays, width, height, out_rgba, "flx_rays_image_temporal");
}

extern "C" flx_status flx_rays_image_temporal_gather(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume, const flx_ray_temporal *temporal,
                                                     const float *rays, uint32_t width, uint32_t height, float *out_rgba) {
  return temporal_host(ctx, params, true, volume, temporal, rays, width, height, out_rgba, "flx_rays_image_temporal_gather");
}

extern "C" flx_status flx_rays_history_reset(flx_context *ctx, int history) {
  static const char *const call = "flx_rays_history_reset";
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = temporal_refusal(ctx, flx_ray_history_reset_check(history), call);
  if (s) return s;
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));          /* (an image in flight may still use the rings) */
  for (int h = 0; h < FLX_RAY_TEMPORAL_HISTORIES; h++) {
    if (history != -1 && history != h) continue;
    flx_context::RayHistory &one = ctx->ray_history[h];
    one.at = flx_ray_history_state{ 0u, 0u, 0, 0 };
    if ((s = one.rings.release(ctx))) return s;
  }
  return FLX_OK;
}

extern "C" flx_status flx_debug_last_ray_temporal(flx_context *ctx, uint32_t out[8]) {
  if (!ctx || !out) return FLX_ERR_INVALID;
  const flx_context::RayTemporalLaunch &t = ctx->last_ray_temporal;
  out[0] = t.slabs; out[1] = t.slab; out[2] = t.depth; out[3] = t.history; out[4] = t.n; out[5] = t.samples; out[6] = t.head; out[7] = t.fused;
  return FLX_OK;
}

extern "C" flx_status flx_debug_last_ray_planes(flx_context *ctx, uint32_t out[8]) {
  if (!ctx || !out) return FLX_ERR_INVALID;
  const flx_context::RayPlanesLaunch &t = ctx->last_ray_planes;
  out[0] = t.slabs; out[1] = t.slab; out[2] = t.groups; out[3] = t.lock; out[4] = t.n; out[5] = t.samples; out[6] = t.query_groups; out[7] = RAY_PLANES_BLOCK;
  return FLX_OK;
}
