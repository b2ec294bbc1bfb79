/* flx_rays_planes_gather.hip — the five filter planes of a caller's rays, and with them ray images and ray images over time, whose every sample ends in a probe volume
 * (include/flexlight_hip_debug.h, "ray images with a volume").  The definition is include/flx_gather.h's: sample s of a ray contributes finalColor_s +
 * importancyFactor_s * A_s where flx_rays_planes adds finalColor_s + importancyFactor_s * ambient; A_s is the volume's irradiance at the sample's last point times the
 * caller's gain, the params' ambient where the volume has nothing to say or the sample shaded nothing.
 *
 * THE LOOKUP IS INLINE.  k_rays_planes (flx_rays_planes.hip) gives a lane one ray for all of its samples, and after a sample's bounce loop the wave is back together:
 * every lane with a first hit is there, and of the sample's PathState only finalColor, importancyFactor and the ray origin are still wanted, beside three floats of
 * normal.  So the corner loop (flx_gather_corners.h: flx_volume.hip's, a row at a time) runs right there, dense — no path records, no second kernel, no slots beyond
 * the hit rows, and the slab rule stays the planes calls' one slot a ray: a 1080p image is one slab.  (flx_rays_gather.hip, whose lanes finish at different trips,
 * had to defer it: five slots a sample, five slabs for the same image.)
 *
 * k_rays_planes_gather<LOCK, MODE, MAP, OFFSETS> is k_rays_planes<LOCK, MODE> to the statement in all three modes, with two differences:
 *   1. bounces after the first go through the pieces bounce() is made of (flx_device.h: shadeSurface + shadeSample, walkBounce, bounceFinish), as
 *      k_rays_paths_gather calls them, so that the iteration's smooth normal facing the ray outlives it; the first bounce's is sf0.smoothNormal of the shared first hit;
 *   2. the sample's last statement: the lookup at (p.ray.origin, that normal) — the ray origin of the last iteration the sample shaded, which the walk leaves alone —,
 *      flx_gather_ambient, flx_gather_path_value.
 * Whether a sample has a last point is wave-uniform: it shades its first hit or (max_reflections == 0, min_importancy > 1) nothing at all.
 * The host side is flx_rays_planes.hip's own — planes_enqueue, image_enqueue, history_advance take the volume and launch this kernel through
 * flx_planes_gather_launch below where they launch k_rays_planes without one; the camera calls are flx_camera.hip's.  Here: the kernel, its launch, the volume's
 * refusals.  Registers, scratch and timings against the plain image with one bounce more: profiles/rays_planes_gather.txt. */
#include <cstring>
#include <string>
#include <type_traits>

/* as flx_rays_planes.hip, whose kernel this one restates */
#define FLX_SINCOS_TABLE 1
#define FLX_ANGLE_TABLE 1
#include "flx_context.h"
#include "flx_gather.h"
#include "flx_gather_corners.h"
#include "flx_kernel_util.h"
#include "flx_planes_gather_args.h"
#include "flx_query_args.h"
#include "flx_ray_planes_args.h"
#include "flx_ray_temporal_args.h"
#include "flx_rays_planes_gather.h"
#include "flx_texel.h"
#include "flx_volume_args.h"
#include "flx_volume_map_host.h"

using namespace flx;

namespace flx {

constexpr uint32_t PLANES_GATHER_BLOCK = 64u;          /* k_rays_planes' RAY_PLANES_BLOCK: consecutive rays a wave draws with one atomic */
constexpr uint32_t PLANES_GATHER_WAVES = 4;            /* k_rays_planes' RAY_PLANES_WAVES */

struct PlanesGatherArgs { DeviceScene sc; DeviceFrame fr; };                                  /* k_rays_planes' RayPlanesArgs */
struct PlanesGatherTemporal { uint32_t *rings; uint32_t packed; };                            /* k_rays_planes' RayTemporalArgs */
enum PlanesGatherMode { GATHER_PLANES = 0, GATHER_TEMPORAL_CANVAS = 1, GATHER_TEMPORAL_FILTER = 2 };      /* k_rays_planes' RayPlanesMode */
struct PlanesGatherNoArgs {};
template <int MODE> using PlanesGatherModeArgs = typename std::conditional<MODE != GATHER_PLANES, PlanesGatherTemporal, PlanesGatherNoArgs>::type;
/* the volume beside them: the arrays as flx_volume.hip's kernels take them, the grid, the map, the gain */
struct PlanesGatherVolume { const float4 *sh, *maps, *offsets; flx_volume_grid g; flx_volume_map map; float gain; };
static_assert(sizeof(PlanesGatherArgs) + sizeof(PlanesGatherTemporal) + sizeof(PlanesGatherVolume) + 64 <= 4096, "the kernel's arguments fit a 4 KB kernarg segment");

/* k_rays_planes (flx_rays_planes.hip says what every argument is) with the volume `va`: maps and map are not read without MAP, offsets not without OFFSETS */
template <bool LOCK, int MODE, bool MAP, bool OFFSETS>
__global__ __launch_bounds__(256, PLANES_GATHER_WAVES) void k_rays_planes_gather(PlanesGatherArgs ra, const float4 *__restrict__ rays, const float4 *__restrict__ hits,
                                                                                uint32_t *__restrict__ planes8, float4 *__restrict__ planes32, uint32_t *__restrict__ queue,
                                                                                uint32_t m, size_t stride, PlanesGatherModeArgs<MODE> th, PlanesGatherVolume va) {
  constexpr bool TEMPORAL = MODE != GATHER_PLANES;
  const DeviceScene &sc = ra.sc;
  const DeviceFrame &fr = ra.fr;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t blocks = (m + PLANES_GATHER_BLOCK - 1u) / PLANES_GATHER_BLOCK;
  /* fragment:475's guard before a sample's first bounce: importancyFactor and originalColor are (1, 1, 1) there for every sample (k_trace_pixels: firstBounce).
   * A sample has a last point exactly where it holds. */
  const bool firstBounce = fr.max_reflections > 0 && length(F3(1.0f, 1.0f, 1.0f) * F3(1.0f, 1.0f, 1.0f)) >= fr.min_importancy * SQRT3;
  WorkCounters cnt = {};
  for (;;) {
    uint32_t b = 0;
    if (lane == 0) b = atomicAdd(queue, 1u);
    b = __builtin_amdgcn_readfirstlane(b);
    if (b >= blocks) break;
    const uint32_t r = b * PLANES_GATHER_BLOCK + lane;   /* b < blocks <= 2^15: no overflow */
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
        flx_trace_params tp = {};                        /* flx_gather_ambient reads the ambient of it alone */
        const f3 ambient = frame_ambient(fr, 0);
        tp.ambient[0] = ambient.x; tp.ambient[1] = ambient.y; tp.ambient[2] = ambient.z;
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
          f3 facing = F3(0.0f, 0.0f, 0.0f);              /* the smooth normal facing the ray of the last iteration shaded */
          bool alive = firstBounce;
          if (firstBounce) {
            facing = sf0.smoothNormal;
            alive = bounceOn<false, LOCK>(sc, fr, sf0, ps, p, origin, cosSampleN, 0, cnt);
          }
          for (int i = 1; alive && i < fr.max_reflections && length(p.importancyFactor * ps.originalColor) >= fr.min_importancy * SQRT3; i++) {
            /* bounce<false, LOCK>() piece by piece, the surface kept (k_rays_paths_gather) */
            ShadeOut so;
            SurfaceCtx sf;
            shadeSurface<false>(sc, fr, p.hit, p.ray, p.lastHitPoint, sf, cnt);
            shadeSample<false>(sc, fr, sf, ps, p, origin, cosSampleN, i, so);
            facing = sf.smoothNormal;
            bool shadowed;
            walkBounce<false, LOCK>(sc, so.needShadow, nextBounceRuns(fr, i, p.importancyFactor, ps.originalColor), so.shadowRay, so.shadowLen, p.ray, shadowed, p.hit, cnt);
            bounceFinish(ps, p, so, shadowed);
            if (p.hit.triangleId == -1) break;
            p.lastHitPoint = p.ray.origin;
          }
          /* the wave is together again: every lane with a first hit looks the volume up at its sample's last point */
          float e[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
          if (firstBounce) {
            const float position[4] = { p.ray.origin.x, p.ray.origin.y, p.ray.origin.z, 1.0f };
            const float normal[3] = { facing.x, facing.y, facing.z };
            gather_corners<MAP, OFFSETS>(va.sh, va.maps, va.offsets, va.g, va.map, position, normal, e);
          }
          float a[3], value[3];
          const float fc[3] = { p.finalColor.x, p.finalColor.y, p.finalColor.z }, im[3] = { p.importancyFactor.x, p.importancyFactor.y, p.importancyFactor.z };
          flx_gather_ambient(&tp, va.gain, firstBounce ? 1 : 0, e, a);
          flx_gather_path_value(fc, im, a, value);
          finalColor = finalColor + F3(value[0], value[1], value[2]);
        }
        /* fragment:614-646, the filter branch */
        const float invSamples = 1.0f / (float)fr.samples;
        finalColor = finalColor * invSamples;
        float ipW = ps.glassFilter;
        if constexpr (TEMPORAL) {
          if (MODE == GATHER_TEMPORAL_CANVAS) { finalColor = finalColor * ps.originalColor; ipW = 1.0f; }      /* fragment:632-636, is_temporal == 1 */
        }
        color = make_float4(flx_fract(finalColor.x), flx_fract(finalColor.y), flx_fract(finalColor.z), 1.0f);
        colorIp = make_float4(flx_floor(finalColor.x) * INV_256, flx_floor(finalColor.y) * INV_256, flx_floor(finalColor.z) * INV_256, ipW);
        origColor = make_float4(ps.originalColor.x, ps.originalColor.y, ps.originalColor.z, flx_min(ps.originalRMEx, ps.firstRayLength) + INV_255);
        rid = make_float4(ps.renderId.x, ps.renderId.y, ps.renderId.z, ps.renderId.w + INV_255);
        roid = make_float4(0.0f, 0.0f, 0.0f, ps.originalTPOx + INV_255);
        if constexpr (TEMPORAL) {
          qc = pack_rgba8(color.x, color.y, color.z, color.w); qip = pack_rgba8(colorIp.x, colorIp.y, colorIp.z, colorIp.w);
          qo = pack_rgba8(origColor.x, origColor.y, origColor.z, origColor.w); qrid = pack_rgba8(rid.x, rid.y, rid.z, rid.w); qoid = pack_rgba8(roid.x, roid.y, roid.z, roid.w);
          /* fragment:640-642 as k_trace_pixels writes it: relativePosition in object space, the origin in world space; the hit row fetched again (k_rays_planes says why) */
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
        if (MODE == GATHER_TEMPORAL_FILTER) {     /* the three targets the pass hands on as they are */
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
        if (MODE == GATHER_TEMPORAL_FILTER) {
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

/* ---- the launch ------------------------------------------------------------------------------------------------------------------------------------- */

namespace {

struct Launch {
  uint32_t groups; hipStream_t stream; PlanesGatherArgs ra; const float4 *rays, *hits; uint32_t *out8; float4 *out32; uint32_t *queue; uint32_t m; size_t stride;
  PlanesGatherTemporal th; PlanesGatherVolume va;
};

template <bool LOCK, int MODE, bool MAP, bool OFFSETS> void launch_as(const Launch &l) {
  if constexpr (MODE == GATHER_PLANES)
    hipLaunchKernelGGL((k_rays_planes_gather<LOCK, MODE, MAP, OFFSETS>), dim3(l.groups), dim3(256), 0, l.stream, l.ra, l.rays, l.hits, l.out8, l.out32, l.queue, l.m, l.stride,
                       PlanesGatherNoArgs(), l.va);
  else
    hipLaunchKernelGGL((k_rays_planes_gather<LOCK, MODE, MAP, OFFSETS>), dim3(l.groups), dim3(256), 0, l.stream, l.ra, l.rays, l.hits, l.out8, l.out32, l.queue, l.m, l.stride,
                       l.th, l.va);
}
template <bool LOCK, int MODE> void launch_volume(const Launch &l, bool map, bool offsets) {
  if (map && offsets) launch_as<LOCK, MODE, true, true>(l);
  else if (offsets) launch_as<LOCK, MODE, false, true>(l);
  else if (map) launch_as<LOCK, MODE, true, false>(l);
  else launch_as<LOCK, MODE, false, false>(l);
}
template <bool LOCK> void launch_mode(const Launch &l, int mode, bool map, bool offsets) {
  if (mode == GATHER_TEMPORAL_FILTER) launch_volume<LOCK, GATHER_TEMPORAL_FILTER>(l, map, offsets);
  else if (mode == GATHER_TEMPORAL_CANVAS) launch_volume<LOCK, GATHER_TEMPORAL_CANVAS>(l, map, offsets);
  else launch_volume<LOCK, GATHER_PLANES>(l, map, offsets);
}

}  // namespace

flx_status flx_planes_gather_launch(flx_context *ctx, bool lock, int mode, uint32_t groups, const DeviceScene &sc, const DeviceFrame &fr, const float4 *rays, const float4 *hits,
                                    uint32_t *out8, float4 *out32, uint32_t *queue, uint32_t m, size_t stride, uint32_t *rings, uint32_t packed, const flx_planes_volume &volume) {
  Launch l;
  l.groups = groups; l.stream = ctx->stream; l.ra.sc = sc; l.ra.fr = fr; l.rays = rays; l.hits = hits; l.out8 = out8; l.out32 = out32; l.queue = queue; l.m = m; l.stride = stride;
  l.th.rings = rings; l.th.packed = packed;
  l.va.sh = volume.sh; l.va.maps = volume.maps; l.va.offsets = volume.offsets; l.va.g = volume.grid; l.va.map = volume.map; l.va.gain = volume.gain;
  const bool map = (volume.flags & FLX_GATHER_HAS_MAP) != 0u, offsets = (volume.flags & FLX_GATHER_HAS_OFFSETS) != 0u;
  if (lock) launch_mode<true>(l, mode, map, offsets);
  else launch_mode<false>(l, mode, map, offsets);
  FLX_HIP(ctx, hipGetLastError());
  flx_context::PlanesGatherLaunch &t = ctx->planes_gather_launch;
  t.groups = groups; t.flags = volume.flags; t.mode = (uint32_t)mode; t.samples = (uint32_t)fr.samples; t.lock = lock ? 1u : 0u;
  return FLX_OK;
}

void flx_planes_gather_ran(flx_context *ctx, uint32_t n, uint32_t slabs, uint32_t slab) {
  flx_context::PlanesGatherLaunch t = ctx->planes_gather_launch;
  t.n = n; t.slabs = slabs; t.slab = slab;
  ctx->last_planes_gather = t;
}

/* ---- the volume's refusals -------------------------------------------------------------------------------------------------------------------------- */

static flx_status fail(flx_context *ctx, flx_status code, const std::string &msg) { return flx_fail(ctx, code, msg.c_str()); }

/* a refusal of flx_gather_args.h in words (flx_rays_gather.hip's, the overlap naming this family's arrays) */
static flx_status gather_refusal(flx_context *ctx, enum flx_gather_refusal why, const char *call) {
  const char *what = "";
  switch (why) {
    case FLX_GATHER_ARGS_OK: return FLX_OK;
    case FLX_GATHER_VOLUME_NULL: what = "the volume is NULL"; break;
    case FLX_GATHER_GAIN: what = "gain is negative or not finite"; break;
    case FLX_GATHER_RESERVED: what = "the volume's reserved word is not 0"; break;
    case FLX_GATHER_MAP_PAIR: what = "map and maps are not both given or both NULL"; break;
    case FLX_GATHER_OVERLAP: what = "an array of the volume overlaps the rays, a plane output or the image"; break;
  }
  return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": " + what);
}

flx_status flx_planes_gather_volume_refused(flx_context *ctx, const flx_gather_volume *volume, const flx_planes_gather_array *call_arrays, int kc, const char *call,
                                            flx_planes_volume *out) {
  const std::string name = call;
  /* the volume calls' own: the grid, the map (only where one is given), the arrays — the SH rows, then the maps against them, then the offsets against both */
  if (!volume) return gather_refusal(ctx, FLX_GATHER_VOLUME_NULL, call);
  uint32_t probes = 0, rows = 0;
  flx_status s = flx_volume_grid_refused(ctx, volume->grid, &probes, call);
  if (s) return s;
  if (volume->map && (s = flx_volume_map_refused(ctx, volume->map, probes, &rows, call))) return s;
  const bool has_map = volume->map && volume->maps, relocated = volume->offsets != nullptr;
  uint64_t address[FLX_GATHER_MAX_ARRAYS], lengths[FLX_GATHER_MAX_ARRAYS];
  const void *others[FLX_GATHER_MAX_ARRAYS];
  int k = 0;
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  {
    const uint64_t sh_address = (uint64_t)(uintptr_t)volume->sh, sh_bytes = flx_volume_sh_bytes(probes);
    const enum flx_volume_refusal why = flx_volume_arrays_check(&sh_address, &sh_bytes, 1);
    if (why == FLX_VOLUME_NULL) return fail(ctx, FLX_ERR_INVALID, name + ": an array is NULL");
    if (why != FLX_VOLUME_ARGS_OK) return fail(ctx, FLX_ERR_INVALID, name + ": an array leaves the address space");
    if (!flx_rows_on_device(ctx, volume->sh, (size_t)sh_bytes))
      return fail(ctx, FLX_ERR_INVALID, name + ": the SH rows are not nx * ny * nz rows of 144 bytes in memory of the context's device, 16-byte aligned");
    address[k] = sh_address; lengths[k] = sh_bytes; others[k] = volume->sh; k++;
  }
  if (has_map) {
    const flx_map_other sh_rows[1] = { { volume->sh, lengths[0] } };
    if ((s = flx_volume_maps_refused(ctx, volume->maps, rows, sh_rows, 1, call))) return s;
    address[k] = (uint64_t)(uintptr_t)volume->maps; lengths[k] = flx_volume_map_bytes(rows); others[k] = volume->maps; k++;
  }
  if (relocated) {
    if ((s = flx_volume_offsets_refused(ctx, volume->offsets, probes, others, lengths, k, call))) return s;
    address[k] = (uint64_t)(uintptr_t)volume->offsets; lengths[k] = (uint64_t)probes * 16u; others[k] = volume->offsets; k++;
  }
  /* the gathered batches' own, then this family's overlap */
  enum flx_gather_refusal own = flx_gather_volume_check(1, volume->gain, volume->reserved, volume->map != nullptr, volume->maps != nullptr);
  if (own == FLX_GATHER_ARGS_OK) own = flx_planes_gather_overlap_check(address, lengths, k, call_arrays, kc);
  if (own != FLX_GATHER_ARGS_OK) return gather_refusal(ctx, own, call);
  if (out) {
    const flx_volume_map none = { 0u, 0u, { 0u, 0u } };
    out->sh = (const float4 *)volume->sh;
    out->maps = has_map ? (const float4 *)volume->maps : nullptr;
    out->offsets = (const float4 *)volume->offsets;
    out->grid = *volume->grid;
    out->map = has_map ? *volume->map : none;
    out->gain = volume->gain;
    out->flags = flx_planes_gather_flags(has_map, relocated);
  }
  return FLX_OK;
}

extern "C" flx_status flx_debug_last_planes_gather(flx_context *ctx, uint32_t out[8]) {
  if (!ctx || !out) return FLX_ERR_INVALID;
  const flx_context::PlanesGatherLaunch &t = ctx->last_planes_gather;
  out[0] = t.n; out[1] = t.slabs; out[2] = t.slab; out[3] = t.groups; out[4] = t.flags; out[5] = t.mode; out[6] = t.samples; out[7] = t.lock;
  return FLX_OK;
}
