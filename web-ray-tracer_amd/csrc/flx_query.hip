/* flx_query.hip — ray queries: a caller's rays cast at the resident scene (include/flexlight_hip_debug.h, "ray queries").
 *
 * What a frame asks of the scene through rayTracer (fragment:172-227) and shadowTest (:231-280), asked with rays of the caller's own: what does this ray hit, is
 * this point lit from there.  The walk is the wavefront pipeline's, unchanged (flx_device.h): the threaded hot-first copy, its top staged in LDS, the rays
 * pre-transformed into every object space where those fit beside a useful tree top (walkSetupRays / walkFetchP / walkBoxP / walkTriT; up to three transforms, the line
 * the rounds draw) and transformed on the fly where they do not (walkFetchT / walkBoxT) — so every answer is the oracle's, bit for bit.
 *
 * k_ray_query is ONE persistent launch.  LDS: [tree top: ldsCount entries x 48 B][T x 4 float4: inverse rotation columns and inverse shift][per thread: T x 40 B
 * of pre-transformed rays] (the last two with pre-transformed rays only).  A wave draws chunks of QUERY_CHUNK consecutive ray indices from one device cursor, one
 * atomic per chunk, and hands them to its free lanes in order: the coherence the caller gave survives.  A lane whose walk ends writes its ray's hit row and takes
 * the next ray once QUERY_BATCH lanes of its wave are free.  No fold, no record, no live list; no wait on another wave or workgroup anywhere: the one shared word
 * is the cursor, zeroed in front of every launch, and every walk ends at the validated scene's terminator.
 *
 * Behind the kernel: the host path that every ray-batch call shares (cast here; trace, surface, planes and images in flx_rays_trace.hip, flx_surface.hip and
 * flx_rays_planes.hip) — declared in flx_context.h, its templates in flx_rays_host.h. */
#include <cstring>
#include <mutex>
#include <string>

#include "flx_context.h"
#include "flx_kernel_util.h"
#include "flx_query_args.h"
#include "flx_rays_host.h"

using namespace flx;

namespace flx {

constexpr uint32_t QUERY_THREADS = 1024;               /* one workgroup per compute unit, four waves per SIMD: the walk kernels' shape (FLX_WF_WALK_THREADS) */
constexpr uint32_t QUERY_BATCH = 24;                   /* free lanes of a wave that trigger a write-out + refill (FLX_WF_BATCH; 40 measured slower: profiles/ray_query.txt) */
constexpr int QUERY_INNER = 8;                         /* entries per walking lane between two looks at the wave's state (FLX_WF_INNER) */
constexpr uint32_t QUERY_LDS_TOTAL = 156u * 1024u;     /* LDS the workgroup may use, of 160 KB per CU (FLX_WF_LDS_TOTAL) */
constexpr uint32_t QUERY_CLOSEST = 1u, QUERY_OCCLUDED = 2u;      /* FLX_RAYS_CLOSEST, FLX_RAYS_OCCLUDED */

enum { Q_EMPTY = 0, Q_SETUP = 1, Q_WALKING = 2, Q_SWITCH = 3, Q_DONE = 4 };

/* COUNT: words 6 and 7 of a hit row are the entries its walks fetched (zeros otherwise; no counting code is compiled in).  PRE: the rays pre-transformed into every
 * object space (else transformed on the fly): a build each, so that neither path's registers weigh on the other's stepping loop. */
template <bool COUNT, bool PRE>
__global__ __launch_bounds__(QUERY_THREADS) void k_ray_query(DeviceScene sc, const float4 *__restrict__ rays, float4 *__restrict__ hits, uint32_t n, uint32_t what,
                                                             uint32_t *__restrict__ ctl, uint32_t ldsCount) {
  extern __shared__ float4 ldsQuery[];
  const uint32_t T = sc.n_transforms;
  float4 *ldsEntries = ldsQuery;
  float4 *ldsXf = ldsQuery + (size_t)ldsCount * 3u;
  float2 *myRays = (float2 *)(ldsXf + (size_t)T * 4u) + (size_t)threadIdx.x * T * 5u;      /* (read and written with pre-transformed rays only) */
  for (uint32_t t = threadIdx.x; t < ldsCount * 3u; t += QUERY_THREADS) ldsEntries[t] = sc.walk[t];
  if (PRE) {
    for (uint32_t t = threadIdx.x; t < T * 4u; t += QUERY_THREADS) {
      const uint32_t tr = t >> 2, k = t & 3u, iI = 2u * tr + 1u;
      ldsXf[t] = k < 3u ? sc.rotation[3u * iI + k] : sc.shift[iI];
    }
  }
  __syncthreads();                                       /* (the only barrier: every wave is on its own from here) */
  const uint32_t lane = threadIdx.x & 63u;
  const bool thick = sc.walk_thick_boxes != 0u;          /* the box test's form, as k_debug_walk<0> chooses it (flx_debug_set_box_test) */
  const bool wantShadow = (what & QUERY_OCCLUDED) != 0u, wantClosest = (what & QUERY_CLOSEST) != 0u;
  const uint32_t nChunks = (uint32_t)(((uint64_t)n + (QUERY_CHUNK - 1u)) / QUERY_CHUNK);

  int st = Q_EMPTY;
  uint32_t rayId = 0;
  Ray ray; ray.origin = F3(0.f, 0.f, 0.f); ray.dir = ray.origin;
  float shadowLen = 0.0f;
  WorkCounters cnt = {};
  WalkState w;
  walkClearResults(w);
  w.src = ray; w.tR = ray; w.minLen = 0.0f; w.i = 0; w.cachedTI = 0; w.mode = 2;
  WalkEntry cur;
  cur.e0 = cur.e1 = cur.e2 = make_float4(0.f, 0.f, 0.f, 0.f);
  uint32_t chunkNext = 0, chunkEnd = 0;                  /* wave-uniform: ray indices drawn and not yet handed to a lane */
  bool itemsLeft = true, drew = false;

  for (;;) {
    const unsigned long long walking = flx_ballot(st == Q_WALKING);
    const unsigned long long workMask = flx_ballot(st == Q_DONE || st == Q_SWITCH);
    const bool canRefill = itemsLeft || chunkNext != chunkEnd;
    const uint32_t parked = 64u - (uint32_t)__popcll(walking);
    if (walking == 0ull || (parked >= QUERY_BATCH && (workMask != 0ull || canRefill))) {
      /* ---- a shadow walk that ended: the ray's closest-hit walk follows where it was asked for (a path's order) ---- */
      if (st == Q_SWITCH) {
        if (wantClosest) { w.mode = 1; st = Q_SETUP; } else st = Q_DONE;
      }
      /* ---- a finished ray: its hit row, two 16-byte stores ---- */
      if (st == Q_DONE) {
        const bool hit = w.tri != -1;
        float4 *o = hits + (size_t)rayId * 2u;
        o[0] = make_float4(hit ? w.suv.x : 0.0f, hit ? w.suv.y : 0.0f, hit ? w.suv.z : 0.0f, __int_as_float(w.tri));
        o[1] = make_float4(__int_as_float(hit ? w.hitTI : 0), __int_as_float(w.shadowed != 0 ? 1 : 0), __uint_as_float(COUNT ? cnt.closest_visits : 0u),
                           __uint_as_float(COUNT ? cnt.shadow_visits : 0u));
        st = Q_EMPTY;
      }
      /* ---- the free lanes take the next rays, in order ---- */
      for (;;) {
        const unsigned long long idle = flx_ballot(st == Q_EMPTY);
        if (idle == 0ull) break;
        if (chunkNext == chunkEnd) {
          if (!itemsLeft) break;
          uint32_t c = 0;
          if (lane == 0) c = atomicAdd(ctl, 1u);           /* (chunks, not rays: the cursor cannot wrap however many waves look once more) */
          c = __builtin_amdgcn_readfirstlane(c);
          if (c >= nChunks) { itemsLeft = false; break; }
          drew = true;
          chunkNext = c * QUERY_CHUNK;
          chunkEnd = (n - chunkNext > QUERY_CHUNK) ? chunkNext + QUERY_CHUNK : n;
        }
        const uint32_t nIdle = (uint32_t)__popcll(idle);
        const uint32_t avail = chunkEnd - chunkNext;
        const uint32_t take = nIdle < avail ? nIdle : avail;
        const uint32_t r = lane_rank(idle);
        if (st == Q_EMPTY && r < take) {
          rayId = chunkNext + r;                           /* < chunkEnd <= n */
          const float4 q0 = rays[(size_t)rayId * 2u], q1 = rays[(size_t)rayId * 2u + 1u];
          ray.origin = F3(q0.x, q0.y, q0.z); ray.dir = F3(q1.x, q1.y, q1.z);
          shadowLen = q0.w;
          walkClearResults(w);
          cnt = {};
          w.mode = wantShadow ? 0 : 1;
          st = Q_SETUP;
        }
        chunkNext += take;
      }
      /* ---- set up walks: fresh rays and rays whose shadow walk just ended ---- */
      if (st == Q_SETUP) {
        const bool shadowMode = w.mode == 0;
        bool ended;
        if (PRE) {
          walkSetupRays(sc, T, ldsXf, myRays, ray, shadowMode);
          w.src = ray; w.tR = ray; w.cachedTI = 0; w.minLen = shadowMode ? shadowLen : POW32; w.i = (int)sc.walk_root;
          reciprocalOfDir(sc, ray.dir, ray.origin, w.inv, w.fastDiv);      /* the untransformed ray (cachedTI = 0, fragment:174-175) */
          ended = walkFetchP<COUNT>(sc, ldsEntries, ldsCount, myRays, w, cur, cnt);
        } else {
          walkStartT(sc, w, w.mode, ray, shadowMode ? shadowLen : POW32);
          ended = walkFetchT<COUNT>(sc, ldsEntries, ldsCount, w, cur, cnt);
        }
        st = ended ? (shadowMode ? Q_SWITCH : Q_DONE) : Q_WALKING;
      }
      if (flx_ballot(st == Q_WALKING) == 0ull) {
        if (itemsLeft || chunkNext != chunkEnd || flx_ballot(st == Q_SWITCH || st == Q_DONE) != 0ull) continue;
        break;                                             /* nothing walking, nothing to write, nothing left to draw */
      }
    }
    /* ---- QUERY_INNER entries for every walking lane ---- */
    if (PRE) {
#pragma unroll 1
      for (int it = 0; it < QUERY_INNER; it++) {
        if (st == Q_WALKING) {
          bool ended = false;
          if (walkIsBoxT(cur)) { if (thick) walkBoxP<true>(w, cur); else walkBoxP(w, cur); }
          else ended = walkTriT(w, cur);
          if (!ended) ended = walkFetchP<COUNT>(sc, ldsEntries, ldsCount, myRays, w, cur, cnt);
          if (ended) st = (w.mode == 0) ? Q_SWITCH : Q_DONE;
        }
      }
    } else {
#pragma unroll 1
      for (int it = 0; it < QUERY_INNER; it++) {
        if (st == Q_WALKING) {
          bool ended = false;
          if (walkIsBoxT(cur)) walkBoxT(w, cur); else ended = walkTriT(w, cur);
          if (!ended) ended = walkFetchT<COUNT>(sc, ldsEntries, ldsCount, w, cur, cnt);
          if (ended) st = (w.mode == 0) ? Q_SWITCH : Q_DONE;
        }
      }
    }
  }
  if (lane == 0 && drew) atomicAdd(ctl + 1, 1u);
}

bool launch_ray_query(const DeviceScene &sc, const float4 *rays, float4 *hits, uint32_t n, uint32_t what, uint32_t *ctl, uint32_t compute_units, uint32_t groups,
                      hipStream_t stream, QueryLaunch *ran) {
  /* LDS first holds every thread's pre-transformed rays (T x 40 B each) and the staged inverse transforms when they leave room for a useful tree top — the rule
   * of the rounds (launch_wavefront): up to three transforms —, the rest goes to the tree top */
  const uint32_t T = sc.n_transforms;
  const uint64_t rayBytes = (uint64_t)QUERY_THREADS * T * 40u + (uint64_t)T * 64u;
  const bool pre = T <= 3u && rayBytes + 8192u <= QUERY_LDS_TOTAL;
  const uint32_t ldsBudget = QUERY_LDS_TOTAL - (pre ? (uint32_t)rayBytes : 0u);
  uint32_t ldsCount = ldsBudget / 48u;
  if (ldsCount > sc.walk_hot) ldsCount = sc.walk_hot;
  const uint32_t ldsBytes = ldsCount * 48u + (pre ? (uint32_t)rayBytes : 0u);
  static std::once_flag once[64];
  static bool ok[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
  const void *const kernels[4] = { (const void *)k_ray_query<false, false>, (const void *)k_ray_query<true, false>, (const void *)k_ray_query<false, true>,
                                   (const void *)k_ray_query<true, true> };      /* [2 * pre + counted] */
  std::call_once(once[dev], [&]() {
    ok[dev] = true;
    for (const void *k : kernels) ok[dev] = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess && ok[dev];
  });
  if (!ok[dev]) return false;
  if (groups == 0u) {
    /* a workgroup per compute unit (its registers and LDS leave room for one), fewer where the rays do not give every lane one */
    const uint32_t full = (uint32_t)(((uint64_t)n + QUERY_THREADS - 1u) / QUERY_THREADS);
    groups = full < compute_units ? full : compute_units;
  }
  if (groups == 0u) groups = 1u;
  const uint32_t pre32 = pre ? 1u : 0u;
  uint32_t nArg = n, whatArg = what, ldsCountArg = ldsCount;
  DeviceScene scArg = sc;
  void *args[] = { &scArg, &rays, &hits, &nArg, &whatArg, &ctl, &ldsCountArg };      /* (one launch statement for the four kernels: by address, in the kernel's order) */
  (void)hipLaunchKernel(kernels[2u * pre32 + ((what & 4u) != 0u ? 1u : 0u)], dim3(groups), dim3(QUERY_THREADS), args, ldsBytes, stream);
  if (ran) { ran->ldsCount = ldsCount; ran->pre = pre32; ran->groups = groups; ran->n = n; ran->what = what; }
  return true;
}

}  // namespace flx

/* ---- the host path the ray-batch calls share (flx_context.h; flx_rays_host.h) -------------------------------------------------------------------- */

static flx_status fail(flx_context *ctx, flx_status code, const char *msg) { return flx_fail(ctx, code, msg); }
static flx_status fail(flx_context *ctx, flx_status code, const std::string &msg) { return flx_fail(ctx, code, msg.c_str()); }

flx_status flx_scene_refused(flx_context *ctx, const char *call) {
  if (!ctx->have_scene || !ctx->have_transforms) return fail(ctx, FLX_ERR_NO_SCENE, std::string(call) + ": no scene and transforms uploaded");
  return FLX_OK;
}

flx_status flx_trace_params_refused(flx_context *ctx, const flx_trace_params *p, const char *call) {
  flx_status s = flx_scene_refused(ctx, call);
  if (s) return s;
  const char *what = "";
  switch (flx_trace_args_check(p != nullptr, p ? p->samples : 0, p ? p->max_reflections : 0, p ? p->texture_width : 0, 0u, 0u, 0u)) {
    case FLX_TRACE_ARGS_OK: return FLX_OK;
    case FLX_TRACE_PARAMS_NULL: what = "params is NULL"; break;
    case FLX_TRACE_SAMPLES: what = "samples is less than 1"; break;
    case FLX_TRACE_REFLECTIONS: what = "max_reflections is negative"; break;
    default: what = "texture_width is less than 1"; break;
  }
  return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": " + what);
}

void flx_trace_frame(const flx_trace_params *p, DeviceFrame &fr, int use_filter, int is_temporal) {
  memset(&fr, 0, sizeof fr);
  fr.use_filter = use_filter;
  fr.is_temporal = is_temporal;
  fr.width = fr.height = fr.rows = fr.frame_rows = fr.frames = fr.tile_rows = fr.tile_count = 1u;
  fr.samples = p->samples; fr.max_reflections = p->max_reflections;
  fr.samples_shift = -1;
  fr.min_importancy = p->min_importancy;
  fr.texture_width = (float)p->texture_width;
  memcpy(fr.view[0].ambient, p->ambient, sizeof fr.view[0].ambient);
  fr.view[0].random_seed = p->random_seed;
}

flx_status flx_wait_for_producer(flx_context *ctx, void *producer_stream) {
  if (!producer_stream) return FLX_OK;
  if (!ctx->query_produced) FLX_HIP(ctx, hipEventCreateWithFlags(&ctx->query_produced, hipEventDisableTiming));
  FLX_HIP(ctx, hipEventRecord(ctx->query_produced, (hipStream_t)producer_stream));
  FLX_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->query_produced, 0));
  return FLX_OK;
}

/* one query launch, its control words zeroed in stream order in front of it: [0] the chunk cursor, [1] the waves that drew (d_trace_ctl: [2] the cursor of the kernel
 * that follows in a slab) */
static flx_status query_enqueue(flx_context *ctx, const DeviceScene &sc, const float4 *rays, float4 *hits, uint32_t n, uint32_t what, uint32_t *ctl, const char *call, QueryLaunch &q) {
  FLX_HIP(ctx, hipMemsetAsync(ctl, 0, 4 * sizeof(uint32_t), ctx->stream));
  if (!launch_ray_query(sc, rays, hits, n, what, ctl, (uint32_t)ctx->prop.multiProcessorCount, ctx->query_groups, ctx->stream, &q))
    return fail(ctx, FLX_ERR_DEVICE, std::string(call) + ": the query kernel cannot have its LDS on this device");
  FLX_HIP(ctx, hipGetLastError());
  return FLX_OK;
}

flx_status flx_slab_first_hits(flx_context *ctx, const DeviceScene &sc, const float4 *rays, uint32_t m, const char *call, QueryLaunch &q) {
  return query_enqueue(ctx, sc, rays, ctx->d_trace_hits, m, FLX_RAYS_CLOSEST, ctx->d_trace_ctl, call, q);
}

/* ---- the calls ------------------------------------------------------------------------------------------------------------------------------------- */

/* what both calls refuse before they look at an array */
static flx_status query_refused(flx_context *ctx, uint32_t what) {
  flx_status s = flx_scene_refused(ctx, "flx_rays_cast");
  if (s) return s;
  if ((what & ~7u) != 0u) return fail(ctx, FLX_ERR_INVALID, "flx_rays_cast: what has a bit beyond FLX_RAYS_CLOSEST | FLX_RAYS_OCCLUDED | FLX_RAYS_COUNT");
  if ((what & 3u) == 0u) return fail(ctx, FLX_ERR_INVALID, "flx_rays_cast: what asks for neither FLX_RAYS_CLOSEST nor FLX_RAYS_OCCLUDED");
  return FLX_OK;
}

extern "C" flx_status flx_rays_cast_device(flx_context *ctx, const void *d_rays, void *d_hits, uint32_t n, uint32_t what, void *producer_stream) {
  static const char *const call = "flx_rays_cast_device";
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = query_refused(ctx, what);
  if (s || n == 0) return s;
  const enum flx_query_refusal arrays = flx_query_args_check((uint64_t)(uintptr_t)d_rays, (uint64_t)(uintptr_t)d_hits, n, what);
  switch (arrays) {
    case FLX_QUERY_ARGS_OK: case FLX_QUERY_OVERLAP: break;      /* (overlap: said after the pointers are known to be the device's) */
    case FLX_QUERY_NULL: return fail(ctx, FLX_ERR_INVALID, "flx_rays_cast_device: an array is NULL");
    default: return fail(ctx, FLX_ERR_INVALID, "flx_rays_cast_device: n rows of 32 bytes leave the address space");
  }
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  const size_t bytes = (size_t)n * FLX_RAY_ROW_BYTES;
  if (!flx_rows_on_device(ctx, d_rays, bytes))
    return fail(ctx, FLX_ERR_INVALID, "flx_rays_cast_device: the rays are not n rows in memory of the context's device, 16-byte aligned");
  if (!flx_rows_on_device(ctx, d_hits, bytes))
    return fail(ctx, FLX_ERR_INVALID, "flx_rays_cast_device: the hits are not n rows in memory of the context's device, 16-byte aligned");
  if (arrays == FLX_QUERY_OVERLAP) return fail(ctx, FLX_ERR_INVALID, "flx_rays_cast_device: the rays and the hits overlap");
  DeviceScene sc;
  if ((s = flx_make_scene(ctx, sc))) return s;              /* (refuses a scene that names a transform not uploaded) */
  if ((s = flx_server_stop(ctx))) return s;                 /* as flx_render_device: the frame server's launch ends after the frames posted to it */
  if ((s = ctx->d_query_ctl.ensure(ctx, 4))) return s;
  if ((s = flx_wait_for_producer(ctx, producer_stream))) return s;
  QueryLaunch ran;
  if ((s = query_enqueue(ctx, sc, (const float4 *)d_rays, (float4 *)d_hits, n, what, ctx->d_query_ctl, call, ran))) return s;
  ctx->last_query = ran;
  return FLX_OK;
}

extern "C" flx_status flx_rays_cast(flx_context *ctx, const float *rays, void *hits, uint32_t n, uint32_t what) {
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = query_refused(ctx, what);
  if (s || n == 0) return s;
  if (!rays || !hits) return fail(ctx, FLX_ERR_INVALID, "flx_rays_cast: an array is NULL");
  return flx_rays_from_host(ctx, rays, n, [&]() { return flx_rays_cast_device(ctx, ctx->d_query_rays, ctx->d_query_hits, n, what, nullptr); },
                            flx_down(&ctx->d_query_hits, (size_t)n * 2u, hits));
}

extern "C" flx_status flx_debug_set_query_groups(flx_context *ctx, uint32_t groups) {
  if (!ctx) return FLX_ERR_INVALID;
  if (groups > 65535u) return fail(ctx, FLX_ERR_INVALID, "flx_debug_set_query_groups: at most 65535 workgroups");
  ctx->query_groups = groups;
  return FLX_OK;
}

extern "C" flx_status flx_debug_last_query(flx_context *ctx, uint32_t out[8]) {
  if (!ctx || !out) return FLX_ERR_INVALID;
  memset(out, 0, 8 * sizeof(uint32_t));
  const QueryLaunch &q = ctx->last_query;
  if (q.groups == 0u) return FLX_OK;                        /* no launch since the scene upload */
  uint32_t ctl[2] = { 0u, 0u };
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  FLX_HIP(ctx, hipMemcpy(ctl, ctx->d_query_ctl, sizeof ctl, hipMemcpyDeviceToHost));
  out[0] = q.ldsCount; out[1] = q.pre; out[2] = q.groups; out[3] = ctl[1]; out[4] = q.n; out[5] = q.what; out[6] = QUERY_CHUNK; out[7] = ctl[0];
  return FLX_OK;
}
