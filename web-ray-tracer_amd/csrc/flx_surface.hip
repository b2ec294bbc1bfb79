/* flx_surface.hip — surface rows: what the surface is where a ray first hits (include/flexlight_hip_debug.h, "surface rows": flx_rays_surface, flx_rays_surface_device,
 * flx_frame_surface, flx_frame_surface_device).
 *
 * The first thing lightTrace computes at a hit (fragment:476-533; shadeSurface, flx_device.h), written out instead of shaded: the hit point, the geometric normal, the
 * smooth normal facing the ray, the texture coordinates and the three material values with the atlases applied — per ray of a caller's batch or per pixel of a frame.
 *   1. first hits.  Rays: k_ray_query as it stands (flx_query.hip, what = FLX_RAYS_CLOSEST) into hit rows of 32 bytes — the closest hit exactly as flx_rays_cast
 *      answers it.  Frames: k_primary as it stands (flx_kernels.hip) into a float4 per pixel — the primary hit as a frame finds it; the two hit rules differ on a few
 *      pixels per million (profiles/rays_trace.txt), so a frame's rows come from the frame's own rule.
 *   2. k_surface<FRAME>: one item per lane, a ray and its hit.  Ray rows and hit rows are read with 16-byte loads (a frame's ray is the camera and primary_dir_v's
 *      direction of the pixel, made in registers).  A miss touches no scene array — its entry is -1 and indexes nothing — and writes its miss rows.  A hit runs
 *      shadeSurface's statements in shadeSurface's order with flx_math.h's routines, but only those the planes asked for need: `fields` is uniform, so a plane that
 *      is not asked for costs neither its gathers nor its arithmetic.  shadeSurface's geometryOffset chain (three distances, three acos, three tan) feeds no row
 *      and is not here.  Plane p of the output starts at out + p * n rows; every lane makes one 16-byte store per plane, a wave 1 KiB contiguous per plane.
 * The hit scratch is the traced batches' (flx_context.h: d_trace_hits, d_trace_ctl), grown and never shrunk; a ray batch is cut into slabs of at most 2^21 rays
 * (flx_trace_slab_rays at one slot a ray; flx_debug_set_trace_slab lowers it), a slab's two launches following each other on the context's stream.  The host waits
 * for nothing — but where the scratch must grow, for the work that may still use it.  The growth, the producer wait, the slab loop and its first hits and the
 * host-memory calls are the ray-batch calls' shared path (flx_query.hip, flx_rays_host.h). */
#include <cstring>

#include "flx_context.h"
#include "flx_kernel_util.h"
#include "flx_query_args.h"
#include "flx_rays_host.h"
#include "flx_surface_args.h"

using namespace flx;

namespace flx {

struct SurfaceArgs {
  DeviceScene sc;
  float texture_width;
  uint32_t width, height;      /* FRAME: the canvas, row 0 on top */
  FrameView view;              /* FRAME: the camera and the inverse view matrix */
};

template <bool FRAME>
__global__ __launch_bounds__(256) void k_surface(SurfaceArgs sa, const float4 *__restrict__ rays, const float4 *__restrict__ hits, float4 *__restrict__ out, uint32_t n,
                                                 size_t planeRows, uint32_t fields) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  const DeviceScene &sc = sa.sc;
  float4 *o = out + r;         /* the lane's row of the next plane asked for */
  auto put = [&](uint32_t bit, float4 row) { if (fields & bit) { *o = row; o += planeRows; } };
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);

  Hit hit;
  const float4 h0 = FRAME ? hits[r] : hits[(size_t)r * 2u];
  hit.suv = F3(h0.x, h0.y, h0.z);
  hit.triangleId = __float_as_int(h0.w);
  if (hit.triangleId == -1) {
    put(FLX_SURFACE_HIT, make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1)));
    for (uint32_t bit = FLX_SURFACE_POSITION; bit <= FLX_SURFACE_TPO; bit <<= 1) put(bit, zero);
    return;
  }
  put(FLX_SURFACE_HIT, h0);
  if ((fields & ~FLX_SURFACE_HIT) == 0u) return;

  Ray ray;
  if (FRAME) {
    DeviceFrame fr;              /* primary_dir_v reads the canvas size alone */
    fr.width = sa.width; fr.height = sa.height;
    const uint32_t row = r / sa.width, px = r - row * sa.width;
    float nx, ny, viewDepthPerS;
    ray.dir = primary_dir_v(fr, sa.view, px, sa.height - 1u - row, nx, ny, viewDepthPerS);
    ray.origin = view_camera(sa.view);
    hit.transformId = (int)sc.geometry[3 * hit.triangleId + 2].y << 1;      /* (what primaryWalkF's Hit carries: 2 x the entry's transform number) */
  } else {
    const float4 q0 = rays[(size_t)r * 2u], q1 = rays[(size_t)r * 2u + 1u];
    ray.origin = F3(q0.x, q0.y, q0.z);
    ray.dir = F3(q1.x, q1.y, q1.z);      /* as given: rayTracer does not normalise it, lightTrace steps along it by s */
    hit.transformId = __float_as_int(hits[(size_t)r * 2u + 1u].x);
  }
  const f3 lastHitPoint = ray.origin;

  /* shadeSurface's statements (fragment:476-533), in its order */
  const f3 origin = ray.dir * hit.suv.x + ray.origin;
  put(FLX_SURFACE_POSITION, make_float4(origin.x, origin.y, origin.z, 1.0f));
  const f3 uvw = F3(1.0f - hit.suv.y - hit.suv.z, hit.suv.y, hit.suv.z);
  M3 rTI = {};
  if (fields & (FLX_SURFACE_GEOMETRY_NORMAL | FLX_SURFACE_NORMAL)) rTI = rotation_at(sc, hit.transformId);
  if (fields & FLX_SURFACE_GEOMETRY_NORMAL) {
    const float4 g0 = sc.geometry[3 * hit.triangleId], g1 = sc.geometry[3 * hit.triangleId + 1], g2 = sc.geometry[3 * hit.triangleId + 2];
    const f3 t0v = mul(rTI, F3(g0.x, g0.y, g0.z));
    const f3 t1v = mul(rTI, F3(g0.w, g1.x, g1.y));
    const f3 t2v = mul(rTI, F3(g1.z, g1.w, g2.x));
    const f3 geometryNormal = normalize(cross(t0v - t1v, t0v - t2v));
    put(FLX_SURFACE_GEOMETRY_NORMAL, make_float4(geometryNormal.x, geometryNormal.y, geometryNormal.z, 0.0f));
  }
  if ((fields & ~(FLX_SURFACE_HIT | FLX_SURFACE_POSITION | FLX_SURFACE_GEOMETRY_NORMAL)) == 0u) return;
  const float4 *at = sc.attributes + 7 * (size_t)hit.triangleId;
  if (fields & FLX_SURFACE_NORMAL) {
    const float4 a0 = at[0], a1 = at[1], a2 = at[2];
    const f3 n0 = mul(rTI, F3(a0.x, a0.y, a0.z));
    const f3 n1 = mul(rTI, F3(a0.w, a1.x, a1.y));
    const f3 n2 = mul(rTI, F3(a1.z, a1.w, a2.x));
    const f3 smoothNormal = normalize(F3((n0.x * uvw.x + n1.x * uvw.y) + n2.x * uvw.z,
                                         (n0.y * uvw.x + n1.y * uvw.y) + n2.y * uvw.z,
                                         (n0.z * uvw.x + n1.z * uvw.y) + n2.z * uvw.z));
    const f3 dir = normalize(origin - lastHitPoint);
    const float signDir = flx_sign(dot(dir, smoothNormal));
    const f3 facing = smoothNormal * (-signDir);
    put(FLX_SURFACE_NORMAL, make_float4(facing.x, facing.y, facing.z, signDir));
  }
  if ((fields & (FLX_SURFACE_UV | FLX_SURFACE_ALBEDO | FLX_SURFACE_RME | FLX_SURFACE_TPO)) == 0u) return;
  /* uv0 = a2.yz, uv1 = (a2.w, a3.x), uv2 = a3.yz */
  const float4 a2 = at[2], a3 = at[3];
  const float bu = (a2.y * uvw.x + a2.w * uvw.y) + a3.y * uvw.z;
  const float bv = (a2.z * uvw.x + a3.x * uvw.y) + a3.z * uvw.z;
  put(FLX_SURFACE_UV, make_float4(bu, bv, __int_as_float(hit.transformId), 0.0f));
  if ((fields & (FLX_SURFACE_ALBEDO | FLX_SURFACE_RME | FLX_SURFACE_TPO)) == 0u) return;
  DeviceFrame tf;                /* fetchTexVal reads the texture width alone */
  tf.texture_width = sa.texture_width;
  WorkCounters cnt;
  const float4 a4 = at[4];
  if (fields & FLX_SURFACE_ALBEDO) {
    const float4 a5 = at[5];
    const f3 albedo = fetchTexVal<false>(sc, tf, 0, bu, bv, a3.w, F3(a4.z, a4.w, a5.x), cnt);
    put(FLX_SURFACE_ALBEDO, make_float4(albedo.x, albedo.y, albedo.z, 0.0f));
  }
  if (fields & FLX_SURFACE_RME) {
    const float4 a5 = at[5];
    const f3 rme = fetchTexVal<false>(sc, tf, 1, bu, bv, a4.x, F3(a5.y, a5.z, a5.w), cnt);
    put(FLX_SURFACE_RME, make_float4(rme.x, rme.y, rme.z, 0.0f));
  }
  if (fields & FLX_SURFACE_TPO) {
    const float4 a6 = at[6];
    const f3 tpo = fetchTexVal<false>(sc, tf, 2, bu, bv, a4.y, F3(a6.x, a6.y, a6.z), cnt);
    put(FLX_SURFACE_TPO, make_float4(tpo.x, tpo.y, tpo.z, 0.0f));
  }
}

}  // namespace flx

/* ---- the calls ------------------------------------------------------------------------------------------------------------------------------------- */

static flx_status fail(flx_context *ctx, flx_status code, const char *msg) { return flx_fail(ctx, code, msg); }

/* a refusal of flx_surface_args.h in words; `call`: the entry point's name */
static flx_status surface_refusal(flx_context *ctx, enum flx_surface_refusal why, const char *call) {
  const char *what = "";
  switch (why) {
    case FLX_SURFACE_ARGS_OK: return FLX_OK;
    case FLX_SURFACE_FIELDS_NONE: what = "fields asks for no plane"; break;
    case FLX_SURFACE_FIELDS_UNKNOWN: what = "fields has a bit beyond FLX_SURFACE_TPO"; break;
    case FLX_SURFACE_TEXTURE_WIDTH: what = "texture_width is less than 1"; break;
    case FLX_SURFACE_PARAMS_NULL: what = "params is NULL"; break;
    case FLX_SURFACE_SIZE: what = "width or height is 0"; break;
    case FLX_SURFACE_TILE: what = "the tile policy does not name the whole frame (0/0/0 or x/0/1)"; break;
    case FLX_SURFACE_PIXELS: what = "the frame has more than 2^32 - 1 pixels"; break;
    case FLX_SURFACE_NULL: what = "an array is NULL"; break;
    case FLX_SURFACE_WRAPS: what = "the rows leave the address space"; break;
    case FLX_SURFACE_OVERLAP: what = "the rays and the planes overlap"; break;
  }
  return fail(ctx, FLX_ERR_INVALID, (std::string(call) + ": " + what).c_str());
}

/* the hit scratch holds `rows` float4 and the launches' words are there */
static flx_status surface_scratch(flx_context *ctx, size_t rows) { return flx_grow(ctx, flx_need(&ctx->d_trace_hits, rows), flx_need(&ctx->d_trace_ctl, 4)); }

extern "C" flx_status flx_rays_surface_device(flx_context *ctx, int32_t texture_width, const void *d_rays, uint32_t n, uint32_t fields, void *d_out, void *producer_stream) {
  static const char *const call = "flx_rays_surface_device";
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = flx_scene_refused(ctx, call);
  if (s || (s = surface_refusal(ctx, flx_surface_fields_check(fields, texture_width), call)) || n == 0) return s;
  uint64_t out_bytes = 0;
  const enum flx_surface_refusal arrays = flx_surface_arrays_check(1, (uint64_t)(uintptr_t)d_rays, (uint64_t)(uintptr_t)d_out, n, fields, &out_bytes);
  if (arrays != FLX_SURFACE_ARGS_OK && arrays != FLX_SURFACE_OVERLAP) return surface_refusal(ctx, arrays, call);      /* (overlap: said after the pointers are known to be the device's) */
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  if (!flx_rows_on_device(ctx, d_rays, (size_t)n * FLX_RAY_ROW_BYTES))
    return fail(ctx, FLX_ERR_INVALID, "flx_rays_surface_device: the rays are not n rows in memory of the context's device, 16-byte aligned");
  if (!flx_rows_on_device(ctx, d_out, (size_t)out_bytes))
    return fail(ctx, FLX_ERR_INVALID, "flx_rays_surface_device: the planes are not popcount(fields) * n rows in memory of the context's device, 16-byte aligned");
  if (arrays == FLX_SURFACE_OVERLAP) return surface_refusal(ctx, arrays, call);
  SurfaceArgs sa;
  memset(&sa, 0, sizeof sa);
  if ((s = flx_make_scene(ctx, sa.sc))) return s;            /* (refuses a scene that names a transform not uploaded) */
  if ((s = flx_server_stop(ctx))) return s;                  /* as flx_render_device: the frame server's launch ends after the frames posted to it */
  sa.texture_width = (float)texture_width;
  flx_ray_slabs cut(ctx, 1u, n);
  if ((s = surface_scratch(ctx, (size_t)cut.most * 2u))) return s;
  if ((s = flx_wait_for_producer(ctx, producer_stream))) return s;
  s = flx_rays_slabs(ctx, sa.sc, d_rays, n, cut, call, [&](uint64_t first, uint32_t m, const float4 *rays) -> flx_status {
    hipLaunchKernelGGL(k_surface<false>, dim3((m + 255u) / 256u), dim3(256), 0, ctx->stream, sa, rays, (const float4 *)ctx->d_trace_hits.get(), (float4 *)d_out + first, m,
                       (size_t)n, fields);
    FLX_HIP(ctx, hipGetLastError());
    return FLX_OK;
  });
  if (s) return s;
  flx_context::SurfaceLaunch ran;
  ran.n = n; ran.fields = fields; ran.slab = cut.slab; ran.slabs = cut.slabs; ran.query_groups = cut.query.groups;
  ctx->last_surface = ran;
  return FLX_OK;
}

extern "C" flx_status flx_rays_surface(flx_context *ctx, int32_t texture_width, const float *rays, uint32_t n, uint32_t fields, void *out) {
  static const char *const call = "flx_rays_surface";
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = flx_scene_refused(ctx, call);
  if (s || (s = surface_refusal(ctx, flx_surface_fields_check(fields, texture_width), call)) || n == 0) return s;
  if (!rays || !out) return surface_refusal(ctx, FLX_SURFACE_NULL, call);
  return flx_rays_from_host(ctx, rays, n, [&]() { return flx_rays_surface_device(ctx, texture_width, ctx->d_query_rays, n, fields, ctx->d_query_hits, nullptr); },
                            flx_down(&ctx->d_query_hits, (size_t)n * flx_surface_planes(fields), out));
}

/* what both frame calls refuse before they look at the output (flx_context.h: flx_volume.hip asks the same for flx_frame_irradiance) */
flx_status flx_frame_surface_refused(flx_context *ctx, const flx_frame_params *p, uint32_t fields, const char *call) {
  flx_status s = flx_scene_refused(ctx, call);
  if (s) return s;
  if (!p) return surface_refusal(ctx, FLX_SURFACE_PARAMS_NULL, call);
  if ((s = surface_refusal(ctx, flx_surface_fields_check(fields, p->texture_width), call))) return s;
  return surface_refusal(ctx, flx_surface_frame_check(1, p->width, p->height, p->tile_rows, p->tile_index, p->tile_count), call);
}

extern "C" flx_status flx_frame_surface_device(flx_context *ctx, const flx_frame_params *params, uint32_t fields, void *d_out) {
  static const char *const call = "flx_frame_surface_device";
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = flx_frame_surface_refused(ctx, params, fields, call);
  if (s) return s;
  const uint32_t n = params->width * params->height;          /* (fits: flx_surface_frame_check) */
  uint64_t out_bytes = 0;
  if ((s = surface_refusal(ctx, flx_surface_arrays_check(0, 0u, (uint64_t)(uintptr_t)d_out, n, fields, &out_bytes), call))) return s;
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  if (!flx_rows_on_device(ctx, d_out, (size_t)out_bytes))
    return fail(ctx, FLX_ERR_INVALID, "flx_frame_surface_device: the planes are not popcount(fields) * width * height rows in memory of the context's device, 16-byte aligned");
  /* the frame k_primary is given: the canvas, the camera and the view of the caller's params, the whole frame; nothing else of them is read */
  flx_frame_params whole;
  memset(&whole, 0, sizeof whole);
  whole.width = params->width; whole.height = params->height;
  memcpy(whole.camera, params->camera, sizeof whole.camera);
  memcpy(whole.view_matrix, params->view_matrix, sizeof whole.view_matrix);
  whole.samples = 1;
  whole.texture_width = params->texture_width;
  SurfaceArgs sa;
  memset(&sa, 0, sizeof sa);
  DeviceFrame fr;
  memset(&fr, 0, sizeof fr);
  if ((s = flx_make_frame(ctx, &whole, sa.sc, fr))) return s;      /* (refuses a scene that names a transform not uploaded) */
  if ((s = flx_server_stop(ctx))) return s;                  /* as flx_render_device: the frame server's launch ends after the frames posted to it */
  sa.texture_width = fr.texture_width;
  sa.width = fr.width; sa.height = fr.height;
  sa.view = fr.view[0];
  if ((s = surface_scratch(ctx, n))) return s;
  launch_primary(sa.sc, fr, ctx->d_trace_hits, nullptr, ctx->stream);
  FLX_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_surface<true>, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, sa, (const float4 *)nullptr, (const float4 *)ctx->d_trace_hits.get(), (float4 *)d_out, n,
                     (size_t)n, fields);
  FLX_HIP(ctx, hipGetLastError());
  flx_context::SurfaceLaunch ran;
  ran.n = n; ran.fields = fields; ran.slab = n; ran.slabs = 1u; ran.frame = 1u;
  ctx->last_surface = ran;
  return FLX_OK;
}

extern "C" flx_status flx_frame_surface(flx_context *ctx, const flx_frame_params *params, uint32_t fields, void *out) {
  static const char *const call = "flx_frame_surface";
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = flx_frame_surface_refused(ctx, params, fields, call);
  if (s) return s;
  if (!out) return surface_refusal(ctx, FLX_SURFACE_NULL, call);
  return flx_rays_from_host(ctx, nullptr, 0u, [&]() { return flx_frame_surface_device(ctx, params, fields, ctx->d_query_hits); },
                            flx_down(&ctx->d_query_hits, (size_t)params->width * params->height * flx_surface_planes(fields), out));
}

extern "C" flx_status flx_debug_last_surface(flx_context *ctx, uint32_t out[8]) {
  if (!ctx || !out) return FLX_ERR_INVALID;
  memset(out, 0, 8 * sizeof(uint32_t));
  const flx_context::SurfaceLaunch &t = ctx->last_surface;
  out[0] = t.slabs; out[1] = t.slab; out[2] = t.n; out[3] = t.fields; out[4] = t.frame; out[5] = t.query_groups;
  return FLX_OK;
}
