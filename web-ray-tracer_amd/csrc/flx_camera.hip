/* flx_camera.hip — the rays of cameras made on the device (include/flexlight_hip_debug.h, "cameras": flx_camera_rays[_device], flx_camera_image[_device],
 * flx_camera_image_temporal[_device]).
 *
 * k_camera_rays: ONE LANE PER RAY.  The arithmetic is include/flx_camera.h's (flx_camera_ray), the text the tests' CPU reference compiles too: the rows are defined
 * bit for bit.  A lane writes its 32-byte row as two 16-byte vector stores, the layout of every ray kernel's rows (flx_query.hip); consecutive lanes write
 * consecutive rows, so a wave's two stores cover 2 KB without a gap.  The grid's y names the camera: a workgroup works for one camera, whose projection and face are
 * uniform — the switch between the projections is a scalar branch — and whose fields are read from the kernel's arguments by scalar loads.  The cameras travel AS
 * KERNEL ARGUMENTS, CAMERA_BATCH of them a launch (a stereo pair, a probe's six faces and any batch up to 32 cameras are one launch; more cameras take further
 * launches on the same stream): nothing is staged and the host waits for nothing.  A pinhole's view matrix is inverted once on the host (flx_camera_prepare).
 * A region shifts the pixel a lane computes, nothing else: sx, sy and the noise words are the whole image's.
 * Nothing to tune beyond the stores: the kernel has no loads but its arguments, no LDS and no scratch (profiles/camera_rays.txt).
 *
 * The image calls make one camera's rays into ctx->d_camera_rays and hand them to flx_rays_image_device / flx_rays_image_temporal_device (flx_rays_planes.hip) on
 * the same stream: there is no second implementation of either.  The host-memory calls are the ray-batch calls' shared path (flx_rays_host.h) with no rays to
 * copy up. */
#include <string>

#include "flx_camera.h"
#include "flx_camera_args.h"
#include "flx_context.h"
#include "flx_ray_planes_args.h"
#include "flx_ray_temporal_args.h"
#include "flx_rays_host.h"
#include "flx_rays_planes_gather.h"

namespace flx {

constexpr uint32_t CAMERA_BATCH = 32u;                 /* cameras a launch takes in its arguments: 32 x 72 bytes of the 4 KB kernarg segment */
constexpr uint32_t CAMERA_THREADS = 256u;
struct CameraBatch { flx_camera_setup cam[CAMERA_BATCH]; };
static_assert(sizeof(CameraBatch) + 64 <= 4096, "the cameras fit a 4 KB kernarg segment");

/* rays: the first row of the launch's first camera; the image is width x height, the rows written are those of its pixels [x0, x0 + w) x [y0, ..), `pixels` of
 * them a camera, in row order; camera blockIdx.y's start at row blockIdx.y * pixels.  blockIdx.x * 256 + threadIdx.x <= 2^32 - 1: the grid's x is at most 2^24. */
__global__ __launch_bounds__(CAMERA_THREADS) void k_camera_rays(CameraBatch batch, float4 *__restrict__ rays, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t w,
                                                                uint32_t pixels) {
  const uint32_t i = blockIdx.x * CAMERA_THREADS + threadIdx.x;
  if (i >= pixels) return;
  const uint32_t ry = i / w, rx = i - ry * w;
  const flx_camera_row r = flx_camera_ray(&batch.cam[blockIdx.y], width, height, x0 + rx, y0 + ry);
  float4 *o = rays + ((size_t)blockIdx.y * pixels + i) * 2u;
  o[0] = make_float4(r.ox, r.oy, r.oz, r.noise_x);
  o[1] = make_float4(r.dx, r.dy, r.dz, r.noise_y);
}

}  // namespace flx

using namespace flx;

/* ---- the calls ------------------------------------------------------------------------------------------------------------------------------------- */

static flx_status fail(flx_context *ctx, flx_status code, const std::string &msg) { return flx_fail(ctx, code, msg.c_str()); }

/* a refusal of flx_camera_args.h in words; which: the camera it is about, where it is about one */
static flx_status camera_refusal(flx_context *ctx, enum flx_camera_refusal why, const char *call, uint32_t which = 0u) {
  const char *what = "";
  bool one = true;
  switch (why) {
    case FLX_CAMERA_ARGS_OK: return FLX_OK;
    case FLX_CAMERA_NONE: what = "cameras is NULL or n_cameras is 0"; one = false; break;
    case FLX_CAMERA_SIZE: what = "width or height is 0"; one = false; break;
    case FLX_CAMERA_RAYS: what = "n_cameras * width * height is 2^32 or more"; one = false; break;
    case FLX_CAMERA_REGION_EMPTY: what = "the region is empty"; one = false; break;
    case FLX_CAMERA_REGION_OUTSIDE: what = "the region leaves the image"; one = false; break;
    case FLX_CAMERA_PROJECTION: what = "projection is none of FLX_CAMERA_PINHOLE .. FLX_CAMERA_CUBE_FACE"; break;
    case FLX_CAMERA_FACE: what = "face is not one of 0 .. 5"; break;
    case FLX_CAMERA_NOT_FINITE: what = "position, basis, extent or jitter holds a value that is not finite"; break;
    case FLX_CAMERA_JITTER: what = "jitter is outside [-0.5, 0.5]"; break;
    case FLX_CAMERA_EXTENT: what = "an extent the projection reads is not above 0"; break;
    case FLX_CAMERA_OUT_NULL: what = "the output is NULL"; one = false; break;
    case FLX_CAMERA_OUT_WRAPS: what = "the rows leave the address space"; one = false; break;
  }
  return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": " + (one ? "camera " + std::to_string(which) + ": " : std::string()) + what);
}

/* the batch and every camera of it; *span <- what the call writes */
static flx_status cameras_refused(flx_context *ctx, const flx_camera *cameras, uint32_t n_cameras, uint32_t width, uint32_t height, const uint32_t *region,
                                  flx_camera_span *span, const char *call) {
  flx_status s = camera_refusal(ctx, flx_camera_batch_check(cameras != nullptr, n_cameras, width, height, region, span), call);
  if (s) return s;
  uint32_t which = 0u;
  const enum flx_camera_refusal why = flx_cameras_check(cameras, n_cameras, &which);
  return camera_refusal(ctx, why, call, which);
}

/* The launches, the arguments accepted: the rows of `span` for every camera into d_rays.  Ordered as flx_rays_cast_device's launch is: behind the frame server's
 * launch, on the context's stream. */
static flx_status camera_enqueue(flx_context *ctx, const flx_camera *cameras, uint32_t n_cameras, uint32_t width, uint32_t height, const flx_camera_span &span, void *d_rays) {
  flx_status s;
  if ((s = flx_server_stop(ctx))) return s;
  const uint32_t pixels = span.w * span.h;                /* (a camera's rows; span.rays = pixels * n_cameras < 2^32) */
  const uint32_t groups = (uint32_t)(((uint64_t)pixels + CAMERA_THREADS - 1u) / CAMERA_THREADS);
  for (uint32_t first = 0; first < n_cameras; first += CAMERA_BATCH) {
    const uint32_t m = n_cameras - first < CAMERA_BATCH ? n_cameras - first : CAMERA_BATCH;
    CameraBatch batch;
    for (uint32_t k = 0; k < CAMERA_BATCH; k++) batch.cam[k] = flx_camera_prepare(cameras + first + (k < m ? k : 0u));      /* (the slots past m: a copy of the first, never read) */
    hipLaunchKernelGGL(k_camera_rays, dim3(groups, m), dim3(CAMERA_THREADS), 0, ctx->stream, batch, (float4 *)d_rays + (size_t)first * pixels * 2u, width, height, span.x0, span.y0,
                       span.w, pixels);
    FLX_HIP(ctx, hipGetLastError());
  }
  return FLX_OK;
}

extern "C" flx_status flx_camera_rays_device(flx_context *ctx, const flx_camera *cameras, uint32_t n_cameras, uint32_t width, uint32_t height, const uint32_t region[4], void *d_rays) {
  static const char *const call = "flx_camera_rays_device";
  if (!ctx) return FLX_ERR_INVALID;
  flx_camera_span span;
  flx_status s = cameras_refused(ctx, cameras, n_cameras, width, height, region, &span, call);
  if (s || (s = camera_refusal(ctx, flx_camera_out_check((uint64_t)(uintptr_t)d_rays, span.rays), call))) return s;
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  if (!flx_rows_on_device(ctx, d_rays, (size_t)span.rays * FLX_RAY_ROW_BYTES))
    return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": the output is not n_cameras * w * h rows in memory of the context's device, 16-byte aligned");
  return camera_enqueue(ctx, cameras, n_cameras, width, height, span, d_rays);
}

extern "C" flx_status flx_camera_rays(flx_context *ctx, const flx_camera *cameras, uint32_t n_cameras, uint32_t width, uint32_t height, const uint32_t region[4], float *rays) {
  static const char *const call = "flx_camera_rays";
  if (!ctx) return FLX_ERR_INVALID;
  flx_camera_span span;
  flx_status s = cameras_refused(ctx, cameras, n_cameras, width, height, region, &span, call);
  if (s) return s;
  if (!rays) return camera_refusal(ctx, FLX_CAMERA_OUT_NULL, call);
  return flx_rays_from_host(ctx, nullptr, 0u, [&]() { return flx_camera_rays_device(ctx, cameras, n_cameras, width, height, region, ctx->d_query_hits); },
                            flx_down(&ctx->d_query_hits, (size_t)span.rays * 2u, rays));
}

/* What the image calls look at before anything is enqueued, in flx_rays_image[_temporal]'s order — the scene and the params, the size, the temporal — and then the
 * camera.  A refusal that is flx_rays_image[_temporal]_device's own is asked of that call, which looks at those before it looks at an array: its words.
 * *n <- width * height. */
static flx_status image_refused(flx_context *ctx, const flx_trace_params *params, bool over_time, const flx_ray_temporal *temporal, int hdr, const flx_camera *camera, uint32_t width,
                                uint32_t height, uint32_t *n, const char *call, bool gather = false, const flx_gather_volume *volume = nullptr) {
  flx_status s = flx_trace_params_refused(ctx, params, call);
  if (s) return s;
  const bool theirs = flx_ray_image_size_check(width, height, n) != FLX_RAY_PLANES_ARGS_OK ||
                      (over_time && flx_ray_temporal_check(temporal != nullptr, temporal ? temporal->history : 0, temporal ? temporal->use_filter : 0, temporal ? temporal->hdr : 0) !=
                                        FLX_RAY_TEMPORAL_ARGS_OK);
  if (theirs && gather)      /* "ray images with a volume": the same of the calls that take one */
    return over_time ? flx_rays_image_temporal_gather_device(ctx, params, volume, temporal, nullptr, width, height, nullptr, nullptr)
                     : flx_rays_image_gather_device(ctx, params, volume, hdr, nullptr, width, height, nullptr, nullptr);
  if (theirs)
    return over_time ? flx_rays_image_temporal_device(ctx, params, temporal, nullptr, width, height, nullptr, nullptr) : flx_rays_image_device(ctx, params, hdr, nullptr, width, height, nullptr, nullptr);
  flx_camera_span span;
  return cameras_refused(ctx, camera, 1u, width, height, nullptr, &span, call);
}

/* Both image calls: the camera's rays into the context's buffer, then the ray-image call on them.  temporal NULL: flx_rays_image_device with hdr.  With `gather` the
 * calls that take a volume: its refusals behind the image's, before the rays are made, then flx_rays_image[_temporal]_gather_device. */
static flx_status image_device(flx_context *ctx, const flx_trace_params *params, bool over_time, const flx_ray_temporal *temporal, int hdr, const flx_camera *camera, uint32_t width,
                               uint32_t height, void *d_out_rgba, const char *call, bool gather = false, const flx_gather_volume *volume = nullptr) {
  uint32_t n = 0;
  flx_status s = image_refused(ctx, params, over_time, temporal, hdr, camera, width, height, &n, call, gather, volume);
  if (s) return s;
  /* the image, looked at before the rays are made: a refusal enqueues nothing */
  if (!d_out_rgba) return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": the image is NULL");
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  if (flx_range_wraps((uint64_t)(uintptr_t)d_out_rgba, (uint64_t)n * FLX_RAY_PLANES_ROW32) || !flx_rows_on_device(ctx, d_out_rgba, (size_t)n * FLX_RAY_PLANES_ROW32))
    return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": the image is not width * height float4 in memory of the context's device, 16-byte aligned");
  if (gather) {
    flx_planes_gather_array mine[FLX_PLANES_GATHER_CALL_ARRAYS];
    const int kc = flx_planes_gather_image_arrays(0u, (uint64_t)(uintptr_t)d_out_rgba, n, mine);
    if ((s = flx_planes_gather_volume_refused(ctx, volume, mine, kc, call, nullptr))) return s;
  }
  if ((s = flx_grow(ctx, flx_need(&ctx->d_camera_rays, (size_t)n * 2u)))) return s;      /* (an earlier image may still read the rays that are about to go) */
  const flx_camera_span whole = { 0u, 0u, width, height, n };
  if ((s = camera_enqueue(ctx, camera, 1u, width, height, whole, ctx->d_camera_rays.get()))) return s;
  if (gather)
    return over_time ? flx_rays_image_temporal_gather_device(ctx, params, volume, temporal, ctx->d_camera_rays.get(), width, height, d_out_rgba, nullptr)
                     : flx_rays_image_gather_device(ctx, params, volume, hdr, ctx->d_camera_rays.get(), width, height, d_out_rgba, nullptr);
  return over_time ? flx_rays_image_temporal_device(ctx, params, temporal, ctx->d_camera_rays.get(), width, height, d_out_rgba, nullptr)
                   : flx_rays_image_device(ctx, params, hdr, ctx->d_camera_rays.get(), width, height, d_out_rgba, nullptr);
}

/* their host-memory twins: the image staged as flx_rays_image stages it */
static flx_status image_host(flx_context *ctx, const flx_trace_params *params, bool over_time, const flx_ray_temporal *temporal, int hdr, const flx_camera *camera, uint32_t width,
                             uint32_t height, float *out_rgba, const char *call, bool gather = false, const flx_gather_volume *volume = nullptr) {
  uint32_t n = 0;
  flx_status s = image_refused(ctx, params, over_time, temporal, hdr, camera, width, height, &n, call, gather, volume);
  if (s) return s;
  if (!out_rgba) return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": the image is NULL");
  if (gather && (s = flx_planes_gather_volume_refused(ctx, volume, nullptr, 0, call, nullptr))) return s;      /* (before anything is staged) */
  return flx_rays_from_host(ctx, nullptr, 0u, [&]() { return image_device(ctx, params, over_time, temporal, hdr, camera, width, height, ctx->d_query_hits, call, gather, volume); },
                            flx_down(&ctx->d_query_hits, n, out_rgba));
}

extern "C" flx_status flx_camera_image_device(flx_context *ctx, const flx_trace_params *params, int hdr, const flx_camera *camera, uint32_t width, uint32_t height, void *d_out_rgba) {
  if (!ctx) return FLX_ERR_INVALID;
  return image_device(ctx, params, false, nullptr, hdr, camera, width, height, d_out_rgba, "flx_camera_image_device");
}

extern "C" flx_status flx_camera_image(flx_context *ctx, const flx_trace_params *params, int hdr, const flx_camera *camera, uint32_t width, uint32_t height, float *out_rgba) {
  if (!ctx) return FLX_ERR_INVALID;
  return image_host(ctx, params, false, nullptr, hdr, camera, width, height, out_rgba, "flx_camera_image");
}

extern "C" flx_status flx_camera_image_temporal_device(flx_context *ctx, const flx_trace_params *params, const flx_ray_temporal *temporal, const flx_camera *camera, uint32_t width,
                                                       uint32_t height, void *d_out_rgba) {
  if (!ctx) return FLX_ERR_INVALID;
  return image_device(ctx, params, true, temporal, 0, camera, width, height, d_out_rgba, "flx_camera_image_temporal_device");
}

extern "C" flx_status flx_camera_image_temporal(flx_context *ctx, const flx_trace_params *params, const flx_ray_temporal *temporal, const flx_camera *camera, uint32_t width,
                                                uint32_t height, float *out_rgba) {
  if (!ctx) return FLX_ERR_INVALID;
  return image_host(ctx, params, true, temporal, 0, camera, width, height, out_rgba, "flx_camera_image_temporal");
}

/* ---- "ray images with a volume": the four calls above with a flx_gather_volume behind the params ------------------------------------------------------ */

extern "C" flx_status flx_camera_image_gather_device(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume, int hdr, const flx_camera *camera,
                                                     uint32_t width, uint32_t height, void *d_out_rgba) {
  if (!ctx) return FLX_ERR_INVALID;
  return image_device(ctx, params, false, nullptr, hdr, camera, width, height, d_out_rgba, "flx_camera_image_gather_device", true, volume);
}

extern "C" flx_status flx_camera_image_gather(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume, int hdr, const flx_camera *camera, uint32_t width,
                                              uint32_t height, float *out_rgba) {
  if (!ctx) return FLX_ERR_INVALID;
  return image_host(ctx, params, false, nullptr, hdr, camera, width, height, out_rgba, "flx_camera_image_gather", true, volume);
}

extern "C" flx_status flx_camera_image_temporal_gather_device(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume, const flx_ray_temporal *temporal,
                                                              const flx_camera *camera, uint32_t width, uint32_t height, void *d_out_rgba) {
  if (!ctx) return FLX_ERR_INVALID;
  return image_device(ctx, params, true, temporal, 0, camera, width, height, d_out_rgba, "flx_camera_image_temporal_gather_device", true, volume);
}

extern "C" flx_status flx_camera_image_temporal_gather(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume, const flx_ray_temporal *temporal,
                                                       const flx_camera *camera, uint32_t width, uint32_t height, float *out_rgba) {
  if (!ctx) return FLX_ERR_INVALID;
  return image_host(ctx, params, true, temporal, 0, camera, width, height, out_rgba, "flx_camera_image_temporal_gather", true, volume);
}
