/* flx_rays_host.h — the templates of the host path the ray-batch calls share (flx_query.hip, flx_rays_trace.hip, flx_surface.hip, flx_rays_planes.hip): growth of the
 * context's buffers behind one wait, the slab loop, the host-memory wrapper.  What is no template is declared in flx_context.h and defined in flx_query.hip.
 * Private to the library. */
#ifndef FLX_RAYS_HOST_H
#define FLX_RAYS_HOST_H

#include "flx_context.h"
#include "flx_query_args.h"

/* `buffer` must hold `count` elements; no buffer: nothing is asked (an output the caller did not want) */
template <typename T> struct flx_room { DeviceBuffer<T> *buffer; size_t count; };
template <typename T> flx_room<T> flx_need(DeviceBuffer<T> *buffer, size_t count) { return { buffer, count }; }

/* These buffers hold these counts.  Where one does not, the host waits ONCE for the context's stream — work in flight may still read or write what is about to go —
 * and each is grown, in the order given. */
template <typename... T> flx_status flx_grow(flx_context *ctx, const flx_room<T> &...rooms) {
  if (((!rooms.buffer || rooms.buffer->fits(rooms.count)) && ...)) return FLX_OK;
  FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  flx_status s = FLX_OK;
  (void)((rooms.buffer && (s = rooms.buffer->ensure(ctx, rooms.count)) != FLX_OK) || ...);
  return s;
}

/* A batch of n > 0 rays cut into slabs for `samples` slots a ray (flx_trace_slab_rays): the slab's size and the largest slab's, which the scratch is grown for; then
 * what flx_rays_slabs ran: the slabs and the last query launch. */
struct flx_ray_slabs {
  uint32_t slab, most, slabs = 0;
  flx::QueryLaunch query;
  flx_ray_slabs(const flx_context *ctx, uint32_t samples, uint32_t n) : slab(flx_trace_slab_rays(samples, ctx->trace_slab)), most(n < slab ? n : slab) {}
};

/* The slab loop.  Per slab: the control words zeroed and the first hits of its rays into d_trace_hits (flx_slab_first_hits), then the feature's own launches:
 * enqueue(first, m, rays) -> flx_status — the slab's first ray in the batch, its rays, their rows — which checks its launches itself. */
template <typename F> flx_status flx_rays_slabs(flx_context *ctx, const flx::DeviceScene &sc, const void *d_rays, uint32_t n, flx_ray_slabs &cut, const char *call, F &&enqueue) {
  for (uint64_t first = 0; first < n; first += cut.slab) {
    const uint32_t m = (uint32_t)(n - first < cut.slab ? n - first : cut.slab);
    const float4 *rays = (const float4 *)d_rays + first * 2u;
    flx_status s;
    if ((s = flx_slab_first_hits(ctx, sc, rays, m, call, cut.query)) || (s = enqueue(first, m, rays))) return s;
    cut.slabs++;
  }
  return FLX_OK;
}

/* An output of a host-memory call: `count` elements of the staging buffer come down to `host`; no host pointer: not asked for */
template <typename T> struct flx_host_out { DeviceBuffer<T> *staging; size_t count; void *host; };
template <typename T> flx_host_out<T> flx_down(DeviceBuffer<T> *staging, size_t count, void *host) { return { staging, count, host }; }
template <typename T> flx_status flx_copy_down(flx_context *ctx, const flx_host_out<T> &out) {
  if (out.host) FLX_HIP(ctx, hipMemcpyAsync(out.host, out.staging->get(), out.count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
  return FLX_OK;
}

/* The host-memory twin of a _device call: the staging grown (flx_grow), the n rays copied up into d_query_rays (rays NULL: the call takes none), device_call() ->
 * flx_status on the staging with no producer stream, the outputs copied down in the order given, and the host waits for them. */
template <typename F, typename... T> flx_status flx_rays_from_host(flx_context *ctx, const float *rays, uint32_t n, F &&device_call, const flx_host_out<T> &...outs) {
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  flx_status s;
  if ((s = flx_grow(ctx, flx_need(rays ? &ctx->d_query_rays : nullptr, (size_t)n * 2u), flx_need(outs.host ? outs.staging : nullptr, outs.count)...))) return s;
  if (rays) FLX_HIP(ctx, hipMemcpyAsync(ctx->d_query_rays, rays, (size_t)n * FLX_RAY_ROW_BYTES, hipMemcpyHostToDevice, ctx->stream));
  if ((s = device_call())) return s;
  (void)(((s = flx_copy_down(ctx, outs)) != FLX_OK) || ...);
  if (s) return s;
  FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return FLX_OK;
}

#endif
