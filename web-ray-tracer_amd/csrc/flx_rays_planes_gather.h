/* flx_rays_planes_gather.h — what flx_rays_planes.hip and flx_camera.hip need of flx_rays_planes_gather.hip ("ray images with a volume"): the volume of a call as its
 * refusals leave it, and the ONE launch of k_rays_planes_gather, which the planes calls' own slab loop makes where it launches k_rays_planes without a volume.
 * Private to the library. */
#ifndef FLX_RAYS_PLANES_GATHER_H
#define FLX_RAYS_PLANES_GATHER_H

#include "flx_context.h"
#include "flx_planes_gather_args.h"

/* an accepted flx_gather_volume: its arrays (maps, offsets: NULL for none), its grid and map by value (no map: zeros), the gain; flags:
 * flx_planes_gather_flags */
struct flx_planes_volume {
  const float4 *sh, *maps, *offsets;
  flx_volume_grid grid;
  flx_volume_map map;
  float gain;
  uint32_t flags;
};

/* flx_rays_trace_gather_device's refusals of a volume, in its order and its words under `call` — NULL, the grid, the map, the arrays, the gain, the reserved word, map
 * and maps —, then an array of the volume that shares a byte with one of the call's kc arrays.  FLX_OK: *out is the volume.  Nothing is enqueued. */
flx_status flx_planes_gather_volume_refused(flx_context *ctx, const flx_gather_volume *volume, const flx_planes_gather_array *call_arrays, int kc, const char *call,
                                            flx_planes_volume *out);

/* k_rays_planes_gather<lock, mode, a map, offsets> over a slab on the context's stream: k_rays_planes' arguments (mode: flx_rays_planes.hip's RayPlanesMode as a
 * number; rings and packed: its RayTemporalArgs, not read in mode 0) and the volume.  It records what ran for flx_debug_last_planes_gather but n and slabs, which the
 * caller's slab loop knows (flx_planes_gather_ran). */
flx_status flx_planes_gather_launch(flx_context *ctx, bool lock, int mode, uint32_t groups, const flx::DeviceScene &sc, const flx::DeviceFrame &fr, const float4 *rays,
                                    const float4 *hits, uint32_t *out8, float4 *out32, uint32_t *queue, uint32_t m, size_t stride, uint32_t *rings, uint32_t packed,
                                    const flx_planes_volume &volume);
/* the whole call succeeded: its rays, its slabs and the rays of a full slab beside what the last launch recorded */
void flx_planes_gather_ran(flx_context *ctx, uint32_t n, uint32_t slabs, uint32_t slab);

#endif
