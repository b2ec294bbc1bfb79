/* flx_volume_map_host.h — what the directional-visibility calls share across files (defined in flx_volume_map.hip): the map's refusals in words, the maps
 * array's, and the launches of k_probe_map.  flx_probes.hip's chunk loop and flx_volume.hip's lookups take an optional map through these.  Private to the library. */
#ifndef FLX_VOLUME_MAP_HOST_H
#define FLX_VOLUME_MAP_HOST_H

#include "flx_context.h"
#include "flx_probe.h"
#include "flx_volume_map_args.h"

/* an array of a call beside the maps: where it lies, for the overlap */
struct flx_map_other { const void *p; uint64_t bytes; };

/* the map and its rows for n_probes probes: FLX_OK and *rows, or the refusal in words */
flx_status flx_volume_map_refused(flx_context *ctx, const flx_volume_map *map, uint32_t n_probes, uint32_t *rows, const char *call);
/* the maps array of `rows` rows against the k other arrays of the call, which their own check has accepted: there, inside 64 bits, memory of the context's device,
 * and apart — in that order */
flx_status flx_volume_maps_refused(flx_context *ctx, const void *d_maps, uint32_t rows, const flx_map_other *others, int k, const char *call);
/* the launches of k_probe_map for n probes' radiance rows, 32 768 probes a launch, on the context's stream; `all`: the probes of the whole call, for
 * flx_debug_last_volume_map */
flx_status flx_probe_map_enqueue(flx_context *ctx, const float4 *d_radiance, uint32_t n, const flx_probe_grid &g, const flx_volume_map &map, float4 *d_maps, uint32_t all);

#endif
