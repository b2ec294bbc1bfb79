/*
 * flx_gather.h — the ambient term of a traced path taken from a probe volume, exactly defined (include/flexlight_hip_debug.h, "ray batches with a volume":
 * flx_rays_trace_gather, flx_rays_trace_gather_device).
 *
 * A path of flx_rays_trace ends in finalColor + importancyFactor * ambient, `ambient` the params' constant: the stand-in for all the light the path did not trace.
 * Here it ends in finalColor + importancyFactor * A, per component, the product first, and A comes from a volume:
 *   THE LAST POINT of a path is the surface point of the last bounce iteration it shaded: x the ray origin of that iteration (the hit point), n that iteration's
 *     smooth normal facing the arriving ray — the floats a FLX_SURFACE_NORMAL row holds for the ray that arrived there.  A path that shaded nothing has none.
 *   THE LOOKUP E = (e0, e1, e2, W) is the volume's lookup of the position row (x, 1.0f) and the normal n: flx_volume_lookup with neither offsets nor map,
 *     flx_volume_map_lookup with a map, flx_volume_relocate_lookup with offsets (with or without a map).  THOSE FUNCTIONS ARE CALLED, not restated.
 *   THE VALUE A_c = (W > 0.0f) ? e_c * gain : ambient[c].  A NaN W takes the constant, and so does a path without a last point.
 * Everything else of a row — the loop guard, the bounces, the walks, the noise, the sum over samples, the scale, originalColor — is flx_rays_trace's.
 * float32, ONE OPERATION PER ROUNDING, compiled with -ffp-contract=off like everything that shares flx_math.h.  The kernels (web-ray-tracer_amd/csrc/
 * flx_rays_gather.hip: k_gather_ambient) and the CPU reference of the tests (tests/rays_gather_ref/flx_rays_gather_ref.c) compile THIS text.  Plain C99, also valid
 * C++ / HIP.  A numerical definition, not a renderer.
 */
#ifndef FLX_GATHER_H
#define FLX_GATHER_H

#include "flx_volume.h"
#include "flx_volume_map.h"
#include "flx_volume_relocate.h"

#define FLX_GATHER_RECORD_PLANES 4u      /* a path record: four float4 — finalColor + bounce iterations; importancyFactor + has-point flag; x; n */
#define FLX_GATHER_RECORD_BYTES 64u

/* THE VALUE: e the lookup's row (not read where the path has no last point), has_point 0 or 1 -> A */
FLX_HD void flx_gather_ambient(const flx_trace_params *params, float gain, int has_point, const float e[4], float a[3]) {
  const int lit = has_point && e[3] > 0.0f;      /* (a NaN W is not > 0) */
  const float g0 = e[0] * gain, g1 = e[1] * gain, g2 = e[2] * gain;
  a[0] = lit ? g0 : params->ambient[0];
  a[1] = lit ? g1 : params->ambient[1];
  a[2] = lit ? g2 : params->ambient[2];
}

/* THE PATH VALUE: finalColor + importancyFactor * A per component, the product first */
FLX_HD void flx_gather_path_value(const float final_color[3], const float importancy[3], const float a[3], float out[3]) {
  const float p0 = importancy[0] * a[0], p1 = importancy[1] * a[1], p2 = importancy[2] * a[2];
  out[0] = final_color[0] + p0; out[1] = final_color[1] + p1; out[2] = final_color[2] + p2;
}

/* THE LOOKUP over rows in memory: which of the three forms a volume takes (map and maps both NULL: none; offsets NULL: probes on the lattice).  position: (x, 1.0f);
 * normal: word 3 is ignored. */
FLX_HD void flx_gather_lookup(const flx_volume_grid *g, const flx_volume_map *map, const float *rows, const float *maps, const float *offsets, const float position[4],
                              const float normal[4], float out[4]) {
  if (offsets) flx_volume_relocate_lookup(g, map, rows, maps, offsets, position, normal, out);
  else if (map) flx_volume_map_lookup(g, map, rows, maps, position, normal, out);
  else flx_volume_lookup(g, rows, position, normal, out);
}

#endif /* FLX_GATHER_H */
