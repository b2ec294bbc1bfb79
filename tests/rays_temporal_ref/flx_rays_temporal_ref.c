/*
 * flx_rays_temporal_ref.c — CPU reference of what flx_rays_image_temporal traces per ray (include/flexlight_hip_debug.h, "ray images over time").  TEST
 * INFRASTRUCTURE ONLY: built by the test modules that need it (tests/rays_temporal_ref/flx_rays_temporal_ref.py) with the oracle's flags into a directory outside
 * git; the product never links it.
 *
 * One exported function.  It says nothing of its own about tracing: it includes the oracle's source and calls the oracle's own static rayTracerImpl and lightTrace,
 * so a ray's SIX rows are what fragment_main (oracle/flx_oracle.c:557-619) writes for a pixel with is_temporal == 1 and use_filter as params gives it — the globals
 * initialised once, the samples run in order on that one Frag — with the row's ray where fragment_main has the camera's: origin for `camera`, the direction as
 * given, the row's two noise coordinates for the pixel's NDC.  (-Wl,-Bsymbolic keeps this library's copy of the oracle's exported names to itself, beside
 * libflx_oracle.so in one process.)
 */
#include "../../oracle/flx_oracle.c"

/* rays: n rows of 8 floats (origin, noise x, direction, noise y); planes: float[6][n][4], before quantisation: renderColor, renderColorIp, renderOriginalColor,
 * renderId, renderOriginalId (flx_render_planes_device's order) and renderLocationId; hits: n bytes, 1 where the ray hits (may be NULL).  Of `params` it reads
 * samples, max_reflections, min_importancy, ambient, random_seed, texture_width and use_filter (0 or 1).  -> 0, or FLX_ERR_INVALID */
int flx_rays_temporal_ref(const flx_scene_view *scene, const flx_frame_params *params, const float *rays, float *planes, uint8_t *hits, uint32_t n, int threads) {
  if (!scene || !params || !scene->geometry || !scene->attributes || !scene->rotation || !scene->shift || (n && (!rays || !planes))) return FLX_ERR_INVALID;
  if (params->samples < 1 || params->max_reflections < 0 || params->texture_width < 1 || (params->use_filter != 0 && params->use_filter != 1)) return FLX_ERR_INVALID;
#ifdef _OPENMP
  if (threads > 0) omp_set_num_threads(threads);
#else
  (void)threads;
#endif
#pragma omp parallel
  {
    Frag f;
    memset(&f, 0, sizeof f);
    f.sc = scene; f.fp = params;
#pragma omp for schedule(dynamic, 16)
    for (uint32_t k = 0; k < n; k++) {
      const float *q = rays + (size_t)k * 8;
      float *row[6];
      for (int p = 0; p < 6; p++) {
        row[p] = planes + ((size_t)p * n + k) * 4;
        memset(row[p], 0, 4 * sizeof(float));               /* not covered: every target stays at the clear colour */
      }
      const v3 origin = V3(q[0], q[1], q[2]), dir = V3(q[4], q[5], q[6]);
      Ray ray = { origin, dir };
      uint64_t visits = 0;
      Hit hit = rayTracerImpl(scene, ray, 0, 0.0f, &visits);
      if (hits) hits[k] = hit.triangleId != -1;
      if (hit.triangleId == -1) continue;
      /* fragment_main from its first line to the targets it writes (oracle/flx_oracle.c), is_temporal == 1 */
      f.firstRayLength = 1.0f; f.glassFilter = 0.0f; f.originalRMEx = 0.0f; f.originalTPOx = 0.0f;
      f.originalColor = V3(0.0f, 0.0f, 0.0f);
      f.renderId.x = f.renderId.y = f.renderId.z = f.renderId.w = 0.0f;
      f.renderOriginalId = f.renderId;
      f.ndc = V3(q[3], q[7], 1.0f);
      v3 finalColor = V3(0.0f, 0.0f, 0.0f);
      for (int i = 0; i < params->samples; i++) {
        float cosSampleN = flx_cos((float)i);
        finalColor = add3(finalColor, lightTrace(&f, hit, dir, origin, cosSampleN, params->max_reflections));
      }
      float invSamples = 1.0f / (float)params->samples;
      finalColor = scale3(finalColor, invSamples);
      if (params->use_filter == 1) {
        row[1][3] = f.glassFilter;
      } else {
        finalColor = mul3(finalColor, f.originalColor);
        row[1][3] = 1.0f;
      }
      row[0][0] = flx_fract(finalColor.x); row[0][1] = flx_fract(finalColor.y); row[0][2] = flx_fract(finalColor.z); row[0][3] = 1.0f;
      row[1][0] = flx_floor(finalColor.x) * INV_256; row[1][1] = flx_floor(finalColor.y) * INV_256; row[1][2] = flx_floor(finalColor.z) * INV_256;
      row[2][0] = f.originalColor.x; row[2][1] = f.originalColor.y; row[2][2] = f.originalColor.z;
      row[2][3] = flx_min(f.originalRMEx, f.firstRayLength) + INV_255;
      row[3][0] = f.renderId.x; row[3][1] = f.renderId.y; row[3][2] = f.renderId.z; row[3][3] = f.renderId.w + INV_255;
      row[4][0] = 0.0f; row[4][1] = 0.0f; row[4][2] = 0.0f; row[4][3] = f.originalTPOx + INV_255;
      /* fragment:640-642; relativePosition is in object space, the origin in world space, as in the shader */
      const float *g = scene->geometry + (size_t)hit.triangleId * 12;
      float w0 = 1.0f - hit.suv.y - hit.suv.z;
      v3 rel = add3(add3(scale3(V3(g[0], g[1], g[2]), w0), scale3(V3(g[3], g[4], g[5]), hit.suv.y)), scale3(V3(g[6], g[7], g[8]), hit.suv.z));
      float div = 2.0f * distance3(rel, origin);
      row[5][0] = flx_mod(rel.x, div) / div; row[5][1] = flx_mod(rel.y, div) / div; row[5][2] = flx_mod(rel.z, div) / div; row[5][3] = INV_255;
    }
  }
  return FLX_OK;
}
