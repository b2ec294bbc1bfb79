/*
 * flx_rays_trace_ref.c — CPU reference of flx_rays_trace (include/flexlight_hip_debug.h, "ray queries").  TEST INFRASTRUCTURE ONLY: built by the test modules
 * that need it (tests/rays_trace_ref/flx_rays_trace_ref.py) with the oracle's flags into a directory outside git; the product never links it.
 *
 * One exported function.  It says nothing of its own about tracing: it includes the oracle's source and calls the oracle's own static rayTracerImpl and lightTrace,
 * so a row is what fragment_main (oracle/flx_oracle.c) computes for a pixel without filter and without temporal, with the row's ray where fragment_main has the
 * camera's: origin for `camera`, the direction as given, the row's two noise coordinates for the pixel's NDC.  (-Wl,-Bsymbolic keeps this library's copy of the
 * oracle's exported names to itself, beside libflx_oracle.so in one process.)
 */
#include "../../oracle/flx_oracle.c"

/* rays: n rows of 8 floats (origin, noise x, direction, noise y); out: n rows of 8 words (r g b, alpha | s, entry, 2 x transform, shades).  Of `params` it reads
 * samples, max_reflections, min_importancy, ambient, random_seed and texture_width.  -> 0, or FLX_ERR_INVALID */
int flx_rays_trace_ref(const flx_scene_view *scene, const flx_frame_params *params, const float *rays, uint32_t *out, uint32_t n, int threads) {
  if (!scene || !params || !scene->geometry || !scene->attributes || !scene->rotation || !scene->shift || (n && (!rays || !out))) return FLX_ERR_INVALID;
  if (params->samples < 1 || params->max_reflections < 0 || params->texture_width < 1) return FLX_ERR_INVALID;
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
      uint32_t *o = out + (size_t)k * 8;
      const v3 origin = V3(q[0], q[1], q[2]), dir = V3(q[4], q[5], q[6]);
      Ray ray = { origin, dir };
      uint64_t visits = 0;
      Hit hit = rayTracerImpl(scene, ray, 0, 0.0f, &visits);
      memset(o, 0, 8 * sizeof(uint32_t));
      o[5] = 0xffffffffu;
      if (hit.triangleId == -1) continue;
      /* fragment_main from its first line to the colour it writes (oracle/flx_oracle.c) */
      f.firstRayLength = 1.0f; f.glassFilter = 0.0f; f.originalRMEx = 0.0f; f.originalTPOx = 0.0f;
      f.originalColor = V3(0.0f, 0.0f, 0.0f);
      f.renderId.x = f.renderId.y = f.renderId.z = f.renderId.w = 0.0f;
      f.renderOriginalId = f.renderId;
      f.ndc = V3(q[3], q[7], 1.0f);
      f.cnt.shades = 0;
      v3 finalColor = V3(0.0f, 0.0f, 0.0f);
      for (int i = 0; i < params->samples; i++) {
        float cosSampleN = flx_cos((float)i);
        finalColor = add3(finalColor, lightTrace(&f, hit, dir, origin, cosSampleN, params->max_reflections));
      }
      float invSamples = 1.0f / (float)params->samples;
      finalColor = scale3(finalColor, invSamples);
      finalColor = mul3(finalColor, f.originalColor);
      float row[5] = { finalColor.x, finalColor.y, finalColor.z, 1.0f, hit.suv.x };
      memcpy(o, row, sizeof row);
      o[5] = (uint32_t)hit.triangleId;
      o[6] = (uint32_t)hit.transformId;
      o[7] = (uint32_t)f.cnt.shades;
    }
  }
  return FLX_OK;
}
