/*
 * flx_rays_planes_gather_ref.c — CPU reference of flx_rays_planes_gather (include/flexlight_hip_debug.h, "ray images with a volume").  TEST INFRASTRUCTURE ONLY: built
 * by the test modules that need it (tests/rays_planes_gather_ref/flx_rays_planes_gather_ref.py) with the oracle's flags into a directory outside git; the product
 * never links it.
 *
 * It is flx_rays_planes_ref's loop (tests/rays_planes_ref/flx_rays_planes_ref.c) with one change: where that calls the oracle's lightTrace it calls lightTracePath of
 * tests/rays_gather_ref/flx_rays_gather_ref.c — which it gets by including that file, as that file includes the oracle — and then flx_gather_lookup,
 * flx_gather_ambient and flx_gather_path_value of include/flx_gather.h.  The globals carry from sample to sample on the one Frag as they do there.
 * (-Wl,-Bsymbolic keeps this library's copy of the oracle's and of the gathered batches' exported names to itself, beside their libraries in one process.)
 */
#include "../rays_gather_ref/flx_rays_gather_ref.c"

#define FLX_PLANES_GATHER_REF_LIT 1u          /* a last point and W > 0: A = E * gain */
#define FLX_PLANES_GATHER_REF_CONSTANT 2u     /* a last point, W not > 0: A = ambient */
#define FLX_PLANES_GATHER_REF_NO_POINT 3u     /* the sample shaded nothing: A = ambient */

/* mode 0: flx_rays_planes_gather's five planes.  mode 1 / 2: the SIX planes a temporal frame stores (tests/rays_temporal_ref/flx_rays_temporal_ref.c, use_filter 0 /
 * 1: the canvas mode multiplies by originalColor and sets the ip plane's w to 1; the sixth plane is renderLocationId), for tests/rays_temporal_ref's pass.
 * rays: n rows of 8 floats; planes: float[5 or 6][n][4] in flx_render_planes_device's order, before quantisation; hits: n bytes, 1 where the ray hits (may be NULL);
 * colour: n rows of 3 floats, c before fract — the samples' mean — (zeros for a miss; may be NULL); classes: n * samples bytes, the class of every sample (0 for a
 * miss; may be NULL).  -> 0, or FLX_ERR_INVALID */
int flx_rays_planes_gather_ref(const flx_scene_view *scene, const flx_frame_params *params, const flx_gather_ref_volume *volume, const float *rays, float *planes, uint8_t *hits,
                               float *colour, uint8_t *classes, uint32_t n, int mode, int threads) {
  if (!scene || !params || !volume || !volume->grid || !volume->sh || !scene->geometry || !scene->attributes || !scene->rotation || !scene->shift || (n && (!rays || !planes)))
    return FLX_ERR_INVALID;
  if (params->samples < 1 || params->max_reflections < 0 || params->texture_width < 1 || mode < 0 || mode > 2) return FLX_ERR_INVALID;
  const int P = mode ? 6 : 5;
  flx_trace_params tp;
  memset(&tp, 0, sizeof tp);
  tp.ambient[0] = params->ambient[0]; tp.ambient[1] = params->ambient[1]; tp.ambient[2] = params->ambient[2];
  const size_t S = (size_t)params->samples;
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
      for (int p = 0; p < P; p++) {
        row[p] = planes + ((size_t)p * n + k) * 4;
        memset(row[p], 0, 4 * sizeof(float));               /* not covered: every target stays at the clear colour */
      }
      if (colour) memset(colour + (size_t)k * 3, 0, 3 * sizeof(float));
      if (classes) memset(classes + (size_t)k * S, 0, S);
      const v3 origin = V3(q[0], q[1], q[2]), dir = V3(q[4], q[5], q[6]);
      Ray ray = { origin, dir };
      uint64_t visits = 0;
      Hit hit = rayTracerImpl(scene, ray, 0, 0.0f, &visits);
      if (hits) hits[k] = hit.triangleId != -1;
      if (hit.triangleId == -1) continue;
      /* fragment_main from its first line to the targets it writes (oracle/flx_oracle.c), the use_filter == 1 branch */
      f.firstRayLength = 1.0f; f.glassFilter = 0.0f; f.originalRMEx = 0.0f; f.originalTPOx = 0.0f;
      f.originalColor = V3(0.0f, 0.0f, 0.0f);
      f.renderId.x = f.renderId.y = f.renderId.z = f.renderId.w = 0.0f;
      f.renderOriginalId = f.renderId;
      f.ndc = V3(q[3], q[7], 1.0f);
      v3 finalColor = V3(0.0f, 0.0f, 0.0f);
      for (int i = 0; i < params->samples; i++) {
        float cosSampleN = flx_cos((float)i);
        const GatherPath p = lightTracePath(&f, hit, dir, origin, cosSampleN, params->max_reflections);
        const float position[4] = { p.x.x, p.x.y, p.x.z, 1.0f }, normal[4] = { p.n.x, p.n.y, p.n.z, 0.0f };
        float e[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, a[3], value[3];
        if (p.hasPoint) flx_gather_lookup(volume->grid, volume->map, volume->sh, volume->maps, volume->offsets, position, normal, e);
        const float fc[3] = { p.finalColor.x, p.finalColor.y, p.finalColor.z }, im[3] = { p.importancyFactor.x, p.importancyFactor.y, p.importancyFactor.z };
        flx_gather_ambient(&tp, volume->gain, p.hasPoint, e, a);
        flx_gather_path_value(fc, im, a, value);
        finalColor = add3(finalColor, V3(value[0], value[1], value[2]));
        if (classes)
          classes[(size_t)k * S + (size_t)i] = !p.hasPoint ? FLX_PLANES_GATHER_REF_NO_POINT : (e[3] > 0.0f ? FLX_PLANES_GATHER_REF_LIT : FLX_PLANES_GATHER_REF_CONSTANT);
      }
      float invSamples = 1.0f / (float)params->samples;
      finalColor = scale3(finalColor, invSamples);
      if (mode == 1) finalColor = mul3(finalColor, f.originalColor);
      if (colour) { colour[(size_t)k * 3] = finalColor.x; colour[(size_t)k * 3 + 1] = finalColor.y; colour[(size_t)k * 3 + 2] = finalColor.z; }
      row[0][0] = flx_fract(finalColor.x); row[0][1] = flx_fract(finalColor.y); row[0][2] = flx_fract(finalColor.z); row[0][3] = 1.0f;
      row[1][0] = flx_floor(finalColor.x) * INV_256; row[1][1] = flx_floor(finalColor.y) * INV_256; row[1][2] = flx_floor(finalColor.z) * INV_256;
      row[1][3] = mode == 1 ? 1.0f : f.glassFilter;
      row[2][0] = f.originalColor.x; row[2][1] = f.originalColor.y; row[2][2] = f.originalColor.z;
      row[2][3] = flx_min(f.originalRMEx, f.firstRayLength) + INV_255;
      row[3][0] = f.renderId.x; row[3][1] = f.renderId.y; row[3][2] = f.renderId.z; row[3][3] = f.renderId.w + INV_255;
      row[4][0] = 0.0f; row[4][1] = 0.0f; row[4][2] = 0.0f; row[4][3] = f.originalTPOx + INV_255;
      if (mode) {
        /* fragment:640-642; relativePosition is in object space, the origin in world space, as in the shader */
        const float *g = scene->geometry + (size_t)hit.triangleId * 12;
        float w0 = 1.0f - hit.suv.y - hit.suv.z;
        v3 rel = add3(add3(scale3(V3(g[0], g[1], g[2]), w0), scale3(V3(g[3], g[4], g[5]), hit.suv.y)), scale3(V3(g[6], g[7], g[8]), hit.suv.z));
        float div = 2.0f * distance3(rel, origin);
        row[5][0] = flx_mod(rel.x, div) / div; row[5][1] = flx_mod(rel.y, div) / div; row[5][2] = flx_mod(rel.z, div) / div; row[5][3] = INV_255;
      }
    }
  }
  return FLX_OK;
}
