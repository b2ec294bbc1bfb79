/*
 * flx_rays_gather_ref.c — CPU reference of flx_rays_trace_gather (include/flexlight_hip_debug.h, "ray batches with a volume").  TEST INFRASTRUCTURE ONLY: built by
 * the test modules that need it (tests/rays_gather_ref/flx_rays_gather_ref.py) with the oracle's flags into a directory outside git; the product never links it.
 *
 * It includes the oracle's source, as tests/rays_trace_ref does, and include/flx_gather.h with the volume headers behind it.  The oracle's lightTrace keeps the
 * last iteration's point in locals nobody outside can reach, so this file carries A RESTATEMENT of lightTrace (oracle/flx_oracle.c), statement for statement, with
 * two differences: it remembers x (ray.origin) and n (the smooth normal facing the ray) of the last iteration it ran, and it returns finalColor, importancyFactor
 * and that point as a record instead of adding importancyFactor * ambient.  tests/test_rays_gather_cpu.py holds the restatement against the oracle's own lightTrace
 * bit for bit (a volume whose every probe is inactive makes every A the params' ambient).  The value and the sum are flx_gather.h's; rayTracerImpl, reservoirSample
 * and everything below them are the oracle's own, called.
 * (-Wl,-Bsymbolic keeps this library's copy of the oracle's exported names to itself, beside libflx_oracle.so in one process.)
 */
#include "../../oracle/flx_oracle.c"

#include "flx_gather.h"

typedef struct GatherPath { v3 finalColor, importancyFactor, x, n; int hasPoint; } GatherPath;

/* lightTrace (oracle/flx_oracle.c, fragment:464-599) up to its last statement */
static GatherPath lightTracePath(Frag *f, Hit hit, v3 dir0, v3 camera, float cosSampleN, int bounces) {
  const flx_scene_view *sc = f->sc;
  const flx_frame_params *fp = f->fp;
  GatherPath out;
  int dontFilter = 1;
  v3 finalColor = V3(0.0f, 0.0f, 0.0f);
  v3 importancyFactor = V3(1.0f, 1.0f, 1.0f);
  f->originalColor = V3(1.0f, 1.0f, 1.0f);
  Ray ray = { camera, dir0 };
  v3 lastHitPoint = camera;
  out.x = V3(0.0f, 0.0f, 0.0f); out.n = V3(0.0f, 0.0f, 0.0f); out.hasPoint = 0;
  for (int i = 0; i < bounces && length3(mul3(importancyFactor, f->originalColor)) >= fp->min_importancy * SQRT3; i++) {
    float fi = (float)i;
    f->cnt.shades++;
    m3 rTI = rotation_at(sc, hit.transformId);
    v3 sTI = shift_at(sc, hit.transformId);
    ray.origin = add3(scale3(ray.unitDirection, hit.suv.x), ray.origin);
    v3 uvw = V3(1.0f - hit.suv.y - hit.suv.z, hit.suv.y, hit.suv.z);
    const float *g = sc->geometry + (size_t)hit.triangleId * 12;
    v3 t0v = m3mul(rTI, V3(g[0], g[1], g[2]));
    v3 t1v = m3mul(rTI, V3(g[3], g[4], g[5]));
    v3 t2v = m3mul(rTI, V3(g[6], g[7], g[8]));
    v3 offsetRayTarget = sub3(ray.origin, sTI);
    v3 geometryNormal = normalize3(cross3(sub3(t0v, t1v), sub3(t0v, t2v)));
    v3 diffs = V3(distance3(offsetRayTarget, t0v), distance3(offsetRayTarget, t1v), distance3(offsetRayTarget, t2v));
    const float *t = sc->attributes + (size_t)hit.triangleId * 28;
    v3 n0 = m3mul(rTI, V3(t[0], t[1], t[2]));
    v3 n1 = m3mul(rTI, V3(t[3], t[4], t[5]));
    v3 n2 = m3mul(rTI, V3(t[6], t[7], t[8]));
    v3 smoothNormal = normalize3(V3((n0.x * uvw.x + n1.x * uvw.y) + n2.x * uvw.z,
                                    (n0.y * uvw.x + n1.y * uvw.y) + n2.y * uvw.z,
                                    (n0.z * uvw.x + n1.z * uvw.y) + n2.z * uvw.z));
    v3 angles = V3(flx_acos(flx_abs(dot3(geometryNormal, n0))), flx_acos(flx_abs(dot3(geometryNormal, n1))),
                   flx_acos(flx_abs(dot3(geometryNormal, n2))));
    v3 angleTan = V3(flx_clamp(flx_tan(angles.x), 0.0f, 1.0f), flx_clamp(flx_tan(angles.y), 0.0f, 1.0f),
                     flx_clamp(flx_tan(angles.z), 0.0f, 1.0f));
    float geometryOffset = dot3(mul3(diffs, angleTan), uvw);
    float bu = (t[9] * uvw.x + t[11] * uvw.y) + t[13] * uvw.z;
    float bv = (t[10] * uvw.x + t[12] * uvw.y) + t[14] * uvw.z;
    Material material;
    material.albedo = fetchTexVal(f, 0, bu, bv, t[15], V3(t[18], t[19], t[20]));
    material.rme = fetchTexVal(f, 1, bu, bv, t[16], V3(t[21], t[22], t[23]));
    material.tpo = fetchTexVal(f, 2, bu, bv, t[17], V3(t[24], t[25], t[26]));

    ray.unitDirection = normalize3(sub3(ray.origin, lastHitPoint));
    float signDir = flx_sign(dot3(ray.unitDirection, smoothNormal));
    smoothNormal = scale3(smoothNormal, -signDir);
    /* THE LAST POINT so far: the first difference to lightTrace */
    out.x = ray.origin; out.n = smoothNormal; out.hasPoint = 1;

    v4 randomVec = noise(fp->random_seed, f->ndc.x, f->ndc.y, fi + cosSampleN);
    v3 randomSpheareVec = normalize3(add3(smoothNormal, normalize3(V3(randomVec.x, randomVec.y, randomVec.z))));
    float BRDF = flx_mix(1.0f, flx_abs(dot3(smoothNormal, ray.unitDirection)), material.rme.y);
    float roughnessBRDF = material.rme.x * BRDF;
    v3 roughNormal = normalize3(mix3(smoothNormal, randomSpheareVec, roughnessBRDF));
    v3 H = normalize3(sub3(roughNormal, ray.unitDirection));
    float VdotH = flx_max(dot3(neg3(ray.unitDirection), H), 0.0f);
    v3 F0 = scale3(material.albedo, BRDF);
    v3 fr = fresnel(F0, VdotH);
    float fresnelReflect = flx_max(fr.x, flx_max(fr.y, fr.z));
    int isSolid = material.tpo.x * fresnelReflect <= flx_abs(randomVec.w);

    if (dontFilter) {
      f->originalTPOx = material.tpo.x;
      f->originalColor = mul3(f->originalColor, material.albedo);
      f->originalRMEx += material.rme.x;
      float scale = flx_exp2_neg_int(i);
      v3 cn = combineNormalRME(smoothNormal, material.rme);
      v4 renderIdUpdate = { scale * cn.x, scale * cn.y, scale * cn.z, scale * 0.0f };
      f->renderId.x += renderIdUpdate.x; f->renderId.y += renderIdUpdate.y;
      f->renderId.z += renderIdUpdate.z; f->renderId.w += renderIdUpdate.w;
      if (i == 0) {
        f->renderOriginalId.x += renderIdUpdate.x; f->renderOriginalId.y += renderIdUpdate.y;
        f->renderOriginalId.z += renderIdUpdate.z; f->renderOriginalId.w += renderIdUpdate.w;
      }
      dontFilter = (material.rme.x < 0.01f && isSolid) || !isSolid;
      if (isSolid && material.tpo.x > 0.01f) {
        f->glassFilter += 1.0f;
        dontFilter = 0;
      }
    } else {
      importancyFactor = mul3(importancyFactor, material.albedo);
    }

    if (i == 1) f->firstRayLength = flx_min(length3(sub3(ray.origin, lastHitPoint)) / length3(sub3(lastHitPoint, camera)), f->firstRayLength);
    v3 localColor = reservoirSample(f, material, ray, randomVec, scale3(roughNormal, -signDir), scale3(smoothNormal, -signDir),
                                    geometryOffset, dontFilter, i);
    finalColor = add3(finalColor, mul3(localColor, importancyFactor));
    if (isSolid) {
      ray.unitDirection = normalize3(mix3(reflect3(ray.unitDirection, smoothNormal), randomSpheareVec, roughnessBRDF));
    } else {
      float eta = flx_mix(1.0f / material.tpo.z, material.tpo.z, flx_max(signDir, 0.0f));
      ray.unitDirection = normalize3(mix3(refract3(ray.unitDirection, smoothNormal, eta), randomSpheareVec, roughnessBRDF));
    }
    /* (the walk nobody reads is not made: lightTrace's own rule, without its as-written mode) */
    if (!(i + 1 < bounces && length3(mul3(importancyFactor, f->originalColor)) >= fp->min_importancy * SQRT3)) break;
    f->cnt.closest_walks++;
    hit = rayTracerImpl(sc, ray, 0, 0.0f, &f->cnt.closest_visits);
    if (hit.triangleId == -1) break;
    lastHitPoint = ray.origin;
  }
  /* the second difference: no `finalColor + importancyFactor * ambient` here */
  out.finalColor = finalColor; out.importancyFactor = importancyFactor;
  return out;
}

/* A volume in host memory: flx_gather_volume's fields with float rows (maps, offsets: NULL for none). */
typedef struct flx_gather_ref_volume {
  const flx_volume_grid *grid; const float *sh; const flx_volume_map *map; const float *maps; const float *offsets; float gain;
} flx_gather_ref_volume;

/* rays: n rows of 8 floats; out: n rows of 8 words (flx_rays_trace_ref's), or NULL; records: n * samples rows of 16 floats — finalColor, importancyFactor,
 * x (word 3: 1.0f with a last point, else 0.0f), n (word 3: 0.0f), row ray * samples + sample; all zeros for a ray that misses —, or NULL; lookups: as many rows of 4
 * floats, the E of each path (zeros without a last point), or NULL.  -> 0, or FLX_ERR_INVALID */
int flx_rays_gather_ref(const flx_scene_view *scene, const flx_frame_params *params, const flx_gather_ref_volume *volume, const float *rays, uint32_t *out, float *records,
                        float *lookups, uint32_t n, int threads) {
  if (!scene || !params || !volume || !volume->grid || !volume->sh || !scene->geometry || !scene->attributes || !scene->rotation || !scene->shift || (n && !rays)) return FLX_ERR_INVALID;
  if (params->samples < 1 || params->max_reflections < 0 || params->texture_width < 1) return FLX_ERR_INVALID;
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
      const v3 origin = V3(q[0], q[1], q[2]), dir = V3(q[4], q[5], q[6]);
      Ray ray = { origin, dir };
      uint64_t visits = 0;
      Hit hit = rayTracerImpl(scene, ray, 0, 0.0f, &visits);
      if (out) { memset(out + (size_t)k * 8, 0, 8 * sizeof(uint32_t)); out[(size_t)k * 8 + 5] = 0xffffffffu; }
      if (records) memset(records + (size_t)k * S * 16, 0, S * 16 * sizeof(float));
      if (lookups) memset(lookups + (size_t)k * S * 4, 0, S * 4 * sizeof(float));
      if (hit.triangleId == -1) continue;
      f.firstRayLength = 1.0f; f.glassFilter = 0.0f; f.originalRMEx = 0.0f; f.originalTPOx = 0.0f;
      f.originalColor = V3(0.0f, 0.0f, 0.0f);
      f.renderId.x = f.renderId.y = f.renderId.z = f.renderId.w = 0.0f;
      f.renderOriginalId = f.renderId;
      f.ndc = V3(q[3], q[7], 1.0f);
      f.cnt.shades = 0;
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
        if (records) {
          float *r = records + ((size_t)k * S + (size_t)i) * 16;
          r[0] = fc[0]; r[1] = fc[1]; r[2] = fc[2]; r[3] = 0.0f;
          r[4] = im[0]; r[5] = im[1]; r[6] = im[2]; r[7] = 0.0f;
          r[8] = p.x.x; r[9] = p.x.y; r[10] = p.x.z; r[11] = p.hasPoint ? 1.0f : 0.0f;
          r[12] = p.n.x; r[13] = p.n.y; r[14] = p.n.z; r[15] = 0.0f;
        }
        if (lookups) memcpy(lookups + ((size_t)k * S + (size_t)i) * 4, e, sizeof e);
      }
      if (!out) continue;
      float invSamples = 1.0f / (float)params->samples;
      finalColor = scale3(finalColor, invSamples);
      finalColor = mul3(finalColor, f.originalColor);
      uint32_t *o = out + (size_t)k * 8;
      float row[5] = { finalColor.x, finalColor.y, finalColor.z, 1.0f, hit.suv.x };
      memcpy(o, row, sizeof row);
      o[5] = (uint32_t)hit.triangleId;
      o[6] = (uint32_t)hit.transformId;
      o[7] = (uint32_t)f.cnt.shades;
    }
  }
  return FLX_OK;
}
