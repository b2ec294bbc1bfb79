/*
 * flx_surface_ref.c — CPU reference of flx_rays_surface and flx_frame_surface (include/flexlight_hip_debug.h, "surface rows").  TEST INFRASTRUCTURE ONLY: built by
 * the test modules that need it (tests/surface_ref/flx_surface_ref.py) with the oracle's flags into a directory outside git; the product never links it.
 *
 * It includes the oracle's source.  The first hit is the oracle's own: rayTracerImpl (mode 0) for a ray, primary_setup and primary_hit for a pixel.  The rows are
 * the statements of lightTrace's first iteration (oracle/flx_oracle.c, "fragment:464-599") that form them, executed with the oracle's own helpers — rotation_at,
 * m3mul, normalize3, fetchTexVal, flx_sign — in lightTrace's order; tests/test_surface_ref_cpu.py holds the result against the oracle's own frames.
 * (-Wl,-Bsymbolic keeps this library's copy of the oracle's exported names to itself, beside libflx_oracle.so in one process.)
 */
#include "../../oracle/flx_oracle.c"

#define SURFACE_PLANES 8

static void put4(float *plane, size_t k, float x, float y, float z, float w) {
  float *o = plane + k * 4;
  o[0] = x; o[1] = y; o[2] = z; o[3] = w;
}

/* rows of item k in the eight planes (each n rows of 4 words, plane p at out + p * n * 4): a hit of the ray (origin, dir); lastHitPoint = origin */
static void surface_rows(Frag *f, Hit hit, v3 origin, v3 dir, float *out, size_t n, size_t k) {
  const flx_scene_view *sc = f->sc;
  float *plane[SURFACE_PLANES];
  for (int p = 0; p < SURFACE_PLANES; p++) plane[p] = out + (size_t)p * n * 4;
  const int32_t none = -1;
  if (hit.triangleId == -1) {
    for (int p = 0; p < SURFACE_PLANES; p++) put4(plane[p], k, 0.0f, 0.0f, 0.0f, 0.0f);
    memcpy(plane[0] + k * 4 + 3, &none, 4);
    return;
  }
  Ray ray = { origin, dir };
  v3 lastHitPoint = origin;
  /* lightTrace, i = 0 */
  m3 rTI = rotation_at(sc, hit.transformId);
  ray.origin = add3(scale3(ray.unitDirection, hit.suv.x), ray.origin);
  v3 uvw = V3(1.0f - hit.suv.y - hit.suv.z, hit.suv.y, hit.suv.z);
  const float *g = sc->geometry + (size_t)hit.triangleId * 12;
  v3 t0v = m3mul(rTI, V3(g[0], g[1], g[2]));
  v3 t1v = m3mul(rTI, V3(g[3], g[4], g[5]));
  v3 t2v = m3mul(rTI, V3(g[6], g[7], g[8]));
  v3 geometryNormal = normalize3(cross3(sub3(t0v, t1v), sub3(t0v, t2v)));
  const float *t = sc->attributes + (size_t)hit.triangleId * 28;
  v3 n0 = m3mul(rTI, V3(t[0], t[1], t[2]));
  v3 n1 = m3mul(rTI, V3(t[3], t[4], t[5]));
  v3 n2 = m3mul(rTI, V3(t[6], t[7], t[8]));
  v3 smoothNormal = normalize3(V3((n0.x * uvw.x + n1.x * uvw.y) + n2.x * uvw.z,
                                  (n0.y * uvw.x + n1.y * uvw.y) + n2.y * uvw.z,
                                  (n0.z * uvw.x + n1.z * uvw.y) + n2.z * uvw.z));
  float bu = (t[9] * uvw.x + t[11] * uvw.y) + t[13] * uvw.z;
  float bv = (t[10] * uvw.x + t[12] * uvw.y) + t[14] * uvw.z;
  Material material;
  material.albedo = fetchTexVal(f, 0, bu, bv, t[15], V3(t[18], t[19], t[20]));
  material.rme = fetchTexVal(f, 1, bu, bv, t[16], V3(t[21], t[22], t[23]));
  material.tpo = fetchTexVal(f, 2, bu, bv, t[17], V3(t[24], t[25], t[26]));
  ray.unitDirection = normalize3(sub3(ray.origin, lastHitPoint));
  float signDir = flx_sign(dot3(ray.unitDirection, smoothNormal));
  smoothNormal = scale3(smoothNormal, -signDir);

  const int32_t entry = hit.triangleId, transform2 = hit.transformId;
  put4(plane[0], k, hit.suv.x, hit.suv.y, hit.suv.z, 0.0f);
  memcpy(plane[0] + k * 4 + 3, &entry, 4);
  put4(plane[1], k, ray.origin.x, ray.origin.y, ray.origin.z, 1.0f);
  put4(plane[2], k, geometryNormal.x, geometryNormal.y, geometryNormal.z, 0.0f);
  put4(plane[3], k, smoothNormal.x, smoothNormal.y, smoothNormal.z, signDir);
  put4(plane[4], k, bu, bv, 0.0f, 0.0f);
  memcpy(plane[4] + k * 4 + 2, &transform2, 4);
  put4(plane[5], k, material.albedo.x, material.albedo.y, material.albedo.z, 0.0f);
  put4(plane[6], k, material.rme.x, material.rme.y, material.rme.z, 0.0f);
  put4(plane[7], k, material.tpo.x, material.tpo.y, material.tpo.z, 0.0f);
}

static int scene_ok(const flx_scene_view *scene) {
  return scene && scene->geometry && scene->attributes && scene->rotation && scene->shift;
}

/* rays: n rows of 8 floats (origin, -, direction, -); out: 8 planes of n rows of 4 words; texture_width as in the frame params -> 0, or FLX_ERR_INVALID */
int flx_surface_ref_rays(const flx_scene_view *scene, int32_t texture_width, const float *rays, float *out, uint32_t n) {
  if (!scene_ok(scene) || texture_width < 1 || (n && (!rays || !out))) return FLX_ERR_INVALID;
  flx_frame_params fp;
  memset(&fp, 0, sizeof fp);
  fp.texture_width = texture_width;
  Frag f;
  memset(&f, 0, sizeof f);
  f.sc = scene; f.fp = &fp;
  for (uint32_t k = 0; k < n; k++) {
    const float *q = rays + (size_t)k * 8;
    const v3 origin = V3(q[0], q[1], q[2]), dir = V3(q[4], q[5], q[6]);
    Ray ray = { origin, dir };
    uint64_t visits = 0;
    Hit hit = rayTracerImpl(scene, ray, 0, 0.0f, &visits);
    surface_rows(&f, hit, origin, dir, out, n, k);
  }
  return FLX_OK;
}

/* the frame of `params` (width, height, camera, view_matrix, texture_width): out: 8 planes of width * height rows, row k = pixel k with row 0 on top */
int flx_surface_ref_frame(const flx_scene_view *scene, const flx_frame_params *params, float *out) {
  if (!scene_ok(scene) || !params || !out || params->width == 0 || params->height == 0 || params->texture_width < 1) return FLX_ERR_INVALID;
  Frag f;
  memset(&f, 0, sizeof f);
  f.sc = scene; f.fp = params;
  PrimarySetup ps;
  primary_setup(params, &ps);
  const size_t n = (size_t)params->width * params->height;
  const v3 camera = V3(params->camera[0], params->camera[1], params->camera[2]);
  for (uint32_t row = 0; row < params->height; row++)
    for (uint32_t px = 0; px < params->width; px++) {
      v3 dir;
      Hit hit = primary_hit(&f, &ps, px, params->height - 1u - row, &dir);
      surface_rows(&f, hit, camera, dir, out, n, (size_t)row * params->width + px);
    }
  return FLX_OK;
}
