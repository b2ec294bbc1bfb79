/*
 * flx_raster_ref.c — CPU reference of the rasterizer renderer.  TEST INFRASTRUCTURE ONLY: built by the test modules that need it
 * (tests/raster_ref/flx_raster_ref.py) with the oracle's flags and linked to oracle/libflx_oracle.so; the product never links it.
 *
 * Follows, function by function (paths relative to the reference checkout):
 *   modules/rasterizerWGL2.js:253-312   the draw: one instance per idBuffer entry, uniforms, the view matrix
 *   modules/rasterizerWGL2.js:395-401   draw state: depth test LESS, depthMask(true), no culling, blend (ONE, ONE_MINUS_SRC_ALPHA / ONE, ONE)
 *   shaders/rasterizer_vertex.glsl:35-69  the vertex stage, re-expressed as a ray cast per pixel (DESIGN.md §2 "Rasterizer")
 *   shaders/rasterizer_fragment.glsl:62-67, 202-291  lookup() and main()
 * The routines the rasterizer shares character for character with the path tracer — shadowTest with rayCuboid and
 * moellerTrumboreCull, forwardTrace with its GGX / Smith / Schlick helpers — and the transcendental pow are the oracle's own
 * (flx_oracle_shadow_test, flx_oracle_forward_trace, flx_oracle_ray_cuboid, flx_oracle_math), not restated here.
 *
 * Unlike k_raster (flx_raster.hip), which shades while it walks and keeps one pending fragment, this file first lists every
 * fragment of a pixel that passes the depth test, in draw order, then shades the ones from the last opaque fragment on and blends
 * them over the clear colour.  The two give the same bytes because a fragment whose clamped alpha is 1 makes the blend's result
 * independent of what was under it.
 */
#include "flx_oracle.h"
#include "flx_math.h"

#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define NEAR_VIEW_DEPTH 0.5f          /* rasterizer_vertex.glsl:63 + the clip volume; DESIGN.md §2 */

typedef struct { float x, y, z; } v3;
static v3 V3(float x, float y, float z) { v3 r = { x, y, z }; return r; }
static v3 add3(v3 a, v3 b) { return V3(a.x + b.x, a.y + b.y, a.z + b.z); }
static v3 sub3(v3 a, v3 b) { return V3(a.x - b.x, a.y - b.y, a.z - b.z); }
static v3 mul3(v3 a, v3 b) { return V3(a.x * b.x, a.y * b.y, a.z * b.z); }
static v3 scale3(v3 a, float s) { return V3(a.x * s, a.y * s, a.z * s); }
static float dot3(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
static v3 cross3(v3 a, v3 b) { return V3(a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y); }
static float length3(v3 a) { return flx_sqrt(dot3(a, a)); }
static v3 normalize3(v3 a) { float l = length3(a); return V3(a.x / l, a.y / l, a.z / l); }
static v3 mix3(v3 a, v3 b, float t) { return V3(flx_mix(a.x, b.x, t), flx_mix(a.y, b.y, t), flx_mix(a.z, b.z, t)); }
/* mat3 (std140: 3 x vec4 columns) * vec3 = (col0 v.x + col1 v.y) + col2 v.z */
static v3 rot_mul(const flx_scene_view *sc, int m, v3 v) {
  const float *r = sc->rotation + (size_t)m * 12;
  return V3((r[0] * v.x + r[4] * v.y) + r[8] * v.z, (r[1] * v.x + r[5] * v.y) + r[9] * v.z, (r[2] * v.x + r[6] * v.y) + r[10] * v.z);
}
static v3 shift_of(const flx_scene_view *sc, int m) { const float *s = sc->shift + (size_t)m * 4; return V3(s[0], s[1], s[2]); }

/* One fragment that passed the depth test: the ray cast's (s, u, v), 2 x its transform, its entry. */
typedef struct { v3 suv; int tI, tri; } Fragment;

/* Coverage (DESIGN.md §2 "Rasterizer", pin 1): what the rasteriser does for the pixel centre's ray — both facings (det != 0,
 * NaN excluded: rasterizerWGL2.js does not enable CULL_FACE), inclusive edges, in front of the near plane, strictly closer than
 * the nearest depth so far (GL LESS: on a tie the earlier instance keeps the pixel).  Returns s = 0 on a miss. */
static v3 raster_cover(v3 a, v3 b, v3 c, v3 o, v3 d, float l, float viewDepthPerS) {
  const v3 zero = { 0.0f, 0.0f, 0.0f };
  v3 edge1 = sub3(b, a), edge2 = sub3(c, a);
  v3 pvec = cross3(d, edge2);
  float det = dot3(edge1, pvec);
  if (!(det < 0.0f || det > 0.0f)) return zero;
  float inv_det = 1.0f / det;
  v3 tvec = sub3(o, a);
  float u = dot3(tvec, pvec) * inv_det;
  if (!(u >= 0.0f && u <= 1.0f)) return zero;
  v3 qvec = cross3(tvec, edge1);
  float v = dot3(d, qvec) * inv_det;
  if (!(v >= 0.0f && u + v <= 1.0f)) return zero;
  float s = dot3(edge2, qvec) * inv_det;
  if (!(s < l) || !(s * viewDepthPerS >= NEAR_VIEW_DEPTH)) return zero;
  return V3(s, u, v);
}

/* The draw for one pixel as the skip-list walk meets the triangles (the order of idBuffer, scene.js:230,267): every triangle
 * the ray meets closer than the nearest depth accepted so far is a fragment; boxes are pruned with that depth (the loop of
 * pathtracer_fragment.glsl:172-227, as for the path tracer's primary rays).  Returns the number of fragments (all of them are
 * counted; at most `cap` are stored).  `trail`, if given, takes the indices of the entries fetched, in order, the terminator included (at most
 * `tcap` of them; *visits counts them all). */
static int raster_walk(const flx_scene_view *sc, v3 origin, v3 dir, float viewDepthPerS, Fragment *frags, int cap, uint64_t *visits, int *trail, int tcap) {
  v3 tO = origin, tD = dir;
  int cachedTI = 0, n = 0;
  float minLen = FLX_POW32;
  int size = (int)sc->n_entries_padded;
  for (int i = 0; i < size; i++) {
    const float *e = sc->geometry + (size_t)i * 12;
    if (trail && *visits < (uint64_t)tcap) trail[*visits] = i;
    (*visits)++;
    int tI = (int)e[9] << 1;
    if (tI != cachedTI) {
      cachedTI = tI;
      tO = rot_mul(sc, tI + 1, add3(origin, shift_of(sc, tI + 1)));
      tD = rot_mul(sc, tI + 1, dir);
    }
    if (e[10] == 0.0f) break;
    if (e[10] == 1.0f) {
      float o3[3] = { tO.x, tO.y, tO.z }, d3[3] = { tD.x, tD.y, tD.z };
      if (!flx_oracle_ray_cuboid(minLen, o3, d3, e, e + 3)) i += (int)e[6];
    } else {
      v3 r = raster_cover(V3(e[0], e[1], e[2]), V3(e[3], e[4], e[5]), V3(e[6], e[7], e[8]), tO, tD, minLen, viewDepthPerS);
      if (r.x != 0.0f) {
        if (n < cap) { frags[n].suv = r; frags[n].tI = tI; frags[n].tri = i; }
        n++;
        minLen = r.x;
      }
    }
  }
  return n;
}

/* rasterizer_fragment.glsl:62-67 lookup(): NEAREST + REPEAT; an empty atlas samples (0,0,0) */
static v3 lookup(const flx_scene_view *sc, int which, float tw, float invTW, float bu, float bv, float texNum) {
  if (!sc->atlas[which]) return V3(0.0f, 0.0f, 0.0f);
  uint32_t W = sc->atlas_w[which], H = sc->atlas_h[which];
  float atlasHeightFactor = (float)W / (float)H * invTW;
  float cx = (bu + flx_mod(texNum, tw)) * invTW;
  float cy = (bv + flx_floor(texNum * invTW)) * atlasHeightFactor;
  float fx = flx_fract(cx) * (float)W, fy = flx_fract(cy) * (float)H;
  uint32_t ix = flx_f2uint(fx), iy = flx_f2uint(fy);
  if (ix >= W) ix = W - 1u;
  if (iy >= H) iy = H - 1u;
  const uint8_t *t = sc->atlas[which] + ((size_t)iy * W + ix) * 4;
  return V3((float)t[0] / 255.0f, (float)t[1] / 255.0f, (float)t[2] / 255.0f);
}
/* rasterizer_fragment.glsl:238-254: mix(attribute, lookup(...), max(sign(texNum + 0.5), 0)) */
static v3 material_field(const flx_scene_view *sc, int which, float tw, float invTW, float bu, float bv, float texNum, v3 attr, uint64_t *texels) {
  float weight = flx_max(flx_sign(texNum + 0.5f), 0.0f);
  if (weight == 1.0f && texels) (*texels)++;
  return mix3(attr, lookup(sc, which, tw, invTW, bu, bv, texNum), weight);
}

/* Pin 2: the fragment's interpolated inputs from the ray cast — uv = (1 - u - v, u) (rasterizer_vertex.glsl:33,66), the third
 * weight as the fragment shader recomputes it (:230,234), `position` over the object-space vertices (vertex:64). */
typedef struct { float w0, w1, w2, bu, bv; v3 position; const float *t; } FragInputs;
static void frag_inputs(const flx_scene_view *sc, v3 suv, int tri, FragInputs *in) {
  in->w0 = 1.0f - suv.y - suv.z;
  in->w1 = suv.y;
  in->w2 = 1.0f - in->w0 - in->w1;
  const float *g = sc->geometry + (size_t)tri * 12;
  in->position = add3(add3(scale3(V3(g[0], g[1], g[2]), in->w0), scale3(V3(g[3], g[4], g[5]), in->w1)), scale3(V3(g[6], g[7], g[8]), in->w2));
  const float *t = sc->attributes + (size_t)tri * 28;
  in->t = t;
  /* mat3x2(t2.yzw, t3.xyz) * vec3(uv, w2) (:232-234) */
  in->bu = (t[9] * in->w0 + t[11] * in->w1) + t[13] * in->w2;
  in->bv = (t[10] * in->w0 + t[12] * in->w1) + t[14] * in->w2;
}

/* material.tpo.x alone: whether the fragment is opaque */
static float fragment_tpo_x(const flx_scene_view *sc, const flx_frame_params *fp, const Fragment *f) {
  FragInputs in;
  frag_inputs(sc, f->suv, f->tri, &in);
  float tw = (float)fp->texture_width, invTW = 1.0f / tw;
  return material_field(sc, 2, tw, invTW, in.bu, in.bv, in.t[17], V3(in.t[24], in.t[25], in.t[26]), NULL).x;
}

/* rasterizer_fragment.glsl:202-291 main() -> renderColor */
static void fragment_main(const flx_scene_view *sc, const flx_frame_params *fp, const Fragment *f, float out[4], flx_counters *cnt) {
  FragInputs in;
  frag_inputs(sc, f->suv, f->tri, &in);
  const float *t = in.t;
  v3 position = in.position;
  int tI = f->tI;
  v3 absolutePosition = add3(rot_mul(sc, tI, position), shift_of(sc, tI));                       /* :228 */
  v3 nSum = add3(add3(scale3(V3(t[0], t[1], t[2]), in.w0), scale3(V3(t[3], t[4], t[5]), in.w1)), scale3(V3(t[6], t[7], t[8]), in.w2));
  v3 smoothNormal = normalize3(rot_mul(sc, tI, nSum));                                             /* :230 */
  float tw = (float)fp->texture_width, invTW = 1.0f / tw;                                          /* :204 */
  uint64_t *texels = cnt ? &cnt->atlas_texels : NULL;
  v3 albedo = material_field(sc, 0, tw, invTW, in.bu, in.bv, t[15], V3(t[18], t[19], t[20]), texels);
  v3 rme = material_field(sc, 1, tw, invTW, in.bu, in.bv, t[16], V3(t[21], t[22], t[23]), texels);
  v3 tpo = material_field(sc, 2, tw, invTW, in.bu, in.bv, t[17], V3(t[24], t[25], t[26]), texels);
  if (cnt) cnt->shades++;
  float material[9] = { albedo.x, albedo.y, albedo.z, rme.x, rme.y, rme.z, tpo.x, tpo.y, tpo.z };
  v3 finalColor = V3(rme.z + fp->ambient[0], rme.z + fp->ambient[1], rme.z + fp->ambient[2]);     /* :256 */
  v3 camera = V3(fp->camera[0], fp->camera[1], fp->camera[2]);
  for (uint32_t j = 0; j < sc->n_lights; j++) {                                                    /* :258-276 */
    const float *lt = sc->lights + (size_t)j * 6;
    float strength = lt[3];
    if (strength <= 0.0f) continue;
    v3 light = V3(lt[0], lt[1], lt[2]);
    v3 dir = sub3(light, absolutePosition);
    v3 lightDir = sub3(light, position);                                                            /* object-space position, as written */
    v3 V = normalize3(sub3(camera, position));
    float ld[3] = { lightDir.x, lightDir.y, lightDir.z }, n3[3] = { smoothNormal.x, smoothNormal.y, smoothNormal.z }, v3a[3] = { V.x, V.y, V.z };
    float lc[3];
    flx_oracle_forward_trace(material, ld, strength, n3, v3a, lc);
    v3 localColor = V3(lc[0], lc[1], lc[2]);
    int showColor = length3(localColor) == 0.0f;
    int shadowed = 0;
    if (!showColor) {
      v3 u = normalize3(dir);
      float o3[3] = { absolutePosition.x, absolutePosition.y, absolutePosition.z }, d3[3] = { u.x, u.y, u.z };
      uint64_t visits = 0;
      shadowed = flx_oracle_shadow_test(sc, o3, d3, length3(dir), &visits);
      if (cnt) { cnt->shadow_walks++; cnt->shadow_visits += visits; }
    }
    if (showColor || !shadowed) finalColor = add3(finalColor, localColor);
  }
  finalColor = mul3(finalColor, albedo);                                                           /* :278 */
  float translucencyFactor = flx_min(1.0f + flx_max(finalColor.x, flx_max(finalColor.y, finalColor.z)) - tpo.x, 1.0f);
  finalColor = mix3(mul3(albedo, albedo), finalColor, translucencyFactor);                        /* :280-281 */
  if (fp->hdr == 1) {                                                                              /* :283-289 */
    finalColor = V3(finalColor.x / (finalColor.x + 1.0f), finalColor.y / (finalColor.y + 1.0f), finalColor.z / (finalColor.z + 1.0f));
    float gamma = 0.8f;
    float e[3] = { 1.0f / gamma, 1.0f / gamma, 1.0f / gamma };
    float x[3] = { 4.0f * finalColor.x, 4.0f * finalColor.y, 4.0f * finalColor.z }, p[3];
    flx_oracle_math(6, x, e, p, 3);
    finalColor = V3(p[0] / 4.0f * 1.3f, p[1] / 4.0f * 1.3f, p[2] / 4.0f * 1.3f);
  }
  out[0] = finalColor.x; out[1] = finalColor.y; out[2] = finalColor.z;
  out[3] = 1.0f - (0.5f * tpo.x);                                                                  /* :291 */
}

/* Pin 3: the fixed-point target clamps (NaN -> 0, the project's RGBA8 store pin); Q = what an RGBA8 channel holds after a store */
static float clamp01(float x) { return !(x > 0.0f) ? 0.0f : (x >= 1.0f ? 1.0f : x); }
static float q8(float x) { return (float)flx_floor(clamp01(x) * 255.0f + 0.5f) / 255.0f; }
/* FUNC_ADD, blendFuncSeparate(ONE, ONE_MINUS_SRC_ALPHA, ONE, ONE) (rasterizerWGL2.js:396-397) into the RGBA8 buffer */
void flx_raster_ref_blend(const float src[4], float dst[4]) {
  float r = clamp01(src[0]), g = clamp01(src[1]), b = clamp01(src[2]), a = clamp01(src[3]);
  float k = 1.0f - a;
  float kr = k * dst[0], kg = k * dst[1], kb = k * dst[2];
  dst[0] = q8(r + kr); dst[1] = q8(g + kg); dst[2] = q8(b + kb);
  dst[3] = q8(a + dst[3]);
}

/* one fragment's main() on its own (the known-answer table): fragment (suv, 2 x transform, entry) -> renderColor; cnt may be NULL */
void flx_raster_ref_fragment(const flx_scene_view *sc, const flx_frame_params *fp, int tI, int tri, const float suv[3], float out[4], flx_counters *cnt) {
  Fragment f = { V3(suv[0], suv[1], suv[2]), tI, tri };
  fragment_main(sc, fp, &f, out, cnt);
}

/* the pixel's ray (pathtracer_vertex.glsl's inverse, as the oracle's primary rays: pixel centre NDC through the inverse view) */
static void pixel_ray(const flx_frame_params *fp, const float inv[9], uint32_t px, uint32_t py_gl, v3 *dir, float *viewDepthPerS) {
  float nx = ((float)px + 0.5f) / (float)fp->width * 2.0f - 1.0f;
  float ny = ((float)py_gl + 0.5f) / (float)fp->height * 2.0f - 1.0f;
  v3 d = V3((inv[0] * nx + inv[1] * ny) + inv[2], (inv[3] * nx + inv[4] * ny) + inv[5], (inv[6] * nx + inv[7] * ny) + inv[8]);
  d = normalize3(d);
  *dir = d;
  *viewDepthPerS = dot3(V3(fp->view_matrix[6], fp->view_matrix[7], fp->view_matrix[8]), d);
}

/* The fragments of pixel (px, py_gl) in draw order (tests): suv[3 n], tI[n], tri[n]; returns their number (at most cap stored). */
int flx_raster_ref_fragments(const flx_scene_view *sc, const flx_frame_params *fp, uint32_t px, uint32_t py_gl, float *suv, int *tI, int *tri, int cap) {
  float inv[9];
  flx_invert3x3(fp->view_matrix, inv);
  v3 d; float vd;
  pixel_ray(fp, inv, px, py_gl, &d, &vd);
  Fragment *fr = (Fragment *)malloc(sizeof(Fragment) * (size_t)(cap > 0 ? cap : 1));
  uint64_t visits = 0;
  int n = raster_walk(sc, V3(fp->camera[0], fp->camera[1], fp->camera[2]), d, vd, fr, cap, &visits, NULL, 0);
  for (int k = 0; k < n && k < cap; k++) {
    suv[3 * k] = fr[k].suv.x; suv[3 * k + 1] = fr[k].suv.y; suv[3 * k + 2] = fr[k].suv.z;
    tI[k] = fr[k].tI; tri[k] = fr[k].tri;
  }
  free(fr);
  return n;
}

/* The entries that the walk of pixel (px, py_gl) fetches, in order, the terminator included (tests: the trips of k_raster's wave are a function of
 * these lists, tests/raster_stacks_util.py wave_schedule); returns their number (at most cap stored). */
int flx_raster_ref_visits(const flx_scene_view *sc, const flx_frame_params *fp, uint32_t px, uint32_t py_gl, int *out, int cap) {
  float inv[9];
  flx_invert3x3(fp->view_matrix, inv);
  v3 d; float vd;
  pixel_ray(fp, inv, px, py_gl, &d, &vd);
  uint64_t visits = 0;
  raster_walk(sc, V3(fp->camera[0], fp->camera[1], fp->camera[2]), d, vd, NULL, 0, &visits, out, cap);
  return (int)visits;
}

/* One frame of the rasterizer: out_rgba flx_tile_row_count * width * 4 floats, rows packed as flx_render packs them. */
int flx_raster_ref_render(const flx_scene_view *sc, const flx_frame_params *fp, float *out_rgba, flx_counters *counters, int threads) {
  if (!sc || !fp || !out_rgba || !sc->geometry || !sc->attributes || !sc->rotation || !sc->shift) return FLX_ERR_INVALID;
  if (fp->width == 0 || fp->height == 0 || fp->texture_width < 1 || (sc->n_lights && !sc->lights)) return FLX_ERR_INVALID;
  uint32_t W = fp->width, H = fp->height;
  uint32_t *rows = (uint32_t *)malloc(sizeof(uint32_t) * H);
  if (!rows) return FLX_ERR_INVALID;
  uint32_t tr = fp->tile_rows, tc = fp->tile_count, ti = fp->tile_index, nrows = 0;
  if (tr == 0 || tc <= 1) { tr = H; tc = 1; ti = 0; }
  for (uint32_t y = 0; y < H; y++) if ((y / tr) % tc == ti) rows[nrows++] = y;
  float inv[9];
  flx_invert3x3(fp->view_matrix, inv);
  v3 camera = V3(fp->camera[0], fp->camera[1], fp->camera[2]);
  flx_counters total;
  memset(&total, 0, sizeof total);
#ifdef _OPENMP
  if (threads > 0) omp_set_num_threads(threads);
#else
  (void)threads;
#endif
#pragma omp parallel
  {
    flx_counters c;
    memset(&c, 0, sizeof c);
    int cap = 64;
    Fragment *frags = (Fragment *)malloc(sizeof(Fragment) * (size_t)cap);
#pragma omp for schedule(dynamic, 1)
    for (uint32_t k = 0; k < nrows; k++) {
      uint32_t py_gl = H - 1u - rows[k];
      for (uint32_t px = 0; px < W; px++) {
        v3 d; float vd;
        pixel_ray(fp, inv, px, py_gl, &d, &vd);
        uint64_t visits = 0;
        int n = raster_walk(sc, camera, d, vd, frags, cap, &visits, NULL, 0);
        if (n > cap) {                        /* more fragments than room: walk again with enough */
          cap = n;
          frags = (Fragment *)realloc(frags, sizeof(Fragment) * (size_t)cap);
          uint64_t again = 0;
          raster_walk(sc, camera, d, vd, frags, cap, &again, NULL, 0);
        }
        c.primary_visits += visits;
        float dst[4] = { 0.0f, 0.0f, 0.0f, 0.0f };                                                 /* clearColor(0,0,0,0) */
        if (n > 0) {
          c.primary_hits++;
          int first = 0;                      /* the last opaque fragment: nothing under it shows */
          for (int m = 0; m < n; m++) {
            float a = 1.0f - 0.5f * fragment_tpo_x(sc, fp, &frags[m]);
            if (clamp01(a) == 1.0f) first = m;
          }
          for (int m = first; m < n; m++) {
            float src[4];
            fragment_main(sc, fp, &frags[m], src, &c);
            flx_raster_ref_blend(src, dst);
          }
        }
        memcpy(out_rgba + ((size_t)k * W + px) * 4, dst, sizeof dst);
      }
    }
    free(frags);
#pragma omp critical
    {
      total.primary_visits += c.primary_visits; total.shadow_visits += c.shadow_visits; total.shadow_walks += c.shadow_walks;
      total.shades += c.shades; total.primary_hits += c.primary_hits; total.atlas_texels += c.atlas_texels;
    }
  }
  free(rows);
  if (counters) *counters = total;
  return FLX_OK;
}
