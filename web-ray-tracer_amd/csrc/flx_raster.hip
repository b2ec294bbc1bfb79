/*
 * flx_raster.hip — the rasterizer renderer (modules/rasterizerWGL2.js with shaders/rasterizer_vertex.glsl and
 * shaders/rasterizer_fragment.glsl) for gfx950: one kernel, k_raster, one lane per pixel, an 8 x 8 screen tile per wave.
 *
 * The reference draws one instance per idBuffer entry (rasterizerWGL2.js:312) with the depth test LESS, depthMask(true), no
 * culling and blendFuncSeparate(ONE, ONE_MINUS_SRC_ALPHA, ONE, ONE) into an RGBA8 drawing buffer cleared to (0,0,0,0)
 * (rasterizerWGL2.js:395-401).  idBuffer lists the triangles in ascending entry index (scene.js:230,267), which is the order in
 * which the skip-list walk meets them, so the depth test is reproduced during ONE walk of the pixel's ray (DESIGN.md §2
 * "Rasterizer"): every triangle the ray meets closer than the nearest depth accepted so far is a fragment that passes the test,
 * and boxes are pruned with that depth, as for the path tracer's primary rays.
 *
 * A lane keeps O(1) state: the nearest depth, the blended colour so far and one PENDING fragment.  An opaque fragment (clamped
 * alpha 1: the blend's result no longer depends on what is under it) drops the pending fragment and the colour; a translucent
 * one has the pending fragment shaded and blended first.  Only the fragments from the last opaque one on are shaded, and the
 * shading — every light with a shadow walk each — happens at ONE place in the walk loop, so its code is there once.  A
 * translucent fragment may still be covered by an opaque one later in the walk; its shading is then wasted, and the work
 * counters leave it out: they count what the fragments from the last opaque one on cost (pin 4).
 */
#include "flx_kernels.h"
#include "flx_kernel_util.h"

namespace flx {

/* The rasterizer's coverage test: the primary-visibility rule of moellerTrumborePrimaryE with both facings —
 * det != 0 (NaN excluded), inclusive edges, near plane at view depth 0.5, strictly closer than the nearest depth so far. */
FLX_DEV bool moellerTrumboreRasterE(f3 a, f3 edge1, f3 edge2, const Ray &ray, float l, float viewDepthPerS, f3 &suv) {
  f3 pvec = cross(ray.dir, edge2);
  float det = dot(edge1, pvec);
  if (!(det < 0.0f || det > 0.0f)) return false;
  float inv_det = recipOf(det, true);
  f3 tvec = ray.origin - a;
  float u = dot(tvec, pvec) * inv_det;
  if (!(u >= 0.0f && u <= 1.0f)) return false;
  f3 qvec = cross(tvec, edge1);
  float v = dot(ray.dir, qvec) * inv_det;
  if (!(v >= 0.0f && u + v <= 1.0f)) return false;
  float s = dot(edge2, qvec) * inv_det;
  if (!(s < l) || !(s * viewDepthPerS >= NEAR_VIEW_DEPTH)) return false;
  suv = F3(s, u, v);
  return s != 0.0f;
}

/* The interpolated vertex weights of a fragment (rasterizer_vertex.glsl:33,66): uv = (1 - u - v, u) from the ray cast, and the
 * third weight as the fragment shader recomputes it, 1.0 - uv.x - uv.y (rasterizer_fragment.glsl:230,234). */
struct RasterWeights { float w0, w1, w2; };
FLX_DEV RasterWeights rasterWeights(f3 suv) {
  RasterWeights w;
  w.w0 = 1.0f - suv.y - suv.z;
  w.w1 = suv.y;
  w.w2 = 1.0f - w.w0 - w.w1;
  return w;
}

/* rasterizer_fragment.glsl:62-67: lookup() — NEAREST + REPEAT on an RGBA8 atlas; an empty atlas samples (0,0,0) */
FLX_DEV f3 rasterLookup(const DeviceScene &sc, int which, float tw, float invTW, float bu, float bv, float texNum) {
  const uchar4 *atlas = sc.atlas[which];
  if (!atlas) return F3(0.0f, 0.0f, 0.0f);
  const uint32_t W = sc.atlas_w[which], H = sc.atlas_h[which];
  const float atlasHeightFactor = (float)W / (float)H * invTW;
  const float cx = (bu + flx_mod(texNum, tw)) * invTW;
  const float cy = (bv + flx_floor(texNum * invTW)) * atlasHeightFactor;
  const float fx = flx_fract(cx) * (float)W, fy = flx_fract(cy) * (float)H;
  uint32_t ix = flx_f2uint(fx), iy = flx_f2uint(fy);
  if (ix >= W) ix = W - 1u;
  if (iy >= H) iy = H - 1u;
  const uchar4 t = atlas[(size_t)iy * W + ix];
  return F3((float)t.x / 255.0f, (float)t.y / 255.0f, (float)t.z / 255.0f);
}
/* rasterizer_fragment.glsl:238-254: mix(attribute, lookup(...), max(sign(texNum + 0.5), 0)) — the lookup always samples, the weight
 * removes it afterwards; `texel` = the weight was 1 (counted as an atlas texel) */
FLX_DEV f3 rasterMaterialField(const DeviceScene &sc, int which, float tw, float invTW, float bu, float bv, float texNum, f3 attr, bool &texel) {
  const float weight = flx_max(flx_sign(texNum + 0.5f), 0.0f);
  texel = weight == 1.0f;
  return mix(attr, rasterLookup(sc, which, tw, invTW, bu, bv, texNum), weight);
}
/* barycentric texture coordinates of a fragment (rasterizer_fragment.glsl:232-234) */
FLX_DEV void rasterTexCoords(const float4 t2, const float4 t3, const RasterWeights &w, float &bu, float &bv) {
  bu = (t2.y * w.w0 + t2.w * w.w1) + t3.y * w.w2;
  bv = (t2.z * w.w0 + t3.x * w.w1) + t3.z * w.w2;
}
/* the clamp of a fixed-point colour target: NaN -> 0 (the project's RGBA8 store pin, quant_unorm8) */
FLX_DEV float rasterClamp01(float x) { return !(x > 0.0f) ? 0.0f : (x >= 1.0f ? 1.0f : x); }
/* Q(x): the value an RGBA8 channel holds after a store, as float32 */
FLX_DEV float rasterQ(float x) { return (float)quant_unorm8(x) / 255.0f; }
/* FUNC_ADD with blendFuncSeparate(ONE, ONE_MINUS_SRC_ALPHA, ONE, ONE) into the RGBA8 buffer (rasterizerWGL2.js:396-397) */
FLX_DEV void rasterBlend(float4 src, float4 &dst) {
  const float sr = rasterClamp01(src.x), sg = rasterClamp01(src.y), sb = rasterClamp01(src.z), sa = rasterClamp01(src.w);
  const float k = 1.0f - sa;
  dst.x = rasterQ(sr + k * dst.x);
  dst.y = rasterQ(sg + k * dst.y);
  dst.z = rasterQ(sb + k * dst.z);
  dst.w = rasterQ(sa + dst.w);
}
/* the alpha a fragment writes (rasterizer_fragment.glsl:291) after the target's clamp is 1: the fragment hides what is under it */
FLX_DEV bool rasterOpaque(float tpoX) { return rasterClamp01(1.0f - 0.5f * tpoX) == 1.0f; }

/* material.tpo.x of a fragment alone (what decides whether it is opaque): the same arithmetic as in rasterShade */
FLX_DEV float rasterTpoX(const DeviceScene &sc, const DeviceFrame &fr, f3 suv, int tri) {
  const RasterWeights w = rasterWeights(suv);
  const float4 *t = sc.attributes + 7 * (size_t)tri;
  const float4 t2 = t[2], t3 = t[3], t4 = t[4], t6 = t[6];
  float bu, bv;
  rasterTexCoords(t2, t3, w, bu, bv);
  const float tw = fr.texture_width, invTW = 1.0f / tw;
  bool texel;
  return rasterMaterialField(sc, 2, tw, invTW, bu, bv, t4.y, F3(t6.x, t6.y, t6.z), texel).x;
}

/* rasterizer_fragment.glsl:202-291, main() for one fragment: (suv, 2 x transform, entry) from the coverage test -> renderColor */
template <bool COUNT>
FLX_DEV float4 rasterShade(const DeviceScene &sc, const DeviceFrame &fr, int hdr, f3 camera, f3 ambient, f3 suv, int tI, int tri, WorkCounters &cnt) {
  const RasterWeights w = rasterWeights(suv);
  const float4 g0 = sc.geometry[3 * (size_t)tri], g1 = sc.geometry[3 * (size_t)tri + 1], g2 = sc.geometry[3 * (size_t)tri + 2];
  /* `position`: the object-space point, interpolated from the vertices (rasterizer_vertex.glsl:64) */
  const f3 position = (F3(g0.x, g0.y, g0.z) * w.w0 + F3(g0.w, g1.x, g1.y) * w.w1) + F3(g1.z, g1.w, g2.x) * w.w2;
  const float4 *t = sc.attributes + 7 * (size_t)tri;
  const float4 t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3], t4 = t[4], t5 = t[5], t6 = t[6];
  const M3 rot = rotation_at(sc, tI);
  const f3 absolutePosition = mul(rot, position) + shift_at(sc, tI);                                         /* :228 */
  /* :230 normals * vec3(uv, 1 - uv.x - uv.y), then rotated once */
  const f3 nSum = (F3(t0.x, t0.y, t0.z) * w.w0 + F3(t0.w, t1.x, t1.y) * w.w1) + F3(t1.z, t1.w, t2.x) * w.w2;
  const f3 smoothNormal = normalize(mul(rot, nSum));
  float bu, bv;
  rasterTexCoords(t2, t3, w, bu, bv);                                                                       /* :232-234 */
  const float tw = fr.texture_width, invTW = 1.0f / tw;                                                    /* :204 */
  Material material;
  bool x0, x1, x2;
  material.albedo = rasterMaterialField(sc, 0, tw, invTW, bu, bv, t3.w, F3(t4.z, t4.w, t5.x), x0);       /* :238-254 */
  material.rme = rasterMaterialField(sc, 1, tw, invTW, bu, bv, t4.x, F3(t5.y, t5.z, t5.w), x1);
  material.tpo = rasterMaterialField(sc, 2, tw, invTW, bu, bv, t4.y, F3(t6.x, t6.y, t6.z), x2);
  if (COUNT) { cnt.shades++; cnt.atlas_texels += (uint32_t)x0 + (uint32_t)x1 + (uint32_t)x2; }
  f3 finalColor = F3(material.rme.z + ambient.x, material.rme.z + ambient.y, material.rme.z + ambient.z);    /* :256 */
  const f3 V = normalize(camera - position);                                                                 /* :269, object-space position as written */
  for (uint32_t j = 0; j < sc.n_lights; j++) {                                                               /* :258-276 */
    const float *lt = sc.lights + (size_t)j * 6;
    const float strength = lt[3];
    if (strength <= 0.0f) continue;
    const f3 light = F3(lt[0], lt[1], lt[2]);
    const f3 dir = light - absolutePosition;
    const f3 localColor = forwardTrace(material, light - position, strength, smoothNormal, V);
    const bool showColor = length(localColor) == 0.0f;
    bool shadowed = false;
    if (!showColor) {
      Ray lightRay; lightRay.origin = absolutePosition; lightRay.dir = normalize(dir);
      Hit unused;
      walkBounce<COUNT, false>(sc, true, false, lightRay, length(dir), lightRay, shadowed, unused, cnt);
    }
    if (showColor || !shadowed) finalColor = finalColor + localColor;
  }
  finalColor = finalColor * material.albedo;                                                                 /* :278 */
  const float translucencyFactor = flx_min(1.0f + flx_max(finalColor.x, flx_max(finalColor.y, finalColor.z)) - material.tpo.x, 1.0f);
  finalColor = mix(material.albedo * material.albedo, finalColor, translucencyFactor);                      /* :280-281 */
  if (hdr == 1) {                                                                                            /* :283-289 */
    finalColor = finalColor / (finalColor + F3(1.0f, 1.0f, 1.0f));
    const float gamma = 0.8f;
    const float e = 1.0f / gamma;
    finalColor = F3(flx_pow(4.0f * finalColor.x, e) / 4.0f * 1.3f, flx_pow(4.0f * finalColor.y, e) / 4.0f * 1.3f,
                    flx_pow(4.0f * finalColor.z, e) / 4.0f * 1.3f);
  }
  return make_float4(finalColor.x, finalColor.y, finalColor.z, 1.0f - (0.5f * material.tpo.x));            /* :291 */
}

/* One lane per pixel; the wave walks its tile's rays over the forward-ordered copy together (as primaryWalkF does) until two
 * trips in a row serve fewer than FLX_PRIMARY_LOCK_MIN rays, then every lane goes on alone over the same array.  Per ray the
 * entries, their order, the arithmetic and the visit count are those of the reference-order walk (tests/raster_ref). */
/* (256, 4): the register allocation must allow four waves per SIMD — 128 VGPRs, no spill without counters, one VGPR with them; bounded at three
 * waves the compiler takes 131 / 139 VGPRs and the frames measured 1 - 14 % slower (profiles/raster_1080p.txt) */
/* The pixel's store: OUT = float4, the drawing buffer's values k / 255 as float32 (flx_raster_render); OUT = uint32_t, the RGBA8 word
 * k_quantize would store for that float4 (the frame loop's canvas bytes and the texture an anti-aliasing pass reads).  Q(k / 255) = k for
 * every k in 0 .. 255 (tests/test_frame_flags_cpu.py), so the word holds the blend's k themselves. */
FLX_DEV void rasterStore(float4 *out, size_t i, float4 c) { out[i] = c; }
FLX_DEV void rasterStore(uint32_t *out, size_t i, float4 c) { out[i] = pack_rgba8(c.x, c.y, c.z, c.w); }
template <bool COUNT, typename OUT>
__global__ __launch_bounds__(256, 4) void k_raster(DeviceScene sc, DeviceFrame fr, int hdr, OUT *__restrict__ out, unsigned long long *__restrict__ counters) {
  const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6);
  uint32_t px, k;
  tile8_pixel(fr, tile, threadIdx.x & 63u, px, k);
  WorkCounters cnt = {};
  WorkCounters seg = {};                      /* the shading's counts since the last opaque fragment: what reaches the pixel (pin 4) */
  const bool inImage = px < fr.width && k < fr.rows;
  float nx, ny, viewDepthPerS = 0.0f;
  Ray ray; ray.origin = F3(0.0f, 0.0f, 0.0f); ray.dir = F3(0.0f, 0.0f, 1.0f);
  if (inImage) {
    const uint32_t py_gl = fr.height - 1u - image_row(fr, k);
    ray.dir = primary_dir(fr, 0, px, py_gl, nx, ny, viewDepthPerS);
    ray.origin = frame_camera(fr, 0);
  }
  const f3 camera = frame_camera(fr, 0), ambient = frame_ambient(fr, 0);
  WalkState w;
  w.tR = ray; w.minLen = POW32;
  reciprocalOfDir(sc, ray.dir, ray.origin, w.inv, w.fastDiv);
  int cachedTI = 0;
  uint32_t nxt = inImage ? sc.fwd_root : WALK_END;
  const fwd_cf4 *L = (const fwd_cf4 *)sc.fwd;
  uint32_t thin = 0;
  bool alone = false;                         /* (wave-uniform) */
  bool pending = false, covered = false;
  f3 pSuv = F3(0.0f, 0.0f, 0.0f);
  int pTI = 0, pTri = 0;
  float4 color = make_float4(0.f, 0.f, 0.f, 0.f);
  for (;;) {
    float4 e0 = make_float4(0.f, 0.f, 0.f, 0.f), e1 = e0, e2 = e0;
    bool mine = false;
    if (!alone) {
      const uint32_t i = __builtin_amdgcn_readfirstlane(__ockl_wfred_min_u32(nxt));
      if (i == WALK_END) {
        if (flx_ballot(pending) == 0ull) break;
      } else {
        uint32_t iu = i;
        asm volatile("" : "+s"(iu));                 /* (a scalar: scalar loads, as in primaryWalkF) */
        const fwd_cf4 *E = L + (size_t)iu * 3u;
        const flx_v4f_ a = E[0], b = E[1], c = E[2];
        e0 = make_float4(a.x, a.y, a.z, a.w); e1 = make_float4(b.x, b.y, b.z, b.w); e2 = make_float4(c.x, c.y, c.z, c.w);
        mine = nxt == i;
        thin = (uint32_t)__popcll(flx_ballot(mine)) < (uint32_t)FLX_PRIMARY_LOCK_MIN ? thin + 1u : 0u;
        alone = thin >= 2u;
      }
    } else {
      mine = nxt != WALK_END;
      if (flx_ballot(mine || pending) == 0ull) break;
      if (mine) { const size_t i = (size_t)nxt * 3u; e0 = sc.fwd[i]; e1 = sc.fwd[i + 1]; e2 = sc.fwd[i + 2]; }
    }
    /* what to shade at this step: the pending fragment, when a translucent fragment comes to lie over it, or in the step after
     * the lane's walk has ended */
    bool shadeNow = false;
    f3 sSuv = pSuv;
    int sTI = pTI, sTri = pTri;
    if (mine) {
      if (COUNT) cnt.primary_visits++;
      const int meta = __float_as_int(e2.z);
      if ((meta & 3) == 0) {
        nxt = WALK_END;                          /* terminator (its fetch counts) */
      } else {
        const int tI = (meta >> 2) << 1;
        if (tI != cachedTI) {
          const int iI = tI + 1;
          const M3 rotationII = rotation_at(sc, iI);
          cachedTI = tI;
          w.tR.origin = mul(rotationII, ray.origin + shift_at(sc, iI));
          w.tR.dir = mul(rotationII, ray.dir);
          reciprocalOfDir(sc, w.tR.dir, w.tR.origin, w.inv, w.fastDiv);
        }
        if ((meta & 3) == 1) {
          nxt = (uint32_t)__float_as_int(rayCuboidFast(w.minLen, w, F3(e0.x, e0.y, e0.z), F3(e0.w, e1.x, e1.y)) ? e2.x : e2.y);
        } else {
          nxt = (uint32_t)__float_as_int(e2.y);
          f3 suv;
          if (moellerTrumboreRasterE(F3(e0.x, e0.y, e0.z), F3(e0.w, e1.x, e1.y), F3(e1.z, e1.w, e2.x), w.tR, w.minLen, viewDepthPerS, suv)) {
            w.minLen = suv.x;                    /* the depth test passed: depthMask(true) */
            covered = true;
            const int tri = __float_as_int(e2.w);
            if (rasterOpaque(rasterTpoX(sc, fr, suv, tri))) {
              color = make_float4(0.f, 0.f, 0.f, 0.f);
              if (COUNT) { seg.shades = 0; seg.shadow_walks = 0; seg.shadow_visits = 0; seg.atlas_texels = 0; }
            } else {
              shadeNow = pending;
            }
            pending = true;
            pSuv = suv; pTI = tI; pTri = tri;
          }
        }
      }
    } else if (pending && nxt == WALK_END) {     /* the walk has ended: its last fragment */
      shadeNow = true; pending = false;
    }
    if (shadeNow) rasterBlend(rasterShade<COUNT>(sc, fr, hdr, camera, ambient, sSuv, sTI, sTri, seg), color);
  }
  if (COUNT) { cnt.shades += seg.shades; cnt.shadow_walks += seg.shadow_walks; cnt.shadow_visits += seg.shadow_visits; cnt.atlas_texels += seg.atlas_texels; }
  if (inImage) {
    if (COUNT && covered) cnt.primary_hits++;
    rasterStore(out, (size_t)k * fr.width + px, color);
  }
  flush_counters<COUNT>(cnt, counters);
}

void launch_raster(const DeviceScene &sc, const DeviceFrame &fr, int hdr, float4 *out, unsigned long long *counters, hipStream_t stream) {
  const uint32_t tiles = ((fr.width + 7u) >> 3) * ((fr.rows + 7u) >> 3);
  const uint32_t blocks = (tiles + 3u) / 4u;
  if (counters) hipLaunchKernelGGL((k_raster<true, float4>), dim3(blocks), dim3(256), 0, stream, sc, fr, hdr, out, counters);
  else hipLaunchKernelGGL((k_raster<false, float4>), dim3(blocks), dim3(256), 0, stream, sc, fr, hdr, out, counters);
}

void launch_raster(const DeviceScene &sc, const DeviceFrame &fr, int hdr, uint32_t *out8, hipStream_t stream) {
  const uint32_t tiles = ((fr.width + 7u) >> 3) * ((fr.rows + 7u) >> 3);
  const uint32_t blocks = (tiles + 3u) / 4u;
  hipLaunchKernelGGL((k_raster<false, uint32_t>), dim3(blocks), dim3(256), 0, stream, sc, fr, hdr, out8, (unsigned long long *)nullptr);
}

}  // namespace flx
