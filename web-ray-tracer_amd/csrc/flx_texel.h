/* flx_texel.h — an RGBA8 render target's texel as the device code stores and fetches it, and temporal accumulation of one texel: shared by the denoise chain and the
 * frames' temporal pass (flx_filter.hip) and by the ray images' temporal instantiation of the planes kernel (flx_rays_planes.hip), so that both histories hold the
 * same bytes and average them by the same operations in the same order. */
#ifndef FLX_TEXEL_H
#define FLX_TEXEL_H

#include "flx_kernel_util.h"

namespace flx {

__device__ __forceinline__ f4 F4(float x, float y, float z, float w) { f4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }

/* k / 255 correctly rounded without the division: RN(k * RN(1/255)) and one residual correction (exact for all 256 bytes) */
__device__ __forceinline__ float unorm8(uint32_t k) {
  const float r = 1.0f / 255.0f, kf = (float)k;
  const float q = kf * r;
  return __builtin_fmaf(__builtin_fmaf(-q, 255.0f, kf), r, q);
}
__device__ __forceinline__ f4 unpack(uint32_t q) { return F4(unorm8(q & 255u), unorm8((q >> 8) & 255u), unorm8((q >> 16) & 255u), unorm8(q >> 24)); }
__device__ __forceinline__ uint32_t rawW(uint32_t q) { return q >> 24; }
__device__ __forceinline__ uint32_t pack(f4 v) { return pack_rgba8(v.x, v.y, v.z, v.w); }

/* Temporal accumulation of one texel (the shader modules/pathtracerWGL2.js:571-662 generates).  qc, qip, qid, qoid: the newest frame's colour, colour integer part,
 * location id and original id AS STORED at the ring's head; slot(k, c, ip, id, oid) fetches the texel's four words of the slot k frames old, 1 <= k < n.  The slots
 * are visited in groups of four, vec4(0) standing in for slots >= n: an all-zero id, an uncovered pixel, "matches" those stand-ins too, as in the shader.  The texels
 * are compared as bytes: two are equal as vec4s exactly when their bytes are (k / 255 is injective).  -> color: the average colour, glassFilter: the average glass
 * filter; centerW: the newest colour's alpha. */
template <typename SLOT>
__device__ __forceinline__ void temporal_texel(uint32_t qc, uint32_t qip, uint32_t qid, uint32_t qoid, int n, SLOT slot, f3 &color, float &glassFilter, float &centerW) {
  float counter = 1.0f, glassCounter = 1.0f;
  const f4 cc = unpack(qc), ci = unpack(qip);
  centerW = cc.w;
  color.x = cc.x + ci.x * 256.0f; color.y = cc.y + ci.y * 256.0f; color.z = cc.z + ci.z * 256.0f;
  glassFilter = ci.w;
  for (int k = 1; k < n; k += 4) {
    uint32_t cs[4], ips[4], ids[4], oids[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (k + j < n) slot(k + j, cs[j], ips[j], ids[j], oids[j]);
      else cs[j] = ips[j] = ids[j] = oids[j] = 0u;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) if (ids[j] == qid) {
      const f4 c = unpack(cs[j]), p = unpack(ips[j]);
      color.x += c.x + p.x * 256.0f; color.y += c.y + p.y * 256.0f; color.z += c.z + p.z * 256.0f;
      counter += 1.0f;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) if (oids[j] == qoid) {
      glassFilter += unorm8(rawW(ips[j]));
      glassCounter += 1.0f;
    }
  }
  color.x /= counter; color.y /= counter; color.z /= counter;
  glassFilter /= glassCounter;
}

/* what the pass writes of that average: with the filter RenderTexture[0] and IpRenderTexture[0] ... */
__device__ __forceinline__ uint32_t temporal_color_texel(f3 color, float centerW) {
  return pack(F4(flx_mod(color.x, 1.0f), flx_mod(color.y, 1.0f), flx_mod(color.z, 1.0f), centerW));
}
__device__ __forceinline__ uint32_t temporal_ip_texel(f3 color, float glassFilter) {
  return pack(F4(flx_floor(color.x) / 256.0f, flx_floor(color.y) / 256.0f, flx_floor(color.z) / 256.0f, glassFilter));
}
/* ... without it the canvas colour, tone-mapped where hdr == 1 */
__device__ __forceinline__ float temporal_tone(float c) {
  c = c / (c + 1.0f);
  const float gamma = 0.8f;
  return flx_pow(4.0f * c, 1.0f / gamma) / 4.0f * 1.3f;
}
__device__ __forceinline__ float4 temporal_canvas(f3 color, float centerW, int hdr) {
  if (hdr == 1) color = F3(temporal_tone(color.x), temporal_tone(color.y), temporal_tone(color.z));
  return make_float4(color.x, color.y, color.z, centerW);
}

}  // namespace flx
#endif
