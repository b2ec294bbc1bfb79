/*
 * flx_atlas.hip — flx_textures_upload's and flx_texture_update's kernel: source images nearest-resampled into the cells of an RGBA8 atlas, by the project's own rule
 * (js/sceneFile.js: buildAtlas), in integers.
 *
 *   k_atlas_cells   grid z: the image (a stride loop beyond 65535), grid y: bands of the cell's rows, grid x: quads of a row.  A lane makes FOUR adjacent texels of
 *                   one destination row and stores them as one 16-byte store where their address allows it — the row's start in the atlas is a multiple of four
 *                   texels whenever the cell width is — and as single texels otherwise: the w % 4 texels at a row's end, and cells whose origin is not 16-byte
 *                   aligned (cell widths that are no multiple of 4).  The source reads are gathers of 4 or 16 bytes: a destination row reads one source row, at
 *                   non-decreasing columns, so the lanes of a row read one line after the other; no LDS.
 *
 * The destination is the atlas (pitch = its width) or the context's stage of one cell (pitch = w).  The kernel writes the texels of the cells it is given and
 * nothing else: what lies outside the cells of a build is cleared by its caller, and an update changes no byte outside its cell.
 */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "flx_kernels.h"
#include "flx_kernel_util.h"

namespace flx {

namespace {

struct AtlasCells {
  uint32_t *dst;
  uint32_t pitch, w, h, tw, first_cell, n;
  uint32_t xshift;                       /* a workgroup's 256 lanes: 1 << xshift quads of a row by 256 >> xshift rows */
  const AtlasSource *table;
  AtlasSource one;
};

/* floor((2d + 1) * s / (2 * size)); narrow: 2 * size * s fits 32 bits, and so does every numerator */
__device__ __forceinline__ uint32_t sourceTexel(uint32_t d, uint32_t s, uint32_t size, bool narrow) {
  if (narrow) return ((2u * d + 1u) * s) / (2u * size);
  return (uint32_t)(((uint64_t)(2u * d + 1u) * s) / (2ull * size));
}

__device__ __forceinline__ uint32_t fetchTexel(const AtlasSource &s, size_t at) {
  if (s.format == ATLAS_RGBA32F) {
    const float4 v = ((const float4 *)s.pixels)[at];
    return pack_rgba8(v.x, v.y, v.z, v.w);
  }
  return ((const uint32_t *)s.pixels)[at];
}

__global__ __launch_bounds__(256) void k_atlas_cells(const AtlasCells a) {
  const uint32_t quads = (a.w + 3u) >> 2;
  const uint32_t q = (blockIdx.x << a.xshift) + (threadIdx.x & ((1u << a.xshift) - 1u));
  if (q >= quads) return;
  const uint32_t x0 = q << 2, rows = 256u >> a.xshift;
  const uint32_t take = min(4u, a.w - x0);                     /* texels of this quad inside the cell */
  for (uint32_t img = blockIdx.z; img < a.n; img += gridDim.z) {
    const AtlasSource s = a.table ? a.table[img] : a.one;
    const uint32_t cell = a.first_cell + img;
    const size_t origin = (size_t)(cell / a.tw) * a.h * a.pitch + (size_t)(cell % a.tw) * a.w + x0;
    const bool narrowX = (uint64_t)2u * a.w * s.sw <= 0xffffffffull, narrowY = (uint64_t)2u * a.h * s.sh <= 0xffffffffull;
    uint32_t sx[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) sx[k] = sourceTexel(min(x0 + k, a.w - 1u), s.sw, a.w, narrowX);
    for (uint32_t y = blockIdx.y * rows + (threadIdx.x >> a.xshift); y < a.h; y += gridDim.y * rows) {
      const size_t row = (size_t)sourceTexel(y, s.sh, a.h, narrowY) * s.sw;
      const size_t d = origin + (size_t)y * a.pitch;
      uint32_t t[4];
#pragma unroll
      for (uint32_t k = 0; k < 4u; k++) t[k] = k < take ? fetchTexel(s, row + sx[k]) : 0u;
      if (take == 4u && (d & 3u) == 0u) {
        *(uint4 *)(a.dst + d) = make_uint4(t[0], t[1], t[2], t[3]);
      } else {
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) if (k < take) a.dst[d + k] = t[k];
      }
    }
  }
}

}  // namespace

void launch_atlas_cells(uint32_t *dst, uint32_t pitch, uint32_t w, uint32_t h, uint32_t tw, uint32_t first_cell, uint32_t n, const AtlasSource *table,
                        const AtlasSource *one, hipStream_t stream) {
  if (n == 0u || w == 0u || h == 0u) return;
  AtlasCells a;
  a.dst = dst; a.pitch = pitch; a.w = w; a.h = h; a.tw = tw; a.first_cell = first_cell; a.n = n; a.table = table;
  a.one = one ? *one : AtlasSource{ nullptr, 0u, 0u, 0u, 0u };
  const uint32_t quads = (w + 3u) >> 2;
  a.xshift = 0;
  while (a.xshift < 6u && (1u << a.xshift) < quads) a.xshift++;          /* (at most a wave across a row: w <= 2048 is 512 quads, 8 workgroups) */
  const uint32_t rows = 256u >> a.xshift;
  const dim3 grid((quads + (1u << a.xshift) - 1u) >> a.xshift, std::min((h + rows - 1u) / rows, 65535u), std::min(n, 65535u));
  hipLaunchKernelGGL(k_atlas_cells, grid, dim3(256), 0, stream, a);
}

}  // namespace flx
