/*
 * flx_splice.hip — flx_scene_splice_device's kernels: a block of the resident entry array replaced, inserted or removed where the arrays are, in device memory.
 *
 *   k_splice_check   a lane per entry and per id of the RESIDENT scene, which an upload has validated (every box: 0 <= skip, entry + skip inside the array).  It
 *                    finds `end` — 1 + the last entry whose word 10 is not 0, the reference's textureLength —, how many ids lie below first_entry and how many at
 *                    or above first_entry + n_old, and the first entry that offends a rule of the splice and its first rule there, as the least key
 *                    entry * 4 + rule:
 *                      0  the parent: it is no box, or its range (parent, parent + skip] does not hold the replaced rows (an insertion: first_entry lies beyond
 *                         parent + skip + 1); a parent_entry that does not lie in front of first_entry offends at entry first_entry;
 *                      1  a box in front of first_entry — behind the parent, or anywhere with FLX_NO_PARENT — reaches first_entry: the parent is not the direct one;
 *                      2  a box among the replaced rows reaches beyond them;
 *                      3  an id lies below the id in front of it (the list is not non-decreasing); it offends at the entry it names, held inside the array.
 *                    It reads words 6 and 10 and the ids, which hold the same bits from one upload to the next, and writes the record alone.
 *   k_splice_rows    the streaming assembly of both arrays into FRESH buffers, a lane per 16 bytes: the 3 float4 of every geometry row, then the 7 of every
 *                    attribute row.  A row in front of first_entry is the old row, the n_new behind it are the caller's, the old tail [first_entry + n_old, end)
 *                    follows moved by delta = n_new - n_old, zeros pad up to the array's length.  Word 6 of the parent and of every box whose range holds the
 *                    parent grows by delta, in integer arithmetic (the lane of a row's second float4 looks at the row's word 10 for it; no other lane reads
 *                    more than its own 16 bytes).
 *   k_splice_ids     the old ids below first_entry, the block's plus first_entry, the old ids at or above first_entry + n_old plus delta: the id list is
 *                    non-decreasing, so the first are its first `below` items and the last its last `above`.
 *
 * The boxes' six floats are launch_refit's (flx_refit.hip) over the assembled array, the derived copies launch_derive_copies' (flx_derive.hip).
 */
#include <hip/hip_runtime.h>

#include "flexlight_hip_debug.h"
#include "flx_kernels.h"

namespace flx {

namespace {

constexpr uint32_t SB = 256;                       /* threads per workgroup */

/* the resident scene's box i covers (i, i + skip]; an upload checked 0 <= skip and i + skip < n */
__device__ __forceinline__ uint32_t reachOf(uint32_t i, float skip) { return i + (uint32_t)skip; }

/* record zeroed.  record[SPLICE_REC_VERDICT] takes the max of ~key: 0 says nothing offends, else the least key is its complement. */
__global__ __launch_bounds__(SB) void k_splice_check(const float4 *__restrict__ geometry, uint32_t n, const int32_t *__restrict__ ids, uint32_t n_ids, uint32_t first,
                                                     uint32_t n_old, uint32_t parent, uint32_t *__restrict__ record) {
  const uint32_t i = blockIdx.x * SB + threadIdx.x;
  const uint32_t last = first + n_old;             /* (the host checked: <= n < 2^28) */
  uint32_t notKey = 0u, end = 0u;
  bool below = false, above = false;
  if (i == 0u && parent != FLX_NO_PARENT && parent >= first) notKey = ~(first * 4u + 0u);
  if (i < n) {
    const float4 g1 = geometry[(size_t)i * 3 + 1], g2 = geometry[(size_t)i * 3 + 2];
    const bool box = g2.z == 1.0f;
    const uint32_t reach = box ? reachOf(i, g1.z) : i;
    if (g2.z != 0.0f) end = i + 1u;
    uint32_t rule = 4u;
    if (i == parent && parent < first && (!box || (n_old ? last - 1u > reach : first > reach + 1u))) rule = 0u;
    else if (box && i < first && (parent == FLX_NO_PARENT || i > parent) && reach >= first) rule = 1u;
    else if (box && i >= first && i < last && reach >= last) rule = 2u;
    if (rule < 4u) notKey = max(notKey, ~(i * 4u + rule));
  }
  if (i < n_ids) {
    const int32_t id = ids[i];
    below = id < (int32_t)first;
    above = id >= (int32_t)last;
    if (i + 1u < n_ids) {
      const int32_t next = ids[i + 1u];
      if (next < id) notKey = max(notKey, ~((uint32_t)min(max(next, 0), (int32_t)n - 1) * 4u + 3u));
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    notKey = max(notKey, (uint32_t)__shfl_xor((int)notKey, d));
    end = max(end, (uint32_t)__shfl_xor((int)end, d));
  }
  const uint32_t belows = (uint32_t)__popcll(__ballot(below)), aboves = (uint32_t)__popcll(__ballot(above));
  if ((threadIdx.x & 63u) == 0u) {                 /* a wave's lanes reduced: one atomic each, and only where there is something to report */
    if (notKey) atomicMax(&record[SPLICE_REC_VERDICT], notKey);
    if (end) atomicMax(&record[SPLICE_REC_END], end);
    if (belows) atomicAdd(&record[SPLICE_REC_IDS_BELOW], belows);
    if (aboves) atomicAdd(&record[SPLICE_REC_IDS_ABOVE], aboves);
  }
}

/* the old array's float4 `part` of row `row` for the new array's row `to`, `width` float4 a row; nullptr: zeros */
__device__ __forceinline__ const float4 *sourceOf(const float4 *old, const float4 *block, uint32_t to, uint32_t part, uint32_t width, const SpliceShape &s) {
  if (to < s.first) return old + (size_t)to * width + part;
  if (to < s.first + s.n_new) return block + (size_t)(to - s.first) * width + part;
  if (to < s.end_new) return old + (size_t)(to - s.n_new + s.n_old) * width + part;      /* (to - delta: >= first + n_old, < end) */
  return nullptr;
}

__global__ __launch_bounds__(SB) void k_splice_rows(const float4 *__restrict__ geometry, const float4 *__restrict__ attributes, const float4 *__restrict__ blockGeometry,
                                                    const float4 *__restrict__ blockAttributes, SpliceShape s, float4 *__restrict__ geometryOut,
                                                    float4 *__restrict__ attributesOut) {
  const uint32_t q = blockIdx.x * SB + threadIdx.x;      /* (n_padded <= 2^24 + 255: 10 * n_padded fits) */
  const uint32_t gcount = s.n_padded * 3u;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  if (q < gcount) {
    const uint32_t row = q / 3u, part = q - row * 3u;
    const float4 *src = sourceOf(geometry, blockGeometry, row, part, 3u, s);
    float4 v = src ? *src : zero;
    if (part == 1u && s.parent != FLX_NO_PARENT && row <= s.parent && s.parent < s.first) {      /* an old row in front of the block: the parent or a box that holds it? */
      const bool box = geometry[(size_t)row * 3 + 2].z == 1.0f;
      if (box && (row == s.parent || reachOf(row, v.z) >= s.parent)) v.z = (float)((long long)(uint32_t)v.z + (long long)s.n_new - (long long)s.n_old);
    }
    geometryOut[q] = v;
  } else if (q - gcount < s.n_padded * 7u) {
    const uint32_t k = q - gcount, row = k / 7u, part = k - row * 7u;
    const float4 *src = sourceOf(attributes, blockAttributes, row, part, 7u, s);
    attributesOut[k] = src ? *src : zero;
  }
}

__global__ __launch_bounds__(SB) void k_splice_ids(const int32_t *__restrict__ ids, uint32_t n_ids, const int32_t *__restrict__ blockIds, uint32_t n_block, uint32_t below,
                                                   uint32_t above, uint32_t first, int32_t delta, int32_t *__restrict__ out) {
  const uint32_t k = blockIdx.x * SB + threadIdx.x;
  if (k >= below + n_block + above) return;
  if (k < below) out[k] = ids[k];
  else if (k < below + n_block) out[k] = blockIds[k - below] + (int32_t)first;
  else out[k] = ids[n_ids - above + (k - below - n_block)] + delta;
}

}  // namespace

void launch_splice_check(const float4 *geometry, uint32_t n_entries, const int32_t *ids, uint32_t n_ids, uint32_t first, uint32_t n_old, uint32_t parent, uint32_t *record,
                         hipStream_t stream) {
  const uint32_t lanes = n_entries > n_ids ? n_entries : n_ids;
  hipLaunchKernelGGL(k_splice_check, dim3((lanes + SB - 1) / SB), dim3(SB), 0, stream, geometry, n_entries, ids, n_ids, first, n_old, parent, record);
}

void launch_splice_rows(const float4 *geometry, const float4 *attributes, const float4 *blockGeometry, const float4 *blockAttributes, const SpliceShape &shape,
                        float4 *geometryOut, float4 *attributesOut, hipStream_t stream) {
  const uint32_t count = shape.n_padded * 10u;
  hipLaunchKernelGGL(k_splice_rows, dim3((count + SB - 1) / SB), dim3(SB), 0, stream, geometry, attributes, blockGeometry, blockAttributes, shape, geometryOut,
                     attributesOut);
}

void launch_splice_ids(const int32_t *ids, uint32_t n_ids, const int32_t *blockIds, uint32_t n_block, uint32_t below, uint32_t above, uint32_t first, int32_t delta,
                       int32_t *out, hipStream_t stream) {
  const uint32_t count = below + n_block + above;
  if (count) hipLaunchKernelGGL(k_splice_ids, dim3((count + SB - 1) / SB), dim3(SB), 0, stream, ids, n_ids, blockIds, n_block, below, above, first, delta, out);
}

}  // namespace flx
