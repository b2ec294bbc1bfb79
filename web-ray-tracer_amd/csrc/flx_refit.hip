/*
 * flx_refit.hip — flx_scene_update's kernels: the rows of a scene whose vertices moved, the boxes above them, the two derived copies.
 *
 * The flatten defines a box as the exact componentwise min / max of every vertex beneath it (modules/scene.js:242-256, 269-279); in the DFS pre-order
 * of the entry array "beneath box i" is the range (i, i + skip].  Min and max are exact and associative, so any decomposition of that range query
 * gives the flatten's bits.  Here, two levels of 256:
 *   k_refit_entries   a workgroup per 256 entries: per-entry triangle bounds, their inclusive prefix and suffix inside the block (LDS scans), the block's total;
 *                     boxes whose range ends inside their own block are answered here, from LDS;
 *   k_refit_blocks    the same scans over the block totals (256 blocks = 65 536 entries a superblock);
 *   k_refit_boxes     every other box: suffix of its first block + whole blocks + prefix of its last block, the whole blocks the same way one level up.
 * Bounds are kept as ORDERED KEYS — the float's bits with the sign folded so that unsigned comparison is the total order -inf < .. < -0 < +0 < .. < +inf,
 * which is how Math.min / Math.max order equal-comparing zeros — so min / max are integer operations and the key maps back to the very float.  (NaN has no
 * place in that order as Math.min treats it: the host refuses NaN vertices.)  No atomics, no level-per-launch climb of the tree.
 *
 * flx_scene_update_device hands the rows over in device memory: k_rows_check_stage holds them against the scene as flx_scene_update's loop does on the host,
 * and copies them into the context's stage in the same pass.
 */
#include <hip/hip_runtime.h>

#include "flx_kernels.h"
#include "flx_kernel_util.h"

namespace flx {

namespace {

constexpr uint32_t RB = 256;                       /* entries per block, blocks per superblock, threads per workgroup */
struct Bounds { uint32_t k[6]; };                  /* keys (flx_kernel_util.h): min x y z, max x y z */

__device__ __forceinline__ Bounds none() { return Bounds{ { KEY_NONE_LO, KEY_NONE_LO, KEY_NONE_LO, KEY_NONE_HI, KEY_NONE_HI, KEY_NONE_HI } }; }
__device__ __forceinline__ void join(Bounds &a, const Bounds &b) {
#pragma unroll
  for (int c = 0; c < 3; c++) { a.k[c] = min(a.k[c], b.k[c]); a.k[3 + c] = max(a.k[3 + c], b.k[3 + c]); }
}
__device__ __forceinline__ bool empty(const Bounds &b) { return b.k[0] == KEY_NONE_LO && b.k[3] == KEY_NONE_HI; }      /* (no finite x is both) */

/* a Bounds per item in global memory: 6 words, 8-byte aligned */
__device__ __forceinline__ Bounds loadBounds(const uint32_t *p, size_t i) {
  const uint2 *q = (const uint2 *)(p + i * 6);
  const uint2 a = q[0], b = q[1], c = q[2];
  return Bounds{ { a.x, a.y, b.x, b.y, c.x, c.y } };
}
__device__ __forceinline__ void storeBounds(uint32_t *p, size_t i, const Bounds &b) {
  uint2 *q = (uint2 *)(p + i * 6);
  q[0] = make_uint2(b.k[0], b.k[1]); q[1] = make_uint2(b.k[2], b.k[3]); q[2] = make_uint2(b.k[4], b.k[5]);
}

/* Inclusive prefix (lower items first) and suffix of `mine` over the workgroup's RB items, through lds[6][RB].  Every thread calls. */
__device__ __forceinline__ void blockScans(const Bounds &mine, uint32_t (*lds)[RB], Bounds &prefix, Bounds &suffix) {
  const uint32_t t = threadIdx.x;
  prefix = mine; suffix = mine;
  for (uint32_t d = 1; d < RB; d <<= 1) {
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 6; c++) lds[c][t] = prefix.k[c];
    __syncthreads();
    if (t >= d) {
      Bounds o;
#pragma unroll
      for (int c = 0; c < 6; c++) o.k[c] = lds[c][t - d];
      join(prefix, o);
    }
  }
  for (uint32_t d = 1; d < RB; d <<= 1) {
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 6; c++) lds[c][t] = suffix.k[c];
    __syncthreads();
    if (t + d < RB) {
      Bounds o;
#pragma unroll
      for (int c = 0; c < 6; c++) o.k[c] = lds[c][t + d];
      join(suffix, o);
    }
  }
  __syncthreads();
}

__device__ __forceinline__ Bounds triangleBounds(const float4 &g0, const float4 &g1, const float4 &g2) {
  Bounds b;
  const float x[3] = { g0.x, g0.w, g1.z }, y[3] = { g0.y, g1.x, g1.w }, z[3] = { g0.z, g1.y, g2.x };
  b.k[0] = min(min(keyOf(x[0]), keyOf(x[1])), keyOf(x[2])); b.k[3] = max(max(keyOf(x[0]), keyOf(x[1])), keyOf(x[2]));
  b.k[1] = min(min(keyOf(y[0]), keyOf(y[1])), keyOf(y[2])); b.k[4] = max(max(keyOf(y[0]), keyOf(y[1])), keyOf(y[2]));
  b.k[2] = min(min(keyOf(z[0]), keyOf(z[1])), keyOf(z[2])); b.k[5] = max(max(keyOf(z[0]), keyOf(z[1])), keyOf(z[2]));
  return b;
}

/* words 0..5 of box row i (g1: its second float4 as loaded: words 6 and 7 stay) */
__device__ __forceinline__ void storeBox(float4 *geometry, size_t i, const Bounds &b, float4 g1) {
  geometry[i * 3] = make_float4(floatOf(b.k[0]), floatOf(b.k[1]), floatOf(b.k[2]), floatOf(b.k[3]));
  g1.x = floatOf(b.k[4]); g1.y = floatOf(b.k[5]);
  geometry[i * 3 + 1] = g1;
}

/* the box's skip count (flx_scene_upload checked: 0 <= skip, i + skip < n_entries) */
__device__ __forceinline__ uint32_t skipOf(const float4 &g1) { return (uint32_t)g1.z; }

__global__ __launch_bounds__(RB) void k_scene_rows(const float4 *__restrict__ rows, float4 *__restrict__ geometry, uint32_t first, uint32_t count /* float4 */) {
  const uint32_t q = blockIdx.x * RB + threadIdx.x;
  if (q >= count) return;
  const uint32_t row = q / 3u, part = q - row * 3u;
  float4 v = rows[q];
  const size_t at = ((size_t)first + row) * 3 + part;
  if (rows[row * 3u + 2u].z == 1.0f) {             /* a box: the refit owns words 0..5 (and a box it does not answer keeps them) */
    if (part == 0u) return;
    if (part == 1u) { const float4 old = geometry[at]; v.x = old.x; v.y = old.y; }
  }
  geometry[at] = v;
}

__global__ __launch_bounds__(RB) void k_refit_entries(float4 *__restrict__ geometry, uint32_t n, uint32_t *__restrict__ pre0, uint32_t *__restrict__ suf0,
                                                      uint32_t *__restrict__ tot0) {
  __shared__ uint32_t val[6][RB], scan[6][RB];
  const uint32_t t = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * RB + t;
  Bounds mine = none();
  float4 g1 = make_float4(0.f, 0.f, 0.f, 0.f);
  uint32_t skip = 0;                               /* > 0: a box with entries beneath it */
  if (i < n) {
    const float4 g2 = geometry[i * 3 + 2];
    if (g2.z == 2.0f) {
      mine = triangleBounds(geometry[i * 3], geometry[i * 3 + 1], g2);
    } else if (g2.z == 1.0f) {
      g1 = geometry[i * 3 + 1];
      skip = skipOf(g1);
    }
  }
#pragma unroll
  for (int c = 0; c < 6; c++) val[c][t] = mine.k[c];
  Bounds prefix, suffix;
  blockScans(mine, scan, prefix, suffix);          /* (its first barrier publishes val) */
  if (i < n) { storeBounds(pre0, i, prefix); storeBounds(suf0, i, suffix); }
  if (t == RB - 1) storeBounds(tot0, blockIdx.x, prefix);
  if (skip > 0u && t + skip < RB) {                /* (t, t + skip] lies in this block */
    Bounds b = none();
    for (uint32_t j = t + 1; j <= t + skip; j++) {
      Bounds o;
#pragma unroll
      for (int c = 0; c < 6; c++) o.k[c] = val[c][j];
      join(b, o);
    }
    if (!empty(b)) storeBox(geometry, i, b, g1);
  }
}

__global__ __launch_bounds__(RB) void k_refit_blocks(const uint32_t *__restrict__ tot0, uint32_t nb0, uint32_t *__restrict__ pre1, uint32_t *__restrict__ suf1,
                                                     uint32_t *__restrict__ tot1) {
  __shared__ uint32_t scan[6][RB];
  const uint32_t t = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * RB + t;
  const Bounds mine = i < nb0 ? loadBounds(tot0, i) : none();
  Bounds prefix, suffix;
  blockScans(mine, scan, prefix, suffix);
  if (i < nb0) { storeBounds(pre1, i, prefix); storeBounds(suf1, i, suffix); }
  if (t == RB - 1) storeBounds(tot1, blockIdx.x, prefix);
}

/* min / max over the items [lo, hi] of one level, lo and hi in DIFFERENT blocks of RB or lo at a block's start: the suffix of lo's block (all of it where lo starts
 * it), the prefix of hi's block (all of it where hi ends it) joined into acc; -> the whole blocks between, [firstWhole, lastWhole] (none if firstWhole > lastWhole) */
__device__ __forceinline__ void rangeEnds(const uint32_t *pre, const uint32_t *suf, uint32_t lo, uint32_t hi, Bounds &acc, uint32_t &firstWhole, uint32_t &lastWhole) {
  firstWhole = lo / RB; lastWhole = hi / RB;
  if (lo % RB != 0u) { join(acc, loadBounds(suf, lo)); firstWhole++; }
  if (hi % RB != RB - 1u) {                        /* (lastWhole-- cannot wrap below firstWhole's block: see the caller's cases) */
    join(acc, loadBounds(pre, hi));
    if (lastWhole == 0u) { firstWhole = 1u; return; }      /* hi in block 0: nothing whole */
    lastWhole--;
  }
}

__global__ __launch_bounds__(RB) void k_refit_boxes(float4 *__restrict__ geometry, uint32_t n, const uint32_t *__restrict__ pre0, const uint32_t *__restrict__ suf0,
                                                    const uint32_t *__restrict__ tot0, const uint32_t *__restrict__ pre1, const uint32_t *__restrict__ suf1,
                                                    const uint32_t *__restrict__ tot1) {
  const uint32_t i = blockIdx.x * RB + threadIdx.x;
  if (i >= n) return;
  if (geometry[(size_t)i * 3 + 2].z != 1.0f) return;
  const float4 g1 = geometry[(size_t)i * 3 + 1];
  const uint32_t skip = skipOf(g1);
  if (skip == 0u || i % RB + skip < RB) return;    /* nothing beneath it; answered in its own block (k_refit_entries) */
  /* lo = i + 1 is in a later block than i, or in i's block with hi in a later one */
  const uint32_t lo = i + 1u, hi = i + skip;
  Bounds acc = none();
  uint32_t fw, lw;
  rangeEnds(pre0, suf0, lo, hi, acc, fw, lw);
  if (fw <= lw) {                                  /* whole blocks fw .. lw: the same question one level up, over the block totals */
    if (fw / RB == lw / RB && fw % RB != 0u && lw % RB != RB - 1u) {
      for (uint32_t b = fw; b <= lw; b++) join(acc, loadBounds(tot0, b));      /* inside one superblock, touching neither end: at most RB - 2 totals */
    } else if (fw / RB == lw / RB && fw % RB != 0u) {
      join(acc, loadBounds(suf1, fw));             /* .. to its end */
    } else {
      uint32_t fs, ls;
      rangeEnds(pre1, suf1, fw, lw, acc, fs, ls);
      for (uint32_t s = fs; s <= ls && fs <= ls; s++) join(acc, loadBounds(tot1, s));      /* whole superblocks: n / 65 536 at the most */
    }
  }
  if (!empty(acc)) storeBox(geometry, i, acc, g1);
}

__global__ __launch_bounds__(RB) void k_rederive(const float4 *__restrict__ geometry, uint32_t n, float4 *__restrict__ copy, uint32_t entries) {
  const uint32_t e = blockIdx.x * RB + threadIdx.x;
  if (e >= entries) return;
  float4 c2 = copy[(size_t)e * 3 + 2];
  const uint32_t type = __float_as_uint(c2.z) & 3u, orig = __float_as_uint(c2.w);
  if ((type != 1u && type != 2u) || orig >= n) return;      /* the shared terminator */
  const float4 g0 = geometry[(size_t)orig * 3], g1 = geometry[(size_t)orig * 3 + 1];
  if (type == 1u) {
    float4 c1 = copy[(size_t)e * 3 + 1];
    c1.x = g1.x; c1.y = g1.y;
    copy[(size_t)e * 3] = g0;
    copy[(size_t)e * 3 + 1] = c1;
  } else {                                         /* vertex a and the edges b - a, c - a: build_threaded's subtractions */
    const float4 g2 = geometry[(size_t)orig * 3 + 2];
    copy[(size_t)e * 3] = make_float4(g0.x, g0.y, g0.z, g0.w - g0.x);
    copy[(size_t)e * 3 + 1] = make_float4(g1.x - g0.y, g1.y - g0.z, g1.z - g0.x, g1.w - g0.y);
    c2.x = g2.x - g0.z;
    copy[(size_t)e * 3 + 2] = c2;
  }
}

/* flx_scene_update_device: the caller's rows are in device memory.  One streaming pass, a lane per float4: the first 3 * n_rows lanes take the geometry rows, the
 * 7 * n_rows behind them the attribute rows (where given).  Every float4 goes into the context's stage as it is, and the geometry lanes hold their part of the row
 * against the scene's own array by flx_scene_update's rules, compared as bits like there:
 *   0  word 10 (kind) differs;  for kind != 0:  1  word 9 (transform number) differs;  a box:  2  word 6 (skip count) differs;  otherwise:  3  a vertex word
 *   that is not finite.
 * The host's loop returns at the first offending row and, within it, at the first of these rules in this order: that is the least row * 4 + rule, so
 * verdict[0] takes an unsigned min of it (set to ~0 before the launch: no row offends).  verdict[1], set to ~0 likewise, becomes 0 when a vertex lies beyond
 * the fast box test's bound.  A wave reduces its lanes' keys before one of them issues the atomic, and only where there is something to report.
 * (Words 6, 9 and 10 of the scene's array hold the same bits from one flx_scene_upload to the next, whatever updates run beside this kernel.) */
__global__ __launch_bounds__(RB) void k_rows_check_stage(const float4 *__restrict__ rows, const float4 *__restrict__ attributes, const float4 *__restrict__ geometry,
                                                         uint32_t first, uint32_t n_rows, float4 *__restrict__ stage_rows, float4 *__restrict__ stage_attributes,
                                                         uint32_t *__restrict__ verdict) {
  const uint32_t q = blockIdx.x * RB + threadIdx.x;      /* (n_rows < 2^28: 10 * n_rows fits) */
  const uint32_t gcount = n_rows * 3u;
  uint32_t key = 0xffffffffu;
  bool beyond = false;
  if (q < gcount) {
    const float4 v = rows[q];
    stage_rows[q] = v;
    const uint32_t row = q / 3u, part = q - row * 3u;
    const float4 last = part == 2u ? v : rows[row * 3u + 2u];      /* words 8 .. 11: the kind the row claims decides what is looked at */
    const float kind = last.z;
    const size_t at = ((size_t)first + row) * 3 + part;
    uint32_t rule = 4u;
    if (part == 2u) {
      const float4 have = geometry[at];
      if (__float_as_uint(v.z) != __float_as_uint(have.z)) rule = 0u;
      else if (kind != 0.0f && __float_as_uint(v.y) != __float_as_uint(have.y)) rule = 1u;
    }
    if (kind == 1.0f) {
      if (part == 1u && __float_as_uint(v.z) != __float_as_uint(geometry[at].z)) rule = min(rule, 2u);
    } else if (kind != 0.0f) {                     /* nine vertex words: 0 .. 3, 4 .. 7, 8 */
      const float w[4] = { v.x, v.y, v.z, v.w };
      const int words = part == 2u ? 1 : 4;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (k < words) {
          const float a = fabsf(w[k]);
          if (!(a < __builtin_inff())) rule = min(rule, 3u);      /* inf and NaN */
          if (!(a <= FLX_FAST_BOX_BOUND)) beyond = true;
        }
      }
    }
    if (rule < 4u) key = row * 4u + rule;
  } else if (attributes && q - gcount < n_rows * 7u) {
    stage_attributes[q - gcount] = attributes[q - gcount];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, d));
  const bool anyBeyond = __any(beyond);
  if ((threadIdx.x & 63u) == 0u) {
    if (key != 0xffffffffu) atomicMin(&verdict[0], key);
    if (anyBeyond) atomicMin(&verdict[1], 0u);
  }
}

struct RefitWork { uint32_t *pre0, *suf0, *tot0, *pre1, *suf1, *tot1; uint32_t nb0, nb1; size_t words; };
RefitWork refit_layout(uint32_t n, uint32_t *base) {
  RefitWork w;
  w.nb0 = (n + RB - 1) / RB; w.nb1 = (w.nb0 + RB - 1) / RB;
  size_t at = 0;
  auto take = [&](size_t items) { uint32_t *p = base ? base + at : nullptr; at += items * 6; return p; };
  w.pre0 = take(n); w.suf0 = take(n); w.tot0 = take(w.nb0); w.pre1 = take(w.nb0); w.suf1 = take(w.nb0); w.tot1 = take(w.nb1);
  w.words = at;
  return w;
}

}  // namespace

size_t refit_workspace_words(uint32_t n_entries) { return refit_layout(n_entries, nullptr).words; }

void launch_scene_rows(const float4 *rows, float4 *geometry, uint32_t first, uint32_t n_rows, hipStream_t stream) {
  const uint32_t count = n_rows * 3u;              /* (n_rows < 2^28: flx_scene_upload) */
  if (count) hipLaunchKernelGGL(k_scene_rows, dim3((count + RB - 1) / RB), dim3(RB), 0, stream, rows, geometry, first, count);
}

void launch_rows_check_stage(const float4 *rows, const float4 *attributes, const float4 *geometry, uint32_t first, uint32_t n_rows, float4 *stage_rows,
                             float4 *stage_attributes, uint32_t *verdict, hipStream_t stream) {
  const uint32_t count = n_rows * (attributes ? 10u : 3u);
  if (count) hipLaunchKernelGGL(k_rows_check_stage, dim3((count + RB - 1) / RB), dim3(RB), 0, stream, rows, attributes, geometry, first, n_rows, stage_rows,
                                stage_attributes, verdict);
}

void launch_refit(float4 *geometry, uint32_t n_entries, uint32_t *work, hipStream_t stream) {
  if (!n_entries) return;
  const RefitWork w = refit_layout(n_entries, work);
  hipLaunchKernelGGL(k_refit_entries, dim3(w.nb0), dim3(RB), 0, stream, geometry, n_entries, w.pre0, w.suf0, w.tot0);
  hipLaunchKernelGGL(k_refit_blocks, dim3(w.nb1), dim3(RB), 0, stream, w.tot0, w.nb0, w.pre1, w.suf1, w.tot1);
  hipLaunchKernelGGL(k_refit_boxes, dim3(w.nb0), dim3(RB), 0, stream, geometry, n_entries, w.pre0, w.suf0, w.tot0, w.pre1, w.suf1, w.tot1);
}

void launch_rederive(const float4 *geometry, uint32_t n_entries, float4 *copy, uint32_t entries, hipStream_t stream) {
  if (entries) hipLaunchKernelGGL(k_rederive, dim3((entries + RB - 1) / RB), dim3(RB), 0, stream, geometry, n_entries, copy, entries);
}

}  // namespace flx
