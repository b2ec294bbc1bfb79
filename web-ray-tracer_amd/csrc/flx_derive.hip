/*
 * flx_derive.hip — flx_scene_upload_device's kernels: what flx_scene_upload decides and derives on the host (flx_scene.hip: its loop over the entries,
 * build_threaded, build_lockstep), decided and derived from an entry array that is in device memory.
 *
 *   k_derive_check      a lane per entry: the host loop's refusals as the least key entry * 4 + rule, max_transform, has_nan, bounded, thick, the counts of boxes and
 *                       of live (non-terminator) entries; meta = type | transform << 2 per entry; and the depth's differences: +1 at i, -1 at i + skip of box i
 *   scans               an exclusive scan over (difference, live) gives (depth, rank among the live entries) per entry: depth[i] = the boxes j < i with
 *                       j + skip_j >= i, which is what build_threaded's stack holds at entry i of a properly nested list
 *   k_derive_histogram  live entries per min(depth, 4096);  k_derive_threshold: the depth d* at which the min(4096, live) shallowest entries end, and how many
 *                       entries r of depth d* are among them.  (From depth d to d + 1 the array passes a box of depth d, so every depth below that of a live
 *                       entry has a live entry: the 4096 shallowest end below depth 4096.)
 *   k_derive_mark       (depth < d*, depth == d*) per live entry, scanned like the first pair: ranks by index on either side of the threshold
 *   k_derive_index      the threaded index of every entry but those below d*: 0 the shared terminator, 1 .. hot the hot set, the rest in the array's order;
 *                       the (at most 4095) entries below d* are listed in the array's order, and k_derive_hot_rank ranks them by (depth, index)
 *   k_derive_emit       both copies, row for row as build_threaded and build_lockstep write them
 *
 * Every decision is an integer one, so the copies are the host's bit for bit for every properly nested list.  An improperly nested list (a box that ends inside
 * another's range) can get other depths than the host's stack gives it, hence another storage order of the threaded copy; links, rows and walks are the same.
 * No kernel waits for another workgroup: every scan is a launch per level (a block's scan, the scan of the block totals, the add back), recursing on the block
 * totals, so any entry count flx_scene_upload takes (2^28 - 1) is covered.
 */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "flx_kernels.h"

namespace flx {

namespace {

constexpr uint32_t DB = 256;                       /* threads per workgroup, items per scan block */
constexpr uint32_t HOT_MAX = 4096;                 /* build_threaded's */
constexpr uint32_t BINS = HOT_MAX + 1;             /* depths 0 .. 4095 and "4096 or deeper" */
constexpr uint32_t BINS_PER_THREAD = 17;           /* 256 * 17 >= BINS */
constexpr uint32_t HIST_GRID = 256;

/* the record (DERIVE_RECORD_WORDS): see flx_kernels.h */
enum { REC_VERDICT = 0, REC_MAX_TRANSFORM, REC_HAS_NAN, REC_UNBOUNDED, REC_BOXES, REC_LIVE, REC_META0, REC_FLAT };
/* the threshold: d*, r, hot, entries below d* */
enum { HP_DEPTH = 0, HP_TAKE, HP_HOT, HP_BELOW };

struct Work {
  uint32_t *record, *hist, *base, *hp, *meta, *index;
  uint2 *below, *x, *y, *totals;
  size_t words;
};
Work layout(uint32_t n, uint32_t *w) {
  Work k;
  size_t at = 0;
  auto take = [&](size_t words) { uint32_t *p = w ? w + at : nullptr; at += (words + 3) & ~(size_t)3; return p; };      /* (16-byte steps) */
  k.record = take(DERIVE_RECORD_WORDS); k.hist = take(BINS);      /* (zeroed together) */
  k.base = take(BINS); k.hp = take(4);
  k.below = (uint2 *)take(HOT_MAX * 2);
  k.meta = take(n); k.index = take(n);
  k.x = (uint2 *)take((size_t)n * 2); k.y = (uint2 *)take((size_t)n * 2);
  k.totals = (uint2 *)take(scan_totals_items(n) * 2);
  k.words = at;
  return k;
}

__device__ __forceinline__ uint2 add2(uint2 a, uint2 b) { return make_uint2(a.x + b.x, a.y + b.y); }

/* exclusive prefix of v over the workgroup's DB threads (wrapping sums: the differences are signed) and the workgroup's total; lds[4]; every thread calls */
__device__ __forceinline__ uint2 blockExclusive(uint2 v, uint2 *lds, uint2 &total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint2 inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t ax = __shfl_up(inc.x, d), ay = __shfl_up(inc.y, d);
    if (lane >= (uint32_t)d) { inc.x += ax; inc.y += ay; }
  }
  __syncthreads();                                 /* (the last call's readers are done with lds) */
  if (lane == 63u) lds[wave] = inc;
  __syncthreads();
  uint2 before = make_uint2(0u, 0u);
  total = make_uint2(0u, 0u);
#pragma unroll
  for (uint32_t w = 0; w < DB / 64u; w++) {
    const uint2 t = lds[w];
    if (w < wave) before = add2(before, t);
    total = add2(total, t);
  }
  return make_uint2(inc.x - v.x + before.x, inc.y - v.y + before.y);
}

/* the host loop of flx_scene_upload, entry i (12 floats: g0 g1 g2): 0 transform number out of range, 1 skip count leaves the array, 2 type not 0, 1 or 2; 3 none */
__device__ __forceinline__ uint32_t ruleOf(uint32_t i, uint32_t n, float skip, float transform, float kind) {
  if (kind != 0.0f && !(transform >= 0.0f && transform < 1048576.0f)) return 0u;
  if (kind == 1.0f) return (!(skip >= 0.0f) || (double)i + (double)skip >= (double)n) ? 1u : 3u;
  return (kind != 0.0f && kind != 2.0f) ? 2u : 3u;
}

/* x zeroed, record zeroed.  record[REC_VERDICT] takes the max of ~key: 0 says no entry offends, else the least key is its complement. */
__global__ __launch_bounds__(DB) void k_derive_check(const float4 *__restrict__ geometry, uint32_t n, uint32_t *__restrict__ record, uint32_t *__restrict__ meta,
                                                     uint2 *__restrict__ x) {
  const uint32_t i = blockIdx.x * DB + threadIdx.x;
  uint32_t notKey = 0u, transform = 0u;
  bool nan = false, unbounded = false, flat = false, box = false, live = false;
  if (i < n) {
    const float4 g0 = geometry[(size_t)i * 3], g1 = geometry[(size_t)i * 3 + 1], g2 = geometry[(size_t)i * 3 + 2];
    const float kind = g2.z;
    const uint32_t rule = ruleOf(i, n, g1.z, g2.y, kind);
    if (rule < 3u) notKey = ~(i * 4u + rule);      /* (i < 2^28) */
    live = kind != 0.0f;
    box = kind == 1.0f;
    const bool transformOk = g2.y >= 0.0f && g2.y < 1048576.0f;
    if (live && transformOk) transform = (uint32_t)g2.y;
    const float w[9] = { g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w, g2.x };
    if (kind == 2.0f) {
#pragma unroll
      for (int k = 0; k < 9; k++) nan = nan || w[k] != w[k];
    }
    if (box) {
#pragma unroll
      for (int k = 0; k < 6; k++) unbounded = unbounded || !(fabsf(w[k]) <= FLX_FAST_BOX_BOUND);
      flat = !(w[0] < w[3] && w[1] < w[4] && w[2] < w[5]);      /* (flx_scene.hip: box_is_thick) */
    }
    const uint32_t m = !live ? 0u : (box ? 1u : 2u) | transform << 2;
    meta[i] = m;
    x[i].y = live ? 1u : 0u;                       /* (.x: the atomics below, other lanes') */
    if (i == 0u) record[REC_META0] = m;
    if (box && rule == 3u) {                       /* the box covers (i, i + skip]: i + skip < n */
      const uint32_t skip = (uint32_t)g1.z;
      if (skip > 0u) {
        atomicAdd(&x[i].x, 1u);
        atomicAdd(&x[i + skip].x, 0xffffffffu);
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    notKey = max(notKey, (uint32_t)__shfl_xor((int)notKey, d));
    transform = max(transform, (uint32_t)__shfl_xor((int)transform, d));
  }
  const bool anyNan = __any(nan), anyUnbounded = __any(unbounded), anyFlat = __any(flat);
  const uint32_t boxes = (uint32_t)__popcll(__ballot(box)), lives = (uint32_t)__popcll(__ballot(live));
  if ((threadIdx.x & 63u) == 0u) {
    if (notKey) atomicMax(&record[REC_VERDICT], notKey);
    if (transform) atomicMax(&record[REC_MAX_TRANSFORM], transform);
    if (anyNan) atomicOr(&record[REC_HAS_NAN], 1u);
    if (anyUnbounded) atomicOr(&record[REC_UNBOUNDED], 1u);
    if (anyFlat) atomicOr(&record[REC_FLAT], 1u);
    if (boxes) atomicAdd(&record[REC_BOXES], boxes);
    if (lives) atomicAdd(&record[REC_LIVE], lives);
  }
}

/* x[i] <- the exclusive prefix of x inside i's block of DB; totals[block] <- the block's sum */
__global__ __launch_bounds__(DB) void k_derive_scan_block(uint2 *__restrict__ x, uint32_t m, uint2 *__restrict__ totals) {
  __shared__ uint2 lds[DB / 64];
  const uint32_t i = blockIdx.x * DB + threadIdx.x;
  const uint2 v = i < m ? x[i] : make_uint2(0u, 0u);
  uint2 total;
  const uint2 before = blockExclusive(v, lds, total);
  if (i < m) x[i] = before;
  if (threadIdx.x == 0u) totals[blockIdx.x] = total;
}

/* x[i] += offsets[i's block] */
__global__ __launch_bounds__(DB) void k_derive_scan_add(uint2 *__restrict__ x, uint32_t m, const uint2 *__restrict__ offsets) {
  const uint32_t i = blockIdx.x * DB + threadIdx.x;
  if (i < m) x[i] = add2(x[i], offsets[blockIdx.x]);
}

/* hist[min(depth, HOT_MAX)] of the live entries; hist zeroed */
__global__ __launch_bounds__(DB) void k_derive_histogram(const uint2 *__restrict__ x, const uint32_t *__restrict__ meta, uint32_t n, uint32_t *__restrict__ hist) {
  __shared__ uint32_t bins[BINS];
  for (uint32_t b = threadIdx.x; b < BINS; b += DB) bins[b] = 0u;
  __syncthreads();
  for (uint32_t i = blockIdx.x * DB + threadIdx.x; i < n; i += gridDim.x * DB)
    if (meta[i] != 0u) atomicAdd(&bins[min(x[i].x, HOT_MAX)], 1u);
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < BINS; b += DB)
    if (bins[b]) atomicAdd(&hist[b], bins[b]);
}

/* one workgroup.  base[d] <- the live entries of depth < d; hp <- d*, r, hot, base[d*]: hot = min(HOT_MAX, live) entries are hot, those of depth < d* and the
 * first r by index of depth d* */
__global__ __launch_bounds__(DB) void k_derive_threshold(const uint32_t *__restrict__ hist, const uint32_t *__restrict__ record, uint32_t *__restrict__ base,
                                                         uint32_t *__restrict__ hp) {
  __shared__ uint2 lds[DB / 64];
  const uint32_t first = threadIdx.x * BINS_PER_THREAD;
  const uint32_t hot = min(record[REC_LIVE], HOT_MAX);
  uint32_t mine = 0u;
  for (uint32_t k = 0; k < BINS_PER_THREAD; k++) if (first + k < BINS) mine += hist[first + k];
  uint2 total;
  uint32_t before = blockExclusive(make_uint2(mine, 0u), lds, total).x;
  if (hot == 0u && threadIdx.x == 0u) { hp[HP_DEPTH] = 0u; hp[HP_TAKE] = 0u; hp[HP_HOT] = 0u; hp[HP_BELOW] = 0u; }
  for (uint32_t k = 0; k < BINS_PER_THREAD; k++) {
    const uint32_t d = first + k;
    if (d >= BINS) break;
    const uint32_t here = hist[d];
    base[d] = before;
    if (before < hot && before + here >= hot) { hp[HP_DEPTH] = d; hp[HP_TAKE] = hot - before; hp[HP_HOT] = hot; hp[HP_BELOW] = before; }
    before += here;
  }
}

__global__ __launch_bounds__(DB) void k_derive_mark(const uint2 *__restrict__ x, const uint32_t *__restrict__ meta, uint32_t n, const uint32_t *__restrict__ hp,
                                                    uint2 *__restrict__ y) {
  const uint32_t i = blockIdx.x * DB + threadIdx.x;
  if (i >= n) return;
  const uint32_t depth = x[i].x, dstar = hp[HP_DEPTH];
  const bool live = meta[i] != 0u;
  y[i] = make_uint2(live && depth < dstar ? 1u : 0u, live && depth == dstar ? 1u : 0u);
}

/* x: (depth, live entries before i), y: (live entries below d* before i, live entries of depth d* before i) */
__global__ __launch_bounds__(DB) void k_derive_index(const uint2 *__restrict__ x, const uint2 *__restrict__ y, const uint32_t *__restrict__ meta, uint32_t n,
                                                     const uint32_t *__restrict__ hp, uint32_t *__restrict__ index, uint2 *__restrict__ below) {
  const uint32_t i = blockIdx.x * DB + threadIdx.x;
  if (i >= n || meta[i] == 0u) return;             /* (no link names a terminator's own index) */
  const uint2 xi = x[i], yi = y[i];
  const uint32_t dstar = hp[HP_DEPTH], take = hp[HP_TAKE], hot = hp[HP_HOT], nBelow = hp[HP_BELOW];
  if (xi.x < dstar) { below[yi.x] = make_uint2(xi.x, i); return; }      /* (yi.x < nBelow <= HOT_MAX - 1) */
  const bool isHot = xi.x == dstar && yi.y < take;
  const uint32_t hotBefore = yi.x + min(yi.y, take);
  index[i] = isHot ? 1u + nBelow + yi.y : 1u + hot + (xi.y - hotBefore);
}

/* the entries below d*, listed in the array's order: by (depth, index) entry k stands behind base[depth] shallower ones and those of its depth listed before it */
__global__ __launch_bounds__(DB) void k_derive_hot_rank(const uint2 *__restrict__ below, const uint32_t *__restrict__ hp, const uint32_t *__restrict__ base,
                                                        uint32_t *__restrict__ index) {
  __shared__ uint32_t depths[HOT_MAX];
  const uint32_t count = min(hp[HP_BELOW], HOT_MAX);
  for (uint32_t k = threadIdx.x; k < count; k += DB) depths[k] = below[k].x;
  __syncthreads();
  const uint32_t k = blockIdx.x * DB + threadIdx.x;
  if (k >= count) return;
  const uint32_t d = depths[k];
  uint32_t same = 0u;
  for (uint32_t m = 0; m < k; m++) same += depths[m] == d ? 1u : 0u;
  index[below[k].y] = 1u + base[d] + same;
}

/* build_threaded's succ and build_lockstep's */
__device__ __forceinline__ uint32_t walkLink(uint64_t j, uint32_t fromTransform, uint32_t n, const uint32_t *meta, const uint32_t *index) {
  if (j >= n) return WALK_END;
  const uint32_t m = meta[j];
  if (m == 0u) return 0u;                          /* the shared terminator */
  return index[j] | (m & 3u) << LINK_KIND_SHIFT | ((m >> 2) != fromTransform ? LINK_XFORM : 0u);
}
__device__ __forceinline__ uint32_t fwdLink(uint64_t j, uint32_t n, uint32_t live, const uint32_t *meta, const uint2 *x) {
  if (j >= n) return WALK_END;
  return meta[j] == 0u ? live : x[j].y;
}

__global__ __launch_bounds__(DB) void k_derive_emit(const float4 *__restrict__ geometry, const uint32_t *__restrict__ meta, const uint2 *__restrict__ x,
                                                    const uint32_t *__restrict__ index, uint32_t n, uint32_t live, float4 *__restrict__ walk,
                                                    float4 *__restrict__ fwd) {
  const uint32_t i = blockIdx.x * DB + threadIdx.x;
  if (i >= n) return;
  if (i == 0u) {                                   /* the shared terminators: all zero */
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < 3; k++) { walk[k] = zero; fwd[(size_t)live * 3 + k] = zero; }
  }
  const uint32_t m = meta[i];
  if (m == 0u) return;
  const uint32_t transform = m >> 2;
  const float4 g0 = geometry[(size_t)i * 3], g1 = geometry[(size_t)i * 3 + 1];
  float4 *w = walk + (size_t)index[i] * 3, *f = fwd + (size_t)x[i].y * 3;
  const float mw = __uint_as_float(m), iw = __uint_as_float(i);
  if ((m & 3u) == 1u) {
    const uint64_t past = (uint64_t)i + 1u + (uint64_t)g1.z;
    w[0] = g0; f[0] = g0;
    w[1] = make_float4(g1.x, g1.y, 0.f, 0.f); f[1] = w[1];
    w[2] = make_float4(__uint_as_float(walkLink((uint64_t)i + 1u, transform, n, meta, index)), __uint_as_float(walkLink(past, transform, n, meta, index)), mw, iw);
    f[2] = make_float4(__uint_as_float(fwdLink((uint64_t)i + 1u, n, live, meta, x)), __uint_as_float(fwdLink(past, n, live, meta, x)), mw, iw);
  } else {                                         /* vertex a and the edges b - a, c - a */
    const float4 g2 = geometry[(size_t)i * 3 + 2];
    const float4 r0 = make_float4(g0.x, g0.y, g0.z, g0.w - g0.x), r1 = make_float4(g1.x - g0.y, g1.y - g0.z, g1.z - g0.x, g1.w - g0.y);
    const float e8 = g2.x - g0.z;
    w[0] = r0; f[0] = r0;
    w[1] = r1; f[1] = r1;
    w[2] = make_float4(e8, __uint_as_float(walkLink((uint64_t)i + 1u, transform, n, meta, index)), mw, iw);
    f[2] = make_float4(e8, __uint_as_float(fwdLink((uint64_t)i + 1u, n, live, meta, x)), mw, iw);
  }
}

/* words 6, 9 and 10 of every entry: flx_scene_update's h_entry_meta */
__global__ __launch_bounds__(DB) void k_entry_meta(const float4 *__restrict__ geometry, uint32_t n, uint32_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * DB + threadIdx.x;
  if (i >= n) return;
  const float4 g1 = geometry[(size_t)i * 3 + 1], g2 = geometry[(size_t)i * 3 + 2];
  out[(size_t)i * 3] = __float_as_uint(g1.z);
  out[(size_t)i * 3 + 1] = __float_as_uint(g2.y);
  out[(size_t)i * 3 + 2] = __float_as_uint(g2.z);
}

uint32_t blocksOf(size_t m) { return (uint32_t)((m + DB - 1) / DB); }

/* x[0 .. m) <- its exclusive prefix; totals: room for every level's block totals */
void exclusiveScan(uint2 *x, uint32_t m, uint2 *totals, hipStream_t stream) {
  const uint32_t nb = blocksOf(m);
  hipLaunchKernelGGL(k_derive_scan_block, dim3(nb), dim3(DB), 0, stream, x, m, totals);
  if (nb <= 1u) return;
  exclusiveScan(totals, nb, totals + ((nb + 1u) & ~1u), stream);
  hipLaunchKernelGGL(k_derive_scan_add, dim3(nb), dim3(DB), 0, stream, x, m, (const uint2 *)totals);
}

}  // namespace

/* every level's block totals, each level's at an even item, and two items beyond (a single block writes its total too) */
size_t scan_totals_items(uint32_t m) {
  size_t totals = 0;
  for (size_t k = m; k > 1; ) { k = (k + DB - 1) / DB; totals += (k + 1) & ~(size_t)1; }
  return totals + 2;
}
void launch_exclusive_scan(uint2 *x, uint32_t m, uint2 *totals, hipStream_t stream) { exclusiveScan(x, m, totals, stream); }

size_t derive_workspace_words(uint32_t n_entries) { return layout(n_entries, nullptr).words; }

hipError_t launch_derive_check(const float4 *geometry, uint32_t n_entries, uint32_t *work, hipStream_t stream) {
  const Work k = layout(n_entries, work);
  hipError_t e;
  if ((e = hipMemsetAsync(k.record, 0, (size_t)((char *)k.base - (char *)k.record), stream)) != hipSuccess) return e;      /* the record and the histogram */
  if ((e = hipMemsetAsync(k.x, 0, (size_t)n_entries * 8, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_derive_check, dim3(blocksOf(n_entries)), dim3(DB), 0, stream, geometry, n_entries, k.record, k.meta, k.x);
  return hipGetLastError();
}

void launch_derive_copies(const float4 *geometry, uint32_t n_entries, uint32_t live, uint32_t *work, float4 *walk, float4 *fwd, hipStream_t stream) {
  const Work k = layout(n_entries, work);
  const uint32_t nb = blocksOf(n_entries);
  exclusiveScan(k.x, n_entries, k.totals, stream);
  hipLaunchKernelGGL(k_derive_histogram, dim3(std::min(nb, HIST_GRID)), dim3(DB), 0, stream, (const uint2 *)k.x, (const uint32_t *)k.meta, n_entries, k.hist);
  hipLaunchKernelGGL(k_derive_threshold, dim3(1), dim3(DB), 0, stream, (const uint32_t *)k.hist, (const uint32_t *)k.record, k.base, k.hp);
  hipLaunchKernelGGL(k_derive_mark, dim3(nb), dim3(DB), 0, stream, (const uint2 *)k.x, (const uint32_t *)k.meta, n_entries, (const uint32_t *)k.hp, k.y);
  exclusiveScan(k.y, n_entries, k.totals, stream);
  hipLaunchKernelGGL(k_derive_index, dim3(nb), dim3(DB), 0, stream, (const uint2 *)k.x, (const uint2 *)k.y, (const uint32_t *)k.meta, n_entries,
                     (const uint32_t *)k.hp, k.index, k.below);
  hipLaunchKernelGGL(k_derive_hot_rank, dim3(HOT_MAX / DB), dim3(DB), 0, stream, (const uint2 *)k.below, (const uint32_t *)k.hp, (const uint32_t *)k.base, k.index);
  hipLaunchKernelGGL(k_derive_emit, dim3(nb), dim3(DB), 0, stream, geometry, (const uint32_t *)k.meta, (const uint2 *)k.x, (const uint32_t *)k.index, n_entries,
                     live, walk, fwd);
}

void launch_entry_meta(const float4 *geometry, uint32_t n_entries, uint32_t *out, hipStream_t stream) {
  if (n_entries) hipLaunchKernelGGL(k_entry_meta, dim3(blocksOf(n_entries)), dim3(DB), 0, stream, geometry, n_entries, out);
}

}  // namespace flx
