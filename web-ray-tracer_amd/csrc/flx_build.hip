/*
 * flx_build.hip — flx_tree_build_device / flx_tree_emit_device's kernels: the box tree flx_mesh.hip's split / updateBoundings / emit build on the host (the
 * reference's generateBVH, modules/scene.js:62-154, 157-187, 190-316), built from triangle rows that are in device memory: the same rows in the same order.
 *
 * The host recursion, level by level.  A node owns a range [first, first + count) of a permutation of the triangles; its children are a STABLE partition of that
 * range into (up to) three buckets, so a range never moves once its node exists and a level is one pass over the positions and one over the level's nodes:
 *   k_tree_nodes     a lane per node of the level: its bounding — the first triangle's own, joined with every later one's widened by NODE_BIAS: min / max are
 *                    monotone under "- bias" / "+ bias", so the later ones come as ONE min / max over float keys (k_tree_bounds) — the centre, which axes
 *                    have room; a node of <= 4 triangles, or beyond the depth limit, or without room on any axis, is a leaf
 *   k_tree_count     a lane per position: the triangles that fit neither half, per axis with room (integer atomics, a wave that lies in one node adds once)
 *   k_tree_decide    a lane per node: the axis with the fewest of them, the LAST among equals
 *   k_tree_bucket    a lane per position: 0 fits the half whose min is the centre, 1 the half whose max is the centre, 2 neither; the flags (bucket 0, bucket 1)
 *   scan             the exclusive scan of the flags (flx_derive.hip's: a launch per level of block totals, no workgroup waits for another); minus its value at
 *                    the node's start it is a triangle's rank in its bucket; bucket 2's rank is what is left of the position's offset in the node
 *   k_tree_kids      a lane per node: the bucket sizes, the number of non-empty ones; scanned: where the node's children stand among the next level's nodes
 *   -- the host waits here for the number of children (none: the tree is done) and makes room for them --
 *   k_tree_children  a lane per node: its children's ranges, r (below), and open[first] += 1
 *   k_tree_scatter   a lane per position: the permutation and each position's node for the next level
 *   k_tree_bounds    a lane per position: min / max keys of a node's triangles but its first (the refit's ordered keys: integer atomics; a wave in one node reduces first)
 * Entry indices need no walk of the tree.  open[p] = the nodes whose range starts at p.  In the depth-first order of the flatten, the triangle at final position p
 * stands behind p triangles and every node that starts at or before p: entry p + inclusive_scan(open)[p].  A node with r ancestors that start where it starts
 * stands behind `first` triangles, the nodes that start before `first`, and those r: entry first + exclusive_scan(open)[first] + r; beneath it lie its `count`
 * triangles and the nodes that start inside its range but itself and those r ancestors.
 *
 * Every decision compares doubles that are sums and halves of floats (uncontracted: -ffp-contract=off), a NaN is refused before, and no decision depends on the
 * sign of a zero: the tree is the host's.  Memory: O(triangles + nodes); the node arrays grow by doubling (chains of single-child nodes are legal, so the
 * number of nodes is not known before).  A build waits once per level of the tree.
 */
#include <hip/hip_runtime.h>

#include "flx_kernels.h"
#include "flx_kernel_util.h"

namespace flx {

namespace {

constexpr uint32_t TB = 256;                       /* threads per workgroup */
constexpr uint32_t NONE = 0xffffffffu;             /* a position whose node takes part in no further level */
constexpr uint32_t LEAF = 3u;                      /* a node's state where it is not an axis */
constexpr uint32_t LEAF_MAX = 4u;                  /* scene.js:6 */
constexpr double NODE_BIAS = 0.00152587890625;     /* scene.js:159 (100 * 2^-16) */
constexpr double MIN_WIDTH = 1.0 / 256.0;          /* scene.js:84 */

__device__ __forceinline__ float lower(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float upper(float a, float b) { return b > a ? b : a; }

/* The rows as flx_tree_build_device refuses them — verdict[0] (~0 before) takes the least row * 4 + rule: 0 word 10 is not 2, 1 word 9 differs from row 0's or is
 * no whole number in [0, 2^20), 2 a vertex is not finite — and what the levels start from: every triangle's bounds, the identity permutation, the root. */
__global__ __launch_bounds__(TB) void k_tree_check(const float4 *__restrict__ rows, uint32_t n, uint32_t *__restrict__ verdict, float2 *__restrict__ tbox,
                                                   uint32_t *__restrict__ perm, uint32_t *__restrict__ owner, uint4 *__restrict__ node, uint32_t *__restrict__ keys,
                                                   uint32_t *__restrict__ open) {
  const uint32_t i = blockIdx.x * TB + threadIdx.x;
  uint32_t key = 0xffffffffu;
  if (i < n) {
    const float4 g0 = rows[(size_t)i * 3], g1 = rows[(size_t)i * 3 + 1], g2 = rows[(size_t)i * 3 + 2];
    const float transform0 = rows[2].y;
    uint32_t rule = 3u;
    const float w[9] = { g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w, g2.x };
#pragma unroll
    for (int k = 0; k < 9; k++) if (!(fabsf(w[k]) < __builtin_inff())) rule = 2u;
    const bool whole = g2.y >= 0.0f && g2.y < 1048576.0f && __float_as_uint((float)(uint32_t)g2.y) == __float_as_uint(g2.y);      /* (not -0, no fraction: the boxes carry these bits) */
    if (!whole || g2.y != transform0) rule = 1u;
    if (g2.z != 2.0f) rule = 0u;
    if (rule < 3u) key = i * 4u + rule;            /* (n <= 2^24) */
    tbox[(size_t)i * 3] = make_float2(lower(lower(w[0], w[3]), w[6]), upper(upper(w[0], w[3]), w[6]));
    tbox[(size_t)i * 3 + 1] = make_float2(lower(lower(w[1], w[4]), w[7]), upper(upper(w[1], w[4]), w[7]));
    tbox[(size_t)i * 3 + 2] = make_float2(lower(lower(w[2], w[5]), w[8]), upper(upper(w[2], w[5]), w[8]));
    perm[i] = i;
    owner[i] = n > LEAF_MAX ? 0u : NONE;
    if (i == 0u) {
      node[0] = make_uint4(0u, n, 0u, LEAF);
#pragma unroll
      for (int c = 0; c < 3; c++) { keys[c] = KEY_NONE_LO; keys[3 + c] = KEY_NONE_HI; }
      open[0] = 1u;                                /* (zeroed before the launch) */
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, d));
  if ((threadIdx.x & 63u) == 0u && key != 0xffffffffu) atomicMin(&verdict[0], key);
}

/* keys[node] <- min / max over the node's triangles but the one at its first position.  A wave whose lanes all stand in one node reduces before lane 0 adds. */
__global__ __launch_bounds__(TB) void k_tree_bounds(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ owner, const uint4 *__restrict__ node,
                                                    const float2 *__restrict__ tbox, uint32_t n, uint32_t *__restrict__ keys) {
  const uint32_t p = blockIdx.x * TB + threadIdx.x;
  const uint32_t c = p < n ? owner[p] : NONE;
  uint32_t k[6] = { KEY_NONE_LO, KEY_NONE_LO, KEY_NONE_LO, KEY_NONE_HI, KEY_NONE_HI, KEY_NONE_HI };
  const bool counts = c != NONE && p != node[c].x;
  if (counts) {
    const size_t t = perm[p];
#pragma unroll
    for (int a = 0; a < 3; a++) { const float2 b = tbox[t * 3 + a]; k[a] = keyOf(b.x); k[3 + a] = keyOf(b.y); }
  }
  const uint32_t c0 = (uint32_t)__shfl((int)c, 0);
  if (__all(c == c0)) {
    if (c0 == NONE) return;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
      for (int a = 0; a < 3; a++) {
        k[a] = min(k[a], (uint32_t)__shfl_xor((int)k[a], d));
        k[3 + a] = max(k[3 + a], (uint32_t)__shfl_xor((int)k[3 + a], d));
      }
    }
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
      for (int a = 0; a < 3; a++) { atomicMin(&keys[(size_t)c0 * 6 + a], k[a]); atomicMax(&keys[(size_t)c0 * 6 + 3 + a], k[3 + a]); }
    }
  } else if (counts) {
#pragma unroll
    for (int a = 0; a < 3; a++) { atomicMin(&keys[(size_t)c * 6 + a], k[a]); atomicMax(&keys[(size_t)c * 6 + 3 + a], k[3 + a]); }
  }
}

/* nodes [base, base + m) of the level `depth`: centre <- the bounding's; cnt <- (0, 0, 0, the axes with room), no axis where the node is a leaf for its size or depth */
__global__ __launch_bounds__(TB) void k_tree_nodes(const uint4 *__restrict__ node, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ perm,
                                                   const float2 *__restrict__ tbox, uint32_t base, uint32_t m, double depth, double maxDepth,
                                                   double *__restrict__ centre, uint4 *__restrict__ cnt) {
  const uint32_t q = blockIdx.x * TB + threadIdx.x;
  if (q >= m) return;
  const size_t j = (size_t)base + q;
  const uint4 nd = node[j];
  uint32_t mask = 0u;
  if (nd.y > LEAF_MAX && !(depth > maxDepth)) {
    const size_t t0 = perm[nd.x];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float2 b = tbox[t0 * 3 + a];
      double lo = (double)b.x, hi = (double)b.y;
      const double olo = (double)floatOf(keys[j * 6 + a]) - NODE_BIAS, ohi = (double)floatOf(keys[j * 6 + 3 + a]) + NODE_BIAS;      /* (count > 4: there are later ones) */
      lo = olo < lo ? olo : lo;
      hi = ohi > hi ? ohi : hi;
      const double c = (lo + hi) / 2.0;
      const double above = hi - c, below = c - lo;
      const double room = below < above ? below : above;
      centre[j * 3 + a] = c;
      if (room > MIN_WIDTH) mask |= 1u << a;
    }
  }
  cnt[j] = make_uint4(0u, 0u, 0u, mask);
}

/* A triangle fits the half above the centre where centre <= its min and the half below where centre >= its max: the node's bounding holds every triangle of the
 * node on all six sides (a min of values none of which lies above the triangle's own), so fitsInBound's other five comparisons are true. */
__global__ __launch_bounds__(TB) void k_tree_count(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ owner, const float2 *__restrict__ tbox,
                                                   const double *__restrict__ centre, uint32_t n, uint4 *__restrict__ cnt) {
  const uint32_t p = blockIdx.x * TB + threadIdx.x;
  const uint32_t j = p < n ? owner[p] : NONE;
  const uint32_t mask = j != NONE ? cnt[j].w : 0u;
  bool straddles[3] = { false, false, false };
  if (mask) {
    const size_t t = perm[p];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      if (mask >> a & 1u) {
        const float2 b = tbox[t * 3 + a];
        const double c = centre[(size_t)j * 3 + a];
        straddles[a] = !(c <= (double)b.x) && !(c >= (double)b.y);
      }
    }
  }
  const uint32_t j0 = (uint32_t)__shfl((int)j, 0);
  const bool oneNode = __all(j == j0);
  uint32_t *const mine = (uint32_t *)&cnt[j != NONE ? j : 0u];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (oneNode) {
      const uint32_t sum = (uint32_t)__popcll(__ballot(straddles[a]));
      if (sum && (threadIdx.x & 63u) == 0u) atomicAdd(mine + a, sum);
    } else if (straddles[a]) {
      atomicAdd(mine + a, 1u);
    }
  }
}

/* node.w <- the axis: the fewest straddlers among the axes with room, the last among equals (scene.js:120: "fewest >= n") */
__global__ __launch_bounds__(TB) void k_tree_decide(uint4 *__restrict__ node, const uint4 *__restrict__ cnt, uint32_t base, uint32_t m) {
  const uint32_t q = blockIdx.x * TB + threadIdx.x;
  if (q >= m) return;
  const size_t j = (size_t)base + q;
  const uint4 c = cnt[j];
  const uint32_t straddlers[3] = { c.x, c.y, c.z };
  uint32_t axis = LEAF, fewest = 0u;
#pragma unroll
  for (uint32_t a = 0; a < 3; a++)
    if ((c.w >> a & 1u) && (axis == LEAF || fewest >= straddlers[a])) { axis = a; fewest = straddlers[a]; }
  uint4 nd = node[j];
  nd.w = axis;
  node[j] = nd;
}

/* positions 0 .. n (n: the scan's last item): bucket, and the flags (bucket 0, bucket 1) */
__global__ __launch_bounds__(TB) void k_tree_bucket(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ owner, const uint4 *__restrict__ node,
                                                    const float2 *__restrict__ tbox, const double *__restrict__ centre, uint32_t n, uint32_t *__restrict__ bucket,
                                                    uint2 *__restrict__ x) {
  const uint32_t p = blockIdx.x * TB + threadIdx.x;
  if (p > n) return;
  uint32_t b = LEAF;
  const uint32_t j = p < n ? owner[p] : NONE;
  if (j != NONE) {
    const uint32_t axis = node[j].w;
    if (axis != LEAF) {
      const float2 t = tbox[(size_t)perm[p] * 3 + axis];
      const double c = centre[(size_t)j * 3 + axis];
      b = c <= (double)t.x ? 0u : (c >= (double)t.y ? 1u : 2u);
    }
  }
  x[p] = make_uint2(b == 0u ? 1u : 0u, b == 1u ? 1u : 0u);
  if (p < n) bucket[p] = b;
}

/* x scanned.  cnt <- (bucket sizes, non-empty buckets); y[q] <- (non-empty buckets, 0) for the scan over the level; y[m] <- 0 */
__global__ __launch_bounds__(TB) void k_tree_kids(const uint4 *__restrict__ node, const uint2 *__restrict__ x, uint32_t base, uint32_t m, uint4 *__restrict__ cnt,
                                                  uint2 *__restrict__ y) {
  const uint32_t q = blockIdx.x * TB + threadIdx.x;
  if (q > m) return;
  uint32_t kids = 0u;
  if (q < m) {
    const size_t j = (size_t)base + q;
    const uint4 nd = node[j];
    uint4 c = make_uint4(0u, 0u, 0u, 0u);
    if (nd.w != LEAF) {
      const uint2 f = x[nd.x], e = x[nd.x + nd.y];
      c.x = e.x - f.x; c.y = e.y - f.y; c.z = nd.y - c.x - c.y;
      c.w = kids = (c.x ? 1u : 0u) + (c.y ? 1u : 0u) + (c.z ? 1u : 0u);
    }
    cnt[j] = c;
  }
  y[q] = make_uint2(kids, 0u);
}

/* y scanned: the children of node base + q are the nodes base + m + y[q].x ..  At most one node of a level starts at a position: open needs no atomic. */
__global__ __launch_bounds__(TB) void k_tree_children(uint4 *__restrict__ node, const uint4 *__restrict__ cnt, const uint2 *__restrict__ y, uint32_t base, uint32_t m,
                                                      uint32_t *__restrict__ keys, uint32_t *__restrict__ open) {
  const uint32_t q = blockIdx.x * TB + threadIdx.x;
  if (q >= m) return;
  const size_t j = (size_t)base + q;
  const uint4 c = cnt[j];
  if (c.w == 0u) return;
  const uint4 nd = node[j];
  const uint32_t size[3] = { c.x, c.y, c.z };
  size_t child = (size_t)base + m + y[q].x;
  uint32_t first = nd.x;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (size[k] == 0u) continue;
    node[child] = make_uint4(first, size[k], first == nd.x ? nd.z + 1u : 0u, LEAF);
#pragma unroll
    for (int a = 0; a < 3; a++) { keys[child * 6 + a] = KEY_NONE_LO; keys[child * 6 + 3 + a] = KEY_NONE_HI; }
    open[first] += 1u;
    first += size[k];
    child++;
  }
}

/* the stable partition: a triangle goes behind the buckets before its own and the triangles of its bucket that stood before it in the node */
__global__ __launch_bounds__(TB) void k_tree_scatter(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ owner, const uint4 *__restrict__ node,
                                                     const uint4 *__restrict__ cnt, const uint2 *__restrict__ x, const uint2 *__restrict__ y,
                                                     const uint32_t *__restrict__ bucket, uint32_t base, uint32_t m, uint32_t n, uint32_t *__restrict__ permOut,
                                                     uint32_t *__restrict__ ownerOut) {
  const uint32_t p = blockIdx.x * TB + threadIdx.x;
  if (p >= n) return;
  const uint32_t j = owner[p], b = bucket[p];
  if (j == NONE || b == LEAF) { permOut[p] = perm[p]; ownerOut[p] = NONE; return; }
  const uint4 nd = node[j], c = cnt[j];
  const uint2 f = x[nd.x], mine = x[p];
  const uint32_t r0 = mine.x - f.x, r1 = mine.y - f.y, r2 = (p - nd.x) - r0 - r1;
  const uint32_t to = nd.x + (b == 0u ? r0 : b == 1u ? c.x + r1 : c.x + c.y + r2);
  const uint32_t size = b == 0u ? c.x : b == 1u ? c.y : c.z;
  const uint32_t child = base + m + y[j - base].x + (b == 0u ? 0u : (c.x ? 1u : 0u) + (b == 2u && c.y ? 1u : 0u));
  permOut[to] = perm[p];
  ownerOut[to] = size > LEAF_MAX ? child : NONE;      /* (a node of <= 4 is a leaf: nobody asks for its bounding) */
}

/* open -> the scan's items, positions 0 .. n */
__global__ __launch_bounds__(TB) void k_tree_open(const uint32_t *__restrict__ open, uint32_t n, uint2 *__restrict__ x) {
  const uint32_t p = blockIdx.x * TB + threadIdx.x;
  if (p <= n) x[p] = make_uint2(p < n ? open[p] : 0u, 0u);
}

/* x: open's exclusive scan.  entry[p] <- the entry of the triangle at position p; node[j] <- (its entry, the entries beneath it, .., ..) */
__global__ __launch_bounds__(TB) void k_tree_index(const uint2 *__restrict__ x, const uint32_t *__restrict__ open, uint32_t n, uint32_t nodes, uint32_t *__restrict__ entry,
                                                   uint4 *__restrict__ node) {
  const uint32_t i = blockIdx.x * TB + threadIdx.x;
  if (i < n) entry[i] = i + x[i].x + open[i];
  if (i < nodes) {
    const uint4 nd = node[i];
    const uint32_t before = x[nd.x].x;
    node[i] = make_uint4(nd.x + before + nd.z, nd.y + (x[nd.x + nd.y].x - before) - nd.z - 1u, nd.x, nd.y);
  }
}

/* The block's rows, a lane per 16 bytes: 10 per triangle (3 of its geometry row, 7 of its attribute row: zeros without attributes), then 10 per node: the box row
 * (words 0..5 are the refit's) and its attribute row of zeros.  ids[k] <- the entry of the k-th triangle in emission order. */
__global__ __launch_bounds__(TB) void k_tree_emit(const float4 *__restrict__ rows, const float4 *__restrict__ attributes, const uint32_t *__restrict__ perm,
                                                  const uint32_t *__restrict__ entry, const uint4 *__restrict__ node, uint32_t n, uint32_t nodes, float transform,
                                                  float4 *__restrict__ geometry, float4 *__restrict__ attributesOut, int32_t *__restrict__ ids) {
  const uint32_t q = blockIdx.x * TB + threadIdx.x;      /* (10 * (n + nodes) < 2^32: the entries are < 2^28) */
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  if (q < n * 10u) {
    const uint32_t p = q / 10u, part = q - p * 10u;
    const size_t t = perm[p], e = entry[p];
    if (part < 3u) geometry[e * 3 + part] = rows[t * 3 + part];
    else attributesOut[e * 7 + (part - 3u)] = attributes ? attributes[t * 7 + (part - 3u)] : zero;
    if (part == 0u) ids[p] = (int32_t)e;
  } else if (q - n * 10u < nodes * 10u) {
    const uint32_t j = (q - n * 10u) / 10u, part = (q - n * 10u) - j * 10u;
    const uint4 nd = node[j];
    const size_t e = nd.x;
    if (part == 0u) geometry[e * 3] = zero;
    else if (part == 1u) geometry[e * 3 + 1] = make_float4(0.f, 0.f, (float)nd.y, 0.f);
    else if (part == 2u) geometry[e * 3 + 2] = make_float4(0.f, transform, 1.0f, 0.f);
    else attributesOut[e * 7 + (part - 3u)] = zero;
  }
}

uint32_t blocksOf(size_t items) { return (uint32_t)((items + TB - 1) / TB); }

}  // namespace

void launch_tree_check(const float4 *rows, uint32_t n, uint32_t *verdict, const TreeArrays &t, hipStream_t stream) {
  hipLaunchKernelGGL(k_tree_check, dim3(blocksOf(n)), dim3(TB), 0, stream, rows, n, verdict, t.tbox, t.perm, t.owner, t.node, t.keys, t.open);
  hipLaunchKernelGGL(k_tree_bounds, dim3(blocksOf(n)), dim3(TB), 0, stream, (const uint32_t *)t.perm, (const uint32_t *)t.owner, (const uint4 *)t.node,
                     (const float2 *)t.tbox, n, t.keys);
}

void launch_tree_level(const TreeArrays &t, uint32_t n, uint32_t base, uint32_t m, uint32_t depth, double maxDepth, hipStream_t stream) {
  hipLaunchKernelGGL(k_tree_nodes, dim3(blocksOf(m)), dim3(TB), 0, stream, (const uint4 *)t.node, (const uint32_t *)t.keys, (const uint32_t *)t.perm,
                     (const float2 *)t.tbox, base, m, (double)depth, maxDepth, t.centre, t.cnt);
  hipLaunchKernelGGL(k_tree_count, dim3(blocksOf(n)), dim3(TB), 0, stream, (const uint32_t *)t.perm, (const uint32_t *)t.owner, (const float2 *)t.tbox,
                     (const double *)t.centre, n, t.cnt);
  hipLaunchKernelGGL(k_tree_decide, dim3(blocksOf(m)), dim3(TB), 0, stream, t.node, (const uint4 *)t.cnt, base, m);
  hipLaunchKernelGGL(k_tree_bucket, dim3(blocksOf((size_t)n + 1)), dim3(TB), 0, stream, (const uint32_t *)t.perm, (const uint32_t *)t.owner, (const uint4 *)t.node,
                     (const float2 *)t.tbox, (const double *)t.centre, n, t.bucket, t.x);
  launch_exclusive_scan(t.x, n + 1u, t.totals, stream);
  hipLaunchKernelGGL(k_tree_kids, dim3(blocksOf((size_t)m + 1)), dim3(TB), 0, stream, (const uint4 *)t.node, (const uint2 *)t.x, base, m, t.cnt, t.y);
  launch_exclusive_scan(t.y, m + 1u, t.totals, stream);
}

void launch_tree_children(const TreeArrays &t, uint32_t n, uint32_t base, uint32_t m, hipStream_t stream) {
  hipLaunchKernelGGL(k_tree_children, dim3(blocksOf(m)), dim3(TB), 0, stream, t.node, (const uint4 *)t.cnt, (const uint2 *)t.y, base, m, t.keys, t.open);
  hipLaunchKernelGGL(k_tree_scatter, dim3(blocksOf(n)), dim3(TB), 0, stream, (const uint32_t *)t.perm, (const uint32_t *)t.owner, (const uint4 *)t.node,
                     (const uint4 *)t.cnt, (const uint2 *)t.x, (const uint2 *)t.y, (const uint32_t *)t.bucket, base, m, n, t.permNext, t.ownerNext);
  hipLaunchKernelGGL(k_tree_bounds, dim3(blocksOf(n)), dim3(TB), 0, stream, (const uint32_t *)t.permNext, (const uint32_t *)t.ownerNext, (const uint4 *)t.node,
                     (const float2 *)t.tbox, n, t.keys);
}

void launch_tree_index(const TreeArrays &t, uint32_t n, uint32_t nodes, hipStream_t stream) {
  hipLaunchKernelGGL(k_tree_open, dim3(blocksOf((size_t)n + 1)), dim3(TB), 0, stream, (const uint32_t *)t.open, n, t.x);
  launch_exclusive_scan(t.x, n + 1u, t.totals, stream);
  hipLaunchKernelGGL(k_tree_index, dim3(blocksOf(n > nodes ? n : nodes)), dim3(TB), 0, stream, (const uint2 *)t.x, (const uint32_t *)t.open, n, nodes, t.entry, t.node);
}

void launch_tree_emit(const float4 *rows, const float4 *attributes, const TreeArrays &t, uint32_t n, uint32_t nodes, float transform, float4 *geometry,
                      float4 *attributesOut, int32_t *ids, hipStream_t stream) {
  hipLaunchKernelGGL(k_tree_emit, dim3(blocksOf(((size_t)n + nodes) * 10)), dim3(TB), 0, stream, rows, attributes, (const uint32_t *)t.perm, (const uint32_t *)t.entry,
                     (const uint4 *)t.node, n, nodes, transform, geometry, attributesOut, ids);
}

}  // namespace flx
