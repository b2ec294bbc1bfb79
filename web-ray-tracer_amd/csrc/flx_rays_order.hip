/* flx_rays_order.hip — a slab's rays in first-hit order (include/flexlight_hip_debug.h, "ray queries": flx_rays_trace_ordered[_device]; the key is
 * include/flx_ray_key.h's, the text the tests' CPU reference compiles too).
 *
 * Between a slab's first hits and its paths kernel (flx_rays_trace.hip), on the context's stream:
 *   1. k_hit_bounds: the box around the slab's live hit points, six words.  A lane reduces its rays, the wave its lanes (shuffles), the workgroup its waves (LDS),
 *      and ONE atomicMin / atomicMax per workgroup and axis finishes on flx_ray_key_map's integers — a total order, so the result cannot depend on who came first.
 *      The six words are set in stream order in front of every slab: bytes of 0xFF for the minima, of 0x00 for the maxima (no float maps to either).
 *   2. k_hit_keys: a lane per ray, flx_ray_key_of against the bounds; a workgroup adds its live rays to the slab's count with one atomic.
 *   3. a stable LSD radix sort of (key, position): 32-bit keys, four passes of 8 bits, three launches a pass —
 *      k_sort_count:   a workgroup takes ORDER_T consecutive items and writes its 256 digit counts to the pass's table, DIGIT-MAJOR: table[digit * groups + group];
 *      k_sort_scan:    the exclusive scan of that table in place.  Digit-major, the scanned word IS the place of a workgroup's first item of a digit: every item of
 *                      a smaller digit and every item of the same digit in an earlier workgroup lies in front of it;
 *      k_sort_scatter: the workgroup's items again.  An item's place is table[digit][group] + the items of its digit in front of it within the workgroup: those of
 *                      earlier waves (four per-wave counts in LDS, added up by the lane that owns the digit), of earlier rounds of its own wave (the wave's running
 *                      count, kept by the digit's first lane of the round) and of lower lanes in its round (ballots over the digit's eight bits give the lanes
 *                      that share the digit).  Waves take consecutive runs of 512 items, rounds consecutive runs of 64, lanes consecutive items: "in front of"
 *                      is the input's order, so equal keys keep it — the sort is STABLE, and NO ATOMIC DECIDES A PLACE (k_sort_count's LDS atomics add up counts,
 *                      which no order can change).
 *      A workgroup's items change from pass to pass, so its counts are made pass by pass; the first pass takes an item's index for its position, which saves a
 *      launch that writes 0 .. m - 1.
 *   The scan: a slab has at most 2^21 rays, so a pass's table has at most 256 * ceil(2^21 / ORDER_T) = 2^18 words.  ONE workgroup of 1024 lanes walks it in tiles
 *   of 4096 words — a lane loads and stores 16 bytes, a wave scans by shuffles, the sixteen wave sums go through LDS, the tile's total is carried into the next —:
 *   at most 64 tiles.  The sums are at most 2^21: nothing wraps.
 * Scratch (flx_context.h): two key and two position buffers of a slab's rays, the table, sixteen control words; 16 bytes a ray and at most 1 MB of table.  The
 * paths kernel reads the order through d_order_pos[0] (four passes: 0 -> 1 -> 0 -> 1 -> 0). */
#include <string>

#include "flx_context.h"
#include "flx_ray_key.h"
#include "flx_ray_order_args.h"
#include "flx_rays_host.h"

namespace flx {

constexpr uint32_t ORDER_T = FLX_ORDER_SORT_ITEMS;     /* T: the items a sort workgroup takes */
constexpr uint32_t ORDER_THREADS = 256u;               /* four waves */
constexpr uint32_t ORDER_WAVES = ORDER_THREADS / 64u;
constexpr uint32_t ORDER_ROUNDS = ORDER_T / ORDER_THREADS;      /* rounds of 64 consecutive items a wave takes: 8 */
constexpr uint32_t ORDER_WAVE_ITEMS = ORDER_ROUNDS * 64u;       /* 512 */
constexpr uint32_t ORDER_PASSES = 4u;
constexpr uint32_t ORDER_SCAN_THREADS = 1024u;
constexpr uint32_t ORDER_BOUNDS_GROUPS = 1024u;        /* most workgroups of k_hit_bounds: a lane then takes up to 8 rays of a full slab */
static_assert(ORDER_ROUNDS * ORDER_THREADS == ORDER_T && ORDER_WAVES == 4u, "a workgroup's waves and rounds cover its items");

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, off); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, off); v = o > v ? o : v; }
  return v;
}

/* ray i's hit point; true for a live ray */
__device__ __forceinline__ bool load_hit_point(const float4 *__restrict__ rays, const float4 *__restrict__ hits, uint32_t i, float ray[8], float hit[4], float p[3]) {
  const float4 q0 = rays[(size_t)i * 2u], q1 = rays[(size_t)i * 2u + 1u], h = hits[(size_t)i * 2u];
  ray[0] = q0.x; ray[1] = q0.y; ray[2] = q0.z; ray[3] = q0.w; ray[4] = q1.x; ray[5] = q1.y; ray[6] = q1.z; ray[7] = q1.w;
  hit[0] = h.x; hit[1] = h.y; hit[2] = h.z; hit[3] = h.w;
  return flx_ray_key_hit_point(ray, hit, p) != 0;
}

/* ctl[0..2] <- min, ctl[3..5] <- max over the live rays' hit points, mapped; ctl was set to 0xFF.. / 0x00.. in front of the launch */
__global__ __launch_bounds__(ORDER_THREADS) void k_hit_bounds(const float4 *__restrict__ rays, const float4 *__restrict__ hits, uint32_t m, uint32_t *__restrict__ ctl) {
  __shared__ uint32_t part[ORDER_WAVES][6];
  uint32_t lo[3] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu }, hi[3] = { 0u, 0u, 0u };
  for (uint32_t i = blockIdx.x * ORDER_THREADS + threadIdx.x; i < m; i += gridDim.x * ORDER_THREADS) {      /* m <= 2^21, the grid's lanes <= 2^18: no wrap */
    float ray[8], hit[4], p[3];
    if (load_hit_point(rays, hits, i, ray, hit, p)) {
      for (int k = 0; k < 3; k++) {
        const uint32_t v = flx_ray_key_map(flx_ray_key_bits(p[k]));
        lo[k] = v < lo[k] ? v : lo[k];
        hi[k] = v > hi[k] ? v : hi[k];
      }
    }
  }
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (int k = 0; k < 3; k++) {
    const uint32_t a = wave_min(lo[k]), b = wave_max(hi[k]);
    if (lane == 0) { part[wave][k] = a; part[wave][3 + k] = b; }
  }
  __syncthreads();
  if (threadIdx.x < 6u) {
    const uint32_t k = threadIdx.x;
    uint32_t v = part[0][k];
    for (uint32_t w = 1; w < ORDER_WAVES; w++) { const uint32_t o = part[w][k]; v = k < 3u ? (o < v ? o : v) : (o > v ? o : v); }
    if (k < 3u) atomicMin(ctl + k, v); else atomicMax(ctl + k, v);
  }
}

/* keys[i] <- ray i's key against the bounds in ctl[0..5]; ctl[6] += the live rays */
__global__ __launch_bounds__(ORDER_THREADS) void k_hit_keys(const float4 *__restrict__ rays, const float4 *__restrict__ hits, uint32_t m, uint32_t *__restrict__ ctl,
                                                            uint32_t *__restrict__ keys) {
  __shared__ uint32_t liveOf[ORDER_WAVES];
  const uint32_t i = blockIdx.x * ORDER_THREADS + threadIdx.x;
  float bounds[6];
  for (int k = 0; k < 6; k++) bounds[k] = flx_ray_key_float(flx_ray_key_unmap(ctl[k]));
  uint32_t key = FLX_RAY_KEY_DEAD;
  if (i < m) {
    const float4 q0 = rays[(size_t)i * 2u], q1 = rays[(size_t)i * 2u + 1u], h = hits[(size_t)i * 2u];
    const float ray[8] = { q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w }, hit[4] = { h.x, h.y, h.z, h.w };
    key = flx_ray_key_of(ray, hit, bounds);
    keys[i] = key;
  }
  const uint32_t live = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(key != FLX_RAY_KEY_DEAD));
  if ((threadIdx.x & 63u) == 0u) liveOf[threadIdx.x >> 6] = live;
  __syncthreads();
  if (threadIdx.x == 0u) {
    uint32_t all = 0;
    for (uint32_t w = 0; w < ORDER_WAVES; w++) all += liveOf[w];
    if (all != 0u) atomicAdd(ctl + 6, all);
  }
}

/* table[digit * groups + group] <- how many of the workgroup's items have the digit */
__global__ __launch_bounds__(ORDER_THREADS) void k_sort_count(const uint32_t *__restrict__ keys, uint32_t m, uint32_t shift, uint32_t groups, uint32_t *__restrict__ table) {
  __shared__ uint32_t hist[256];
  hist[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t first = blockIdx.x * ORDER_T;
  for (uint32_t r = 0; r < ORDER_ROUNDS; r++) {
    const uint32_t idx = first + r * ORDER_THREADS + threadIdx.x;
    if (idx < m) atomicAdd(&hist[(keys[idx] >> shift) & 255u], 1u);
  }
  __syncthreads();
  table[(size_t)threadIdx.x * groups + blockIdx.x] = hist[threadIdx.x];
}

/* the exclusive scan of table[0 .. words) in place; words is a multiple of 4 (256 x groups), the table 16-byte aligned.  One workgroup. */
__global__ __launch_bounds__(ORDER_SCAN_THREADS) void k_sort_scan(uint32_t *__restrict__ table, uint32_t words) {
  __shared__ uint32_t waveSum[ORDER_SCAN_THREADS / 64u];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t carry = 0u;
  for (uint32_t base = 0; base < words; base += ORDER_SCAN_THREADS * 4u) {
    const uint32_t i = base + threadIdx.x * 4u;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (i < words) v = *(const uint4 *)(table + i);
    const uint32_t own = v.x + v.y + v.z + v.w;
    uint32_t incl = own;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)incl, off);
      if (lane >= (uint32_t)off) incl += o;
    }
    if (lane == 63u) waveSum[wave] = incl;
    __syncthreads();
    uint32_t before = 0u, total = 0u;
    for (uint32_t w = 0; w < ORDER_SCAN_THREADS / 64u; w++) {
      const uint32_t x = waveSum[w];
      before += w < wave ? x : 0u;
      total += x;
    }
    const uint32_t at = carry + before + (incl - own);
    if (i < words) *(uint4 *)(table + i) = make_uint4(at, at + v.x, at + v.x + v.y, at + v.x + v.y + v.z);
    carry += total;
    __syncthreads();                                     /* waveSum is written again in the next tile */
  }
}

/* posIn NULL: an item's position is its index (the first pass) */
__global__ __launch_bounds__(ORDER_THREADS) void k_sort_scatter(const uint32_t *__restrict__ keysIn, const uint32_t *__restrict__ posIn, uint32_t *__restrict__ keysOut,
                                                                uint32_t *__restrict__ posOut, uint32_t m, uint32_t shift, uint32_t groups,
                                                                const uint32_t *__restrict__ table) {
  __shared__ volatile uint32_t waveCount[ORDER_WAVES][256];      /* a wave's items of a digit so far */
  __shared__ uint32_t place[ORDER_WAVES][256];                   /* where a wave's first item of a digit goes */
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t w = 0; w < ORDER_WAVES; w++) waveCount[w][threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t first = blockIdx.x * ORDER_T + wave * ORDER_WAVE_ITEMS + lane;
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t key[ORDER_ROUNDS], rankIn[ORDER_ROUNDS];
#pragma unroll
  for (uint32_t r = 0; r < ORDER_ROUNDS; r++) {
    const uint32_t idx = first + r * 64u;
    const bool valid = idx < m;
    key[r] = valid ? keysIn[idx] : 0xFFFFFFFFu;
    const uint32_t d = (key[r] >> shift) & 255u;
    unsigned long long same = __builtin_amdgcn_ballot_w64(valid);      /* the valid lanes that share this lane's digit */
#pragma unroll
    for (uint32_t bit = 0; bit < 8u; bit++) {
      const bool set = ((d >> bit) & 1u) != 0u;
      const unsigned long long vote = __builtin_amdgcn_ballot_w64(set);
      same &= set ? vote : ~vote;
    }
    const uint32_t rank = (uint32_t)__popcll(same & below);
    uint32_t start = 0u;
    if (valid && rank == 0u) {                                         /* the digit's first lane of the round keeps the wave's count: one lane a digit */
      start = waveCount[wave][d];
      waveCount[wave][d] = start + (uint32_t)__popcll(same);
    }
    const int leader = valid ? (int)__builtin_ctzll(same) : (int)lane;      /* (valid: same holds this lane at least) */
    start = (uint32_t)__shfl((int)start, leader);
    rankIn[r] = start + rank;
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {
    const uint32_t d = threadIdx.x;
    uint32_t run = table[(size_t)d * groups + blockIdx.x];
    for (uint32_t w = 0; w < ORDER_WAVES; w++) { place[w][d] = run; run += waveCount[w][d]; }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < ORDER_ROUNDS; r++) {
    const uint32_t idx = first + r * 64u;
    if (idx < m) {
      const uint32_t dst = place[wave][(key[r] >> shift) & 255u] + rankIn[r];
      if (dst < m) {                                                   /* (always: the table counted these keys) */
        keysOut[dst] = key[r];
        posOut[dst] = posIn ? posIn[idx] : idx;
      }
    }
  }
}

}  // namespace flx

using namespace flx;

static flx_status fail(flx_context *ctx, flx_status code, const std::string &msg) { return flx_fail(ctx, code, msg.c_str()); }

size_t flx_order_room(uint32_t most) { return most; }
size_t flx_order_table_room(uint32_t most) { return flx_sort_table_words(most); }

/* the stable sort of d_order_keys[0][0 .. m) enqueued: the order ends in d_order_pos[0], the sorted keys in d_order_keys[0] */
static flx_status sort_enqueue(flx_context *ctx, uint32_t m, uint32_t *groups) {
  const uint32_t g = flx_sort_groups(m);
  uint32_t *table = ctx->d_order_counts.get();
  for (uint32_t pass = 0; pass < ORDER_PASSES; pass++) {
    const uint32_t in = pass & 1u, out = in ^ 1u, shift = pass * 8u;
    hipLaunchKernelGGL(k_sort_count, dim3(g), dim3(ORDER_THREADS), 0, ctx->stream, ctx->d_order_keys[in].get(), m, shift, g, table);
    hipLaunchKernelGGL(k_sort_scan, dim3(1), dim3(ORDER_SCAN_THREADS), 0, ctx->stream, table, 256u * g);
    hipLaunchKernelGGL(k_sort_scatter, dim3(g), dim3(ORDER_THREADS), 0, ctx->stream, ctx->d_order_keys[in].get(), pass == 0u ? (const uint32_t *)nullptr : ctx->d_order_pos[in].get(),
                       ctx->d_order_keys[out].get(), ctx->d_order_pos[out].get(), m, shift, g, (const uint32_t *)table);
    FLX_HIP(ctx, hipGetLastError());
  }
  if (groups) *groups = g;
  return FLX_OK;
}

/* bounds and keys of m rays into ctl[0..6] and d_order_keys[0] */
static flx_status keys_enqueue(flx_context *ctx, const float4 *rays, const float4 *hits, uint32_t m, uint32_t *ctl) {
  FLX_HIP(ctx, hipMemsetAsync(ctl, 0xFF, 3 * sizeof(uint32_t), ctx->stream));
  FLX_HIP(ctx, hipMemsetAsync(ctl + 3, 0x00, 5 * sizeof(uint32_t), ctx->stream));
  const uint32_t full = (m + ORDER_THREADS - 1u) / ORDER_THREADS;
  hipLaunchKernelGGL(k_hit_bounds, dim3(full < ORDER_BOUNDS_GROUPS ? full : ORDER_BOUNDS_GROUPS), dim3(ORDER_THREADS), 0, ctx->stream, rays, hits, m, ctl);
  hipLaunchKernelGGL(k_hit_keys, dim3(full), dim3(ORDER_THREADS), 0, ctx->stream, rays, hits, m, ctl, ctx->d_order_keys[0].get());
  FLX_HIP(ctx, hipGetLastError());
  return FLX_OK;
}

flx_status flx_slab_order(flx_context *ctx, const float4 *rays, const float4 *hits, uint32_t m, uint32_t *groups) {
  flx_status s = keys_enqueue(ctx, rays, hits, m, ctx->d_order_ctl.get());
  return s ? s : sort_enqueue(ctx, m, groups);
}

/* ---- the debug calls ------------------------------------------------------------------------------------------------------------------------------- */

static flx_status sort_args_refused(flx_context *ctx, enum flx_sort_refusal why, const char *call) {
  switch (why) {
    case FLX_SORT_ARGS_OK: return FLX_OK;
    case FLX_SORT_NULL: return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": an array is NULL");
    default: return fail(ctx, FLX_ERR_INVALID, std::string(call) + ": n is 0 or above 2^21, the most rays of a slab");
  }
}

extern "C" flx_status flx_debug_sort_keys(flx_context *ctx, const uint32_t *keys, uint32_t n, uint32_t *order) {
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = sort_args_refused(ctx, flx_sort_args_check((uint64_t)(uintptr_t)keys, (uint64_t)(uintptr_t)order, 1u, 1u, n), "flx_debug_sort_keys");
  if (s) return s;
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  if ((s = flx_server_stop(ctx))) return s;
  if ((s = flx_grow(ctx, flx_need(&ctx->d_order_keys[0], flx_order_room(n)), flx_need(&ctx->d_order_keys[1], flx_order_room(n)), flx_need(&ctx->d_order_pos[0], flx_order_room(n)),
                    flx_need(&ctx->d_order_pos[1], flx_order_room(n)), flx_need(&ctx->d_order_counts, flx_order_table_room(n)))))
    return s;
  FLX_HIP(ctx, hipMemcpyAsync(ctx->d_order_keys[0].get(), keys, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  if ((s = sort_enqueue(ctx, n, nullptr))) return s;
  FLX_HIP(ctx, hipMemcpyAsync(order, ctx->d_order_pos[0].get(), (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return FLX_OK;
}

extern "C" flx_status flx_debug_hit_keys(flx_context *ctx, const float *rays, const void *hits, uint32_t n, uint32_t *keys, float bounds[6]) {
  if (!ctx) return FLX_ERR_INVALID;
  flx_status s = sort_args_refused(ctx, flx_sort_args_check((uint64_t)(uintptr_t)rays, (uint64_t)(uintptr_t)hits, (uint64_t)(uintptr_t)keys, (uint64_t)(uintptr_t)bounds, n),
                                   "flx_debug_hit_keys");
  if (s) return s;
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  if ((s = flx_server_stop(ctx))) return s;
  if ((s = flx_grow(ctx, flx_need(&ctx->d_query_rays, (size_t)n * 2u), flx_need(&ctx->d_query_hits, (size_t)n * 2u), flx_need(&ctx->d_order_keys[0], flx_order_room(n)),
                    flx_need(&ctx->d_order_ctl, 16))))
    return s;
  uint32_t *ctl = ctx->d_order_ctl.get() + 8;            /* (the second eight: a traced batch's live count stays what it was) */
  FLX_HIP(ctx, hipMemcpyAsync(ctx->d_query_rays.get(), rays, (size_t)n * FLX_RAY_ROW_BYTES, hipMemcpyHostToDevice, ctx->stream));
  FLX_HIP(ctx, hipMemcpyAsync(ctx->d_query_hits.get(), hits, (size_t)n * FLX_RAY_ROW_BYTES, hipMemcpyHostToDevice, ctx->stream));
  if ((s = keys_enqueue(ctx, ctx->d_query_rays.get(), ctx->d_query_hits.get(), n, ctl))) return s;
  uint32_t mapped[6];
  FLX_HIP(ctx, hipMemcpyAsync(keys, ctx->d_order_keys[0].get(), (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  FLX_HIP(ctx, hipMemcpyAsync(mapped, ctl, sizeof mapped, hipMemcpyDeviceToHost, ctx->stream));
  FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < 6; k++) bounds[k] = flx_ray_key_float(flx_ray_key_unmap(mapped[k]));
  return FLX_OK;
}

extern "C" flx_status flx_debug_last_ray_order(flx_context *ctx, uint32_t out[8]) {
  if (!ctx || !out) return FLX_ERR_INVALID;
  const flx_context::OrderLaunch &o = ctx->last_ray_order;
  out[0] = o.ordered; out[1] = ORDER_T; out[2] = o.groups; out[3] = o.passes; out[4] = o.n; out[5] = 0u; out[6] = 0u; out[7] = 0u;
  if (o.ordered) {
    FLX_HIP(ctx, hipSetDevice(ctx->device));
    FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    FLX_HIP(ctx, hipMemcpy(&out[5], ctx->d_order_ctl.get() + 6, sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  return FLX_OK;
}
