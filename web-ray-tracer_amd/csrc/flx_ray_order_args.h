/* flx_ray_order_args.h — what the ordered trace and the sort's debug calls decide about their arguments before they ask the device anything: plain C++, no HIP, so
 * that a stand-alone program can hold it under the sanitizers (tests/ray_order_args_main.cc). */
#ifndef FLX_RAY_ORDER_ARGS_H
#define FLX_RAY_ORDER_ARGS_H

#include <stdint.h>

#include "flx_query_args.h"      /* FLX_TRACE_SLAB_RAYS: the most rays a slab has, hence the most keys a sort takes */

#define FLX_ORDER_KNOWN_BITS 1u      /* FLX_TRACE_ORDER_HITS */
#define FLX_ORDER_SORT_ITEMS 2048u   /* T: the items a sort workgroup takes (flx_rays_order.hip: ORDER_T) */

/* flx_rays_trace_ordered[_device]'s `order` */
static inline int flx_order_bits_known(uint32_t order) { return (order & ~FLX_ORDER_KNOWN_BITS) == 0u; }

enum flx_sort_refusal {
  FLX_SORT_ARGS_OK = 0,
  FLX_SORT_NULL,                     /* a NULL array */
  FLX_SORT_COUNT                     /* n is 0 or above 2^21 */
};

/* flx_debug_sort_keys' and flx_debug_hit_keys' arrays (addresses as integers; all must be there) and n: 1 .. 2^21 */
static inline enum flx_sort_refusal flx_sort_args_check(uint64_t a, uint64_t b, uint64_t c, uint64_t d, uint32_t n) {
  if (a == 0u || b == 0u || c == 0u || d == 0u) return FLX_SORT_NULL;
  if (n == 0u || n > FLX_TRACE_SLAB_RAYS) return FLX_SORT_COUNT;
  return FLX_SORT_ARGS_OK;
}

/* workgroups of the sort of n keys, and the words of one pass's digit-major count table: at most 1024 and 2^18 for a slab's 2^21 rays (n + T - 1 cannot wrap:
 * n <= 2^21) */
static inline uint32_t flx_sort_groups(uint32_t n) { return (n + (FLX_ORDER_SORT_ITEMS - 1u)) / FLX_ORDER_SORT_ITEMS; }
static inline uint32_t flx_sort_table_words(uint32_t n) { return 256u * flx_sort_groups(n); }

#endif
