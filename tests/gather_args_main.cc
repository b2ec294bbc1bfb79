/* Stand-alone check of flx_gather_volume_check, flx_gather_arrays_check and the slab rule (web-ray-tracer_amd/csrc/flx_gather_args.h): what
 * flx_rays_trace_gather_device decides about its volume without a device.  tests/test_rays_gather_cpu.py compiles it with -fsanitize=address,undefined and runs it;
 * it prints "ok <cases>" and returns 0, or says which case failed. */
#include <float.h>
#include <math.h>
#include <stdio.h>

#include "flx_gather_args.h"

static int failures = 0, cases = 0;
static void expect(const char *name, long long got, long long want) {
  cases++;
  if (got != want) { printf("FAILED %s: got %lld, want %lld\n", name, got, want); failures++; }
}

int main(void) {
  const uint64_t A = 0x7f0000000000ull, TOP = UINT64_MAX;
  const float inf = INFINITY, nan = NAN;
  /* the volume's own words, in the order they are said */
  expect("no volume", flx_gather_volume_check(0, 1.0f, 0u, 0, 0), FLX_GATHER_VOLUME_NULL);
  expect("no volume before a bad gain", flx_gather_volume_check(0, -1.0f, 1u, 1, 0), FLX_GATHER_VOLUME_NULL);
  expect("gain negative", flx_gather_volume_check(1, -1.0f, 0u, 0, 0), FLX_GATHER_GAIN);
  expect("gain the least negative", flx_gather_volume_check(1, -FLT_TRUE_MIN, 0u, 0, 0), FLX_GATHER_GAIN);
  expect("gain +inf", flx_gather_volume_check(1, inf, 0u, 0, 0), FLX_GATHER_GAIN);
  expect("gain -inf", flx_gather_volume_check(1, -inf, 0u, 0, 0), FLX_GATHER_GAIN);
  expect("gain NaN", flx_gather_volume_check(1, nan, 0u, 0, 0), FLX_GATHER_GAIN);
  expect("gain before reserved", flx_gather_volume_check(1, nan, 7u, 1, 0), FLX_GATHER_GAIN);
  expect("gain 0", flx_gather_volume_check(1, 0.0f, 0u, 0, 0), FLX_GATHER_ARGS_OK);
  expect("gain -0", flx_gather_volume_check(1, -0.0f, 0u, 0, 0), FLX_GATHER_ARGS_OK);
  expect("gain FLT_MAX", flx_gather_volume_check(1, FLT_MAX, 0u, 0, 0), FLX_GATHER_ARGS_OK);
  expect("gain the least", flx_gather_volume_check(1, FLT_TRUE_MIN, 0u, 1, 1), FLX_GATHER_ARGS_OK);
  expect("reserved 1", flx_gather_volume_check(1, 1.0f, 1u, 0, 0), FLX_GATHER_RESERVED);
  expect("reserved all ones", flx_gather_volume_check(1, 1.0f, 0xffffffffu, 1, 1), FLX_GATHER_RESERVED);
  expect("reserved before the pair", flx_gather_volume_check(1, 1.0f, 1u, 1, 0), FLX_GATHER_RESERVED);
  expect("map without maps", flx_gather_volume_check(1, 1.0f, 0u, 1, 0), FLX_GATHER_MAP_PAIR);
  expect("maps without map", flx_gather_volume_check(1, 1.0f, 0u, 0, 1), FLX_GATHER_MAP_PAIR);
  expect("map and maps", flx_gather_volume_check(1, 1.0f, 0u, 1, 1), FLX_GATHER_ARGS_OK);
  expect("neither", flx_gather_volume_check(1, 1.0f, 0u, 0, 0), FLX_GATHER_ARGS_OK);
  expect("any non-zero is given", flx_gather_volume_check(1, 1.0f, 0u, 5, -3), FLX_GATHER_ARGS_OK);
  /* each array of the volume against the rays and the radiance: n rows of 32 bytes, half-open ranges */
  const uint32_t n = 64;
  const uint64_t rows = (uint64_t)n * 32u, rays = A, radiance = A + 0x100000;
  {
    const uint64_t address[3] = { A + 0x200000, A + 0x300000, A + 0x400000 }, bytes[3] = { 27u * 144u, 27u * 16u * 16u, 27u * 16u };
    expect("apart", flx_gather_arrays_check(address, bytes, 3, rays, radiance, n), FLX_GATHER_ARGS_OK);
    expect("no arrays", flx_gather_arrays_check(address, bytes, 0, rays, radiance, n), FLX_GATHER_ARGS_OK);
  }
  for (int which = 0; which < 3; which++) {
    uint64_t address[3] = { A + 0x200000, A + 0x300000, A + 0x400000 };
    const uint64_t bytes[3] = { 27u * 144u, 27u * 16u * 16u, 27u * 16u };
    address[which] = rays;
    expect("an array is the rays", flx_gather_arrays_check(address, bytes, 3, rays, radiance, n), FLX_GATHER_OVERLAP);
    address[which] = radiance;
    expect("an array is the radiance", flx_gather_arrays_check(address, bytes, 3, rays, radiance, n), FLX_GATHER_OVERLAP);
    address[which] = rays + rows - 1u;
    expect("an array starts in the rays' last byte", flx_gather_arrays_check(address, bytes, 3, rays, radiance, n), FLX_GATHER_OVERLAP);
    address[which] = rays + rows;
    expect("an array right behind the rays", flx_gather_arrays_check(address, bytes, 3, rays, radiance, n), FLX_GATHER_ARGS_OK);
    address[which] = radiance - bytes[which];
    expect("an array right in front of the radiance", flx_gather_arrays_check(address, bytes, 3, rays, radiance, n), FLX_GATHER_ARGS_OK);
    address[which] = radiance - bytes[which] + 1u;
    expect("an array ends in the radiance's first byte", flx_gather_arrays_check(address, bytes, 3, rays, radiance, n), FLX_GATHER_OVERLAP);
    address[which] = radiance + 32u;
    expect("an array inside the radiance", flx_gather_arrays_check(address, bytes, which + 1, rays, radiance, n), FLX_GATHER_OVERLAP);
  }
  {
    /* the ends of the address space: arrays that touch there share no byte; the largest n */
    const uint64_t address[1] = { TOP - 144u }, bytes[1] = { 144u };
    expect("touching at the top", flx_gather_arrays_check(address, bytes, 1, TOP - 144u - 32u, A, 1), FLX_GATHER_ARGS_OK);
    expect("overlapping at the top", flx_gather_arrays_check(address, bytes, 1, TOP - 144u - 31u, A, 1), FLX_GATHER_OVERLAP);
    const uint64_t far[1] = { A + 0x2000000000ull };
    expect("huge n stops short", flx_gather_arrays_check(far, bytes, 1, A, A + 0x4000000000ull, 0xffffffffu), FLX_GATHER_ARGS_OK);
    const uint64_t reached[1] = { A + 0x1fffffffe0ull - 1u };
    expect("huge n reaches the array", flx_gather_arrays_check(reached, bytes, 1, A, A + 0x4000000000ull, 0xffffffffu), FLX_GATHER_OVERLAP);
  }
  /* slabs: five slots a sample under the traced batches' 2^24; whole blocks of 64 rays, at least one; the lookup's workgroups cover the records */
  expect("slots, 1 sample", flx_gather_slab_slots(1), 5);
  expect("slots, most samples that fit", flx_gather_slab_slots(UINT32_MAX / 5u), (UINT32_MAX / 5u) * 5u);
  expect("slots saturate", flx_gather_slab_slots(UINT32_MAX / 5u + 1u), UINT32_MAX);
  expect("slots saturate, most samples", flx_gather_slab_slots(0x7fffffffu), UINT32_MAX);
  expect("slab, 1 sample", flx_gather_slab_rays(1, 0), 1u << 21);
  expect("slab, 2 samples", flx_gather_slab_rays(2, 0), ((1u << 24) / 10u) & ~63u);
  expect("slab, 8 samples", flx_gather_slab_rays(8, 0), ((1u << 24) / 40u) & ~63u);
  expect("slab, most samples", flx_gather_slab_rays(0x7fffffffu, 0), 64);
  expect("slab, ceiling 64", flx_gather_slab_rays(3, 64), 64);
  expect("slab, ceiling 1", flx_gather_slab_rays(3, 1), 1);
  for (uint32_t s = 1; s != 0 && s <= 0x7fffffffu; s = s < 0x40000000u ? s * 2u + (s & 1u) : (s == 0x7fffffffu ? 0u : 0x7fffffffu)) {
    const uint64_t slab = flx_gather_slab_rays(s, 0), units = ((slab + 63u) >> 6) * s;
    expect("records and slots fit", slab == 64u || slab * s * FLX_GATHER_SLOTS <= (1ull << 24), 1);
    expect("slab units fit", units + (1ull << 22) < (1ull << 32), 1);
  }
  expect("groups, 0 records", flx_gather_groups(0), 0);
  expect("groups, 1 record", flx_gather_groups(1), 1);
  expect("groups, 256 records", flx_gather_groups(256), 1);
  expect("groups, 257 records", flx_gather_groups(257), 2);
  expect("groups, 2^32 records", flx_gather_groups(1ull << 32), 1u << 24);
  if (failures) return 1;
  printf("ok %d\n", cases);
  return 0;
}
