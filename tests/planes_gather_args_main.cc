/* Stand-alone check of web-ray-tracer_amd/csrc/flx_planes_gather_args.h: what the ray-image calls that take a volume decide about it without a device — the arrays
 * of a call, the volume's arrays against them, the flags word, the slab rule — and, through flx_gather_args.h, the order in which the volume's own words are refused.
 * tests/test_planes_gather_args_cpu.py compiles it, plainly and with -fsanitize=address,undefined, and runs it; it prints "ok <cases>" and returns 0, or says which
 * case failed. */
#include <float.h>
#include <math.h>
#include <stdio.h>

#include "flx_planes_gather_args.h"

static int failures = 0, cases = 0;
static void expect(const char *name, long long got, long long want) {
  cases++;
  if (got != want) { printf("FAILED %s: got %lld, want %lld\n", name, got, want); failures++; }
}

int main(void) {
  const uint64_t A = 0x7f0000000000ull, TOP = UINT64_MAX;
  const uint32_t n = 1080;
  flx_planes_gather_array call[FLX_PLANES_GATHER_CALL_ARRAYS];
  /* the arrays of a planes call: rays 32 n, planes8 5 * 4 n, planes32 5 * 16 n; only those asked for */
  expect("planes: all three", flx_planes_gather_planes_arrays(A, A + 0x100000, A + 0x200000, n, call), 3);
  expect("planes: rays bytes", (long long)call[0].bytes, 32ll * n);
  expect("planes: planes8 at", call[1].address == A + 0x100000, 1);
  expect("planes: planes8 bytes", (long long)call[1].bytes, 20ll * n);
  expect("planes: planes32 bytes", (long long)call[2].bytes, 80ll * n);
  expect("planes: no planes32", flx_planes_gather_planes_arrays(A, A + 0x100000, 0, n, call), 2);
  expect("planes: no planes8", flx_planes_gather_planes_arrays(A, 0, A + 0x200000, n, call), 2);
  expect("planes: planes32 second", (long long)call[1].bytes, 80ll * n);
  expect("planes: nothing", flx_planes_gather_planes_arrays(0, 0, 0, n, call), 0);
  expect("planes: most rays", flx_planes_gather_planes_arrays(A, 0, A + 0x8000000000ull, 0xffffffffu, call), 2);
  expect("planes: most rays, bytes", call[1].bytes == 80ull * 0xffffffffull, 1);
  /* an image call: rays 32 n and the image 16 n; a camera call has no rays of the caller's */
  expect("image: both", flx_planes_gather_image_arrays(A, A + 0x100000, n, call), 2);
  expect("image: image bytes", (long long)call[1].bytes, 16ll * n);
  expect("image: a camera's", flx_planes_gather_image_arrays(0, A + 0x100000, n, call), 1);
  expect("image: a camera's image first", call[0].address == A + 0x100000 && call[0].bytes == 16ull * n, 1);
  /* each array of the volume against each array of the call: half-open ranges */
  const uint64_t bytes[3] = { 48u * 144u, 48u * 16u * 16u, 48u * 16u };
  const int kc = flx_planes_gather_planes_arrays(A, A + 0x100000, A + 0x200000, n, call);
  {
    const uint64_t address[3] = { A + 0x300000, A + 0x400000, A + 0x500000 };
    expect("apart", flx_planes_gather_overlap_check(address, bytes, 3, call, kc), FLX_GATHER_ARGS_OK);
    expect("no arrays of the volume", flx_planes_gather_overlap_check(address, bytes, 0, call, kc), FLX_GATHER_ARGS_OK);
    expect("no arrays of the call", flx_planes_gather_overlap_check(address, bytes, 3, call, 0), FLX_GATHER_ARGS_OK);
  }
  for (int which = 0; which < 3; which++)
    for (int other = 0; other < kc; other++) {
      uint64_t address[3] = { A + 0x300000, A + 0x400000, A + 0x500000 };
      address[which] = call[other].address;
      expect("an array is an array of the call", flx_planes_gather_overlap_check(address, bytes, 3, call, kc), FLX_GATHER_OVERLAP);
      address[which] = call[other].address + call[other].bytes - 1u;
      expect("an array starts in the last byte", flx_planes_gather_overlap_check(address, bytes, 3, call, kc), FLX_GATHER_OVERLAP);
      address[which] = call[other].address + call[other].bytes;
      expect("an array right behind", flx_planes_gather_overlap_check(address, bytes, 3, call, kc), FLX_GATHER_ARGS_OK);
      address[which] = call[other].address - bytes[which];
      expect("an array right in front", flx_planes_gather_overlap_check(address, bytes, 3, call, kc), FLX_GATHER_ARGS_OK);
      address[which] = call[other].address - bytes[which] + 1u;
      expect("an array ends in the first byte", flx_planes_gather_overlap_check(address, bytes, 3, call, kc), FLX_GATHER_OVERLAP);
      address[which] = call[other].address + 16u;
      expect("an array inside, the later arrays not looked at", flx_planes_gather_overlap_check(address, bytes, which + 1, call, kc), FLX_GATHER_OVERLAP);
      expect("an array inside an array the call does not name", flx_planes_gather_overlap_check(address, bytes, which + 1, call, other), FLX_GATHER_ARGS_OK);
    }
  {
    /* the top of the address space: arrays that touch there share no byte */
    const uint64_t address[1] = { TOP - 144u }, one[1] = { 144u };
    flx_planes_gather_array top[1] = { { TOP - 144u - 16u, 16u } };
    expect("touching at the top", flx_planes_gather_overlap_check(address, one, 1, top, 1), FLX_GATHER_ARGS_OK);
    top[0].address += 1u;
    expect("overlapping at the top", flx_planes_gather_overlap_check(address, one, 1, top, 1), FLX_GATHER_OVERLAP);
  }
  /* the volume's own words keep flx_rays_trace_gather's order: NULL, gain, reserved, the pair */
  expect("no volume first", flx_gather_volume_check(0, NAN, 1u, 1, 0), FLX_GATHER_VOLUME_NULL);
  expect("gain before reserved", flx_gather_volume_check(1, -1.0f, 1u, 1, 0), FLX_GATHER_GAIN);
  expect("gain inf", flx_gather_volume_check(1, INFINITY, 0u, 0, 0), FLX_GATHER_GAIN);
  expect("reserved before the pair", flx_gather_volume_check(1, 1.0f, 1u, 1, 0), FLX_GATHER_RESERVED);
  expect("the pair", flx_gather_volume_check(1, 1.0f, 0u, 0, 1), FLX_GATHER_MAP_PAIR);
  expect("gain 0", flx_gather_volume_check(1, 0.0f, 0u, 1, 1), FLX_GATHER_ARGS_OK);
  expect("gain FLT_MAX", flx_gather_volume_check(1, FLT_MAX, 0u, 0, 0), FLX_GATHER_ARGS_OK);
  /* the flags word and the slab rule: one slot a ray whatever the samples, 2^21 rays, so a 1080p image is one slab */
  expect("flags: plain", flx_planes_gather_flags(0, 0), 0);
  expect("flags: a map", flx_planes_gather_flags(1, 0), 1);
  expect("flags: offsets", flx_planes_gather_flags(0, 1), 2);
  expect("flags: both", flx_planes_gather_flags(7, -1), 3);
  expect("slab", flx_planes_gather_slab_rays(0), 1u << 21);
  expect("slab holds 1080p", flx_planes_gather_slab_rays(0) >= 1920u * 1080u, 1);
  expect("slab, ceiling 64", flx_planes_gather_slab_rays(64), 64);
  expect("slab, ceiling 1", flx_planes_gather_slab_rays(1), 1);
  expect("slab, a ceiling above it", flx_planes_gather_slab_rays(1u << 22), 1u << 21);
  if (failures) return 1;
  printf("ok %d\n", cases);
  return 0;
}
