/* Stand-alone check of flx_ray_planes_args.h (web-ray-tracer_amd/csrc): what flx_rays_planes_device and flx_rays_image_device decide about their arguments without a
 * device.  tests/test_rays_planes_cpu.py compiles it with -fsanitize=address,undefined and runs it; it prints "ok <cases>" and returns 0, or says which case failed. */
#include <stdio.h>

#include "flx_ray_planes_args.h"

static int failures = 0, cases = 0;
static void expect(const char *name, long long got, long long want) {
  cases++;
  if (got != want) { printf("FAILED %s: got %lld, want %lld\n", name, got, want); failures++; }
}

int main(void) {
  const uint64_t A = 0x7f0000000000ull, B = 0x7e0000000000ull, TOP = UINT64_MAX;
  const uint32_t N = 0xffffffffu;
  uint32_t n = 7;
  /* planes: which pointers are given */
  expect("both planes NULL", flx_ray_planes_arrays_check(A, 0, 0, 16), FLX_RAY_PLANES_NONE);
  expect("both planes NULL before the rays", flx_ray_planes_arrays_check(0, 0, 0, 16), FLX_RAY_PLANES_NONE);
  expect("rays NULL", flx_ray_planes_arrays_check(0, A, B, 16), FLX_RAY_PLANES_NULL);
  expect("rays NULL, bytes alone", flx_ray_planes_arrays_check(0, A, 0, 16), FLX_RAY_PLANES_NULL);
  expect("bytes alone", flx_ray_planes_arrays_check(A, B, 0, 16), FLX_RAY_PLANES_ARGS_OK);
  expect("floats alone", flx_ray_planes_arrays_check(A, 0, B, 16), FLX_RAY_PLANES_ARGS_OK);
  expect("both", flx_ray_planes_arrays_check(A, B, B + 0x100000, 16), FLX_RAY_PLANES_ARGS_OK);
  expect("one ray", flx_ray_planes_arrays_check(A, B, B + 32u, 1), FLX_RAY_PLANES_ARGS_OK);
  expect("largest n", flx_ray_planes_arrays_check(A, B, A + 0x10000000000ull, N), FLX_RAY_PLANES_ARGS_OK);
  /* address + bytes leaving 64 bits: rays n * 32, planes8 n * 20, planes32 n * 80 */
  expect("rays end at the top", flx_ray_planes_arrays_check(TOP - 32u, A, 0, 1), FLX_RAY_PLANES_ARGS_OK);
  expect("rays wrap", flx_ray_planes_arrays_check(TOP - 31u, A, 0, 1), FLX_RAY_PLANES_WRAPS);
  expect("bytes end at the top", flx_ray_planes_arrays_check(A, TOP - 20u, 0, 1), FLX_RAY_PLANES_ARGS_OK);
  expect("bytes wrap", flx_ray_planes_arrays_check(A, TOP - 19u, 0, 1), FLX_RAY_PLANES_WRAPS);
  expect("the fifth byte plane wraps", flx_ray_planes_arrays_check(A, TOP - 16u, 0, 1), FLX_RAY_PLANES_WRAPS);
  expect("floats end at the top", flx_ray_planes_arrays_check(A, 0, TOP - 80u, 1), FLX_RAY_PLANES_ARGS_OK);
  expect("floats wrap", flx_ray_planes_arrays_check(A, 0, TOP - 79u, 1), FLX_RAY_PLANES_WRAPS);
  expect("the fifth float plane wraps", flx_ray_planes_arrays_check(A, 0, TOP - 64u, 1), FLX_RAY_PLANES_WRAPS);
  expect("largest n, floats end at the top", flx_ray_planes_arrays_check(A, 0, TOP - (uint64_t)N * 80u, N), FLX_RAY_PLANES_ARGS_OK);
  expect("largest n, floats wrap", flx_ray_planes_arrays_check(A, 0, TOP - (uint64_t)N * 80u + 1u, N), FLX_RAY_PLANES_WRAPS);
  expect("largest n, bytes wrap", flx_ray_planes_arrays_check(A, TOP - (uint64_t)N * 20u + 1u, 0, N), FLX_RAY_PLANES_WRAPS);
  expect("a plane not asked for is not looked at", flx_ray_planes_arrays_check(A, B, 0, N), FLX_RAY_PLANES_ARGS_OK);
  expect("wraps are said before overlaps", flx_ray_planes_arrays_check(A, A, TOP - 79u, 1), FLX_RAY_PLANES_WRAPS);
  /* an output against the rays */
  expect("bytes are the rays", flx_ray_planes_arrays_check(A, A, 0, 1), FLX_RAY_PLANES_OVERLAP_RAYS);
  expect("floats are the rays", flx_ray_planes_arrays_check(A, 0, A, 1), FLX_RAY_PLANES_OVERLAP_RAYS);
  expect("bytes right behind the rays", flx_ray_planes_arrays_check(A, A + 64u * 32u, 0, 64), FLX_RAY_PLANES_ARGS_OK);
  expect("bytes start in the last ray", flx_ray_planes_arrays_check(A, A + 64u * 32u - 1u, 0, 64), FLX_RAY_PLANES_OVERLAP_RAYS);
  expect("rays right behind the bytes", flx_ray_planes_arrays_check(A + 64u * 20u, A, 0, 64), FLX_RAY_PLANES_ARGS_OK);
  expect("rays start in the fifth byte plane", flx_ray_planes_arrays_check(A + 64u * 20u - 1u, A, 0, 64), FLX_RAY_PLANES_OVERLAP_RAYS);
  expect("rays where a sixth byte plane would be", flx_ray_planes_arrays_check(A + 64u * 20u, A, 0, 64), FLX_RAY_PLANES_ARGS_OK);
  expect("floats right behind the rays", flx_ray_planes_arrays_check(A, 0, A + 64u * 32u, 64), FLX_RAY_PLANES_ARGS_OK);
  expect("floats start in the last ray", flx_ray_planes_arrays_check(A, 0, A + 64u * 32u - 16u, 64), FLX_RAY_PLANES_OVERLAP_RAYS);
  expect("rays right behind the floats", flx_ray_planes_arrays_check(A + 64u * 80u, 0, A, 64), FLX_RAY_PLANES_ARGS_OK);
  expect("rays inside the fifth float plane", flx_ray_planes_arrays_check(A + 64u * 80u - 16u, 0, A, 64), FLX_RAY_PLANES_OVERLAP_RAYS);
  expect("rays inside the floats", flx_ray_planes_arrays_check(A + 4096u, 0, A, 0x10000), FLX_RAY_PLANES_OVERLAP_RAYS);
  expect("floats inside the rays", flx_ray_planes_arrays_check(A, B, A + 4096u, 0x10000), FLX_RAY_PLANES_OVERLAP_RAYS);
  expect("the rays are said before the other output", flx_ray_planes_arrays_check(A, A, A, 4), FLX_RAY_PLANES_OVERLAP_RAYS);
  expect("huge n reaches the bytes", flx_ray_planes_arrays_check(A, A + (uint64_t)N * 32u - 1u, 0, N), FLX_RAY_PLANES_OVERLAP_RAYS);
  expect("huge n ends in front of them", flx_ray_planes_arrays_check(A, A + (uint64_t)N * 32u, 0, N), FLX_RAY_PLANES_ARGS_OK);
  /* the two outputs against each other */
  expect("the same output twice", flx_ray_planes_arrays_check(A, B, B, 4), FLX_RAY_PLANES_OVERLAP_OUT);
  expect("floats right behind the bytes", flx_ray_planes_arrays_check(A, B, B + 64u * 20u, 64), FLX_RAY_PLANES_ARGS_OK);
  expect("floats start in the fifth byte plane", flx_ray_planes_arrays_check(A, B, B + 64u * 20u - 4u, 64), FLX_RAY_PLANES_OVERLAP_OUT);
  expect("bytes right behind the floats", flx_ray_planes_arrays_check(A, B + 64u * 80u, B, 64), FLX_RAY_PLANES_ARGS_OK);
  expect("bytes start in the fifth float plane", flx_ray_planes_arrays_check(A, B + 64u * 80u - 1u, B, 64), FLX_RAY_PLANES_OVERLAP_OUT);
  expect("bytes inside the floats", flx_ray_planes_arrays_check(A, B + 4096u, B, 0x10000), FLX_RAY_PLANES_OVERLAP_OUT);
  expect("touching at the top", flx_ray_planes_arrays_check(A, TOP - 100u, TOP - 80u, 1), FLX_RAY_PLANES_ARGS_OK);
  /* an image's size */
  expect("width 0", flx_ray_image_size_check(0, 48, &n), FLX_RAY_PLANES_SIZE);
  expect("height 0", flx_ray_image_size_check(64, 0, &n), FLX_RAY_PLANES_SIZE);
  expect("both 0", flx_ray_image_size_check(0, 0, &n), FLX_RAY_PLANES_SIZE);
  expect("width 0 of most rows", flx_ray_image_size_check(0, N, &n), FLX_RAY_PLANES_SIZE);
  expect("n is left alone by a refusal", n, 7);
  expect("64 x 48", flx_ray_image_size_check(64, 48, &n), FLX_RAY_PLANES_ARGS_OK);
  expect("its rays", n, 64 * 48);
  expect("one pixel", flx_ray_image_size_check(1, 1, &n), FLX_RAY_PLANES_ARGS_OK);
  expect("its ray", n, 1);
  expect("65535 x 65537", flx_ray_image_size_check(65535u, 65537u, &n), FLX_RAY_PLANES_ARGS_OK);
  expect("its rays: 2^32 - 1", n, 0xffffffffll);
  expect("65536 x 65536: 2^32", flx_ray_image_size_check(65536u, 65536u, &n), FLX_RAY_PLANES_PIXELS);
  expect("n is left alone by that refusal too", n, 0xffffffffll);
  expect("the largest canvas", flx_ray_image_size_check(N, N, &n), FLX_RAY_PLANES_PIXELS);
  expect("one row of most pixels", flx_ray_image_size_check(N, 1, &n), FLX_RAY_PLANES_ARGS_OK);
  expect("one column of most pixels", flx_ray_image_size_check(1, N, (uint32_t *)0), FLX_RAY_PLANES_ARGS_OK);
  expect("2 x 2^31: 2^32", flx_ray_image_size_check(2, 0x80000000u, &n), FLX_RAY_PLANES_PIXELS);
  /* an image's arrays: rays n * 32, out n * 16 */
  expect("image rays NULL", flx_ray_image_arrays_check(0, A, 16), FLX_RAY_PLANES_NULL);
  expect("image out NULL", flx_ray_image_arrays_check(A, 0, 16), FLX_RAY_PLANES_NULL);
  expect("image arrays apart", flx_ray_image_arrays_check(A, B, 16), FLX_RAY_PLANES_ARGS_OK);
  expect("image rays end at the top", flx_ray_image_arrays_check(TOP - 32u, A, 1), FLX_RAY_PLANES_ARGS_OK);
  expect("image rays wrap", flx_ray_image_arrays_check(TOP - 31u, A, 1), FLX_RAY_PLANES_WRAPS);
  expect("image out ends at the top", flx_ray_image_arrays_check(A, TOP - 16u, 1), FLX_RAY_PLANES_ARGS_OK);
  expect("image out wraps", flx_ray_image_arrays_check(A, TOP - 15u, 1), FLX_RAY_PLANES_WRAPS);
  expect("largest image wraps", flx_ray_image_arrays_check(A, TOP - (uint64_t)N * 16u + 1u, N), FLX_RAY_PLANES_WRAPS);
  expect("largest image ends at the top", flx_ray_image_arrays_check(A, TOP - (uint64_t)N * 16u, N), FLX_RAY_PLANES_ARGS_OK);
  expect("image is the rays", flx_ray_image_arrays_check(A, A, 1), FLX_RAY_PLANES_OVERLAP_RAYS);
  expect("image right behind the rays", flx_ray_image_arrays_check(A, A + 64u * 32u, 64), FLX_RAY_PLANES_ARGS_OK);
  expect("image starts in the last ray", flx_ray_image_arrays_check(A, A + 64u * 32u - 1u, 64), FLX_RAY_PLANES_OVERLAP_RAYS);
  expect("rays right behind the image", flx_ray_image_arrays_check(A + 64u * 16u, A, 64), FLX_RAY_PLANES_ARGS_OK);
  expect("rays start in the image's last byte", flx_ray_image_arrays_check(A + 64u * 16u - 1u, A, 64), FLX_RAY_PLANES_OVERLAP_RAYS);
  expect("image inside the rays", flx_ray_image_arrays_check(A, A + 4096u, 0x10000), FLX_RAY_PLANES_OVERLAP_RAYS);
  /* the overlap rule itself */
  expect("empty ranges share nothing", flx_ray_planes_overlap(A, 0, A, 0), 0);
  expect("ranges that touch", flx_ray_planes_overlap(A, 16, A + 16u, 16), 0);
  expect("ranges that share a byte", flx_ray_planes_overlap(A, 17, A + 16u, 16), 1);
  if (failures) return 1;
  printf("ok %d\n", cases);
  return 0;
}
