/* Stand-alone check of flx_surface_args.h (web-ray-tracer_amd/csrc): what flx_rays_surface_device and flx_frame_surface_device decide about their arguments without a
 * device.  tests/test_surface_ref_cpu.py compiles it with -fsanitize=address,undefined and runs it; it prints "ok <cases>" and returns 0, or says which case failed. */
#include <stdio.h>

#include "flx_surface_args.h"

static int failures = 0, cases = 0;
static void expect(const char *name, long long got, long long want) {
  cases++;
  if (got != want) { printf("FAILED %s: got %lld, want %lld\n", name, got, want); failures++; }
}

int main(void) {
  const uint64_t A = 0x7f0000000000ull, TOP = UINT64_MAX;
  const uint32_t N = 0xffffffffu;
  uint64_t bytes = 0;
  /* fields and texture_width, in the order they are said */
  expect("fields 0", flx_surface_fields_check(0u, 32), FLX_SURFACE_FIELDS_NONE);
  expect("fields 0 before texture width", flx_surface_fields_check(0u, 0), FLX_SURFACE_FIELDS_NONE);
  expect("bit 256", flx_surface_fields_check(256u, 32), FLX_SURFACE_FIELDS_UNKNOWN);
  expect("bit 256 beside known ones", flx_surface_fields_check(256u | 255u, 32), FLX_SURFACE_FIELDS_UNKNOWN);
  expect("the top bit", flx_surface_fields_check(0x80000001u, 32), FLX_SURFACE_FIELDS_UNKNOWN);
  expect("unknown bit before texture width", flx_surface_fields_check(512u, -1), FLX_SURFACE_FIELDS_UNKNOWN);
  expect("texture width 0", flx_surface_fields_check(1u, 0), FLX_SURFACE_TEXTURE_WIDTH);
  expect("texture width most negative", flx_surface_fields_check(255u, INT32_MIN), FLX_SURFACE_TEXTURE_WIDTH);
  expect("all planes", flx_surface_fields_check(255u, 1), FLX_SURFACE_ARGS_OK);
  expect("texture width largest", flx_surface_fields_check(128u, INT32_MAX), FLX_SURFACE_ARGS_OK);
  for (uint32_t bit = 1u; bit <= 128u; bit <<= 1) expect("a single plane", flx_surface_fields_check(bit, 32), FLX_SURFACE_ARGS_OK);
  /* planes and where they start */
  expect("planes of 0", flx_surface_planes(0u), 0);
  expect("planes of 255", flx_surface_planes(255u), 8);
  expect("planes of HIT | ALBEDO", flx_surface_planes(1u | 32u), 2);
  expect("planes of all bits", flx_surface_planes(0xffffffffu), 32);
  expect("index of HIT", flx_surface_plane_index(255u, 1u), 0);
  expect("index of TPO among all", flx_surface_plane_index(255u, 128u), 7);
  expect("index of ALBEDO in HIT | ALBEDO", flx_surface_plane_index(1u | 32u, 32u), 1);
  expect("index of TPO alone", flx_surface_plane_index(128u, 128u), 0);
  expect("index of RME in NORMAL | RME | TPO", flx_surface_plane_index(8u | 64u | 128u, 64u), 1);
  /* a frame's params */
  expect("no params", flx_surface_frame_check(0, 64, 48, 0, 0, 0), FLX_SURFACE_PARAMS_NULL);
  expect("width 0", flx_surface_frame_check(1, 0, 48, 0, 0, 0), FLX_SURFACE_SIZE);
  expect("height 0", flx_surface_frame_check(1, 64, 0, 0, 0, 0), FLX_SURFACE_SIZE);
  expect("size before tile", flx_surface_frame_check(1, 0, 0, 8, 1, 2), FLX_SURFACE_SIZE);
  expect("0/0/0", flx_surface_frame_check(1, 64, 48, 0, 0, 0), FLX_SURFACE_ARGS_OK);
  expect("x/0/1", flx_surface_frame_check(1, 64, 48, 8, 0, 1), FLX_SURFACE_ARGS_OK);
  expect("0/0/1", flx_surface_frame_check(1, 64, 48, 0, 0, 1), FLX_SURFACE_ARGS_OK);
  expect("largest x/0/1", flx_surface_frame_check(1, 64, 48, N, 0, 1), FLX_SURFACE_ARGS_OK);
  expect("8/0/2", flx_surface_frame_check(1, 64, 48, 8, 0, 2), FLX_SURFACE_TILE);
  expect("8/1/2", flx_surface_frame_check(1, 64, 48, 8, 1, 2), FLX_SURFACE_TILE);
  expect("8/0/0", flx_surface_frame_check(1, 64, 48, 8, 0, 0), FLX_SURFACE_TILE);
  expect("0/1/0", flx_surface_frame_check(1, 64, 48, 0, 1, 0), FLX_SURFACE_TILE);
  expect("8/1/1", flx_surface_frame_check(1, 64, 48, 8, 1, 1), FLX_SURFACE_TILE);
  expect("0/0/most", flx_surface_frame_check(1, 64, 48, 0, 0, N), FLX_SURFACE_TILE);
  expect("65535 x 65537 pixels", flx_surface_frame_check(1, 65535u, 65537u, 0, 0, 0), FLX_SURFACE_ARGS_OK);
  expect("65536 x 65536 pixels", flx_surface_frame_check(1, 65536u, 65536u, 0, 0, 0), FLX_SURFACE_PIXELS);
  expect("the largest canvas", flx_surface_frame_check(1, N, N, 0, 0, 0), FLX_SURFACE_PIXELS);
  expect("one row of most pixels", flx_surface_frame_check(1, N, 1, 0, 0, 1), FLX_SURFACE_ARGS_OK);
  /* the arrays: NULL */
  expect("rays NULL", flx_surface_arrays_check(1, 0, A, 16, 255u, &bytes), FLX_SURFACE_NULL);
  expect("out NULL", flx_surface_arrays_check(1, A, 0, 16, 255u, &bytes), FLX_SURFACE_NULL);
  expect("a frame's out NULL", flx_surface_arrays_check(0, 0, 0, 16, 255u, &bytes), FLX_SURFACE_NULL);
  expect("a frame has no rays", flx_surface_arrays_check(0, 0, A, 16, 255u, &bytes), FLX_SURFACE_ARGS_OK);
  expect("the bytes of 16 rows of 8 planes", (long long)bytes, 16 * 16 * 8);
  expect("no place for the bytes", flx_surface_arrays_check(0, 0, A, 16, 255u, (uint64_t *)0), FLX_SURFACE_ARGS_OK);
  /* bytes: popcount(fields) * n * 16 */
  expect("one plane", flx_surface_arrays_check(1, A, A + 0x100000, 100, 32u, &bytes), FLX_SURFACE_ARGS_OK);
  expect("the bytes of one plane", (long long)bytes, 1600);
  expect("two planes", flx_surface_arrays_check(1, A, A + 0x100000, 100, 1u | 32u, &bytes), FLX_SURFACE_ARGS_OK);
  expect("the bytes of two planes", (long long)bytes, 3200);
  expect("largest n, all planes", flx_surface_arrays_check(1, A, A + 0x10000000000ull, N, 255u, &bytes), FLX_SURFACE_ARGS_OK);
  expect("the bytes of the largest call", bytes == (uint64_t)N * 128u, 1);
  /* address + bytes leaving 64 bits */
  expect("out ends at the top", flx_surface_arrays_check(0, 0, TOP - 16u, 1, 1u, &bytes), FLX_SURFACE_ARGS_OK);
  expect("out wraps", flx_surface_arrays_check(0, 0, TOP - 15u, 1, 1u, &bytes), FLX_SURFACE_WRAPS);
  expect("the second plane wraps", flx_surface_arrays_check(0, 0, TOP - 16u, 1, 3u, &bytes), FLX_SURFACE_WRAPS);
  expect("eight planes end at the top", flx_surface_arrays_check(0, 0, TOP - (uint64_t)N * 128u, N, 255u, &bytes), FLX_SURFACE_ARGS_OK);
  expect("eight planes wrap", flx_surface_arrays_check(0, 0, TOP - (uint64_t)N * 128u + 1u, N, 255u, &bytes), FLX_SURFACE_WRAPS);
  expect("rays end at the top", flx_surface_arrays_check(1, TOP - 32u, A, 1, 1u, &bytes), FLX_SURFACE_ARGS_OK);
  expect("rays wrap", flx_surface_arrays_check(1, TOP - 31u, A, 1, 1u, &bytes), FLX_SURFACE_WRAPS);
  expect("a frame's rays are not looked at", flx_surface_arrays_check(0, TOP - 31u, A, 1, 1u, &bytes), FLX_SURFACE_ARGS_OK);
  /* overlap: the rays' n * 32 bytes against the planes' popcount(fields) * n * 16 */
  expect("same array", flx_surface_arrays_check(1, A, A, 1, 1u, &bytes), FLX_SURFACE_OVERLAP);
  expect("one plane right behind the rays", flx_surface_arrays_check(1, A, A + 64u * 32u, 64, 1u, &bytes), FLX_SURFACE_ARGS_OK);
  expect("one plane starts in the last ray", flx_surface_arrays_check(1, A, A + 64u * 32u - 1u, 64, 1u, &bytes), FLX_SURFACE_OVERLAP);
  expect("rays right behind one plane", flx_surface_arrays_check(1, A + 64u * 16u, A, 64, 1u, &bytes), FLX_SURFACE_ARGS_OK);
  expect("rays start in one plane's last byte", flx_surface_arrays_check(1, A + 64u * 16u - 1u, A, 64, 1u, &bytes), FLX_SURFACE_OVERLAP);
  expect("rays right behind eight planes", flx_surface_arrays_check(1, A + 64u * 128u, A, 64, 255u, &bytes), FLX_SURFACE_ARGS_OK);
  expect("rays inside the eighth plane", flx_surface_arrays_check(1, A + 64u * 128u - 16u, A, 64, 255u, &bytes), FLX_SURFACE_OVERLAP);
  expect("rays behind two planes, where a third would be", flx_surface_arrays_check(1, A + 64u * 32u, A, 64, 1u | 32u, &bytes), FLX_SURFACE_ARGS_OK);
  expect("the same place with three planes", flx_surface_arrays_check(1, A + 64u * 32u, A, 64, 1u | 32u | 64u, &bytes), FLX_SURFACE_OVERLAP);
  expect("rays inside the planes", flx_surface_arrays_check(1, A + 4096u, A, 0x10000, 255u, &bytes), FLX_SURFACE_OVERLAP);
  expect("planes inside the rays", flx_surface_arrays_check(1, A, A + 4096u, 0x10000, 1u, &bytes), FLX_SURFACE_OVERLAP);
  expect("touching at the top", flx_surface_arrays_check(1, TOP - 48u, TOP - 16u, 1, 1u, &bytes), FLX_SURFACE_ARGS_OK);
  expect("huge n reaches the planes", flx_surface_arrays_check(1, A, A + (uint64_t)N * 32u - 1u, N, 1u, &bytes), FLX_SURFACE_OVERLAP);
  expect("huge n ends in front of them", flx_surface_arrays_check(1, A, A + (uint64_t)N * 32u, N, 1u, &bytes), FLX_SURFACE_ARGS_OK);
  if (failures) return 1;
  printf("ok %d\n", cases);
  return 0;
}
