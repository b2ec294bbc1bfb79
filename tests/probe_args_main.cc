/* Stand-alone check of web-ray-tracer_amd/csrc/flx_probe_args.h: what the light-probe calls decide about their arguments without a device — every refusal, their
 * order, and the chunk arithmetic.  tests/test_probes_cpu.py compiles it with -fsanitize=address,undefined and runs it; it prints "ok <cases>" and returns 0, or
 * says which case failed. */
#include <math.h>
#include <stdio.h>

#include "flx_probe_args.h"

static int failures = 0, cases = 0;
static void expect(const char *name, long long got, long long want) {
  cases++;
  if (got != want) { printf("FAILED %s: got %lld, want %lld\n", name, got, want); failures++; }
}

int main(void) {
  const uint64_t A = 0x7f0000000000ull, TOP = 0xffffffffffffffffull;
  const float zero[3] = { 0.0f, 0.0f, 0.0f }, sky[3] = { 0.5f, 1.0f, 2.0f };
  const float nan0[3] = { NAN, 0.0f, 0.0f }, inf1[3] = { 0.0f, INFINITY, 0.0f }, ninf2[3] = { 0.0f, 0.0f, -INFINITY };
  /* the params, in the header's order */
  expect("params ok", flx_probe_params_check(1, 8u, 0u, zero, 0.0f), FLX_PROBE_ARGS_OK);
  expect("params ok, hits and a sky", flx_probe_params_check(1, 256u, 1u, sky, -3.0f), FLX_PROBE_ARGS_OK);
  expect("params ok, w 1", flx_probe_params_check(1, 1u, 1u, sky, 0.0f), FLX_PROBE_ARGS_OK);
  expect("params NULL", flx_probe_params_check(0, 8u, 0u, nullptr, 0.0f), FLX_PROBE_PARAMS_NULL);
  expect("params NULL before everything", flx_probe_params_check(0, 0u, 2u, nullptr, NAN), FLX_PROBE_PARAMS_NULL);
  expect("face 0", flx_probe_params_check(1, 0u, 0u, zero, 0.0f), FLX_PROBE_FACE_SIZE);
  expect("face 257", flx_probe_params_check(1, 257u, 0u, zero, 0.0f), FLX_PROBE_FACE_SIZE);
  expect("face largest", flx_probe_params_check(1, 0xffffffffu, 0u, zero, 0.0f), FLX_PROBE_FACE_SIZE);
  expect("face before order", flx_probe_params_check(1, 0u, 2u, nan0, 0.0f), FLX_PROBE_FACE_SIZE);
  expect("order 2", flx_probe_params_check(1, 8u, 2u, zero, 0.0f), FLX_PROBE_ORDER);
  expect("order 3", flx_probe_params_check(1, 8u, 3u, zero, 0.0f), FLX_PROBE_ORDER);
  expect("order top bit", flx_probe_params_check(1, 8u, 0x80000000u, zero, 0.0f), FLX_PROBE_ORDER);
  expect("order before sky", flx_probe_params_check(1, 8u, 2u, nan0, 0.0f), FLX_PROBE_ORDER);
  expect("sky NaN", flx_probe_params_check(1, 8u, 0u, nan0, 0.0f), FLX_PROBE_NOT_FINITE);
  expect("sky inf", flx_probe_params_check(1, 8u, 1u, inf1, 0.0f), FLX_PROBE_NOT_FINITE);
  expect("sky -inf", flx_probe_params_check(1, 8u, 0u, ninf2, 0.0f), FLX_PROBE_NOT_FINITE);
  expect("reserved NaN", flx_probe_params_check(1, 8u, 0u, zero, NAN), FLX_PROBE_NOT_FINITE);
  expect("reserved inf", flx_probe_params_check(1, 8u, 0u, sky, INFINITY), FLX_PROBE_NOT_FINITE);
  expect("face check 1", flx_probe_face_check(1u), FLX_PROBE_ARGS_OK);
  expect("face check 256", flx_probe_face_check(256u), FLX_PROBE_ARGS_OK);
  expect("face check 0", flx_probe_face_check(0u), FLX_PROBE_FACE_SIZE);
  expect("face check 257", flx_probe_face_check(257u), FLX_PROBE_FACE_SIZE);
  /* R, and n R against 2^32 */
  expect("R at w 1", flx_probe_rays_of(1u), 6);
  expect("R at w 8", flx_probe_rays_of(8u), 384);
  expect("R at w 256", flx_probe_rays_of(256u), 393216);
  uint32_t rays = 77u;
  expect("count 0", flx_probe_count_check(0u, 256u, &rays), FLX_PROBE_ARGS_OK);
  expect("count 0 rays", rays, 0);
  expect("count w 8", flx_probe_count_check(5u, 8u, &rays), FLX_PROBE_ARGS_OK);
  expect("count w 8 rays", rays, 1920);
  /* w = 1: R = 6; 715 827 882 x 6 = 2^32 - 4, one more probe is 2^32 + 2 */
  expect("count below 2^32", flx_probe_count_check(715827882u, 1u, &rays), FLX_PROBE_ARGS_OK);
  expect("count below 2^32 rays", rays, 4294967292ll);
  rays = 77u;
  expect("count above 2^32", flx_probe_count_check(715827883u, 1u, &rays), FLX_PROBE_RAYS);
  expect("a refusal leaves rays", rays, 77);
  /* (R = 6 w w has the factor 3 and is even: no n R is 2^32 or 2^32 - 1 itself; these are the nearest products on either side, here for the largest R) */
  expect("w 256 below 2^32", flx_probe_count_check(10922u, 256u, &rays), FLX_PROBE_ARGS_OK);
  expect("w 256 below 2^32 rays", rays, 10922ll * 393216ll);
  expect("w 256 above 2^32", flx_probe_count_check(10923u, 256u, &rays), FLX_PROBE_RAYS);
  expect("largest n, w 1", flx_probe_count_check(0xffffffffu, 1u, &rays), FLX_PROBE_RAYS);
  expect("largest n, w 256", flx_probe_count_check(0xffffffffu, 256u, nullptr), FLX_PROBE_RAYS);
  expect("no rays wanted", flx_probe_count_check(3u, 3u, nullptr), FLX_PROBE_ARGS_OK);
  /* the arrays: NULL, the end of the address space, overlap — in that order */
  expect("arrays ok", flx_probe_arrays_check(A, 64, A + 64, 144), FLX_PROBE_ARGS_OK);
  expect("arrays ok, the other way", flx_probe_arrays_check(A + 144, 64, A, 144), FLX_PROBE_ARGS_OK);
  expect("first NULL", flx_probe_arrays_check(0, 64, A, 144), FLX_PROBE_NULL);
  expect("second NULL", flx_probe_arrays_check(A, 64, 0, 144), FLX_PROBE_NULL);
  expect("NULL before wraps", flx_probe_arrays_check(0, 64, TOP - 8, 144), FLX_PROBE_NULL);
  expect("first wraps", flx_probe_arrays_check(TOP - 63, 65, A, 144), FLX_PROBE_WRAPS);
  expect("first ends at the top", flx_probe_arrays_check(TOP - 64, 64, A, 144), FLX_PROBE_ARGS_OK);
  expect("second wraps", flx_probe_arrays_check(A, 64, TOP - 100, 144), FLX_PROBE_WRAPS);
  expect("the most rays wrap", flx_probe_arrays_check(A, 16, TOP - (0xffffffffull * 32ull) + 1ull, 0xffffffffull * 32ull), FLX_PROBE_WRAPS);
  expect("wraps before overlap", flx_probe_arrays_check(TOP - 10, 64, TOP - 10, 144), FLX_PROBE_WRAPS);
  expect("the same array", flx_probe_arrays_check(A, 64, A, 144), FLX_PROBE_OVERLAP);
  expect("one byte shared", flx_probe_arrays_check(A, 64, A + 63, 144), FLX_PROBE_OVERLAP);
  expect("one byte shared, the other way", flx_probe_arrays_check(A + 143, 64, A, 144), FLX_PROBE_OVERLAP);
  expect("inside", flx_probe_arrays_check(A, 1024, A + 512, 144), FLX_PROBE_OVERLAP);
  /* chunks: max(1, 2^21 / R), a ceiling below it */
  expect("chunk w 1", flx_probe_chunk(1u, 0u), 349525);
  expect("chunk w 8", flx_probe_chunk(8u, 0u), 5461);
  expect("chunk w 16", flx_probe_chunk(16u, 0u), 1365);
  expect("chunk w 256", flx_probe_chunk(256u, 0u), 5);
  expect("chunk ceiling", flx_probe_chunk(8u, 2u), 2);
  expect("chunk ceiling above", flx_probe_chunk(8u, 6000u), 5461);
  expect("chunk ceiling equal", flx_probe_chunk(256u, 5u), 5);
  for (uint32_t w = 1; w <= FLX_PROBE_FACE_MAX; w++) {
    const uint32_t chunk = flx_probe_chunk(w, 0u);
    expect("a chunk has a probe", chunk >= 1u, 1);
    expect("a chunk's rays fit a slab", (uint64_t)chunk * flx_probe_rays_of(w) <= FLX_TRACE_SLAB_RAYS, 1);
    expect("one more probe would not", (uint64_t)(chunk + 1u) * flx_probe_rays_of(w) > FLX_TRACE_SLAB_RAYS, 1);
  }
  expect("chunks of 5 by 2", flx_probe_chunks(5u, 2u), 3);
  expect("chunks of 4 by 2", flx_probe_chunks(4u, 2u), 2);
  expect("chunks of 1", flx_probe_chunks(1u, 5461u), 1);
  expect("chunks of the largest n", flx_probe_chunks(0xffffffffu, 1u), 0xffffffffll);
  expect("chunks of the largest n by 2", flx_probe_chunks(0xffffffffu, 2u), 0x80000000ll);
  expect("reduce groups of 1", flx_probe_reduce_groups(1u), 1);
  expect("reduce groups of 4", flx_probe_reduce_groups(4u), 1);
  expect("reduce groups of 5", flx_probe_reduce_groups(5u), 2);
  expect("reduce groups of the largest n", flx_probe_reduce_groups(0xffffffffu), 0x40000000ll);
  expect("row bytes", FLX_PROBE_POSITION_BYTES + FLX_PROBE_SH_BYTES, 160);
  if (failures) return 1;
  printf("ok %d\n", cases);
  return 0;
}
