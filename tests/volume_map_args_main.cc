/* Stand-alone check of web-ray-tracer_amd/csrc/flx_volume_map_args.h: what the directional-visibility calls decide about a map and a maps array without a device —
 * every refusal of a map and their order, m and k at their ends, n_probes m m on either side of 2^31, and the maps array against every other array of its call.
 * tests/test_volume_map_cpu.py compiles it with -fsanitize=address,undefined and runs it; it prints "ok <cases>" and returns 0, or says which case failed. */
#include <stdio.h>

#include "flx_volume_map_args.h"

static int failures = 0, cases = 0;
static void expect(const char *name, long long got, long long want) {
  cases++;
  if (got != want) { printf("FAILED %s: got %lld, want %lld\n", name, got, want); failures++; }
}

static flx_volume_map good(void) {
  flx_volume_map m = { 8u, 5u, { 0u, 0u } };
  return m;
}

int main(void) {
  const uint64_t A = 0x7f0000000000ull, TOP = 0xffffffffffffffffull;
  flx_volume_map m = good();
  /* the map, in the header's order */
  expect("map ok", flx_volume_map_check(&m), FLX_VOLUME_MAP_ARGS_OK);
  expect("map NULL", flx_volume_map_check(nullptr), FLX_VOLUME_MAP_NULL);
  m = good(); m.size = 0u;
  expect("size 0", flx_volume_map_check(&m), FLX_VOLUME_MAP_SIZE);
  m = good(); m.size = 1u;
  expect("size 1", flx_volume_map_check(&m), FLX_VOLUME_MAP_ARGS_OK);
  m = good(); m.size = 16u;
  expect("size 16", flx_volume_map_check(&m), FLX_VOLUME_MAP_ARGS_OK);
  m = good(); m.size = 17u;
  expect("size 17", flx_volume_map_check(&m), FLX_VOLUME_MAP_SIZE);
  m = good(); m.size = 0xffffffffu;
  expect("size 2^32 - 1", flx_volume_map_check(&m), FLX_VOLUME_MAP_SIZE);
  m = good(); m.size = 65536u;
  expect("size 2^16 (its square is 0 in 32 bits)", flx_volume_map_check(&m), FLX_VOLUME_MAP_SIZE);
  m = good(); m.size = 0u; m.sharpness = 9u;
  expect("size before sharpness", flx_volume_map_check(&m), FLX_VOLUME_MAP_SIZE);
  m = good(); m.sharpness = 0u;
  expect("sharpness 0", flx_volume_map_check(&m), FLX_VOLUME_MAP_ARGS_OK);
  m = good(); m.sharpness = 8u;
  expect("sharpness 8", flx_volume_map_check(&m), FLX_VOLUME_MAP_ARGS_OK);
  m = good(); m.sharpness = 9u;
  expect("sharpness 9", flx_volume_map_check(&m), FLX_VOLUME_MAP_SHARPNESS);
  m = good(); m.sharpness = 0x80000000u;
  expect("sharpness top bit", flx_volume_map_check(&m), FLX_VOLUME_MAP_SHARPNESS);
  m = good(); m.sharpness = 9u; m.reserved[0] = 1u;
  expect("sharpness before reserved", flx_volume_map_check(&m), FLX_VOLUME_MAP_SHARPNESS);
  for (int i = 0; i < 2; i++) {
    m = good(); m.reserved[i] = 1u;
    expect("reserved 1", flx_volume_map_check(&m), FLX_VOLUME_MAP_RESERVED);
    m = good(); m.reserved[i] = 0x80000000u;
    expect("reserved top bit", flx_volume_map_check(&m), FLX_VOLUME_MAP_RESERVED);
  }
  /* n_probes m m on either side of 2^31 */
  uint32_t rows = 77u;
  expect("no probes", flx_volume_map_rows_check(0u, 16u, &rows), FLX_VOLUME_MAP_ARGS_OK);
  expect("no rows", rows, 0);
  expect("no rows wanted", flx_volume_map_rows_check(3u, 4u, nullptr), FLX_VOLUME_MAP_ARGS_OK);
  expect("3 probes of 4 x 4", flx_volume_map_rows_check(3u, 4u, &rows), FLX_VOLUME_MAP_ARGS_OK);
  expect("48 rows", rows, 48);
  expect("2^31 - 1 probes of 1 x 1", flx_volume_map_rows_check(0x7fffffffu, 1u, &rows), FLX_VOLUME_MAP_ARGS_OK);
  expect("2^31 - 1 rows", rows, 0x7fffffffll);
  rows = 77u;
  expect("2^31 probes of 1 x 1", flx_volume_map_rows_check(0x80000000u, 1u, &rows), FLX_VOLUME_MAP_ROWS);
  expect("a refusal leaves rows", rows, 77);
  expect("2^23 - 1 probes of 16 x 16", flx_volume_map_rows_check(0x7fffffu, 16u, &rows), FLX_VOLUME_MAP_ARGS_OK);
  expect("2^31 - 256 rows", rows, 0x7fffff00ll);
  expect("2^23 probes of 16 x 16", flx_volume_map_rows_check(0x800000u, 16u, &rows), FLX_VOLUME_MAP_ROWS);
  expect("2^29 - 1 probes of 2 x 2", flx_volume_map_rows_check(0x1fffffffu, 2u, &rows), FLX_VOLUME_MAP_ARGS_OK);
  expect("2^29 probes of 2 x 2", flx_volume_map_rows_check(0x20000000u, 2u, &rows), FLX_VOLUME_MAP_ROWS);
  expect("2^24 probes of 16 x 16 (a 32-bit product is 0)", flx_volume_map_rows_check(0x1000000u, 16u, &rows), FLX_VOLUME_MAP_ROWS);
  expect("2^32 - 1 probes of 16 x 16", flx_volume_map_rows_check(0xffffffffu, 16u, &rows), FLX_VOLUME_MAP_ROWS);
  expect("2^30 + 1 probes of 2 x 2 (a 32-bit product is 4)", flx_volume_map_rows_check(0x40000001u, 2u, &rows), FLX_VOLUME_MAP_ROWS);
  expect("the bytes of a row", flx_volume_map_bytes(1u), 16);
  expect("the most bytes", flx_volume_map_bytes(0x7fffffffu), 0x7fffffffll * 16ll);
  expect("one row short", flx_volume_map_bytes(48u) - flx_volume_map_bytes(47u), FLX_VOLUME_MAP_ROW_BYTES);
  /* the maps array against one to four others: NULL, the end of the address space, overlap — in that order; every pairing */
  {
    const uint64_t at[4] = { A, A + 3456, A + 3456 + 16000, A + 3456 + 32000 }, bytes[4] = { 3456, 16000, 16000, 16000 };
    const uint64_t maps = A + 3456 + 48000, maps_bytes = 768;
    for (int k = 0; k <= 4; k++) {
      expect("maps ok", flx_volume_maps_check(maps, maps_bytes, at, bytes, k), FLX_VOLUME_MAP_ARGS_OK);
      expect("maps NULL", flx_volume_maps_check(0u, maps_bytes, at, bytes, k), FLX_VOLUME_MAPS_NULL);
      expect("maps wrap by a byte", flx_volume_maps_check(TOP - maps_bytes + 1, maps_bytes, at, bytes, k), FLX_VOLUME_MAPS_WRAPS);
      expect("maps end at the top", flx_volume_maps_check(TOP - maps_bytes, maps_bytes, at, bytes, k), FLX_VOLUME_MAP_ARGS_OK);
      for (int j = 0; j < 4; j++) {
        const long long want = j < k ? FLX_VOLUME_MAPS_OVERLAP : FLX_VOLUME_MAP_ARGS_OK;
        expect("the same array", flx_volume_maps_check(at[j], maps_bytes, at, bytes, k), want);
        expect("the last byte shared", flx_volume_maps_check(at[j] + bytes[j] - 1, maps_bytes, at, bytes, k) != FLX_VOLUME_MAP_ARGS_OK, j < k || j + 1 < k);
        expect("inside", flx_volume_maps_check(at[j] + 16, 16, at, bytes, k), want);
        expect("around", flx_volume_maps_check(at[j] - (j ? 0 : 16), bytes[j] + 32, at, bytes, k) != FLX_VOLUME_MAP_ARGS_OK, j < k || j + 1 < k);
      }
    }
    expect("NULL before overlap", flx_volume_maps_check(0u, TOP, at, bytes, 4), FLX_VOLUME_MAPS_NULL);
    expect("wraps before overlap", flx_volume_maps_check(A, TOP, at, bytes, 4), FLX_VOLUME_MAPS_WRAPS);
    expect("back to back before", flx_volume_maps_check(A - 768, 768, at, bytes, 4), FLX_VOLUME_MAP_ARGS_OK);
    expect("a byte more before", flx_volume_maps_check(A - 768, 769, at, bytes, 4), FLX_VOLUME_MAPS_OVERLAP);
    expect("back to back behind", flx_volume_maps_check(at[3] + bytes[3], 768, at, bytes, 4), FLX_VOLUME_MAP_ARGS_OK);
    expect("a byte less behind", flx_volume_maps_check(at[3] + bytes[3] - 1, 768, at, bytes, 4), FLX_VOLUME_MAPS_OVERLAP);
  }
  /* k_probe_map's grid */
  expect("bin groups of 1", flx_volume_map_bin_groups(1u), 1);
  expect("bin groups of 4", flx_volume_map_bin_groups(4u), 1);
  expect("bin groups of 5", flx_volume_map_bin_groups(5u), 2);
  expect("bin groups of 16", flx_volume_map_bin_groups(16u), 16);
  expect("launches of 0", flx_volume_map_launches(0u), 0);
  expect("launches of 1", flx_volume_map_launches(1u), 1);
  expect("launches of 32768", flx_volume_map_launches(32768u), 1);
  expect("launches of 32769", flx_volume_map_launches(32769u), 2);
  expect("launches of the most probes", flx_volume_map_launches(0x7fffffffu), 65536);
  if (failures) return 1;
  printf("ok %d\n", cases);
  return 0;
}
