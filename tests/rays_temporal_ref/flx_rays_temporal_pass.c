/*
 * flx_rays_temporal_pass.c — the oracle's own temporal pass and denoise chain over rings the caller holds.  TEST INFRASTRUCTURE ONLY, built with
 * flx_rays_temporal_ref.c into one library outside git.
 *
 * It says nothing of its own about either: it includes the oracle's source (oracle/flx_oracle_filter.c) and calls its static temporal_pass and filter_chain_u8 the
 * way render_frames does for a frame.  The rings live in the test (Python), newest first, so that moved rays, scene changes, resets and interleaved histories are
 * all expressible there.
 */
#include "../../oracle/flx_oracle_filter.c"

static uint8_t *plane_copy(const uint8_t *src, size_t bytes) {
  uint8_t *dst = (uint8_t *)malloc(bytes);
  if (dst) memcpy(dst, src, bytes);
  return dst;
}

/* rings: uint8[4][n][H][W][4], ring r (colour, colour integer part, location id, original id) slot k at rings + (r * n + k) * W * H * 4, slot 0 the frame just
 * stored, rows top-down.  original_color, id: the new frame's renderOriginalColor and renderId texels, uint8[H][W][4] (read with use_filter == 1 only).
 * out: float[H][W][4]: without the filter the pass' canvas colour, with it the chain's over the pass' RenderTexture[0] / IpRenderTexture[0], original_color, id
 * and ring 3's slot 0.  -> 0, or FLX_ERR_INVALID */
int flx_rays_temporal_pass_ref(int W, int H, int hdr, int use_filter, int n, const uint8_t *rings, const uint8_t *original_color, const uint8_t *id, float *out, int threads) {
  if (W <= 0 || H <= 0 || n < 1 || n > 16 || !rings || !out || (use_filter && (!original_color || !id))) return FLX_ERR_INVALID;
#ifdef _OPENMP
  if (threads > 0) omp_set_num_threads(threads);
#else
  (void)threads;
#endif
  const size_t bytes = (size_t)W * H * 4;
  uint8_t *slot[4][16];
  for (int r = 0; r < 4; r++) for (int k = 0; k < 16; k++) slot[r][k] = k < n ? (uint8_t *)rings + ((size_t)r * n + k) * bytes : NULL;
  History h = { slot[0], slot[1], slot[2], slot[3], n };
  if (!use_filter) {
    temporal_pass(&h, W, H, hdr, 0, NULL, NULL, out);
    return FLX_OK;
  }
  /* as render_frames: R0 / Ip0 become RenderTexture[0] / IpRenderTexture[0]; the chain frees what it is given */
  uint8_t *R0 = plane_copy(slot[0][0], bytes), *Ip0 = plane_copy(slot[1][0], bytes);
  uint8_t *O0 = plane_copy(original_color, bytes), *Id0 = plane_copy(id, bytes), *OId = plane_copy(slot[3][0], bytes);
  if (!R0 || !Ip0 || !O0 || !Id0 || !OId) { free(R0); free(Ip0); free(O0); free(Id0); free(OId); return FLX_ERR_INVALID; }
  temporal_pass(&h, W, H, hdr, 1, R0, Ip0, NULL);
  return filter_chain_u8(W, H, hdr, R0, Ip0, O0, Id0, OId, out);
}
