/* flx_texture_args.h — what flx_textures_upload[_device] and flx_texture_update[_device] decide about their arguments before they ask the device anything, and the
 * atlas rule's integers: plain C++, no HIP, so that a stand-alone program can hold it under the sanitizers (tests/texture_args_main.cc). */
#ifndef FLX_TEXTURE_ARGS_H
#define FLX_TEXTURE_ARGS_H

#include <stddef.h>
#include <stdint.h>

#include "flexlight_hip_debug.h"      /* flx_image, FLX_IMAGE_* */

#define FLX_ATLAS_MAX_WIDTH 2048u     /* the reference's canvas width: tw = floor(2048 / cell_w) cells in a row */

/* in the order the calls say them; the three rules of an image in the order they are met within it */
enum flx_textures_refusal {
  FLX_TEXTURES_ARGS_OK = 0,
  FLX_TEXTURES_WHICH,                /* which is not 0, 1 or 2 */
  FLX_TEXTURES_NULL,                 /* images NULL with n > 0; the update's image NULL */
  FLX_TEXTURES_CELL_W,               /* cell_w 0 or above 2048 */
  FLX_TEXTURES_CELL_H,               /* cell_h 0 */
  FLX_TEXTURES_NOT_BUILT,            /* update: no atlas built by flx_textures_upload* is resident */
  FLX_TEXTURES_INDEX,                /* update: index >= n */
  FLX_TEXTURES_PIXELS,               /* an image's pixels are NULL */
  FLX_TEXTURES_DIMENSION,            /* an image's width or height is 0 */
  FLX_TEXTURES_FORMAT,               /* an image's format is neither FLX_IMAGE_RGBA8 nor FLX_IMAGE_RGBA32F */
  FLX_TEXTURES_TALL,                 /* cell_h * n is 2^31 or more: the atlas' height and the rule's 2y + 1 would leave 32 bits */
  FLX_TEXTURES_REFUSALS
};

static const char *const FLX_TEXTURES_UPLOAD_REFUSAL[FLX_TEXTURES_REFUSALS] = {
  "", "flx_textures_upload: which must be 0, 1 or 2", "flx_textures_upload: images is NULL", "flx_textures_upload: cell_w must be 1 .. 2048",
  "flx_textures_upload: cell_h is 0", "", "", "flx_textures_upload: an image's pixels are NULL", "flx_textures_upload: an image's width or height is 0",
  "flx_textures_upload: an image's format is neither FLX_IMAGE_RGBA8 nor FLX_IMAGE_RGBA32F", "flx_textures_upload: the atlas would be 2^31 texels high or more" };
static const char *const FLX_TEXTURE_UPDATE_REFUSAL[FLX_TEXTURES_REFUSALS] = {
  "", "flx_texture_update: which must be 0, 1 or 2", "flx_texture_update: image is NULL", "", "",
  "flx_texture_update: no atlas built by flx_textures_upload is resident", "flx_texture_update: index is not a cell of the atlas",
  "flx_texture_update: the image's pixels are NULL", "flx_texture_update: the image's width or height is 0",
  "flx_texture_update: the image's format is neither FLX_IMAGE_RGBA8 nor FLX_IMAGE_RGBA32F", "" };

/* one image's three rules */
static inline enum flx_textures_refusal flx_image_check(const flx_image *image) {
  if (!image->pixels) return FLX_TEXTURES_PIXELS;
  if (image->width == 0u || image->height == 0u) return FLX_TEXTURES_DIMENSION;
  if (image->format != FLX_IMAGE_RGBA8 && image->format != FLX_IMAGE_RGBA32F) return FLX_TEXTURES_FORMAT;
  return FLX_TEXTURES_ARGS_OK;
}

/* what an upload says before it looks at an image (n == 0 is "none": nothing else is looked at) */
static inline enum flx_textures_refusal flx_textures_cells_check(int which, int have_images, uint32_t n, uint32_t cell_w, uint32_t cell_h) {
  if (which < 0 || which > 2) return FLX_TEXTURES_WHICH;
  if (n == 0u) return FLX_TEXTURES_ARGS_OK;
  if (!have_images) return FLX_TEXTURES_NULL;
  if (cell_w == 0u || cell_w > FLX_ATLAS_MAX_WIDTH) return FLX_TEXTURES_CELL_W;
  if (cell_h == 0u) return FLX_TEXTURES_CELL_H;
  return FLX_TEXTURES_ARGS_OK;
}

/* flx_textures_upload's arguments; *offender <- the image that is refused */
static inline enum flx_textures_refusal flx_textures_upload_check(int which, const flx_image *images, uint32_t n, uint32_t cell_w, uint32_t cell_h, uint32_t *offender) {
  enum flx_textures_refusal r = flx_textures_cells_check(which, images != NULL, n, cell_w, cell_h);
  if (r != FLX_TEXTURES_ARGS_OK) return r;
  for (uint32_t i = 0; i < n; i++)
    if ((r = flx_image_check(images + i)) != FLX_TEXTURES_ARGS_OK) { if (offender) *offender = i; return r; }
  if ((uint64_t)cell_h * n >= 0x80000000ull) return FLX_TEXTURES_TALL;
  return FLX_TEXTURES_ARGS_OK;
}

/* flx_texture_update's; cells: how many cells the resident atlas `which` was built with by flx_textures_upload* (0: none, or a prebuilt atlas) */
static inline enum flx_textures_refusal flx_texture_update_check(int which, uint32_t cells, uint32_t index, const flx_image *image) {
  if (which < 0 || which > 2) return FLX_TEXTURES_WHICH;
  if (!image) return FLX_TEXTURES_NULL;
  if (cells == 0u) return FLX_TEXTURES_NOT_BUILT;
  if (index >= cells) return FLX_TEXTURES_INDEX;
  return flx_image_check(image);
}

/* bytes of a texel; of an image's tight rows, 0 where they do not fit 64 bits */
static inline uint32_t flx_image_texel_bytes(uint32_t format) { return format == FLX_IMAGE_RGBA32F ? 16u : 4u; }
static inline uint64_t flx_image_bytes(const flx_image *image) {
  const uint64_t texels = (uint64_t)image->width * image->height;      /* (< 2^64) */
  const uint64_t each = flx_image_texel_bytes(image->format);
  return texels > UINT64_MAX / each ? 0u : texels * each;
}

/* the atlas rule (js/sceneFile.js: buildAtlas): cells in a row, the atlas' size, a cell's origin */
static inline uint32_t flx_atlas_cells_per_row(uint32_t cell_w) { return FLX_ATLAS_MAX_WIDTH / cell_w; }
static inline uint32_t flx_atlas_width(uint32_t cell_w) { return cell_w * flx_atlas_cells_per_row(cell_w); }
static inline uint32_t flx_atlas_height(uint32_t cell_h, uint32_t n) { return cell_h * n; }      /* (the reference's too-tall canvas: fetchTexVal divides by it) */
/* the source texel of destination texel d of `size`: floor((2d + 1) * s / (2 * size)), = Math.floor((d + 0.5) * s / size); 2d + 1 < 2^32 */
static inline uint32_t flx_atlas_source_texel(uint32_t d, uint32_t s, uint32_t size) { return (uint32_t)(((uint64_t)(2u * d + 1u) * s) / (2ull * size)); }

#endif
