/*
 * flexlight_napi.cc — thin N-API shim over the C ABI of libflexlight_hip.so (include/flexlight_hip.h).
 *
 * One JS function per C entry point, typed arrays in, typed arrays out, no logic: the JavaScript
 * renderer (js/pathtracerHIP.js) is to this addon what modules/pathtracerWGL2.js is to the WebGL2
 * context.  A non-zero flx_status becomes a JS exception carrying flx_last_error().  Memory: every
 * typed array stays owned by JS; the library copies in during the call (napi_get_typedarray_info
 * gives the backing store, nothing is retained).  Built with plain g++ against /usr/include/node
 * (no node-gyp, no network): napi/Makefile.
 */
#include <node_api.h>
#include <hip/hip_runtime_api.h>      /* bakeVolume's SH rows stay in device memory between calls: hipMalloc, hipMemcpy, hipFree and nothing else */

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "flexlight_hip.h"
#include "flexlight_hip_debug.h"      /* flx_scene_update */

#define NAPI_OK(env, call)                                                     \
  do {                                                                         \
    if ((call) != napi_ok) { napi_throw_error((env), nullptr, "N-API call failed: " #call); return nullptr; } \
  } while (0)

static napi_value fail(napi_env env, flx_context *ctx, const char *what, flx_status rc) {
  std::string msg = std::string(what) + " failed (" + std::to_string(rc) + "): " + flx_last_error(ctx);
  napi_throw_error(env, nullptr, msg.c_str());
  return nullptr;
}

static bool get_args(napi_env env, napi_callback_info info, size_t want, napi_value *argv) {
  size_t argc = want;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < want) {
    napi_throw_type_error(env, nullptr, "wrong number of arguments");
    return false;
  }
  return true;
}

/* What a context handle points to: the context and the ArrayBuffers handed out over its pinned frame slots (frameEnd).  Those
 * buffers are views of memory the LIBRARY owns — freed by halt(), re-allocated when a larger frame needs a bigger slot, re-used
 * by the frame after the next — so the box keeps a weak reference to each and DETACHES it (length 0, no pointer) the moment its
 * memory stops being that frame's: a JavaScript holder of an old frame then reads an empty array, never freed memory. */
struct CtxBox {
  flx_context *ctx = nullptr;              /* first member: a handle also reads as flx_context ** */
  int device = 0;                          /* the GPU it was created on (bakeVolume allocates there) */
  struct View { const void *ptr; napi_ref ref; };
  std::vector<View> views;
  bool busy = false;                       /* a frameEndAsync is waiting for the GPU on a worker thread: the context is that thread's until its promise settles */
};
static void detach_view(napi_env env, CtxBox::View &v) {
  napi_value buf = nullptr;
  if (napi_get_reference_value(env, v.ref, &buf) == napi_ok && buf) (void)napi_detach_arraybuffer(env, buf);      /* (collected already: nothing to do) */
  napi_delete_reference(env, v.ref);
}
/* detach the views for which keep(ptr) is false */
template <typename Keep> static void detach_views(napi_env env, CtxBox *box, Keep keep) {
  size_t n = 0;
  for (auto &v : box->views) { if (keep(v.ptr)) box->views[n++] = v; else detach_view(env, v); }
  box->views.resize(n);
}
static CtxBox *get_box(napi_env env, napi_value v) {
  void *p = nullptr;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p) { napi_throw_type_error(env, nullptr, "expected a context handle"); return nullptr; }
  CtxBox *box = static_cast<CtxBox *>(p);
  if (!box->ctx) { napi_throw_error(env, nullptr, "context was halted"); return nullptr; }
  if (box->busy) { napi_throw_error(env, nullptr, "a frameEndAsync of this context is pending: await it first"); return nullptr; }
  return box;
}
static flx_context *get_ctx(napi_env env, napi_value v) {
  CtxBox *box = get_box(env, v);
  return box ? box->ctx : nullptr;
}

/* typed array -> pointer + element count; null / undefined -> nullptr, 0 */
static bool typed(napi_env env, napi_value v, napi_typedarray_type want, void **data, size_t *len) {
  napi_valuetype t;
  napi_typeof(env, v, &t);
  if (t == napi_null || t == napi_undefined) { *data = nullptr; *len = 0; return true; }
  bool is = false;
  napi_is_typedarray(env, v, &is);
  napi_typedarray_type type;
  if (!is || napi_get_typedarray_info(env, v, &type, len, data, nullptr, nullptr) != napi_ok ||
      (type != want && !(want == napi_uint8_array && type == napi_uint8_clamped_array))) {
    napi_throw_type_error(env, nullptr, "expected a typed array of the right element type");
    return false;
  }
  return true;
}

static bool num(napi_env env, napi_value obj, const char *key, double *out, bool required = true) {
  napi_value v;
  bool has = false;
  napi_has_named_property(env, obj, key, &has);
  if (!has) {
    if (required) { napi_throw_type_error(env, nullptr, (std::string("frame params: missing ") + key).c_str()); return false; }
    return true;
  }
  napi_get_named_property(env, obj, key, &v);
  napi_valuetype t;
  napi_typeof(env, v, &t);
  if (t == napi_boolean) { bool b; napi_get_value_bool(env, v, &b); *out = b ? 1.0 : 0.0; return true; }
  if (napi_get_value_double(env, v, out) != napi_ok) { napi_throw_type_error(env, nullptr, (std::string("frame params: ") + key + " is not a number").c_str()); return false; }
  return true;
}

static bool floats(napi_env env, napi_value obj, const char *key, float *dst, size_t n) {
  napi_value v;
  if (napi_get_named_property(env, obj, key, &v) != napi_ok) return false;
  for (size_t i = 0; i < n; i++) {
    napi_value e; double d;
    if (napi_get_element(env, v, (uint32_t)i, &e) != napi_ok || napi_get_value_double(env, e, &d) != napi_ok) {
      napi_throw_type_error(env, nullptr, (std::string("frame params: ") + key + " needs " + std::to_string(n) + " numbers").c_str());
      return false;
    }
    dst[i] = (float)d;
  }
  return true;
}

static void finalize_ctx(napi_env env, void *data, void *) {
  CtxBox *box = static_cast<CtxBox *>(data);
  for (auto &v : box->views) napi_delete_reference(env, v.ref);      /* (finalizers may not touch JS values; whoever still holds a view keeps the handle alive through its frame object) */
  if (box->ctx) flx_context_destroy(box->ctx);
  delete box;
}

/* createContext(device) -> handle */
static napi_value CreateContext(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  if (!get_args(env, info, 1, argv)) return nullptr;
  int32_t device = 0;
  NAPI_OK(env, napi_get_value_int32(env, argv[0], &device));
  flx_context *ctx = nullptr;
  flx_status rc = flx_context_create(device, &ctx);
  if (rc != FLX_OK) return fail(env, nullptr, "flx_context_create", rc);
  napi_value ext;
  CtxBox *box = new CtxBox();
  box->ctx = ctx;
  box->device = device;
  NAPI_OK(env, napi_create_external(env, box, finalize_ctx, nullptr, &ext));
  return ext;
}

/* destroyContext(handle): halt() */
static napi_value DestroyContext(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  if (!get_args(env, info, 1, argv)) return nullptr;
  void *p = nullptr;
  if (napi_get_value_external(env, argv[0], &p) == napi_ok && p) {
    CtxBox *box = static_cast<CtxBox *>(p);
    if (box->busy) { napi_throw_error(env, nullptr, "destroyContext: a frameEndAsync is pending: await it first"); return nullptr; }
    detach_views(env, box, [](const void *) { return false; });      /* the pinned slots are about to be freed */
    if (box->ctx) { flx_context_destroy(box->ctx); box->ctx = nullptr; }
  }
  return nullptr;
}

/* uploadScene(handle, geometry Float32Array, attributes Float32Array, ids Int32Array) */
static napi_value UploadScene(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  void *g, *a, *ids; size_t ng, na, nids;
  if (!typed(env, argv[1], napi_float32_array, &g, &ng) || !typed(env, argv[2], napi_float32_array, &a, &na) ||
      !typed(env, argv[3], napi_int32_array, &ids, &nids)) return nullptr;
  if (ng % 12 != 0 || na / 28 != ng / 12 || na % 28 != 0) { napi_throw_range_error(env, nullptr, "geometry needs 12 and attributes 28 floats per entry"); return nullptr; }
  flx_status rc = flx_scene_upload(ctx, (const float *)g, (const float *)a, (uint32_t)(ng / 12), (const int32_t *)ids, (uint32_t)nids);
  if (rc != FLX_OK) return fail(env, ctx, "flx_scene_upload", rc);
  return nullptr;
}

/* the arguments of updateSceneRows / groupUpdateSceneRows after the handle: first, geometry Float32Array(12 n), attributes Float32Array(28 n) | null */
static bool row_args(napi_env env, napi_value *argv, uint32_t *first, const float **g, const float **a, uint32_t *n) {
  void *pg, *pa; size_t ng, na;
  if (napi_get_value_uint32(env, argv[0], first) != napi_ok) { napi_throw_type_error(env, nullptr, "updateSceneRows: first is not a number"); return false; }
  if (!typed(env, argv[1], napi_float32_array, &pg, &ng) || !typed(env, argv[2], napi_float32_array, &pa, &na)) return false;
  if (ng % 12 != 0 || (pa && (na % 28 != 0 || na / 28 != ng / 12))) { napi_throw_range_error(env, nullptr, "geometry needs 12 and attributes 28 floats per row"); return false; }
  *g = (const float *)pg; *a = (const float *)pa; *n = (uint32_t)(ng / 12);
  return true;
}
/* updateSceneRows(handle, first, geometry, attributes | null): flx_scene_update */
static napi_value UpdateSceneRows(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  uint32_t first, n; const float *g, *a;
  if (!row_args(env, argv + 1, &first, &g, &a, &n)) return nullptr;
  flx_status rc = flx_scene_update(ctx, first, n, g, a);
  if (rc != FLX_OK) return fail(env, ctx, "flx_scene_update", rc);
  return nullptr;
}

/* castRays(handle, rays Float32Array(8 n), what) -> ArrayBuffer(32 n): flx_rays_cast, the hit rows as the library writes them (include/flexlight_hip_debug.h) */
static napi_value CastRays(napi_env env, napi_callback_info info) {
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  void *rays; size_t len; uint32_t what;
  if (!typed(env, argv[1], napi_float32_array, &rays, &len)) return nullptr;
  if (napi_get_value_uint32(env, argv[2], &what) != napi_ok) { napi_throw_type_error(env, nullptr, "castRays: what is not a number"); return nullptr; }
  if (len % 8 != 0 || len / 8 > 0xffffffffu) { napi_throw_range_error(env, nullptr, "castRays: a ray needs 8 floats (origin, l, direction, one unused)"); return nullptr; }
  void *hits = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, (len / 8) * 32, &hits, &buf));
  flx_status rc = flx_rays_cast(ctx, (const float *)rays, hits, (uint32_t)(len / 8), what);
  if (rc != FLX_OK) return fail(env, ctx, "flx_rays_cast", rc);
  return buf;
}

/* uploadTransforms(handle, rotation Float32Array(24 T), shift Float32Array(8 T)) */
static napi_value UploadTransforms(napi_env env, napi_callback_info info) {
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  void *r, *s; size_t nr, ns;
  if (!typed(env, argv[1], napi_float32_array, &r, &nr) || !typed(env, argv[2], napi_float32_array, &s, &ns)) return nullptr;
  if (ns % 8 != 0 || nr != ns * 3) { napi_throw_range_error(env, nullptr, "rotation needs 24 and shift 8 floats per transform"); return nullptr; }
  flx_status rc = flx_transforms_upload(ctx, (const float *)r, (const float *)s, (uint32_t)(ns / 8));
  if (rc != FLX_OK) return fail(env, ctx, "flx_transforms_upload", rc);
  return nullptr;
}

/* uploadLights(handle, lights Float32Array(6 L)) */
static napi_value UploadLights(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  void *l; size_t nl;
  if (!typed(env, argv[1], napi_float32_array, &l, &nl)) return nullptr;
  if (nl % 6 != 0) { napi_throw_range_error(env, nullptr, "lights needs 6 floats per light"); return nullptr; }
  flx_status rc = flx_lights_upload(ctx, (const float *)l, (uint32_t)(nl / 6));
  if (rc != FLX_OK) return fail(env, ctx, "flx_lights_upload", rc);
  return nullptr;
}

/* uploadAtlas(handle, which, rgba Uint8Array | null, width, height) */
static napi_value UploadAtlas(napi_env env, napi_callback_info info) {
  napi_value argv[5];
  if (!get_args(env, info, 5, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  int32_t which; uint32_t w, h;
  NAPI_OK(env, napi_get_value_int32(env, argv[1], &which));
  void *px; size_t n;
  if (!typed(env, argv[2], napi_uint8_array, &px, &n)) return nullptr;
  NAPI_OK(env, napi_get_value_uint32(env, argv[3], &w));
  NAPI_OK(env, napi_get_value_uint32(env, argv[4], &h));
  if (px && n != (size_t)w * h * 4) { napi_throw_range_error(env, nullptr, "atlas needs width*height*4 bytes"); return nullptr; }
  flx_status rc = flx_atlas_upload(ctx, which, (const uint8_t *)px, w, h);
  if (rc != FLX_OK) return fail(env, ctx, "flx_atlas_upload", rc);
  return nullptr;
}

/* an image of uploadTextures / updateTexture: { width, height, data: Uint8Array | Uint8ClampedArray (RGBA8) | Float32Array (RGBA32F) }, width * height * 4 elements */
static bool read_image(napi_env env, napi_value v, flx_image *out) {
  napi_valuetype t;
  napi_typeof(env, v, &t);
  if (t != napi_object) { napi_throw_type_error(env, nullptr, "a texture is { width, height, data }"); return false; }
  napi_value vw, vh, vd;
  uint32_t w = 0, h = 0;
  if (napi_get_named_property(env, v, "width", &vw) != napi_ok || napi_get_value_uint32(env, vw, &w) != napi_ok ||
      napi_get_named_property(env, v, "height", &vh) != napi_ok || napi_get_value_uint32(env, vh, &h) != napi_ok ||
      napi_get_named_property(env, v, "data", &vd) != napi_ok) { napi_throw_type_error(env, nullptr, "a texture is { width, height, data }"); return false; }
  bool is = false;
  napi_is_typedarray(env, vd, &is);
  napi_typedarray_type type; size_t len = 0; void *data = nullptr;
  if (!is || napi_get_typedarray_info(env, vd, &type, &len, &data, nullptr, nullptr) != napi_ok ||
      (type != napi_uint8_array && type != napi_uint8_clamped_array && type != napi_float32_array)) {
    napi_throw_type_error(env, nullptr, "a texture's data is a Uint8Array, a Uint8ClampedArray or a Float32Array"); return false;
  }
  if (len != (size_t)w * h * 4) { napi_throw_range_error(env, nullptr, "a texture's data needs width*height*4 elements"); return false; }
  out->pixels = data; out->width = w; out->height = h; out->format = type == napi_float32_array ? FLX_IMAGE_RGBA32F : FLX_IMAGE_RGBA8;
  return true;
}
/* the arguments of uploadTextures / groupUploadTextures after the handle: which, [image, ...], cellWidth, cellHeight */
static bool textures_args(napi_env env, napi_value *argv, int32_t *which, std::vector<flx_image> &images, uint32_t *cw, uint32_t *ch) {
  uint32_t n = 0;
  bool isArray = false;
  napi_is_array(env, argv[1], &isArray);
  if (napi_get_value_int32(env, argv[0], which) != napi_ok || !isArray || napi_get_array_length(env, argv[1], &n) != napi_ok ||
      napi_get_value_uint32(env, argv[2], cw) != napi_ok || napi_get_value_uint32(env, argv[3], ch) != napi_ok) {
    napi_throw_type_error(env, nullptr, "uploadTextures: which, an array of textures, cellWidth, cellHeight"); return false;
  }
  images.resize(n);
  for (uint32_t i = 0; i < n; i++) {
    napi_value e;
    if (napi_get_element(env, argv[1], i, &e) != napi_ok || !read_image(env, e, &images[i])) return false;
  }
  return true;
}
/* ... of updateTexture / groupUpdateTexture: which, index, image */
static bool texture_args(napi_env env, napi_value *argv, int32_t *which, uint32_t *index, flx_image *image) {
  if (napi_get_value_int32(env, argv[0], which) != napi_ok || napi_get_value_uint32(env, argv[1], index) != napi_ok) {
    napi_throw_type_error(env, nullptr, "updateTexture: which, index, texture"); return false;
  }
  return read_image(env, argv[2], image);
}
/* uploadTextures(handle, which, [{ width, height, data }, ...], cellWidth, cellHeight): flx_textures_upload — the atlas is built on the device */
static napi_value UploadTextures(napi_env env, napi_callback_info info) {
  napi_value argv[5];
  if (!get_args(env, info, 5, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  int32_t which; uint32_t cw, ch; std::vector<flx_image> images;
  if (!textures_args(env, argv + 1, &which, images, &cw, &ch)) return nullptr;
  flx_status rc = flx_textures_upload(ctx, which, images.data(), (uint32_t)images.size(), cw, ch);
  if (rc != FLX_OK) return fail(env, ctx, "flx_textures_upload", rc);
  return nullptr;
}
/* updateTexture(handle, which, index, { width, height, data }): flx_texture_update — one cell of the resident atlas replaced */
static napi_value UpdateTexture(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  int32_t which; uint32_t index; flx_image image;
  if (!texture_args(env, argv + 1, &which, &index, &image)) return nullptr;
  flx_status rc = flx_texture_update(ctx, which, index, &image);
  if (rc != FLX_OK) return fail(env, ctx, "flx_texture_update", rc);
  return nullptr;
}

static bool read_params(napi_env env, napi_value o, flx_frame_params *p) {
  memset(p, 0, sizeof *p);
  double d = 0;
  if (!num(env, o, "width", &d)) return false; p->width = (uint32_t)d;
  if (!num(env, o, "height", &d)) return false; p->height = (uint32_t)d;
  if (!floats(env, o, "camera", p->camera, 3) || !floats(env, o, "viewMatrix", p->view_matrix, 9) || !floats(env, o, "ambient", p->ambient, 3)) return false;
  if (!num(env, o, "samples", &d)) return false; p->samples = (int32_t)d;
  if (!num(env, o, "maxReflections", &d)) return false; p->max_reflections = (int32_t)d;
  if (!num(env, o, "minImportancy", &d)) return false; p->min_importancy = (float)d;
  d = 0; if (!num(env, o, "useFilter", &d, false)) return false; p->use_filter = (int32_t)d;
  d = 0; if (!num(env, o, "isTemporal", &d, false)) return false; p->is_temporal = (int32_t)d;
  d = 1; if (!num(env, o, "hdr", &d, false)) return false; p->hdr = (int32_t)d;
  d = 0; if (!num(env, o, "randomSeed", &d, false)) return false; p->random_seed = (float)d;
  if (!num(env, o, "textureWidth", &d)) return false; p->texture_width = (int32_t)d;
  d = 0; if (!num(env, o, "tileRows", &d, false)) return false; p->tile_rows = (uint32_t)d;
  d = 0; if (!num(env, o, "tileIndex", &d, false)) return false; p->tile_index = (uint32_t)d;
  d = 0; if (!num(env, o, "tileCount", &d, false)) return false; p->tile_count = (uint32_t)d;
  d = 4; if (!num(env, o, "temporalSamples", &d, false)) return false; p->temporal_samples = (int32_t)d;
  return true;
}

/* a traced call's params { samples, maxReflections, minImportancy, ambient, randomSeed?, textureWidth } -> flx_trace_params; `call`: the JavaScript name, for the
 * messages.  A JavaScript number -> int32_t is refused where the cast would not be defined (NaN, beyond the type's range); the library judges the values that fit */
static bool read_trace_params(napi_env env, napi_value o, const char *call, flx_trace_params *p) {
  memset(p, 0, sizeof *p);
  double d = 0;
  auto int32 = [&](const char *key, int32_t *out) {
    if (!num(env, o, key, &d)) return false;
    if (!(d >= -2147483648.0 && d <= 2147483647.0)) { napi_throw_range_error(env, nullptr, (std::string(call) + ": " + key + " is not a number an int32 holds").c_str()); return false; }
    *out = (int32_t)d;
    return true;
  };
  if (!int32("samples", &p->samples) || !int32("maxReflections", &p->max_reflections)) return false;
  if (!num(env, o, "minImportancy", &d)) return false; p->min_importancy = (float)d;
  if (!floats(env, o, "ambient", p->ambient, 3)) return false;
  d = 0; if (!num(env, o, "randomSeed", &d, false)) return false; p->random_seed = (float)d;
  return int32("textureWidth", &p->texture_width);
}

/* traceRays(handle, rays Float32Array(8 n), params { samples, maxReflections, minImportancy, ambient, randomSeed?, textureWidth }) -> ArrayBuffer(32 n):
 * flx_rays_trace, the radiance rows as the library writes them (include/flexlight_hip_debug.h) */
static napi_value TraceRays(napi_env env, napi_callback_info info) {
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  void *rays; size_t len;
  if (!typed(env, argv[1], napi_float32_array, &rays, &len)) return nullptr;
  if (len % 8 != 0 || len / 8 > 0xffffffffu) { napi_throw_range_error(env, nullptr, "traceRays: a ray needs 8 floats (origin, noise x, direction, noise y)"); return nullptr; }
  flx_trace_params p;
  if (!read_trace_params(env, argv[2], "traceRays", &p)) return nullptr;
  void *rows = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, (len / 8) * 32, &rows, &buf));
  flx_status rc = flx_rays_trace(ctx, &p, (const float *)rays, rows, (uint32_t)(len / 8));
  if (rc != FLX_OK) return fail(env, ctx, "flx_rays_trace", rc);
  return buf;
}

/* traceRaysOrdered(handle, rays Float32Array(8 n), params (traceRays'), order) -> ArrayBuffer(32 n): flx_rays_trace_ordered — traceRays' rows, each slab's rays
 * traced in the order `order` asks for (1: FLX_TRACE_ORDER_HITS; the library refuses a bit it does not know) */
static napi_value TraceRaysOrdered(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  void *rays; size_t len;
  if (!typed(env, argv[1], napi_float32_array, &rays, &len)) return nullptr;
  if (len % 8 != 0 || len / 8 > 0xffffffffu) { napi_throw_range_error(env, nullptr, "traceRaysOrdered: a ray needs 8 floats (origin, noise x, direction, noise y)"); return nullptr; }
  flx_trace_params p;
  if (!read_trace_params(env, argv[2], "traceRaysOrdered", &p)) return nullptr;
  uint32_t order = 0;
  if (napi_get_value_uint32(env, argv[3], &order) != napi_ok) { napi_throw_type_error(env, nullptr, "traceRaysOrdered: order is not a number"); return nullptr; }
  void *rows = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, (len / 8) * 32, &rows, &buf));
  flx_status rc = flx_rays_trace_ordered(ctx, &p, (const float *)rays, rows, (uint32_t)(len / 8), order);
  if (rc != FLX_OK) return fail(env, ctx, "flx_rays_trace_ordered", rc);
  return buf;
}

/* traceProbes(handle, positions Float32Array(4 n), params (traceRays'), { faceSize, order, sky[3] }) -> ArrayBuffer(144 n): flx_probes_sh, one SH row of 36 floats
 * per probe position (include/flexlight_hip_debug.h "light probes"); the library judges the values */
static napi_value TraceProbes(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  void *positions; size_t len;
  if (!typed(env, argv[1], napi_float32_array, &positions, &len)) return nullptr;
  if (len % 4 != 0 || len / 4 > 0xffffffffu) { napi_throw_range_error(env, nullptr, "traceProbes: a position needs 4 floats (x, y, z and a word that is ignored)"); return nullptr; }
  flx_trace_params p;
  if (!read_trace_params(env, argv[2], "traceProbes", &p)) return nullptr;
  flx_probe_params q;
  memset(&q, 0, sizeof q);
  napi_value v;
  if (napi_get_named_property(env, argv[3], "faceSize", &v) != napi_ok || napi_get_value_uint32(env, v, &q.face_size) != napi_ok ||
      napi_get_named_property(env, argv[3], "order", &v) != napi_ok || napi_get_value_uint32(env, v, &q.order) != napi_ok) {
    napi_throw_type_error(env, nullptr, "traceProbes: faceSize and order are numbers");
    return nullptr;
  }
  if (!floats(env, argv[3], "sky", q.sky, 3)) return nullptr;
  void *rows = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, (len / 4) * 144, &rows, &buf));
  flx_status rc = flx_probes_sh(ctx, &p, &q, (const float *)positions, (uint32_t)(len / 4), (float *)rows);
  if (rc != FLX_OK) return fail(env, ctx, "flx_probes_sh", rc);
  return buf;
}

/* probeIrradiance(row Float32Array(36), normal Float32Array(3)) -> Float32Array(3): flx_probe_irradiance, the library's one definition; no context */
static napi_value ProbeIrradiance(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return nullptr;
  void *row, *normal; size_t row_len, normal_len;
  if (!typed(env, argv[0], napi_float32_array, &row, &row_len) || !typed(env, argv[1], napi_float32_array, &normal, &normal_len)) return nullptr;
  if (row_len != 36 || normal_len != 3) { napi_throw_range_error(env, nullptr, "probeIrradiance: an SH row of 36 floats and a normal of 3"); return nullptr; }
  void *out = nullptr;
  napi_value buf, array;
  NAPI_OK(env, napi_create_arraybuffer(env, 12, &out, &buf));
  flx_probe_irradiance((const float *)row, (const float *)normal, (float *)out);
  NAPI_OK(env, napi_create_typedarray(env, napi_float32_array, 3, buf, 0, &array));
  return array;
}

/* PROBE VOLUMES (include/flexlight_hip_debug.h "probe volumes").  A volume handle owns the grid's SH rows IN DEVICE MEMORY — baked there by flx_volume_bake_device and
 * read there by the lookups, so that a frame's irradiance costs no upload — and a second device buffer the lookups of host rays stage through, grown and never
 * shrunk.  It keeps its context's handle alive and frees its memory when JavaScript lets go of it. */
struct VolumeBox {
  flx_volume_grid grid;
  uint32_t probes = 0;
  int device = 0;
  void *d_sh = nullptr, *d_io = nullptr;
  size_t io_bytes = 0;
  napi_ref context = nullptr;
  /* directional visibility ("directional visibility"): baked with { map: { size, sharpness } }, the handle also owns the probes' octahedral maps in device memory
   * and the lookups read them (the _map calls); without, d_maps stays NULL and every call is the plain one */
  flx_volume_map map = { 0u, 0u, { 0u, 0u } };
  void *d_maps = nullptr;
  /* volume updates ("volume updates"): updateVolume re-bakes listed probes with the face size, order and sky the volume was baked with */
  flx_probe_params probe = { 0u, 0u, { 0.0f, 0.0f, 0.0f }, 0.0f };
  /* probe relocation ("probe relocation"): one offset row per probe in device memory, zero-filled at the first relocateVolume; a handle that has them goes through
   * the relocated calls, one without goes where it went */
  void *d_offsets = nullptr;
};
static void finalize_volume(napi_env env, void *data, void *) {
  VolumeBox *v = static_cast<VolumeBox *>(data);
  if (hipSetDevice(v->device) == hipSuccess) { (void)hipFree(v->d_sh); (void)hipFree(v->d_io); (void)hipFree(v->d_maps); (void)hipFree(v->d_offsets); }
  if (v->context) napi_delete_reference(env, v->context);
  delete v;
}
static bool hip_ok(napi_env env, hipError_t e, const char *what) {
  if (e == hipSuccess) return true;
  napi_throw_error(env, nullptr, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
  return false;
}
/* the volume's staging holds `bytes` */
static bool volume_room(napi_env env, VolumeBox *v, size_t bytes) {
  if (v->io_bytes >= bytes) return true;
  if (!hip_ok(env, hipSetDevice(v->device), "hipSetDevice") || !hip_ok(env, hipFree(v->d_io), "hipFree")) return false;
  v->d_io = nullptr; v->io_bytes = 0;
  if (!hip_ok(env, hipMalloc(&v->d_io, bytes), "hipMalloc")) return false;
  v->io_bytes = bytes;
  return true;
}
static VolumeBox *get_volume(napi_env env, napi_value v, const CtxBox *box) {
  void *p = nullptr;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p) { napi_throw_type_error(env, nullptr, "expected a volume handle"); return nullptr; }
  VolumeBox *volume = static_cast<VolumeBox *>(p);
  if (volume->device != box->device) { napi_throw_error(env, nullptr, "the volume was baked on another GPU"); return nullptr; }
  return volume;
}
/* { origin[3], spacing[3], count[3], normalBias, floor, visibility } -> flx_volume_grid; the library judges the values */
static bool read_grid(napi_env env, napi_value o, flx_volume_grid *g) {
  memset(g, 0, sizeof *g);
  float count[3];
  double d = 0;
  if (!floats(env, o, "origin", g->origin, 3) || !floats(env, o, "spacing", g->spacing, 3) || !floats(env, o, "count", count, 3)) return false;
  for (int a = 0; a < 3; a++) {
    if (!(count[a] >= 0.0f && count[a] <= 4294967040.0f) || count[a] != (float)(uint32_t)count[a]) { napi_throw_range_error(env, nullptr, "volume grid: count holds three whole numbers a uint32 holds"); return false; }
    g->count[a] = (uint32_t)count[a];
  }
  if (!num(env, o, "normalBias", &d)) return false; g->normal_bias = (float)d;
  if (!num(env, o, "floor", &d)) return false; g->floor = (float)d;
  d = 1; if (!num(env, o, "visibility", &d, false)) return false; g->flags = d != 0.0 ? FLX_VOLUME_VISIBILITY : 0u;
  return true;
}

/* { backShare, minFront, reach, limit, iterations, faceSize } -> the relocation, its passes and its face size; the library judges the values */
struct RelocateOptions { struct flx_volume_relocate r; uint32_t iterations, face_size; };
static bool read_relocate(napi_env env, napi_value o, RelocateOptions *out) {
  double d = 0;
  memset(out, 0, sizeof *out);
  if (!num(env, o, "backShare", &d)) return false; out->r.back_share = (float)d;
  if (!num(env, o, "minFront", &d)) return false; out->r.min_front = (float)d;
  if (!num(env, o, "reach", &d)) return false; out->r.reach = (float)d;
  if (!num(env, o, "limit", &d)) return false; out->r.limit = (float)d;
  napi_value v;
  if (napi_get_named_property(env, o, "iterations", &v) != napi_ok || napi_get_value_uint32(env, v, &out->iterations) != napi_ok ||
      napi_get_named_property(env, o, "faceSize", &v) != napi_ok || napi_get_value_uint32(env, v, &out->face_size) != napi_ok) {
    napi_throw_type_error(env, nullptr, "relocateVolume: iterations and faceSize are numbers");
    return false;
  }
  return true;
}
/* the volume has offset rows: zero-filled where it had none */
static bool volume_offsets(napi_env env, VolumeBox *v) {
  if (v->d_offsets) return true;
  if (!hip_ok(env, hipSetDevice(v->device), "hipSetDevice") || !hip_ok(env, hipMalloc(&v->d_offsets, (size_t)v->probes * 16), "hipMalloc")) return false;
  return hip_ok(env, hipMemset(v->d_offsets, 0, (size_t)v->probes * 16), "hipMemset");
}
/* `iterations` passes of flx_volume_relocate_device on the volume's offsets and one frozen pass, which moves nothing and classifies every probe where it stands */
static flx_status relocate_passes(flx_context *ctx, VolumeBox *v, int32_t texture_width, const RelocateOptions &o) {
  struct flx_volume_relocate r = o.r;
  for (uint32_t k = 0; k <= o.iterations; k++) {
    r.flags = k == o.iterations ? FLX_VOLUME_RELOCATE_FREEZE : 0u;
    const flx_status rc = flx_volume_relocate_device(ctx, texture_width, &v->grid, &r, o.face_size, v->d_offsets, nullptr);
    if (rc != FLX_OK) return rc;
  }
  return FLX_OK;
}

/* bakeVolume(handle, grid, params (traceRays'), { faceSize, order, sky[3], map: { size, sharpness } or undefined, relocate: relocateVolume's options or undefined })
 * -> volume handle: flx_volume_bake_device — with a map flx_volume_bake_map_device — into device memory the handle owns; with relocate the probes are relocated first
 * (from zero offsets) and the bake is flx_volume_bake_relocated_device's, from the moved positions */
static napi_value BakeVolume(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  CtxBox *box = get_box(env, argv[0]);
  if (!box) return nullptr;
  flx_volume_grid grid;
  flx_trace_params p;
  flx_probe_params q;
  if (!read_grid(env, argv[1], &grid) || !read_trace_params(env, argv[2], "bakeVolume", &p)) return nullptr;
  memset(&q, 0, sizeof q);
  napi_value v;
  if (napi_get_named_property(env, argv[3], "faceSize", &v) != napi_ok || napi_get_value_uint32(env, v, &q.face_size) != napi_ok ||
      napi_get_named_property(env, argv[3], "order", &v) != napi_ok || napi_get_value_uint32(env, v, &q.order) != napi_ok) {
    napi_throw_type_error(env, nullptr, "bakeVolume: faceSize and order are numbers");
    return nullptr;
  }
  if (!floats(env, argv[3], "sky", q.sky, 3)) return nullptr;
  flx_volume_map map = { 0u, 0u, { 0u, 0u } };
  napi_valuetype map_type = napi_undefined;
  if (napi_get_named_property(env, argv[3], "map", &v) != napi_ok || napi_typeof(env, v, &map_type) != napi_ok) { napi_throw_type_error(env, nullptr, "bakeVolume: map is { size, sharpness }"); return nullptr; }
  const bool has_map = map_type != napi_undefined;
  if (has_map) {
    napi_value field;
    if (map_type != napi_object || napi_get_named_property(env, v, "size", &field) != napi_ok || napi_get_value_uint32(env, field, &map.size) != napi_ok ||
        napi_get_named_property(env, v, "sharpness", &field) != napi_ok || napi_get_value_uint32(env, field, &map.sharpness) != napi_ok) {
      napi_throw_type_error(env, nullptr, "bakeVolume: map is { size, sharpness }, two numbers");
      return nullptr;
    }
  }
  RelocateOptions relocate;
  napi_valuetype relocate_type = napi_undefined;
  if (napi_get_named_property(env, argv[3], "relocate", &v) != napi_ok || napi_typeof(env, v, &relocate_type) != napi_ok) { napi_throw_type_error(env, nullptr, "bakeVolume: relocate is an object"); return nullptr; }
  const bool relocated = relocate_type != napi_undefined;
  if (relocated && (relocate_type != napi_object || !read_relocate(env, v, &relocate))) {
    bool pending = false;
    napi_is_exception_pending(env, &pending);
    if (!pending) napi_throw_type_error(env, nullptr, "bakeVolume: relocate is { backShare, minFront, reach, limit, iterations, faceSize }");
    return nullptr;
  }
  /* a grid the library refuses (a count of 0, 2^31 probes or more) gets no memory: the library says why */
  const uint64_t xy = (uint64_t)grid.count[0] * grid.count[1];
  const uint64_t probes = xy <= 0x7fffffffull ? xy * grid.count[2] : xy;
  if (probes == 0 || probes > 0x7fffffffull) return fail(env, box->ctx, "flx_volume_bake_device", flx_volume_bake_device(box->ctx, &p, &q, &grid, nullptr, nullptr));
  /* ... and so does a map it refuses (a size outside 1 .. 16, 2^31 rows or more) */
  const uint64_t map_rows = has_map && map.size >= 1u && map.size <= 16u ? probes * (map.size * map.size) : 0u;
  if (has_map && (map_rows == 0 || map_rows > 0x7fffffffull))
    return fail(env, box->ctx, "flx_volume_bake_map_device", flx_volume_bake_map_device(box->ctx, &p, &q, &grid, &map, nullptr, nullptr, nullptr));
  VolumeBox *volume = new VolumeBox();
  volume->grid = grid; volume->probes = (uint32_t)probes; volume->device = box->device;
  napi_value ext;
  if (napi_create_external(env, volume, finalize_volume, nullptr, &ext) != napi_ok) { delete volume; napi_throw_error(env, nullptr, "N-API call failed: napi_create_external"); return nullptr; }
  NAPI_OK(env, napi_create_reference(env, argv[0], 1, &volume->context));
  if (!hip_ok(env, hipSetDevice(box->device), "hipSetDevice") || !hip_ok(env, hipMalloc(&volume->d_sh, (size_t)probes * 144), "hipMalloc")) return nullptr;
  if (has_map && !hip_ok(env, hipMalloc(&volume->d_maps, (size_t)map_rows * 16), "hipMalloc")) return nullptr;
  volume->map = map;
  volume->probe = q;
  if (relocated) {
    if (!volume_offsets(env, volume)) return nullptr;
    flx_status rc = relocate_passes(box->ctx, volume, p.texture_width, relocate);
    if (rc != FLX_OK) return fail(env, box->ctx, "flx_volume_relocate_device", rc);
    rc = flx_volume_bake_relocated_device(box->ctx, &p, &q, &grid, has_map ? &map : nullptr, volume->d_offsets, volume->d_sh, volume->d_maps, nullptr);
    if (rc == FLX_OK) rc = flx_sync(box->ctx);
    if (rc != FLX_OK) return fail(env, box->ctx, "flx_volume_bake_relocated_device", rc);
    return ext;
  }
  flx_status rc = has_map ? flx_volume_bake_map_device(box->ctx, &p, &q, &grid, &map, volume->d_sh, volume->d_maps, nullptr)
                          : flx_volume_bake_device(box->ctx, &p, &q, &grid, volume->d_sh, nullptr);
  if (rc == FLX_OK) rc = flx_sync(box->ctx);
  if (rc != FLX_OK) return fail(env, box->ctx, has_map ? "flx_volume_bake_map_device" : "flx_volume_bake_device", rc);
  return ext;
}

/* volumeRows(handle, volume) -> ArrayBuffer(144 probes): the SH rows, fetched from the device */
static napi_value VolumeRows(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return nullptr;
  CtxBox *box = get_box(env, argv[0]);
  VolumeBox *volume = box ? get_volume(env, argv[1], box) : nullptr;
  if (!volume) return nullptr;
  void *rows = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, (size_t)volume->probes * 144, &rows, &buf));
  flx_status rc = flx_sync(box->ctx);
  if (rc != FLX_OK) return fail(env, box->ctx, "flx_sync", rc);
  if (!hip_ok(env, hipSetDevice(box->device), "hipSetDevice") || !hip_ok(env, hipMemcpy(rows, volume->d_sh, (size_t)volume->probes * 144, hipMemcpyDeviceToHost), "hipMemcpy")) return nullptr;
  return buf;
}

/* volumeMaps(handle, volume) -> ArrayBuffer(16 size size probes): the map rows of a volume baked with a map, fetched from the device */
static napi_value VolumeMaps(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return nullptr;
  CtxBox *box = get_box(env, argv[0]);
  VolumeBox *volume = box ? get_volume(env, argv[1], box) : nullptr;
  if (!volume) return nullptr;
  if (!volume->d_maps) { napi_throw_error(env, nullptr, "volumeMaps: the volume was baked without a map"); return nullptr; }
  const size_t bytes = (size_t)volume->probes * volume->map.size * volume->map.size * 16;
  void *rows = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, bytes, &rows, &buf));
  flx_status rc = flx_sync(box->ctx);
  if (rc != FLX_OK) return fail(env, box->ctx, "flx_sync", rc);
  if (!hip_ok(env, hipSetDevice(box->device), "hipSetDevice") || !hip_ok(env, hipMemcpy(rows, volume->d_maps, bytes, hipMemcpyDeviceToHost), "hipMemcpy")) return nullptr;
  return buf;
}

/* volumeOffsets(handle, volume) -> ArrayBuffer(16 probes): the offset rows of a volume that has them, fetched from the device */
static napi_value VolumeOffsets(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return nullptr;
  CtxBox *box = get_box(env, argv[0]);
  VolumeBox *volume = box ? get_volume(env, argv[1], box) : nullptr;
  if (!volume) return nullptr;
  if (!volume->d_offsets) { napi_throw_error(env, nullptr, "volumeOffsets: the volume was never relocated"); return nullptr; }
  void *rows = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, (size_t)volume->probes * 16, &rows, &buf));
  flx_status rc = flx_sync(box->ctx);
  if (rc != FLX_OK) return fail(env, box->ctx, "flx_sync", rc);
  if (!hip_ok(env, hipSetDevice(box->device), "hipSetDevice") || !hip_ok(env, hipMemcpy(rows, volume->d_offsets, (size_t)volume->probes * 16, hipMemcpyDeviceToHost), "hipMemcpy")) return nullptr;
  return buf;
}

/* relocateVolume(handle, volume, textureWidth, { backShare, minFront, reach, limit, iterations, faceSize }) -> ArrayBuffer(16 probes): the volume's offset rows —
 * zero-filled at the first call — after `iterations` passes of flx_volume_relocate_device and one frozen pass.  The volume's SH rows and maps are left as they are:
 * the caller bakes or updates again.  The library judges the values. */
static napi_value RelocateVolume(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  CtxBox *box = get_box(env, argv[0]);
  VolumeBox *volume = box ? get_volume(env, argv[1], box) : nullptr;
  if (!volume) return nullptr;
  int32_t tw;
  if (napi_get_value_int32(env, argv[2], &tw) != napi_ok) { napi_throw_type_error(env, nullptr, "relocateVolume: textureWidth is not a number"); return nullptr; }
  RelocateOptions o;
  if (!read_relocate(env, argv[3], &o)) return nullptr;
  const bool fresh = volume->d_offsets == nullptr;
  if (!volume_offsets(env, volume)) return nullptr;
  flx_status rc = relocate_passes(box->ctx, volume, tw, o);
  if (rc == FLX_OK) rc = flx_sync(box->ctx);
  if (rc != FLX_OK) {
    if (fresh) { (void)hipFree(volume->d_offsets); volume->d_offsets = nullptr; }      /* a refused first call leaves the handle without offsets: it goes where it went */
    return fail(env, box->ctx, "flx_volume_relocate_device", rc);
  }
  void *rows = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, (size_t)volume->probes * 16, &rows, &buf));
  if (!hip_ok(env, hipMemcpy(rows, volume->d_offsets, (size_t)volume->probes * 16, hipMemcpyDeviceToHost), "hipMemcpy")) return nullptr;
  return buf;
}

/* updateVolume(handle, volume, params (traceRays'), { hysteresis, indices: Uint32Array or undefined, first, stride, count }) -> ArrayBuffer(4 n): flx_volume_update_device
 * on the volume's resident rows (and maps, where it has them), in place; the list goes up into the volume's staging and the states come down from behind it.  The
 * library judges the values. */
static napi_value UpdateVolume(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  CtxBox *box = get_box(env, argv[0]);
  if (!box) return nullptr;
  VolumeBox *volume = get_volume(env, argv[1], box);
  if (!volume) return nullptr;
  flx_trace_params p;
  if (!read_trace_params(env, argv[2], "updateVolume", &p)) return nullptr;
  struct flx_volume_update u = { 0.0f, 0u, 0u, 0u };
  double h = 0;
  if (!num(env, argv[3], "hysteresis", &h)) return nullptr;
  u.hysteresis = (float)h;
  napi_value v;
  napi_valuetype list_type = napi_undefined;
  if (napi_get_named_property(env, argv[3], "indices", &v) != napi_ok || napi_typeof(env, v, &list_type) != napi_ok) { napi_throw_type_error(env, nullptr, "updateVolume: indices is a Uint32Array"); return nullptr; }
  void *indices = nullptr;
  size_t n = 0;
  if (list_type != napi_undefined) {
    if (!typed(env, v, napi_uint32_array, &indices, &n)) return nullptr;
  } else {
    napi_value field;
    uint32_t count = 0;
    if (napi_get_named_property(env, argv[3], "first", &field) != napi_ok || napi_get_value_uint32(env, field, &u.first) != napi_ok ||
        napi_get_named_property(env, argv[3], "stride", &field) != napi_ok || napi_get_value_uint32(env, field, &u.stride) != napi_ok ||
        napi_get_named_property(env, argv[3], "count", &field) != napi_ok || napi_get_value_uint32(env, field, &count) != napi_ok) {
      napi_throw_type_error(env, nullptr, "updateVolume: probes is a Uint32Array or { first, stride, count }, three numbers");
      return nullptr;
    }
    n = count;
  }
  if (n > 0xffffffffu) { napi_throw_range_error(env, nullptr, "updateVolume: more indices than a uint32 counts"); return nullptr; }
  /* a list the library refuses for its length gets no memory: the library says why */
  const bool fits = n <= volume->probes;
  void *states = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, fits ? n * 4 : 0, &states, &buf));
  char *d_list = nullptr, *d_state = nullptr;
  if (fits && n > 0) {
    if (!volume_room(env, volume, n * 8)) return nullptr;
    d_list = static_cast<char *>(volume->d_io); d_state = d_list + n * 4;
    if (indices && !hip_ok(env, hipMemcpy(d_list, indices, n * 4, hipMemcpyHostToDevice), "hipMemcpy")) return nullptr;
  }
  /* (a handle with offsets: the listed probes are traced from their offset positions) */
  flx_status rc = volume->d_offsets
                      ? flx_volume_update_relocated_device(box->ctx, &p, &volume->probe, &volume->grid, volume->d_maps ? &volume->map : nullptr, &u, indices && fits ? d_list : nullptr,
                                                           (uint32_t)n, volume->d_offsets, volume->d_sh, volume->d_maps, d_state, nullptr)
                      : flx_volume_update_device(box->ctx, &p, &volume->probe, &volume->grid, volume->d_maps ? &volume->map : nullptr, &u, indices && fits ? d_list : nullptr, (uint32_t)n,
                                                 volume->d_sh, volume->d_maps, d_state, nullptr);
  if (rc == FLX_OK) rc = flx_sync(box->ctx);
  if (rc != FLX_OK) return fail(env, box->ctx, volume->d_offsets ? "flx_volume_update_relocated_device" : "flx_volume_update_device", rc);
  if (n > 0 && !hip_ok(env, hipMemcpy(states, d_state, n * 4, hipMemcpyDeviceToHost), "hipMemcpy")) return nullptr;
  return buf;
}

/* frameIrradiance(handle, params, volume) -> ArrayBuffer(16 width height): flx_frame_irradiance_device on the volume's rows, the image fetched */
static napi_value FrameIrradiance(napi_env env, napi_callback_info info) {
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return nullptr;
  CtxBox *box = get_box(env, argv[0]);
  if (!box) return nullptr;
  flx_frame_params p;
  if (!read_params(env, argv[1], &p)) return nullptr;
  VolumeBox *volume = get_volume(env, argv[2], box);
  if (!volume) return nullptr;
  if ((uint64_t)p.width * p.height > 0xffffffffull) { napi_throw_range_error(env, nullptr, "frameIrradiance: the frame has more than 2^32 - 1 pixels"); return nullptr; }
  const size_t bytes = (size_t)p.width * p.height * 16;
  void *image = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, bytes, &image, &buf));
  if (!volume_room(env, volume, bytes ? bytes : 16)) return nullptr;
  flx_status rc = volume->d_offsets ? flx_frame_irradiance_relocated_device(box->ctx, &p, &volume->grid, volume->d_sh, volume->d_io, volume->d_maps ? &volume->map : nullptr, volume->d_maps,
                                                                            volume->d_offsets)
                  : volume->d_maps  ? flx_frame_irradiance_map_device(box->ctx, &p, &volume->grid, volume->d_sh, volume->d_io, &volume->map, volume->d_maps)
                                    : flx_frame_irradiance_device(box->ctx, &p, &volume->grid, volume->d_sh, volume->d_io);
  if (rc == FLX_OK) rc = flx_sync(box->ctx);
  if (rc != FLX_OK)
    return fail(env, box->ctx, volume->d_offsets ? "flx_frame_irradiance_relocated_device" : volume->d_maps ? "flx_frame_irradiance_map_device" : "flx_frame_irradiance_device", rc);
  if (!hip_ok(env, hipMemcpy(image, volume->d_io, bytes, hipMemcpyDeviceToHost), "hipMemcpy")) return nullptr;
  return buf;
}

/* raysIrradiance(handle, rays Float32Array(8 n), textureWidth, volume) -> ArrayBuffer(16 n): flx_rays_irradiance_device on the volume's rows; the rays go up into
 * the volume's staging, the rows come down from behind them */
static napi_value RaysIrradiance(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  CtxBox *box = get_box(env, argv[0]);
  if (!box) return nullptr;
  void *rays; size_t len; int32_t tw;
  if (!typed(env, argv[1], napi_float32_array, &rays, &len)) return nullptr;
  if (napi_get_value_int32(env, argv[2], &tw) != napi_ok) { napi_throw_type_error(env, nullptr, "raysIrradiance: textureWidth is not a number"); return nullptr; }
  if (len % 8 != 0 || len / 8 > 0xffffffffu) { napi_throw_range_error(env, nullptr, "raysIrradiance: a ray needs 8 floats (origin, one unused, direction, one unused)"); return nullptr; }
  VolumeBox *volume = get_volume(env, argv[3], box);
  if (!volume) return nullptr;
  const size_t n = len / 8;
  void *rows = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, n * 16, &rows, &buf));
  if (n == 0) return buf;
  if (!volume_room(env, volume, n * 48)) return nullptr;
  char *d_rays = static_cast<char *>(volume->d_io), *d_rows = d_rays + n * 32;
  if (!hip_ok(env, hipMemcpy(d_rays, rays, n * 32, hipMemcpyHostToDevice), "hipMemcpy")) return nullptr;
  flx_status rc = volume->d_offsets ? flx_rays_irradiance_relocated_device(box->ctx, tw, &volume->grid, volume->d_sh, d_rays, (uint32_t)n, d_rows, volume->d_maps ? &volume->map : nullptr,
                                                                           volume->d_maps, volume->d_offsets, nullptr)
                  : volume->d_maps  ? flx_rays_irradiance_map_device(box->ctx, tw, &volume->grid, volume->d_sh, d_rays, (uint32_t)n, d_rows, &volume->map, volume->d_maps, nullptr)
                                    : flx_rays_irradiance_device(box->ctx, tw, &volume->grid, volume->d_sh, d_rays, (uint32_t)n, d_rows, nullptr);
  if (rc == FLX_OK) rc = flx_sync(box->ctx);
  if (rc != FLX_OK)
    return fail(env, box->ctx, volume->d_offsets ? "flx_rays_irradiance_relocated_device" : volume->d_maps ? "flx_rays_irradiance_map_device" : "flx_rays_irradiance_device", rc);
  if (!hip_ok(env, hipMemcpy(rows, d_rows, n * 16, hipMemcpyDeviceToHost), "hipMemcpy")) return nullptr;
  return buf;
}

/* traceRaysGather(handle, rays Float32Array(8 n), params (traceRays'), order, volume, gain) -> ArrayBuffer(32 n): flx_rays_trace_gather_device on the volume's rows —
 * its SH rows, its maps and its offsets where it has them, all resident —: traceRays' rows whose paths end in the volume's irradiance at their last point times gain
 * (include/flexlight_hip_debug.h "ray batches with a volume").  The rays go up into the volume's staging, the rows come down from behind them. */
static napi_value TraceRaysGather(napi_env env, napi_callback_info info) {
  napi_value argv[6];
  if (!get_args(env, info, 6, argv)) return nullptr;
  CtxBox *box = get_box(env, argv[0]);
  if (!box) return nullptr;
  void *rays; size_t len;
  if (!typed(env, argv[1], napi_float32_array, &rays, &len)) return nullptr;
  if (len % 8 != 0 || len / 8 > 0xffffffffu) { napi_throw_range_error(env, nullptr, "traceRays: a ray needs 8 floats (origin, noise x, direction, noise y)"); return nullptr; }
  flx_trace_params p;
  if (!read_trace_params(env, argv[2], "traceRays", &p)) return nullptr;
  uint32_t order = 0;
  if (napi_get_value_uint32(env, argv[3], &order) != napi_ok) { napi_throw_type_error(env, nullptr, "traceRays: order is not a number"); return nullptr; }
  VolumeBox *volume = get_volume(env, argv[4], box);
  if (!volume) return nullptr;
  double gain = 0;
  if (napi_get_value_double(env, argv[5], &gain) != napi_ok) { napi_throw_type_error(env, nullptr, "traceRays: gain is not a number"); return nullptr; }
  const size_t n = len / 8;
  void *rows = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, n * 32, &rows, &buf));
  if (!volume_room(env, volume, n ? n * 64 : 64)) return nullptr;
  char *d_rays = static_cast<char *>(volume->d_io), *d_rows = d_rays + n * 32;
  if (n > 0 && !hip_ok(env, hipMemcpy(d_rays, rays, n * 32, hipMemcpyHostToDevice), "hipMemcpy")) return nullptr;
  flx_gather_volume v;
  memset(&v, 0, sizeof v);
  v.grid = &volume->grid; v.sh = volume->d_sh;
  v.map = volume->d_maps ? &volume->map : nullptr; v.maps = volume->d_maps;
  v.offsets = volume->d_offsets;
  v.gain = (float)gain;
  flx_status rc = flx_rays_trace_gather_device(box->ctx, &p, &v, d_rays, d_rows, (uint32_t)n, order, nullptr);
  if (rc == FLX_OK) rc = flx_sync(box->ctx);
  if (rc != FLX_OK) return fail(env, box->ctx, "flx_rays_trace_gather_device", rc);
  if (n > 0 && !hip_ok(env, hipMemcpy(rows, d_rows, n * 32, hipMemcpyDeviceToHost), "hipMemcpy")) return nullptr;
  return buf;
}

/* rayImage(handle, rays Float32Array(8 width height), width, height, params (traceRays'), hdr) -> ArrayBuffer(16 width height): flx_rays_image, the rays in image
 * order (row 0 on top) traced into the five filter planes and denoised by the chain; float4 per pixel (include/flexlight_hip_debug.h) */
static napi_value RayImage(napi_env env, napi_callback_info info) {
  napi_value argv[6];
  if (!get_args(env, info, 6, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  void *rays; size_t len; uint32_t width, height;
  if (!typed(env, argv[1], napi_float32_array, &rays, &len)) return nullptr;
  if (napi_get_value_uint32(env, argv[2], &width) != napi_ok || napi_get_value_uint32(env, argv[3], &height) != napi_ok) {
    napi_throw_type_error(env, nullptr, "rayImage: width and height are numbers");
    return nullptr;
  }
  if (len % 8 != 0 || (uint64_t)(len / 8) != (uint64_t)width * height) { napi_throw_range_error(env, nullptr, "rayImage: width * height rays of 8 floats (origin, noise x, direction, noise y)"); return nullptr; }
  flx_trace_params p;
  if (!read_trace_params(env, argv[4], "rayImage", &p)) return nullptr;
  bool hdr = true;
  if (napi_get_value_bool(env, argv[5], &hdr) != napi_ok) { napi_throw_type_error(env, nullptr, "rayImage: hdr is a boolean"); return nullptr; }
  void *image = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, (len / 8) * 16, &image, &buf));
  flx_status rc = flx_rays_image(ctx, &p, hdr ? 1 : 0, (const float *)rays, width, height, (float *)image);
  if (rc != FLX_OK) return fail(env, ctx, "flx_rays_image", rc);
  return buf;
}

/* a temporal image's { history, temporalSamples, filter, hdr } -> flx_ray_temporal; `call`: the JavaScript name, for the messages */
static bool read_ray_temporal(napi_env env, napi_value o, const char *call, flx_ray_temporal *t) {
  memset(t, 0, sizeof *t);
  double d = 0;
  auto int32 = [&](const char *key, int32_t *out) {
    if (!num(env, o, key, &d)) return false;
    if (!(d >= -2147483648.0 && d <= 2147483647.0)) { napi_throw_range_error(env, nullptr, (std::string(call) + ": " + key + " is not a number an int32 holds").c_str()); return false; }
    *out = (int32_t)d;
    return true;
  };
  if (!int32("history", &t->history) || !int32("temporalSamples", &t->temporal_samples)) return false;
  napi_value v;
  bool filter = true, hdr = true;
  if (napi_get_named_property(env, o, "filter", &v) != napi_ok || napi_get_value_bool(env, v, &filter) != napi_ok ||
      napi_get_named_property(env, o, "hdr", &v) != napi_ok || napi_get_value_bool(env, v, &hdr) != napi_ok) {
    napi_throw_type_error(env, nullptr, (std::string(call) + ": filter and hdr are booleans").c_str());
    return false;
  }
  t->use_filter = filter ? 1 : 0; t->hdr = hdr ? 1 : 0;
  return true;
}

/* rayImageTemporal(handle, rays Float32Array(8 width height), width, height, params (traceRays'), { history, temporalSamples, filter, hdr }) ->
 * ArrayBuffer(16 width height): flx_rays_image_temporal, the ray image accumulated over that history of the context's, denoised where filter is true */
static napi_value RayImageTemporal(napi_env env, napi_callback_info info) {
  napi_value argv[6];
  if (!get_args(env, info, 6, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  void *rays; size_t len; uint32_t width, height;
  if (!typed(env, argv[1], napi_float32_array, &rays, &len)) return nullptr;
  if (napi_get_value_uint32(env, argv[2], &width) != napi_ok || napi_get_value_uint32(env, argv[3], &height) != napi_ok) {
    napi_throw_type_error(env, nullptr, "rayImageTemporal: width and height are numbers");
    return nullptr;
  }
  if (len % 8 != 0 || (uint64_t)(len / 8) != (uint64_t)width * height) { napi_throw_range_error(env, nullptr, "rayImageTemporal: width * height rays of 8 floats (origin, noise x, direction, noise y)"); return nullptr; }
  flx_trace_params p;
  if (!read_trace_params(env, argv[4], "rayImageTemporal", &p)) return nullptr;
  flx_ray_temporal t;
  if (!read_ray_temporal(env, argv[5], "rayImageTemporal", &t)) return nullptr;
  void *image = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, (len / 8) * 16, &image, &buf));
  flx_status rc = flx_rays_image_temporal(ctx, &p, &t, (const float *)rays, width, height, (float *)image);
  if (rc != FLX_OK) return fail(env, ctx, "flx_rays_image_temporal", rc);
  return buf;
}

/* a camera { projection, face, position[3], basis[9], extent[2], jitter[2] } (pathtracerHIP.js: cameraOf makes it) -> flx_camera; the library judges the values */
static bool read_camera(napi_env env, napi_value o, const char *call, flx_camera *c) {
  memset(c, 0, sizeof *c);
  napi_valuetype t;
  if (napi_typeof(env, o, &t) != napi_ok || t != napi_object) { napi_throw_type_error(env, nullptr, (std::string(call) + ": camera is an object").c_str()); return false; }
  double d = 0;
  auto int32 = [&](const char *key, int32_t *out) {
    if (!num(env, o, key, &d)) return false;
    if (!(d >= -2147483648.0 && d <= 2147483647.0)) { napi_throw_range_error(env, nullptr, (std::string(call) + ": " + key + " is not a number an int32 holds").c_str()); return false; }
    *out = (int32_t)d;
    return true;
  };
  return int32("projection", &c->projection) && int32("face", &c->face) && floats(env, o, "position", c->position, 3) && floats(env, o, "basis", c->basis, 9) &&
         floats(env, o, "extent", c->extent, 2) && floats(env, o, "jitter", c->jitter, 2);
}

static bool image_size(napi_env env, napi_value w, napi_value h, const char *call, uint32_t *width, uint32_t *height) {
  if (napi_get_value_uint32(env, w, width) != napi_ok || napi_get_value_uint32(env, h, height) != napi_ok) {
    napi_throw_type_error(env, nullptr, (std::string(call) + ": width and height are numbers").c_str());
    return false;
  }
  return true;
}

/* cameraRays(handle, camera, width, height, region [x0, y0, w, h] | null) -> ArrayBuffer(32 w h): flx_camera_rays, the camera's ray rows made on the device */
static napi_value CameraRays(napi_env env, napi_callback_info info) {
  napi_value argv[5];
  if (!get_args(env, info, 5, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  flx_camera c; uint32_t width, height, region[4] = { 0u, 0u, 0u, 0u };
  if (!read_camera(env, argv[1], "cameraRays", &c) || !image_size(env, argv[2], argv[3], "cameraRays", &width, &height)) return nullptr;
  napi_valuetype t;
  napi_typeof(env, argv[4], &t);
  const bool whole = t == napi_null || t == napi_undefined;
  for (uint32_t k = 0; !whole && k < 4u; k++) {
    napi_value e;
    if (napi_get_element(env, argv[4], k, &e) != napi_ok || napi_get_value_uint32(env, e, &region[k]) != napi_ok) {
      napi_throw_type_error(env, nullptr, "cameraRays: region is [x0, y0, w, h] or null");
      return nullptr;
    }
  }
  /* the rows the call writes where it accepts the arguments; one row's room for whatever it refuses */
  const uint64_t w = whole ? width : region[2], h = whole ? height : region[3];
  const uint64_t rows = (w == 0u || h == 0u || w > width || h > height || (uint64_t)width * height > 0xffffffffull) ? 1u : w * h;
  void *rays = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, (size_t)rows * 32u, &rays, &buf));
  flx_status rc = flx_camera_rays(ctx, &c, 1u, width, height, whole ? nullptr : region, (float *)rays);
  if (rc != FLX_OK) return fail(env, ctx, "flx_camera_rays", rc);
  return buf;
}

/* the image's room where the library accepts the size; one pixel's for whatever it refuses */
static size_t image_bytes(uint32_t width, uint32_t height) {
  const uint64_t pixels = (uint64_t)width * height;
  return (size_t)((pixels == 0u || pixels > 0xffffffffull) ? 1u : pixels) * 16u;
}

/* cameraImage(handle, camera, width, height, params (traceRays'), hdr) -> ArrayBuffer(16 width height): flx_camera_image — rayImage with the rays made on the device */
static napi_value CameraImage(napi_env env, napi_callback_info info) {
  napi_value argv[6];
  if (!get_args(env, info, 6, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  flx_camera c; uint32_t width, height; flx_trace_params p;
  if (!read_camera(env, argv[1], "cameraImage", &c) || !image_size(env, argv[2], argv[3], "cameraImage", &width, &height) || !read_trace_params(env, argv[4], "cameraImage", &p)) return nullptr;
  bool hdr = true;
  if (napi_get_value_bool(env, argv[5], &hdr) != napi_ok) { napi_throw_type_error(env, nullptr, "cameraImage: hdr is a boolean"); return nullptr; }
  void *image = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, image_bytes(width, height), &image, &buf));
  flx_status rc = flx_camera_image(ctx, &p, hdr ? 1 : 0, &c, width, height, (float *)image);
  if (rc != FLX_OK) return fail(env, ctx, "flx_camera_image", rc);
  return buf;
}

/* cameraImageTemporal(handle, camera, width, height, params, { history, temporalSamples, filter, hdr }) -> ArrayBuffer(16 width height): flx_camera_image_temporal */
static napi_value CameraImageTemporal(napi_env env, napi_callback_info info) {
  napi_value argv[6];
  if (!get_args(env, info, 6, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  flx_camera c; uint32_t width, height; flx_trace_params p; flx_ray_temporal t;
  if (!read_camera(env, argv[1], "cameraImageTemporal", &c) || !image_size(env, argv[2], argv[3], "cameraImageTemporal", &width, &height) ||
      !read_trace_params(env, argv[4], "cameraImageTemporal", &p) || !read_ray_temporal(env, argv[5], "cameraImageTemporal", &t)) return nullptr;
  void *image = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, image_bytes(width, height), &image, &buf));
  flx_status rc = flx_camera_image_temporal(ctx, &p, &t, &c, width, height, (float *)image);
  if (rc != FLX_OK) return fail(env, ctx, "flx_camera_image_temporal", rc);
  return buf;
}

/* ---- ray images with a volume: the four image calls above and the planes with bakeVolume's handle and a gain behind them (include/flexlight_hip_debug.h "ray images
 * with a volume").  The library's host calls take host rays and a volume whose arrays are on the device, which is what a handle holds. */
static bool read_gather_volume(napi_env env, napi_value volume, napi_value gain, CtxBox *box, const char *call, flx_gather_volume *v) {
  VolumeBox *vb = get_volume(env, volume, box);
  if (!vb) return false;
  double g = 0;
  if (napi_get_value_double(env, gain, &g) != napi_ok) { napi_throw_type_error(env, nullptr, (std::string(call) + ": gain is not a number").c_str()); return false; }
  memset(v, 0, sizeof *v);
  v->grid = &vb->grid; v->sh = vb->d_sh;
  v->map = vb->d_maps ? &vb->map : nullptr; v->maps = vb->d_maps;
  v->offsets = vb->d_offsets;
  v->gain = (float)g;
  return true;
}

/* rayPlanesGather(handle, rays Float32Array(8 n), params (traceRays'), volume, gain) -> ArrayBuffer(20 n): flx_rays_planes_gather's five RGBA8 planes, plane p from
 * texel p n */
static napi_value RayPlanesGather(napi_env env, napi_callback_info info) {
  napi_value argv[5];
  if (!get_args(env, info, 5, argv)) return nullptr;
  CtxBox *box = get_box(env, argv[0]);
  if (!box) return nullptr;
  void *rays; size_t len;
  if (!typed(env, argv[1], napi_float32_array, &rays, &len)) return nullptr;
  if (len % 8 != 0 || len / 8 > 0xffffffffu) { napi_throw_range_error(env, nullptr, "rayPlanesGather: a ray needs 8 floats (origin, noise x, direction, noise y)"); return nullptr; }
  flx_trace_params p; flx_gather_volume v;
  if (!read_trace_params(env, argv[2], "rayPlanesGather", &p) || !read_gather_volume(env, argv[3], argv[4], box, "rayPlanesGather", &v)) return nullptr;
  const size_t n = len / 8;
  void *planes = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, n * 20, &planes, &buf));
  flx_status rc = flx_rays_planes_gather(box->ctx, &p, &v, (const float *)rays, (uint32_t)n, planes, nullptr);
  if (rc != FLX_OK) return fail(env, box->ctx, "flx_rays_planes_gather", rc);
  return buf;
}

/* rayImageGather(handle, rays, width, height, params, hdr, volume, gain) -> ArrayBuffer(16 width height): flx_rays_image_gather — rayImage lit by the volume */
static napi_value RayImageGather(napi_env env, napi_callback_info info) {
  napi_value argv[8];
  if (!get_args(env, info, 8, argv)) return nullptr;
  CtxBox *box = get_box(env, argv[0]);
  if (!box) return nullptr;
  void *rays; size_t len; uint32_t width, height;
  if (!typed(env, argv[1], napi_float32_array, &rays, &len) || !image_size(env, argv[2], argv[3], "rayImageGather", &width, &height)) return nullptr;
  if (len % 8 != 0 || (uint64_t)(len / 8) != (uint64_t)width * height) { napi_throw_range_error(env, nullptr, "rayImageGather: width * height rays of 8 floats (origin, noise x, direction, noise y)"); return nullptr; }
  flx_trace_params p; flx_gather_volume v;
  if (!read_trace_params(env, argv[4], "rayImageGather", &p)) return nullptr;
  bool hdr = true;
  if (napi_get_value_bool(env, argv[5], &hdr) != napi_ok) { napi_throw_type_error(env, nullptr, "rayImageGather: hdr is a boolean"); return nullptr; }
  if (!read_gather_volume(env, argv[6], argv[7], box, "rayImageGather", &v)) return nullptr;
  void *image = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, (len / 8) * 16, &image, &buf));
  flx_status rc = flx_rays_image_gather(box->ctx, &p, &v, hdr ? 1 : 0, (const float *)rays, width, height, (float *)image);
  if (rc != FLX_OK) return fail(env, box->ctx, "flx_rays_image_gather", rc);
  return buf;
}

/* rayImageTemporalGather(handle, rays, width, height, params, { history, temporalSamples, filter, hdr }, volume, gain) -> ArrayBuffer(16 width height):
 * flx_rays_image_temporal_gather, over the same histories as rayImageTemporal */
static napi_value RayImageTemporalGather(napi_env env, napi_callback_info info) {
  napi_value argv[8];
  if (!get_args(env, info, 8, argv)) return nullptr;
  CtxBox *box = get_box(env, argv[0]);
  if (!box) return nullptr;
  void *rays; size_t len; uint32_t width, height;
  if (!typed(env, argv[1], napi_float32_array, &rays, &len) || !image_size(env, argv[2], argv[3], "rayImageTemporalGather", &width, &height)) return nullptr;
  if (len % 8 != 0 || (uint64_t)(len / 8) != (uint64_t)width * height) { napi_throw_range_error(env, nullptr, "rayImageTemporalGather: width * height rays of 8 floats (origin, noise x, direction, noise y)"); return nullptr; }
  flx_trace_params p; flx_ray_temporal t; flx_gather_volume v;
  if (!read_trace_params(env, argv[4], "rayImageTemporalGather", &p) || !read_ray_temporal(env, argv[5], "rayImageTemporalGather", &t) ||
      !read_gather_volume(env, argv[6], argv[7], box, "rayImageTemporalGather", &v)) return nullptr;
  void *image = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, (len / 8) * 16, &image, &buf));
  flx_status rc = flx_rays_image_temporal_gather(box->ctx, &p, &v, &t, (const float *)rays, width, height, (float *)image);
  if (rc != FLX_OK) return fail(env, box->ctx, "flx_rays_image_temporal_gather", rc);
  return buf;
}

/* cameraImageGather(handle, camera, width, height, params, hdr, volume, gain) -> ArrayBuffer(16 width height): flx_camera_image_gather */
static napi_value CameraImageGather(napi_env env, napi_callback_info info) {
  napi_value argv[8];
  if (!get_args(env, info, 8, argv)) return nullptr;
  CtxBox *box = get_box(env, argv[0]);
  if (!box) return nullptr;
  flx_camera c; uint32_t width, height; flx_trace_params p; flx_gather_volume v;
  if (!read_camera(env, argv[1], "cameraImageGather", &c) || !image_size(env, argv[2], argv[3], "cameraImageGather", &width, &height) ||
      !read_trace_params(env, argv[4], "cameraImageGather", &p)) return nullptr;
  bool hdr = true;
  if (napi_get_value_bool(env, argv[5], &hdr) != napi_ok) { napi_throw_type_error(env, nullptr, "cameraImageGather: hdr is a boolean"); return nullptr; }
  if (!read_gather_volume(env, argv[6], argv[7], box, "cameraImageGather", &v)) return nullptr;
  void *image = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, image_bytes(width, height), &image, &buf));
  flx_status rc = flx_camera_image_gather(box->ctx, &p, &v, hdr ? 1 : 0, &c, width, height, (float *)image);
  if (rc != FLX_OK) return fail(env, box->ctx, "flx_camera_image_gather", rc);
  return buf;
}

/* cameraImageTemporalGather(handle, camera, width, height, params, { history, temporalSamples, filter, hdr }, volume, gain) -> ArrayBuffer(16 width height):
 * flx_camera_image_temporal_gather */
static napi_value CameraImageTemporalGather(napi_env env, napi_callback_info info) {
  napi_value argv[8];
  if (!get_args(env, info, 8, argv)) return nullptr;
  CtxBox *box = get_box(env, argv[0]);
  if (!box) return nullptr;
  flx_camera c; uint32_t width, height; flx_trace_params p; flx_ray_temporal t; flx_gather_volume v;
  if (!read_camera(env, argv[1], "cameraImageTemporalGather", &c) || !image_size(env, argv[2], argv[3], "cameraImageTemporalGather", &width, &height) ||
      !read_trace_params(env, argv[4], "cameraImageTemporalGather", &p) || !read_ray_temporal(env, argv[5], "cameraImageTemporalGather", &t) ||
      !read_gather_volume(env, argv[6], argv[7], box, "cameraImageTemporalGather", &v)) return nullptr;
  void *image = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, image_bytes(width, height), &image, &buf));
  flx_status rc = flx_camera_image_temporal_gather(box->ctx, &p, &v, &t, &c, width, height, (float *)image);
  if (rc != FLX_OK) return fail(env, box->ctx, "flx_camera_image_temporal_gather", rc);
  return buf;
}

/* rayHistoryReset(handle, history): flx_rays_history_reset, -1 for all of the context's ray-image histories */
static napi_value RayHistoryReset(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  int32_t history = -1;
  if (napi_get_value_int32(env, argv[1], &history) != napi_ok) { napi_throw_type_error(env, nullptr, "rayHistoryReset: history is a number"); return nullptr; }
  flx_status rc = flx_rays_history_reset(ctx, history);
  if (rc != FLX_OK) return fail(env, ctx, "flx_rays_history_reset", rc);
  return nullptr;
}

/* the planes a surface call may write: popcount(fields) for fields the library takes; anything else is left to the library to refuse, with room for one plane */
static size_t surface_planes(uint32_t fields) {
  size_t planes = 0;
  if (fields <= 255u) for (uint32_t f = fields; f != 0u; f &= f - 1u) planes++;
  return planes ? planes : 1;
}
/* surfaceRays(handle, rays Float32Array(8 n), fields, textureWidth) -> ArrayBuffer(popcount(fields) * n * 16): flx_rays_surface, the planes as the library writes them
 * (include/flexlight_hip_debug.h, "surface rows") */
static napi_value SurfaceRays(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  void *rays; size_t len; uint32_t fields; int32_t tw;
  if (!typed(env, argv[1], napi_float32_array, &rays, &len)) return nullptr;
  if (napi_get_value_uint32(env, argv[2], &fields) != napi_ok) { napi_throw_type_error(env, nullptr, "surfaceRays: fields is not a number"); return nullptr; }
  if (napi_get_value_int32(env, argv[3], &tw) != napi_ok) { napi_throw_type_error(env, nullptr, "surfaceRays: textureWidth is not a number"); return nullptr; }
  if (len % 8 != 0 || len / 8 > 0xffffffffu) { napi_throw_range_error(env, nullptr, "surfaceRays: a ray needs 8 floats (origin, one unused, direction, one unused)"); return nullptr; }
  void *planes = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, surface_planes(fields) * (len / 8) * 16, &planes, &buf));
  flx_status rc = flx_rays_surface(ctx, tw, (const float *)rays, (uint32_t)(len / 8), fields, planes);
  if (rc != FLX_OK) return fail(env, ctx, "flx_rays_surface", rc);
  return buf;
}
/* frameSurface(handle, params, fields) -> ArrayBuffer(popcount(fields) * width * height * 16): flx_frame_surface */
static napi_value FrameSurface(napi_env env, napi_callback_info info) {
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  flx_frame_params p;
  uint32_t fields;
  if (!read_params(env, argv[1], &p)) return nullptr;
  if (napi_get_value_uint32(env, argv[2], &fields) != napi_ok) { napi_throw_type_error(env, nullptr, "frameSurface: fields is not a number"); return nullptr; }
  if ((uint64_t)p.width * p.height > 0xffffffffull) { napi_throw_range_error(env, nullptr, "frameSurface: the frame has more than 2^32 - 1 pixels"); return nullptr; }
  void *planes = nullptr;
  napi_value buf;
  NAPI_OK(env, napi_create_arraybuffer(env, surface_planes(fields) * (size_t)p.width * p.height * 16, &planes, &buf));
  flx_status rc = flx_frame_surface(ctx, &p, fields, planes);
  if (rc != FLX_OK) return fail(env, ctx, "flx_frame_surface", rc);
  return buf;
}

/* tileRowCount(params) -> rows this context renders */
static napi_value TileRowCount(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  if (!get_args(env, info, 1, argv)) return nullptr;
  flx_frame_params p;
  if (!read_params(env, argv[0], &p)) return nullptr;
  napi_value r;
  NAPI_OK(env, napi_create_uint32(env, flx_tile_row_count(&p), &r));
  return r;
}

/* render(handle, params, out Float32Array(rows*width*4), wantCounters) -> { frameMs, traceMs, counters? } */
static napi_value Render(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  flx_frame_params p;
  if (!read_params(env, argv[1], &p)) return nullptr;
  void *out; size_t n;
  if (!typed(env, argv[2], napi_float32_array, &out, &n)) return nullptr;
  if (!out || n != (size_t)flx_tile_row_count(&p) * p.width * 4) { napi_throw_range_error(env, nullptr, "out needs rows*width*4 floats"); return nullptr; }
  bool want = false;
  napi_get_value_bool(env, argv[3], &want);
  flx_counters c;
  flx_status rc = flx_render(ctx, &p, (float *)out, nullptr, want ? &c : nullptr);
  if (rc != FLX_OK) return fail(env, ctx, "flx_render", rc);
  float frame_ms = 0.f, trace_ms = 0.f;
  flx_last_frame_ms(ctx, &frame_ms, &trace_ms);
  napi_value res, v;
  NAPI_OK(env, napi_create_object(env, &res));
  napi_create_double(env, frame_ms, &v); napi_set_named_property(env, res, "frameMs", v);
  napi_create_double(env, trace_ms, &v); napi_set_named_property(env, res, "traceMs", v);
  if (want) {
    napi_value co;
    napi_create_object(env, &co);
    const char *names[8] = { "primaryVisits", "closestVisits", "shadowVisits", "closestWalks", "shadowWalks", "shades", "primaryHits", "atlasTexels" };
    const uint64_t vals[8] = { c.primary_visits, c.closest_visits, c.shadow_visits, c.closest_walks, c.shadow_walks, c.shades, c.primary_hits, c.atlas_texels };
    for (int i = 0; i < 8; i++) { napi_create_double(env, (double)vals[i], &v); napi_set_named_property(env, co, names[i], v); }
    napi_set_named_property(env, res, "counters", co);
  }
  return res;
}

/* rasterRender(handle, params, out Float32Array(rows*width*4), wantCounters) -> { frameMs, counters? }: the rasterizer renderer
 * (flx_raster_render), synchronous */
static napi_value RasterRender(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  flx_frame_params p;
  if (!read_params(env, argv[1], &p)) return nullptr;
  void *out; size_t n;
  if (!typed(env, argv[2], napi_float32_array, &out, &n)) return nullptr;
  if (!out || n != (size_t)flx_tile_row_count(&p) * p.width * 4) { napi_throw_range_error(env, nullptr, "out needs rows*width*4 floats"); return nullptr; }
  bool want = false;
  napi_get_value_bool(env, argv[3], &want);
  flx_counters c;
  flx_status rc = flx_raster_render(ctx, &p, (float *)out, nullptr, want ? &c : nullptr);
  if (rc != FLX_OK) return fail(env, ctx, "flx_raster_render", rc);
  float frame_ms = 0.f;
  flx_last_frame_ms(ctx, &frame_ms, nullptr);
  napi_value res, v;
  NAPI_OK(env, napi_create_object(env, &res));
  napi_create_double(env, frame_ms, &v); napi_set_named_property(env, res, "frameMs", v);
  if (want) {
    napi_value co;
    napi_create_object(env, &co);
    const char *names[8] = { "primaryVisits", "closestVisits", "shadowVisits", "closestWalks", "shadowWalks", "shades", "primaryHits", "atlasTexels" };
    const uint64_t vals[8] = { c.primary_visits, c.closest_visits, c.shadow_visits, c.closest_walks, c.shadow_walks, c.shades, c.primary_hits, c.atlas_texels };
    for (int i = 0; i < 8; i++) { napi_create_double(env, (double)vals[i], &v); napi_set_named_property(env, co, names[i], v); }
    napi_set_named_property(env, res, "counters", co);
  }
  return res;
}

/* renderBatch(handle, [params, ...], out Float32Array, wantCounters) -> { frameMs, counters? }: flx_render_batch, the frames
 * one after the other in `out` */
static napi_value RenderBatch(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  uint32_t count = 0;
  bool isArray = false;
  napi_is_array(env, argv[1], &isArray);
  if (!isArray || napi_get_array_length(env, argv[1], &count) != napi_ok || count < 1 || count > FLX_MAX_BATCH_FRAMES) {
    napi_throw_range_error(env, nullptr, "renderBatch: an array of 1 .. 32 frame parameter objects");
    return nullptr;
  }
  flx_frame_params p[FLX_MAX_BATCH_FRAMES];
  for (uint32_t i = 0; i < count; i++) {
    napi_value e;
    NAPI_OK(env, napi_get_element(env, argv[1], i, &e));
    if (!read_params(env, e, &p[i])) return nullptr;
  }
  void *out; size_t n;
  if (!typed(env, argv[2], napi_float32_array, &out, &n)) return nullptr;
  if (!out || n != (size_t)count * flx_tile_row_count(&p[0]) * p[0].width * 4) { napi_throw_range_error(env, nullptr, "out needs frames*rows*width*4 floats"); return nullptr; }
  bool want = false;
  napi_get_value_bool(env, argv[3], &want);
  flx_counters c;
  flx_status rc = flx_render_batch(ctx, p, count, (float *)out, want ? &c : nullptr);
  if (rc != FLX_OK) return fail(env, ctx, "flx_render_batch", rc);
  float frame_ms = 0.f, trace_ms = 0.f;
  flx_last_frame_ms(ctx, &frame_ms, &trace_ms);
  napi_value res, v;
  NAPI_OK(env, napi_create_object(env, &res));
  napi_create_double(env, frame_ms, &v); napi_set_named_property(env, res, "frameMs", v);
  if (want) {
    napi_value co;
    napi_create_object(env, &co);
    const char *names[8] = { "primaryVisits", "closestVisits", "shadowVisits", "closestWalks", "shadowWalks", "shades", "primaryHits", "atlasTexels" };
    const uint64_t vals[8] = { c.primary_visits, c.closest_visits, c.shadow_visits, c.closest_walks, c.shadow_walks, c.shades, c.primary_hits, c.atlas_texels };
    for (int i = 0; i < 8; i++) { napi_create_double(env, (double)vals[i], &v); napi_set_named_property(env, co, names[i], v); }
    napi_set_named_property(env, res, "counters", co);
  }
  return res;
}

/* temporalReset(handle): forget the temporal history */
static napi_value TemporalReset(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  if (!get_args(env, info, 1, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  flx_status rc = flx_temporal_reset(ctx);
  if (rc != FLX_OK) return fail(env, ctx, "flx_temporal_reset", rc);
  return nullptr;
}

/* deviceInfo(handle) -> { name, computeUnits } */
static napi_value DeviceInfo(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  if (!get_args(env, info, 1, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  char name[256]; uint32_t cus = 0;
  flx_device_info(ctx, name, sizeof name, &cus);
  napi_value res, v;
  NAPI_OK(env, napi_create_object(env, &res));
  napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &v); napi_set_named_property(env, res, "name", v);
  napi_create_uint32(env, cus, &v); napi_set_named_property(env, res, "computeUnits", v);
  return res;
}

/* ---- native scene import (flx_mesh_*): meshImport(objText, mtlText | null) -> handle; the Object3D operations; counts; flatten -- */
static void mesh_finalize(napi_env, void *data, void *) {
  flx_mesh **box = static_cast<flx_mesh **>(data);
  if (*box) flx_mesh_destroy(*box);
  delete box;
}
static flx_mesh *get_mesh(napi_env env, napi_value v) {
  void *p = nullptr;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p || !*static_cast<flx_mesh **>(p)) { napi_throw_type_error(env, nullptr, "expected a mesh handle"); return nullptr; }
  return *static_cast<flx_mesh **>(p);
}
static bool get_text(napi_env env, napi_value v, std::string &out, bool &present) {
  napi_valuetype t;
  napi_typeof(env, v, &t);
  present = !(t == napi_null || t == napi_undefined);
  if (!present) return true;
  size_t len = 0;
  if (napi_get_value_string_utf8(env, v, nullptr, 0, &len) != napi_ok) { napi_throw_type_error(env, nullptr, "expected a string"); return false; }
  out.resize(len + 1);
  napi_get_value_string_utf8(env, v, &out[0], len + 1, &len);
  out.resize(len);
  return true;
}
static napi_value MeshImport(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return nullptr;
  std::string obj, mtl; bool hasObj = false, hasMtl = false;
  if (!get_text(env, argv[0], obj, hasObj) || !get_text(env, argv[1], mtl, hasMtl)) return nullptr;
  if (!hasObj) { napi_throw_type_error(env, nullptr, "meshImport: OBJ text expected"); return nullptr; }
  flx_mesh *m = nullptr;
  if (flx_mesh_import_obj(obj.data(), obj.size(), hasMtl ? mtl.data() : nullptr, mtl.size(), &m) != FLX_OK) { napi_throw_error(env, nullptr, "flx_mesh_import_obj failed"); return nullptr; }
  flx_mesh **box = new flx_mesh *(m);
  napi_value ext;
  NAPI_OK(env, napi_create_external(env, box, mesh_finalize, nullptr, &ext));
  return ext;
}
static napi_value MeshCounts(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  if (!get_args(env, info, 1, argv)) return nullptr;
  flx_mesh *m = get_mesh(env, argv[0]);
  if (!m) return nullptr;
  napi_value res, v;
  NAPI_OK(env, napi_create_object(env, &res));
  napi_create_uint32(env, flx_mesh_entry_count(m), &v); napi_set_named_property(env, res, "entries", v);
  napi_create_uint32(env, flx_mesh_triangle_count(m), &v); napi_set_named_property(env, res, "triangles", v);
  return res;
}
static napi_value MeshSetTransform(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return nullptr;
  flx_mesh *m = get_mesh(env, argv[0]);
  if (!m) return nullptr;
  uint32_t n = 0;
  NAPI_OK(env, napi_get_value_uint32(env, argv[1], &n));
  flx_mesh_set_transform(m, n);
  return nullptr;
}
static napi_value MeshMove(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  flx_mesh *m = get_mesh(env, argv[0]);
  if (!m) return nullptr;
  double d[3];
  for (int i = 0; i < 3; i++) NAPI_OK(env, napi_get_value_double(env, argv[1 + i], &d[i]));
  flx_mesh_move(m, d[0], d[1], d[2]);
  return nullptr;
}
static napi_value MeshScale(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return nullptr;
  flx_mesh *m = get_mesh(env, argv[0]);
  if (!m) return nullptr;
  double s = 1;
  NAPI_OK(env, napi_get_value_double(env, argv[1], &s));
  flx_mesh_scale(m, s);
  return nullptr;
}
/* meshSetMaterial(handle, field, Float64Array values) */
static napi_value MeshSetMaterial(napi_env env, napi_callback_info info) {
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return nullptr;
  flx_mesh *m = get_mesh(env, argv[0]);
  if (!m) return nullptr;
  int32_t field = 0;
  NAPI_OK(env, napi_get_value_int32(env, argv[1], &field));
  void *vals = nullptr; size_t n = 0;
  if (!typed(env, argv[2], napi_float64_array, &vals, &n)) return nullptr;
  if (n < 3) { napi_throw_type_error(env, nullptr, "meshSetMaterial: Float64Array(3) expected"); return nullptr; }
  if (flx_mesh_set_material(m, field, static_cast<const double *>(vals)) != FLX_OK) { napi_throw_error(env, nullptr, "flx_mesh_set_material: unknown field"); return nullptr; }
  return nullptr;
}
static napi_value MeshBounding(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  if (!get_args(env, info, 1, argv)) return nullptr;
  flx_mesh *m = get_mesh(env, argv[0]);
  if (!m) return nullptr;
  double box[6];
  flx_mesh_bounding(m, box);
  napi_value res;
  NAPI_OK(env, napi_create_array_with_length(env, 6, &res));
  for (uint32_t i = 0; i < 6; i++) { napi_value v; napi_create_double(env, box[i], &v); napi_set_element(env, res, i, v); }
  return res;
}
/* meshFlatten(handle, Float32Array geometry[12 * entries], Float32Array attributes[28 * entries], Int32Array ids[triangles]) -> [min xyz, max xyz] */
static napi_value MeshFlatten(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  flx_mesh *m = get_mesh(env, argv[0]);
  if (!m) return nullptr;
  void *g = nullptr, *a = nullptr, *ids = nullptr; size_t ng = 0, na = 0, ni = 0;
  if (!typed(env, argv[1], napi_float32_array, &g, &ng) || !typed(env, argv[2], napi_float32_array, &a, &na) || !typed(env, argv[3], napi_int32_array, &ids, &ni)) return nullptr;
  const size_t e = flx_mesh_entry_count(m), t = flx_mesh_triangle_count(m);
  if (ng < 12 * e || na < 28 * e || ni < t) { napi_throw_range_error(env, nullptr, "meshFlatten: arrays too small"); return nullptr; }
  float box[6] = { 0, 0, 0, 0, 0, 0 };
  if (flx_mesh_flatten(m, static_cast<float *>(g), static_cast<float *>(a), static_cast<int32_t *>(ids), box) != FLX_OK) { napi_throw_error(env, nullptr, "flx_mesh_flatten failed"); return nullptr; }
  napi_value res;
  NAPI_OK(env, napi_create_array_with_length(env, 6, &res));
  for (uint32_t i = 0; i < 6; i++) { napi_value v; napi_create_double(env, box[i], &v); napi_set_element(env, res, i, v); }
  return res;
}

/* fxaa / taa (handle, width, height, Float32Array in, Float32Array out); taaReset(handle) */
static napi_value post_pass(napi_env env, napi_callback_info info, int which) {
  napi_value argv[5];
  if (!get_args(env, info, 5, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  uint32_t w = 0, h = 0;
  NAPI_OK(env, napi_get_value_uint32(env, argv[1], &w));
  NAPI_OK(env, napi_get_value_uint32(env, argv[2], &h));
  void *in = nullptr, *out = nullptr; size_t ni = 0, no = 0;
  if (!typed(env, argv[3], napi_float32_array, &in, &ni) || !typed(env, argv[4], napi_float32_array, &out, &no)) return nullptr;
  if (ni < (size_t)w * h * 4 || no < (size_t)w * h * 4) { napi_throw_range_error(env, nullptr, "anti-aliasing pass: arrays smaller than width * height * 4"); return nullptr; }
  flx_status rc = which == 0 ? flx_fxaa(ctx, w, h, static_cast<const float *>(in), static_cast<float *>(out))
                             : flx_taa(ctx, w, h, static_cast<const float *>(in), static_cast<float *>(out));
  if (rc != FLX_OK) return fail(env, ctx, which == 0 ? "flx_fxaa" : "flx_taa", rc);
  return nullptr;
}
/* present(handle, width, height, in Float32Array, out Uint8Array | Uint8ClampedArray): the canvas' RGBA8 drawing buffer */
static napi_value Present(napi_env env, napi_callback_info info) {
  napi_value argv[5];
  if (!get_args(env, info, 5, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  uint32_t w = 0, h = 0;
  napi_get_value_uint32(env, argv[1], &w); napi_get_value_uint32(env, argv[2], &h);
  void *in; size_t n_in;
  if (!typed(env, argv[3], napi_float32_array, &in, &n_in)) return nullptr;
  napi_typedarray_type type; size_t n_out; void *out; napi_value buf; size_t off;
  if (napi_get_typedarray_info(env, argv[4], &type, &n_out, &out, &buf, &off) != napi_ok || (type != napi_uint8_array && type != napi_uint8_clamped_array)) {
    napi_throw_type_error(env, nullptr, "present: out must be a Uint8Array or Uint8ClampedArray");
    return nullptr;
  }
  if (!in || !out || n_in != (size_t)w * h * 4 || n_out != n_in) { napi_throw_range_error(env, nullptr, "present: in and out need width*height*4 elements"); return nullptr; }
  flx_status rc = flx_present(ctx, w, h, (const float *)in, (uint8_t *)out);
  if (rc != FLX_OK) return fail(env, ctx, "flx_present", rc);
  return nullptr;
}
static napi_value Fxaa(napi_env env, napi_callback_info info) { return post_pass(env, info, 0); }
static napi_value Taa(napi_env env, napi_callback_info info) { return post_pass(env, info, 1); }
static napi_value TaaReset(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  if (!get_args(env, info, 1, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  flx_taa_reset(ctx);
  return nullptr;
}

/* packTransforms(Float64Array matrices[9 T], Float64Array positions[3 T], Float32Array rotation[24 T], Float32Array shift[8 T]) */
static napi_value PackTransforms(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  void *m = nullptr, *p = nullptr, *r = nullptr, *s = nullptr; size_t nm = 0, np = 0, nr = 0, ns = 0;
  if (!typed(env, argv[0], napi_float64_array, &m, &nm) || !typed(env, argv[1], napi_float64_array, &p, &np) ||
      !typed(env, argv[2], napi_float32_array, &r, &nr) || !typed(env, argv[3], napi_float32_array, &s, &ns)) return nullptr;
  const size_t T = nm / 9;
  if (nm != 9 * T || np < 3 * T || nr < 24 * T || ns < 8 * T) { napi_throw_range_error(env, nullptr, "packTransforms: array sizes do not agree"); return nullptr; }
  if (flx_transforms_pack((uint32_t)T, static_cast<const double *>(m), static_cast<const double *>(p), static_cast<float *>(r), static_cast<float *>(s)) != FLX_OK) {
    napi_throw_error(env, nullptr, "flx_transforms_pack failed"); return nullptr;
  }
  return nullptr;
}


/* ---- the frame loop: frameBegin(handle, params, rgba8[, { renderer, antialiasing }]) / frameEnd(handle) -> { pixels, gpuMs } ---------------------------
 * The optional fourth argument: renderer 'rasterizer' (flx_raster_render's frame; anything else: the path tracer's), antialiasing 'fxaa' | 'taa' (the pass
 * inside the loop: FLX_FRAME_FXAA / FLX_FRAME_TAA; anything else: none).
 * `pixels` is a typed array over the context's pinned host buffer (no copy).  It belongs to that frame until the library re-uses
 * or frees the buffer — the frameBegin that will copy a newer frame into it (with two lanes: the fourth after the one that made
 * it; with one lane the second), a frameBegin that re-allocates it for a larger frame, or halt() — at which point the addon
 * DETACHES it: `pixels.length` becomes 0 instead of the array showing another frame or freed memory. */
static int frame_flags(napi_env env, napi_value opts, bool &ok) {
  ok = true;
  napi_valuetype t;
  napi_typeof(env, opts, &t);
  if (t == napi_undefined || t == napi_null) return 0;
  if (t != napi_object) { napi_throw_type_error(env, nullptr, "frameBegin: the fourth argument is { renderer, antialiasing }"); ok = false; return 0; }
  int flags = 0;
  napi_value v;
  std::string text;
  bool present = false;
  if (napi_get_named_property(env, opts, "renderer", &v) != napi_ok || !get_text(env, v, text, present)) { ok = false; return 0; }
  if (present && text == "rasterizer") flags |= FLX_FRAME_RASTERIZER;
  if (napi_get_named_property(env, opts, "antialiasing", &v) != napi_ok || !get_text(env, v, text, present)) { ok = false; return 0; }
  if (present && text == "fxaa") flags |= FLX_FRAME_FXAA;
  else if (present && text == "taa") flags |= FLX_FRAME_TAA;
  return flags;
}
static napi_value FrameBegin(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  size_t argc = 4;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 3) {
    napi_throw_type_error(env, nullptr, "wrong number of arguments");
    return nullptr;
  }
  CtxBox *box = get_box(env, argv[0]);
  if (!box) return nullptr;
  flx_context *ctx = box->ctx;
  flx_frame_params p;
  if (!read_params(env, argv[1], &p)) return nullptr;
  bool rgba8 = false;
  napi_get_value_bool(env, argv[2], &rgba8);
  bool ok = true;
  const int flags = argc > 3 ? frame_flags(env, argv[3], ok) : 0;
  if (!ok) return nullptr;
  flx_status rc = flx_frame_begin(ctx, &p, (rgba8 ? FLX_FRAME_RGBA8 : FLX_FRAME_FLOAT) | flags);
  /* a larger frame (canvas or renderQuality changed) made the library re-allocate a pinned slot: the views over the old one go
   * (no JavaScript has run since the free — this is one native call) */
  const void *slots[4] = { nullptr, nullptr, nullptr, nullptr };
  int begun = -1;
  (void)flx_frame_host_slots(ctx, slots, &begun);
  /* ... and the slot the frame just begun will be copied into stops being the older frame's that was handed out over it */
  const void *reused = (rc == FLX_OK && begun >= 0) ? slots[begun] : nullptr;
  detach_views(env, box, [&](const void *q) { return q != reused && (q == slots[0] || q == slots[1] || q == slots[2] || q == slots[3]); });
  if (rc != FLX_OK) return fail(env, ctx, "flx_frame_begin", rc);
  return nullptr;
}
static void no_free(napi_env, void *, void *) {}
/* { pixels, gpuMs } over the pinned slot (or the group's image) the frame is in */
static napi_value frame_result(napi_env env, std::vector<CtxBox::View> &views, const void *pixels, size_t bytes, float ms, bool rgba8) {
  napi_value res, buf, arr, v;
  NAPI_OK(env, napi_create_object(env, &res));
  NAPI_OK(env, napi_create_external_arraybuffer(env, const_cast<void *>(pixels), bytes, no_free, nullptr, &buf));
  {
    CtxBox::View view = { pixels, nullptr };
    NAPI_OK(env, napi_create_reference(env, buf, 0, &view.ref));      /* weak: the view lives as long as JavaScript holds it */
    views.push_back(view);
  }
  if (rgba8) NAPI_OK(env, napi_create_typedarray(env, napi_uint8_clamped_array, bytes, buf, 0, &arr));
  else NAPI_OK(env, napi_create_typedarray(env, napi_float32_array, bytes / 4, buf, 0, &arr));
  napi_set_named_property(env, res, "pixels", arr);
  napi_create_double(env, ms, &v); napi_set_named_property(env, res, "gpuMs", v);
  return res;
}
static napi_value FrameEnd(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return nullptr;
  CtxBox *box = get_box(env, argv[0]);
  if (!box) return nullptr;
  flx_context *ctx = box->ctx;
  bool rgba8 = false;
  napi_get_value_bool(env, argv[1], &rgba8);
  const void *pixels = nullptr; size_t bytes = 0; float ms = 0.f;
  flx_status rc = flx_frame_end(ctx, &pixels, &bytes, &ms);
  if (rc != FLX_OK) return fail(env, ctx, "flx_frame_end", rc);
  /* the slot now holds THIS frame: an older frame's view of the same memory (two frames back on this lane) is detached */
  detach_views(env, box, [&](const void *q) { return q != pixels; });
  return frame_result(env, box->views, pixels, bytes, ms, rgba8);
}

static napi_value FramesInFlight(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  if (!get_args(env, info, 1, argv)) return nullptr;
  flx_context *ctx = get_ctx(env, argv[0]);
  if (!ctx) return nullptr;
  napi_value v;
  napi_create_int32(env, flx_frames_in_flight(ctx), &v);
  return v;
}

/* ---- several GPUs in this process (flx_group_*): the same calls with a group handle -------------------------------------- */
/* What a group handle points to: the group and the ArrayBuffers handed out over its frame images (groupFrameEnd), detached when their memory stops being
 * that frame's (CtxBox above does the same for one context). */
struct GroupBox {
  flx_group *g = nullptr;                  /* first member: a handle also reads as flx_group ** */
  std::vector<CtxBox::View> views;
  bool busy = false;                       /* a groupFrameEndAsync is pending */
};
static void detach_group_views(napi_env env, GroupBox *box) {
  for (auto &v : box->views) detach_view(env, v);
  box->views.clear();
}
static void finalize_group(napi_env env, void *data, void *) {
  GroupBox *box = static_cast<GroupBox *>(data);
  for (auto &v : box->views) napi_delete_reference(env, v.ref);
  if (box->g) flx_group_destroy(box->g);
  delete box;
}
static GroupBox *get_group_box(napi_env env, napi_value v) {
  void *p = nullptr;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p) { napi_throw_type_error(env, nullptr, "expected a group handle"); return nullptr; }
  GroupBox *box = static_cast<GroupBox *>(p);
  if (!box->g) { napi_throw_error(env, nullptr, "group was halted"); return nullptr; }
  if (box->busy) { napi_throw_error(env, nullptr, "a groupFrameEndAsync of this group is pending: await it first"); return nullptr; }
  return box;
}
static flx_group *get_group(napi_env env, napi_value v) {
  GroupBox *box = get_group_box(env, v);
  return box ? box->g : nullptr;
}
static napi_value gfail(napi_env env, flx_group *g, const char *what, flx_status rc) {
  std::string msg = std::string(what) + " failed (" + std::to_string(rc) + "): " + flx_group_last_error(g);
  napi_throw_error(env, nullptr, msg.c_str());
  return nullptr;
}
/* createGroup([device, ...]) -> handle */
static napi_value CreateGroup(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  if (!get_args(env, info, 1, argv)) return nullptr;
  uint32_t n = 0;
  bool isArray = false;
  napi_is_array(env, argv[0], &isArray);
  if (!isArray || napi_get_array_length(env, argv[0], &n) != napi_ok || n < 1 || n > 64) { napi_throw_range_error(env, nullptr, "createGroup: an array of 1 .. 64 device numbers"); return nullptr; }
  int devices[64];
  for (uint32_t i = 0; i < n; i++) { napi_value e; int32_t d = 0; napi_get_element(env, argv[0], i, &e); NAPI_OK(env, napi_get_value_int32(env, e, &d)); devices[i] = d; }
  flx_group *g = nullptr;
  flx_status rc = flx_group_create((int)n, devices, &g);
  if (rc != FLX_OK) return gfail(env, nullptr, "flx_group_create", rc);
  napi_value ext;
  GroupBox *box = new GroupBox();
  box->g = g;
  NAPI_OK(env, napi_create_external(env, box, finalize_group, nullptr, &ext));
  return ext;
}
static napi_value DestroyGroup(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  if (!get_args(env, info, 1, argv)) return nullptr;
  void *p = nullptr;
  if (napi_get_value_external(env, argv[0], &p) == napi_ok && p) {
    GroupBox *box = static_cast<GroupBox *>(p);
    if (box->busy) { napi_throw_error(env, nullptr, "destroyGroup: a groupFrameEndAsync is pending: await it first"); return nullptr; }
    detach_group_views(env, box);          /* the images are freed with the group: whoever still holds a frame reads an empty array */
    if (box->g) { flx_group_destroy(box->g); box->g = nullptr; }
  }
  return nullptr;
}
static napi_value GroupInfo(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  if (!get_args(env, info, 1, argv)) return nullptr;
  flx_group *g = get_group(env, argv[0]);
  if (!g) return nullptr;
  napi_value res, v;
  NAPI_OK(env, napi_create_object(env, &res));
  napi_create_int32(env, flx_group_size(g), &v); napi_set_named_property(env, res, "size", v);
  napi_get_boolean(env, flx_group_uses_rccl(g) != 0, &v); napi_set_named_property(env, res, "rccl", v);
  return res;
}
static napi_value GroupUploadScene(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  flx_group *grp = get_group(env, argv[0]);
  if (!grp) return nullptr;
  void *g, *a, *ids; size_t ng, na, nids;
  if (!typed(env, argv[1], napi_float32_array, &g, &ng) || !typed(env, argv[2], napi_float32_array, &a, &na) ||
      !typed(env, argv[3], napi_int32_array, &ids, &nids)) return nullptr;
  if (ng % 12 != 0 || na / 28 != ng / 12 || na % 28 != 0) { napi_throw_range_error(env, nullptr, "geometry needs 12 and attributes 28 floats per entry"); return nullptr; }
  flx_status rc = flx_group_scene_upload(grp, (const float *)g, (const float *)a, (uint32_t)(ng / 12), (const int32_t *)ids, (uint32_t)nids);
  if (rc != FLX_OK) return gfail(env, grp, "flx_group_scene_upload", rc);
  return nullptr;
}
static napi_value GroupUpdateSceneRows(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  flx_group *grp = get_group(env, argv[0]);
  if (!grp) return nullptr;
  uint32_t first, n; const float *g, *a;
  if (!row_args(env, argv + 1, &first, &g, &a, &n)) return nullptr;
  flx_status rc = flx_group_scene_update(grp, first, n, g, a);
  if (rc != FLX_OK) return gfail(env, grp, "flx_group_scene_update", rc);
  return nullptr;
}
static napi_value GroupUploadTransforms(napi_env env, napi_callback_info info) {
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return nullptr;
  flx_group *grp = get_group(env, argv[0]);
  if (!grp) return nullptr;
  void *r, *s; size_t nr, ns;
  if (!typed(env, argv[1], napi_float32_array, &r, &nr) || !typed(env, argv[2], napi_float32_array, &s, &ns)) return nullptr;
  if (ns % 8 != 0 || nr != ns * 3) { napi_throw_range_error(env, nullptr, "rotation needs 24 and shift 8 floats per transform"); return nullptr; }
  flx_status rc = flx_group_transforms_upload(grp, (const float *)r, (const float *)s, (uint32_t)(ns / 8));
  if (rc != FLX_OK) return gfail(env, grp, "flx_group_transforms_upload", rc);
  return nullptr;
}
static napi_value GroupUploadLights(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return nullptr;
  flx_group *grp = get_group(env, argv[0]);
  if (!grp) return nullptr;
  void *l; size_t nl;
  if (!typed(env, argv[1], napi_float32_array, &l, &nl)) return nullptr;
  if (nl % 6 != 0) { napi_throw_range_error(env, nullptr, "lights needs 6 floats per light"); return nullptr; }
  flx_status rc = flx_group_lights_upload(grp, (const float *)l, (uint32_t)(nl / 6));
  if (rc != FLX_OK) return gfail(env, grp, "flx_group_lights_upload", rc);
  return nullptr;
}
static napi_value GroupUploadAtlas(napi_env env, napi_callback_info info) {
  napi_value argv[5];
  if (!get_args(env, info, 5, argv)) return nullptr;
  flx_group *grp = get_group(env, argv[0]);
  if (!grp) return nullptr;
  int32_t which; uint32_t w, h;
  NAPI_OK(env, napi_get_value_int32(env, argv[1], &which));
  void *px; size_t n;
  if (!typed(env, argv[2], napi_uint8_array, &px, &n)) return nullptr;
  NAPI_OK(env, napi_get_value_uint32(env, argv[3], &w));
  NAPI_OK(env, napi_get_value_uint32(env, argv[4], &h));
  if (px && n != (size_t)w * h * 4) { napi_throw_range_error(env, nullptr, "atlas needs width*height*4 bytes"); return nullptr; }
  flx_status rc = flx_group_atlas_upload(grp, which, (const uint8_t *)px, w, h);
  if (rc != FLX_OK) return gfail(env, grp, "flx_group_atlas_upload", rc);
  return nullptr;
}
static napi_value GroupUploadTextures(napi_env env, napi_callback_info info) {
  napi_value argv[5];
  if (!get_args(env, info, 5, argv)) return nullptr;
  flx_group *grp = get_group(env, argv[0]);
  if (!grp) return nullptr;
  int32_t which; uint32_t cw, ch; std::vector<flx_image> images;
  if (!textures_args(env, argv + 1, &which, images, &cw, &ch)) return nullptr;
  flx_status rc = flx_group_textures_upload(grp, which, images.data(), (uint32_t)images.size(), cw, ch);
  if (rc != FLX_OK) return gfail(env, grp, "flx_group_textures_upload", rc);
  return nullptr;
}
static napi_value GroupUpdateTexture(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  flx_group *grp = get_group(env, argv[0]);
  if (!grp) return nullptr;
  int32_t which; uint32_t index; flx_image image;
  if (!texture_args(env, argv + 1, &which, &index, &image)) return nullptr;
  flx_status rc = flx_group_texture_update(grp, which, index, &image);
  if (rc != FLX_OK) return gfail(env, grp, "flx_group_texture_update", rc);
  return nullptr;
}
/* groupRender(handle, [params, ...], tileRows, out Float32Array(frames*height*width*4), wantCounters) -> { frameMs, counters? } */
static napi_value GroupRender(napi_env env, napi_callback_info info) {
  napi_value argv[5];
  if (!get_args(env, info, 5, argv)) return nullptr;
  flx_group *grp = get_group(env, argv[0]);
  if (!grp) return nullptr;
  uint32_t count = 0;
  bool isArray = false;
  napi_is_array(env, argv[1], &isArray);
  if (!isArray || napi_get_array_length(env, argv[1], &count) != napi_ok || count < 1 || count > FLX_MAX_BATCH_FRAMES) {
    napi_throw_range_error(env, nullptr, "groupRender: an array of 1 .. 32 frame parameter objects");
    return nullptr;
  }
  flx_frame_params p[FLX_MAX_BATCH_FRAMES];
  for (uint32_t i = 0; i < count; i++) {
    napi_value e;
    NAPI_OK(env, napi_get_element(env, argv[1], i, &e));
    if (!read_params(env, e, &p[i])) return nullptr;
  }
  uint32_t tileRows = 8;
  NAPI_OK(env, napi_get_value_uint32(env, argv[2], &tileRows));
  void *out; size_t n;
  if (!typed(env, argv[3], napi_float32_array, &out, &n)) return nullptr;
  if (!out || n != (size_t)count * p[0].height * p[0].width * 4) { napi_throw_range_error(env, nullptr, "out needs frames*height*width*4 floats"); return nullptr; }
  bool want = false;
  napi_get_value_bool(env, argv[4], &want);
  flx_counters c;
  flx_status rc = flx_group_render(grp, p, count, tileRows, (float *)out, want ? &c : nullptr);
  if (rc != FLX_OK) return gfail(env, grp, "flx_group_render", rc);
  float frame_ms = 0.f, trace_ms = 0.f;
  flx_last_frame_ms(flx_group_context(grp, 0), &frame_ms, &trace_ms);
  napi_value res, v;
  NAPI_OK(env, napi_create_object(env, &res));
  napi_create_double(env, frame_ms, &v); napi_set_named_property(env, res, "frameMs", v);
  napi_create_double(env, trace_ms, &v); napi_set_named_property(env, res, "traceMs", v);
  if (want) {
    napi_value co;
    napi_create_object(env, &co);
    const char *names[8] = { "primaryVisits", "closestVisits", "shadowVisits", "closestWalks", "shadowWalks", "shades", "primaryHits", "atlasTexels" };
    const uint64_t vals[8] = { c.primary_visits, c.closest_visits, c.shadow_visits, c.closest_walks, c.shadow_walks, c.shades, c.primary_hits, c.atlas_texels };
    for (int i = 0; i < 8; i++) { napi_create_double(env, (double)vals[i], &v); napi_set_named_property(env, co, names[i], v); }
    napi_set_named_property(env, res, "counters", co);
  }
  return res;
}

/* groupRenderRgba8(handle, params, tileRows, out Uint8ClampedArray(height*width*4)) -> { frameMs }: one frame as the canvas' RGBA8, the strips quantised on
 * their GPUs before the exchange (flx_group_render_rgba8: a quarter of the bytes gathered and copied out) */
static napi_value GroupRenderRgba8(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  flx_group *grp = get_group(env, argv[0]);
  if (!grp) return nullptr;
  flx_frame_params p;
  if (!read_params(env, argv[1], &p)) return nullptr;
  uint32_t tileRows = 8;
  NAPI_OK(env, napi_get_value_uint32(env, argv[2], &tileRows));
  void *out; size_t n;
  if (!typed(env, argv[3], napi_uint8_array, &out, &n)) return nullptr;
  if (!out || n != (size_t)p.height * p.width * 4) { napi_throw_range_error(env, nullptr, "out needs height*width*4 bytes"); return nullptr; }
  flx_status rc = flx_group_render_rgba8(grp, &p, 1, tileRows, (uint8_t *)out, nullptr);
  if (rc != FLX_OK) return gfail(env, grp, "flx_group_render_rgba8", rc);
  float frame_ms = 0.f, trace_ms = 0.f;
  flx_last_frame_ms(flx_group_context(grp, 0), &frame_ms, &trace_ms);
  napi_value res, v;
  NAPI_OK(env, napi_create_object(env, &res));
  napi_create_double(env, frame_ms, &v); napi_set_named_property(env, res, "frameMs", v);
  return res;
}

/* ---- the group's frame loop: groupFrameBegin(handle, params, tileRows, rgba8) / groupFrameEnd(handle, rgba8) -> { pixels, gpuMs } ------
 * flx_group_frame_begin / _end: every GPU's frame server resolves its strips straight into ONE image in pinned host memory; `pixels` is a Float32Array
 * (or, rgba8, a Uint8ClampedArray of the canvas' bytes: the servers quantise as they resolve) over that image (no copy), the frame's until the NEXT groupFrameBegin — which may be the frame that re-uses the image — detaches it (and
 * groupSetFrameLanes, destroyGroup). */
static napi_value GroupFrameBegin(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  GroupBox *box = get_group_box(env, argv[0]);
  if (!box) return nullptr;
  flx_frame_params p;
  if (!read_params(env, argv[1], &p)) return nullptr;
  uint32_t tileRows = 8;
  NAPI_OK(env, napi_get_value_uint32(env, argv[2], &tileRows));
  bool rgba8 = false;
  napi_get_value_bool(env, argv[3], &rgba8);
  detach_group_views(env, box);
  flx_status rc = flx_group_frame_begin(box->g, &p, tileRows, rgba8 ? FLX_FRAME_RGBA8 : FLX_FRAME_FLOAT);
  if (rc != FLX_OK) return gfail(env, box->g, "flx_group_frame_begin", rc);
  return nullptr;
}
static napi_value GroupFrameEnd(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return nullptr;
  GroupBox *box = get_group_box(env, argv[0]);
  if (!box) return nullptr;
  bool rgba8 = false;
  napi_get_value_bool(env, argv[1], &rgba8);
  const void *pixels = nullptr; size_t bytes = 0; float ms = 0.f;
  flx_status rc = flx_group_frame_end(box->g, &pixels, &bytes, &ms);
  if (rc != FLX_OK) return gfail(env, box->g, "flx_group_frame_end", rc);
  return frame_result(env, box->views, pixels, bytes, ms, rgba8);
}
/* ---- frameEndAsync(handle, rgba8) / groupFrameEndAsync(handle, rgba8) -> Promise<{ pixels, gpuMs }> ------------------------------------------
 * The reference's loop hands the frame to the browser and returns to the event loop (modules/pathtracerWGL2.js:300-302); flx_frame_end WAITS for the GPU.
 * Here the wait happens on a libuv worker thread (napi_async_work) and the promise settles on the main thread, which meanwhile runs timers, I/O and the
 * application's own code.  While the promise is pending the context (group) belongs to the worker: every other call on it throws. */
struct EndWork {
  napi_async_work work = nullptr;
  napi_deferred deferred = nullptr;
  napi_ref handle = nullptr;               /* keeps the context / group handle alive */
  CtxBox *box = nullptr;
  GroupBox *gbox = nullptr;
  bool rgba8 = false;
  flx_status rc = FLX_OK;
  const void *pixels = nullptr; size_t bytes = 0; float ms = 0.f;
  std::string err;
};
static void end_execute(napi_env, void *data) {      /* worker thread: no N-API calls here */
  EndWork *w = static_cast<EndWork *>(data);
  if (w->box) {
    w->rc = flx_frame_end(w->box->ctx, &w->pixels, &w->bytes, &w->ms);
    if (w->rc != FLX_OK) w->err = std::string("flx_frame_end failed (") + std::to_string(w->rc) + "): " + flx_last_error(w->box->ctx);
  } else {
    w->rc = flx_group_frame_end(w->gbox->g, &w->pixels, &w->bytes, &w->ms);
    if (w->rc != FLX_OK) w->err = std::string("flx_group_frame_end failed (") + std::to_string(w->rc) + "): " + flx_group_last_error(w->gbox->g);
  }
}
static void end_complete(napi_env env, napi_status status, void *data) {      /* main thread */
  EndWork *w = static_cast<EndWork *>(data);
  if (w->box) w->box->busy = false; else w->gbox->busy = false;
  napi_value out = nullptr;
  if (status == napi_ok && w->rc == FLX_OK) {
    if (w->box) detach_views(env, w->box, [&](const void *q) { return q != w->pixels; });
    out = frame_result(env, w->box ? w->box->views : w->gbox->views, w->pixels, w->bytes, w->ms, w->rgba8);
  }
  if (out) napi_resolve_deferred(env, w->deferred, out);
  else {
    bool pending = false;
    napi_is_exception_pending(env, &pending);
    napi_value ex = nullptr;
    if (pending) napi_get_and_clear_last_exception(env, &ex);
    if (!ex) {
      napi_value msg;
      napi_create_string_utf8(env, w->err.empty() ? "frameEndAsync: cancelled" : w->err.c_str(), NAPI_AUTO_LENGTH, &msg);
      napi_create_error(env, nullptr, msg, &ex);
    }
    napi_reject_deferred(env, w->deferred, ex);
  }
  napi_delete_reference(env, w->handle);
  napi_delete_async_work(env, w->work);
  delete w;
}
static napi_value end_async(napi_env env, napi_callback_info info, bool group) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return nullptr;
  CtxBox *box = group ? nullptr : get_box(env, argv[0]);
  GroupBox *gbox = group ? get_group_box(env, argv[0]) : nullptr;
  if (!box && !gbox) return nullptr;
  EndWork *w = new EndWork();
  w->box = box; w->gbox = gbox;
  napi_get_value_bool(env, argv[1], &w->rgba8);
  napi_value promise, name;
  if (napi_create_promise(env, &w->deferred, &promise) != napi_ok || napi_create_reference(env, argv[0], 1, &w->handle) != napi_ok ||
      napi_create_string_utf8(env, group ? "flx_group_frame_end" : "flx_frame_end", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, nullptr, name, end_execute, end_complete, w, &w->work) != napi_ok) {
    delete w;
    napi_throw_error(env, nullptr, "frameEndAsync: could not create the work item");
    return nullptr;
  }
  if (box) box->busy = true; else gbox->busy = true;
  if (napi_queue_async_work(env, w->work) != napi_ok) {
    if (box) box->busy = false; else gbox->busy = false;
    napi_delete_reference(env, w->handle); napi_delete_async_work(env, w->work); delete w;
    napi_throw_error(env, nullptr, "frameEndAsync: could not queue the work item");
    return nullptr;
  }
  return promise;
}
static napi_value FrameEndAsync(napi_env env, napi_callback_info info) { return end_async(env, info, false); }
static napi_value GroupFrameEndAsync(napi_env env, napi_callback_info info) { return end_async(env, info, true); }
static napi_value GroupFramesInFlight(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  if (!get_args(env, info, 1, argv)) return nullptr;
  flx_group *g = get_group(env, argv[0]);
  if (!g) return nullptr;
  napi_value v;
  napi_create_int32(env, flx_group_frames_in_flight(g), &v);
  return v;
}
static napi_value GroupSetFrameLanes(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return nullptr;
  GroupBox *box = get_group_box(env, argv[0]);
  if (!box) return nullptr;
  int32_t lanes = 3;
  NAPI_OK(env, napi_get_value_int32(env, argv[1], &lanes));
  flx_status rc = flx_group_set_frame_lanes(box->g, lanes);
  if (rc != FLX_OK) return gfail(env, box->g, "flx_group_set_frame_lanes", rc);
  detach_group_views(env, box);            /* (the images are made again for the new depth) */
  return nullptr;
}
/* groupTemporalReset(handle): every context of the group forgets the history of its strips (flx_group_temporal_reset) */
static napi_value GroupTemporalReset(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  if (!get_args(env, info, 1, argv)) return nullptr;
  flx_group *g = get_group(env, argv[0]);
  if (!g) return nullptr;
  flx_status rc = flx_group_temporal_reset(g);
  if (rc != FLX_OK) return gfail(env, g, "flx_group_temporal_reset", rc);
  return nullptr;
}

static napi_value Version(napi_env env, napi_callback_info) {
  napi_value v;
  napi_create_string_utf8(env, flx_version(), NAPI_AUTO_LENGTH, &v);
  return v;
}

static napi_value Init(napi_env env, napi_value exports) {
  const struct { const char *name; napi_callback fn; } fns[] = {
    { "createContext", CreateContext }, { "destroyContext", DestroyContext }, { "uploadScene", UploadScene }, { "updateSceneRows", UpdateSceneRows }, { "castRays", CastRays }, { "traceRays", TraceRays }, { "traceRaysOrdered", TraceRaysOrdered }, { "traceRaysGather", TraceRaysGather }, { "traceProbes", TraceProbes }, { "probeIrradiance", ProbeIrradiance }, { "bakeVolume", BakeVolume }, { "volumeRows", VolumeRows }, { "volumeMaps", VolumeMaps }, { "updateVolume", UpdateVolume }, { "relocateVolume", RelocateVolume }, { "volumeOffsets", VolumeOffsets }, { "frameIrradiance", FrameIrradiance }, { "raysIrradiance", RaysIrradiance }, { "rayImage", RayImage }, { "rayImageTemporal", RayImageTemporal }, { "rayHistoryReset", RayHistoryReset }, { "cameraRays", CameraRays }, { "cameraImage", CameraImage }, { "cameraImageTemporal", CameraImageTemporal }, { "rayPlanesGather", RayPlanesGather }, { "rayImageGather", RayImageGather }, { "rayImageTemporalGather", RayImageTemporalGather }, { "cameraImageGather", CameraImageGather }, { "cameraImageTemporalGather", CameraImageTemporalGather },{ "surfaceRays", SurfaceRays }, { "frameSurface", FrameSurface }, { "groupUpdateSceneRows", GroupUpdateSceneRows },
    { "uploadTransforms", UploadTransforms }, { "uploadLights", UploadLights }, { "uploadAtlas", UploadAtlas }, { "uploadTextures", UploadTextures }, { "updateTexture", UpdateTexture },
    { "tileRowCount", TileRowCount }, { "render", Render }, { "rasterRender", RasterRender }, { "renderBatch", RenderBatch }, { "temporalReset", TemporalReset }, { "deviceInfo", DeviceInfo }, { "version", Version },
    { "meshImport", MeshImport }, { "meshCounts", MeshCounts }, { "meshSetTransform", MeshSetTransform }, { "meshMove", MeshMove },
    { "meshScale", MeshScale }, { "meshSetMaterial", MeshSetMaterial }, { "meshFlatten", MeshFlatten }, { "meshBounding", MeshBounding }, { "packTransforms", PackTransforms },
    { "present", Present }, { "fxaa", Fxaa }, { "taa", Taa }, { "taaReset", TaaReset },
    { "frameBegin", FrameBegin }, { "frameEnd", FrameEnd }, { "frameEndAsync", FrameEndAsync }, { "groupFrameEndAsync", GroupFrameEndAsync }, { "framesInFlight", FramesInFlight },
    { "createGroup", CreateGroup }, { "destroyGroup", DestroyGroup }, { "groupInfo", GroupInfo }, { "groupUploadScene", GroupUploadScene },
    { "groupUploadTransforms", GroupUploadTransforms }, { "groupUploadLights", GroupUploadLights }, { "groupUploadAtlas", GroupUploadAtlas }, { "groupUploadTextures", GroupUploadTextures }, { "groupUpdateTexture", GroupUpdateTexture },
    { "groupRender", GroupRender }, { "groupRenderRgba8", GroupRenderRgba8 }, { "groupFrameBegin", GroupFrameBegin }, { "groupFrameEnd", GroupFrameEnd }, { "groupFramesInFlight", GroupFramesInFlight },
    { "groupSetFrameLanes", GroupSetFrameLanes }, { "groupTemporalReset", GroupTemporalReset },
  };
  for (const auto &f : fns) {
    napi_value fn;
    if (napi_create_function(env, f.name, NAPI_AUTO_LENGTH, f.fn, nullptr, &fn) != napi_ok) return nullptr;
    napi_set_named_property(env, exports, f.name, fn);
  }
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
