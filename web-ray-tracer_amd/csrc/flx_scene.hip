/* flx_scene.hip — what changes the resident scene: the uploads of the C ABI (include/flexlight_hip.h) and the updates of an uploaded scene's rows
 * (include/flexlight_hip_debug.h), from host memory and from device memory, over one path each.  The order of the steps is the point: what waits for the frame
 * loop's second lane, what is enqueued behind the frames in flight, what a refused call may have touched (nothing).  Its kernels: flx_refit.hip, flx_derive.hip. */
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "flx_context.h"
#include "flx_texture_args.h"

using namespace flx;

static flx_status fail(flx_context *ctx, flx_status code, const char *msg) { return flx_fail(ctx, code, msg); }

/* Scene arrays live in device buffers that persist across uploads: an upload of the same or a smaller size reuses the
 * buffer (the reference refills its transform UBO and light texture every frame, pathtracerWGL2.js:258-262, 361-365 — a
 * per-frame hipFree + hipMalloc would put two device synchronisations into every frame).  Small arrays (transforms, lights:
 * a few hundred bytes per frame) go through a ring of pinned staging slots and are copied in stream order, without waiting
 * for the frames already enqueued; large ones are copied from the caller's memory and waited for.  Either way the caller's
 * buffer is not retained. */
constexpr size_t STAGE_SLOT_BYTES = 64 * 1024;
constexpr int STAGE_SLOTS = 8;

/* The static scene arrays (geometry, attributes, ids, the threaded and forward-ordered copies, atlases) are SHARED with the
 * frame loop's second lane (mirror_scene): its frames read them on another stream.  An upload of one of them therefore first
 * waits for the twin's frames in flight (they must not see the array change under them, nor new metadata over old contents)
 * and ends with the copy complete, so that the twin's next frame — enqueued on its own stream, which does not order itself after
 * the primary's — finds the new contents.  Scene and atlas uploads are per scene, not per frame; what changes per frame
 * (lights, transforms) lives in per-lane buffers and stays asynchronous. */
static flx_status shared_upload_begin(flx_context *ctx) {
  if (ctx->twin) FLX_HIP(ctx, hipStreamSynchronize(ctx->twin->stream));
  return FLX_OK;
}
static flx_status shared_upload_end(flx_context *ctx) {
  if (ctx->twin) FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return FLX_OK;
}

/* What every upload of an array does before its copy: the frame server ends, the versions count, and dst has room for `bytes` — 0 bytes is "none", released (the
 * kernels test the pointer).  A buffer that must grow waits for its readers on both lanes first. */
template <typename T>
static flx_status make_room(flx_context *ctx, DeviceBuffer<T> &dst, size_t bytes) {
  { flx_status ss = flx_server_stop(ctx); if (ss) return ss; }      /* (a running frame server reads the scene) */
  ctx->structure_version++;              /* (the uploads a launch for a scene that moves goes on over do not come through here: flx_transforms_upload) */
  ctx->scene_version++;                  /* (the frame server's launch does not go on over a changed scene) */
  if (bytes == 0) {
    if (dst && ctx->twin) FLX_HIP(ctx, hipStreamSynchronize(ctx->twin->stream));
    return dst.release(ctx);
  }
  const size_t count = (bytes + sizeof(T) - 1) / sizeof(T);
  if (dst.fits(count)) return FLX_OK;
  if (dst) {
    FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->twin) FLX_HIP(ctx, hipStreamSynchronize(ctx->twin->stream));      /* (the frame loop's second lane may be reading a shared array) */
  }
  return dst.ensure(ctx, count);
}

template <typename T>
static flx_status upload(flx_context *ctx, DeviceBuffer<T> &dst, const void *src, size_t bytes) {
  flx_status s = make_room(ctx, dst, bytes);
  if (s || bytes == 0) return s;
  if (bytes <= STAGE_SLOT_BYTES) {
    if (!ctx->stage) {
      if ((s = ctx->stage.ensure(ctx, STAGE_SLOT_BYTES * STAGE_SLOTS, hipHostMallocDefault))) return s;
      for (auto &ev : ctx->stage_done) FLX_HIP(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    const int k = ctx->stage_next;
    ctx->stage_next = (k + 1) % STAGE_SLOTS;
    if (ctx->stage_used[k]) FLX_HIP(ctx, hipEventSynchronize(ctx->stage_done[k]));      /* the copy that last read this slot (eight uploads ago) */
    memcpy(ctx->stage + (size_t)k * STAGE_SLOT_BYTES, src, bytes);
    FLX_HIP(ctx, hipMemcpyAsync(dst, ctx->stage + (size_t)k * STAGE_SLOT_BYTES, bytes, hipMemcpyHostToDevice, ctx->stream));
    FLX_HIP(ctx, hipEventRecord(ctx->stage_done[k], ctx->stream));
    ctx->stage_used[k] = true;
    return FLX_OK;
  }
  if (ctx->twin) FLX_HIP(ctx, hipStreamSynchronize(ctx->twin->stream));      /* a scene array the second lane may still be reading */
  FLX_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));          /* the caller's buffer is not retained */
  return FLX_OK;
}

/* upload() for an array that is in device memory already (d_src == nullptr: room only, a kernel fills it): a copy on the device in stream order, and no wait
 * behind it: flx_scene_upload_device waits once, at its end. */
template <typename T>
static flx_status upload_from_device(flx_context *ctx, DeviceBuffer<T> &dst, const void *d_src, size_t bytes) {
  flx_status s = make_room(ctx, dst, bytes);
  if (!s && bytes && d_src) FLX_HIP(ctx, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return s;
}

/* update_stream — where the calls that take device memory check it, beside the frames in flight on the context's stream — and the events of these paths
 * (flx_context.h): all made here, at the first call that needs one. */
static flx_status ensure_side_stream(flx_context *ctx) {
  if (!ctx->update_stream) FLX_HIP(ctx, hipStreamCreateWithFlags(&ctx->update_stream, hipStreamNonBlocking));
  for (hipEvent_t *ev : { &ctx->update_done, &ctx->update_checked, &ctx->update_produced, &ctx->geometry_uploaded })
    if (!*ev) FLX_HIP(ctx, hipEventCreateWithFlags(ev, hipEventDisableTiming));
  return FLX_OK;
}
/* a check on update_stream: behind what the caller's stream has produced (nullptr: the arrays are complete) .. */
static flx_status check_on_side_stream(flx_context *ctx, void *producer_stream) {
  flx_status s = ensure_side_stream(ctx);
  if (s || !producer_stream) return s;
  FLX_HIP(ctx, hipEventRecord(ctx->update_produced, (hipStream_t)producer_stream));
  FLX_HIP(ctx, hipStreamWaitEvent(ctx->update_stream, ctx->update_produced, 0));
  return FLX_OK;
}
/* .. and the host waits for that stream alone: the frames in flight on ctx->stream go on */
static flx_status await_check(flx_context *ctx) {
  FLX_HIP(ctx, hipEventRecord(ctx->update_checked, ctx->update_stream));
  FLX_HIP(ctx, hipEventSynchronize(ctx->update_checked));
  return FLX_OK;
}

/* Threaded, hot-first copy of the skip list (DeviceScene::walk).  The reference's array is the DFS
 * pre-order of the AABB tree with a skip count per node (scene.js:224-282); a walk only ever moves to
 * "the next entry" or "the next entry after the subtree".  Writing those two successors into every
 * entry makes the storage order free, so the shallow levels — which every ray crosses — go to the
 * front where the walk kernel keeps them in LDS.  Entry contents, the sequence of entries a given
 * ray visits and therefore every result are unchanged. */
#ifndef FLX_AB_HOT_ORDER
#define FLX_AB_HOT_ORDER 0
#endif
constexpr uint32_t HOT_MAX = 4096;               /* upper bound of entries worth ordering by depth */
static void build_threaded(const float *geometry, uint32_t n, std::vector<float> &out, uint32_t &n_out, uint32_t &n_hot, uint32_t &root) {
  /* live entries: everything a walk can reach = all entries before the first terminator that is reached;
   * keep every non-terminator entry plus ONE shared terminator. */
  std::vector<uint32_t> depth(n, 0);
  {
    std::vector<uint32_t> stack;                 /* last index of the enclosing subtrees */
    for (uint32_t i = 0; i < n; i++) {
      while (!stack.empty() && i > stack.back()) stack.pop_back();
      depth[i] = (uint32_t)stack.size();
      const float *e = geometry + (size_t)i * 12;
      if (e[10] == 1.0f) stack.push_back(i + (uint32_t)e[6]);
    }
  }
  std::vector<uint32_t> order;                   /* original indices of non-terminator entries, hot first */
  order.reserve(n);
  for (uint32_t i = 0; i < n; i++) if (geometry[(size_t)i * 12 + 10] != 0.0f) order.push_back(i);
  /* shallowest HOT_MAX entries first (stable: by depth, then original index), the rest in original order */
  std::vector<uint32_t> byDepth(order);
  std::stable_sort(byDepth.begin(), byDepth.end(), [&](uint32_t a, uint32_t b) { return depth[a] < depth[b]; });
#if FLX_AB_HOT_ORDER      /* A/B builds only: the hot-first order from a file of original indices (tools: the oracle's visit histogram), to bound what a better choice of the LDS top can bring */
  if (const char *f = getenv("FLX_HOT_ORDER")) {
    if (FILE *fh = fopen(f, "rb")) {
      std::vector<uint32_t> given(byDepth.size());
      const size_t got = fread(given.data(), 4, given.size(), fh);
      fclose(fh);
      if (got == given.size()) byDepth = given;
    }
  }
#endif
  const uint32_t hot = (uint32_t)std::min<size_t>(HOT_MAX, byDepth.size());
  std::vector<char> isHot(n, 0);
  for (uint32_t k = 0; k < hot; k++) isHot[byDepth[k]] = 1;
  std::vector<uint32_t> newIndex(n, WALK_END);
  uint32_t next = 0;
  const uint32_t terminator = next++;            /* threaded index 0: the shared terminator (every full walk ends on it) */
  for (uint32_t k = 0; k < hot; k++) newIndex[byDepth[k]] = next++;
  for (uint32_t i : order) if (!isHot[i]) newIndex[i] = next++;
  n_out = next;
  n_hot = hot + 1;
  out.assign((size_t)n_out * 12, 0.0f);
  auto bits = [](uint32_t u) { float f; memcpy(&f, &u, 4); return f; };
  /* link to original successor j from an entry with transform number `fromT` (flx_device.h: LINK_*) */
  auto succ = [&](uint64_t j, uint32_t fromT) -> uint32_t {
    if (j >= n) return WALK_END;                 /* loop bound reached: no fetch (fragment:184) */
    const float *e = geometry + (size_t)j * 12;
    if (e[10] == 0.0f) return terminator;        /* kind 0; a terminator's transform is never used */
    const uint32_t kind = e[10] == 1.0f ? 1u : 2u;
    return newIndex[j] | kind << LINK_KIND_SHIFT | ((uint32_t)e[9] != fromT ? LINK_XFORM : 0u);
  };
  root = succ(0, 0);                             /* a walk starts with the untransformed ray (cachedTI = 0, fragment:174) */
  for (uint32_t i : order) {
    const float *e = geometry + (size_t)i * 12;
    float *o = out.data() + (size_t)newIndex[i] * 12;
    const uint32_t type = e[10] == 1.0f ? 1u : 2u;
    const uint32_t meta = type | ((uint32_t)e[9] << 2);
    if (type == 1u) {
      for (int k = 0; k < 6; k++) o[k] = e[k];
      o[8] = bits(succ((uint64_t)i + 1, (uint32_t)e[9]));
      o[9] = bits(succ((uint64_t)i + 1 + (uint64_t)e[6], (uint32_t)e[9]));
      o[10] = bits(meta);
      o[11] = bits(i);
    } else {
      /* vertex a, then the two edges b - a and c - a of fragment:124-125 (the same single-precision subtractions the
       * shader does per visit, done once here) */
      for (int k = 0; k < 3; k++) { o[k] = e[k]; o[3 + k] = e[3 + k] - e[k]; o[6 + k] = e[6 + k] - e[k]; }
      o[9] = bits(succ((uint64_t)i + 1, (uint32_t)e[9]));
      o[10] = bits(meta);
      o[11] = bits(i);
    }
  }
  /* terminator entry stays all zero (meta type 0) */
}

/* The lockstep walk's copy (flx_device.h: walkLockPass): the live entries in the reference's own order — every successor of
 * an entry lies further on — in the threaded layout, with plain indices as links and the shared terminator last.  Built for
 * scenes of at most FLX_LOCK_MAX entries whose entries all stand in transform 0, i.e. are tested with the untransformed ray
 * (fragment:174-175). */
static void build_lockstep(const float *geometry, uint32_t n, std::vector<float> &out, uint32_t &n_out, uint32_t &root, uint32_t &boxes) {
  std::vector<uint32_t> order;
  boxes = 0;
  for (uint32_t i = 0; i < n; i++) if (geometry[(size_t)i * 12 + 10] == 1.0f) boxes++;
  for (uint32_t i = 0; i < n; i++) if (geometry[(size_t)i * 12 + 10] != 0.0f) order.push_back(i);
  const uint32_t terminator = (uint32_t)order.size();
  std::vector<uint32_t> newIndex(n, terminator);
  for (uint32_t k = 0; k < terminator; k++) newIndex[order[k]] = k;
  n_out = terminator + 1u;
  out.assign((size_t)n_out * 12, 0.0f);
  auto bits = [](uint32_t u) { float f; memcpy(&f, &u, 4); return f; };
  auto succ = [&](uint64_t j) -> uint32_t { return j >= n ? WALK_END : newIndex[j]; };      /* (a terminator's newIndex is the shared one) */
  root = succ(0);
  for (uint32_t i : order) {
    const float *e = geometry + (size_t)i * 12;
    float *o = out.data() + (size_t)newIndex[i] * 12;
    if (e[10] == 1.0f) {
      for (int k = 0; k < 6; k++) o[k] = e[k];
      o[8] = bits(succ((uint64_t)i + 1));
      o[9] = bits(succ((uint64_t)i + 1 + (uint64_t)e[6]));
      o[10] = bits(1u | ((uint32_t)e[9] << 2));
    } else {
      for (int k = 0; k < 3; k++) { o[k] = e[k]; o[3 + k] = e[3 + k] - e[k]; o[6 + k] = e[6 + k] - e[k]; }      /* as build_threaded */
      o[9] = bits(succ((uint64_t)i + 1));
      o[10] = bits(2u | ((uint32_t)e[9] << 2));
    }
    o[11] = bits(i);
  }
}

/* whether [p, p + bytes) is device memory of this context's device, 16-byte aligned (or to `align`, a power of two) */
static bool rows_on_device(const flx_context *ctx, const void *p, size_t bytes, uintptr_t align = 16) {
  hipPointerAttribute_t at;
  if (((uintptr_t)p & (align - 1u)) || hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  if (at.type != hipMemoryTypeDevice || at.device != ctx->device) return false;
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return (uintptr_t)p - (uintptr_t)base + bytes <= size;
}
bool flx_rows_on_device(const flx_context *ctx, const void *p, size_t bytes) { return rows_on_device(ctx, p, bytes); }      /* (flx_query.hip asks the same of its rays and hits) */
bool flx_words_on_device(const flx_context *ctx, const void *p, size_t bytes) { return rows_on_device(ctx, p, bytes, 4); }      /* (flx_volume_update.hip: a list's indices and states) */

/* What an upload learns about its entry array.  flx_scene_upload fills it from its scan and the two builders, flx_scene_upload_device from the record of
 * k_derive_check (flx_derive.hip); the two derivations stay apart, each is the other's oracle (tests/test_scene_upload_device_gpu.py). */
struct SceneFacts {
  uint32_t max_transform = 0, walk_entries = 0, walk_hot = 0, walk_root = 0, fwd_entries = 0, fwd_root = 0, lock_boxes = 0;
  bool has_nan = false, bounded = true;          /* a triangle has a NaN vertex (no updates then: flx_context.h); the precondition of the walk's fast box test holds */
  bool thick = true;                             /* no box is flat (box_is_thick): the frame kernels' box test may take its single-comparison form */
};

/* A box with room between its two planes on every axis (words 0..2 min, 3..5 max); a NaN corner or min > max has none.  What the scene's walk_thick_boxes asks of every box. */
static bool box_is_thick(const float *e) { return e[0] < e[3] && e[1] < e[4] && e[2] < e[5]; }
extern "C" int flx_debug_boxes_thick(const float *geometry, uint32_t n_entries) {
  if (!geometry) return 0;
  for (uint32_t i = 0; i < n_entries; i++) if (geometry[(size_t)i * 12 + 10] == 1.0f && !box_is_thick(geometry + (size_t)i * 12)) return 0;
  return 1;
}

/* Why an entry array is refused, in the order the host's loop meets the rules within an entry; the values are k_derive_check's rule numbers. */
enum UploadRule { UPLOAD_RULE_TRANSFORM, UPLOAD_RULE_SKIP, UPLOAD_RULE_TYPE };
static const char *const SCENE_UPLOAD_REFUSAL[3] = { "flx_scene_upload: transform number out of range", "flx_scene_upload: AABB skip count leaves the entry array",
                                                     "flx_scene_upload: entry type is not 0, 1 or 2" };

/* what both uploads refuse before an entry is looked at */
static flx_status upload_refused(flx_context *ctx, const void *geometry, const void *attributes, uint32_t n_entries_padded, const void *ids, uint32_t n_ids) {
  if (!ctx) return FLX_ERR_INVALID;
  if (!geometry || !attributes || n_entries_padded == 0) return fail(ctx, FLX_ERR_INVALID, "flx_scene_upload: empty scene");
  if (n_ids && !ids) return fail(ctx, FLX_ERR_INVALID, "flx_scene_upload: ids is NULL");
  if (n_entries_padded > LINK_INDEX) return fail(ctx, FLX_ERR_INVALID, "flx_scene_upload: more than 2^28 - 1 entries");
  return FLX_OK;
}

/* from the first array that changes until adopt_scene the context has no scene */
static void begin_scene(flx_context *ctx) { ctx->have_scene = false; ctx->last_walk_lds = WalkLdsLaunch(); ctx->last_query = QueryLaunch(); ctx->geometry_version++; }
static void adopt_scene(flx_context *ctx, uint32_t n_entries_padded, uint32_t n_ids, const SceneFacts &f) {
  ctx->walk_entries = f.walk_entries; ctx->walk_hot = f.walk_hot; ctx->walk_root = f.walk_root; ctx->walk_fast_boxes = f.bounded ? 1u : 0u;
  ctx->walk_thick_boxes = f.thick ? 1u : 0u;
  ctx->fwd_entries = f.fwd_entries; ctx->fwd_root = f.fwd_root; ctx->lock_boxes = f.lock_boxes;
  ctx->lock_ok = f.max_transform == 0 && f.fwd_entries <= FLX_LOCK_MAX;
  ctx->n_entries = n_entries_padded; ctx->n_ids = n_ids; ctx->max_transform = f.max_transform; ctx->scene_has_nan = f.has_nan;
}

extern "C" flx_status flx_scene_upload(flx_context *ctx, const float *geometry, const float *attributes, uint32_t n_entries_padded,
                                       const int32_t *ids, uint32_t n_ids) {
  if (flx_status refused = upload_refused(ctx, geometry, attributes, n_entries_padded, ids, n_ids)) return refused;
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  ctx->sv_want_ver = false;                 /* (another scene: it has not moved yet) */
  /* Validate the skip list on the host: a skip that leaves the array would make the walk read out of
   * bounds on the GPU (the shader's texelFetch would be robust-access clamped; we refuse instead). */
  SceneFacts facts;
  std::vector<uint32_t> entry_meta((size_t)n_entries_padded * 3);      /* what flx_scene_update holds its rows against */
  for (uint32_t i = 0; i < n_entries_padded; i++) {
    const float *e = geometry + (size_t)i * 12;
    memcpy(&entry_meta[(size_t)i * 3], e + 6, 4); memcpy(&entry_meta[(size_t)i * 3 + 1], e + 9, 8);
    if (e[10] == 2.0f) for (int k = 0; k < 9; k++) if (e[k] != e[k]) facts.has_nan = true;
    if (e[10] != 0.0f) {
      if (!(e[9] >= 0.0f && e[9] < 1048576.0f)) return fail(ctx, FLX_ERR_INVALID, SCENE_UPLOAD_REFUSAL[UPLOAD_RULE_TRANSFORM]);
      if ((uint32_t)e[9] > facts.max_transform) facts.max_transform = (uint32_t)e[9];
    }
    if (e[10] == 1.0f) {
      float skip = e[6];
      if (!(skip >= 0.0f) || (double)i + (double)skip >= (double)n_entries_padded) return fail(ctx, FLX_ERR_INVALID, SCENE_UPLOAD_REFUSAL[UPLOAD_RULE_SKIP]);
      for (int k = 0; k < 6; k++) if (!(std::fabs(e[k]) <= FLX_FAST_BOX_BOUND)) facts.bounded = false;
      if (!box_is_thick(e)) facts.thick = false;
    } else if (e[10] != 0.0f && e[10] != 2.0f) {
      return fail(ctx, FLX_ERR_INVALID, SCENE_UPLOAD_REFUSAL[UPLOAD_RULE_TYPE]);
    }
  }
  flx_status s;
  if ((s = ensure_side_stream(ctx)) || (s = shared_upload_begin(ctx))) return s;
  begin_scene(ctx);
  if ((s = upload(ctx, ctx->d_geometry, geometry, (size_t)n_entries_padded * 48))) return s;
  if ((s = upload(ctx, ctx->d_attributes, attributes, (size_t)n_entries_padded * 112))) return s;
  if ((s = upload(ctx, ctx->d_ids, ids, (size_t)n_ids * 4))) return s;
  /* (a small array is copied in stream order: flx_scene_update_device's check reads the geometry on another stream, flx_scene_splice_device's the ids too) */
  FLX_HIP(ctx, hipEventRecord(ctx->geometry_uploaded, ctx->stream));
  std::vector<float> copy;
  build_threaded(geometry, n_entries_padded, copy, facts.walk_entries, facts.walk_hot, facts.walk_root);
  if ((s = upload(ctx, ctx->d_walk, copy.data(), copy.size() * sizeof(float)))) return s;
  /* the forward-ordered copy: the primary rays' walk steps through it wave by wave, and — small scenes in one object space — the
   * bounce walks of the per-pixel and persistent path kernels do */
  build_lockstep(geometry, n_entries_padded, copy, facts.fwd_entries, facts.fwd_root, facts.lock_boxes);
  if ((s = upload(ctx, ctx->d_fwd, copy.data(), copy.size() * sizeof(float)))) return s;
  adopt_scene(ctx, n_entries_padded, n_ids, facts);
  ctx->h_entry_meta.swap(entry_meta); ctx->entry_meta_stale = false;
  if ((s = shared_upload_end(ctx))) return s;
  ctx->have_scene = true;
  return FLX_OK;
}

/* The tail of every change of the scene that is made in device memory (flx_scene_upload_device, flx_scene_splice_device): d_geometry, d_attributes and d_ids hold
 * the new arrays, or will in stream order; rec is the record k_derive_check made of d_geometry's contents, and the derive workspace stands as that check left it,
 * behind `checked` where it ran on another stream than the context's (nullptr: on the context's).  Room for both derived copies, launch_derive_copies for
 * build_threaded and build_lockstep, the context's scalars, and one wait for the context's stream. */
static flx_status derive_and_adopt(flx_context *ctx, uint32_t n_entries_padded, uint32_t n_ids, const uint32_t *rec, hipEvent_t checked) {
  const uint32_t live = rec[5], meta0 = rec[6];
  SceneFacts facts;
  facts.max_transform = rec[1]; facts.has_nan = rec[2] != 0u; facts.bounded = rec[3] == 0u; facts.lock_boxes = rec[4]; facts.thick = rec[7] == 0u;
  /* both copies hold the live entries and one shared terminator; entry 0 is the shallowest entry with the lowest index: hot, the threaded copy's entry 1 */
  facts.walk_entries = facts.fwd_entries = live + 1u; facts.walk_hot = std::min(live, HOT_MAX) + 1u;
  facts.walk_root = meta0 == 0u ? 0u : 1u | (meta0 & 3u) << LINK_KIND_SHIFT | ((meta0 >> 2) != 0u ? LINK_XFORM : 0u);
  facts.fwd_root = meta0 == 0u ? live : 0u;
  flx_status s;
  if ((s = upload_from_device(ctx, ctx->d_walk, nullptr, (size_t)facts.walk_entries * 48))) return s;
  if ((s = upload_from_device(ctx, ctx->d_fwd, nullptr, (size_t)facts.fwd_entries * 48))) return s;
  if (checked) FLX_HIP(ctx, hipStreamWaitEvent(ctx->stream, checked, 0));      /* the workspace as the check left it */
  launch_derive_copies(ctx->d_geometry, n_entries_padded, live, ctx->d_derive, ctx->d_walk, ctx->d_fwd, ctx->stream);
  FLX_HIP(ctx, hipGetLastError());
  adopt_scene(ctx, n_entries_padded, n_ids, facts);
  ctx->h_entry_meta.clear(); ctx->entry_meta_stale = true;      /* (it stays on the device until a flx_scene_update of host rows asks for it: fetch_entry_meta) */
  FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));          /* the caller's arrays are not retained (and: shared_upload_end) */
  ctx->have_scene = true;
  return FLX_OK;
}

/* flx_scene_upload for arrays in device memory.  What the host's loop over the entries decides, k_derive_check (flx_derive.hip) decides on update_stream, into the
 * derive workspace alone: the host waits for that stream, reads the record of scalars, and a refused array has touched nothing of the context's scene and enqueued
 * nothing on its stream.  From there on this is flx_scene_upload with copies on the device for its copies across the bus and launch_derive_copies for
 * build_threaded and build_lockstep; one wait for the context's stream at the end: the caller's arrays are free (and a second lane finds the scene complete). */
extern "C" flx_status flx_scene_upload_device(flx_context *ctx, const void *d_geometry, const void *d_attributes, uint32_t n_entries_padded, const void *d_ids,
                                              uint32_t n_ids, void *producer_stream) {
  if (flx_status refused = upload_refused(ctx, d_geometry, d_attributes, n_entries_padded, d_ids, n_ids)) return refused;
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  if (!rows_on_device(ctx, d_geometry, (size_t)n_entries_padded * 48) || !rows_on_device(ctx, d_attributes, (size_t)n_entries_padded * 112) ||
      (n_ids && !rows_on_device(ctx, d_ids, (size_t)n_ids * 4)))
    return fail(ctx, FLX_ERR_INVALID, "flx_scene_upload_device: the arrays are not in memory of the context's device, 16-byte aligned");
  ctx->sv_want_ver = false;                 /* (another scene: it has not moved yet) */
  flx_status s;
  /* (nothing in flight uses the workspace: this call and fetch_entry_meta end with a wait) */
  if ((s = ctx->d_derive.ensure(ctx, derive_workspace_words(n_entries_padded))) || (s = ctx->h_derive_record.ensure(ctx, DERIVE_RECORD_WORDS, hipHostMallocDefault))) return s;
  if ((s = check_on_side_stream(ctx, producer_stream))) return s;
  FLX_HIP(ctx, launch_derive_check((const float4 *)d_geometry, n_entries_padded, ctx->d_derive, ctx->update_stream));
  FLX_HIP(ctx, hipMemcpyAsync(ctx->h_derive_record, ctx->d_derive, DERIVE_RECORD_WORDS * 4, hipMemcpyDeviceToHost, ctx->update_stream));
  if ((s = await_check(ctx))) return s;
  const uint32_t *rec = ctx->h_derive_record;
  const uint32_t rule = ~rec[0] & 3u;
  if (rec[0] != 0u) return fail(ctx, FLX_ERR_INVALID, SCENE_UPLOAD_REFUSAL[rule < 3u ? rule : 2u]);
  if ((s = shared_upload_begin(ctx))) return s;
  begin_scene(ctx);
  if ((s = upload_from_device(ctx, ctx->d_geometry, d_geometry, (size_t)n_entries_padded * 48))) return s;
  FLX_HIP(ctx, hipEventRecord(ctx->geometry_uploaded, ctx->stream));      /* (flx_scene_update_device's check reads the array on another stream) */
  if ((s = upload_from_device(ctx, ctx->d_attributes, d_attributes, (size_t)n_entries_padded * 112))) return s;
  if ((s = upload_from_device(ctx, ctx->d_ids, d_ids, (size_t)n_ids * 4))) return s;
  return derive_and_adopt(ctx, n_entries_padded, n_ids, rec, ctx->update_checked);
}

/* Why a splice is refused by what the resident scene holds; the values are k_splice_check's rule numbers (flx_splice.hip). */
static const char *const SCENE_SPLICE_REFUSAL[4] = {
  "flx_scene_splice_device: parent_entry is not a box in front of first_entry whose range holds the replaced rows",
  "flx_scene_splice_device: a box between parent_entry and first_entry reaches first_entry (parent_entry is not the direct parent)",
  "flx_scene_splice_device: a box among the replaced rows reaches beyond them",
  "flx_scene_splice_device: the resident id list is not non-decreasing" };

/* k_derive_check over an array assembled on the context's stream, there, and the host waits for its record */
static flx_status check_assembled(flx_context *ctx, const float4 *geometry, uint32_t n_entries_padded) {
  FLX_HIP(ctx, launch_derive_check(geometry, n_entries_padded, ctx->d_derive, ctx->stream));
  FLX_HIP(ctx, hipMemcpyAsync(ctx->h_derive_record, ctx->d_derive, DERIVE_RECORD_WORDS * 4, hipMemcpyDeviceToHost, ctx->stream));
  FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return FLX_OK;
}

/* A block of the resident scene replaced, inserted or removed in device memory.  Three steps, each behind a verdict:
 *   1. k_splice_check (flx_splice.hip) on update_stream, over the resident geometry and ids, into four words: the host waits for that stream alone — the frames in
 *      flight go on — and knows `end`, the id counts and whether a rule of the splice is broken;
 *   2. on the context's stream, behind the frames in flight (they read the old arrays to their end): the assembly of both arrays and of the ids into FRESH
 *      memory, and flx_scene_upload's validation of the assembled array (launch_derive_check); the host waits for the stream and the verdict;
 *   3. the refit of every box of the assembled array (only now: it follows skip counts), the check once more for what it says of the refitted boxes (the bounded
 *      and the thick flags) and as the base of the derivation; the fresh arrays become the context's, the old ones are freed, and the rest is flx_scene_upload_device's tail.
 * Until step 3 a refusal has touched the workspaces and the fresh arrays alone, which go with it.  The frame server's launch ends before step 2. */
extern "C" flx_status flx_scene_splice_device(flx_context *ctx, uint32_t first_entry, uint32_t n_old, uint32_t parent_entry, const void *d_geometry,
                                              const void *d_attributes, uint32_t n_new, const void *d_ids, uint32_t n_new_ids, void *producer_stream) {
  if (!ctx) return FLX_ERR_INVALID;
  if (!ctx->have_scene) return fail(ctx, FLX_ERR_NO_SCENE, "flx_scene_splice_device before flx_scene_upload");
  if (n_old == 0 && n_new == 0) return fail(ctx, FLX_ERR_INVALID, "flx_scene_splice_device: n_old and n_new are both 0");
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  if ((n_new && (!d_geometry || !d_attributes || !rows_on_device(ctx, d_geometry, (size_t)n_new * 48) || !rows_on_device(ctx, d_attributes, (size_t)n_new * 112))) ||
      (n_new_ids && (!d_ids || !rows_on_device(ctx, d_ids, (size_t)n_new_ids * 4))))
    return fail(ctx, FLX_ERR_INVALID, "flx_scene_splice_device: an array is not in memory of the context's device, 16-byte aligned, or too short");
  static const char *const beyond = "flx_scene_splice_device: the replaced rows leave the scene (first_entry + n_old lies beyond its last entry)";
  if ((uint64_t)first_entry + n_old > ctx->n_entries) return fail(ctx, FLX_ERR_INVALID, beyond);      /* (end <= n_entries: the kernel's lanes may rely on it) */
  if (ctx->scene_has_nan)
    return fail(ctx, FLX_ERR_INVALID, "flx_scene_splice_device: the uploaded scene has a NaN vertex (its boxes cannot be refitted as the flatten makes them)");
  flx_status s;
  if ((s = ctx->d_update_verdict.ensure(ctx, SPLICE_RECORD_WORDS)) || (s = ctx->h_update_verdict.ensure(ctx, SPLICE_RECORD_WORDS, hipHostMallocDefault))) return s;
  if ((s = check_on_side_stream(ctx, producer_stream))) return s;
  FLX_HIP(ctx, hipStreamWaitEvent(ctx->update_stream, ctx->geometry_uploaded, 0));      /* (words 6 and 10 and the ids: written by an upload alone) */
  FLX_HIP(ctx, hipMemsetAsync(ctx->d_update_verdict, 0, SPLICE_RECORD_WORDS * 4, ctx->update_stream));
  launch_splice_check(ctx->d_geometry, ctx->n_entries, ctx->d_ids, ctx->n_ids, first_entry, n_old, parent_entry, ctx->d_update_verdict, ctx->update_stream);
  FLX_HIP(ctx, hipGetLastError());
  FLX_HIP(ctx, hipMemcpyAsync(ctx->h_update_verdict, ctx->d_update_verdict, SPLICE_RECORD_WORDS * 4, hipMemcpyDeviceToHost, ctx->update_stream));
  if ((s = await_check(ctx))) return s;
  const uint32_t verdict = ctx->h_update_verdict[SPLICE_REC_VERDICT], end = ctx->h_update_verdict[SPLICE_REC_END];
  const uint32_t below = ctx->h_update_verdict[SPLICE_REC_IDS_BELOW], above = ctx->h_update_verdict[SPLICE_REC_IDS_ABOVE];
  if ((uint64_t)first_entry + n_old > end) return fail(ctx, FLX_ERR_INVALID, beyond);
  const int64_t end_new = (int64_t)end + (int64_t)n_new - (int64_t)n_old;
  if (end_new <= 0 || end_new > (int64_t)1 << 24)      /* (a skip count beyond 2^24 is no exact float any more) */
    return fail(ctx, FLX_ERR_INVALID, "flx_scene_splice_device: the scene would have no entry, or more than 2^24");
  if (verdict != 0u) return fail(ctx, FLX_ERR_INVALID, SCENE_SPLICE_REFUSAL[~verdict & 3u]);
  /* everything the next steps need is there before anything is enqueued */
  const uint32_t n_padded = ((uint32_t)end_new + 255u) / 256u * 256u, n_ids = below + n_new_ids + above;
  const SpliceShape shape = { first_entry, n_old, n_new, parent_entry, (uint32_t)end_new, n_padded };
  DeviceBuffer<float4> geometry, attributes;
  DeviceBuffer<int32_t> ids;
  if ((s = geometry.ensure(ctx, (size_t)n_padded * 3)) || (s = attributes.ensure(ctx, (size_t)n_padded * 7)) || (n_ids && (s = ids.ensure(ctx, n_ids)))) return s;
  /* (nothing in flight uses the derive workspace: flx_scene_upload_device, this call and fetch_entry_meta end with a wait) */
  if ((s = ctx->d_derive.ensure(ctx, derive_workspace_words(n_padded))) || (s = ctx->h_derive_record.ensure(ctx, DERIVE_RECORD_WORDS, hipHostMallocDefault))) return s;
  if (!ctx->d_refit.fits(refit_workspace_words(n_padded))) {
    FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));      /* (an earlier update's refit may still use it) */
    if ((s = ctx->d_refit.ensure(ctx, refit_workspace_words(n_padded)))) return s;
  }
  if ((s = flx_server_stop(ctx))) return s;      /* (its launch would keep the kernels below waiting; it ends at any change of the scene) */
  FLX_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->update_checked, 0));      /* the caller's rows: update_stream waited for their producer */
  launch_splice_rows(ctx->d_geometry, ctx->d_attributes, (const float4 *)d_geometry, (const float4 *)d_attributes, shape, geometry, attributes, ctx->stream);
  launch_splice_ids(ctx->d_ids, ctx->n_ids, (const int32_t *)d_ids, n_new_ids, below, above, first_entry, (int32_t)n_new - (int32_t)n_old, ids, ctx->stream);
  FLX_HIP(ctx, hipGetLastError());
  const uint32_t *rec = ctx->h_derive_record;
  if ((s = check_assembled(ctx, geometry, n_padded))) return s;
  if (rec[0] != 0u) return fail(ctx, FLX_ERR_INVALID, SCENE_UPLOAD_REFUSAL[std::min(~rec[0] & 3u, 2u)]);
  launch_refit(geometry, n_padded, ctx->d_refit, ctx->stream);      /* (every skip count keeps inside the array: checked) */
  if ((s = check_assembled(ctx, geometry, n_padded))) return s;
  /* the caller's arrays are free from here; the fresh ones become the scene's, as an upload's copies would have filled them */
  ctx->sv_want_ver = false;                 /* (another scene: it has not moved yet) */
  if ((s = shared_upload_begin(ctx))) return s;      /* (the second lane's frames in flight read the old arrays) */
  begin_scene(ctx);
  ctx->d_geometry = std::move(geometry); ctx->d_attributes = std::move(attributes);
  if (n_ids) ctx->d_ids = std::move(ids);
  else if ((s = ctx->d_ids.release(ctx))) return s;
  FLX_HIP(ctx, hipEventRecord(ctx->geometry_uploaded, ctx->stream));
  return derive_and_adopt(ctx, n_padded, n_ids, rec, nullptr);
}

/* h_entry_meta after flx_scene_upload_device, which leaves it on the device: words 6, 9 and 10 of every entry, compacted by a kernel and copied back, at the first
 * update of host rows (rows in device memory are held against d_geometry itself).  On update_stream, behind the upload's copy of the geometry: the frames in flight
 * on the context's stream go on. */
static flx_status fetch_entry_meta(flx_context *ctx) {
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  flx_status s;
  if ((s = ctx->d_derive.ensure(ctx, std::max(derive_workspace_words(ctx->n_entries), (size_t)ctx->n_entries * 3))) || (s = ensure_side_stream(ctx))) return s;
  FLX_HIP(ctx, hipStreamWaitEvent(ctx->update_stream, ctx->geometry_uploaded, 0));
  launch_entry_meta(ctx->d_geometry, ctx->n_entries, ctx->d_derive, ctx->update_stream);
  FLX_HIP(ctx, hipGetLastError());
  ctx->h_entry_meta.resize((size_t)ctx->n_entries * 3);
  FLX_HIP(ctx, hipMemcpyAsync(ctx->h_entry_meta.data(), ctx->d_derive, (size_t)ctx->n_entries * 12, hipMemcpyDeviceToHost, ctx->update_stream));
  FLX_HIP(ctx, hipStreamSynchronize(ctx->update_stream));
  ctx->entry_meta_stale = false;
  return FLX_OK;
}

/* Why a row is refused, in the order the host's loop meets the rules within a row; the values are k_rows_check_stage's rule numbers (flx_refit.hip). */
enum UpdateRule { UPDATE_RULE_KIND, UPDATE_RULE_TRANSFORM, UPDATE_RULE_SKIP, UPDATE_RULE_FINITE };
static const char *const SCENE_UPDATE_REFUSAL[4] = { "flx_scene_update: a row changes its kind (word 10)", "flx_scene_update: a row changes its transform number (word 9)",
                                                     "flx_scene_update: a box row changes its skip count (word 6)", "flx_scene_update: a vertex is not finite" };

/* what both updates refuse before a row is looked at (an update of no rows is done once it is known to lie in the array: the callers return FLX_OK) */
static flx_status update_refused(flx_context *ctx, uint32_t first_entry, uint32_t n_entries, const void *geometry) {
  if (!ctx) return FLX_ERR_INVALID;
  if (!ctx->have_scene) return fail(ctx, FLX_ERR_NO_SCENE, "flx_scene_update before flx_scene_upload");
  if ((uint64_t)first_entry + n_entries > ctx->n_entries) return fail(ctx, FLX_ERR_INVALID, "flx_scene_update: the rows leave the entry array");
  if (n_entries == 0) return FLX_OK;
  if (!geometry) return fail(ctx, FLX_ERR_INVALID, "flx_scene_update: geometry is NULL");
  if (ctx->scene_has_nan) return fail(ctx, FLX_ERR_INVALID, "flx_scene_update: the uploaded scene has a NaN vertex (its boxes cannot be refitted as the flatten makes them)");
  return FLX_OK;
}

/* Everything an update needs is there before anything is enqueued: a failed allocation leaves the scene as it was.  Rows from host memory need pinned_floats of
 * h_update; rows in device memory (pinned_floats 0) the verdict pair and, with device_attributes, the stage of their attribute rows. */
static flx_status ensure_update_buffers(flx_context *ctx, uint32_t n_entries, size_t pinned_floats, bool device_attributes) {
  flx_status s;
  if ((s = ensure_side_stream(ctx))) return s;
  if (ctx->update_pending) { FLX_HIP(ctx, hipEventSynchronize(ctx->update_done)); ctx->update_pending = false; }      /* (the last update's copies and scatter read h_update and the stage) */
  if (pinned_floats) s = ctx->h_update.ensure(ctx, pinned_floats, hipHostMallocDefault);
  else if (!(s = ctx->d_update_verdict.ensure(ctx, 4))) s = ctx->h_update_verdict.ensure(ctx, 4, hipHostMallocDefault);
  if (s) return s;
  const size_t rows = (size_t)n_entries * 3, attributes = device_attributes ? (size_t)n_entries * 7 : 0, refit = refit_workspace_words(ctx->n_entries);
  if (ctx->d_update_rows.fits(rows) && (!attributes || ctx->d_update_attributes.fits(attributes)) && ctx->d_refit.fits(refit)) return FLX_OK;
  FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));      /* (an earlier update's kernels and copies may still read what is freed here) */
  if ((s = ctx->d_update_rows.ensure(ctx, rows)) || (attributes && (s = ctx->d_update_attributes.ensure(ctx, attributes)))) return s;
  return ctx->d_refit.ensure(ctx, refit);
}

/* Rows that passed enter the scene: scattered into d_geometry, every box refitted and both derived copies brought up to date ON THE DEVICE (flx_refit.hip).  The
 * links, the storage order and the ids of the scene depend on entry kinds, skip counts and transform numbers alone, and those stay: nothing is sorted or threaded
 * again.  Ordered like an upload() of a shared scene array — the frame server's launch ends, the second lane's frames in flight are waited for, the result is
 * complete before the call returns where there is a second lane — but NOT behind a wait for this context's own frames in flight: the copies and kernels follow them
 * on its stream.  staged: the event behind which the check kernel has filled the stage; nullptr: the geometry rows are in h_update and cross the bus here. */
enum RowsFrom { ROWS_NONE, ROWS_PINNED, ROWS_DEVICE };      /* an update's attribute rows: none; behind the geometry rows in h_update; in d_update_attributes */
static flx_status commit_rows(flx_context *ctx, uint32_t first_entry, uint32_t n_entries, bool bounded, RowsFrom attributes, hipEvent_t staged) {
  flx_status s;
  if ((s = flx_server_stop(ctx)) || (s = shared_upload_begin(ctx))) return s;          /* (a running frame server reads the scene) */
  ctx->geometry_version++; ctx->scene_version++; ctx->structure_version++;
  if (!bounded) ctx->walk_fast_boxes = 0u;          /* until the next flx_scene_upload: both box tests give the same bits under the precondition */
  ctx->walk_thick_boxes = 0u;                       /* the refit below makes the boxes on the device and nothing reads them back: not known to be thick (a hint of speed alone), until the next upload */
  if (staged) FLX_HIP(ctx, hipStreamWaitEvent(ctx->stream, staged, 0));
  else FLX_HIP(ctx, hipMemcpyAsync(ctx->d_update_rows, ctx->h_update, (size_t)n_entries * 48, hipMemcpyHostToDevice, ctx->stream));
  float4 *const rows = ctx->d_attributes + (size_t)first_entry * 7;
  if (attributes == ROWS_PINNED) FLX_HIP(ctx, hipMemcpyAsync(rows, ctx->h_update + (size_t)n_entries * 12, (size_t)n_entries * 112, hipMemcpyHostToDevice, ctx->stream));
  if (attributes == ROWS_DEVICE) FLX_HIP(ctx, hipMemcpyAsync(rows, ctx->d_update_attributes, (size_t)n_entries * 112, hipMemcpyDeviceToDevice, ctx->stream));
  launch_scene_rows(ctx->d_update_rows, ctx->d_geometry, first_entry, n_entries, ctx->stream);
  FLX_HIP(ctx, hipEventRecord(ctx->update_done, ctx->stream));      /* the stage has been consumed: the next update of either kind waits for this before it overwrites it */
  ctx->update_pending = true;
  launch_refit(ctx->d_geometry, ctx->n_entries, ctx->d_refit, ctx->stream);
  launch_rederive(ctx->d_geometry, ctx->n_entries, ctx->d_walk, ctx->walk_entries, ctx->stream);
  launch_rederive(ctx->d_geometry, ctx->n_entries, ctx->d_fwd, ctx->fwd_entries, ctx->stream);
  FLX_HIP(ctx, hipGetLastError());
  return shared_upload_end(ctx);
}

/* Rows of the uploaded scene replaced (vertices that moved, their attribute rows): only the rows cross the bus, and every refusal comes before anything is touched. */
extern "C" flx_status flx_scene_update(flx_context *ctx, uint32_t first_entry, uint32_t n_entries, const float *geometry, const float *attributes) {
  flx_status s = update_refused(ctx, first_entry, n_entries, geometry);
  if (s || n_entries == 0) return s;
  bool bounded = true;
  if (ctx->entry_meta_stale && (s = fetch_entry_meta(ctx))) return s;      /* (the scene came through flx_scene_upload_device) */
  for (uint32_t r = 0; r < n_entries; r++) {
    const float *e = geometry + (size_t)r * 12;
    const uint32_t *m = &ctx->h_entry_meta[((size_t)first_entry + r) * 3];
    uint32_t w6, w9, w10;
    memcpy(&w6, e + 6, 4); memcpy(&w9, e + 9, 4); memcpy(&w10, e + 10, 4);
    if (w10 != m[2]) return fail(ctx, FLX_ERR_INVALID, SCENE_UPDATE_REFUSAL[UPDATE_RULE_KIND]);
    if (e[10] == 0.0f) continue;
    if (w9 != m[1]) return fail(ctx, FLX_ERR_INVALID, SCENE_UPDATE_REFUSAL[UPDATE_RULE_TRANSFORM]);
    if (e[10] == 1.0f) {
      if (w6 != m[0]) return fail(ctx, FLX_ERR_INVALID, SCENE_UPDATE_REFUSAL[UPDATE_RULE_SKIP]);
    } else {
      for (int k = 0; k < 9; k++) {
        if (!std::isfinite(e[k])) return fail(ctx, FLX_ERR_INVALID, SCENE_UPDATE_REFUSAL[UPDATE_RULE_FINITE]);
        if (!(std::fabs(e[k]) <= FLX_FAST_BOX_BOUND)) bounded = false;      /* (the boxes are min / max of vertices) */
      }
    }
  }
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  const size_t gfloats = (size_t)n_entries * 12, afloats = attributes ? (size_t)n_entries * 28 : 0;
  if ((s = ensure_update_buffers(ctx, n_entries, gfloats + afloats, false))) return s;
  memcpy(ctx->h_update, geometry, gfloats * 4);
  if (attributes) memcpy(ctx->h_update + gfloats, attributes, afloats * 4);
  return commit_rows(ctx, first_entry, n_entries, bounded, attributes ? ROWS_PINNED : ROWS_NONE, nullptr);
}

/* flx_scene_update for rows in device memory.  What the host's loop over the rows decides there, k_rows_check_stage (flx_refit.hip) decides here, on update_stream:
 * the host waits for that stream alone — the frames in flight on ctx->stream go on — and reads the verdict.  The same pass has copied the rows into the stage.
 * Nothing of the scene has been touched and nothing is enqueued on ctx->stream when a row is refused. */
extern "C" flx_status flx_scene_update_device(flx_context *ctx, uint32_t first_entry, uint32_t n_entries, const void *d_geometry, const void *d_attributes,
                                              void *producer_stream) {
  flx_status s = update_refused(ctx, first_entry, n_entries, d_geometry);
  if (s || n_entries == 0) return s;
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  if (!rows_on_device(ctx, d_geometry, (size_t)n_entries * 48) || (d_attributes && !rows_on_device(ctx, d_attributes, (size_t)n_entries * 112)))
    return fail(ctx, FLX_ERR_INVALID, "flx_scene_update_device: the rows are not in memory of the context's device, 16-byte aligned");
  if ((s = ensure_update_buffers(ctx, n_entries, 0, d_attributes != nullptr)) || (s = check_on_side_stream(ctx, producer_stream))) return s;
  FLX_HIP(ctx, hipStreamWaitEvent(ctx->update_stream, ctx->geometry_uploaded, 0));      /* (words 6, 9 and 10 of d_geometry: written by an upload alone) */
  FLX_HIP(ctx, hipMemsetAsync(ctx->d_update_verdict, 0xff, 16, ctx->update_stream));
  launch_rows_check_stage((const float4 *)d_geometry, (const float4 *)d_attributes, ctx->d_geometry, first_entry, n_entries, ctx->d_update_rows,
                          ctx->d_update_attributes, ctx->d_update_verdict, ctx->update_stream);
  FLX_HIP(ctx, hipGetLastError());
  FLX_HIP(ctx, hipMemcpyAsync(ctx->h_update_verdict, ctx->d_update_verdict, 16, hipMemcpyDeviceToHost, ctx->update_stream));
  if ((s = await_check(ctx))) return s;
  const uint32_t verdict = ctx->h_update_verdict[0];
  if (verdict != 0xffffffffu) return fail(ctx, FLX_ERR_INVALID, SCENE_UPDATE_REFUSAL[verdict & 3u]);
  return commit_rows(ctx, first_entry, n_entries, ctx->h_update_verdict[1] != 0u, d_attributes ? ROWS_DEVICE : ROWS_NONE, ctx->update_checked);
}

/* ---- a mesh's box tree, built on the device (flx_build.hip) ----------------------------------------------------------------------------------------------
 * Why a row is refused, in the order they are met within a row; the values are k_tree_check's rule numbers. */
constexpr uint32_t TREE_MAX_TRIANGLES = 1u << 24;
static const char *const TREE_BUILD_REFUSAL[3] = { "flx_tree_build_device: a row is not a triangle (word 10 is not 2)",
                                                   "flx_tree_build_device: a row's transform number (word 9) differs from row 0's or is no whole number in [0, 2^20)",
                                                   "flx_tree_build_device: a vertex is not finite" };

static TreeArrays tree_arrays(flx_context *ctx) {
  auto &t = ctx->tree;
  return TreeArrays{ t.tbox, t.perm[t.current], t.perm[t.current ^ 1], t.owner[t.current], t.owner[t.current ^ 1], t.open, t.bucket, t.entry, t.x, t.y, t.totals,
                     t.node, t.cnt, t.keys, t.centre };
}

/* the arrays per node, for `capacity` nodes; what they hold of the first `kept` nodes stays (a copy on update_stream, waited for before the old arrays go) */
template <typename T>
static flx_status tree_grow(flx_context *ctx, DeviceBuffer<T> &buffer, size_t kept, size_t items) {
  DeviceBuffer<T> bigger;
  flx_status s = bigger.ensure(ctx, items);
  if (s) return s;
  if (kept) {
    FLX_HIP(ctx, hipMemcpyAsync(bigger, buffer, kept * sizeof(T), hipMemcpyDeviceToDevice, ctx->update_stream));
    FLX_HIP(ctx, hipStreamSynchronize(ctx->update_stream));
  }
  buffer = std::move(bigger);
  return FLX_OK;
}
static flx_status tree_node_room(flx_context *ctx, uint32_t n_triangles, size_t kept, size_t capacity) {
  auto &t = ctx->tree;
  flx_status s;
  if (t.node_capacity < capacity || !t.node) {
    if (kept == 0) { t.node.release(ctx); t.cnt.release(ctx); t.keys.release(ctx); t.centre.release(ctx); t.y.release(ctx); }      /* (nothing to carry: not both sizes at once) */
    if ((s = tree_grow(ctx, t.node, kept, capacity)) || (s = tree_grow(ctx, t.cnt, kept, capacity)) || (s = tree_grow(ctx, t.keys, kept * 6, capacity * 6)) ||
        (s = tree_grow(ctx, t.centre, 0, capacity * 3)) || (s = tree_grow(ctx, t.y, kept ? kept + 1 : 0, capacity + 1))) { t.node_capacity = 0; return s; }
    t.node_capacity = capacity;
  }
  return t.totals.ensure(ctx, std::max(scan_totals_items(n_triangles + 1u), scan_totals_items((uint32_t)t.node_capacity + 1u)));
}

/* The host's split, a level per round: the level's kernels, then the host waits — on update_stream alone, the frames in flight go on — for the number of children
 * the level has, makes room for them where the node arrays are full, and launches what makes them.  The first wait brings the refusals' verdict too.  A refused
 * or failed build leaves no tree (flx_tree_emit_device is refused); the uploaded scene is not touched in any case. */
extern "C" flx_status flx_tree_build_device(flx_context *ctx, const void *d_triangles, uint32_t n_triangles, void *producer_stream, uint32_t *n_entries) {
  if (!ctx) return FLX_ERR_INVALID;
  auto &t = ctx->tree;
  t.valid = false;
  if (!d_triangles || !n_entries) return fail(ctx, FLX_ERR_INVALID, "flx_tree_build_device: d_triangles or n_entries is NULL");
  if (n_triangles == 0 || n_triangles > TREE_MAX_TRIANGLES) return fail(ctx, FLX_ERR_INVALID, "flx_tree_build_device: n_triangles is 0 or above 2^24");
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  if (!rows_on_device(ctx, d_triangles, (size_t)n_triangles * 48))
    return fail(ctx, FLX_ERR_INVALID, "flx_tree_build_device: the rows are not in memory of the context's device, 16-byte aligned");
  const uint32_t n = n_triangles;
  flx_status s;
  if ((s = ensure_side_stream(ctx))) return s;
  FLX_HIP(ctx, hipStreamSynchronize(ctx->update_stream));      /* (the last build's index kernels, an emit's refit: before an array of theirs is replaced) */
  if ((s = t.tbox.ensure(ctx, (size_t)n * 3)) || (s = t.perm[0].ensure(ctx, n)) || (s = t.perm[1].ensure(ctx, n)) || (s = t.owner[0].ensure(ctx, n)) ||
      (s = t.owner[1].ensure(ctx, n)) || (s = t.open.ensure(ctx, (size_t)n + 1)) || (s = t.bucket.ensure(ctx, n)) || (s = t.entry.ensure(ctx, n)) ||
      (s = t.x.ensure(ctx, (size_t)n + 1)) || (s = t.verdict.ensure(ctx, 4)) || (s = ctx->h_tree_record.ensure(ctx, 4, hipHostMallocDefault)) ||
      (s = tree_node_room(ctx, n, 0, std::max(t.node_capacity, (size_t)n + 64))))
    return s;
  if ((s = check_on_side_stream(ctx, producer_stream))) return s;
  hipStream_t stream = ctx->update_stream;
  uint32_t *const rec = ctx->h_tree_record;
  t.current = 0;
  FLX_HIP(ctx, hipMemsetAsync(t.verdict, 0xff, 16, stream));
  FLX_HIP(ctx, hipMemsetAsync(t.open, 0, ((size_t)n + 1) * 4, stream));
  launch_tree_check((const float4 *)d_triangles, n, t.verdict, tree_arrays(ctx), stream);
  FLX_HIP(ctx, hipMemcpyAsync(rec, t.verdict, 4, hipMemcpyDeviceToHost, stream));
  FLX_HIP(ctx, hipMemcpyAsync(rec + 1, (const char *)d_triangles + 36, 4, hipMemcpyDeviceToHost, stream));      /* row 0's word 9: the boxes' */
  const double maxDepth = std::log2((double)n) + 8.0;          /* flx_mesh.hip: importObj */
  uint32_t base = 0, m = 1, total = 1;
  for (uint32_t depth = 0; ; depth++) {
    launch_tree_level(tree_arrays(ctx), n, base, m, depth, maxDepth, stream);
    FLX_HIP(ctx, hipGetLastError());
    FLX_HIP(ctx, hipMemcpyAsync(rec + 2, t.y.get() + m, 8, hipMemcpyDeviceToHost, stream));
    if ((s = await_check(ctx))) return s;
    if (depth == 0 && rec[0] != 0xffffffffu) return fail(ctx, FLX_ERR_INVALID, TREE_BUILD_REFUSAL[std::min(rec[0] & 3u, 2u)]);
    const uint32_t children = rec[2];
    if (children == 0) break;
    if ((uint64_t)n + total + children > LINK_INDEX) return fail(ctx, FLX_ERR_INVALID, "flx_tree_build_device: the tree has more than 2^28 - 1 entries");
    if ((size_t)total + children > t.node_capacity &&
        (s = tree_node_room(ctx, n, total, std::max(t.node_capacity * 2, (size_t)total + children)))) return s;
    launch_tree_children(tree_arrays(ctx), n, base, m, stream);
    t.current ^= 1;
    base += m; m = children; total += children;
  }
  launch_tree_index(tree_arrays(ctx), n, total, stream);
  FLX_HIP(ctx, hipGetLastError());
  t.n_triangles = n; t.n_nodes = total;
  memcpy(&t.transform, rec + 1, 4);
  t.valid = true;
  *n_entries = n + total;
  return FLX_OK;
}

/* the last build's block: rows and ids, the boxes' floats by the refit that flx_scene_update runs; on update_stream, waited for */
extern "C" flx_status flx_tree_emit_device(flx_context *ctx, const void *d_triangles, const void *d_attributes, void *d_geometry, void *d_attributes_out, void *d_ids) {
  if (!ctx) return FLX_ERR_INVALID;
  auto &t = ctx->tree;
  if (!t.valid) return fail(ctx, FLX_ERR_INVALID, "flx_tree_emit_device without a successful flx_tree_build_device");
  if (!d_triangles || !d_geometry || !d_attributes_out || !d_ids) return fail(ctx, FLX_ERR_INVALID, "flx_tree_emit_device: an array is NULL");
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t n = t.n_triangles, entries = n + t.n_nodes;
  if (!rows_on_device(ctx, d_triangles, (size_t)n * 48))
    return fail(ctx, FLX_ERR_INVALID, "flx_tree_emit_device: d_triangles is not the build's n_triangles rows in memory of the context's device, 16-byte aligned");
  if ((d_attributes && !rows_on_device(ctx, d_attributes, (size_t)n * 112)) || !rows_on_device(ctx, d_geometry, (size_t)entries * 48) ||
      !rows_on_device(ctx, d_attributes_out, (size_t)entries * 112) || !rows_on_device(ctx, d_ids, (size_t)n * 4))
    return fail(ctx, FLX_ERR_INVALID, "flx_tree_emit_device: an array is not in memory of the context's device, 16-byte aligned, or too short for the build");
  flx_status s;
  if ((s = t.refit.ensure(ctx, refit_workspace_words(entries)))) return s;      /* (the last emit was waited for) */
  launch_tree_emit((const float4 *)d_triangles, (const float4 *)d_attributes, tree_arrays(ctx), n, t.n_nodes, t.transform, (float4 *)d_geometry,
                   (float4 *)d_attributes_out, (int32_t *)d_ids, ctx->update_stream);
  launch_refit((float4 *)d_geometry, entries, t.refit, ctx->update_stream);
  FLX_HIP(ctx, hipGetLastError());
  FLX_HIP(ctx, hipStreamSynchronize(ctx->update_stream));
  return FLX_OK;
}

extern "C" flx_status flx_transforms_upload(flx_context *ctx, const float *rotation, const float *shift, uint32_t n_transforms) {
  if (!ctx) return FLX_ERR_INVALID;
  if (!rotation || !shift || n_transforms == 0) return fail(ctx, FLX_ERR_INVALID, "flx_transforms_upload: need at least the identity transform");
  /* The reference refills its transform UBO and its light texture every frame (pathtracerWGL2.js:258-262, 361-365), changed or not.  An upload of what the
   * device holds already is nothing: no copy — and above all no end of a running frame server (upload() stops it: it reads the scene), whose frames in
   * flight would otherwise be completed one by one under a host that re-sends a static scene's arrays per frame. */
  if (!ctx->is_twin && ctx->have_transforms && ctx->n_transforms == n_transforms && ctx->d_rotation && ctx->d_shift &&
      ctx->h_rotation.size() == (size_t)n_transforms * 24 && ctx->h_shift.size() == (size_t)n_transforms * 8 &&
      memcmp(ctx->h_rotation.data(), rotation, (size_t)n_transforms * 96) == 0 && memcmp(ctx->h_shift.data(), shift, (size_t)n_transforms * 32) == 0) return FLX_OK;
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  flx_status s;
  /* the same transforms, moved: the scene moves (the frame server's next launch takes them per frame; one that does already goes on) */
  const bool moved = !ctx->is_twin && ctx->have_transforms && ctx->n_transforms == n_transforms && ctx->d_rotation && ctx->d_shift;
  if (moved && ctx->sv_moving) ctx->sv_want_ver = true;
  if (moved && ctx->sv_running && ctx->sv_ver) {
    /* the running launch takes the transforms with every frame (server_post: from the host's copy) and does not read the device's arrays: they follow when the
     * launch has ended (dyn_flush) — a copy on this context's stream now would wait for that end */
    ctx->transforms_version++; ctx->scene_version++; ctx->dyn_version++;
    ctx->h_rotation.assign(rotation, rotation + (size_t)n_transforms * 24);
    ctx->h_shift.assign(shift, shift + (size_t)n_transforms * 8);
    ctx->dyn_device_stale |= 1u;
    return FLX_OK;
  }
  ctx->have_transforms = false;             /* (until both arrays are in: a failed upload must not pass for the arrays it replaced) */
  ctx->transforms_version++;
  if ((s = upload(ctx, ctx->d_rotation, rotation, (size_t)n_transforms * 96))) return s;
  if ((s = upload(ctx, ctx->d_shift, shift, (size_t)n_transforms * 32))) return s;
  ctx->dyn_device_stale &= ~1u;
  ctx->n_transforms = n_transforms;
  ctx->have_transforms = true;
  if (!ctx->is_twin) {                      /* kept for the frame loop's second lane (flx_frame_begin) */
    ctx->h_rotation.assign(rotation, rotation + (size_t)n_transforms * 24);
    ctx->h_shift.assign(shift, shift + (size_t)n_transforms * 8);
    ctx->dyn_version++;
  }
  return FLX_OK;
}

extern "C" flx_status flx_lights_upload(flx_context *ctx, const float *lights, uint32_t n_lights) {
  if (!ctx) return FLX_ERR_INVALID;
  if (n_lights && !lights) return fail(ctx, FLX_ERR_INVALID, "flx_lights_upload: lights is NULL");
  if (!ctx->is_twin && ctx->have_lights && ctx->n_lights == n_lights && ctx->h_lights.size() == (size_t)n_lights * 6 &&
      (n_lights == 0 || memcmp(ctx->h_lights.data(), lights, (size_t)n_lights * 24) == 0)) return FLX_OK;      /* (as flx_transforms_upload: the same lights again) */
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  flx_status s;
  const bool moved = !ctx->is_twin && ctx->have_lights && ctx->n_lights == n_lights && n_lights != 0 && ctx->d_lights;      /* (as flx_transforms_upload) */
  if (moved && ctx->sv_moving) ctx->sv_want_ver = true;
  if (moved && ctx->sv_running && ctx->sv_ver) {
    ctx->scene_version++; ctx->dyn_version++;
    ctx->h_lights.assign(lights, lights + (size_t)n_lights * 6);
    ctx->dyn_device_stale |= 2u;
    return FLX_OK;
  }
  ctx->have_lights = false;
  if ((s = upload(ctx, ctx->d_lights, lights, (size_t)n_lights * 24))) return s;
  ctx->dyn_device_stale &= ~2u;
  ctx->n_lights = n_lights;
  if (!ctx->is_twin) { ctx->h_lights.assign(lights, lights + (size_t)n_lights * 6); ctx->dyn_version++; ctx->have_lights = true; }
  return FLX_OK;
}

extern "C" flx_status flx_atlas_upload(flx_context *ctx, int which, const uint8_t *rgba, uint32_t width, uint32_t height) {
  if (!ctx) return FLX_ERR_INVALID;
  if (which < 0 || which > 2) return fail(ctx, FLX_ERR_INVALID, "flx_atlas_upload: which must be 0, 1 or 2");
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  size_t bytes = rgba ? (size_t)width * height * 4 : 0;
  flx_status s;
  if ((s = shared_upload_begin(ctx))) return s;
  ctx->atlas_cells[which] = {};              /* (a prebuilt atlas has no known cells: flx_texture_update is refused after it) */
  if ((s = upload(ctx, ctx->d_atlas[which], rgba, bytes))) return s;
  ctx->atlas_w[which] = bytes ? width : 0;
  ctx->atlas_h[which] = bytes ? height : 0;
  return shared_upload_end(ctx);
}

/* ---- atlases built on the device, one texture replaced in place (flx_atlas.hip) ---------------------------------------------------------------------------------
 * The argument rules that need no device: flx_texture_args.h. */
static_assert(FLX_IMAGE_RGBA8 == ATLAS_RGBA8 && FLX_IMAGE_RGBA32F == ATLAS_RGBA32F, "the kernel's formats are the header's");
static const char *const TEXTURE_NOT_ON_DEVICE = "an image's pixels are not in memory of the context's device, not aligned (4 bytes for RGBA8, 16 for RGBA32F), or the allocation ends before the image";

static bool image_on_device(const flx_context *ctx, const flx_image *image) {
  const uint64_t bytes = flx_image_bytes(image);
  return bytes != 0u && bytes <= SIZE_MAX && rows_on_device(ctx, image->pixels, (size_t)bytes, flx_image_texel_bytes(image->format));
}

/* host images staged behind each other in d_texture_src, each at a multiple of 16 bytes, by copies on `stream`; sources[i] <- where image i then is.  Nothing in
 * flight reads the buffer: every call that fills it waits for the kernel that reads it before it returns. */
static flx_status stage_host_images(flx_context *ctx, const flx_image *images, uint32_t n, std::vector<AtlasSource> &sources, hipStream_t stream) {
  size_t total = 0;
  for (uint32_t i = 0; i < n; i++) total += ((size_t)flx_image_bytes(images + i) + 15u) / 16u;
  flx_status s;
  if ((s = ctx->d_texture_src.ensure(ctx, total))) return s;
  size_t at = 0;
  for (uint32_t i = 0; i < n; i++) {
    const size_t bytes = (size_t)flx_image_bytes(images + i);
    FLX_HIP(ctx, hipMemcpyAsync(ctx->d_texture_src + at, images[i].pixels, bytes, hipMemcpyHostToDevice, stream));
    sources[i] = AtlasSource{ ctx->d_texture_src + at, images[i].width, images[i].height, images[i].format, 0u };
    at += (bytes + 15u) / 16u;
  }
  return FLX_OK;
}

static flx_status textures_upload(flx_context *ctx, int which, const flx_image *images, uint32_t n, uint32_t cell_w, uint32_t cell_h, void *producer_stream, bool device) {
  if (!ctx) return FLX_ERR_INVALID;
  if (flx_textures_refusal r = flx_textures_cells_check(which, images != nullptr, n, cell_w, cell_h)) return fail(ctx, FLX_ERR_INVALID, FLX_TEXTURES_UPLOAD_REFUSAL[r]);
  if (n == 0) return flx_atlas_upload(ctx, which, nullptr, 0, 0);      /* "none" */
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  for (uint32_t i = 0; i < n; i++) {
    if (flx_textures_refusal r = flx_image_check(images + i)) return fail(ctx, FLX_ERR_INVALID, FLX_TEXTURES_UPLOAD_REFUSAL[r]);
    if (device ? !image_on_device(ctx, images + i) : flx_image_bytes(images + i) == 0u)
      return fail(ctx, FLX_ERR_INVALID, device ? (std::string("flx_textures_upload_device: ") + TEXTURE_NOT_ON_DEVICE).c_str() : "flx_textures_upload: an image's bytes do not fit 64 bits");
  }
  if ((uint64_t)cell_h * n >= 0x80000000ull) return fail(ctx, FLX_ERR_INVALID, FLX_TEXTURES_UPLOAD_REFUSAL[FLX_TEXTURES_TALL]);
  const uint32_t tw = flx_atlas_cells_per_row(cell_w), W = flx_atlas_width(cell_w), H = flx_atlas_height(cell_h, n);
  std::vector<AtlasSource> sources(n);
  flx_status s;
  if ((s = ensure_side_stream(ctx))) return s;
  if (device) {
    for (uint32_t i = 0; i < n; i++) sources[i] = AtlasSource{ images[i].pixels, images[i].width, images[i].height, images[i].format, 0u };
    if (producer_stream) FLX_HIP(ctx, hipEventRecord(ctx->update_produced, (hipStream_t)producer_stream));
  }
  /* from here the atlas changes: until the end the context has none */
  if ((s = shared_upload_begin(ctx))) return s;
  ctx->atlas_cells[which] = {}; ctx->atlas_w[which] = ctx->atlas_h[which] = 0;
  if ((s = make_room(ctx, ctx->d_atlas[which], (size_t)W * H * 4))) return s;
  if (device && producer_stream) FLX_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->update_produced, 0));
  if (!device && (s = stage_host_images(ctx, images, n, sources, ctx->stream))) return s;
  /* transparent black outside the n cells (the buffer may come from a larger atlas): the rows from the first cell row that is not full */
  uint32_t *const atlas = (uint32_t *)ctx->d_atlas[which].get();
  const size_t full_rows = (size_t)(n / tw) * cell_h;
  if (full_rows < H) FLX_HIP(ctx, hipMemsetAsync(atlas + full_rows * W, 0, ((size_t)H - full_rows) * W * 4, ctx->stream));
  for (uint32_t first = 0; first < n; first += ATLAS_TABLE_IMAGES) {
    const uint32_t count = std::min(n - first, ATLAS_TABLE_IMAGES);
    const uint64_t sv = ctx->scene_version, tv = ctx->structure_version;
    if ((s = upload(ctx, ctx->d_texture_table, sources.data() + first, (size_t)count * sizeof(AtlasSource)))) return s;      /* (the staging ring; in stream order) */
    ctx->scene_version = sv; ctx->structure_version = tv;      /* (one upload, counted once) */
    launch_atlas_cells(atlas, W, cell_w, cell_h, tw, first, count, ctx->d_texture_table, nullptr, ctx->stream);
    FLX_HIP(ctx, hipGetLastError());
  }
  ctx->atlas_w[which] = W; ctx->atlas_h[which] = H;
  ctx->atlas_cells[which].w = cell_w; ctx->atlas_cells[which].h = cell_h; ctx->atlas_cells[which].n = n;
  FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));          /* the caller's pixels are not retained (and: shared_upload_end) */
  return FLX_OK;
}

extern "C" flx_status flx_textures_upload(flx_context *ctx, int which, const flx_image *images, uint32_t n, uint32_t cell_w, uint32_t cell_h) {
  return textures_upload(ctx, which, images, n, cell_w, cell_h, nullptr, false);
}
extern "C" flx_status flx_textures_upload_device(flx_context *ctx, int which, const flx_image *images, uint32_t n, uint32_t cell_w, uint32_t cell_h, void *producer_stream) {
  return textures_upload(ctx, which, images, n, cell_w, cell_h, producer_stream, true);
}

/* One cell replaced, step for step as flx_scene_update_device and commit_rows: the image resampled on update_stream into the stage of one cell (the host waits for
 * that stream alone: the frames in flight go on, the caller's pixels are free); then the frame server's launch ends, the second lane's frames are waited for, and the
 * context's stream copies the stage into the cell behind its own frames in flight — the same kernel, the stage as an RGBA8 source of the cell's size. */
static flx_status texture_update(flx_context *ctx, int which, uint32_t index, const flx_image *image, void *producer_stream, bool device) {
  if (!ctx) return FLX_ERR_INVALID;
  const uint32_t cells = which >= 0 && which <= 2 && ctx->d_atlas[which] ? ctx->atlas_cells[which].n : 0u;
  if (flx_textures_refusal r = flx_texture_update_check(which, cells, index, image)) return fail(ctx, FLX_ERR_INVALID, FLX_TEXTURE_UPDATE_REFUSAL[r]);
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  if (device ? !image_on_device(ctx, image) : flx_image_bytes(image) == 0u)
    return fail(ctx, FLX_ERR_INVALID, device ? (std::string("flx_texture_update_device: ") + TEXTURE_NOT_ON_DEVICE).c_str() : "flx_texture_update: the image's bytes do not fit 64 bits");
  const uint32_t w = ctx->atlas_cells[which].w, h = ctx->atlas_cells[which].h, tw = flx_atlas_cells_per_row(w);
  flx_status s;
  if ((s = ensure_side_stream(ctx))) return s;
  if (ctx->update_pending) { FLX_HIP(ctx, hipEventSynchronize(ctx->update_done)); ctx->update_pending = false; }      /* (the last update's copy reads the stage) */
  if ((s = ctx->d_texture_cell.ensure(ctx, (size_t)w * h))) return s;
  if ((s = check_on_side_stream(ctx, device ? producer_stream : nullptr))) return s;
  std::vector<AtlasSource> source(1, AtlasSource{ image->pixels, image->width, image->height, image->format, 0u });
  if (!device && (s = stage_host_images(ctx, image, 1, source, ctx->update_stream))) return s;
  launch_atlas_cells(ctx->d_texture_cell, w, w, h, 1u, 0u, 1u, nullptr, &source[0], ctx->update_stream);
  FLX_HIP(ctx, hipGetLastError());
  if ((s = await_check(ctx))) return s;
  if ((s = flx_server_stop(ctx)) || (s = shared_upload_begin(ctx))) return s;          /* (a running frame server reads the atlas) */
  ctx->scene_version++; ctx->structure_version++;
  FLX_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->update_checked, 0));
  const AtlasSource staged = { ctx->d_texture_cell.get(), w, h, ATLAS_RGBA8, 0u };
  launch_atlas_cells((uint32_t *)ctx->d_atlas[which].get(), ctx->atlas_w[which], w, h, tw, index, 1u, nullptr, &staged, ctx->stream);
  FLX_HIP(ctx, hipGetLastError());
  FLX_HIP(ctx, hipEventRecord(ctx->update_done, ctx->stream));      /* the stage has been consumed: the next update of either kind waits for this before it overwrites it */
  ctx->update_pending = true;
  return shared_upload_end(ctx);
}

extern "C" flx_status flx_texture_update(flx_context *ctx, int which, uint32_t index, const flx_image *image) { return texture_update(ctx, which, index, image, nullptr, false); }
extern "C" flx_status flx_texture_update_device(flx_context *ctx, int which, uint32_t index, const flx_image *image, void *producer_stream) {
  return texture_update(ctx, which, index, image, producer_stream, true);
}

extern "C" flx_status flx_debug_atlas_read(flx_context *ctx, int which, uint8_t *out, size_t bytes, uint32_t *width, uint32_t *height) {
  if (!ctx) return FLX_ERR_INVALID;
  if (which < 0 || which > 2) return fail(ctx, FLX_ERR_INVALID, "flx_debug_atlas_read: which must be 0, 1 or 2");
  const bool have = ctx->d_atlas[which] != nullptr;
  const uint32_t W = have ? ctx->atlas_w[which] : 0u, H = have ? ctx->atlas_h[which] : 0u;
  if (width) *width = W;
  if (height) *height = H;
  const size_t need = (size_t)W * H * 4;
  if (!out || need == 0) return FLX_OK;
  if (bytes < need) return fail(ctx, FLX_ERR_INVALID, "flx_debug_atlas_read: out is smaller than the atlas");
  FLX_HIP(ctx, hipSetDevice(ctx->device));
  FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  FLX_HIP(ctx, hipMemcpy(out, ctx->d_atlas[which].get(), need, hipMemcpyDeviceToHost));
  return FLX_OK;
}

extern "C" flx_status flx_scene_upload_view(flx_context *ctx, const flx_scene_view *v) {
  if (!ctx || !v) return FLX_ERR_INVALID;
  flx_status s;
  if ((s = flx_scene_upload(ctx, v->geometry, v->attributes, v->n_entries_padded, v->ids, v->n_ids))) return s;
  if ((s = flx_transforms_upload(ctx, v->rotation, v->shift, v->n_transforms))) return s;
  if ((s = flx_lights_upload(ctx, v->lights, v->n_lights))) return s;
  for (int i = 0; i < 3; i++)
    if ((s = flx_atlas_upload(ctx, i, v->atlas[i], v->atlas_w[i], v->atlas_h[i]))) return s;
  return FLX_OK;
}

/* the device's transforms and lights follow the host's copies (uploads that a launch for a scene that moves went on over): before anything else reads them */
flx_status flx_dyn_flush(flx_context *ctx) {
  const uint32_t stale = ctx->dyn_device_stale;
  if (!stale || ctx->sv_running) return FLX_OK;
  FLX_HIP(ctx, hipSetDevice(ctx->device));      /* (a group ends its contexts' launches one after the other from one thread) */
  ctx->dyn_device_stale = 0u;
  flx_status s;
  const uint64_t sv = ctx->scene_version, dv = ctx->dyn_version;
  const uint32_t tv = ctx->transforms_version;
  if (stale & 1u) {
    const std::vector<float> r = ctx->h_rotation, sh = ctx->h_shift;
    if ((s = upload(ctx, ctx->d_rotation, r.data(), r.size() * sizeof(float)))) return s;
    if ((s = upload(ctx, ctx->d_shift, sh.data(), sh.size() * sizeof(float)))) return s;
  }
  if (stale & 2u) {
    const std::vector<float> l = ctx->h_lights;
    if ((s = upload(ctx, ctx->d_lights, l.data(), l.size() * sizeof(float)))) return s;
  }
  ctx->scene_version = sv; ctx->dyn_version = dv; ctx->transforms_version = tv;      /* (the same contents the versions were counted for) */
  return FLX_OK;
}
