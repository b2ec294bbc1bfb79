/*
 * flexlight_hip.h — C ABI of libflexlight_hip.so: FlexLight's path-tracing inner loop on MI355X.
 *
 * The reference has no plugin / FFI interface; the boundary this library sits behind is the
 * duck-typed renderer object FlexLight selects by string (flexlight.js:106-129, constructed
 * flexlight.js:113, members modules/pathtracerWGL2.js:25-78,143,167,191).  Every entry point
 * below replaces one piece of what that object does with the WebGL2 driver; the JavaScript
 * renderer (web-ray-tracer_amd/js/pathtracerHIP.js) binds them through the N-API shim
 * (web-ray-tracer_amd/napi/flexlight_napi.cc), tests and bench.py bind them through ctypes.
 *
 * Conventions: plain pointers and sizes only; the caller owns every host pointer, the library
 * copies in during the call and keeps nothing; every function returns 0 on success and a
 * non-zero flx_status otherwise, with text from flx_last_error(); nothing throws or aborts.
 * A context is bound to one GPU and is not thread-safe.  There is NO CPU fallback: without a
 * GPU flx_context_create fails.
 */
#ifndef FLEXLIGHT_HIP_H
#define FLEXLIGHT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int flx_status;
enum {
  FLX_OK = 0,
  FLX_ERR_INVALID = 1,      /* bad argument / inconsistent sizes */
  FLX_ERR_DEVICE = 2,       /* HIP runtime error (message has the hipError string) */
  FLX_ERR_NO_SCENE = 3,     /* render before scene / transforms upload */
  FLX_ERR_NO_GPU = 4        /* no usable gfx950 device */
};

typedef struct flx_context flx_context;

/* Host view of the flattened scene: SURVEY.md §8a rows D1–D6.  All pointers are host memory. */
typedef struct flx_scene_view {
  const float *geometry;        /* D1: 12 f32 per entry, n_entries_padded entries (scene.js:224-298) */
  const float *attributes;      /* D2: 28 f32 per entry, same index (scene.js:635-641) */
  uint32_t n_entries_padded;    /* multiple of 256; zero entries terminate traversal */
  const int32_t *ids;           /* D3: entry index of every triangle (scene.js:267,302) */
  uint32_t n_ids;
  const float *rotation;        /* D4: per transform 24 f32: forward then inverse std140 mat3 (scene.js:500-521) */
  const float *shift;           /* D4: per transform 8 f32: position xyz_, -position xyz_ */
  uint32_t n_transforms;
  const float *lights;          /* D5: per light x y z intensity variation 0 (pathtracerWGL2.js:143-165) */
  uint32_t n_lights;
  const uint8_t *atlas[3];      /* D6: RGBA8 atlases: 0 albedo (tex), 1 pbr, 2 translucency; may be NULL */
  uint32_t atlas_w[3], atlas_h[3];
} flx_scene_view;

/* Per-frame uniforms: SURVEY.md §8a row D7 (modules/pathtracerWGL2.js:329-347) plus the tile policy. */
typedef struct flx_frame_params {
  uint32_t width, height;       /* canvas size */
  float camera[3];              /* cameraPosition */
  float view_matrix[9];         /* row-major rows as built at pathtracerWGL2.js:312-318 */
  int32_t samples;              /* config.samplesPerRay */
  int32_t max_reflections;      /* config.maxReflections */
  float min_importancy;         /* config.minImportancy */
  int32_t use_filter;           /* config.filter: write the five G-buffers and run the denoise chain */
  int32_t is_temporal;          /* config.temporal: fract/floor split (fragment:626-629) + the temporal accumulation pass over the context's history */
  int32_t hdr;                  /* config.hdr, final filter tone map */
  float ambient[3];             /* scene.ambientLight */
  float random_seed;            /* 0 unless temporal (pathtracerWGL2.js:347) */
  int32_t texture_width;        /* floor(2048 / standardTextureSizes[0]) */
  /* Tile policy (multi-GPU): the frame is cut into strips of tile_rows image rows,
   * strip s belongs to the context with s % tile_count == tile_index.  0/0/0 or x/0/1 = whole frame. */
  uint32_t tile_rows, tile_index, tile_count;
  int32_t temporal_samples;     /* config.temporalSamples: history depth of the temporal pass (1..16; 0 = 4) */
} flx_frame_params;

/* Work counters of one frame; identical numbers come out of the CPU oracle for the same frame and
 * feed the algorithmic-bytes roofline of SURVEY.md §8d. */
typedef struct flx_counters {
  uint64_t primary_visits;      /* D1 entries fetched by the primary-visibility walks (P0) */
  uint64_t closest_visits;      /* ... by rayTracer walks (T1) */
  uint64_t shadow_visits;       /* ... by shadowTest walks (T2) */
  uint64_t closest_walks;
  uint64_t shadow_walks;
  uint64_t shades;              /* bounce iterations executed (S1) */
  uint64_t primary_hits;        /* pixels with a primary hit */
  uint64_t atlas_texels;        /* atlas texels fetched (S5) */
} flx_counters;

/* Optional float32 pre-quantisation G-buffers (row D8), W*H*4 floats each, packed like the radiance. */
typedef struct flx_gbuffers {
  float *color;                 /* renderColor */
  float *color_ip;              /* renderColorIp */
  float *original_color;        /* renderOriginalColor */
  float *id;                    /* renderId */
  float *original_id;           /* renderOriginalId */
  float *location_id;           /* renderLocationId (fragment:640-642); may be NULL */
} flx_gbuffers;

/* ---- life cycle -------------------------------------------------------------------------------- */
/* Replaces canvas.getContext('webgl2') + prepareEngine() (pathtracerWGL2.js:60-68,556-788). */
flx_status flx_context_create(int device, flx_context **out);
/* Replaces halt()'s gl.loseContext() (pathtracerWGL2.js:70-77). */
void flx_context_destroy(flx_context *ctx);
const char *flx_last_error(const flx_context *ctx);     /* ctx may be NULL: last creation error */

/* ---- uploads ----------------------------------------------------------------------------------- */
/* Replaces updateScene()'s two texImage2D uploads + idBuffer (pathtracerWGL2.js:167-189,367-368). */
flx_status flx_scene_upload(flx_context *ctx, const float *geometry, const float *attributes,
                            uint32_t n_entries_padded, const int32_t *ids, uint32_t n_ids);
/* Replaces the per-frame UBO fill from Transform.buildWGL2Arrays() (pathtracerWGL2.js:361-365). */
flx_status flx_transforms_upload(flx_context *ctx, const float *rotation, const float *shift, uint32_t n_transforms);
/* Replaces updatePrimaryLightSources() (pathtracerWGL2.js:143-165). n_lights may be 0. */
flx_status flx_lights_upload(flx_context *ctx, const float *lights, uint32_t n_lights);
/* Replaces #updateAtlas (pathtracerWGL2.js:85-104); which: 0 albedo, 1 pbr, 2 translucency. rgba NULL = none. */
flx_status flx_atlas_upload(flx_context *ctx, int which, const uint8_t *rgba, uint32_t width, uint32_t height);
/* All of the above from one view. */
flx_status flx_scene_upload_view(flx_context *ctx, const flx_scene_view *scene);
/* (A scene whose VERTICES move need not come through here again: flx_scene_update, flexlight_hip_debug.h, takes the rows that changed.) */

/* ---- one frame ---------------------------------------------------------------------------------- */
/* Number of image rows the tile policy of `params` assigns to this context (whole frame: height). */
uint32_t flx_tile_row_count(const flx_frame_params *params);
/* Image row (0 = top) of the context's k-th packed row. */
uint32_t flx_tile_row_at(const flx_frame_params *params, uint32_t k);

/* Replaces renderFrame() (pathtracerWGL2.js:375-554) for one frame: path-trace pass and, with
 * use_filter, the denoise chain.  out_rgba: flx_tile_row_count()*width*4 floats (host), rows packed
 * in strip order, top row first; without filter = renderColor of fragment:631 (miss pixels 0,0,0,0),
 * with filter = the final filter's canvas colour.  gbuffers / counters may be NULL. */
flx_status flx_render(flx_context *ctx, const flx_frame_params *params, float *out_rgba,
                      const flx_gbuffers *gbuffers, flx_counters *counters);
/* Temporal frames (is_temporal = 1) keep config.temporalSamples frames of history in the context, like the
 * reference's TempTexture rings (pathtracerWGL2.js:389-402,419-460): every call rotates the ring, traces with
 * params->random_seed (the caller passes frame % temporalSamples, pathtracerWGL2.js:291,347) and averages the
 * history where the packed ids match.  flx_temporal_reset forgets the history (a resize does the same).  A temporal frame
 * without the filter may be tiled (params->tile_*): the pass is per pixel, and the context keeps the history of exactly the
 * rows it traces — a change of temporalSamples, size or tile policy starts a fresh history, and a context given no rows does
 * nothing.  Filter frames are whole frames (the denoise chain reads neighbouring pixels; tiled ones are refused). */
flx_status flx_temporal_reset(flx_context *ctx);
/* Same, output left in DEVICE memory (d_out_rgba is a device pointer on the context's GPU, e.g. a
 * torch tensor's data_ptr) and enqueued on the context's stream without a host sync: for the
 * multi-GPU gather over RCCL.  Call flx_sync before reading on another stream. */
flx_status flx_render_device(flx_context *ctx, const flx_frame_params *params, void *d_out_rgba);
/* A batch of 1 .. 32 frames in one pass of the pipeline (the reference renders frame after frame, pathtracerWGL2.js:329
 * frameCycle; frames without temporal accumulation do not depend on each other — with use_filter the trace of the batch is one
 * pass and the denoise chain then runs frame by frame, every time from the reference's frame-0 texture state; whole frames only).  The frames may differ
 * in camera, view_matrix, ambient and random_seed only; every other field must equal params[0]'s.  Output: the frames one
 * after the other, float4[n_frames][rows][width] with rows = flx_tile_row_count(params) — each frame bit-identical to its
 * flx_render.  The kernels of the pass run once over n_frames times the paths, so the per-kernel costs that do not shrink
 * with the frame (the tail of every walk kernel, launches) are paid once per batch: throughput mode, latency n frames. */
flx_status flx_render_batch(flx_context *ctx, const flx_frame_params *params, uint32_t n_frames, float *out_rgba, flx_counters *counters);
flx_status flx_render_batch_device(flx_context *ctx, const flx_frame_params *params, uint32_t n_frames, void *d_out_rgba);
#define FLX_MAX_BATCH_FRAMES 32
flx_status flx_sync(flx_context *ctx);
/* The rasterizer renderer: replaces rasterizerWGL2.js's rasterizingPass (rasterizerWGL2.js:253-312, the draw state of :395-401)
 * with shaders/rasterizer_vertex.glsl and rasterizer_fragment.glsl:202-291 — every triangle drawn two-sided under the depth test
 * LESS and blended (ONE, ONE_MINUS_SRC_ALPHA / ONE, ONE) into the RGBA8 drawing buffer cleared to (0,0,0,0); the pins are
 * DESIGN.md §2 "Rasterizer".  Uses width, height, camera, view_matrix, hdr, ambient, texture_width and the tile policy; ignores
 * the path-tracing fields.  Output rows as flx_render; every value is the buffer's byte k as k / 255 (flx_present gives the bytes
 * back).  Exactly one of out_rgba (host) / d_out_rgba (device memory, enqueued on the context's stream) is non-NULL; counters
 * may be NULL (given, the call waits for the frame). */
flx_status flx_raster_render(flx_context *ctx, const flx_frame_params *params, float *out_rgba, void *d_out_rgba, flx_counters *counters);
/* Use an existing hipStream_t (e.g. torch's current stream) instead of the context's own. NULL restores it. */
flx_status flx_set_stream(flx_context *ctx, void *hip_stream);
/* GPU time of the last frame between HIP events on the context's stream, and of its dominant
 * (trace) kernel alone; milliseconds. */
flx_status flx_last_frame_ms(flx_context *ctx, float *frame_ms, float *trace_kernel_ms);

/* ---- the frame loop ------------------------------------------------------------------------------------
 * The reference's renderFrame() (pathtracerWGL2.js:375-554) ends with draw calls the browser presents on its own; the
 * JavaScript thread never waits for the GPU.  flx_frame_begin is that half: it enqueues one frame — trace, temporal pass,
 * denoise chain as flx_render would run them, then optionally the 8-bit store of the canvas (flx_present) — and the copy of
 * the result into a pinned host buffer the context owns (on a copy stream: the next frame's kernels start meanwhile), and
 * returns.  flx_frame_end waits for the OLDEST frame begun and hands out its pixels and its GPU time.  At most two frames (three with
 * flx_set_frame_lanes(ctx, 3)) are in flight (a set of buffers each): the host prepares and begins frame N + 1 while frame N is traced and copied.  The pixels
 * stay valid until the second flx_frame_begin after the one that made them (or the context's end); rows and tiles as flx_render: a temporal frame
 * may be tiled without the filter (the history of the context's own rows), a filter frame is whole.  Temporal frames run on the first lane, where the
 * history lives.
 * `format & 0x0f` is one of FLX_FRAME_FLOAT / _RGBA8 / _DEVICE; the flags below may be OR'ed into it (flx_frame_begin only, not
 * flx_frame_begin_gathered or flx_group_frame_begin):
 *   FLX_FRAME_FXAA / FLX_FRAME_TAA: the anti-aliasing pass runs over the frame inside the loop — the frame equals flx_render (or
 *     flx_raster_render) followed by flx_fxaa / flx_taa, and with FLX_FRAME_RGBA8 the pass stores the canvas' bytes itself.  Whole
 *     frames only (the passes read neighbouring texels), one of the two.  FXAA frames use either lane, each lane its own plane; TAA
 *     frames rotate the context's ring of flx_taa (advanced when the frame is begun: flx_taa_reset applies to the frames begun after
 *     it, a change of size resets it) and run on the first lane.
 *   FLX_FRAME_RASTERIZER: the frame is flx_raster_render's (the path-tracing fields are ignored, tiles as flx_render), uncounted, on
 *     both lanes.
 * The frame server (flx_set_frame_chain) takes none of these frames: a running launch is ended first.  Frames of every kind may be
 * interleaved and complete in the order they were begun. */
#define FLX_FRAME_FLOAT 0      /* float32 RGBA, what flx_render returns */
#define FLX_FRAME_RGBA8 1      /* bytes R G B A as the canvas' drawing buffer holds them (flx_present): a quarter of the bytes over PCIe */
#define FLX_FRAME_DEVICE 2     /* float32 RGBA left in device memory: flx_frame_end hands out a device pointer (no copy to the host) */
#define FLX_FRAME_FXAA        0x10   /* the FXAA pass (flx_fxaa_device) over the frame, inside the loop */
#define FLX_FRAME_TAA         0x20   /* the TAA pass (flx_taa_device) over the frame, inside the loop: the context's nine-frame ring */
#define FLX_FRAME_RASTERIZER  0x100  /* the frame is the rasterizer's (what flx_raster_render draws), not the path tracer's */
flx_status flx_frame_begin(flx_context *ctx, const flx_frame_params *params, int format);
flx_status flx_frame_end(flx_context *ctx, const void **pixels, size_t *bytes, float *gpu_ms);
/* The pinned host buffers behind flx_frame_end's `pixels` (FLX_FRAME_FLOAT / FLX_FRAME_RGBA8): slots[0..1] the first lane's,
 * slots[2..3] the second lane's (NULL where none is allocated); *last_begun (may be NULL) = index in `slots` of the buffer the
 * frame begun last will be copied into, -1 if that frame stays in device memory or none was begun.  For bindings that hand the
 * buffers out as zero-copy views and must retire a view when its memory is re-used or re-allocated (napi/flexlight_napi.cc). */
flx_status flx_frame_host_slots(flx_context *ctx, const void *slots[4], int *last_begun);
/* frames begun and not yet ended (0 .. 3) */
int flx_frames_in_flight(const flx_context *ctx);
/* 2 (default): the two frames in flight run on two lanes — two streams with a workspace each (+2 GB at 1080p x 8 spp), the static
 * scene arrays shared — so that frame k + 1's kernels fill the CUs the tails of frame k's kernels leave idle: a whole 1080p dragon frame
 * completes every 6.3 ms instead of every 6.5 ms, each frame's own time (gpu_ms) a little longer.  1: one lane, frames one after the other
 * on the context's stream.  3: three frames in flight where the frame server takes the frames (flx_set_frame_chain), as 2 elsewhere.
 * Temporal frames always use the first lane (their history lives there). */
flx_status flx_set_frame_lanes(flx_context *ctx, int lanes);
/* How consecutive frames of the loop overlap on the GPU.  The reference renders frame after frame from one context without waiting for the GPU
 * (modules/pathtracerWGL2.js:254-303); a frame's own launches, though, end in a drain — the last paths of the frame keep a few waves busy while the
 * other CUs idle — and for a short frame (a rank's eighth of a 1080p frame: 0.8 ms of work, 1.65 ms from launch to end) the drain is half of the time.
 *   0  every frame has its own launches, on the lanes of flx_set_frame_lanes;
 *   1  refused (FLX_ERR_INVALID): the chain of launches it once selected — the frame kernel of frame k working ahead on frame k + 1 — was removed, the
 *      relaunch per frame cost what the overlap gained;
 *   2  (default) the frame server (csrc/flx_server.hip) for frames of fewer than 64 8 x 8 screen tiles per CU — a rank's share of a frame — and mode 0 for the
 *      others: ONE persistent launch renders the loop's frames as flx_frame_begin posts them (the view goes through pinned memory; nothing is launched per
 *      frame), every workgroup works on the oldest frame first and fills its idle lanes with the next ones, resolves the screen tiles it made and the last
 *      one through with a frame tells the host.  With three frames in flight a rank's eighth of the 1080p dragon frame completes every 0.93 - 0.98 ms (all
 *      eight ranks; two lanes: 1.29, one frame at a time: 1.65; profiles/r04_share_scaling.txt).  The launch ends when the loop runs empty (or, by itself, when the host has
 *      said nothing for two seconds: frames in flight that are complete by then are handed out as usual and the next frame starts another launch), or when a frame
 *      of another shape, a scene upload, a synchronous render or flx_sync needs the device;
 *   3  the frame server for every frame it can take, whatever its size (a whole 1080p frame: 6.46 ms against 6.32 on two lanes).
 * The chained modes take frames without filter and temporal accumulation, scenes of more than 128 entries, strips of a multiple of 8 rows, float or
 * device output, work counters off; any other frame runs as in mode 0.  Frames are bit-identical to their own flx_render and complete in order.  A
 * watchdog that trips inside a launch makes flx_frame_end return FLX_ERR_DEVICE. */
flx_status flx_set_frame_chain(flx_context *ctx, int mode);
/* The frame server resolves the loop's frames straight into images the CALLER owns: d_images[i] (n_images = 2 or 3 = the loop's frames in flight;
 * float4[height][width]; addresses this context's GPU can write — its own memory, a peer GPU's through the peer mapping, pinned host memory) takes the frames
 * begun i-th, (i + n)-th, ...  With params.tile_count > 1 the context writes its row strips where the image has them, so the contexts of a device group
 * complete ONE image between them with no exchange, no reassembly kernel and no copy (flx_group_frame_begin does exactly this).  While a target is set, frames
 * must be ones the server takes and FLX_FRAME_DEVICE; flx_frame_end hands out the image's address.  n_images = 0: the launch's own buffers again.  Frames in
 * flight are completed where they were begun. */
flx_status flx_frame_target_set(flx_context *ctx, void *const *d_images, uint32_t n_images);
/* ... images of the canvas' RGBA8 — uint8[height][width][4], the bytes flx_present stores: the launch quantises its tiles as it resolves them (a quarter of the bytes
 * every GPU of a group writes).  Without a target the server does the same for frames begun as FLX_FRAME_RGBA8. */
flx_status flx_frame_target_set8(flx_context *ctx, void *const *d_images, uint32_t n_images);
/* Device faults reach the status code.  The frame kernels' wait loops have watchdogs (seconds); a wave that gives up — or finds a ring slot that never
 * fills — sets a bit in the context's device error word (pinned host memory), and the next call in which the host waits for frames (flx_render,
 * flx_render_batch, flx_frame_end, flx_sync) returns FLX_ERR_DEVICE with the bits in flx_last_error and clears the word: the frame is incomplete.  A healthy
 * frame never gets there (flexlight_hip_debug.h: flx_debug_inject_fault forces it for tests). */

/* Filter frames on several GPUs.  The path-trace pass is per pixel and shards by row strips like a frame
 * without filter; the denoise chain reads up to ~194 rows around a pixel and runs on the whole frame.  So every rank
 *   1. flx_render_planes_device: traces its strips (params->tile_*, use_filter = 1, is_temporal = 0) and stores the
 *      reference's five render targets — RenderTexture, IpRenderTexture, OriginalRenderTexture, IdRenderTexture,
 *      OriginalIdRenderTexture (pathtracerWGL2.js:224-252) — as the RGBA8 they are, rows packed like a tiled frame:
 *      d_planes = uint32[5][rows of this rank][width];
 *   2. all-gathers the planes (5 x 8.3 MB at 1080p) and puts the rows in image order (flx_tile_row_at);
 *   3. flx_filter_planes_device: runs the chain (pathtracerWGL2.js:462-550) over uint32[5][height][width] into
 *      float4[height][width] — bit-identical to flx_render_device of the whole frame on one context. */
flx_status flx_render_planes_device(flx_context *ctx, const flx_frame_params *params, void *d_planes);
flx_status flx_filter_planes_device(flx_context *ctx, const flx_frame_params *params, const void *d_planes, void *d_out_rgba);

/* ---- several GPUs -----------------------------------------------------------------------
 * The path shards by pixels: the frame is cut into strips of tile_rows image rows, strip s belongs to rank s % n, the scene is
 * replicated on every GPU, and ONE exchange step per frame (or batch of frames) brings the strips together: ncclAllGather
 * (RCCL over xGMI) of the packed strips on the contexts' streams, then a kernel of the library puts the gathered rows in
 * image order.  With use_filter the five RGBA8 render targets are gathered instead (5 x 8.3 MB at 1080p) and the denoise
 * chain, which reads up to ~194 rows around a pixel, runs on the whole frame.  Temporal frames go through a group's frame loop
 * only (flx_group_frame_begin), where every context keeps the history of its own strips; the stateless and batch entry points
 * below refuse them.  The reference has one WebGL2 context per renderer (pathtracerWGL2.js:60-68); this is what
 * `new FlexLight(canvas, { devices: N })` of the JavaScript host layer sits on. */

/* One process per GPU (bench.py under torch.distributed.run).  Rank 0 makes an id (ncclGetUniqueId) and hands it to the other
 * ranks by any means; every rank then joins its context to the communicator (ncclCommInitRank; collective: all ranks call). */
#define FLX_COMM_ID_BYTES 128
flx_status flx_comm_unique_id(uint8_t *id /* FLX_COMM_ID_BYTES */);
flx_status flx_comm_init_rank(flx_context *ctx, const uint8_t *id, int n_ranks, int rank);
flx_status flx_comm_destroy(flx_context *ctx);          /* also done by flx_context_destroy */
/* This rank's strips of n_frames frames (1 .. 32; params[i].tile_rows > 0, tile_index = the rank, tile_count = n_ranks; a
 * filter frame alone): traced, all-gathered, reassembled — d_frames = float4[n_frames][height][width] in device memory, the
 * same on every rank and bit-identical to the frames one context renders.  Everything is enqueued on the context's stream
 * without a host synchronisation; flx_last_frame_ms then spans first kernel .. last byte of the gathered frame. */
flx_status flx_render_gathered_device(flx_context *ctx, const flx_frame_params *params, uint32_t n_frames, void *d_frames);
/* The same with ONE receiver — the rank that presents the frame.  ncclGroupStart, one ncclSend per rank to `root`, n ncclRecv on
 * `root`, ncclGroupEnd: a 1080p frame is 33 MB (a 4K frame 133 MB) that the other n - 1 ranks no longer receive; `root`
 * reassembles (and runs the denoise chain of a filter frame), the others are done when their strips are sent.  d_frames is read
 * on `root` only (may be NULL elsewhere).  The reference presents from its one context (pathtracerWGL2.js:60-68, 552-553). */
flx_status flx_render_gathered_root_device(flx_context *ctx, const flx_frame_params *params, uint32_t n_frames, int root, void *d_frames);
/* The gathered frames as the canvas' RGBA8 — the bytes flx_present stores, floor(clamp(x) * 255 + 0.5) per channel (what the reference's canvas holds after
 * pathtracerWGL2.js:552-553 has drawn into it): every rank quantises its strips where it traced them and a QUARTER of the bytes is exchanged (8.3 MB of a
 * 1080p frame in all instead of 33 MB; 33 instead of 133 MB at 4K).  d_frames_rgba8 = uint8[n_frames][height][width][4] in device memory.  root < 0: all-gather,
 * every rank gets the frames; root >= 0: that rank alone (NULL elsewhere).  Frames without the filter (a filter frame's exchange is its five render targets). */
flx_status flx_render_gathered_rgba8_device(flx_context *ctx, const flx_frame_params *params, uint32_t n_frames, int root, void *d_frames_rgba8);
/* The frame loop (flx_frame_begin / flx_frame_end) over the communicator: every rank begins the same frame with its own
 * tile_index; the frames alternate between the context's two lanes, the second lane gathering over a communicator of its own
 * (ncclCommSplit of the first, made by flx_comm_init_rank), so that frame k + 1's kernels fill the CUs the tails of frame k's
 * kernels leave idle on every rank.  root < 0: flx_frame_end hands out the whole frame on every rank; root >= 0: on that rank
 * (0 bytes elsewhere).  Frames complete in order; at most two in flight. */
flx_status flx_frame_begin_gathered(flx_context *ctx, const flx_frame_params *params, int format, int root);

/* One process per GPU WITHOUT a collective: the ranks' frame servers (flx_set_frame_chain) complete ONE image in the root rank's device memory.  The root
 * allocates n_images (2 or 3 = frames in flight) images and exports them (flx_share_create: a hipIpcMemHandle and the name of a page of POSIX shared memory
 * in `handle`, which the caller hands to the other ranks — bench.py broadcasts it over torch.distributed); the others map them (flx_share_join: their stores
 * go over xGMI); every rank's launch resolves its row strips where the image has them.  The loop is the frame loop's: flx_frame_begin_shared (params.tile_count
 * = the ranks, .tile_index = this rank) / flx_frame_end_shared, up to n_images frames in flight on every rank — a frame the frame server does not take (a scene of <= 128
 * entries, a last strip cut by the frame's edge; not filter / temporal frames) is rendered on the rank's two lanes and its strips are copied into the image when the frame is
 * taken (the two kinds cannot be in flight together) —; on the root
 * flx_frame_end_shared waits until every rank has completed its strips of the frame and hands out the image (device memory; valid until the root's next
 * flx_frame_begin_shared — no rank overwrites an image before that), elsewhere it returns NULL / 0 bytes.  Frames equal flx_render of one context bit for bit.
 * A rank that fails or does not answer within 5 s makes every rank's next call return FLX_ERR_DEVICE instead of waiting.  The root is the context that
 * presents, as the reference's one context does (pathtracerWGL2.js:552-553). */
#define FLX_SHARE_HANDLE_BYTES 128
flx_status flx_share_create(flx_context *ctx, uint32_t width, uint32_t height, uint32_t n_images, int n_ranks, int rank, uint8_t *handle /* [FLX_SHARE_HANDLE_BYTES] out */);
flx_status flx_share_join(flx_context *ctx, const uint8_t *handle, int rank);
flx_status flx_share_leave(flx_context *ctx);      /* (also done by flx_context_destroy) */
flx_status flx_frame_begin_shared(flx_context *ctx, const flx_frame_params *params);
flx_status flx_frame_end_shared(flx_context *ctx, const void **image, size_t *bytes, float *ms);

/* One process, n GPUs (the JavaScript host: Node is one process): n contexts, one RCCL communicator each (ncclCommInitAll).
 * `devices` may name one GPU more than once — a rehearsal on a one-GPU box, where RCCL refuses two ranks on a device: the
 * strips are then exchanged with device-to-device copies, everything else is unchanged (flx_group_uses_rccl says which). */
typedef struct flx_group flx_group;
int flx_group_uses_rccl(const flx_group *group);
flx_status flx_group_create(int n, const int *devices, flx_group **out);
void flx_group_destroy(flx_group *group);
const char *flx_group_last_error(const flx_group *group);   /* group may be NULL: last creation error */
int flx_group_size(const flx_group *group);
/* to_root = 1 (default): only context 0 — the one flx_group_render hands the frame out from — receives the strips (ncclSend / ncclRecv,
 * or copies into context 0 alone); 0: all-gather, every context ends up with the frame. */
flx_status flx_group_set_gather(flx_group *group, int to_root);
flx_context *flx_group_context(flx_group *group, int rank);          /* owned by the group; for per-context settings and timings */
/* the uploads of a context, applied to every context of the group (the scene is replicated) */
flx_status flx_group_scene_upload(flx_group *group, const float *geometry, const float *attributes, uint32_t n_entries_padded,
                                  const int32_t *ids, uint32_t n_ids);
flx_status flx_group_transforms_upload(flx_group *group, const float *rotation, const float *shift, uint32_t n_transforms);
flx_status flx_group_lights_upload(flx_group *group, const float *lights, uint32_t n_lights);
flx_status flx_group_atlas_upload(flx_group *group, int which, const uint8_t *rgba, uint32_t width, uint32_t height);
flx_status flx_group_scene_upload_view(flx_group *group, const flx_scene_view *scene);
/* n_frames frames (1 = one frame; a batch like flx_render_batch; a filter frame alone) rendered by all contexts of the group:
 * params[i].tile_* are ignored, strips of tile_rows rows.  out_rgba = float4[n_frames][height][width] on the host, equal to
 * flx_render / flx_render_batch of one context bit for bit.  counters (may be NULL): summed over the contexts. */
flx_status flx_group_render(flx_group *group, const flx_frame_params *params, uint32_t n_frames, uint32_t tile_rows, float *out_rgba,
                            flx_counters *counters);
/* ... as the canvas' RGBA8 (flx_render_gathered_rgba8_device): out_rgba8 = uint8[n_frames][height][width][4] on the host, equal to flx_present of flx_group_render's frames */
flx_status flx_group_render_rgba8(flx_group *group, const flx_frame_params *params, uint32_t n_frames, uint32_t tile_rows, uint8_t *out_rgba8,
                                  flx_counters *counters);
/* The group's frame loop — what the reference's render loop is to its one context (pathtracerWGL2.js:254-303: a frame per animation callback, the host
 * never waits for the GPU).  flx_group_frame_begin posts the frame to every context's frame server (flx_set_frame_chain) and returns; every server renders
 * its context's strips and resolves them straight into ONE image the group owns — pinned host memory that every GPU writes over its own PCIe link
 * (FLX_FRAME_FLOAT; FLX_FRAME_RGBA8: the canvas' bytes, quantised by the servers as they resolve their tiles), or context 0's device memory through the peer mapping
 * (FLX_FRAME_DEVICE) — so a frame needs no exchange, no reassembly and no copy.
 * flx_group_frame_end waits for the oldest frame's completion words (no stream is synchronised) and hands the image out: float4[height][width], valid until
 * `lanes` more frames have been begun; ms: the slowest context's time from the post to its word, on the host's clock.  Up to `lanes` frames (2 or 3,
 * default 3) are in flight; frames complete in order and equal flx_render's bit for bit.  Float frames the server does not take (temporal frames, scenes
 * of <= 128 entries, strips that are no multiple of 8 rows) are begun on every context's two lanes and their strips copied into the image by the matching
 * flx_group_frame_end; filter frames, and the canvas' bytes of frames the server does not take, are rendered as flx_group_render does inside
 * flx_group_frame_begin.  Temporal frames (not FLX_FRAME_DEVICE): every context keeps the history of its own strips (flx_temporal_reset), so a sequence equals
 * the same sequence on one context frame by frame, and with the filter the five render targets after the temporal pass are exchanged and the chain runs on
 * context 0.  The history starts again where it does on one context, and also where tile_rows changes.  flx_group_temporal_reset: flx_temporal_reset on
 * every context. */
flx_status flx_group_frame_begin(flx_group *group, const flx_frame_params *params, uint32_t tile_rows, int format);
flx_status flx_group_frame_end(flx_group *group, const void **pixels, size_t *bytes, float *ms);
int flx_group_frames_in_flight(const flx_group *group);
flx_status flx_group_set_frame_lanes(flx_group *group, int lanes);
flx_status flx_group_temporal_reset(flx_group *group);

/* Anti-aliasing post passes: config.antialiasing = 'fxaa' | 'taa' of the reference (modules/fxaa.js:7-137,
 * modules/taa.js:11-59).  Both read the RGBA8 texture the renderer drew into — the frame is stored as the reference stores it,
 * floor(clamp(x) * 255 + 0.5) — and return the float the shader writes to the canvas, rows top-down like every frame here.
 * TAA keeps the last nine frames in the context (zero textures before that; reset by a change of size or flx_taa_reset); the
 * sub-pixel camera jitter of taa.js:120-127 is the caller's (js/pathtracerHIP.js).  *_device take device pointers and run on the
 * context's stream; the others copy in and out and wait. */
flx_status flx_fxaa_device(flx_context *ctx, uint32_t width, uint32_t height, const void *d_in_rgba, void *d_out_rgba);
flx_status flx_taa_device(flx_context *ctx, uint32_t width, uint32_t height, const void *d_in_rgba, void *d_out_rgba);
flx_status flx_fxaa(flx_context *ctx, uint32_t width, uint32_t height, const float *in_rgba, float *out_rgba);
flx_status flx_taa(flx_context *ctx, uint32_t width, uint32_t height, const float *in_rgba, float *out_rgba);
flx_status flx_taa_reset(flx_context *ctx);
/* 8-bit present: what the RGBA8 drawing buffer of the reference's canvas holds after the last pass wrote
 * `out_color` to it (pathtracerWGL2.js:552-553, gl.bindFramebuffer(null)): floor(clamp(x, 0, 1) * 255 + 0.5) per channel,
 * bytes R G B A, rows top-down.  out_rgba8: width * height * 4 bytes. */
flx_status flx_present_device(flx_context *ctx, uint32_t width, uint32_t height, const void *d_in_rgba, void *d_out_rgba8);
flx_status flx_present(flx_context *ctx, uint32_t width, uint32_t height, const float *in_rgba, uint8_t *out_rgba8);


/* ---- native scene import (host only, needs no GPU and no context) ---------------------------------
 * One imported object: Scene.importMtl + Scene.importObj of the reference (modules/scene.js:330-487) including the
 * generateBVH (:62-154) it ends with, the Object3D operations an application applies to the result (:774-839), and its
 * block of generateArraysFromGraph (:190-316).  The arrays equal what the JavaScript host layer produces for the same
 * object, bit for bit; a scene's flattening splices the block in (skip counts are relative, ids are entry indices
 * relative to the block's first entry). */
typedef struct flx_mesh flx_mesh;
flx_status flx_mesh_import_obj(const char *obj_text, size_t obj_len, const char *mtl_text /* or NULL */, size_t mtl_len, flx_mesh **out);
void flx_mesh_destroy(flx_mesh *mesh);
uint32_t flx_mesh_entry_count(const flx_mesh *mesh);          /* AABB nodes + triangles */
uint32_t flx_mesh_triangle_count(const flx_mesh *mesh);
flx_status flx_mesh_set_transform(flx_mesh *mesh, uint32_t transform_number);
flx_status flx_mesh_move(flx_mesh *mesh, double x, double y, double z);
flx_status flx_mesh_scale(flx_mesh *mesh, double s);
#define FLX_MESH_COLOR 0          /* 3 values, 0..255 */
#define FLX_MESH_ROUGHNESS 1
#define FLX_MESH_METALLICITY 2
#define FLX_MESH_EMISSIVENESS 3
#define FLX_MESH_TRANSLUCENCY 4
#define FLX_MESH_IOR 5
#define FLX_MESH_TEXTURE_NUMS 6   /* 3 values: albedo, pbr, translucency texture numbers (-1 = none) */
flx_status flx_mesh_set_material(flx_mesh *mesh, int field, const double *values);
/* Scene.updateBoundings of the object (scene.js:157-187): [xmin, xmax, ymin, ymax, zmin, zmax], nodes widened by 100 * 2^-16 */
flx_status flx_mesh_bounding(flx_mesh *mesh, double box[6]);
/* geometry: 12 floats per entry, attributes: 28 floats per entry, ids: one entry index per triangle, minmax: the block's box */
flx_status flx_mesh_flatten(const flx_mesh *mesh, float *geometry, float *attributes, int32_t *ids, float minmax[6]);

/* the per-frame transform arrays in native code — Transform.buildWGL2Arrays (scene.js:500-521) with the
 * reference's Moore-Penrose inverse (math.js:56-101).  matrices: 9 doubles per transform, row major, = scale x rotation;
 * positions: 3 per transform; out: rotation 24 floats and shift 8 floats per transform, ready for flx_transforms_upload. */
flx_status flx_transforms_pack(uint32_t n_transforms, const double *matrices, const double *positions, float *rotation, float *shift);

/* Device name / CU count of the context's GPU. */
flx_status flx_device_info(flx_context *ctx, char *name, uint32_t name_len, uint32_t *compute_units);
const char *flx_version(void);

/* Work counters, kernel-organisation knobs for A/B runs, fault injection, device-side evaluators of single routines and the launch diagnostics are NOT part of
 * this boundary: include/flexlight_hip_debug.h (same library, same ABI rules; used by tests/, tools/ and bench.py). */

#ifdef __cplusplus
}
#endif
#endif /* FLEXLIGHT_HIP_H */
