/* flx_context.h — the context behind the C ABI and the internal helpers flx_api.hip shares with flx_scene.hip and flx_group.hip (the
 * RCCL gather across contexts).  Private to the library. */
#ifndef FLX_CONTEXT_H
#define FLX_CONTEXT_H

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <string>
#include <vector>

#include "flexlight_hip.h"
#include "flexlight_hip_debug.h"
#include "flx_kernels.h"
#include "flx_ray_temporal_args.h"
#include "flx_server.h"

struct flx_share;                                 /* flx_share.hip: this context's part in the ranks' shared frames */
typedef struct ncclComm *flx_nccl_comm;          /* = ncclComm_t (rccl.h), kept out of this header */

#ifndef FLX_WF_GROUPS
#define FLX_WF_GROUPS 1      /* measured on MI355X: 2-4 concurrent chains are slower than one (profiles/r01_ab_stream_groups.txt) */
#endif
constexpr int WF_MAX_GROUPS = 4;
#ifndef FLX_SAMPLE_PARALLEL_DEFAULT
#define FLX_SAMPLE_PARALLEL_DEFAULT 1
#endif
#ifndef FLX_FRAME_CHAIN_DEFAULT
#define FLX_FRAME_CHAIN_DEFAULT 2      /* flx_set_frame_chain's default: the frame server where a frame is a rank's thin share */
#endif
constexpr int FLX_COUNTER_SLOTS = 80;          /* 8 work counters + 32 scheduler diagnostics (flx_get_diag) + 40 tail profile (flx_get_tail_diag) */

extern thread_local std::string g_create_error;

struct flx_context;

/* The memory of a context (and of a debug hook's call): `capacity()` elements of T in device memory or, Pinned, in page-locked host memory.  It owns what it
 * allocated and frees it when it goes; it moves and is not copied.  The one exception is a view made by borrow(): the frame loop's second lane reads the first
 * lane's static scene arrays through such views and never frees them.  It converts to T *, so launches and copies take it as they took the pointer. */
template <typename T, bool Pinned = false> struct Buffer {
  Buffer() = default;
  Buffer(Buffer &&o) noexcept : p(o.p), n(o.n), owned(o.owned) { o.p = nullptr; o.n = 0; o.owned = true; }
  Buffer &operator=(Buffer &&o) noexcept {
    if (this != &o) { (void)hip_free(); p = o.p; n = o.n; owned = o.owned; o.p = nullptr; o.n = 0; o.owned = true; }
    return *this;
  }
  ~Buffer() { (void)hip_free(); }
  operator T *() const { return p; }
  T *get() const { return p; }
  T *operator->() const { return p; }
  size_t capacity() const { return n; }
  bool fits(size_t count) const { return p && n >= count; }
  /* Room for `count` elements (for one where count is 0, so that there is a pointer to hand on): kept when it fits(); else freed FIRST and then allocated — a frame
   * that grows does not hold both sizes at once.  A failure sets ctx->err like FLX_HIP and leaves the buffer empty: no stale capacity over freed memory.  Neither
   * waits for the work in flight on purpose: who must, does so before the call.  pinned_flags: hipHostMalloc's. */
  flx_status ensure(flx_context *ctx, size_t count, unsigned pinned_flags = 0);
  flx_status release(flx_context *ctx);      /* empty from here on (also where the free fails) */
  void borrow(const Buffer &o) { (void)hip_free(); p = o.p; n = o.n; owned = false; }
 private:
  T *p = nullptr;
  size_t n = 0;
  bool owned = true;
  hipError_t hip_free() {
    T *mine = owned ? p : nullptr;
    p = nullptr; n = 0; owned = true;
    return !mine ? hipSuccess : Pinned ? hipHostFree(mine) : hipFree(mine);
  }
};
template <typename T> using DeviceBuffer = Buffer<T, false>;
template <typename T> using PinnedBuffer = Buffer<T, true>;

struct flx_context {
  int device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  std::string err;
  hipDeviceProp_t prop;
  /* resident scene */
  DeviceBuffer<float4> d_geometry, d_attributes, d_rotation, d_shift;      /* (a twin: geometry, attributes, ids, walk, fwd and the atlases are views of the primary's: mirror_scene) */
  DeviceBuffer<float4> d_walk;                     /* threaded hot-first copy of the skip list */
  uint32_t walk_entries = 0, walk_hot = 0, walk_root = 0, walk_fast_boxes = 0;
  uint32_t walk_thick_boxes = 0;                   /* every box of the scene is known to have min < max on all three axes (DeviceScene::walk_thick_boxes: a hint of speed alone) */
  int box_test = -1;                               /* flx_debug_set_box_test: the frame kernels' box test, -1 by walk_thick_boxes, 0 the cross-pair form, 1 the single comparison */
  DeviceBuffer<float4> d_fwd;                      /* the live entries in the reference's order (every successor further on): primary walk, lockstep walk */
  uint32_t fwd_entries = 0, fwd_root = 0, lock_boxes = 0;
  int last_organisation = 0;                     /* flx_last_organisation: what launch_wavefront ran for the last frame (0: another pipeline) */
  flx::WalkLdsLaunch last_walk_lds;                /* flx_debug_last_walk_lds: what the last wavefront or server launch staged of the tree's top (zeros: none since the scene upload) */
  int frame_front = 1;                           /* flx_set_frame_front: the frame kernel traces the primary rays and shades bounce 0 itself (0 two kernels in front, 1 automatic, 2 inside wherever the frame kernel runs, 3 one kernel in front) */
  DeviceBuffer<uint32_t> d_frame_rings;            /* k_wf_frame: per chain and workgroup three rings of WF_FRAME_RING path ids */
  int frame_rings_chains = 0;                    /* chains it has slices for */
  int wf_organisation = 0;                       /* wavefront pipeline: 0 automatic, 1 rounds, 2 frame kernel (flx_set_wavefront_organisation) */
  bool lock_ok = false;                          /* the scene is small and in one object space: its bounce walks may go in lockstep */
  bool lock_use = true;                          /* flx_set_lockstep */
  bool gb_float_wanted = false;                  /* flx_render was given `gbuffers`: the filter frame keeps its float G-buffers */
  int sample_parallel = FLX_SAMPLE_PARALLEL_DEFAULT;      /* flx_debug_set_sample_parallel: k_trace_samples instead of k_trace_pixels where the frame allows it */
  /* Adaptive tile order (flx_debug_set_adaptive_order; on by default): k_resolve sums what every screen tile's paths cost (time in walk lanes), k_tile_order makes the
   * next frame's draw order of it — the lightest tiles last, so that the launch does not end in the chains of a heavy tile's paths.  Frames do not depend on the order. */
  int adaptive_order = 1;
  DeviceBuffer<float> d_tile_time; DeviceBuffer<uint32_t> d_auto_order;
  uint32_t auto_order_tiles = 0, auto_order_width = 0, auto_order_rows = 0; int auto_order_mode = -1;      /* the frame shape d_auto_order is for (0 tiles: none yet) */
  DeviceBuffer<uint32_t> d_tile_order; uint32_t tile_order_n = 0;      /* flx_debug_set_tile_order: the frame kernel's draw order over the tile_order_n screen tiles of a frame (used for frames of as many) */
  DeviceBuffer<unsigned long long> d_tile_cost;      /* flx_debug_tile_cost: counted frames' visits per screen tile, for frames of up to capacity() tiles */
  DeviceBuffer<int32_t> d_ids;
  DeviceBuffer<float> d_lights;
  DeviceBuffer<uchar4> d_atlas[3];
  uint32_t atlas_w[3] = { 0, 0, 0 }, atlas_h[3] = { 0, 0, 0 };
  /* flx_textures_upload / flx_texture_update (flx_atlas.hip).  atlas_cells: what the resident atlas was built with (n 0: none, or a prebuilt one: no cell updates).
   * d_texture_table: the build's table of sources, filled through the staging ring.  d_texture_src: the host variants' sources, staged; nothing in flight reads it
   * when a call returns.  d_texture_cell: an update's resampled cell, read on the context's stream behind its frames: update_done guards it like the row stage. */
  struct { uint32_t w = 0, h = 0, n = 0; } atlas_cells[3];
  DeviceBuffer<flx::AtlasSource> d_texture_table;
  DeviceBuffer<uint4> d_texture_src;
  DeviceBuffer<uint32_t> d_texture_cell;
  uint32_t n_entries = 0, n_ids = 0, n_transforms = 0, n_lights = 0;
  uint32_t max_transform = 0;                   /* largest transform number an entry names */
  bool have_scene = false, have_transforms = false, have_lights = false;
  /* flx_scene_update (rows of the uploaded scene replaced, the boxes refitted on the device: flx_refit.hip).  What the host must know of the scene to check the rows it
   * is given without reading the device: the bits of words 6, 9 and 10 of every entry, kept at flx_scene_upload; whether a triangle of the upload had a NaN vertex
   * (the refit's min / max would not carry it into the boxes as Math.min does: such a scene takes no updates).  The rows go through pinned memory of the context's
   * into d_update_rows, from where a kernel scatters them (update_done: that kernel, and with it whatever last read the stage); d_refit is the refit's workspace.
   * flx_scene_update_device's rows are in device memory already: a kernel on update_stream checks them against d_geometry and copies them into d_update_rows and
   * d_update_attributes; its verdict (d_update_verdict, two words) comes back through h_update_verdict, update_checked follows that copy, update_produced is
   * recorded on the caller's stream.  geometry_uploaded follows flx_scene_upload's copy of the geometry array, which the check reads.  The stream and the four
   * events are made in one place, at the first call that needs one (flx_scene.hip: ensure_side_stream). */
  std::vector<uint32_t> h_entry_meta;
  bool scene_has_nan = false;
  PinnedBuffer<float> h_update;
  hipEvent_t update_done = nullptr;
  bool update_pending = false;
  DeviceBuffer<float4> d_update_rows, d_update_attributes;
  DeviceBuffer<uint32_t> d_update_verdict;
  PinnedBuffer<uint32_t> h_update_verdict;
  hipStream_t update_stream = nullptr;
  hipEvent_t update_checked = nullptr, update_produced = nullptr, geometry_uploaded = nullptr;
  DeviceBuffer<uint32_t> d_refit;
  /* flx_scene_upload_device (flx_derive.hip): its workspace, whose first words are the record of scalars that comes back through h_derive_record.  Such an upload
   * leaves h_entry_meta on the device: entry_meta_stale, and the first flx_scene_update of host rows fetches it (fetch_entry_meta), 12 bytes per entry. */
  DeviceBuffer<uint32_t> d_derive;
  PinnedBuffer<uint32_t> h_derive_record;
  bool entry_meta_stale = false;
  /* flx_tree_build_device (flx_build.hip): the tree of the last successful build — the permutation, the nodes, the entry indices — which flx_tree_emit_device writes
   * out; the arrays per triangle, the arrays per node (node_capacity of them: grown by doubling), the refit's workspace for the emitted block.  All of it is used
   * on update_stream alone.  h_tree_record: the refusals' verdict and, level by level, the number of children. */
  struct {
    DeviceBuffer<float2> tbox; DeviceBuffer<uint32_t> perm[2], owner[2], open, bucket, entry, keys, verdict, refit; DeviceBuffer<uint2> x, y, totals;
    DeviceBuffer<uint4> node, cnt; DeviceBuffer<double> centre;
    size_t node_capacity = 0;
    uint32_t n_triangles = 0, n_nodes = 0; int current = 0; float transform = 0.0f; bool valid = false;
  } tree;
  PinnedBuffer<uint32_t> h_tree_record;
  /* DeviceScene::angle_tan: per triangle, from the geometry / attribute arrays and this context's transforms; made again (on this context's stream, in front of
   * the frame that needs it) when any of them changed: angle_key = the versions it was made from */
  DeviceBuffer<float4> d_angle_tan;
  uint64_t angle_key = ~0ull;
  uint32_t geometry_version = 0;                 /* counts uploads of the geometry / attribute arrays (the second lane copies the primary's: mirror_scene) */
  uint32_t transforms_version = 0;               /* counts uploads of this context's transforms */
  int angle_table = 1;                           /* flx_debug: 0 = the shading computes the values itself */
  /* WavefrontBuffers::cosSample: cos((float)s) of the first WF_COS_SAMPLES sample numbers, made once on this context's stream in front of the first launch that reads it */
  DeviceBuffer<float> d_cos_sample;
  bool cos_sample_made = false;
  /* frame workspace */
  DeviceBuffer<float4> d_out;
  DeviceBuffer<float4> d_gb[6];
  DeviceBuffer<uint32_t> d_planes[13];                /* the filter chain's RGBA8 render targets */
  DeviceBuffer<uint32_t> d_qbatch;               /* batches of filter frames: the five render targets of every frame, 5 x pixels */
  /* temporal history: rings of RGBA8 planes (colour, colour ip, location id, original id), newest at ring_head, of the rows this
   * context traces (packed strips of a tiled frame): for frames of ring_n slots, ring_w x ring_h and the (normalised) tile policy ring_tile_* */
  DeviceBuffer<uint32_t> d_ring[4][16];
  int ring_n = 0, ring_head = 0;
  uint32_t ring_w = 0, ring_h = 0;
  uint32_t ring_tile_rows = 0, ring_tile_index = 0, ring_tile_count = 0;
  /* v2 pipeline workspace: primary hits, per-(sample,pixel) radiance, last sample's originalColor, item queue */
  DeviceBuffer<float4> d_hits, d_samples, d_last;
  DeviceBuffer<uint32_t> d_queue;
  /* pipeline 3 (wavefront) workspace */
  DeviceBuffer<float4> d_rec;                      /* 8 float4 per path */
  DeviceBuffer<float4> d_tail_pool;               /* per walk workgroup: WF_TAIL_POOL_F4 float4 */
  DeviceBuffer<uint32_t> d_aa[10];                 /* RGBA8 planes of the anti-aliasing passes: [0..8] the TAA ring, [9] FXAA's input */
  uint32_t aa_w = 0, aa_h = 0;
  int taa_head = 0, taa_filled = 0;
  DeviceBuffer<float4> d_aa_io[2];                /* staging for the host-pointer variants */
  DeviceBuffer<float4> d_rec0, d_pix0;           /* compact bounce-0 records: 3 float4 per path, 3 float4 per pixel */
  DeviceBuffer<uint32_t> d_live[2];              /* (both of one size) */
  DeviceBuffer<uint32_t> d_wfcounts;               /* per chain: counts, walkQueue, [WF_MAX_BOUNCES + 2] each */
  int pipeline = 0;                              /* 0 auto, 1 per-pixel megakernel, 2 persistent paths, 3 wavefront */
  int last_pipeline = 0;                         /* what the last frame ran */
  flx::TraceKernel last_trace = { -1, -1, -1 };     /* ... and which per-pixel kernel, where that was pipeline 1 (all -1 otherwise) */
  int wf_groups = FLX_WF_GROUPS;                 /* wavefront pipeline: independent item groups on separate streams (tails of one overlap the other) */
  hipStream_t aux_stream[3] = { nullptr, nullptr, nullptr };
  hipEvent_t ev_fork = nullptr, ev_join[3] = { nullptr, nullptr, nullptr };
  /* device error word: pinned, device-mapped; a frame kernel's watchdog that trips sets WF_ERR_* bits in it and the host returns FLX_ERR_DEVICE where it next waits */
  PinnedBuffer<uint32_t> h_dev_error; uint32_t *d_dev_error = nullptr;      /* (its device address) */
  uint32_t inject_watchdog = 0, inject_flags = 0; /* flx_debug_inject_fault */
  DeviceBuffer<unsigned long long> d_counters;
  bool counters_enabled = false;
  flx_counters last_counters = {};
  hipEvent_t ev_frame0 = nullptr, ev_frame1 = nullptr, ev_k0 = nullptr, ev_k1 = nullptr;
  bool timed = false;
  /* several GPUs (flx_group.hip): this context's RCCL communicator and the buffers of the gather */
  flx_nccl_comm comm = nullptr;
  flx_nccl_comm comm_twin = nullptr;             /* a second communicator over the same ranks (ncclCommSplit) for the frame loop's second lane */
  int last_gather_root = -1;                     /* how the last gathered frame was exchanged: -1 all-gather, else the receiving rank */
  int comm_rank = 0, comm_size = 1;
  bool comm_owned = false;                       /* made by flx_comm_init_rank (else by a group's ncclCommInitAll) */
  DeviceBuffer<float4> d_send, d_recv;           /* this rank's packed strips; every rank's */
  DeviceBuffer<float4> d_send8;                  /* this rank's strips as RGBA8 texels (flx_render_gathered_rgba8_device), counted in float4 */
  DeviceBuffer<float4> d_frames;                 /* group mode: the gathered frames in image order */
  DeviceBuffer<float4> d_gplanes;                /* filter frames: the five gathered render targets in image order, counted in float4 */
  /* the frame loop (flx_frame_begin / flx_frame_end): two slots of device output + pinned host memory, a copy stream */
  /* (three slots where flx_set_frame_lanes(3) lets three chained frames be in flight, two otherwise) */
  DeviceBuffer<float4> d_slot[3];
  DeviceBuffer<uint32_t> d_slot8[3];
  PinnedBuffer<uint8_t> h_slot[3];               /* bytes */
  size_t slot_bytes[3] = { 0, 0, 0 };
  hipStream_t copy_stream = nullptr;
  hipEvent_t ev_slot_start[3] = {}, ev_slot_traced[3] = {}, ev_slot_done[3] = {};
  uint64_t frames_begun = 0, frames_ended = 0;
  bool slot_host[3] = { true, true, true };      /* the slot's frame is copied to pinned host memory (else it stays in d_slot) */
  /* two lanes: a twin context (own stream + workspace, shared static scene arrays) takes every other frame of the loop */
  flx_context *twin = nullptr;
  bool is_twin = false;
  int frame_lanes = 2;
  uint64_t lane_next = 0;
  struct { flx_context *lane; int slot; } fifo[3] = {};
  int fifo_n = 0;
  std::vector<float> h_lights, h_rotation, h_shift;      /* host copies of what changes per frame, for the twin's own buffers */
  uint64_t dyn_version = 0, twin_dyn_version = 0;
  int frame_chain = FLX_FRAME_CHAIN_DEFAULT;     /* flx_set_frame_chain: 0 never, 2 the frame server for a rank's thin share, 3 for every frame it can take */
  uint64_t scene_version = 0;                    /* bumped by every upload */
  uint64_t begin_scene_version = 0;              /* ... as the last flx_frame_begin found it (0: no frame begun yet) */
  int last_chained = 0;                          /* flx_last_chained: 0 the last frame of the loop was not chained, 3 the frame server took it */
  /* the frame server (flx_server.hip): one persistent launch renders the loop's frames as they are posted (flx_set_frame_chain mode 2) */
  DeviceBuffer<flx::ServerSlot> d_sv_slots;
  PinnedBuffer<flx::ServerMail> h_sv_mail; flx::ServerMail *d_sv_mail = nullptr;      /* pinned host memory and its device address */
  DeviceBuffer<flx::ServerMail> d_sv_relay;
  DeviceBuffer<uint32_t> d_sv_rings;
  DeviceBuffer<float4> d_sv_out;                 /* the launch's resolved frames: [slot] x sv_out_pixels */
  size_t sv_out_pixels = 0;
  DeviceBuffer<uint32_t> d_sv_tiles;              /* [workgroup][slot] x sv_tile_cap: the screen tiles a workgroup made of a frame */
  size_t sv_tile_cap = 0;                        /* ... the length of one such list, as the launch is told it */
  float slot_latency_ms[3] = { -1.f, -1.f, -1.f }; /* server frames: post .. complete on the host's clock (flx_frame_end's gpu_ms); < 0: timed by events */
  const void *slot_dev_ptr[3] = { nullptr, nullptr, nullptr };      /* where the frame of an output slot really is in device memory when that is not d_slot[k] (server frames) */
  DeviceBuffer<unsigned long long> d_sv_stats;
  hipStream_t sv_stream = nullptr;
  bool sv_running = false;
  uint32_t sv_depth = 0, sv_next_seq = 0, sv_next_slot = 0, sv_counter = 0;
  flx_frame_params sv_params = {};               /* the shape of the frames the running launch takes */
  uint64_t sv_scene_version = 0;
  /* A scene that MOVES (changed lights / transforms of the same counts, frame after frame): the launch takes those arrays with every frame (ServerMail::blob) and
   * goes on over their uploads. */
  uint64_t structure_version = 0;                /* bumped by every upload but those (scene_version counts them all) */
  uint64_t sv_structure_version = 0;
  bool sv_ver = false;                           /* the running launch takes the lights and transforms per frame */
  uint32_t dyn_device_stale = 0;                 /* bit 0 / 1: d_rotation + d_shift / d_lights are behind h_rotation .. (uploads the launch went on over): dyn_flush */
  bool sv_want_ver = false;                      /* the scene has moved since it was uploaded: the next launch does */
  int sv_moving = 1;                             /* flx_set_server_moving_scenes: 0 = never (every changed upload ends the launch, as before round 4) */
  DeviceBuffer<uint32_t> d_sv_versions;          /* [3 arrays][workgroup x depth + slot]: the launch's versions of rotation / shift / lights */
  bool sv_out8 = false;                          /* the running launch resolves RGBA8 (ServerArgs::out8) */
  bool sv_target8 = false;                       /* flx_frame_target_set8: the target images are uint32 RGBA8 per pixel */
  float4 *sv_target[3] = { nullptr, nullptr, nullptr };      /* flx_frame_target_set: whole images the launch resolves this context's strips into (a peer GPU's memory, pinned host memory, ..) */
  uint64_t sv_target_posted = 0;                 /* frames posted since flx_frame_target_set: frame g goes to image g % n, whatever launch takes it */
  uint32_t sv_target_slots = 0;                  /* 0: none — the launch's own d_sv_out */
  flx_share *share = nullptr;
  uint32_t sv_groups = 0;                        /* flx_debug_set_server_groups: workgroups of the launch (0: one per CU) — two launches beside each other on one GPU, to rehearse a device group */
  struct { bool valid; uint32_t seq, slot; int format; flx::DeviceFrame fr; std::chrono::steady_clock::time_point posted; } sv_pending[3] = {};      /* per output slot: the server frame that will land there */
  /* ray queries (flx_query.hip): the host call's staging, grown and never shrunk; the launch's two device words (the chunk cursor, the waves that drew a chunk);
   * what the last launch since the scene upload was (flx_debug_last_query) */
  DeviceBuffer<float4> d_query_rays, d_query_hits;
  DeviceBuffer<uint32_t> d_query_ctl;
  hipEvent_t query_produced = nullptr;            /* recorded on the caller's producer_stream, waited for by the context's */
  flx::QueryLaunch last_query;
  uint32_t query_groups = 0;                     /* flx_debug_set_query_groups: workgroups of the query launch (0: its own choice) */
  /* traced ray batches (flx_rays_trace.hip): the scratch of a slab of rays, grown and never shrunk — the first hits' rows, a slot per (sample, ray), the last
   * sample's originalColor per ray —, the four words of a slab's launches, what the last batch ran (flx_debug_last_trace) */
  DeviceBuffer<float4> d_trace_hits, d_trace_slots, d_trace_last;
  DeviceBuffer<uint32_t> d_trace_ctl;
  struct TraceLaunch { uint32_t slabs = 0, slab = 0, path_groups = 0, lock = 0, n = 0, samples = 0, query_groups = 0; } last_trace_rays;
  uint32_t trace_slab = 0;                       /* flx_debug_set_trace_slab: most rays of a slab (0: flx_trace_slab_rays' own ceiling) */
  /* traced batches in first-hit order (flx_rays_order.hip): the sort's scratch for a slab of rays, grown with the trace's scratch and never shrunk — two key and two
   * position buffers (a pass reads one pair and writes the other; the order ends in d_order_pos[0]), the digit-major count table of one pass, and sixteen control words:
   * [0..2] the least hit point per axis and [3..5] the greatest, as flx_ray_key_map's integers, [6] the slab's live rays, [7] unused, [8..15] the same for flx_debug_hit_keys —; what the last traced batch did
   * (flx_debug_last_ray_order) */
  DeviceBuffer<uint32_t> d_order_keys[2], d_order_pos[2], d_order_counts, d_order_ctl;
  struct OrderLaunch { uint32_t ordered = 0, groups = 0, passes = 0, n = 0; } last_ray_order;
  /* surface rows (flx_surface.hip): their hit scratch is the traced batches' above, their host variants' staging the queries'; what the last call ran
   * (flx_debug_last_surface) */
  struct SurfaceLaunch { uint32_t slabs = 0, slab = 0, n = 0, fields = 0, frame = 0, query_groups = 0; } last_surface;
  /* filter planes of ray batches (flx_rays_planes.hip): their hit scratch is the traced batches' too; the five RGBA8 planes of a ray image (and the host
   * variant's byte planes), grown and never shrunk; what the last call ran (flx_debug_last_ray_planes) */
  DeviceBuffer<uint32_t> d_ray_planes;
  struct RayPlanesLaunch { uint32_t slabs = 0, slab = 0, groups = 0, lock = 0, n = 0, samples = 0, query_groups = 0; } last_ray_planes;
  /* ray images over time (flx_rays_image_temporal[_device]): FLX_RAY_HISTORIES histories, each four rings (colour, colour ip, location id, original id: d_ring's)
   * of at.n RGBA8 planes of at.width * at.height texels back to back in one allocation, slot s of ring j at texel (j * at.n + s) * width * height, the newest at slot
   * at.head; allocated on first use, released by flx_rays_history_reset.  at.n == 0: no history.  The frames' ring above and these never touch each other.  What the last call ran (flx_debug_last_ray_temporal) */
  struct RayHistory { DeviceBuffer<uint32_t> rings; flx_ray_history_state at = { 0u, 0u, 0, 0 }; } ray_history[FLX_RAY_TEMPORAL_HISTORIES];
  struct RayTemporalLaunch { uint32_t slabs = 0, slab = 0, depth = 0, history = 0, n = 0, samples = 0, head = 0, fused = 0; } last_ray_temporal;
  /* cameras (flx_camera.hip): the rays flx_camera_image[_temporal]_device makes for the image calls that follow on the same stream, grown and never shrunk */
  DeviceBuffer<float4> d_camera_rays;
  /* light probes (flx_probes.hip): the rays and the radiance rows of one chunk of probes, which flx_probes_sh_device makes, traces and reduces on the same stream —
   * at most 2^21 rays x 32 bytes each —, and the host variants' positions; all grown and never shrunk.  What the last flx_probes_sh[_device] ran
   * (flx_debug_last_probes) */
  DeviceBuffer<float4> d_probe_rays, d_probe_radiance, d_probe_positions;
  struct ProbeLaunch { uint32_t chunks = 0, chunk = 0, face_size = 0, n = 0, order = 0, rays = 0, reduce_groups = 0; } last_probes;
  uint32_t probe_chunk = 0;                      /* flx_debug_set_probe_chunk: most probes of a chunk (0: as many as a trace slab's 2^21 rays hold) */
  /* probe volumes (flx_volume.hip): the grid's positions flx_volume_bake_device makes for flx_probes_sh_device; the position plane and the normal plane of a slab
   * of rays (at most 2^21 x 32 bytes) or of a frame, which flx_rays_irradiance_device and flx_frame_irradiance_device take for the lookup behind them; the host
   * variants' SH rows; all grown and never shrunk.  What the last lookup ran (flx_debug_last_volume) */
  DeviceBuffer<float4> d_volume_positions, d_volume_surface, d_volume_sh;
  struct VolumeLaunch { uint32_t n = 0, slabs = 0, slab = 0, probes = 0, flags = 0, source = 0, groups = 0; } last_volume;
  /* directional visibility (flx_volume_map.hip): the host variants' map rows, going up or coming down; grown and never shrunk.  What the last map reduction ran
   * (flx_debug_last_volume_map) */
  DeviceBuffer<float4> d_volume_maps;
  struct VolumeMapLaunch { uint32_t probes = 0, size = 0, sharpness = 0, launches = 0, groups = 0, face_size = 0; } last_volume_map;
  /* volume updates (flx_volume_update.hip): the listed probes' positions, their new SH rows and their new map rows, which flx_volume_update_device makes, bakes and
   * blends on the same stream (the host blend's new rows go up into the latter two); the host variants' list and states; all grown behind flx_grow's one wait and
   * never shrunk.  What the last blend or update ran (flx_debug_last_volume_update) */
  DeviceBuffer<float4> d_update_positions, d_update_sh, d_update_maps;
  DeviceBuffer<uint32_t> d_update_indices, d_update_state;
  struct VolumeUpdateLaunch { uint32_t entries = 0, groups = 0, size = 0, listed = 0, chunks = 0, fused = 0; } last_volume_update;
  /* probe relocation (flx_volume_relocate.hip): the positions of one chunk of probes and the HIT plane and the NORMAL plane of their rays (at most 2^21 x 32
   * bytes), which flx_volume_relocate_device makes, casts and reduces on the same stream — the rays themselves are d_probe_rays above —; the host variants' offset
   * rows; all grown behind flx_grow's one wait and never shrunk.  What the last reduction or relocation ran (flx_debug_last_volume_relocate) */
  DeviceBuffer<float4> d_relocate_positions, d_relocate_planes, d_relocate_offsets;
  struct VolumeRelocateLaunch { uint32_t probes = 0, face_size = 0, chunks = 0, chunk = 0, groups = 0, flags = 0, first = 0, fused = 0; } last_volume_relocate;
  /* ray batches with a volume (flx_rays_gather.hip): the path records of a slab, four float4 a (ray, sample) as planes, grown with the traced batches' scratch above
   * — which a slab of these uses too — behind flx_grow's one wait and never shrunk.  What the last batch ran (flx_debug_last_gather) */
  DeviceBuffer<float4> d_gather_records;
  struct GatherLaunch { uint32_t n = 0, slabs = 0, slab = 0, path_groups = 0, lookup_groups = 0, flags = 0, order = 0; } last_gather;
  /* ray images with a volume (flx_rays_planes_gather.hip): no buffer of their own — the scratch is the planes calls' hit rows.  What the last launch ran, and the
   * last call that succeeded as a whole (flx_debug_last_planes_gather) */
  struct PlanesGatherLaunch { uint32_t n = 0, slabs = 0, slab = 0, groups = 0, flags = 0, mode = 0, samples = 0, lock = 0; } planes_gather_launch, last_planes_gather;
  /* uploads: pinned staging ring */
  PinnedBuffer<uint8_t> stage;
  hipEvent_t stage_done[8] = {};
  bool stage_used[8] = {};
  int stage_next = 0;
};

#define FLX_HIP(ctx, expr)                                                                    \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                          \
      return FLX_ERR_DEVICE;                                                                  \
    }                                                                                         \
  } while (0)

flx_status flx_fail(flx_context *ctx, flx_status code, const char *msg);

template <typename T, bool Pinned> flx_status Buffer<T, Pinned>::release(flx_context *ctx) {
  FLX_HIP(ctx, hip_free());
  return FLX_OK;
}
template <typename T, bool Pinned> flx_status Buffer<T, Pinned>::ensure(flx_context *ctx, size_t count, unsigned pinned_flags) {
  if (fits(count)) return FLX_OK;
  FLX_HIP(ctx, hip_free());
  const size_t elements = count ? count : 1;
  void *q = nullptr;
  FLX_HIP(ctx, Pinned ? hipHostMalloc(&q, elements * sizeof(T), pinned_flags) : hipMalloc(&q, elements * sizeof(T)));
  p = (T *)q; n = elements;
  return FLX_OK;
}


/* flx_group.hip: this context's strips traced, exchanged over its communicator (root < 0: all-gather; else only `root` receives) and
 * put in image order, all enqueued on its stream */
flx_status flx_gather_enqueue(flx_context *ctx, const flx_frame_params *params, uint32_t n_frames, int root, void *d_frames, bool rgba8 = false);

/* flx_api.hip */
flx_status flx_make_frame(flx_context *ctx, const flx_frame_params *p, flx::DeviceScene &sc, flx::DeviceFrame &fr);
flx_status flx_make_scene(flx_context *ctx, flx::DeviceScene &sc);      /* the scene alone, for a call that renders no frame */
flx_status flx_angle_table(flx_context *ctx, flx::DeviceScene &sc);     /* sc.angle_tan <- the context's per-triangle table, made again first (on its stream) where the scene or its transforms changed */
flx_status flx_make_batch(flx_context *ctx, const flx_frame_params *params, uint32_t n_frames, flx::DeviceScene &sc, flx::DeviceFrame &fr);
flx_status flx_run_frame(flx_context *ctx, const flx::DeviceScene &sc, const flx::DeviceFrame &fr, float4 *d_out, const flx::GBufferPtrs &gb);
int flx_server_takes_moving_scene(const flx_context *ctx);                       /* the scene has moved and its lights and transforms fit a post: the server's launches take them per frame */
int flx_server_continues(flx_context *ctx, const flx_frame_params *params);      /* the running launch of the frame server takes this frame as it is */
flx_status flx_server_prepare(flx_context *ctx, const flx_frame_params *params); /* the launch ends; everything a launch for frames like this needs is allocated */
flx_status flx_server_stop(flx_context *ctx);      /* the frame server's launch ends (after the frames posted to it), the frames in flight are resolved into their output slots */
bool flx_rows_on_device(const flx_context *ctx, const void *p, size_t bytes);      /* flx_scene.hip: [p, p + bytes) is memory of the context's device, 16-byte aligned, inside one allocation */
bool flx_words_on_device(const flx_context *ctx, const void *p, size_t bytes);     /* flx_scene.hip: the same for an array of 4-byte words: 4-byte aligned */
flx_status flx_volume_grid_refused(flx_context *ctx, const flx_volume_grid *grid, uint32_t *probes, const char *call);      /* flx_volume.hip: a grid's refusals in words; *probes <- nx ny nz of an accepted one */
/* flx_volume_update.hip: everything flx_volume_update_device refuses, under the caller's name (n_list == 0: FLX_OK before the arrays); the update and the list alone */
flx_status flx_volume_update_args_refused(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, const flx_volume_map *map,
                                          const struct flx_volume_update *update, const void *d_indices, uint32_t n_list, void *d_sh, void *d_maps, void *d_state, uint32_t *probes,
                                          uint32_t *new_rows, const char *call);
flx_status flx_volume_update_list_refused(flx_context *ctx, const struct flx_volume_update *update, bool has_list, uint32_t n_list, uint32_t probes, const char *call);
flx_status flx_volume_offsets_refused(flx_context *ctx, const void *d_offsets, uint32_t probes, const void *const *others, const uint64_t *other_bytes, int k, const char *call);      /* flx_volume_relocate.hip: the offset rows of a relocated lookup against the call's other arrays */
flx_status flx_dyn_flush(flx_context *ctx);       /* flx_scene.hip: the device's transforms and lights follow the host's copies, where a launch went on over their uploads */
flx_status flx_check_device_error(flx_context *ctx);      /* FLX_ERR_DEVICE (and the word cleared) if a frame kernel's watchdog has tripped since the last check */
/* a temporal filter frame's strips (params->tile_*; use_filter = 1, is_temporal = 1): traced, the temporal pass over this context's history,
 * the five render targets the chain reads stored to d_planes = uint32[5][rows][width] (flx_render_planes_device's layout); enqueued on its stream */
flx_status flx_temporal_planes_enqueue(flx_context *ctx, const flx_frame_params *params, void *d_planes);
/* flx_filter_planes_device; stamp_start = false leaves the frame's start event alone (the trace of the same frame recorded it) */
flx_status flx_filter_planes_enqueue(flx_context *ctx, const flx_frame_params *params, const void *d_planes, void *d_out_rgba, bool stamp_start);
/* flx_query.hip: the host path the ray-batch calls share — cast, trace, surface, planes, images; its templates are flx_rays_host.h's.  `call`: the entry point's
 * name, which every message begins with. */
flx_status flx_scene_refused(flx_context *ctx, const char *call);      /* FLX_ERR_NO_SCENE where no scene and transforms are uploaded */
flx_status flx_trace_params_refused(flx_context *ctx, const flx_trace_params *p, const char *call);      /* that, then a flx_trace_params' refusals (flx_trace_args_check) in words */
/* the frame bounce() is given for a caller's rays: one view, the params' seed and ambient; use_filter makes bounce() keep renderId too */
void flx_trace_frame(const flx_trace_params *p, flx::DeviceFrame &fr, int use_filter, int is_temporal);
flx_status flx_wait_for_producer(flx_context *ctx, void *producer_stream);      /* the context's stream waits for what the caller's stream holds now (NULL: nothing to wait for) */
/* a slab's head: d_trace_ctl's four words zeroed, the closest hits of m rays into d_trace_hits; q <- the launch */
flx_status flx_slab_first_hits(flx_context *ctx, const flx::DeviceScene &sc, const float4 *rays, uint32_t m, const char *call, flx::QueryLaunch &q);
/* flx_surface.hip: what flx_frame_surface[_device] refuses before it looks at its output — the scene, the params, the fields, the frame's shape — in its words */
flx_status flx_frame_surface_refused(flx_context *ctx, const flx_frame_params *p, uint32_t fields, const char *call);
/* flx_rays_order.hip: the words the sort's scratch must hold for a slab of at most `most` rays — keys and positions (each of the two), the count table —, and a slab's
 * order: bounds, keys and the stable sort of m rays against their hit rows, enqueued on the context's stream; the order is d_order_pos[0]; *groups <- the sort's
 * workgroups */
size_t flx_order_room(uint32_t most);
size_t flx_order_table_room(uint32_t most);
flx_status flx_slab_order(flx_context *ctx, const float4 *rays, const float4 *hits, uint32_t m, uint32_t *groups);

#endif
