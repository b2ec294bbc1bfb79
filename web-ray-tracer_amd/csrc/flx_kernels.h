/* flx_kernels.h — host-visible launchers of the HIP kernels (flx_kernels.hip). */
#ifndef FLX_KERNELS_H
#define FLX_KERNELS_H

#include "flx_device.h"

#ifndef FLX_PATHS_ANGLE_TABLE
#define FLX_PATHS_ANGLE_TABLE 1        /* k_paths reads the shading's per-triangle table too (DeviceScene::angle_tan): at the seven waves per SIMD it ran at first the table's dependent load cost it 1 %,
                                        * at four it gains 5 % — theater 9.29 -> 8.80 ms (profiles/r04_paths_occupancy.txt) */
#endif
#ifndef FLX_FRAME_ANGLE_TABLE
#define FLX_FRAME_ANGLE_TABLE 1        /* the frame kernel with the front of the frame inside, unstamped (whole frames: k_wf_frame<., true>), reads the table at bounce 0 and at every later
                                        * shade: its shade waves are the producer its walk waves wait for, and the three acos and three tan in double are a third of a later
                                        * shade's instructions (profiles/shade_needless.txt).  flx_run_frame makes the table in front of such a launch */
#endif
#ifndef FLX_SERVER_ANGLE_TABLE
#define FLX_SERVER_ANGLE_TABLE 1       /* the frame server with a static scene reads it too (flx_frame_begin makes it in front of the launch; any upload ends the launch).  Round 4 lost 9 % on a
                                        * rank's eighth with two frames in flight (profiles/r04_angle_table.txt); with today's trips it gains 8 % there, 1.06 -> 0.975 ms, and nothing
                                        * else moves (profiles/shade_needless.txt).  A scene that moves has transforms per frame slot, which one table cannot follow: it computes */
#endif
#ifndef FLX_THIN_ANGLE_TABLE
#define FLX_THIN_ANGLE_TABLE 0         /* 1, a measuring build: also the stamped frame kernel with the front inside (thin frames: a rank's quarter) reads it.  Not measured: it computes */
#endif
#define FLX_FAST_BOX_BOUND 5.764607523034235e17f      /* 2^59: rayCuboidR's precondition, flx_device.h */
namespace flx {

struct GBufferPtrs {
  float4 *color, *color_ip, *original_color, *id, *original_id, *location_id;
  /* the same five planes as the RGBA8 render targets the filter chain reads (stored as k_quantize would store them), or null */
  uint32_t *q_color = nullptr, *q_color_ip = nullptr, *q_original_color = nullptr, *q_id = nullptr, *q_original_id = nullptr;
};

/* which per-pixel kernel a launch ran (flx_debug_last_trace_kernel): samples = 0 k_trace_pixels, S k_trace_samples<S>; lockstep, counted: its LOCK and COUNT */
struct TraceKernel { int samples, lockstep, counted; };
/* counters: 8 x u64 in flx_counters order, or nullptr (no counting code is compiled in). */
TraceKernel launch_trace_pixels(const DeviceScene &sc, const DeviceFrame &fr, float4 *out, const GBufferPtrs &gb,
                                unsigned long long *counters, hipStream_t stream, int sample_parallel = 0);
/* v2 pipeline: primary hits (float4 s,u,v,triangleId-as-bits per pixel) -> persistent path kernel -> resolve. */
uint32_t path_item_count(const DeviceFrame &fr);
uint64_t path_item_count64(const DeviceFrame &fr);
void launch_primary(const DeviceScene &sc, const DeviceFrame &fr, float4 *hits, unsigned long long *counters, hipStream_t stream);
void launch_paths(const DeviceScene &sc, const DeviceFrame &fr, const float4 *hits, float4 *sampleRadiance, float4 *lastOriginal,
                  uint32_t *queue, uint32_t blocks, unsigned long long *counters, hipStream_t stream);
/* sampleStride: float4 between the planes of two samples (0: the frame's own pixel count; the chained frame loop resolves one slot of a stacked workspace) */
/* tileTime (or nullptr): += what the paths of every 8 x 8 screen tile cost, for launch_tile_order */
void launch_resolve(const DeviceFrame &fr, const float4 *hits, const float4 *sampleRadiance, const float4 *lastOriginal, float4 *out,
                    hipStream_t stream, size_t sampleStride = 0, float *tileTime = nullptr);
/* the frame kernel's draw order over n screen tiles from their cost in the last frame (cleared for the next); mode 0: the lightest tenth last,
 * 1: sixteen classes, heaviest first; screen order inside a class */
void launch_tile_order(float *tileTime, uint32_t *order, uint32_t n, int mode, hipStream_t stream);
/* pipeline 3 (flx_wavefront.hip): per bounce a dense shade kernel and a persistent walk kernel; path state in HBM. */
constexpr int WF_MAX_BOUNCES = 250;
struct WavefrontBuffers {
  float4 *rec;                  /* 8 x float4 (128 B) per path item */
  uint32_t *live[2];            /* live path lists, alternating per bounce */
  uint32_t *counts;             /* [WF_MAX_BOUNCES + 2] slots used in the live list of round r */
  uint32_t *walkQueue;          /* [WF_MAX_BOUNCES + 2] per-round refill cursor of the walk kernel */
  uint32_t item_base, item_count; /* the path items [item_base, item_base + item_count) this group of launches owns */
  const float4 *hits;
  float4 *sampleRadiance, *lastOriginal;
  unsigned long long *counters; /* or nullptr */
  float4 *tailPool;             /* WF_TAIL_POOL_F4 float4 per walk workgroup: scratch of the tail consolidation */
  /* Compact records of bounce 0 (or nullptr: full records).  The samples of a pixel share the primary hit, so what their
   * first shading yields splits into a part per pixel — next origin, shadow origin, albedo, base luminance: pix0, 3 float4,
   * indexed [screen tile][lane] —
   * and a part per sample — next direction + flags, shadow direction + length, lit colour: rec0, 3 float4; importancy is
   * (1,1,1) and the running colour 0 there.  48 B per path instead of a 128-byte line: shade0 writes, and the bounce-0 walk
   * kernel reads, 0.9 GB per 1080p x 8 frame instead of 2.1; the walk kernel's fold writes a full record for the paths
   * that go on (a fifth of them). */
  float4 *rec0, *pix0;
  uint32_t *frameRings;         /* the frame kernel's rings of path ids: WF_FRAME_RINGS x WF_FRAME_RING per walk workgroup (k_wf_frame), or nullptr */
  uint32_t front;               /* frame kernel: 1 = it also traces the primary rays and shades bounce 0 (hits need not be there, item_base must be 0) */
  uint32_t *error;              /* the context's device error word (pinned host memory, WF_ERR_* bits), or nullptr: a watchdog that trips says so here (flx_status FLX_ERR_DEVICE at the next point the host waits) */
  uint32_t watchdog;            /* frame kernels: polls after which a wave that waits gives up (0: FQ_WATCHDOG, seconds); fault injection sets it low */
  uint32_t inject;              /* fault injection (flx_debug_inject_fault): WF_INJECT_* */
  uint32_t stampCosts;          /* frame kernel with its front inside: 1 = the variant whose walk lanes stamp what a path cost (k_wf_frame_stamped: adaptive tile order) */
  uint32_t tileCostPrimary;     /* tileCost (below) has a second half for the primary rays' visits per tile */
  const uint32_t *tileOrder;    /* frame kernel with its front inside: the screen tile the q-th draw from the frame's tile queue makes (a permutation of the frame's tiles), or nullptr: tile q */
  unsigned long long *tileCost; /* counted frames: entries visited by the paths of every screen tile (flx_debug_tile_cost), or nullptr */
  /* cos((float)s) for the sample numbers s < cosSampleCount (k_cos_sample: flx_cos itself, once per context), or nullptr / 0: the shading of the persistent frame kernels
   * reads the value where a shade computed it — 83 vector instructions, 29 of them double precision, for a number that depends on the sample alone.  Samples beyond the
   * count are computed as before.  (At the end: every other member keeps its place in the kernels' arguments.) */
  const float *cosSample = nullptr;
  uint32_t cosSampleCount = 0;
};
/* the arguments of the shade kernels and the frame kernels, read from the kernarg segment where they are used (flx_frame_common.h) */
struct FrameArgs { DeviceScene sc; DeviceFrame fr; WavefrontBuffers wb; };
constexpr uint32_t WF_FRAME_RING = 16384;
/* device error word: who gave up */
constexpr uint32_t WF_ERR_SHADE_WATCHDOG = 1u, WF_ERR_WALK_WATCHDOG = 2u, WF_ERR_LIST = 4u, WF_ERR_LEFTOVER = 8u, WF_ERR_RING_SLOT = 16u, WF_ERR_SERVER_IDLE = 32u, WF_ERR_SERVER_TIMEOUT = 64u;
constexpr uint32_t WF_INJECT_NO_SHADING = 1u;      /* the shade waves of a frame kernel drop what they pop: the paths never come back and the walk waves' watchdog must trip */
constexpr uint32_t WF_FRAME_RINGS = 3;       /* to shade, to walk, fresh (tile, sample) units */
constexpr size_t WF_TAIL_POOL_F4 = 1024 * 8;
size_t wavefront_live_capacity(const DeviceFrame &fr, uint32_t compute_units);
/* organisation: 0 automatic — the whole bounce loop in ONE persistent launch (k_wf_frame: walk waves and shade waves of a workgroup
 * hand paths to each other through LDS rings, no barrier between bounces) where the scene's transforms leave room in LDS, else
 * rounds; 1 = rounds (one k_wf_shade + k_wf_walk_pre pair per bounce); 2 = the frame kernel (rounds if it does not fit). */
bool wavefront_front_in_kernel(const DeviceScene &sc, const DeviceFrame &fr, uint32_t item_count, int organisation);
/* -> what ran: 1 rounds, 2 the frame kernel, 3 the frame kernel with the front of the frame inside it; -1: wb.front set but the frame kernel cannot run; -2: the walk
 * kernels' dynamic LDS limit could not be raised on this device */
/* What a walk launch staged of the tree's top (flx_debug_last_walk_lds): the ldsCount it was given, whether its rays are pre-transformed, and which launch it was
 * (1 rounds, 2 the frame kernel, 3 the frame kernel with the front inside, 4 the frame server) */
struct WalkLdsLaunch { uint32_t ldsCount = 0, pre = 0, kind = 0, nTransforms = 0; int boxTest = -1; };      /* boxTest: the box test compiled into the frame kernel or server kernel launched, 0 cross pairs, 1 single comparison; -1: none of them ran */
int launch_wavefront(const DeviceScene &sc, const DeviceFrame &fr, const WavefrontBuffers &wb, uint32_t compute_units, bool count,
                     int organisation, hipEvent_t walk0_begin, hipEvent_t walk0_end, hipStream_t stream, WalkLdsLaunch *ran = nullptr);
/* denoise chain (flx_filter.hip): 13 RGBA8 planes = the reference's RenderTexture[0..3], IpRenderTexture[0..3],
 * OriginalRenderTexture[0..1], IdRenderTexture[0..1], OriginalIdRenderTexture (pathtracerWGL2.js:224-252). */
struct FilterPlanes { uint32_t *R[4], *Ip[4], *O[2], *Id[2], *OId; };
/* anti-aliasing post passes over RGBA8 planes (modules/fxaa.js, modules/taa.js); taa planes newest first, null = zero texture */
void launch_fxaa(const uint32_t *plane, float4 *out, int W, int H, hipStream_t stream);
void launch_taa(const uint32_t *const planes[9], float4 *out, int W, int H, hipStream_t stream);
/* ... storing the canvas' RGBA8 of what they compute (pack_rgba8: flx_present of the float output) */
void launch_fxaa(const uint32_t *plane, uint32_t *out8, int W, int H, hipStream_t stream);
void launch_taa(const uint32_t *const planes[9], uint32_t *out8, int W, int H, hipStream_t stream);
/* float4 plane -> RGBA8 plane (a render-target store) */
void launch_quantize(const float4 *src, uint32_t *dst, size_t n, hipStream_t stream);
void launch_angle_tan(const DeviceScene &sc, float4 *out, hipStream_t stream);      /* DeviceScene::angle_tan for the scene as it stands */
constexpr uint32_t WF_COS_SAMPLES = 64;      /* sample numbers a context's cosine table holds (WavefrontBuffers::cosSample) */
void launch_cos_sample(float *out, uint32_t n, hipStream_t stream);                 /* out[s] <- flx_cos((float)s), s < n */
/* the chain over planes whose slot 0 (R[0], Ip[0], O[0], Id[0], OId) holds the frame */
void launch_filter_chain(const FilterPlanes &pl, float4 *out, int W, int H, int hdr, hipStream_t stream);
/* temporal accumulation (pathtracerWGL2.js:571-662), one pass after the trace of a temporal frame over its `pixels` in storage order (a whole frame, or a
 * context's packed strips): the float G-buffers of the new frame are stored as the ring-head planes ring_*[0] (RGBA8, k_quantize's bytes) and averaged with
 * the n - 1 older slots ring_*[1 .. n - 1].  Without the filter (dColor null) -> the canvas float4 `out`; with it -> dColor / dIp (RenderTexture[0] /
 * IpRenderTexture[0]) and dOColor / dId / dOId, the other render targets the chain reads. */
struct TemporalPass {
  const float4 *color, *color_ip, *location_id, *original_id, *original_color, *id;
  uint32_t *ring_c[16], *ring_ip[16], *ring_id[16], *ring_oid[16];
  int n, hdr;
  size_t pixels;
  float4 *out;
  uint32_t *dColor, *dIp, *dOColor, *dId, *dOId;
};
void launch_temporal(const TemporalPass &pass, hipStream_t stream);
/* the rasterizer renderer (flx_raster.hip): one frame of k_raster into float4 out[rows][width] (the RGBA8 drawing buffer's values as float32) */
void launch_raster(const DeviceScene &sc, const DeviceFrame &fr, int hdr, float4 *out, unsigned long long *counters, hipStream_t stream);
/* ... into the RGBA8 words k_quantize would store for that frame (uncounted) */
void launch_raster(const DeviceScene &sc, const DeviceFrame &fr, int hdr, uint32_t *out8, hipStream_t stream);
/* flx_scene_update (flx_refit.hip).  n_rows rows (3 float4 each) -> geometry rows [first, first + n_rows); a box row keeps its words 0..5 */
void launch_scene_rows(const float4 *rows, float4 *geometry, uint32_t first, uint32_t n_rows, hipStream_t stream);
/* flx_scene_update_device.  n_rows rows in device memory (and their 7 float4 of attributes each, or nullptr) copied into stage_rows / stage_attributes and held
 * against geometry rows [first, first + n_rows) by flx_scene_update's rules.  verdict: two words, both ~0 before the launch; [0] <- the least
 * row * 4 + rule (0 kind, 1 transform number, 2 skip count, 3 a vertex not finite) of a row that offends, [1] <- 0 if a vertex lies beyond the fast box bound */
void launch_rows_check_stage(const float4 *rows, const float4 *attributes, const float4 *geometry, uint32_t first, uint32_t n_rows, float4 *stage_rows,
                             float4 *stage_attributes, uint32_t *verdict, hipStream_t stream);
/* words 0..5 of every box row with a skip count s > 0 = min / max over the vertices of the triangle rows in (i, i + s], -0 below +0 (a box over no triangle keeps
 * its floats); work: refit_workspace_words(n_entries) words */
size_t refit_workspace_words(uint32_t n_entries);
void launch_refit(float4 *geometry, uint32_t n_entries, uint32_t *work, hipStream_t stream);
/* the threaded or the forward-ordered copy (`entries` of them) follows the geometry rows: the six floats of a box, a triangle's vertex and two edges; links and meta words stay */
void launch_rederive(const float4 *geometry, uint32_t n_entries, float4 *copy, uint32_t entries, hipStream_t stream);
/* flx_scene_upload_device (flx_derive.hip): flx_scene_upload's decisions and both derived copies from an entry array in device memory.  work: derive_workspace_words(n_entries)
 * words, the record in its first DERIVE_RECORD_WORDS.  launch_derive_check fills the record: [0] 0 where no entry offends, else ~(entry * 4 + rule) of the first entry
 * the host's loop refuses and its first rule there (0 transform number out of range, 1 skip count leaves the array, 2 type not 0, 1 or 2); [1] max_transform;
 * [2] a triangle has a NaN vertex; [3] a box coordinate is not finite or beyond 2^59; [4] boxes; [5] live (non-terminator) entries; [6] entry 0's meta word;
 * [7] a box is flat: not min < max on all three axes (a NaN corner included).
 * It touches the workspace alone.  launch_derive_copies, for an array that passed: walk <- build_threaded's copy (live + 1 entries, min(4096, live) + 1 of them hot),
 * fwd <- build_lockstep's (live + 1), bit for bit for a properly nested skip list; no kernel waits for another workgroup, every scan is a launch per level and
 * recurses on its block totals: any entry count flx_scene_upload takes. */
constexpr uint32_t DERIVE_RECORD_WORDS = 8;
size_t derive_workspace_words(uint32_t n_entries);
hipError_t launch_derive_check(const float4 *geometry, uint32_t n_entries, uint32_t *work, hipStream_t stream);
void launch_derive_copies(const float4 *geometry, uint32_t n_entries, uint32_t live, uint32_t *work, float4 *walk, float4 *fwd, hipStream_t stream);
/* out <- words 6, 9 and 10 of every entry (3 words each): what flx_scene_update holds host rows against */
void launch_entry_meta(const float4 *geometry, uint32_t n_entries, uint32_t *out, hipStream_t stream);
/* x[0 .. m) <- its exclusive prefix, both words (wrapping sums), as flx_scene_upload_device's scans: a launch per level of block totals.  totals: scan_totals_items(m) items */
size_t scan_totals_items(uint32_t m);
void launch_exclusive_scan(uint2 *x, uint32_t m, uint2 *totals, hipStream_t stream);
/* flx_tree_build_device / flx_tree_emit_device (flx_build.hip): flx_mesh.hip's tree over n triangle rows, level by level.  Per triangle or position: tbox (its bounds:
 * (min, max) per axis), perm / owner and their next level's (the triangle at a position; the node it stands in while that node may split), open (nodes that start
 * there: n + 1), bucket, entry, x (n + 1).  Per node, `capacity` of them: node (first, count, ancestors starting at first, axis or 3: a leaf; after
 * launch_tree_index: its entry, the entries beneath it), keys (6), centre (3), cnt, y (capacity + 1).  totals: room for the scans of x and of y. */
struct TreeArrays {
  float2 *tbox; uint32_t *perm, *permNext, *owner, *ownerNext, *open, *bucket, *entry; uint2 *x, *y, *totals;
  uint4 *node, *cnt; uint32_t *keys; double *centre;
};
/* verdict[0] (~0 before) <- the least row * 4 + rule of a refused row (0 word 10 is not 2, 1 word 9 differs from row 0's or is no whole number in [0, 2^20), 2 a vertex is not
 * finite); the bounds, the identity permutation, the root (open zeroed before) */
void launch_tree_check(const float4 *rows, uint32_t n, uint32_t *verdict, const TreeArrays &t, hipStream_t stream);
/* the level's nodes [base, base + m) decide and count their children: y[m].x <- how many the level has; then, with room for them: their ranges, the next level's perm / owner */
void launch_tree_level(const TreeArrays &t, uint32_t n, uint32_t base, uint32_t m, uint32_t depth, double maxDepth, hipStream_t stream);
void launch_tree_children(const TreeArrays &t, uint32_t n, uint32_t base, uint32_t m, hipStream_t stream);
/* entry[p] and (entry, entries beneath) of every node, from the scan of open */
void launch_tree_index(const TreeArrays &t, uint32_t n, uint32_t nodes, hipStream_t stream);
/* the block's n + nodes rows of both arrays (a box row's words 0..5: launch_refit's) and the ids */
void launch_tree_emit(const float4 *rows, const float4 *attributes, const TreeArrays &t, uint32_t n, uint32_t nodes, float transform, float4 *geometry,
                      float4 *attributesOut, int32_t *ids, hipStream_t stream);
/* flx_scene_splice_device (flx_splice.hip).  launch_splice_check, over the resident geometry (n_entries rows) and ids, fills the record (SPLICE_RECORD_WORDS, zeroed
 * before): [0] 0 where nothing offends, else ~(entry * 4 + rule) of the first offending entry and its first rule (0 the parent, 1 not the direct parent, 2 a box cut
 * in two, 3 the ids are out of order); [1] end: 1 + the last entry whose word 10 is not 0; [2] ids below first; [3] ids at or above first + n_old.  first + n_old
 * <= n_entries.  launch_splice_rows assembles both arrays (n_padded rows each, fresh memory): rows [0, first) of the old, n_new of the block, the old rows
 * [first + n_old, end) — end_new = end + n_new - n_old —, zeros; word 6 of the parent and of the boxes that hold it grows by n_new - n_old.  launch_splice_ids: the
 * first `below` old ids, the block's plus first, the last `above` old ids plus delta. */
enum { SPLICE_REC_VERDICT = 0, SPLICE_REC_END, SPLICE_REC_IDS_BELOW, SPLICE_REC_IDS_ABOVE, SPLICE_RECORD_WORDS };
struct SpliceShape { uint32_t first, n_old, n_new, parent, end_new, n_padded; };
void launch_splice_check(const float4 *geometry, uint32_t n_entries, const int32_t *ids, uint32_t n_ids, uint32_t first, uint32_t n_old, uint32_t parent, uint32_t *record,
                         hipStream_t stream);
void launch_splice_rows(const float4 *geometry, const float4 *attributes, const float4 *blockGeometry, const float4 *blockAttributes, const SpliceShape &shape,
                        float4 *geometryOut, float4 *attributesOut, hipStream_t stream);
void launch_splice_ids(const int32_t *ids, uint32_t n_ids, const int32_t *blockIds, uint32_t n_block, uint32_t below, uint32_t above, uint32_t first, int32_t delta,
                       int32_t *out, hipStream_t stream);
/* flx_textures_upload / flx_texture_update (flx_atlas.hip): n source images nearest-resampled into cells of w x h texels of an RGBA8 image of `pitch` texels a row:
 * image i fills cell first_cell + i, at column cell % tw, row cell / tw; texel (x, y) of a cell <- source texel (floor((2x + 1) sw / 2w), floor((2y + 1) sh / 2h)),
 * copied (ATLAS_RGBA8) or quantised by pack_rgba8 (ATLAS_RGBA32F).  The sources: table[0 .. n) in device memory, or — table nullptr, n = 1 — *one, passed by value.
 * It writes the texels of those cells and no others.  One launch: at most ATLAS_TABLE_IMAGES images (a slot of the staging ring holds their table). */
enum { ATLAS_RGBA8 = 0, ATLAS_RGBA32F = 1 };
struct AtlasSource { const void *pixels; uint32_t sw, sh, format, pad; };
constexpr uint32_t ATLAS_TABLE_IMAGES = 2048;
void launch_atlas_cells(uint32_t *dst, uint32_t pitch, uint32_t w, uint32_t h, uint32_t tw, uint32_t first_cell, uint32_t n, const AtlasSource *table,
                        const AtlasSource *one, hipStream_t stream);
/* ray queries (flx_query.hip): n caller's rays (2 float4 each) walked through the scene by one persistent launch, a hit row (2 float4) per ray; what: FLX_RAYS_*.
 * ctl: two device words, zeroed in front of the launch on the same stream: [0] the cursor the waves draw chunks of QUERY_CHUNK consecutive rays from, [1] <- waves
 * that drew at least one.  groups: workgroups wanted (0: one per compute unit, no more than the rays fill).  *ran: what was launched.  false: the kernel cannot have
 * its LDS on this device. */
constexpr uint32_t QUERY_CHUNK = 128;
struct QueryLaunch { uint32_t ldsCount = 0, pre = 0, groups = 0, n = 0, what = 0; };
bool launch_ray_query(const DeviceScene &sc, const float4 *rays, float4 *hits, uint32_t n, uint32_t what, uint32_t *ctl, uint32_t compute_units, uint32_t groups,
                      hipStream_t stream, QueryLaunch *ran);
void launch_debug_math(int fn, const float *a, const float *b, float *out, uint32_t n, hipStream_t stream);
void launch_debug_intersect(int fn, const float *in, float *out, uint32_t n, hipStream_t stream);
bool launch_debug_walk(int variant, const DeviceScene &sc, const float *in, float *out, uint32_t n, hipStream_t stream);      /* false: the scene does not allow that variant */
/* variant 0 of launch_debug_walk with the threaded entries [0, ldsCount) staged in LDS (ldsCount <= walk_hot); out: 10 floats per ray.  false: the LDS it needs is more than
 * the kernel may have */
bool launch_debug_walk_staged(const DeviceScene &sc, uint32_t ldsCount, const float *in, float *out, uint32_t n, hipStream_t stream);

}  // namespace flx
#endif
