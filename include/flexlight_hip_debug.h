/*
 * flexlight_hip_debug.h — instrumentation, A/B knobs and test hooks of libflexlight_hip.so.
 *
 * NOT the drop-in boundary (that is include/flexlight_hip.h: what a FlexLight host binds).  What is here exists for the parity tests
 * (device-side evaluators of single routines, work counters compared with the oracle's), for A/B measurements (which kernel organisation runs a frame:
 * every choice renders the same frame, bit for bit), for fault injection and for the launch diagnostics tools/ prints.  Same library, same ABI rules
 * (extern "C", plain pointers and sizes); a host never needs any of it.  tests/, tools/ and bench.py bind these through flexlight_hip/capi.py.
 */
#ifndef FLEXLIGHT_HIP_DEBUG_H
#define FLEXLIGHT_HIP_DEBUG_H

#include "flexlight_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Counters of the last flx_render_device frame (collected only when enabled; costs atomics). */
flx_status flx_set_counters_enabled(flx_context *ctx, int enabled);
flx_status flx_get_counters(flx_context *ctx, flx_counters *out);

/* The last frame begun in the loop: 0 its own launches, 3 it went to the frame server. */
flx_status flx_last_chained(flx_context *ctx, int *chained);

/* A scene that MOVES in the frame server.  The reference refills its transform UBO and its light texture before every frame (modules/pathtracerWGL2.js:258-262,
 * 361-365) and an example like examples/dragon.js turns an object every tick.  Once flx_transforms_upload / flx_lights_upload has brought CHANGED contents of the
 * same counts, the server's next launch takes those arrays WITH every frame — they are posted with the frame's view, a version per frame in flight, and a later
 * upload no longer ends the launch (round 4 before this: every changed upload ended it and the frames went to the lanes).  Scenes whose 32 words per transform + 6
 * per light exceed 1024 keep the old behaviour, and so does flx_set_server_moving_scenes(ctx, 0).  Frames are bit-identical either way.
 * flx_server_moving: 1 while a launch of that kind is running. */
flx_status flx_set_server_moving_scenes(flx_context *ctx, int on);
int flx_server_moving(const flx_context *ctx);

/* Would flx_frame_begin hand this frame to the frame server (under flx_set_frame_chain(ctx, 3): whatever its size)?  1 / 0. */
int flx_frame_server_takes(flx_context *ctx, const flx_frame_params *params);
/* Which of the images of flx_frame_target_set the frame begun last goes to (-1: none). */
int flx_frame_target_index(const flx_context *ctx);

/* Device faults reach the status code.  The frame kernels' wait loops have watchdogs (seconds); a wave that gives up — or finds a ring slot that never
 * fills — sets a bit in the context's device error word (pinned host memory), and the next call in which the host waits for frames (flx_render,
 * flx_render_batch, flx_frame_end, flx_sync) returns FLX_ERR_DEVICE with the bits in flx_last_error and clears the word: the frame is incomplete.  A healthy
 * frame never gets there; this hook forces it for tests: the next frames' kernels give up after `watchdog_polls` polls (0: the built-in limit) and, with
 * FLX_INJECT_NO_SHADING, their shade waves drop every batch they pop, so that the walk waves wait for paths that never come back. */
#define FLX_INJECT_NO_SHADING 1u
flx_status flx_debug_inject_fault(flx_context *ctx, uint32_t watchdog_polls, uint32_t flags);
/* The shading keeps a per-triangle table of what fragment:500-512 derives from a triangle and its transform alone (three acos and three tan per shade otherwise),
 * made again at scene / transform uploads.  0: every shade computes the values itself — the same floats; for A/B runs. */
flx_status flx_debug_set_angle_table(flx_context *ctx, int on);
/* The per-pixel kernel (filter / temporal frames, small scenes) with the samples of a pixel side by side: k_trace_samples — a workgroup per 8 x 8 screen tile, a wave per
 * sample, the cross-sample globals of the shader (fragment:83-89) replayed in the shader's order afterwards — for frames of 2, 4 or 8 samples and at most 4 bounces; 0: the
 * sample-sequential k_trace_pixels always.  Frames, G-buffers and work counters are identical; for A/B runs (profiles/r05_sample_parallel.txt). */
flx_status flx_debug_set_sample_parallel(flx_context *ctx, int on);
/* Which per-pixel kernel the last frame ran, where it ran pipeline 1 (flx_last_pipeline): samples_side_by_side 0 for the sample-sequential k_trace_pixels,
 * S for k_trace_samples<S>; lockstep 1 for the variant with the wave's lockstep walk; counted 1 for the build with the work counters.  All three are -1
 * when the last frame ran another pipeline.  For tests: they prove which instantiation rendered a frame. */
flx_status flx_debug_last_trace_kernel(flx_context *ctx, int *samples_side_by_side, int *lockstep, int *counted);
/* the order in which the frame kernel draws a frame's 8 x 8 screen tiles: order[q] = the tile of the q-th draw (a permutation of the frame's n tiles; n = 0: tile q); frames do not depend on it */
flx_status flx_debug_set_tile_order(flx_context *ctx, const uint32_t *order, uint32_t n);
/* the adaptive tile order — the draw order made from what every tile cost in the last frame of the same shape (the lightest tiles last) — on (1, the default) or off (0: screen order) */
flx_status flx_debug_set_adaptive_order(flx_context *ctx, int on);
/* the sort behind it on its own (tests): the order k_tile_order makes of n per-tile costs — mode 1: sixteen classes of equal size, heaviest first, screen order inside a class (what the library uses);
 * 0: two classes, the lightest tenth last */
flx_status flx_debug_tile_order_of(flx_context *ctx, const float *cost, uint32_t n, int mode, uint32_t *order);
/* counted frames sum the entries visited by the paths of every screen tile: n > 0 turns that on (and zeroes the sums) for frames of up to n tiles, out copies the sums out first, n = 0 turns it off */
flx_status flx_debug_tile_cost(flx_context *ctx, unsigned long long *out, uint32_t n);
/* Rehearsal of a device group on ONE GPU: the frame server's launch takes `groups` CUs only (0: all), so that the launches of several contexts run beside
 * each other. */
flx_status flx_debug_set_server_groups(flx_context *ctx, uint32_t groups);
/* diagnostics of the frame server's last launch (csrc/flx_server.h: SVS_*): start, end, frames completed, tiles, batches, rotations, ... */
flx_status flx_get_server_stats(flx_context *ctx, uint64_t *out /* [16] */);
/* the control words of up to four workgroups of the frame server that gave up (72 words each: workgroup, wave, its 64 LDS control words, the relayed posts, the slots' tile cursors) */
flx_status flx_get_server_dump(flx_context *ctx, uint64_t *out /* [4 * 72] */);

/* ranks of the context's communicator as RCCL reports them (ncclCommCount); 0: the context belongs to none */
int flx_comm_count(const flx_context *ctx);

/* Kernel organisation of the path-trace pass.  0 = automatic: the sample-sequential per-pixel kernel when use_filter /
 * is_temporal need the cross-sample G-buffer state; for scenes of up to 128 entries the per-pixel kernel too, or — from 32 bounce
 * iterations per pixel (4 with four or more lights) in frames of at least 2^20 paths — the persistent path kernel; the wavefront
 * pipeline for everything larger; 1 = per-pixel kernel, 2 = persistent path kernel, 3 = wavefront pipeline.
 * Results are identical; the explicit values are for A/B timing and tests.  flx_last_pipeline: what the last frame ran. */
flx_status flx_set_pipeline(flx_context *ctx, int pipeline);
flx_status flx_last_pipeline(flx_context *ctx, int *pipeline);
/* Scenes of at most 128 entries that all stand in transform 0 (cornell, cornell.obj, the theater) are walked by the wave in
 * lockstep over the entries in the reference's order instead of lane by lane over the threaded copy (per-pixel and persistent
 * path kernels; same entries per ray, same arithmetic, same counters).  on = 0 switches that off, for A/B timing and tests. */
flx_status flx_set_lockstep(flx_context *ctx, int on);
/* Wavefront pipeline: run the bounce loop as 1..4 independent chains of screen-tile ranges on separate HIP
 * streams (default 1: more chains measured slower, profiles/r01_ab_stream_groups.txt), so that the tail of one chain's persistent walk kernel overlaps the other's work. */
flx_status flx_set_wavefront_groups(flx_context *ctx, int groups);
/* Wavefront pipeline: how the bounce loop is laid out on the GPU.  0 (default): automatic — ONE persistent launch for all bounces
 * (k_wf_frame: the walk waves and shade waves of a workgroup pass paths to each other through LDS rings; no kernel boundary, hence no
 * tail, between the bounces) where the scene's object spaces leave room in LDS, rounds otherwise; 1: rounds, a shade + walk kernel
 * pair per bounce (the round-1/2 organisation); 2: the frame kernel where it fits.  Frames and work counters are identical. */
flx_status flx_set_wavefront_organisation(flx_context *ctx, int organisation);
/* Wavefront pipeline: who traces the primary rays and shades bounce 0.  0: two kernels in front of the bounce loop (k_primary, k_wf_shade0); 3: ONE kernel in
 * front (k_wf_front: a wave traces the primary rays of its 8 x 8 screen tile and shades it straight away); 2: the frame kernel itself wherever it runs — its shade waves
 * make the fresh paths one screen tile at a time while its walk waves walk the earlier ones — and one kernel in front elsewhere; 1 (default): automatic — the frame
 * kernel itself where a workgroup gets at least 32 screen tiles (a whole 1080p frame: yes, a rank's eighth of one: no), else one kernel in front up to 128 M paths
 * a pass, two beyond.  Frames and work counters are identical. */
flx_status flx_set_frame_front(flx_context *ctx, int mode);
/* What the wavefront pipeline ran for the last frame: 1 rounds, 2 the frame kernel, 3 the frame kernel with the front of the frame inside it;
 * 0 when another pipeline rendered it (flx_last_pipeline). */
flx_status flx_last_organisation(flx_context *ctx, int *organisation);

/* ---- diagnostics --------------------------------------------------------------------------------- */
/* Evaluate one of include/flx_math.h's routines on the GPU for n inputs (b may be NULL for unary
 * functions); used by tests to prove CPU/GPU bit equality.  fn: 0 sin 1 cos 2 tan 3 acos 4 atan2
 * 5 exp 6 pow 7 tanh 8 floor 9 sqrt 10 div. */
flx_status flx_debug_math(flx_context *ctx, int fn, const float *a, const float *b, float *out, uint32_t n);
/* Evaluate one of the intersection routines on the GPU, AS THE KERNELS CALL IT, for n rows; used by tests to hold the device code against literal
 * answers computed from the shader text (tests/golden/intersect_kat.json.gz).  fn 0: moellerTrumbore (fragment:123-140) through the walk kernels'
 * routine over stored edges (exact 1/det from v_rcp_f32, branch-free acceptance), 1: moellerTrumboreCull (:143-158) through the same routine, 2: rayCuboid
 * (:161-167) through the walk kernels' box test (interval test, exact quotients by reciprocal, IEEE division where their preconditions fail); 3, 4, 5: the
 * same three as the per-pixel kernel calls them; 6: fn 2 for a scene whose boxes are NOT bounded (walk_fast_boxes = 0: every quotient by IEEE division) — fn 2 stands for a
 * scene that is, so its rows must keep flx_scene_upload's bound: every box coordinate finite with |x| <= 2^59 (tests/golden/intersect_edge_kat.json.gz); 7: fn 2 with the
 * interval test in its single-comparison form, the one the frame kernels take for a scene without a flat box (flx_debug_walk_thick_boxes) — a flat box may be put through it like any other; 8: fn 7 for a scene whose boxes are not bounded, as 6 is to 2.  Rows: triangles 16 floats (a, b, c, origin, direction, l), boxes 13 (l, origin, direction, min, max);
 * out: 3 floats per row for fn 0 and 3 ((s, u, v) of a hit, zeros otherwise), else one float 0 / 1. */
flx_status flx_debug_intersect(flx_context *ctx, int fn, const float *in, float *out, uint32_t n);
/* The uploaded scene's walk_fast_boxes, read-only: 1 when every coordinate of every box entry (type 1) is finite with |x| <= 2^59 — the precondition under which the
 * walk kernels take their box quotients through reciprocals; triangle entries do not count. */
flx_status flx_debug_walk_fast_boxes(flx_context *ctx, int *fast);
/* The uploaded scene's walk_thick_boxes, read-only: 1 when every box entry (type 1) is KNOWN to have min < max on all three axes.  The frame kernels and the frame server
 * then decide "surely hit" in their box test from one comparison, lo(tmax) >= hi(tmin), instead of three cross-pair ones; a flat box can never pass that comparison and
 * would take the exact quotients every time it is hit, so a scene that has one keeps the cross-pair form.  A hint of speed alone — both forms give the reference's
 * boolean for every box.  flx_scene_upload, flx_scene_upload_device and flx_scene_splice_device look at every box (of the spliced scene: as refitted); flx_scene_update and
 * flx_scene_update_device refit the boxes on the device without reading them back and clear the hint until the next upload. */
flx_status flx_debug_walk_thick_boxes(flx_context *ctx, int *thick);
/* Which form the frame kernels and the frame server take from the next frame on: -1 by the scene's hint (the default), 0 the cross-pair form, 1 the single comparison.
 * flx_debug_walk's variant 0 and flx_debug_walk_staged — the frame kernels' lane walk, a ray at a time — follow the same choice.  For tests: frames, walks and work
 * counters are the same in either form on every scene. */
flx_status flx_debug_set_box_test(flx_context *ctx, int form);
/* The form compiled into the kernel the last frame kernel or frame server launch ran (what flx_debug_last_walk_lds describes): 0 cross pairs (k_wf_frame_flat,
 * k_wf_frame_stamped_flat, k_wf_server<., false>), 1 the single comparison (k_wf_frame, k_wf_frame_stamped, k_wf_server<., true>); -1: the rounds or another pipeline ran,
 * or nothing since the scene upload.  Both give the same frames: this is the one place that tells which ran. */
flx_status flx_debug_last_box_test(flx_context *ctx, int *form);
/* Whether every box entry (word 10 == 1) of an entry array has min < max on all three axes — flx_scene_upload's own scan, on the host, no context: n_entries rows of 12
 * floats.  A NaN corner or min > max is not thick. */
int flx_debug_boxes_thick(const float *geometry, uint32_t n_entries);
/* ---- vertex updates ------------------------------------------------------------------------------- */
/* Beyond the drop-in boundary, like everything in this header: a host that only knows flx_scene_upload renders every scene (the reference's updateScene() is that
 * call), this is the shorter way for a scene whose topology stands still.  (Declared here and not in flexlight_hip.h because that header is held at the 80
 * functions it has: tests/test_capi_cpu.py.  The JavaScript renderers, the N-API addon and capi.py bind it like any other call.) */
/* A scene whose VERTICES move (a cloth, a wave surface, a morphing mesh: the application sets primitive.vertices and calls renderer.updateScene()).
 * Replace rows [first_entry, first_entry + n_entries) of the uploaded scene and refit every box.  The rows must keep what
 * the scene holds in words 6 (skip count, boxes), 9 (transform number) and 10 (kind).  Words 0..5 of box rows are ignored:
 * the device computes them — the componentwise min / max of the vertices of all triangle rows the box skips over, which is what the
 * flatten computes (modules/scene.js:242-256, 269-279), bit for bit; a box that skips nothing, or nothing but boxes, keeps its six floats.
 * attributes may be NULL: the attribute rows stay.  The caller's buffers are free when the call returns.  A frame begun before the call
 * renders the old geometry, a frame begun after it the new.  FLX_ERR_INVALID (and the scene exactly what it was) for a range that leaves
 * the array, a changed metadata word, a vertex that is not finite, and for a scene that was uploaded with a NaN vertex (Math.min would
 * carry it into the boxes above; the device's min does not); FLX_ERR_NO_SCENE before flx_scene_upload. */
flx_status flx_scene_update(flx_context *ctx, uint32_t first_entry, uint32_t n_entries,
                            const float *geometry /* n_entries * 12 */, const float *attributes /* n_entries * 28 or NULL */);
flx_status flx_group_scene_update(flx_group *group, uint32_t first_entry, uint32_t n_entries, const float *geometry, const float *attributes);
/* flx_scene_update for rows that are ALREADY ON THE DEVICE (a simulation kernel's output, a torch tensor, another library's buffer): d_geometry and d_attributes
 * are pointers into device memory of ctx's device, 16-byte aligned (FLX_ERR_INVALID otherwise: a host pointer, another device's memory, an allocation that ends
 * before the rows do).  A kernel holds the rows against the scene where flx_scene_update's loop does so on the host: the same refusals with the same messages, the
 * first offending row and its first rule, and a refused call leaves the scene exactly as it was.  producer_stream: the hipStream_t on which the rows were written —
 * the check waits for what is enqueued there at the time of the call — or NULL: the rows are complete (NULL does not name the legacy default stream).  The check
 * runs on a stream of the context's own and the host waits for it alone, not for the context's frames in flight; the rows are copied into the context's memory
 * by then, so the caller's buffers are free when the call returns.  Everything else is flx_scene_update.  A group keeps the host call (flx_group_scene_update): the
 * rows live on one device, its contexts on several. */
flx_status flx_scene_update_device(flx_context *ctx, uint32_t first_entry, uint32_t n_entries,
                                   const void *d_geometry /* n_entries * 12 floats, on ctx's device */,
                                   const void *d_attributes /* n_entries * 28 floats or NULL */,
                                   void *producer_stream /* hipStream_t that wrote the rows, or NULL: they are complete */);
/* flx_scene_upload for arrays that are ALREADY ON THE DEVICE (a mesh a simulation or a torch op produced, a tree rebuilt there): geometry, attributes and ids are
 * pointers into device memory of ctx's device, 16-byte aligned, each allocation long enough for its array (FLX_ERR_INVALID with a message of its own otherwise; d_ids
 * may be NULL when n_ids is 0).  Everything flx_scene_upload decides and derives on the host — the refusals, max_transform, the NaN and bounded-box flags, the
 * threaded hot-first copy, the forward-ordered copy — kernels decide and derive (csrc/flx_derive.hip), with the same results: the same refusals in the same order
 * with the same messages (an empty scene; more than 2^28 - 1 entries; then the first offending entry and, within it, the first of: transform number out of range,
 * skip count leaves the array, type not 0, 1 or 2), and for every properly nested skip list the same four device arrays bit for bit, hence the same frames.  A
 * list that is not properly nested (a box whose range ends inside another's) still gives a valid scene, every link naming the entry's original successor and every
 * walk visiting the same entries, but the storage order of the threaded copy may differ from the host's.  A refused call leaves the context's scene exactly as it
 * was, still renderable.  No array crosses the bus in either direction: eight words of scalars come back.  The scans behind the derivation recurse on their block
 * totals, a launch per level: any n_entries_padded flx_scene_upload takes.  producer_stream: as for flx_scene_update_device.  Ordered like flx_scene_upload: a
 * frame begun before the call renders the old scene, a frame begun after it the new; the call waits for the context's stream before it returns, and the caller's
 * arrays are free then.  flx_scene_update and flx_scene_update_device work afterwards as after flx_scene_upload (the first update of HOST rows fetches the 12 bytes
 * per entry it holds its rows against).  A group keeps the host call (flx_group_scene_upload): the arrays live on one device, its contexts on several. */
flx_status flx_scene_upload_device(flx_context *ctx,
                                   const void *d_geometry   /* n_entries_padded * 12 floats, on ctx's device */,
                                   const void *d_attributes /* n_entries_padded * 28 floats */,
                                   uint32_t n_entries_padded,
                                   const void *d_ids /* n_ids int32, or NULL when n_ids == 0 */, uint32_t n_ids,
                                   void *producer_stream /* hipStream_t that wrote the arrays, or NULL: complete */);
/* A mesh's block of the entry array BUILT ON THE DEVICE from triangles that are in device memory (a simulation's output, a torch op's, a mesh whose topology
 * changes): what flx_mesh_import_obj + flx_mesh_flatten make on the host of the same triangles in the same order — the reference's generateBVH: leaves of at most
 * 4, a split at the bounding's centre on the axis with the fewest straddlers, three stable buckets, depth <= log2(n) + 8 — the same rows in the same order, bit
 * for bit (where no box holds both a -0 and a +0 on one axis: the refit orders them, Math.min does not), and the same ids.  Primitives are single triangles; the
 * reference's two-triangle planes are not built here.
 * flx_tree_build_device builds the tree of n_triangles geometry rows of kind 2 (9 vertex words, word 9 the transform number, word 10 = 2) level by level
 * (csrc/flx_build.hip) and keeps it in the context: the permutation, the nodes, the entry indices.  It runs on a stream of the context's own, touches nothing of
 * the uploaded scene, waits for no frame in flight, and returns when the host knows *n_entries = boxes + triangles: one wait per level of the tree.  The caller's
 * rows are free then.  producer_stream: as for flx_scene_update_device.  FLX_ERR_INVALID, each with a message of its own, and no tree kept: n_triangles 0 or above
 * 2^24; rows not in memory of ctx's device, not 16-byte aligned or in too short an allocation; then the first offending row and within it the first of: word 10
 * is not 2, word 9 differs from row 0's or is no whole number in [0, 2^20), a vertex is not finite; a tree of more than 2^28 - 1 entries.
 * flx_tree_emit_device writes the block of the last successful build: geometry and attribute rows of the boxes (attribute rows of zeros; the six floats by the
 * refit flx_scene_update runs) and of the triangles (copied unchanged; d_attributes NULL: zeros), ids[k] = the entry, counted from the block's first, of the k-th
 * triangle in emission order.  d_triangles: the rows the tree was built from (their count is what can be checked); every array in memory of ctx's device,
 * 16-byte aligned, long enough for the build's counts, and complete.  It returns when the arrays are complete and may be called again.  FLX_ERR_INVALID without a
 * successful build.  The block is ready to be spliced into the resident scene by flx_scene_splice_device (or, by hand, into an entry array, ids offset by its first
 * entry, for flx_scene_upload_device). */
flx_status flx_tree_build_device(flx_context *ctx,
                                 const void *d_triangles /* n_triangles * 12 floats, on ctx's device, in the order the host builder would be given them */,
                                 uint32_t n_triangles, void *producer_stream /* hipStream_t that wrote the rows, or NULL: complete */,
                                 uint32_t *n_entries /* out: boxes + triangles */);
flx_status flx_tree_emit_device(flx_context *ctx, const void *d_triangles,
                                const void *d_attributes /* n_triangles * 28 floats, or NULL: attribute rows of zeros */,
                                void *d_geometry /* n_entries * 12 floats */, void *d_attributes_out /* n_entries * 28 floats */, void *d_ids /* n_triangles int32 */);
/* A block of the RESIDENT scene replaced, inserted or removed in device memory: the step between "a tree can be built on the device" (flx_tree_emit_device's
 * block) and "a mesh of my scene can change shape on the device".  The caller keeps no copy of the scene's arrays: the context holds them.
 * Rows [first_entry, first_entry + n_old) go (n_old 0: an insertion in front of first_entry), the n_new rows of d_geometry / d_attributes come (n_new 0, the
 * pointers ignored: a removal).  parent_entry names the box that DIRECTLY holds that range, FLX_NO_PARENT: it stands at top level.  With end = 1 + the last
 * resident entry whose word 10 is not 0 (the reference's textureLength; a kernel finds it) and delta = n_new - n_old, the resident scene becomes what
 * flx_scene_upload makes of this array: rows [0, first_entry) as they are; the new rows; the old rows [first_entry + n_old, end), moved by delta; rows of zeros up
 * to the next multiple of 256 entries; word 6 (the skip count) of parent_entry and of every box whose range holds parent_entry grown by delta, in integer
 * arithmetic; and every box refitted as flx_scene_update refits them, over the whole array — the ancestors' six floats are then what a fresh flatten computes
 * (modules/scene.js:242-256), bit for bit; a box that skips nothing, or only boxes, keeps its six floats.  The id list becomes the old ids below first_entry, then
 * d_ids' n_new_ids ids plus first_entry (they count from the block's first entry, as flx_tree_emit_device writes them; NULL / 0: none), then the old ids at or
 * above first_entry + n_old plus delta; old ids of the replaced rows are dropped.  Both derived copies, max_transform, the NaN and bounded flags and the lockstep
 * eligibility are derived of the assembled arrays as flx_scene_upload_device derives them.  A parent left without children stays, a box with skip count 0 (the
 * reference's flatten would not emit it): removing it is a splice of the parent itself.
 * Refusals: FLX_ERR_NO_SCENE before an upload; FLX_ERR_INVALID, each with a message of its own and the resident scene — arrays, ids, frames — exactly what it
 * was: n_old and n_new both 0; an array not in memory of ctx's device, not 16-byte aligned or in too short an allocation; first_entry + n_old beyond end; end +
 * delta 0 or above 2^24 (a larger skip count is no exact float); a scene uploaded with a NaN vertex (as flx_scene_update); then what a kernel over the resident
 * geometry and ids finds, the first offending entry and its first rule: (a) parent_entry is no box, or its range (parent, parent + skip] does not hold the
 * replaced rows — for an insertion: first_entry > parent + skip + 1; first_entry == parent + skip + 1 appends to the parent — (a parent_entry that does not lie
 * in front of first_entry offends at entry first_entry); (b) a box between parent_entry and first_entry (FLX_NO_PARENT: any box in front of first_entry) reaches
 * first_entry: parent_entry is not the direct parent; (c) a box among the replaced rows reaches beyond them; (d) the resident id list is not non-decreasing, as
 * every list of the flatten is (the id that falls below its predecessor offends at the entry it names).  Last, the assembled array passes flx_scene_upload's
 * validation: a block with a bad transform number, skip count or type is refused with that call's three messages.
 * Ordered like flx_scene_upload_device: the checks run beside the frames in flight, the assembly behind them into fresh memory (never in place under a frame that
 * reads the old arrays); a frame begun before the call renders the old scene, a frame begun after it the new; the frame server's launch ends; the call waits for
 * the context's stream, and the caller's arrays are free when it returns.  flx_scene_update and flx_scene_update_device work afterwards as after an upload.
 * producer_stream: as for flx_scene_update_device, for all three arrays.  A group keeps the host calls (flx_group_scene_upload): the arrays live on one device,
 * its contexts on several; and there is no JavaScript binding: JavaScript has no device pointers. */
#define FLX_NO_PARENT 0xffffffffu
flx_status flx_scene_splice_device(flx_context *ctx, uint32_t first_entry, uint32_t n_old, uint32_t parent_entry,
                                   const void *d_geometry /* n_new * 12 floats, on ctx's device */, const void *d_attributes /* n_new * 28 floats */, uint32_t n_new,
                                   const void *d_ids /* n_new_ids int32, relative to the block's first entry, or NULL */, uint32_t n_new_ids,
                                   void *producer_stream /* hipStream_t that wrote the arrays, or NULL: complete */);
/* ---- textures ------------------------------------------------------------------------------------- */
/* Beyond the drop-in boundary, like the scene paths above (flx_atlas_upload of a finished atlas is the drop-in call).  An atlas BUILT ON THE DEVICE from its source
 * images, and ONE texture of it replaced in place.  The rule is the project's own (js/sceneFile.js: buildAtlas, which stays the yardstick): with tw = floor(2048 /
 * cell_w), the atlas is cell_w * tw wide and cell_h * n high (the reference's too-tall canvas, modules/pathtracerWGL2.js:85-104: fetchTexVal divides by it); image i
 * fills the cell at column i % tw, row floor(i / tw); destination texel (x, y) of a cell reads source texel (floor((2x + 1) * width / (2 * cell_w)), floor((2y + 1) *
 * height / (2 * cell_h))) — integers throughout, = Math.floor((x + 0.5) * width / cell_w) for every size; every texel outside the n cells is transparent black.
 * An image has tight rows.  FLX_IMAGE_RGBA8: 4 bytes a texel, copied.  FLX_IMAGE_RGBA32F: 4 floats a texel, each stored as the library's RGBA8 render targets store
 * a channel: floor(clamp(x, 0, 1) * 255 + 0.5), NaN -> 0; the nearest texel is picked first, then quantised.  What the frame kernels read keeps its layout and bytes.
 * flx_textures_upload replaces atlas `which` (0 albedo, 1 pbr, 2 translucency) from images in HOST memory, flx_textures_upload_device from images in memory of ctx's
 * device (a torch tensor, a decoded video frame, a frame flx_render_device made): 4-byte aligned for RGBA8, 16 for RGBA32F.  n == 0 is "none", exactly
 * flx_atlas_upload(ctx, which, NULL, 0, 0).  The context remembers cell_w, cell_h and n for later cell updates; flx_atlas_upload forgets them (a prebuilt atlas has
 * no known cells).  Ordered like flx_atlas_upload and flx_scene_upload_device: the frame server's launch ends, a second lane's frames in flight are waited for, the
 * kernel runs on the context's stream behind its own frames, and the call waits for that stream before it returns: the caller's pixels are free.
 * flx_texture_update[_device] replaces cell `index` of the resident atlas from one image of any size and either format; no other byte of the atlas changes.  Ordered
 * like flx_scene_update_device: the image is resampled into memory of the context's on a stream of its own (behind producer_stream), the host waits for that alone —
 * the context's frames in flight go on, the caller's pixels are free on return — and the cell is copied in behind those frames.  A frame begun before the call shows
 * the old texture, a frame begun after it the new one.
 * producer_stream: as for flx_scene_update_device.
 * Refusals, FLX_ERR_INVALID each with a message of its own, the atlas and what the context remembers of it exactly as they were, nothing enqueued on the context's
 * stream; in this order: which not 0 .. 2; images NULL with n > 0; cell_w 0 or above 2048; cell_h 0; then the first offending image and within it the first of:
 * pixels NULL, a dimension of 0, an unknown format, and — device variants — pixels not in memory of ctx's device, not aligned, or in an allocation that ends before
 * the image does; last, an atlas of 2^31 texels in height or more.  The update, instead of the cell sizes: no atlas built by flx_textures_upload* is resident;
 * index >= n.  A group keeps the host calls, as for scenes. */
#define FLX_IMAGE_RGBA8   0u
#define FLX_IMAGE_RGBA32F 1u
typedef struct flx_image { const void *pixels; uint32_t width, height, format; } flx_image;      /* tight rows */
flx_status flx_textures_upload(flx_context *ctx, int which, const flx_image *images, uint32_t n, uint32_t cell_w, uint32_t cell_h);      /* pixels in host memory */
flx_status flx_textures_upload_device(flx_context *ctx, int which, const flx_image *images, uint32_t n, uint32_t cell_w, uint32_t cell_h,
                                      void *producer_stream /* hipStream_t that wrote the pixels, or NULL: complete */);      /* pixels on ctx's device */
flx_status flx_texture_update(flx_context *ctx, int which, uint32_t index, const flx_image *image);
flx_status flx_texture_update_device(flx_context *ctx, int which, uint32_t index, const flx_image *image, void *producer_stream);
flx_status flx_group_textures_upload(flx_group *group, int which, const flx_image *images, uint32_t n, uint32_t cell_w, uint32_t cell_h);
flx_status flx_group_texture_update(flx_group *group, int which, uint32_t index, const flx_image *image);
/* Atlas `which` as the device holds it, after everything enqueued so far: *width, *height (0, 0: none) and, where out is not NULL, its width * height * 4 bytes
 * (FLX_ERR_INVALID where `bytes` is less).  out may be NULL to ask the size. */
flx_status flx_debug_atlas_read(flx_context *ctx, int which, uint8_t *out, size_t bytes, uint32_t *width, uint32_t *height);
/* ---- ray queries ---------------------------------------------------------------------------------- */
/* Beyond the drop-in boundary, like the vertex updates above, and bound the same way (the N-API addon and the JavaScript renderers bind the host call: castRays).
 * Rays of the CALLER'S OWN cast at the resident scene: what does this ray hit, is this point lit from there, which object is under the cursor — what every frame asks
 * through rayTracer and shadowTest, answered by the same walk (the threaded hot-first copy, its top in LDS, lanes refilled as their walks end: csrc/flx_query.hip)
 * with the oracle's bits.
 * A RAY ROW is 32 bytes, two 16-byte loads: words 0..2 the origin, 3 `l` (shadowTest's length; unused otherwise), 4..6 the direction, 7 ignored.  The closest-hit
 * walk starts at the reference's minLen (POW32), as rayTracer does: it takes no length.
 * A HIT ROW is 32 bytes, two 16-byte vector stores: words 0..2 float s, u, v of the closest hit; 3 int32 its entry index, -1 for none; 4 int32 2 x its transform
 * number; 5 int32 occluded, 0 or 1; 6 uint32 the entries the closest-hit walk fetched, 7 uint32 those the shadow walk fetched.  A miss has zeros in words 0..2 and
 * 4 and -1 in word 3 (flx_debug_walk's columns); a walk that was not asked for leaves zeros in its words (-1 in word 3); words 6 and 7 are zero without
 * FLX_RAYS_COUNT.  With both walks asked for a ray's shadow walk runs first, in a path's order.
 * s is a WORLD-SPACE parameter of the ray as given: the direction is not normalised, the hit point is origin + s * direction.  FLX_RAYS_OCCLUDED is the renderer's
 * own predicate with its quirks: one-sided, and `l` is compared in object space after the transformed direction was normalised — it
 * answers "would the renderer light this point", not a geometric any-hit.
 * flx_rays_cast_device is ordered like flx_render_device: enqueued on the context's stream with no wait of the host (flx_sync before the hits are read on another
 * stream), behind every upload, update, splice and frame enqueued before it — it sees the scene as of the call — and frames in flight finish unchanged.  Where the
 * frame server's launch is running it does what flx_render_device does: the launch ends after the frames posted to it, which are resolved into their output slots
 * (the host waits for that, and only then).  producer_stream: the hipStream_t on which the rays were written — the query waits for what is enqueued there at the
 * time of the call — or NULL: they are complete (as for flx_scene_update_device).  The caller keeps both arrays alive until the work is complete.  n == 0: FLX_OK,
 * nothing enqueued (the scene and `what` are looked at first: no scene or a bad `what` is refused for any n).  flx_rays_cast is the same for host arrays: staged through memory the context owns (grown, never shrunk); it waits and copies the hits out.
 * Refusals, each with a message of its own and nothing enqueued: FLX_ERR_NO_SCENE before a scene and transforms are up; FLX_ERR_INVALID where `what` has neither
 * FLX_RAYS_CLOSEST nor FLX_RAYS_OCCLUDED or has an unknown bit; for an array that is not memory of the context's device, not 16-byte aligned or in an allocation
 * too short for n rows; where the two arrays overlap. */
#define FLX_RAYS_CLOSEST  1u   /* rayTracer  (fragment:172-227) of every ray */
#define FLX_RAYS_OCCLUDED 2u   /* shadowTest (fragment:231-280) of every ray, with the row's l */
#define FLX_RAYS_COUNT    4u   /* also write the entries each walk fetched (a build of the kernel of its own) */
flx_status flx_rays_cast_device(flx_context *ctx, const void *d_rays /* n * 8 floats, on ctx's device */, void *d_hits /* n * 8 words */, uint32_t n, uint32_t what,
                                void *producer_stream /* hipStream_t that wrote the rays, or NULL: they are complete */);
flx_status flx_rays_cast(flx_context *ctx, const float *rays /* n * 8 floats */, void *hits /* n * 8 words */, uint32_t n, uint32_t what);      /* host arrays */
/* workgroups the query launch takes (0, the default: its own choice — one per compute unit, fewer where the rays do not give every lane one).  For tests: one
 * workgroup makes every lane take ray after ray.  A traced batch (flx_rays_trace_device, below) takes the same number for BOTH of its persistent launches: the first-hit
 * launch (1024 lanes a workgroup) and the paths kernel (256 lanes a workgroup).  So do flx_rays_planes[_device] and flx_rays_image[_device]: the first-hit launch and the
 * planes kernel (256 lanes a workgroup). */
flx_status flx_debug_set_query_groups(flx_context *ctx, uint32_t groups);
/* The last query launch since the scene upload (zeros if none): out[0] its ldsCount (entries of the tree's top staged in LDS), [1] whether its rays were
 * pre-transformed (0: transformed on the fly), [2] workgroups launched (1024 lanes each), [3] waves that drew at least one chunk, [4] n, [5] what, [6] the rays of a
 * chunk (consecutive indices a wave draws with one atomic), [7] draws made, the ones past the last chunk included.  It waits for the context's stream. */
flx_status flx_debug_last_query(flx_context *ctx, uint32_t out[8]);
/* RADIANCE along the caller's rays: what the renderer sees along each — another projection (panorama, fisheye, orthographic, a stereo pair), light probes, the
 * reflection rays of a hybrid renderer, a pipeline that makes its own rays.  For every ray row: hit = rayTracer(origin, direction), the closest hit exactly as
 * FLX_RAYS_CLOSEST answers it; no hit gives the miss row; otherwise c = the sum over s = 0 .. samples - 1 of lightTrace(hit, direction, origin, cos(float(s)),
 * max_reflections) added in sample order, then c * (1.0f / (float)samples), then c * originalColor as the LAST sample left it: a frame's pixel without filter and
 * without temporal (fragment:601-632), with the oracle's bits.  The ray's origin stands wherever lightTrace uses the camera (lastHitPoint, firstRayLength); the
 * direction is used as given, not normalised, as rayTracer takes it.
 * A RAY ROW is the query's, 32 bytes: words 0..2 the origin, 3 NOISE X, 4..6 the direction, 7 NOISE Y — the two words a closest-hit query does not read.  noise()
 * is fed the two noise coordinates where a frame feeds it the pixel's NDC: RAYS WITH EQUAL NOISE COORDINATES DRAW EQUAL RANDOM NUMBERS, so give every ray of a
 * batch its own (a frame's are spread over [-1, 1)^2; capi.noise_coordinates does that for n rays).
 * A RADIANCE ROW is 32 bytes, two 16-byte vector stores: words 0..2 float r, g, b; 3 float 1.0 for a hit, 0.0 for a miss (the frame's alpha); 4 float s of the
 * first hit; 5 int32 its entry, -1 for none; 6 int32 2 x its transform; 7 uint32 the bounce iterations shaded over all samples (the oracle's `shades` for this
 * ray).  A MISS ROW IS ALL ZEROS with -1 in word 5: as in a frame, where a pixel with no primary hit is (0, 0, 0, 0) — not the ambient light.
 * A ray batch has no width, height or camera, hence the params of its own.  Temporal accumulation is image-space over a history: a loose batch has none, a ray
 * IMAGE traced again frame after frame has (flx_rays_image_temporal_device, below).
 * The FILTER's bookkeeping does carry over: the denoise chain reads nothing of a camera, and its five render targets are per ray (flx_rays_planes_device, below;
 * flx_rays_image_device traces a ray IMAGE and runs the chain over it).  This call is the unfiltered radiance.
 * Ordering, producer_stream, the frame server, lights and transforms uploaded over a running launch, the staging of the host variant and n == 0 are
 * flx_rays_cast_device's and flx_rays_cast's, word for word: enqueued on the context's stream with no wait of the host, it sees the scene as of the call, frames in
 * flight finish unchanged; n == 0: FLX_OK, nothing enqueued (the scene and the params are looked at first).  The batch is cut into slabs of rays so that the
 * context's scratch (hit rows, samples slots of 16 bytes a ray, grown and never shrunk) has a ceiling: at most 2^24 slots and 2^21 rays a slab, at least 64 rays;
 * any n works at any sample count the device's memory holds 64 rays' slots of.  (Where that scratch must grow, the host waits for the stream first.)
 * Refusals, each with a message of its own and nothing enqueued: FLX_ERR_NO_SCENE before a scene and transforms are up; FLX_ERR_INVALID for NULL params, samples < 1,
 * max_reflections < 0 or texture_width < 1; for an array that is NULL, not memory of the context's device, not 16-byte aligned or in an allocation too short for n
 * rows; where the two arrays overlap.  A group traces no rays, as it casts none. */
typedef struct flx_trace_params {
  int32_t samples, max_reflections;
  float min_importancy;
  float ambient[3];
  float random_seed;
  int32_t texture_width;
} flx_trace_params;
flx_status flx_rays_trace_device(flx_context *ctx, const flx_trace_params *params, const void *d_rays /* n * 8 floats, on ctx's device */, void *d_radiance /* n * 8 words */,
                                 uint32_t n, void *producer_stream /* hipStream_t that wrote the rays, or NULL: they are complete */);
flx_status flx_rays_trace(flx_context *ctx, const flx_trace_params *params, const float *rays /* n * 8 floats */, void *radiance /* n * 8 words */, uint32_t n);      /* host arrays */
/* most rays of a slab of a traced batch (0, the default: the ceiling above).  For tests: a small value makes a batch span several slabs.  flx_debug_set_query_groups
 * sets the workgroups of a slab's first-hit launch AND of its paths kernel (256 lanes each there).  Both apply to flx_rays_planes[_device] and
 * flx_rays_image[_device] (below) as they do to a traced batch: the slab's ceiling, and the workgroups of the first-hit launch and of the planes kernel. */
flx_status flx_debug_set_trace_slab(flx_context *ctx, uint32_t rays);
/* The last traced batch (zeros if none): out[0] its slabs, [1] the rays of a full slab, [2] workgroups of the last slab's paths kernel, [3] whether its bounce walks
 * went in lockstep, [4] n, [5] samples, [6] workgroups of the last slab's first-hit launch, [7] the items a wave draws with one atomic.  It waits for nothing. */
flx_status flx_debug_last_trace(flx_context *ctx, uint32_t out[8]);
/* A traced batch IN FIRST-HIT ORDER: flx_rays_trace_device for rays that arrive in no useful order — reflection rays, probe rays, rays a pipeline made for itself.
 * The rows of a batch do not depend on each other, so the library may trace a slab's rays in any order: with FLX_TRACE_ORDER_HITS it sorts each slab by the Morton
 * code of the first hit points (include/flx_ray_key.h: the key, exactly defined; csrc/flx_rays_order.hip: bounds, keys and a stable radix sort on the device) and
 * the paths kernel takes its rays through that order, so that a wave's 64 lanes start in one corner of the scene.  THE RADIANCE ROWS ARE flx_rays_trace_device's,
 * BIT FOR BIT, IN THE CALLER'S ORDER; what changes is the time (profiles/rays_order.txt) and 16 bytes of scratch a ray of a slab more (at most 2^21 rays: 33 MB).
 * order == 0 is flx_rays_trace_device itself, with the same launches.  Ordering, producer_stream, the frame server, slabs, n == 0 and the host call's staging are
 * flx_rays_trace_device's and flx_rays_trace's, word for word.  Refusals: an unknown bit of `order` is FLX_ERR_INVALID with its own message (for any n, after the
 * scene and the params were looked at); every other refusal is flx_rays_trace's under this call's name. */
#define FLX_TRACE_ORDER_HITS 1u   /* trace each slab's rays in the order of their first hit points' Morton codes */
flx_status flx_rays_trace_ordered_device(flx_context *ctx, const flx_trace_params *params, const void *d_rays /* n * 8 floats, on ctx's device */,
                                         void *d_radiance /* n * 8 words */, uint32_t n, uint32_t order, void *producer_stream /* as flx_rays_trace_device's */);
flx_status flx_rays_trace_ordered(flx_context *ctx, const flx_trace_params *params, const float *rays /* n * 8 floats */, void *radiance /* n * 8 words */, uint32_t n,
                                  uint32_t order);      /* host arrays */
/* The sort alone, for tests: order[0 .. n) <- the positions 0 .. n - 1 in ascending order of keys[], equal keys in the order given (numpy.argsort(keys,
 * kind="stable")).  Host arrays, staged through the context's memory; it waits.  n from 1 to 2^21, the most rays of a slab; FLX_ERR_INVALID otherwise, or for a
 * NULL array.  Needs no scene. */
flx_status flx_debug_sort_keys(flx_context *ctx, const uint32_t *keys, uint32_t n, uint32_t *order);
/* Bounds and keys alone, for tests: n ray rows and their FLX_RAYS_CLOSEST hit rows (of which words 0 and 3 are read) -> keys[n] and bounds[6] (lo x y z, hi x y z;
 * unused and no numbers where no ray is live), as include/flx_ray_key.h defines them.  Host arrays, staged; it waits.  n and refusals as flx_debug_sort_keys'. */
flx_status flx_debug_hit_keys(flx_context *ctx, const float *rays /* n * 8 floats */, const void *hits /* n * 8 words */, uint32_t n, uint32_t *keys, float bounds[6]);
/* The last traced batch (flx_rays_trace[_device] or the ordered calls; zeros but [1] if none), set only when the whole call succeeded: out[0] whether it was
 * ordered, [1] T, the items a sort workgroup takes, [2] the sort workgroups of its last slab, [3] the sort passes run, [4] n, [5] the live rays of its last slab
 * (rays with a first hit at a finite point), [6] and [7] reserved, zero.  [2], [3] and [5] are zero after an unordered batch.  After an ordered batch it waits for
 * the context's stream. */
flx_status flx_debug_last_ray_order(flx_context *ctx, uint32_t out[8]);
/* The denoise chain's FIVE FILTER PLANES for the caller's rays, and a ray IMAGE traced and denoised: what flx_render_planes_device and flx_render (use_filter = 1)
 * are for the pixels behind the pinhole camera, for any rays — a panorama, a fisheye or orthographic view, a stereo pair, a probe's faces, a hybrid renderer's
 * reflection buffer — at the 1 - 8 samples per ray the renderer is built for.  A ray row and flx_trace_params are flx_rays_trace's.
 * Per ray: hit = rayTracer(origin, direction), exactly as FLX_RAYS_CLOSEST answers it.  A MISS WRITES ZEROS IN ALL FIVE PLANES, as fragment_main does for an
 * uncovered pixel.  A hit is fragment_main with use_filter == 1 and is_temporal == 0 (fragment:601-646): the shader's globals (firstRayLength, glassFilter,
 * originalRMEx, originalTPOx, renderId) are initialised once per ray and THE SAMPLES RUN IN ORDER ON THAT ONE STATE; with c = the samples' sum * (1.0f / samples):
 *   plane 0 renderColor          fract(c), alpha 1
 *   plane 1 renderColorIp        floor(c) / 256, alpha glassFilter
 *   plane 2 renderOriginalColor  originalColor as the last sample left it, alpha min(originalRMEx, firstRayLength) + 1/255
 *   plane 3 renderId             renderId, its w plus 1/255
 *   plane 4 renderOriginalId     (0, 0, 0, originalTPOx + 1/255)
 * — flx_render_planes_device's order, with the oracle's bits.  The ray's origin stands wherever lightTrace uses the camera, the row's two noise words stand in for
 * the pixel's NDC, the direction is used as given: all as in flx_rays_trace.
 * d_planes32: float4[5][n], the values before quantisation; d_planes8: uint32[5][n], each the RGBA8 texel a render target stores of that value (NaN and values
 * <= 0 give 0, values >= 1 give 255, else (uint8)(x * 255 + 0.5f)): what flx_filter_planes_device reads.  Plane p starts at row p * n.  Either may be NULL, not both.
 * flx_rays_image_device: the rays in image order, row 0 on top, n = width * height; the planes go to memory the context owns (grown, never shrunk), the chain follows
 * exactly as flx_filter_planes_device launches it (the reference's frame-0 texture state; it reads width, height and hdr only) and writes float4[height][width].
 * With a camera's rays the image is flx_render's with use_filter = 1, bit for bit wherever rayTracer and a frame's primary walk agree on the first hit.
 * TEMPORAL ACCUMULATION OF RAY IMAGES IS OUT OF SCOPE OF THESE CALLS, which keep nothing from one image to the next (and a loose batch of rays has no history to be
 * matched against).  A ray IMAGE traced again frame after frame has one: flx_rays_image_temporal[_device] (below) accumulates it over time.
 * Ordering, producer_stream, the frame server, lights and transforms uploaded over a running launch, the staging of the host variants (they wait and copy out) and
 * n == 0 (FLX_OK, nothing enqueued, the scene and the params looked at first) are flx_rays_trace_device's and flx_rays_trace's, word for word.  The batch is cut
 * into slabs of at most 2^21 rays; the scratch is the traced batches' hit rows alone, 32 bytes a ray.  (Where scratch, planes or staging must grow, the host waits
 * for the stream first.)
 * Refusals, each with a message of its own and nothing enqueued: flx_rays_trace's for the scene and the params; FLX_ERR_INVALID where both plane pointers are NULL;
 * where width or height is 0 (whatever the rays) or width * height is 2^32 or more; for an array that is NULL, not memory of the context's device, not 16-byte
 * aligned or in an allocation too short; where an output overlaps the rays, or the two outputs each other.  A group has no such call, as it traces no rays. */
flx_status flx_rays_planes_device(flx_context *ctx, const flx_trace_params *params, const void *d_rays /* n * 8 floats, on ctx's device */, uint32_t n,
                                  void *d_planes8 /* uint32[5][n] RGBA8, or NULL */, void *d_planes32 /* float4[5][n] pre-quantisation, or NULL */,
                                  void *producer_stream /* hipStream_t that wrote the rays, or NULL: they are complete */);
flx_status flx_rays_planes(flx_context *ctx, const flx_trace_params *params, const float *rays /* n * 8 floats */, uint32_t n, void *planes8, void *planes32);      /* host arrays */
flx_status flx_rays_image_device(flx_context *ctx, const flx_trace_params *params, int hdr, const void *d_rays /* width * height * 8 floats, on ctx's device */,
                                 uint32_t width, uint32_t height, void *d_out_rgba /* float4[height][width] */, void *producer_stream);
flx_status flx_rays_image(flx_context *ctx, const flx_trace_params *params, int hdr, const float *rays, uint32_t width, uint32_t height, float *out_rgba);      /* host arrays */
/* The last planes or image call (zeros if none): out[0] its slabs, [1] the rays of a full slab, [2] workgroups of the last slab's planes kernel, [3] whether its
 * bounce walks went in lockstep, [4] n, [5] samples, [6] workgroups of the last slab's first-hit launch, [7] the rays a wave draws with one atomic.  It waits for
 * nothing. */
flx_status flx_debug_last_ray_planes(flx_context *ctx, uint32_t out[8]);
/* RAY IMAGES OVER TIME: temporal accumulation (config.temporal of the reference, on by default there) for a ray image — the same width * height rays in the same
 * order, traced again frame after frame — as flx_render with is_temporal = 1 accumulates the frames behind the pinhole camera.  The reference's temporal pass is
 * strictly per pixel and reads nothing of a camera; the id it matches on, renderLocationId (fragment:640-642), is defined for any ray.
 * The context keeps FLX_RAY_HISTORIES histories, named by `history`.  A history holds four rings of N RGBA8 planes of width * height texels: colour, colour integer
 * part, location id, original id.  N = temporal_samples by flx_frame_params' rule (<= 0 -> 4, > 16 -> 16).
 * One call: ray rows, flx_trace_params and the image order (row 0 on top) are flx_rays_image's.  The caller passes random_seed; the reference passes
 * frame % temporalSamples.  The first hit is rayTracer(origin, direction) exactly as FLX_RAYS_CLOSEST answers it.  A HIT is fragment_main with is_temporal == 1 and
 * use_filter as given, the ray's origin where a frame has its camera, the row's two noise words where a frame has the pixel's NDC: with use_filter == 1 the five
 * targets flx_rays_planes writes; with use_filter == 0, c = the samples' average, renderColor = (fract(c * originalColor), 1) and renderColorIp =
 * (floor(c * originalColor) / 256, 1); and in both modes a sixth target, over the hit entry's object-space vertices a, b, c:
 *   rel = (a * (1 - u - v) + b * u) + c * v;  div = 2 * distance(rel, origin);  renderLocationId = (mod(rel, div) / div, 1/255)
 * A MISS WRITES ZEROS in all six.  The call rotates the ring (the oldest slot becomes the head), stores the new frame's four texels at the head and runs the
 * reference's temporal pass on the texel of the ray's own index in every slot: the slots whose location id equals the new frame's add their colour, those whose
 * original id equals it add their glass filter (slots visited in groups of four, vec4(0) standing in for slots at or beyond N, which an all-zero id matches too,
 * as in the shader).  Without the filter the averaged canvas colour is the output, tone-mapped where hdr == 1.  With it the pass' five RGBA8 targets feed the
 * denoise chain exactly as flx_filter_planes_device starts it (frame-0 texture state; it reads width, height and hdr only).  With a camera's rays, seed f % N,
 * the sequence is flx_render's temporal sequence after flx_temporal_reset, bit for bit wherever rayTracer and a frame's primary walk agree on the first hit.
 * The whole job runs in the planes kernel, in the lane that owns the ray (csrc/flx_rays_planes.hip): no float G-buffer, no second pass over the image.
 * A history is keyed by (width, height, N): a call with another key starts that history afresh — zero planes, head 0 —, as a resize does for frames;
 * flx_rays_history_reset does the same on demand (history -1: all of them) and releases the rings' memory; it waits for the context's stream.  The rings are
 * allocated on first use and freed with the context.  The frames' own history (flx_temporal_reset) and these never touch each other.  There is no reprojection
 * under motion, as the reference has none: a ray whose location id changes starts over.
 * Ordering, producer_stream, the frame server and the staging of the host variant are flx_rays_image_device's and flx_rays_image's, word for word; calls on one
 * history are ordered by the context's stream.  (Where a history is (re)allocated the host waits for the stream first.)
 * Refusals, each with a message of its own, nothing enqueued AND THE HISTORY EXACTLY WHAT IT WAS, neither rotated nor re-keyed: flx_rays_image's for the scene, the
 * params, the size and the arrays; temporal NULL; history outside 0 .. FLX_RAY_HISTORIES - 1; use_filter or hdr not 0 or 1; flx_rays_history_reset with history
 * below -1 or above 7.  A group has no such call, as it traces no rays. */
#define FLX_RAY_HISTORIES 8
typedef struct flx_ray_temporal {
  int32_t history;           /* 0 .. FLX_RAY_HISTORIES - 1: which of the context's ray-image histories */
  int32_t temporal_samples;  /* depth N, by flx_frame_params' rule: <= 0 -> 4, > 16 -> 16 */
  int32_t use_filter;        /* 0: the temporal pass' canvas colour; 1: the denoise chain follows it */
  int32_t hdr;
} flx_ray_temporal;
flx_status flx_rays_image_temporal_device(flx_context *ctx, const flx_trace_params *params, const flx_ray_temporal *temporal,
                                          const void *d_rays /* width * height * 8 floats, on ctx's device */, uint32_t width, uint32_t height,
                                          void *d_out_rgba /* float4[height][width] */, void *producer_stream);
flx_status flx_rays_image_temporal(flx_context *ctx, const flx_trace_params *params, const flx_ray_temporal *temporal, const float *rays, uint32_t width, uint32_t height,
                                   float *out_rgba);      /* host arrays */
flx_status flx_rays_history_reset(flx_context *ctx, int history /* -1: all of them */);
/* The last temporal ray image (zeros if none): out[0] its slabs, [1] the rays of a full slab, [2] N, [3] the history, [4] n, [5] samples, [6] the ring's head after
 * the call, [7] 1 if the temporal pass ran inside the planes kernel.  It waits for nothing. */
flx_status flx_debug_last_ray_temporal(flx_context *ctx, uint32_t out[8]);
/* CAMERAS: the rays of a camera made ON THE DEVICE, so that a ray image needs no rays from the host — 32 bytes a pixel that would otherwise be built by the caller
 * and cross the bus for every image.  Five projections; the arithmetic is include/flx_camera.h's, float32 with one rounding per operation, shared by the kernel
 * (csrc/flx_camera.hip: k_camera_rays) and by a CPU reference, so rows are defined bit for bit.
 * Pixel (px, row) of a width x height image, row 0 on top, py = height - 1 - row:
 *   sx = ((float)px + (0.5f + jitter[0])) / (float)width * 2.0f - 1.0f, sy likewise from py, height and jitter[1];
 *   THE ROW'S NOISE WORDS (3 and 7) ARE THE SAME EXPRESSIONS WITH ZERO JITTER: the pixel's NDC as a frame computes it, so a camera's rays draw a frame's random
 *   numbers whatever the jitter.  world(l) = (right * l.x + up * l.y) + forward * l.z per component; every direction ends in normalize3, v / sqrt((x x + y y) + z z).
 *   PINHOLE       d = normalize3(V^-1 (sx, sy, 1)), V = basis = flx_frame_params.view_matrix, inverted once on the host (flx_invert3x3); origin = position.  With
 *                 zero jitter these are the bits of a frame's primary ray.
 *   PANORAMA      equirectangular: lon = sx * (0.5f * extent[0]), lat = sy * (0.5f * extent[1]); l = (sin lon cos lat, sin lat, cos lon cos lat); d = normalize3(world(l))
 *   FISHEYE       equidistant: q = sqrt(sx sx + sy sy), theta = q * (0.5f * extent[0]); l = (sin theta * sx / q, sin theta * sy / q, cos theta), (0, 0, 1) at q == 0;
 *                 d = normalize3(world(l)).  NOT MASKED: the corners beyond the image circle continue the mapping (q up to sqrt 2); mask q > 1 yourself.
 *   ORTHOGRAPHIC  origin = position + (right * (sx * (0.5f * extent[0])) + up * (sy * (0.5f * extent[1]))); d = normalize3(forward)
 *   CUBE_FACE     l = F + R sx + U sy with the face's axes below, whose entries are 0 or +-1: l's components are exactly +-1, +-sx, +-sy, and the shared edge of two
 *                 faces gets the same l from both.  d = normalize3(world(l)).
 *                   face 0 (+x): F (1,0,0) R (0,0,-1) U (0,1,0)     1 (-x): F (-1,0,0) R (0,0,1) U (0,1,0)     2 (+y): F (0,1,0) R (1,0,0) U (0,0,-1)
 *                   face 3 (-y): F (0,-1,0) R (1,0,0) U (0,0,1)     4 (+z): F (0,0,1) R (1,0,0) U (0,1,0)      5 (-z): F (0,0,-1) R (-1,0,0) U (0,1,0)
 * flx_camera_rays_device writes ray rows (flx_rays_trace's: origin, noise x, direction, noise y) for n_cameras cameras of one image size in ONE launch — a stereo
 * pair, a probe's six faces, a mixed batch: camera c's rows start at row c * w * h.  region = { x0, y0, w, h } of the image, or NULL for all of it: only the
 * region's rays are written, in row order, and they are BIT FOR BIT the rows of the same pixels of the whole image (sx, sy and the noise words are always the full
 * image's).  It needs a context for its device and stream and NO SCENE.  Ordering is flx_rays_cast_device's: enqueued on the context's stream with no wait of
 * the host, behind a frame server's launch.  Trace, planes and surface rows of a camera's rays are two calls on the device: this one, then flx_rays_trace_device,
 * flx_rays_planes_device or flx_rays_surface_device with producer_stream NULL.  flx_camera_rays is the same into host memory, staged through memory the context
 * owns; it waits and copies out.
 * flx_camera_image[_temporal]_device: ONE camera's rays into a buffer the context owns (grown, never shrunk), then exactly what flx_rays_image_device /
 * flx_rays_image_temporal_device run on width * height rays: the image is theirs bit for bit, and ordering, the frame server, slabs, histories and refusals
 * are theirs word for word.  The host variants stage the image only.
 * Refusals, each FLX_ERR_INVALID with a message of its own and nothing enqueued: cameras NULL or n_cameras 0; width or height 0; n_cameras * width * height of
 * 2^32 or more; a region that is empty or leaves the image; a projection that is none of the five; a face outside 0 .. 5; a field (position, basis, extent,
 * jitter) that is not finite; a jitter outside [-0.5, 0.5]; an extent <= 0 where the projection reads it; an output that is NULL, not memory of the context's
 * device, not 16-byte aligned or too short.  The image calls return FLX_ERR_NO_SCENE before a scene and transforms are up and refuse everything
 * flx_rays_image[_temporal] refuses.  A group has no such call, as it traces no rays. */
#define FLX_CAMERA_PINHOLE      0
#define FLX_CAMERA_PANORAMA     1
#define FLX_CAMERA_FISHEYE      2
#define FLX_CAMERA_ORTHOGRAPHIC 3
#define FLX_CAMERA_CUBE_FACE    4
typedef struct flx_camera {
  int32_t projection;   /* FLX_CAMERA_* */
  int32_t face;         /* CUBE_FACE: 0 .. 5 = +x -x +y -y +z -z; 0 otherwise */
  float position[3];
  float basis[9];       /* PINHOLE: the frame params' view_matrix, used exactly as a frame uses it.  Others: rows right, up, forward in world space, used as given
                           (neither normalised nor orthogonalised) */
  float extent[2];      /* PANORAMA: the horizontal and vertical angle covered (rad; 2 pi, pi = the sphere).  FISHEYE: [0] the full field of view across the
                           image's width (rad), [1] unused.  ORTHOGRAPHIC: width, height of the window in world units.  PINHOLE, CUBE_FACE: unused */
  float jitter[2];      /* sub-pixel offset in pixels, each in [-0.5, 0.5] */
} flx_camera;
flx_status flx_camera_rays_device(flx_context *ctx, const flx_camera *cameras /* host */, uint32_t n_cameras, uint32_t width, uint32_t height,
                                  const uint32_t region[4] /* x0, y0, w, h, or NULL */, void *d_rays /* n_cameras * w * h * 8 floats, on ctx's device */);
flx_status flx_camera_rays(flx_context *ctx, const flx_camera *cameras, uint32_t n_cameras, uint32_t width, uint32_t height, const uint32_t region[4], float *rays);      /* host array out */
flx_status flx_camera_image_device(flx_context *ctx, const flx_trace_params *params, int hdr, const flx_camera *camera, uint32_t width, uint32_t height,
                                   void *d_out_rgba /* float4[height][width] */);
flx_status flx_camera_image(flx_context *ctx, const flx_trace_params *params, int hdr, const flx_camera *camera, uint32_t width, uint32_t height, float *out_rgba);      /* host array out */
flx_status flx_camera_image_temporal_device(flx_context *ctx, const flx_trace_params *params, const flx_ray_temporal *temporal, const flx_camera *camera, uint32_t width,
                                            uint32_t height, void *d_out_rgba /* float4[height][width] */);
flx_status flx_camera_image_temporal(flx_context *ctx, const flx_trace_params *params, const flx_ray_temporal *temporal, const flx_camera *camera, uint32_t width,
                                     uint32_t height, float *out_rgba);      /* host array out */
/* LIGHT PROBES: probe positions in, one spherical-harmonic (SH) row per probe out, and nothing but positions and SH rows crossing the bus.  A probe is a
 * position and a face size w (1 .. 256); its R = 6 w w texels are six w x w cube faces, t = (face * w + row) * w + px, the faces in flx_camera's cube-face order,
 * row 0 on top.  Every float is defined bit for bit in include/flx_probe.h, float32 with one rounding per operation, which the kernels (csrc/flx_probes.hip:
 * k_probe_rays, k_probe_sh) and a CPU reference compile alike.
 * THE RAY of texel t: origin and direction are flx_camera_ray's for a FLX_CAMERA_CUBE_FACE camera of that face with the identity basis, zero jitter, the probe's
 * position and size w x w, bit for bit.  THE NOISE WORDS ARE NOT THE CAMERA'S (the six faces of a probe would share them, and equal noise words draw equal random
 * numbers): with cols = ceil(sqrt(R)) and rows = ceil(R / cols) in integers, noise x is the camera's NDC expression of (t % cols, cols) and noise y that of
 * (t / cols, rows), zero jitter.  Every ray of a probe draws its own random numbers and every probe draws the same ones as every other probe: a probe's row
 * depends on its position, w and the params, and on nothing else in the call.
 * THE WEIGHT of texel t, with sx, sy as the camera computes them: q = (1 + sx sx) + sy sy, d_omega = cell / (q sqrt(q)), cell = 4 / (w w).  THE WEIGHTS ARE NOT
 * RENORMALISED: their sum is 4 pi (1 + e_w), e_w = 0.910, 0.0396, 0.0281, 0.0153, 0.00383, 0.00096, 0.00024 for w = 1, 2, 3, 4, 8, 16, 32; the row carries the sum.
 * THE BASIS: real SH bands 0 - 2 of the direction (x, y, z): K0; K1 y, K1 z, K1 x; K2 x y, K2 y z, K3 (3 z z - 1), K2 x z, K4 (x x - y y).
 * THE TERMS of texel t: its radiance row is flx_rays_trace's.  It is a hit where word 3 is not 0.0f; then L = words 0 .. 2 and s = word 4, the first-hit distance;
 * otherwise L = params->sky (a miss row is all zeros, as in a frame: sky lets an open scene have an environment, sky = 0 keeps the frame's meaning).  Coefficient
 * i, channel c gets L_c (b_i d_omega); four more sums get d_omega (all texels), d_omega (hits only), d_omega s and d_omega (s s) (hits only): the visibility
 * moments a probe volume uses against leaking.
 * THE ORDER OF THE 31 SUMS is part of the definition: 64 slots; slot j adds its texels j, j + 64, j + 128, .. in ascending order onto 0.0f; then for off = 1, 2, 4,
 * 8, 16, 32 every slot becomes v[j] + v[j ^ off], after which all slots are equal.  A sum that meets a NaN is some NaN; its payload is not defined.
 * THE SH ROW: 144 bytes, nine float4; coefficient i in words 4 i .. 4 i + 2; word 4 i + 3 holds for i = 0 .. 3 the four extra sums in the order above and 0.0f
 * for i >= 4.
 * flx_probe_irradiance (a plain host function, no context, no device): E_c = ((A0 (sh[c] b0)) + A1 ((sh[4 + c] b1 + sh[8 + c] b2) + sh[12 + c] b3)) + A2 (the five
 * band-2 products summed in ascending i), A0 = pi, A1 = 2 pi / 3, A2 = pi / 4 as float32, b_i the basis at n (used as given), one rounding per operation.
 * flx_probe_rays_device writes the n_probes * R ray rows of the probes at d_positions (rows of 4 floats, word 3 ignored), probe p's rows from row p * R; it needs
 * NO SCENE, like flx_camera_rays_device.  POSITIONS ON THE DEVICE CANNOT BE LOOKED AT: a position that is not finite is traced as given.
 * flx_probe_reduce_device reduces n_probes * R radiance rows to n_probes SH rows.  flx_probes_sh_device is the whole path: it cuts the probes into chunks of
 * max(1, 2^21 / R) probes — the most rays of a trace slab; flx_debug_set_probe_chunk sets a smaller number, 0 the default — and runs per chunk, on the context's
 * stream, k_probe_rays into a buffer the context owns, flx_rays_trace_ordered_device (params->order: 0 or FLX_TRACE_ORDER_HITS, the same rows either way) from
 * there into a second one, and k_probe_sh into the chunk's rows of d_sh.  Both buffers are grown and never shrunk; together they end at 2^21 rays x 64 bytes.
 * The result is bit for bit that of the three calls made one after the other, whatever the chunk.
 * Ordering, producer_stream, the frame server and n_probes == 0 (FLX_OK, nothing enqueued, the scene and the params looked at first) are flx_rays_trace_device's,
 * word for word: enqueued on the context's stream with no wait of the host, frames in flight finish unchanged.  (Where a buffer must grow, the host waits for the
 * stream first.)  flx_probe_rays, flx_probe_reduce and flx_probes_sh are the same for host arrays, staged through memory the context owns; they wait and copy out.
 * Refusals, each with a message of its own, nothing enqueued and the output untouched: for flx_probes_sh[_device] the scene's and the trace params', asked of
 * flx_rays_trace_ordered_device in its words; then FLX_ERR_INVALID for params NULL; face_size 0 or above 256; a bit of order beyond FLX_TRACE_ORDER_HITS; a sky or
 * reserved value that is not finite; n_probes * R of 2^32 or more (the ray and reduce calls, which handle that many rows in one piece); an array that is NULL, not
 * memory of the context's device, not 16-byte aligned, in an allocation too short, or that overlaps the other.  A group has no such call, as it traces no rays. */
typedef struct flx_probe_params {
  uint32_t face_size;   /* w: 1 .. 256 texels along a cube face's edge */
  uint32_t order;       /* 0 or FLX_TRACE_ORDER_HITS, handed to flx_rays_trace_ordered_device */
  float sky[3];         /* L of a texel whose ray hits nothing */
  float reserved;       /* 0; must be finite */
} flx_probe_params;
flx_status flx_probe_rays_device(flx_context *ctx, const void *d_positions /* n_probes * 4 floats, word 3 ignored */, uint32_t n_probes, uint32_t face_size,
                                 void *d_rays /* n_probes * 6 w w * 8 floats */, void *producer_stream /* hipStream_t that wrote the positions, or NULL */);
flx_status flx_probe_rays(flx_context *ctx, const float *positions, uint32_t n_probes, uint32_t face_size, float *rays);      /* host arrays */
flx_status flx_probe_reduce_device(flx_context *ctx, const void *d_radiance /* n_probes * 6 w w rows of 32 bytes */, uint32_t n_probes, const flx_probe_params *params,
                                   void *d_sh /* n_probes * 9 float4 */, void *producer_stream /* hipStream_t that wrote the radiance, or NULL */);
flx_status flx_probe_reduce(flx_context *ctx, const void *radiance, uint32_t n_probes, const flx_probe_params *params, float *sh);      /* host arrays */
flx_status flx_probes_sh_device(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const void *d_positions /* n_probes * 4 floats */,
                                uint32_t n_probes, void *d_sh /* n_probes * 9 float4 */, void *producer_stream);
flx_status flx_probes_sh(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const float *positions, uint32_t n_probes, float *sh);      /* host arrays */
void flx_probe_irradiance(const float sh[36], const float n[3], float out[3]);
flx_status flx_debug_set_probe_chunk(flx_context *ctx, uint32_t probes /* 0: the default */);
/* The last flx_probes_sh[_device] (zeros if none): out[0] its chunks, [1] the probes of a full chunk, [2] the face size, [3] n_probes, [4] order, [5] the rays of a
 * probe, [6] workgroups of the last chunk's k_probe_sh, [7] zero.  It waits for nothing. */
flx_status flx_debug_last_probes(flx_context *ctx, uint32_t out[8]);
/* PROBE VOLUMES: a regular grid of light probes, baked into SH rows on the device, and THE LOOKUP that joins them with surface rows: for every surface point the
 * irradiance the grid gives it.  A hybrid renderer is three device calls with no host arithmetic in between: flx_volume_bake_device, flx_frame_surface_device (or
 * the rasterizer), flx_volume_irradiance_device — or the last two in one, flx_frame_irradiance_device.  Every float is defined bit for bit in include/flx_volume.h,
 * float32 with one rounding per operation, which the kernels (csrc/flx_volume.hip: k_volume_positions, k_volume_irradiance) and a CPU reference compile alike.
 * THE GRID (flx_volume_grid): probe (ix, iy, iz) has index p = (iz ny + iy) nx + ix and, per axis, the position origin + (float)i spacing (the product, then the sum).
 * THE LOOKUP takes a FLX_SURFACE_POSITION row (x, hit) and a FLX_SURFACE_NORMAL row (n, .); the normal is used as given, not normalised.
 *   1. A miss — word 3 of the position equal to 0.0f — gives four 0.0f and reads no probe.
 *   2. x' = n normal_bias + x per axis (the product, then the sum).
 *   3. g = (x' - origin) / spacing; g = (g >= 0) ? g : 0 (a NaN becomes 0); g = (g <= (float)(count - 1)) ? g : (float)(count - 1).
 *   4. i = min((uint32_t)g, count - 2) where count >= 2, else 0; f = g - (float)i.
 *   5. Corner k = kx + 2 ky + 4 kz, k = 0 .. 7 ascending, is the probe at min(i_a + k_a, count_a - 1) per axis.  t = (tx ty) tz, t_a = k_a ? f_a : 1 - f_a.
 *      d = probe - x', dist = sqrt((dx dx + dy dy) + dz dz), dir = d / dist (three quotients; zero where dist == 0), c = (((dirx nx + diry ny) + dirz nz) + 1) 0.5,
 *      wb = c c + 0.2.  wv = 1 unless FLX_VOLUME_VISIBILITY is set and the row's sh[7] > 0; then mean = sh[11] / sh[7], mean2 = sh[15] / sh[7],
 *      var = |mean2 - mean mean|, and where dist > mean: delta = dist - mean, den = var + delta delta, ch = den > 0 ? var / den : 0, wv = max((ch ch) ch, floor)
 *      with max(a, b) = (a < b) ? b : a; otherwise wv = 1.  w_k = (t wb) wv, E_k = flx_probe_irradiance's of row k and n.
 *   6. W and S_c start at 0.0f and add w_k and w_k E_k,c (the product first) in ascending k — also where t == 0: one path.
 *   7. The row is (S_0 / W, S_1 / W, S_2 / W, W); four 0.0f where W <= 0.  A NaN W is neither > 0 nor <= 0 and takes the quotients: a NaN anywhere gives some NaN.
 * WHERE THE ISSUE OF AN ORDER WAS OPEN it is fixed as written above: products before the sums that take them, sums of three left to right, x before y before z.
 * THE MOMENTS ARE THOSE OF THE WHOLE SPHERE, not of a direction: the visibility weight is isotropic (include/flx_volume.h says what that costs); the directional
 * visibility map is include/flx_volume_map.h's and has calls of its own ("directional visibility" below), and the flag turns the test off.
 * flx_volume_positions_device writes the grid's nx ny nz positions as rows of 4 floats (word 3 is 0.0f), flx_probes_sh_device's input; it needs NO SCENE.
 * flx_volume_bake_device writes them into a buffer the context owns and runs flx_probes_sh_device from there — there is no second probe path —: bit for bit the
 * two calls one after the other.  flx_volume_irradiance_device is the lookup for n points: d_sh the grid's SH rows, d_positions and d_normals planes of n rows of 16
 * bytes, d_out n rows of 16 bytes; it needs NO SCENE.  flx_rays_irradiance_device and flx_frame_irradiance_device take the two planes (FLX_SURFACE_POSITION |
 * FLX_SURFACE_NORMAL) with flx_rays_surface_device / flx_frame_surface_device AS THEY STAND into a buffer the context owns (grown and never shrunk) and the lookup
 * follows on the same stream: bit for bit the surface call followed by flx_volume_irradiance_device.  A ray batch goes in slabs of at most 2^21 rays
 * (flx_debug_set_trace_slab lowers it for tests), so that the buffer ends at 2^21 x 32 bytes; a frame's holds width x height x 32 bytes.
 * Ordering, producer_stream, the frame server and n == 0 (FLX_OK, nothing enqueued, the grid and the scene looked at first) are flx_rays_trace_device's, word for
 * word: enqueued on the context's stream with no wait of the host, frames in flight finish unchanged.  (Where a buffer must grow, the host waits for the stream
 * first.)  The calls without _device are the same for host arrays, staged through memory the context owns; they wait and copy out.  flx_volume_irradiance_of is a
 * plain host function (no context, no device): the lookup of one point over SH rows in host memory.  A group has no such call.
 * Refusals, each FLX_ERR_INVALID with a message of its own, nothing enqueued and the output untouched: a NULL grid (or NULL probe params: flx_probes_sh's words); a
 * count of 0; nx ny nz of 2^31 or more; an origin or a spacing that is not finite; a spacing <= 0; a normal_bias that is negative or not finite; a floor outside
 * [0, 1] or not finite; unknown flag bits; a reserved word that is not 0; an array that is NULL, not memory of the context's device, not 16-byte aligned, in an
 * allocation too short for its rows, or that overlaps another of the call.  The scene's, the trace params', the probe params' and the surface calls' own refusals
 * are passed through in their own words (those calls are asked first). */
#define FLX_VOLUME_VISIBILITY 1u
typedef struct flx_volume_grid {
  float origin[3];      /* probe (0, 0, 0) */
  float spacing[3];     /* > 0 per axis */
  uint32_t count[3];    /* nx, ny, nz: at least 1 each, nx ny nz below 2^31 */
  float normal_bias;    /* >= 0: how far along the normal the sample point is lifted off the surface */
  float floor;          /* 0 .. 1: the least visibility weight */
  uint32_t flags;       /* FLX_VOLUME_VISIBILITY or 0 */
  uint32_t reserved;    /* 0 */
} flx_volume_grid;
flx_status flx_volume_positions_device(flx_context *ctx, const flx_volume_grid *grid, void *d_positions /* nx ny nz * 4 floats */, void *producer_stream /* hipStream_t that last used d_positions, or NULL */);
flx_status flx_volume_positions(flx_context *ctx, const flx_volume_grid *grid, float *positions);      /* host array */
flx_status flx_volume_bake_device(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid,
                                  void *d_sh /* nx ny nz * 9 float4 */, void *producer_stream);
flx_status flx_volume_bake(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, float *sh);      /* host array */
flx_status flx_volume_irradiance_device(flx_context *ctx, const flx_volume_grid *grid, const void *d_sh /* nx ny nz * 9 float4 */, const void *d_positions /* n * 4 floats */,
                                        const void *d_normals /* n * 4 floats */, uint32_t n, void *d_out /* n * 4 floats */, void *producer_stream /* hipStream_t that wrote the inputs, or NULL */);
flx_status flx_volume_irradiance(flx_context *ctx, const flx_volume_grid *grid, const float *sh, const float *positions, const float *normals, uint32_t n, float *out);      /* host arrays */
flx_status flx_rays_irradiance_device(flx_context *ctx, int32_t texture_width, const flx_volume_grid *grid, const void *d_sh, const void *d_rays /* n * 8 floats */, uint32_t n,
                                      void *d_out /* n * 4 floats */, void *producer_stream);
flx_status flx_rays_irradiance(flx_context *ctx, int32_t texture_width, const flx_volume_grid *grid, const float *sh, const float *rays, uint32_t n, float *out);      /* host arrays */
flx_status flx_frame_irradiance_device(flx_context *ctx, const flx_frame_params *params, const flx_volume_grid *grid, const void *d_sh, void *d_out /* width * height * 4 floats */);
flx_status flx_frame_irradiance(flx_context *ctx, const flx_frame_params *params, const flx_volume_grid *grid, const float *sh, float *out);      /* host arrays */
void flx_volume_irradiance_of(const flx_volume_grid *grid, const float *sh_rows, const float position[4], const float normal[4], float out[4]);
/* The last lookup — flx_volume_irradiance[_device], flx_rays_irradiance[_device] or flx_frame_irradiance[_device] — (zeros if none): out[0] its points, [1] its slabs,
 * [2] the points of a full slab, [3] the grid's probes, [4] the grid's flags, [5] 1 for rays, 2 for a frame, 0 for planes of the caller's, [6] workgroups of the last
 * slab's k_volume_irradiance, [7] zero.  (The kernel has one path: there is no count of waves by path to report.)  It waits for nothing. */
flx_status flx_debug_last_volume(flx_context *ctx, uint32_t out[8]);
/* DIRECTIONAL VISIBILITY: an octahedral map of filtered distance moments per probe, reduced on the device from the radiance rows the SH row is reduced from, baked
 * with the volume, and read by the lookup in place of the SH row's whole-sphere moments — the cure for light leaking through walls and for open rooms dimmed for
 * nothing.  All of it is calls of its own beside the ones above, which do what they did.  Every float is defined bit for bit in include/flx_volume_map.h, which the
 * kernels (csrc/flx_volume_map.hip: k_probe_map; csrc/flx_volume.hip: k_volume_irradiance_map) and a CPU reference compile alike.
 * THE MAP (flx_volume_map): m x m bins, bin b = by m + bx, each a row of 4 floats; probe p's rows start at row p m m of the maps array.  The centre of bin (bx, by)
 * in the octahedral square is u = ndc(bx, m), v = ndc(by, m), ndc(i, m) = (((float)i + 0.5) / (float)m) 2 - 1 (flx_camera_ndc).
 * DECODE (u, v) to a direction: z = (1 - |u|) - |v|; where z < 0: x = (1 - |v|) sgn(u), y = (1 - |u|) sgn(v), sgn(a) = (a >= 0) ? 1 : -1, the products exact;
 *   otherwise x = u, y = v; l = sqrt((x x + y y) + z z); three quotients by l.
 * ENCODE a direction to a bin: l1 = (|x| + |y|) + |z|; where not l1 > 0 the bin is 0; px = x / l1, py = y / l1; where z < 0 the decode's two expressions on (px, py);
 *   per axis g = ((p + 1) 0.5) (float)m, g = (g >= 0) ? g : 0 (a NaN becomes 0), the index min((uint32_t)g, m - 1).  No index leaves the map.
 * THE TERMS of cube texel t for a bin of direction b: direction d and d_omega of the texel are the probe reduction's; c = (dx bx + dy by) + dz bz, c = (c > 0) ? c : 0,
 *   c squared `sharpness` times, g = d_omega c.  The texel is a hit where word 3 of its radiance row is not 0.0f; s is word 4.  The bin's row is (sum of g over hits,
 *   of g s over hits, of g (s s) over hits, of g over all texels); a miss adds 0.0f to the first three.
 * THE ORDER OF THE FOUR SUMS is the probe reduction's, word for word: 64 slots; slot j adds its texels j, j + 64, .. in ascending order onto 0.0f; then for off = 1,
 *   2, 4, 8, 16, 32 every slot becomes v[j] + v[j ^ off].  A sum that meets a NaN is some NaN.
 * THE DIRECTIONAL WEIGHT: with dir of step 5 of the lookup above (from the sample point to the probe), q = the row of the bin of (-dir0, -dir1, -dir2) — the nearest
 *   bin —; wv = 1 unless FLX_VOLUME_VISIBILITY is set and q[0] > 0; then mean = q[1] / q[0], mean2 = q[2] / q[0], and from there step 5's text unchanged.  A bin that
 *   nothing hit leaves the probe fully visible in that direction.  Everything else of the lookup is as above.
 * WHERE THE ISSUE OF AN ORDER WAS OPEN it is fixed as written here: x before y before z, sums of three left to right, the fold's operands 1 - |v| and 1 - |u| each
 *   one difference, s s before its product with g, by before bx only in b = by m + bx.
 * LEFT OUT: bilinear taps between bins, map borders, maps for groups of GPUs.  (Hysteresis between bakes: "volume updates" below; probe relocation: "probe
 * relocation" below them.)
 * flx_probe_map_device reduces n_probes * 6 w w radiance rows to n_probes * m m map rows; it needs NO SCENE.  flx_probes_sh_map_device is flx_probes_sh_device's
 * chunk loop — the same function — with k_probe_map enqueued beside k_probe_sh on each chunk's radiance: bit for bit the separate calls' rows, whatever the chunk.
 * flx_volume_bake_map_device is flx_volume_bake_device with maps.  flx_volume_irradiance_map_device, flx_rays_irradiance_map_device and
 * flx_frame_irradiance_map_device are their siblings plus (map, d_maps), one implementation behind both.  flx_volume_irradiance_map_of is the lookup of one point on
 * the host.  Ordering, producer_stream, the frame server and n == 0 are the siblings'.  The calls without _device are the same for host arrays.
 * Refusals, each FLX_ERR_INVALID with a message of its own, nothing enqueued and the outputs untouched, asked after the siblings' own, which pass through in their
 * words: map NULL; size 0 or above 16; sharpness above 8; a reserved word that is not 0; n_probes * m * m of 2^31 rows or more (a maps array ends below 2^35 bytes);
 * a maps array that is NULL, not memory of the context's device, not 16-byte aligned, in an allocation too short, or that overlaps another array of the call. */
typedef struct flx_volume_map {
  uint32_t size;        /* m: 1 .. 16 bins along the octahedral square's edge */
  uint32_t sharpness;   /* k: 0 .. 8, the filter's exponent is 2^k */
  uint32_t reserved[2]; /* 0 */
} flx_volume_map;
flx_status flx_probe_map_device(flx_context *ctx, const void *d_radiance /* n_probes * 6 w w rows of 32 bytes */, uint32_t n_probes, uint32_t face_size, const flx_volume_map *map,
                                void *d_maps /* n_probes * m m float4 */, void *producer_stream /* hipStream_t that wrote the radiance, or NULL */);
flx_status flx_probe_map(flx_context *ctx, const void *radiance, uint32_t n_probes, uint32_t face_size, const flx_volume_map *map, float *maps);      /* host arrays */
flx_status flx_probes_sh_map_device(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_map *map, const void *d_positions,
                                    uint32_t n_probes, void *d_sh /* n_probes * 9 float4 */, void *d_maps /* n_probes * m m float4 */, void *producer_stream);
flx_status flx_probes_sh_map(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_map *map, const float *positions, uint32_t n_probes,
                             float *sh, float *maps);      /* host arrays */
flx_status flx_volume_bake_map_device(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, const flx_volume_map *map,
                                      void *d_sh, void *d_maps, void *producer_stream);
flx_status flx_volume_bake_map(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, const flx_volume_map *map, float *sh,
                               float *maps);      /* host arrays */
flx_status flx_volume_irradiance_map_device(flx_context *ctx, const flx_volume_grid *grid, const void *d_sh, const void *d_positions, const void *d_normals, uint32_t n, void *d_out,
                                            const flx_volume_map *map, const void *d_maps /* nx ny nz * m m float4 */, void *producer_stream);
flx_status flx_volume_irradiance_map(flx_context *ctx, const flx_volume_grid *grid, const float *sh, const float *positions, const float *normals, uint32_t n, float *out,
                                     const flx_volume_map *map, const float *maps);      /* host arrays */
flx_status flx_rays_irradiance_map_device(flx_context *ctx, int32_t texture_width, const flx_volume_grid *grid, const void *d_sh, const void *d_rays, uint32_t n, void *d_out,
                                          const flx_volume_map *map, const void *d_maps, void *producer_stream);
flx_status flx_rays_irradiance_map(flx_context *ctx, int32_t texture_width, const flx_volume_grid *grid, const float *sh, const float *rays, uint32_t n, float *out,
                                   const flx_volume_map *map, const float *maps);      /* host arrays */
flx_status flx_frame_irradiance_map_device(flx_context *ctx, const flx_frame_params *params, const flx_volume_grid *grid, const void *d_sh, void *d_out, const flx_volume_map *map,
                                           const void *d_maps);
flx_status flx_frame_irradiance_map(flx_context *ctx, const flx_frame_params *params, const flx_volume_grid *grid, const float *sh, float *out, const flx_volume_map *map,
                                    const float *maps);      /* host arrays */
void flx_volume_irradiance_map_of(const flx_volume_grid *grid, const flx_volume_map *map, const float *sh_rows, const float *map_rows, const float position[4], const float normal[4],
                                  float out[4]);
/* The last map reduction — flx_probe_map[_device], or the last chunk's of flx_probes_sh_map[_device] / flx_volume_bake_map[_device] — (zeros if none): out[0] its
 * probes (of the whole call), [1] m, [2] k, [3] launches of k_probe_map (of the last chunk), [4] workgroups of its last launch, [5] the face size, [6], [7] zero.  It
 * waits for nothing. */
flx_status flx_debug_last_volume_map(flx_context *ctx, uint32_t out[8]);
/* VOLUME UPDATES: a probe volume that lives over many frames.  Each frame a LIST of its probes is retraced (the caller varies trace->random_seed from update to
 * update; with equal seeds an update is deterministic) and the new rows are blended into the resident ones with a hysteresis, a poisoned new row is rejected, and
 * nothing but the call crosses the bus.  All of it is calls of its own beside the ones above, which do what they did.  Every sum of an SH row and of a map row is
 * linear in the radiance rows, so blending the sums is blending the moments and the lookups read the rows as they always did.  Every float is defined bit for bit in
 * include/flx_volume_update.h, which the kernels (csrc/flx_volume_update.hip: k_volume_positions_list, k_volume_blend) and a CPU reference compile alike.
 * THE LIST: entry j of n_list names the probe d_indices[j] where a list is given, otherwise update->first + j update->stride, computed in 64 bits (a rotating
 *   subset is first = frame % stride, with no list made anywhere).
 * THE STATE of an entry, one uint32 per entry of d_state, the rules tried in this order ("finite": the exponent bits are not all ones):
 *   3 SKIPPED  the index is nx ny nz or more.  Nothing of the volume is read or written; no index leaves the grid.
 *   2 KEPT     any of the 36 words of the NEW SH row is not finite.  The probe's SH row and all its map rows keep their bits.
 *   1 TAKEN    h == 0, or the OLD row's word 3 (the sum of d_omega over all texels) is not > 0 — never baked, zero-initialised, a NaN —, or any old word is not
 *              finite.  The new row's bits are copied.
 *   0 BLENDED  otherwise.  With g = 1 - h computed once, every word is old + ((new - old) g): the difference, the product, the sum.  A word whose new bits equal
 *              its old ones keeps them (so does a row, for every h; -0.0f too).  Overflow of a finite difference is left as IEEE gives it.
 * THE MAP ROWS of a probe follow the probe's state, with two exceptions per row: where the probe blends or takes, a map row with a NEW word that is not finite
 *   keeps its old bits; where the probe blends, a map row with an OLD word that is not finite takes the new bits.
 * THE POSITION of entry j is flx_volume.h's of its probe; a skipped entry gets the position of probe nx ny nz - 1, and the blend ignores its rows.
 * flx_volume_positions_list_device writes the n_list position rows (flx_probes_sh_device's input); it needs NO SCENE.  flx_volume_blend_device blends n_list new
 * SH rows (entry-major: n_list x 9 float4) and, with a map, n_list m m new map rows into the grid's resident rows d_sh (and d_maps), and writes the states where
 * d_state is given; it needs NO SCENE.  flx_volume_update_device is the whole path on the context's stream: k_volume_positions_list into a buffer the context
 * owns, flx_probes_sh_device (flx_probes_sh_map_device with a map) AS IT STANDS from there into two more — there is no second probe path, so its chunks and slabs
 * apply —, and k_volume_blend: bit for bit the three calls one after the other.  The buffers are grown behind one wait and never shrunk.
 * A LIST IN DEVICE MEMORY CANNOT BE LOOKED AT: entries out of range are SKIPPED, and a probe named twice gets one of the possible results, TORN ROWS INCLUDED (two
 * waves write the same rows in no order).  The calls without _device are the same for host arrays, staged through memory the context owns; they wait and copy out,
 * and they REFUSE A DUPLICATE among the entries inside the grid, since they can look.  flx_volume_blend_row_of is a plain host function (no context, no device): one
 * SH row with its bins map rows, updated in place; -> the state.
 * Ordering, producer_stream, the frame server and n_list == 0 (FLX_OK, nothing enqueued, the rules below that need no array looked at first) are
 * flx_probes_sh_device's, word for word: enqueued on the context's stream with no wait of the host, frames in flight finish unchanged.
 * Refusals, each with a message of its own, nothing enqueued and the outputs untouched.  The siblings' come first in their own words: the scene's, the trace
 * params', the probe params' (flx_volume_update only), the grid's, the map's where one is given.  Then FLX_ERR_INVALID for update NULL; a hysteresis that is not
 * finite or outside [0, 1]; a reserved word that is not 0; n_list above nx ny nz; an arithmetic list (no d_indices) with stride 0 and n_list > 1, or whose last
 * entry first + (n_list - 1) stride is nx ny nz or more — the host can see these —; maps without a map, or a map without maps; an array that is NULL, misaligned
 * (16 bytes; 4 for indices and states), leaving the address space, not memory of the context's device, in an allocation too short, or overlapping another array
 * of the call. */
struct flx_volume_update {
  float hysteresis;     /* h: finite, 0 .. 1; 0 takes the new rows, 1 keeps the old ones */
  uint32_t first;       /* the arithmetic list (no d_indices): entry j names probe first + j stride */
  uint32_t stride;
  uint32_t reserved;    /* 0 */
};
#define FLX_VOLUME_UPDATE_STATES 4u      /* 0 blended, 1 taken, 2 kept, 3 skipped */
flx_status flx_volume_positions_list_device(flx_context *ctx, const flx_volume_grid *grid, const struct flx_volume_update *update, const void *d_indices /* n_list uint32, or NULL */,
                                            uint32_t n_list, void *d_positions /* n_list * 4 floats */, void *producer_stream /* hipStream_t that wrote the indices, or NULL */);
flx_status flx_volume_positions_list(flx_context *ctx, const flx_volume_grid *grid, const struct flx_volume_update *update, const uint32_t *indices, uint32_t n_list,
                                     float *positions);      /* host arrays */
flx_status flx_volume_blend_device(flx_context *ctx, const flx_volume_grid *grid, const flx_volume_map *map /* or NULL */, const struct flx_volume_update *update,
                                   const void *d_indices /* n_list uint32, or NULL */, uint32_t n_list, const void *d_new_sh /* n_list * 9 float4 */,
                                   const void *d_new_maps /* n_list * m m float4; NULL without a map */, void *d_sh /* nx ny nz * 9 float4 */,
                                   void *d_maps /* nx ny nz * m m float4; NULL without a map */, void *d_state /* n_list uint32, or NULL */, void *producer_stream);
flx_status flx_volume_blend(flx_context *ctx, const flx_volume_grid *grid, const flx_volume_map *map, const struct flx_volume_update *update, const uint32_t *indices,
                            uint32_t n_list, const float *new_sh, const float *new_maps, float *sh, float *maps, uint32_t *state);      /* host arrays; sh and maps in and out */
flx_status flx_volume_update_device(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, const flx_volume_map *map /* or NULL */,
                                    const struct flx_volume_update *update, const void *d_indices, uint32_t n_list, void *d_sh, void *d_maps, void *d_state, void *producer_stream);
flx_status flx_volume_update(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, const flx_volume_map *map,
                             const struct flx_volume_update *update, const uint32_t *indices, uint32_t n_list, float *sh, float *maps, uint32_t *state);      /* host arrays; sh and maps in and out */
uint32_t flx_volume_blend_row_of(const struct flx_volume_update *update, uint32_t bins, const float new_sh[36], const float *new_maps, float sh[36], float *maps);
/* The last flx_volume_blend[_device] or flx_volume_update[_device] (zeros if none): out[0] its entries, [1] workgroups of k_volume_blend, [2] m (0 without a map),
 * [3] 1 where a list was given, 0 for the arithmetic one, [4] the chunks of the bake behind it (0 for a blend alone), [5] 1 for an update, 0 for a blend; [6], [7]
 * zero.  It waits for nothing. */
flx_status flx_debug_last_volume_update(flx_context *ctx, uint32_t out[8]);
/* PROBE RELOCATION: flx_volume_position puts every probe exactly on the lattice, and a lattice point inside geometry or within a hair of a wall gives a probe
 * that bakes black and is blended into eight cells all the same.  Every probe gets AN OFFSET ROW — one float4: words 0 .. 2 the offset from its lattice point in
 * world units, word 3 a uint32 STATE —, made on the device from the first hits of the probe's own cube-face rays, and positions, bakes, updates and lookups that
 * honour the rows.  A zero-initialised array means "no offsets, every probe active".  All of it is calls of its own beside the ones above, which do what they did.
 * Every word is defined bit for bit in include/flx_volume_relocate.h, which the kernels (csrc/flx_volume_relocate.hip: k_probe_relocate,
 * k_volume_positions_offset; csrc/flx_volume.hip: the relocated lookups) and a CPU reference compile alike.
 * THE REDUCTION of a probe's R = 6 w w texels: row t of a FLX_SURFACE_HIT plane and of a FLX_SURFACE_NORMAL plane.  A texel is a HIT where the HIT row's word 3
 *   (int32) is not -1; a hit is BACK where the NORMAL row's word 3 is > 0, FRONT where it is < 0, NEITHER where it is 0 or a NaN.  H counts the hits, B the backs;
 *   the closest back, the closest front (least s = the HIT row's word 0) and the farthest front (greatest s) are pairs (s, t), TIES TO THE LOWEST t.  A hit whose s
 *   is a NaN or negative counts but takes part in no extreme (-0.0f takes part as 0.0f).  Counts are integers and extremes exact selections: there is no order of
 *   sums to fix.  A texel's direction is recomputed from t (include/flx_probe.h); no ray row is read.
 * THE MOVE, o the old offset as given, the rules tried in this order; inside = (float)B > back_share (float)R (the product first):
 *   1 inside, and a closest back exists: o' = o + dir_cb (s_cb + min_front 0.5) — min_front 0.5 first, then the sum, then per axis the product and the sum.
 *   2 otherwise, a closest front exists and s_cf < min_front: where (dir_cf . dir_ff) <= 0.5, o' = o + dir_ff min(s_ff, min_front); otherwise (a NaN too) o' = o.
 *   3 otherwise: len = sqrt((ox ox + oy oy) + oz oz); margin = min(s_cf - min_front, len), len where no front exists; where len > 0: o' = o - (o / len) margin (three
 *     quotients, three products, three differences); otherwise o' = o.
 *   o' is ACCEPTED where its three words are finite and |o'_a| <= limit spacing_a per axis (the product first); otherwise the row keeps o's bits.  Under
 *   FLX_VOLUME_RELOCATE_FREEZE the row always keeps o's bits and only the state is written.
 * THE STATE: bit 0 INACTIVE — inside, or no front hit with s <= reach —; bits 1 - 2 the rule that fired, 1 .. 3; bit 3 REJECTED — a move was computed and not
 *   accepted.  IT DESCRIBES THE POSITION THE RAYS WERE CAST FROM: iterate the call a few times and end with one frozen call.
 * WHERE THE ISSUE OF AN ORDER WAS OPEN it is fixed as written here: x before y before z, dot products and the squared length (x x + y y) + z z with the products
 *   first, min(a, b) = (b < a) ? b : a.
 * THE POSITION of probe p with offsets is flx_volume.h's plus the offset, one sum per axis, word 3 0.0f; of a list's entry (update and d_indices as for "volume
 *   updates"; an entry outside the grid gets probe nx ny nz - 1) the same.  update NULL: the whole grid, n = nx ny nz.
 * THE LOOKUP WITH OFFSETS is the lookup above — the directional one where a map is given — with two changes: step 5 takes d = (probe + offset) - x', one sum, one
 *   difference per axis; and an INACTIVE corner adds nothing and NONE OF ITS ROWS ARE READ (a NaN row in a dead probe does not poison its neighbours).  The
 *   trilinear weights stay the lattice cell's; all eight corners inactive give four 0.0f.
 * flx_probe_relocate_device is the reduction alone over two planes of the caller's, n_probes R rows each, probe first_probe + i's rows from row i R; it updates
 * offset rows first_probe .. first_probe + n_probes - 1 of d_offsets (nx ny nz rows) in place; NO SCENE.  flx_volume_positions_offset_device: NO SCENE.
 * flx_volume_relocate_device is the whole path on the context's stream: the probes in chunks of max(1, 2^21 / R) (flx_debug_set_probe_chunk lowers it), per chunk
 * k_volume_positions_offset, k_probe_rays, flx_rays_surface_device AS IT STANDS with FLX_SURFACE_HIT | FLX_SURFACE_NORMAL into a buffer the context owns (grown
 * behind one wait, never shrunk), k_probe_relocate: bit for bit the calls one after the other, whatever the chunk.  The relocated lookups are the _map siblings'
 * signatures plus d_offsets; map and d_maps may both be NULL for the whole-sphere moments.  flx_volume_irradiance_relocated_of is one point on the host,
 * flx_volume_relocate_row_of one probe's planes to its offset row on the host.  flx_volume_bake_relocated_device is flx_volume_positions_offset_device into a buffer
 * the context owns and flx_probes_sh_device (flx_probes_sh_map_device with a map) from there; flx_volume_update_relocated_device the same with a list, then
 * flx_volume_blend_device: bit for bit those calls.
 * Ordering, producer_stream, the frame server and n == 0 are flx_probes_sh_device's, word for word.  The calls without _device are the same for host arrays.
 * Refusals, each with a message of its own, nothing enqueued and the outputs untouched.  The siblings' come first in their own words.  Then FLX_ERR_INVALID for
 * relocate NULL; back_share outside [0, 1] or not finite; min_front negative or not finite; reach not > 0 or not finite; limit outside [0, 0.5] or not finite;
 * unknown flag bits; a reserved word that is not 0; face_size 0 or above 256; first_probe + n_probes beyond the grid (in 64 bits); n_probes R of 2^32 or more; an
 * array that is NULL, misaligned, leaving the address space, not memory of the context's device, in an allocation too short, or overlapping another of the call. */
#define FLX_VOLUME_RELOCATE_FREEZE 1u
struct flx_volume_relocate {
  float back_share;     /* 0 .. 1; typical 0.25 */
  float min_front;      /* >= 0, finite: the distance to keep from front faces */
  float reach;          /* > 0, finite: a probe whose nearest front face is farther than this lights nothing */
  float limit;          /* 0 .. 0.5: the share of the spacing an offset may reach per axis; typical 0.45 */
  uint32_t flags;       /* FLX_VOLUME_RELOCATE_FREEZE or 0 */
  uint32_t reserved;    /* 0 */
};
flx_status flx_probe_relocate_device(flx_context *ctx, const flx_volume_grid *grid, const struct flx_volume_relocate *relocate, const void *d_hit /* n_probes * 6 w w float4 */,
                                     const void *d_normal /* the same */, uint32_t n_probes, uint32_t face_size, uint32_t first_probe, void *d_offsets /* nx ny nz float4, in and out */,
                                     void *producer_stream);
flx_status flx_probe_relocate(flx_context *ctx, const flx_volume_grid *grid, const struct flx_volume_relocate *relocate, const void *hit, const void *normal, uint32_t n_probes,
                              uint32_t face_size, uint32_t first_probe, float *offsets);      /* host arrays; offsets in and out */
flx_status flx_volume_positions_offset_device(flx_context *ctx, const flx_volume_grid *grid, const void *d_offsets /* nx ny nz float4 */, const struct flx_volume_update *update /* or NULL */,
                                              const void *d_indices /* n uint32, or NULL */, uint32_t n, void *d_positions /* n * 4 floats */, void *producer_stream);
flx_status flx_volume_positions_offset(flx_context *ctx, const flx_volume_grid *grid, const float *offsets, const struct flx_volume_update *update, const uint32_t *indices, uint32_t n,
                                       float *positions);      /* host arrays */
flx_status flx_volume_relocate_device(flx_context *ctx, int32_t texture_width, const flx_volume_grid *grid, const struct flx_volume_relocate *relocate, uint32_t face_size,
                                      void *d_offsets /* nx ny nz float4, in and out */, void *producer_stream);
flx_status flx_volume_relocate(flx_context *ctx, int32_t texture_width, const flx_volume_grid *grid, const struct flx_volume_relocate *relocate, uint32_t face_size,
                               float *offsets);      /* host array; in and out */
flx_status flx_volume_irradiance_relocated_device(flx_context *ctx, const flx_volume_grid *grid, const void *d_sh, const void *d_positions, const void *d_normals, uint32_t n,
                                                  void *d_out, const flx_volume_map *map /* or NULL */, const void *d_maps /* or NULL */, const void *d_offsets, void *producer_stream);
flx_status flx_volume_irradiance_relocated(flx_context *ctx, const flx_volume_grid *grid, const float *sh, const float *positions, const float *normals, uint32_t n, float *out,
                                           const flx_volume_map *map, const float *maps, const float *offsets);      /* host arrays */
flx_status flx_rays_irradiance_relocated_device(flx_context *ctx, int32_t texture_width, const flx_volume_grid *grid, const void *d_sh, const void *d_rays, uint32_t n, void *d_out,
                                                const flx_volume_map *map, const void *d_maps, const void *d_offsets, void *producer_stream);
flx_status flx_rays_irradiance_relocated(flx_context *ctx, int32_t texture_width, const flx_volume_grid *grid, const float *sh, const float *rays, uint32_t n, float *out,
                                         const flx_volume_map *map, const float *maps, const float *offsets);      /* host arrays */
flx_status flx_frame_irradiance_relocated_device(flx_context *ctx, const flx_frame_params *params, const flx_volume_grid *grid, const void *d_sh, void *d_out, const flx_volume_map *map,
                                                 const void *d_maps, const void *d_offsets);
flx_status flx_frame_irradiance_relocated(flx_context *ctx, const flx_frame_params *params, const flx_volume_grid *grid, const float *sh, float *out, const flx_volume_map *map,
                                          const float *maps, const float *offsets);      /* host arrays */
flx_status flx_volume_bake_relocated_device(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, const flx_volume_map *map /* or NULL */,
                                            const void *d_offsets, void *d_sh, void *d_maps /* NULL without a map */, void *producer_stream);
flx_status flx_volume_bake_relocated(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, const flx_volume_map *map,
                                     const float *offsets, float *sh, float *maps);      /* host arrays */
flx_status flx_volume_update_relocated_device(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, const flx_volume_map *map /* or NULL */,
                                              const struct flx_volume_update *update, const void *d_indices, uint32_t n_list, const void *d_offsets, void *d_sh, void *d_maps, void *d_state,
                                              void *producer_stream);
flx_status flx_volume_update_relocated(flx_context *ctx, const flx_trace_params *trace, const flx_probe_params *params, const flx_volume_grid *grid, const flx_volume_map *map,
                                       const struct flx_volume_update *update, const uint32_t *indices, uint32_t n_list, const float *offsets, float *sh, float *maps,
                                       uint32_t *state);      /* host arrays; sh and maps in and out */
void flx_volume_irradiance_relocated_of(const flx_volume_grid *grid, const flx_volume_map *map /* or NULL */, const float *sh_rows, const float *map_rows /* or NULL */,
                                        const float *offset_rows, const float position[4], const float normal[4], float out[4]);
void flx_volume_relocate_row_of(const flx_volume_grid *grid, const struct flx_volume_relocate *relocate, uint32_t face_size, const float *hit /* 6 w w * 4 floats */,
                                const float *normal /* the same */, float offset[4] /* in and out */);
/* The last flx_probe_relocate[_device] or flx_volume_relocate[_device] (zeros if none): out[0] its probes, [1] the face size, [2] its chunks (0 for the reduction
 * alone), [3] the probes of a full chunk, [4] workgroups of the last k_probe_relocate, [5] the relocation's flags, [6] first_probe, [7] 1 for the whole path.  It
 * waits for nothing. */
flx_status flx_debug_last_volume_relocate(flx_context *ctx, uint32_t out[8]);
/* SURFACE ROWS: what the surface is where a ray first hits — the question between "where does it hit" (flx_rays_cast) and "what radiance comes back"
 * (flx_rays_trace, flx_render).  The planes (AOVs) a denoiser of the caller's own, compositing or the shading of a hybrid renderer needs beside the noisy radiance:
 * position, geometric normal, shading normal, texture coordinates, and albedo, RME and TPO with the atlases applied.  They are the first thing lightTrace computes
 * at a hit (fragment:476-533) and have the oracle's bits: the same operations in the same order (csrc/flx_surface.hip: k_surface).
 * `fields` names the planes.  A PLANE is n rows of 16 bytes, one row per ray (or per pixel, row k = pixel k of flx_render's frame, row 0 on top).  Only the planes
 * asked for are written; they follow each other in bit order of `fields`: plane p starts at out + p * n * 16 bytes, and the output is popcount(fields) * n * 16
 * bytes.  A row, by plane (lightTrace's names):
 *   FLX_SURFACE_HIT              float s, u, v; int32 the entry index, -1 for none — flx_rays_cast's words 0..3
 *   FLX_SURFACE_POSITION         origin + s * direction, formed as ray.origin is at fragment:479 (direction * s + origin); float 1.0 for a hit, 0.0 for a miss
 *   FLX_SURFACE_GEOMETRY_NORMAL  normalize(cross(t0v - t1v, t0v - t2v)) of the transformed vertices, NOT flipped towards the ray; 0
 *   FLX_SURFACE_NORMAL           the smooth normal FACING THE RAY (smoothNormal * -signDir, with lastHitPoint = the ray's origin); float signDir: -1 a front face
 *                                was hit, +1 a back face, 0 at grazing incidence
 *   FLX_SURFACE_UV               float bu, bv, the interpolated texture coordinates; int32 2 x the entry's transform number (flx_rays_cast's word 4); 0
 *   FLX_SURFACE_ALBEDO           fetchTexVal(0, ..) r, g, b: the albedo atlas' texel, or the entry's own colour where it names no texture; 0
 *   FLX_SURFACE_RME              fetchTexVal(1, ..): roughness, metallicity, emissiveness; 0
 *   FLX_SURFACE_TPO              fetchTexVal(2, ..): translucency, particle density, optical density; 0
 * A MISS ROW IS ALL ZEROS in every plane, with -1 in word 3 of the HIT plane.  (These are not flx_gbuffers' planes: those are packed for the reference's RGBA8
 * denoise chain — normals in 4-bit codes, albedo multiplied over several bounces, no depth, no position.)
 * flx_rays_surface_device: the rays are flx_rays_cast's ray rows (words 3 and 7 are ignored); the closest hit is found exactly as FLX_RAYS_CLOSEST finds it, into
 * scratch the context owns (grown and never shrunk; the batch is cut into slabs of at most 2^21 rays so that it has a ceiling, flx_debug_set_trace_slab lowers it
 * for tests), and k_surface follows on the same stream.  texture_width: the frame params' (floor(2048 / standardTextureSizes[0])).
 * flx_frame_surface_device: the pixel's primary hit is found AS A FRAME FINDS IT (k_primary with the frame's own direction per pixel, not rayTracer: the two hit
 * rules differ on a few pixels per million); the ray is the camera position and that direction.  Of the params only width, height, camera, view_matrix and
 * texture_width are read; the tile policy must name the whole frame (0/0/0 or x/0/1).  A group has no such call, as it casts no rays.
 * Ordering, producer_stream, the frame server and n == 0 are flx_rays_cast_device's, word for word: enqueued on the context's stream with no wait of the host, it
 * sees the scene as of the call, frames in flight finish unchanged; n == 0: FLX_OK, nothing enqueued (the scene and the arguments are looked at first).  (Where
 * the scratch must grow, the host waits for the stream first.)  flx_rays_surface and flx_frame_surface are the same for host arrays: staged through memory the
 * context owns; they wait and copy the planes out.
 * Refusals, each with a message of its own and nothing enqueued: FLX_ERR_NO_SCENE before a scene and transforms are up; FLX_ERR_INVALID for fields 0 or with a bit
 * above FLX_SURFACE_TPO; texture_width < 1; NULL params; a width or height of 0 (or more than 2^32 - 1 pixels); a tile policy that is not the whole frame; an array
 * that is NULL, that is not memory of the context's device or not 16-byte aligned (device variants), or that sits in an allocation too short; planes or an array's end
 * that leave 64 bits; rays and output that overlap. */
#define FLX_SURFACE_HIT             1u
#define FLX_SURFACE_POSITION        2u
#define FLX_SURFACE_GEOMETRY_NORMAL 4u
#define FLX_SURFACE_NORMAL          8u
#define FLX_SURFACE_UV              16u
#define FLX_SURFACE_ALBEDO          32u
#define FLX_SURFACE_RME             64u
#define FLX_SURFACE_TPO             128u
flx_status flx_rays_surface_device(flx_context *ctx, int32_t texture_width, const void *d_rays /* n * 8 floats, on ctx's device */, uint32_t n, uint32_t fields,
                                   void *d_out /* popcount(fields) * n * 16 bytes */, void *producer_stream /* hipStream_t that wrote the rays, or NULL: they are complete */);
flx_status flx_rays_surface(flx_context *ctx, int32_t texture_width, const float *rays /* n * 8 floats */, uint32_t n, uint32_t fields, void *out);      /* host arrays */
flx_status flx_frame_surface_device(flx_context *ctx, const flx_frame_params *params, uint32_t fields, void *d_out /* planes of width * height rows, on ctx's device */);
flx_status flx_frame_surface(flx_context *ctx, const flx_frame_params *params, uint32_t fields, void *out);      /* host array */
/* The last surface call (zeros if none): out[0] its slabs, [1] the rays of a full slab (a frame: its pixels), [2] n, [3] fields, [4] 1 for a frame, [5] workgroups of
 * the last slab's first-hit launch (a frame: 0); [6], [7] zero.  It waits for nothing. */
flx_status flx_debug_last_surface(flx_context *ctx, uint32_t out[8]);
/* The uploaded scene as the device holds it, after everything enqueued so far: which 0 the geometry rows (12 floats per entry), 1 the attribute rows (28),
 * 2 the threaded hot-first copy (12 per entry of walk_entries), 3 the forward-ordered copy (12 per entry of fwd_entries: flx_debug_last_walk_lds' out[5], out[6]),
 * 4 the id list (an int32 in every 4 bytes of out, n_ids of them).
 * The first n_floats floats of the array; FLX_ERR_INVALID beyond its end.  Tests compare flx_scene_update's arrays with a fresh upload's. */
flx_status flx_debug_scene_read(flx_context *ctx, int which, float *out, uint32_t n_floats);
/* Walk n rays through the uploaded scene on the GPU, AS THE KERNELS DO, one ray per lane: rayTracer (fragment:172-227) and shadowTest (:230-279) of each ray;
 * used by tests to hold the device walks against literal answers computed from the shader text (tests/golden/walk_kat.json.gz).  variant 0: the wavefront
 * pipeline's lane walk over the threaded, hot-first copy with the rays pre-transformed into every object space; 1: the per-pixel / persistent kernels' lane
 * walk; 2: their wave-wide lockstep walk (scenes of at most 128 entries in one object space).  rays: 7 floats each (origin, direction, shadowTest's l);
 * out: 8 floats each: s, u, v, 2 x transform number and entry index of the closest hit (zeros and -1 for none), entries that walk fetched, shadowTest's
 * answer (0 / 1), entries the shadow walk fetched. */
flx_status flx_debug_walk(flx_context *ctx, int variant, const float *rays, float *out, uint32_t n);
/* Variant 0 of flx_debug_walk with the threaded entries [0, min(lds_count, walk_hot)) staged in LDS as the wavefront walk kernels stage the tree's top, every other
 * entry fetched from global memory (walkFetchP, walkSetupRays).  out: 10 floats per ray: flx_debug_walk's 8, then the entries both walks fetched from LDS and
 * the entries they fetched from global memory.  FLX_ERR_INVALID when the staged entries, the transforms and the rays need more than the kernel's 160 KB of LDS. */
flx_status flx_debug_walk_staged(flx_context *ctx, uint32_t lds_count, const float *rays, float *out, uint32_t n);
/* out[0 .. 3]: the last wavefront frame or frame server launch since the scene upload (zeros if none): the ldsCount (entries of the tree's top staged in LDS) it
 * launched with, whether its rays were pre-transformed (0 / 1), which launch (1 rounds, 2 the frame kernel, 3 the frame kernel with the front inside, 4 the frame
 * server), n_transforms; out[4 .. 6]: the uploaded scene's walk_hot, walk_entries and fwd_entries (the size the lockstep copy is judged by). */
flx_status flx_debug_last_walk_lds(flx_context *ctx, uint32_t out[7]);
/* Scheduler statistics of the last counted frame (wavefront pipeline): for bounce b = 0..3 (3 = all
 * later ones) out[2b] = wave-iterations of the walk kernel, out[2b+1] = fold/refill batches. */
flx_status flx_get_diag(flx_context *ctx, uint64_t out[32]);   /* out[8..12]: bounce-0 walk kernel stamps: fold, refill, step cycles, wave lifetime, waves; out[16+3b..]: per bounce sum / count / max of wave lifetimes */
/* Tail profile of the last counted frame (wavefront pipeline, walk kernel of the round given to the build by FLX_TAIL_DIAG_ROUND, default 0):
 * for k = 0 .. 11 out[3k], out[3k+1], out[3k+2] = sum / count / max over the walk workgroups of the shader cycles since the workgroup's start
 * at which its walks in flight first numbered <= 2^k; out[36..38] the same for the moment the workgroup found the walk queue dry. */
flx_status flx_get_tail_diag(flx_context *ctx, uint64_t out[40]);
/* ---- ray batches with a volume (beside "ray queries" and "probe volumes" above, whose types it takes) --------------------------------------------- */
/* A TRACED BATCH WHOSE PATHS END IN A PROBE VOLUME: flx_rays_trace_ordered_device with the ambient term looked up.  A path of flx_rays_trace ends in finalColor +
 * importancyFactor * ambient, the params' constant standing for all the light the path did not trace.  Here it ends in finalColor + importancyFactor * A, per
 * component, the product first (include/flx_gather.h: the definition, which the kernels and the tests' CPU reference compile alike):
 *   THE LAST POINT of a path is the surface point of the last bounce iteration it shaded: x that iteration's ray origin, n its smooth normal facing the arriving ray
 *     — a FLX_SURFACE_POSITION and a FLX_SURFACE_NORMAL row's floats for the ray that arrived there.  A path that shaded nothing (max_reflections == 0, or the loop
 *     guard failing before bounce 0) has none.
 *   THE LOOKUP E = (e0, e1, e2, W) of the position row (x, 1.0f) and n: flx_volume_irradiance_of's with neither offsets nor map, flx_volume_irradiance_map_of's with
 *     a map, flx_volume_irradiance_relocated_of's with offsets (with or without a map).
 *   THE VALUE A_c = (W > 0.0f) ? e_c * gain : params->ambient[c]; a NaN W and a path without a last point take the constant.  Irradiance over pi is the radiance a
 *     Lambertian surface sends on, which is what `ambient` stands for: a gain of (float)(1 / pi) is the usual one.
 * Everything else of a radiance row — the loop guard, the bounces, the walks, the noise, the sum over samples in sample order, the scale, originalColor, the eight
 * words, the miss row — is flx_rays_trace's.  Two bounces and a volume stand in for many bounces at the cost of two bounces and one lookup.
 * Three launches a slab behind its first hits (csrc/flx_rays_gather.hip): k_rays_paths_gather writes a PATH RECORD of 64 bytes per (ray, sample), k_gather_ambient
 * looks the records up one lane each and writes the 16-byte slots k_rays_resolve reads.  Ray rows, radiance rows, `order`, producer_stream, the frame server, n == 0,
 * slabs and the host call's staging are flx_rays_trace_ordered_device's and flx_rays_trace_ordered's, word for word; a slab's scratch holds five 16-byte slots a
 * (ray, sample) where theirs holds one, under the same 256 MB.  flx_debug_set_trace_slab and flx_debug_set_query_groups apply as they do there.  A group has no
 * such call; frames do not take a volume; filter planes and ray images take one through the calls of "ray images with a volume" below.
 * Refusals, each with nothing enqueued and the output untouched, in this order: the scene's and the trace params' own and an unknown bit of `order` (for any n); for
 * n > 0 the rays' and the radiance's, all in flx_rays_trace_ordered's words under this call's name; a NULL volume; the grid's and the map's (a map only where one is
 * given) and the volume's arrays' — NULL, not memory of the context's device, not 16-byte aligned, too short, overlapping each other — in the volume calls' words;
 * then, FLX_ERR_INVALID with a message of its own each: a gain that is negative or not finite; a reserved word that is not 0; `map` and `maps` not both given or both
 * NULL; an array of the volume that overlaps the rays or the radiance. */
typedef struct flx_gather_volume {
  const flx_volume_grid *grid;
  const void *sh;            /* nx ny nz * 9 float4 */
  const flx_volume_map *map; /* or NULL */
  const void *maps;          /* nx ny nz * m m float4; NULL without a map */
  const void *offsets;       /* nx ny nz float4 ("probe relocation"), or NULL: probes on the lattice */
  float gain;                /* finite, >= 0 */
  uint32_t reserved;         /* 0 */
} flx_gather_volume;
flx_status flx_rays_trace_gather_device(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume /* host struct, arrays on ctx's device */,
                                        const void *d_rays /* n * 8 floats */, void *d_radiance /* n * 8 words */, uint32_t n, uint32_t order /* 0 or FLX_TRACE_ORDER_HITS */,
                                        void *producer_stream /* as flx_rays_trace_device's */);
flx_status flx_rays_trace_gather(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume /* host arrays */, const float *rays, void *radiance, uint32_t n,
                                 uint32_t order);
/* The last batch traced with a volume (zeros but [7] if none), set only when the whole call succeeded: out[0] its rays, [1] its slabs, [2] the rays of a full slab,
 * [3] workgroups of the last slab's paths kernel, [4] workgroups of its lookup kernel, [5] bit 0 a map, bit 1 offsets, [6] whether it was ordered, [7] the bytes of
 * one path record.  It waits for nothing. */
flx_status flx_debug_last_gather(flx_context *ctx, uint32_t out[8]);
/* ---- ray images with a volume (beside "ray queries", "ray images over time", "cameras" and "ray batches with a volume" above, whose types it takes) ---------- */
/* THE FILTER PLANES, THE RAY IMAGES AND THE RAY IMAGES OVER TIME WHOSE SAMPLES END IN A PROBE VOLUME: the displayable output — the five planes, the denoise chain,
 * the temporal histories — lit by a volume.  THE RULE: a gathered plane row is flx_rays_planes' row ("ray queries") with one change: sample s of a ray contributes
 * flx_gather_path_value(finalColor_s, importancyFactor_s, A_s) where flx_rays_planes adds finalColor_s + importancyFactor_s * ambient.  A_s is computed exactly as
 * include/flx_gather.h defines it: flx_gather_lookup at the sample's last point (x, n), in whichever of the three forms the volume takes, then flx_gather_ambient with
 * the caller's gain; the params' ambient where W is not > 0 and where the sample shaded nothing (max_reflections == 0, min_importancy > 1).  The last point of a
 * sample is a gathered batch's: x the ray origin of the last bounce iteration the sample shaded, n that iteration's smooth normal facing the arriving ray.
 * Everything else is unchanged: the globals carried from sample to sample, the sample order, the scale, fract / floor, planes 2 to 4, the miss row of zeros, the
 * RGBA8 packing, the temporal pass in the lane that owns the ray, finalColor * originalColor in the temporal canvas mode.  include/flx_gather.h has no new function.
 * The lookup runs INLINE in the planes kernel (csrc/flx_rays_planes_gather.hip: k_rays_planes_gather), at the end of every sample's bounce loop, where the wave is
 * together again: no records, no second kernel; the scratch is the hit rows only and a slab is one slot a ray, 2^21 rays, so that a 1080p image is one slab.
 * Each call has its sibling's signature with the volume after the params.  The _device calls take a host struct whose arrays are memory of the context's device.
 * THE HOST CALLS TAKE HOST RAYS AND HOST OUTPUTS BUT A VOLUME WHOSE ARRAYS ARE ON THE DEVICE, as a volume handle's are (flx_volume_bake_device's rows): a volume is
 * resident, the rays of an image are not.  The camera calls make the rays on the device as flx_camera_image[_temporal]_device do and hand them on.
 * The temporal calls use the same FLX_RAY_HISTORIES histories as flx_rays_image_temporal: A HISTORY DOES NOT KNOW WHETHER A VOLUME LIT IT — images with and without
 * a volume, or with different volumes, blend in one history if the caller names the same one; flx_rays_history_reset is the caller's business.
 * Ordering, producer_stream, the frame server, n == 0, slabs, flx_debug_set_trace_slab and flx_debug_set_query_groups are the siblings', word for word.
 * Refusals, each with nothing enqueued, the outputs untouched and the history exactly what it was, in this order: 1. the sibling's own for the scene, the params, the
 * size, the temporal, the camera and the arrays, under the new call's name; 2. flx_rays_trace_gather's for the volume: a NULL volume, the grid's, the map's, the
 * arrays', a gain that is negative or not finite, a reserved word that is not 0, `map` and `maps` not both given or both NULL; 3. an array of the volume that
 * overlaps the rays, a plane output or the image.  A group has no such call; frames do not take a volume. */
flx_status flx_rays_planes_gather_device(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume /* host struct, arrays on ctx's device */,
                                         const void *d_rays, uint32_t n, void *d_planes8, void *d_planes32, void *producer_stream);
flx_status flx_rays_planes_gather(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume /* arrays on ctx's device */, const float *rays, uint32_t n,
                                  void *planes8, void *planes32);
flx_status flx_rays_image_gather_device(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume, int hdr, const void *d_rays, uint32_t width,
                                        uint32_t height, void *d_out_rgba, void *producer_stream);
flx_status flx_rays_image_gather(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume /* arrays on ctx's device */, int hdr, const float *rays,
                                 uint32_t width, uint32_t height, float *out_rgba);
flx_status flx_rays_image_temporal_gather_device(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume, const flx_ray_temporal *temporal,
                                                 const void *d_rays, uint32_t width, uint32_t height, void *d_out_rgba, void *producer_stream);
flx_status flx_rays_image_temporal_gather(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume /* arrays on ctx's device */,
                                          const flx_ray_temporal *temporal, const float *rays, uint32_t width, uint32_t height, float *out_rgba);
flx_status flx_camera_image_gather_device(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume, int hdr, const flx_camera *camera, uint32_t width,
                                          uint32_t height, void *d_out_rgba);
flx_status flx_camera_image_gather(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume /* arrays on ctx's device */, int hdr,
                                   const flx_camera *camera, uint32_t width, uint32_t height, float *out_rgba);
flx_status flx_camera_image_temporal_gather_device(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume, const flx_ray_temporal *temporal,
                                                   const flx_camera *camera, uint32_t width, uint32_t height, void *d_out_rgba);
flx_status flx_camera_image_temporal_gather(flx_context *ctx, const flx_trace_params *params, const flx_gather_volume *volume /* arrays on ctx's device */,
                                            const flx_ray_temporal *temporal, const flx_camera *camera, uint32_t width, uint32_t height, float *out_rgba);
/* The last planes, image or temporal call with a volume (zeros if none), set only when the whole call succeeded: out[0] its rays, [1] its slabs, [2] the rays of a
 * full slab, [3] workgroups of the last planes launch, [4] bit 0 a map, bit 1 offsets, [5] the mode (0 planes, 1 the temporal canvas, 2 the temporal filter),
 * [6] samples, [7] whether the lockstep walk ran.  It waits for nothing. */
flx_status flx_debug_last_planes_gather(flx_context *ctx, uint32_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* FLEXLIGHT_HIP_DEBUG_H */
