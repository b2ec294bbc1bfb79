#!/usr/bin/env python3
"""What a traced ray batch costs (flx_rays_trace_device, csrc/flx_rays_trace.hip) on the dragon scene of bench.py: the 1080p camera's rays, 8 spp, 4 bounces.
  (a) pixel order   the camera's rays as k_primary makes them (origin = the camera, direction = primary_dir_v's bits, noise = the pixel's NDC), row by row,
  (b) shuffled      the same rays in an order shuffled by a fixed seed,
  (c) bounce        origins on the hit points of (a), directions cosine-distributed about the way back to the camera, random noise coordinates,
and, the references on the same build, flx_render_device of that frame with flx_set_pipeline(ctx, 2) — the structure the batch has — and with the default pipeline.
GPU time between two events recorded on the context's stream around each call; the five are measured in turn, round after round (REPEATS rounds after WARMUP), and
reported as median [min .. max].  Once, outside the timed region, the rows of (a) are held against flx_render_device's frame: words 0..3 are the frame's pixel, bit
for bit, wherever the frame's hit rule and rayTracer agree (they differ on back faces, within 2^-16 of an edge, on ties and at the near plane).  GPU box.

--ordered: the three sets through flx_rays_trace_ordered_device (FLX_TRACE_ORDER_HITS: each slab's rays traced in the order of their first hit points,
csrc/flx_rays_order.hip) beside the unordered call, the six calls in turn, and nothing else; the ordered rows are held against the unordered rows once, outside the
timed region, all eight words.  It writes profiles/rays_order.txt: every ordered call against its unordered twin and the ordered shuffled call against the unordered
pixel-ordered one, each with the verdict whether the difference lies outside the two calls' own min .. max.  With a library that lacks the ordered call (FLX_LIB: an
earlier build, the control) the three unordered calls are measured alone.
--profile-once: one pass over the calls and no report, for a run under rocprofv3 --kernel-trace --stats.

usage: rays_trace_time.py [--ordered] [--profile-once] [--out profiles/rays_trace.txt] [--repeats 15]"""
import os
import sys

import numpy as np
import torch                                   # (before the library: INTEGRATION.md, Build)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "web-ray-tracer_amd"))
from flexlight_hip import capi
from flexlight_hip.scene_io import Scene

ORDERED = "--ordered" in sys.argv
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "rays_order.txt" if ORDERED else "rays_trace.txt")
REPEATS = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 15
WARMUP = 3
W, H, SPP, BOUNCES = 1920, 1080, 8, 4

sc = Scene.golden("dragon")
p = sc.frame_params(width=W, height=H, samples=SPP, max_reflections=BOUNCES, use_filter=0)
t = capi.TraceParams.of_frame(p)


def camera_rows():
    """the rays k_primary traces for the frame, in pixel order, with the bits of flx_invert3x3 (double) and primary_dir_v (float32, operation by operation)"""
    a, b, c, d, e, f, g, h, i = [float(x) for x in p.view_matrix]
    A, B, Cc = e * i - f * h, -(d * i - f * g), d * h - e * g
    r = 1.0 / (a * A + b * B + c * Cc)
    iv = np.array([A * r, -(b * i - c * h) * r, (b * f - c * e) * r, B * r, (a * i - c * g) * r, -(a * f - c * d) * r, Cc * r, -(a * h - b * g) * r, (a * e - b * d) * r]).astype(np.float32)
    f32 = np.float32
    px, row = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    py = f32(H - 1) - row                                                     # image row 0 is the top, NDC y points up
    nx = (px + f32(0.5)) / f32(W) * f32(2.0) - f32(1.0)
    ny = (py + f32(0.5)) / f32(H) * f32(2.0) - f32(1.0)
    dx, dy, dz = [(iv[3 * k] * nx + iv[3 * k + 1] * ny) + iv[3 * k + 2] for k in range(3)]
    length = np.sqrt((dx * dx + dy * dy) + dz * dz)
    rows = np.zeros((W * H, 8), np.float32)
    rows[:, 0:3] = list(p.camera)
    rows[:, 3], rows[:, 7] = nx.reshape(-1), ny.reshape(-1)
    rows[:, 4], rows[:, 5], rows[:, 6] = (dx / length).reshape(-1), (dy / length).reshape(-1), (dz / length).reshape(-1)
    return rows


def bounce_rows(camera, radiance, rng):
    """from the hit points of the camera's rays (a miss keeps its ray), a cosine-distributed direction about the way back to the camera; random noise coordinates"""
    cols = capi.unpack_radiance(radiance)
    hit = cols["entry"] != -1
    rows = camera.copy()
    point = camera[:, 0:3] + cols["s"][:, None] * camera[:, 4:7]
    normal = -camera[:, 4:7]
    a = np.where(np.abs(normal[:, 0:1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    t1 = np.cross(normal, a)
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(normal, t1)
    u1, u2 = rng.random(len(rows)), rng.random(len(rows))
    r, phi = np.sqrt(u1), 2.0 * np.pi * u2
    d = (r * np.cos(phi))[:, None] * t1 + (r * np.sin(phi))[:, None] * t2 + np.sqrt(1.0 - u1)[:, None] * normal
    rows[hit, 0:3] = (point + 1e-3 * normal)[hit]
    rows[hit, 4:7] = d[hit]
    rows[:, 3], rows[:, 7] = rng.uniform(-1.0, 1.0, len(rows)), rng.uniform(-1.0, 1.0, len(rows))
    return rows


ctx = capi.Context(0)
stream = torch.cuda.Stream()
ctx.set_stream(stream.cuda_stream)
ctx.update_scene(sc)
rng = np.random.default_rng(2024)
a = camera_rows()
first = ctx.trace_rays(a, t)
sets = [("pixel order", a), ("shuffled", a[rng.permutation(len(a))]), ("bounce", bounce_rows(a, first, rng))]
d_frame = torch.empty((H * W, 4), dtype=torch.float32, device="cuda")
d_out = torch.empty((len(a), 32), dtype=torch.uint8, device="cuda")
d_sets = [(name, torch.from_numpy(rows).cuda()) for name, rows in sets]
torch.cuda.synchronize()

# ---- once, outside the timed region: the rows of (a) against the library's own frame ----
ctx.set_pipeline(2)
ctx.render_device(p, d_frame.data_ptr())
ctx.trace_rays_device(d_sets[0][1], t, d_out)
ctx.sync()
frame = d_frame.cpu().numpy().view(np.uint32)
rows = d_out.cpu().numpy().view(np.uint32).reshape(-1, 8)
assert np.array_equal(rows, np.ascontiguousarray(first).view(np.uint32).reshape(-1, 8))          # the device call and the host call: the same rows
equal = (rows[:, 0:4] == frame).all(axis=1)
assert equal.mean() > 0.995, equal.mean()
ctx.set_pipeline(0)
ctx.render_device(p, d_frame.data_ptr())
ctx.sync()
assert np.array_equal(d_frame.cpu().numpy().view(np.uint32), frame)                              # the default pipeline's frame is pipeline 2's
default_pipeline = ctx.last_pipeline()


def frame_call(pipeline):
    def call():
        ctx.set_pipeline(pipeline)
        ctx.render_device(p, d_frame.data_ptr())
    return call


calls = [("flx_rays_trace_device, " + name, (lambda d: lambda: ctx.trace_rays_device(d, t, d_out))(d)) for name, d in d_sets]
have_ordered = hasattr(capi.LIB, "flx_rays_trace_ordered_device")
if ORDERED and have_ordered:
    d_twin = torch.empty_like(d_out)
    for name, d in d_sets:                     # once, outside the timed region: the ordered rows are the unordered rows
        ctx.trace_rays_device(d, t, d_out)
        ctx.trace_rays_ordered_device(d, t, d_twin)
        ctx.sync()
        assert torch.equal(d_out, d_twin), name
    order_info = ctx.last_ray_order()
    del d_twin
    calls = [c for name, d in d_sets for c in (("flx_rays_trace_device, " + name, (lambda d: lambda: ctx.trace_rays_device(d, t, d_out))(d)),
                                                ("flx_rays_trace_ordered_device, " + name, (lambda d: lambda: ctx.trace_rays_ordered_device(d, t, d_out))(d)))]
elif not ORDERED:
    calls += [("flx_render_device, flx_set_pipeline(ctx, 2)", frame_call(2)), ("flx_render_device, default pipeline (%s)" % (default_pipeline,), frame_call(0))]
if "--profile-once" in sys.argv:
    for name, call in calls:
        call()
    ctx.sync()
    ctx.close()
    sys.exit(0)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
ms = {name: [] for name, _ in calls}
for k in range(WARMUP + REPEATS):
    for name, call in calls:
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        if k >= WARMUP:
            ms[name].append(e0.elapsed_time(e1))
ctx.set_pipeline(0)
info, last = ctx.device_info(), ctx.last_trace()
cols_a, cols_c = capi.unpack_radiance(first), capi.unpack_radiance(ctx.trace_rays(sets[2][1], t))
lines = ["traced ray batches on the dragon scene (tests/golden/ref_dragon.flxs.gz): the %d x %d camera's %d rays, %d spp, %d bounces; %s, %d CUs" % (W, H, len(a), SPP, BOUNCES, info[0], info[1]),
         "GPU ms between two events around each call, the five calls in turn, median of %d rounds after %d warm-up rounds [min .. max]" % (REPEATS, WARMUP), ""]
med = {name: float(np.median(v)) for name, v in ms.items()}
for name, _ in calls:
    lines.append("  %-52s %8.3f ms [%8.3f .. %8.3f]" % (name, med[name], min(ms[name]), max(ms[name])))
if ORDERED:
    lines[1] = "GPU ms between two events around each call, the %d calls in turn, median of %d rounds after %d warm-up rounds [min .. max]" % (len(calls), REPEATS, WARMUP)
    lines[2:2] = ["library: %s" % os.path.basename(os.path.dirname(os.path.abspath(capi.LIB_PATH)))] if os.environ.get("FLX_LIB") else []

    def against(new, old):
        apart = min(ms[new]) > max(ms[old]) or max(ms[new]) < min(ms[old])
        return "  %-48s / %-44s %6.3f  (%+8.3f ms; %s the two calls' min .. max)" % (new, old, med[new] / med[old], med[new] - med[old], "OUTSIDE" if apart else "inside")

    if have_ordered:
        lines += ["", "ratios of the medians:"]
        lines += [against("flx_rays_trace_ordered_device, " + name, "flx_rays_trace_device, " + name) for name, _ in d_sets]
        lines += [against("flx_rays_trace_ordered_device, shuffled", "flx_rays_trace_device, pixel order"), against("flx_rays_trace_device, shuffled", "flx_rays_trace_device, pixel order")]
        lines += ["", "the sort of the last batch: %d workgroups of T = %d items, %d passes, %d of %d rays live" % (order_info["groups"], order_info["T"], order_info["passes"], order_info["live"], order_info["n"]),
                  "verified once outside the timed region: the ordered rows of every set equal the unordered rows, all eight words"]
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    ctx.close()
    sys.exit(0)
p2 = med["flx_render_device, flx_set_pipeline(ctx, 2)"]
spread = max(ms["flx_render_device, flx_set_pipeline(ctx, 2)"]) - min(ms["flx_render_device, flx_set_pipeline(ctx, 2)"])
lines += ["", "ratio to the pipeline-2 frame (the run's spread of that frame: %.3f ms = %.1f %%):" % (spread, 100.0 * spread / p2)]
for name, _ in calls[:3]:
    lines.append("  %-52s %6.3f" % (name, med[name] / p2))
lines += ["", "the batch: %d slab(s) of at most %d rays, %d workgroups of 256 lanes in the paths kernel, %d of 1024 in the first-hit kernel, lockstep %d" % (
              last["slabs"], last["slab"], last["path_groups"], last["query_groups"], last["lockstep"]),
          "set pixel order: hit %.3f, bounce iterations per ray %.2f;  set bounce: hit %.3f, bounce iterations per ray %.2f" % (
              (cols_a["entry"] != -1).mean(), cols_a["shades"].mean(), (cols_c["entry"] != -1).mean(), cols_c["shades"].mean()),
          "verified once outside the timed region: words 0..3 of the pixel-ordered rows equal flx_render_device's frame bit for bit on %d of %d pixels (%.4f %%; the rest: the frame's hit rule against rayTracer's)" % (
              equal.sum(), equal.size, 100.0 * equal.mean())]
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("\n".join(lines), flush=True)
ctx.close()
