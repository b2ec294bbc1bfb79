#!/usr/bin/env python3
"""What a traced batch costs when its paths end in a probe volume (flx_rays_trace_gather_device, csrc/flx_rays_gather.hip) against the plain batch with one bounce
more (flx_rays_trace_device), on the dragon scene of bench.py: the 1920 x 1080 pinhole camera's rays made on the device (flx_camera_rays_device), 8 samples, a
16 x 8 x 16 volume with a map over the scene's first hit points, baked on the device.
  flx_rays_trace_device at K = 1, 2, 3, 4 bounces, flx_rays_trace_gather_device at K = 1, 2, 3 and, to tell the cost of the slabs from the cost of the tail, the plain
  trace cut into the gathered batch's slabs at K = 1, 2, 3: the ten calls in turn, round after round: GPU time between two
  events recorded on the context's stream around each call, REPEATS rounds after WARMUP, reported as median [min .. max].
  THE BAR: gather at K bounces costs less than the plain trace at K + 1 — the tail is cheaper than the bounce it replaces —, said per K with whether the two calls'
  min .. max lie apart.  The overhead ratio gather(K) / trace(K).  Once, outside the timed region: the mean absolute difference of the K = 1 and K = 2 gathered images
  to the plain K = 4 image beside that of the plain K = 1 and K = 2 images (a description of what the feature buys, not a threshold).
--profile-once: one pass over the calls and no report, for a run under rocprofv3 --kernel-trace --stats.  GPU box.

usage: rays_gather_time.py [--profile-once] [--out profiles/rays_gather_times.txt] [--repeats 15]"""
import os
import sys

import numpy as np
import torch                                   # (before the library: INTEGRATION.md, Build)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "web-ray-tracer_amd"))
from flexlight_hip import capi
from flexlight_hip.scene_io import Scene

out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "rays_gather_times.txt")
REPEATS = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 15
WARMUP = 3
W, H, SPP = 1920, 1080, 8
COUNT, FACE, MAP = (16, 8, 16), 8, capi.VolumeMap(8, 5)

sc = Scene.golden("dragon")
p = sc.frame_params(width=W, height=H, samples=SPP, max_reflections=4, use_filter=0)


def params(bounces):
    t = capi.TraceParams.of_frame(p)
    t.max_reflections = bounces
    return t


ctx = capi.Context(0)
stream = torch.cuda.Stream()
ctx.set_stream(stream.cuda_stream)
ctx.update_scene(sc)
d_rays = ctx.camera_rays_device(capi.Camera.pinhole(p), W, H)
d_out = torch.empty((W * H, 32), dtype=torch.uint8, device="cuda")
ctx.trace_rays_device(d_rays, params(1), d_out)
ctx.sync()
# the grid: COUNT probes over the first hit points, a twentieth of their extent around them
rays = d_rays.cpu().numpy()
cols = capi.unpack_radiance(d_out)
hit = cols["entry"] != -1
points = rays[hit, 0:3].astype(np.float64) + rays[hit, 4:7].astype(np.float64) * cols["s"][hit, None]
lo, hi = points.min(axis=0), points.max(axis=0)
pad = (hi - lo).max() * 0.05
lo, hi = lo - pad, hi + pad
grid = capi.VolumeGrid(tuple(lo), tuple((hi - lo) / (np.array(COUNT) - 1)), COUNT, 0.01 * float((hi - lo).max()), 0.05, capi.VOLUME_VISIBILITY)
d_sh, d_maps = ctx.volume_bake_map_device(grid, params(4), capi.ProbeParams(FACE), MAP)
ctx.sync()

plain = {k: (lambda k: lambda: ctx.trace_rays_device(d_rays, params(k), d_out))(k) for k in (1, 2, 3, 4)}
gather = {k: (lambda k: lambda: ctx.trace_rays_gather_device(d_rays, params(k), grid, d_sh, MAP, d_maps, out=d_out))(k) for k in (1, 2, 3)}
GATHER_SLAB = ((1 << 24) // (5 * SPP)) & ~63          # flx_gather_slab_rays: five slots a (ray, sample) where the plain batch has one


def slabbed(k):
    """the plain batch cut into the gathered batch's slabs (flx_debug_set_trace_slab): what the cut alone costs the persistent kernels"""
    def call():
        ctx.set_trace_slab(GATHER_SLAB)
        ctx.trace_rays_device(d_rays, params(k), d_out)
        ctx.set_trace_slab(0)
    return call


calls = [("flx_rays_trace_device, K = %d" % k, plain[k]) for k in (1, 2, 3, 4)] + [("flx_rays_trace_gather_device, K = %d" % k, gather[k]) for k in (1, 2, 3)]
calls += [("flx_rays_trace_device in the gather's slabs, K = %d" % k, slabbed(k)) for k in (1, 2, 3)]
if "--profile-once" in sys.argv:
    for name, call in calls:
        call()
    ctx.sync()
    ctx.close()
    sys.exit(0)


def image(call):
    call()
    ctx.sync()
    return capi.unpack_radiance(d_out)["rgb"].astype(np.float64)


# ---- once, outside the timed region: what the volume buys an image of few bounces ----
want = image(plain[4])
differences = [("flx_rays_trace_device, K = %d (the constant ambient)" % k, float(np.nanmean(np.abs(image(plain[k]) - want)))) for k in (1, 2)]      # (nanmean: the scene has pixels that are NaN in the oracle too)
differences += [("flx_rays_trace_gather_device, K = %d" % k, float(np.nanmean(np.abs(image(gather[k]) - want)))) for k in (1, 2)]
last = ctx.last_gather()

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
info = ctx.device_info()
med = {name: float(np.median(v)) for name, v in ms.items()}
lines = ["traced batches with a volume on the dragon scene (tests/golden/ref_dragon.flxs.gz): the %d x %d pinhole camera's %d rays made on the device, %d samples; a %d x %d x %d volume with a map "
         "(size %d, sharpness %d), baked on the device with face size %d; %s, %d CUs" % (W, H, W * H, SPP, COUNT[0], COUNT[1], COUNT[2], MAP.size, MAP.sharpness, FACE, info[0], info[1]),
         "GPU ms between two events around each call, the %d calls in turn, median of %d rounds after %d warm-up rounds [min .. max]; each call timed alone, under no profiler" % (
             len(calls), REPEATS, WARMUP), ""]
for name, _ in calls:
    lines.append("  %-52s %8.3f ms [%8.3f .. %8.3f]" % (name, med[name], min(ms[name]), max(ms[name])))
lines += ["", "THE BAR — gather at K bounces against the plain trace at K + 1 (the tail against the bounce it replaces):"]
for k in (1, 2, 3):
    new, old = "flx_rays_trace_gather_device, K = %d" % k, "flx_rays_trace_device, K = %d" % (k + 1)
    apart = min(ms[new]) > max(ms[old]) or max(ms[new]) < min(ms[old])
    lines.append("  gather(%d) / trace(%d)  %6.3f  (%+8.3f ms; %s the two calls' min .. max)  %s" % (
        k, k + 1, med[new] / med[old], med[new] - med[old], "OUTSIDE" if apart else "inside", "HOLDS" if med[new] < med[old] and apart else "DOES NOT HOLD"))
lines += ["", "the overhead — gather at K bounces against the plain trace at K:"]
for k in (1, 2, 3):
    new, old = "flx_rays_trace_gather_device, K = %d" % k, "flx_rays_trace_device, K = %d" % k
    lines.append("  gather(%d) / trace(%d)  %6.3f  (%+8.3f ms)" % (k, k, med[new] / med[old], med[new] - med[old]))
lines += ["", "what the cut into slabs alone costs — the plain trace in the gathered batch's slabs of %d rays against the plain trace in one slab:" % GATHER_SLAB]
for k in (1, 2, 3):
    new, old = "flx_rays_trace_device in the gather's slabs, K = %d" % k, "flx_rays_trace_device, K = %d" % k
    lines.append("  slabbed trace(%d) / trace(%d)  %6.3f  (%+8.3f ms);  gather(%d) / slabbed trace(%d)  %6.3f" % (k, k, med[new] / med[old], med[new] - med[old], k, k, med["flx_rays_trace_gather_device, K = %d" % k] / med[new]))
lines += ["", "mean absolute difference of an image's r, g, b to the plain K = 4 image (gain 1 / pi; a description, not a threshold):"]
lines += ["  %-52s %.6f" % d for d in differences]
lines += ["", "the gathered batch: %d slab(s) of at most %d rays, %d workgroups of 256 lanes in the paths kernel, %d in the lookup kernel, a path record of %d bytes" % (
    last["slabs"], last["slab"], last["path_groups"], last["lookup_groups"], last["record_bytes"])]
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("\n".join(lines), flush=True)
ctx.close()
