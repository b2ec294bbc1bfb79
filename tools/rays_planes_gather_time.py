#!/usr/bin/env python3
"""What a ray image costs when its samples end in a probe volume (flx_rays_image_gather_device, csrc/flx_rays_planes_gather.hip: the lookup inline in the planes
kernel) against the plain image with one bounce more (flx_rays_image_device), on the dragon scene of bench.py: the 1920 x 1080 pinhole camera's rays made on the
device (flx_camera_rays_device), at 8 samples and at 1 sample, a 16 x 8 x 16 volume with a map over the scene's first hit points, baked on the device.
  flx_rays_image_device at K = 1, 2, 3, 4 bounces and flx_rays_image_gather_device at K = 1, 2, 3, per sample count: the calls in turn, round after round: GPU time
  between two events recorded on the context's stream around each call, REPEATS rounds after WARMUP, reported as median [min .. max].
  THE BAR (the gathered batches', profiles/rays_gather.txt): gather at K bounces costs less than the plain image at K + 1 — the tail is cheaper than the bounce it
  replaces — and the two calls' min .. max do not overlap, said per K.  The overhead ratio gather(K) / plain(K).  The slab count of the 1080p image, which must be 1.
--profile-once: one pass over the calls and no report, for a run under rocprofv3 --kernel-trace --stats.  GPU box.

usage: rays_planes_gather_time.py [--profile-once] [--out profiles/rays_planes_gather_times.txt] [--repeats 15]"""
import os
import sys

import numpy as np
import torch                                   # (before the library: INTEGRATION.md, Build)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "web-ray-tracer_amd"))
from flexlight_hip import capi
from flexlight_hip.scene_io import Scene

out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "rays_planes_gather_times.txt")
REPEATS = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 15
WARMUP = 3
W, H, SAMPLES = 1920, 1080, (8, 1)
COUNT, FACE, MAP = (16, 8, 16), 8, capi.VolumeMap(8, 5)

sc = Scene.golden("dragon")
p = sc.frame_params(width=W, height=H, samples=8, max_reflections=4, use_filter=1)


def params(samples, bounces):
    t = capi.TraceParams.of_frame(p)
    t.samples, t.max_reflections = samples, bounces
    return t


ctx = capi.Context(0)
stream = torch.cuda.Stream()
ctx.set_stream(stream.cuda_stream)
ctx.update_scene(sc)
d_rays = ctx.camera_rays_device(capi.Camera.pinhole(p), W, H)
d_rows = torch.empty((W * H, 32), dtype=torch.uint8, device="cuda")
d_out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
ctx.trace_rays_device(d_rays, params(1, 1), d_rows)
ctx.sync()
# the grid: COUNT probes over the first hit points, a twentieth of their extent around them (tools/rays_gather_time.py's)
rays = d_rays.cpu().numpy()
cols = capi.unpack_radiance(d_rows)
hit = cols["entry"] != -1
points = rays[hit, 0:3].astype(np.float64) + rays[hit, 4:7].astype(np.float64) * cols["s"][hit, None]
lo, hi = points.min(axis=0), points.max(axis=0)
pad = (hi - lo).max() * 0.05
lo, hi = lo - pad, hi + pad
grid = capi.VolumeGrid(tuple(lo), tuple((hi - lo) / (np.array(COUNT) - 1)), COUNT, 0.01 * float((hi - lo).max()), 0.05, capi.VOLUME_VISIBILITY)
d_sh, d_maps = ctx.volume_bake_map_device(grid, params(8, 4), capi.ProbeParams(FACE), MAP)
ctx.sync()
del d_rows
volume = ctx.gather_volume(grid, d_sh, MAP, d_maps)

plain = {(s, k): (lambda s, k: lambda: ctx.ray_image_device(d_rays, W, H, params(s, k), True, d_out))(s, k) for s in SAMPLES for k in (1, 2, 3, 4)}
gather = {(s, k): (lambda s, k: lambda: ctx.ray_image_gather_device(d_rays, W, H, params(s, k), volume, True, d_out))(s, k) for s in SAMPLES for k in (1, 2, 3)}
PLAIN, GATHER = "flx_rays_image_device, %d samples, K = %d", "flx_rays_image_gather_device, %d samples, K = %d"
calls = []
for s in SAMPLES:
    calls += [(PLAIN % (s, k), plain[(s, k)]) for k in (1, 2, 3, 4)] + [(GATHER % (s, k), gather[(s, k)]) for k in (1, 2, 3)]
if "--profile-once" in sys.argv:
    for name, call in calls:
        call()
    ctx.sync()
    ctx.close()
    sys.exit(0)

gather[(8, 2)]()
ctx.sync()
last = ctx.last_planes_gather()

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
lines = ["ray images with a volume on the dragon scene (tests/golden/ref_dragon.flxs.gz): the %d x %d pinhole camera's %d rays made on the device; a %d x %d x %d volume with a map "
         "(size %d, sharpness %d), baked on the device with face size %d; %s, %d CUs" % (W, H, W * H, COUNT[0], COUNT[1], COUNT[2], MAP.size, MAP.sharpness, FACE, info[0], info[1]),
         "GPU ms between two events around each call (planes kernel and denoise chain), the %d calls in turn, median of %d rounds after %d warm-up rounds [min .. max]; each call timed "
         "alone, under no profiler" % (len(calls), REPEATS, WARMUP), ""]
for name, _ in calls:
    lines.append("  %-52s %8.3f ms [%8.3f .. %8.3f]" % (name, med[name], min(ms[name]), max(ms[name])))
for s in SAMPLES:
    lines += ["", "THE BAR at %d sample(s) — gather at K bounces against the plain image at K + 1 (the tail against the bounce it replaces):" % s]
    for k in (1, 2, 3):
        new, old = GATHER % (s, k), PLAIN % (s, k + 1)
        apart = min(ms[new]) > max(ms[old]) or max(ms[new]) < min(ms[old])
        lines.append("  gather(%d) / plain(%d)  %6.3f  (%+8.3f ms; %s the two calls' min .. max)  %s" % (
            k, k + 1, med[new] / med[old], med[new] - med[old], "OUTSIDE" if apart else "inside", "HOLDS" if med[new] < med[old] and apart else "DOES NOT HOLD"))
    lines += ["", "the overhead at %d sample(s) — gather at K bounces against the plain image at K:" % s]
    for k in (1, 2, 3):
        new, old = GATHER % (s, k), PLAIN % (s, k)
        lines.append("  gather(%d) / plain(%d)  %6.3f  (%+8.3f ms)" % (k, k, med[new] / med[old], med[new] - med[old]))
lines += ["", "the 1080p image with a volume: %d slab(s) of at most %d rays, %d workgroups of 256 lanes in the planes kernel, lockstep %d, flags %d" % (
    last["slabs"], last["slab"], last["groups"], last["lockstep"], last["flags"])]
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("\n".join(lines), flush=True)
ctx.close()
