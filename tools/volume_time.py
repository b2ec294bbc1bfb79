#!/usr/bin/env python3
"""What the probe-volume lookup costs (flx_volume_irradiance_device, flx_frame_irradiance_device; csrc/flx_volume.hip: k_volume_irradiance) on the frame it was
made for: the dragon scene at 1920 x 1080, grids of 8 x 8 x 8 and 32 x 32 x 32 probes over the bounding box of the frame's first hits (shrunk by a tenth on every
side), baked once with face size 4, 1 sample, 2 bounces.
Timed with device events on the context's stream around each call, the calls in turn, round after round, median of REPEATS rounds after WARMUP [min .. max]:
  lookup, frame order                   flx_volume_irradiance_device on the frame's position and normal planes as flx_frame_surface_device left them
  lookup, shuffled                      the same points in a random order: a wave's lanes lie in as many cells
  hipMemcpyDtoDAsync                    the yardstick: the 48 bytes a point the kernel must move (two planes in, one out), read and written by the copy
  flx_frame_surface_device              POSITION | NORMAL alone
  flx_frame_irradiance_device           the two in one call
Once, outside the timed region, the fused call is held against the two calls and the shuffled points' rows against the frame's, bit for bit.  GPU box.
(The uniform path for waves inside one cell, which this tool timed against the gather through a debug knob while both existed, is recorded in profiles/volume.txt.)

usage: volume_time.py [--out FILE] [--repeats 15] [--small]      (its output is recorded in profiles/volume.txt; --small: 256 x 144 and a 4 x 4 x 4 grid, to try the tool)"""
import ctypes as C
import os
import sys

import numpy as np
import torch                                   # (before the library: INTEGRATION.md, Build)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "web-ray-tracer_amd"))
from flexlight_hip import capi
from flexlight_hip.scene_io import Scene

out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
REPEATS = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 15
SMALL = "--small" in sys.argv
WARMUP = 3
W, H = (256, 144) if SMALL else (1920, 1080)
N = W * H
GRIDS = ((4, 4, 4),) if SMALL else ((8, 8, 8), (32, 32, 32))
SURFACE = capi.SURFACE_POSITION | capi.SURFACE_NORMAL


def hip_runtime():
    """the HIP runtime this process has loaded already (torch's), by the path it was mapped from"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime is loaded")


ctx = capi.Context(0)
stream = torch.cuda.Stream()
ctx.set_stream(stream.cuda_stream)
sc = Scene.golden("dragon")
ctx.update_scene(sc)
p = sc.frame_params(width=W, height=H, samples=1, max_reflections=2, use_filter=0)
t = capi.TraceParams.of_frame(p)
q = capi.ProbeParams(face_size=4)
info = ctx.device_info()

d_planes = torch.empty((2, N, 4), dtype=torch.float32, device="cuda")
ctx.frame_surface_device(p, SURFACE, d_planes)
ctx.sync()
planes = d_planes.cpu().numpy()
hit = planes[0][:, 3] != 0.0
lo, hi = planes[0][hit][:, :3].min(axis=0), planes[0][hit][:, :3].max(axis=0)
lo, hi = lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo)
order = torch.from_numpy(np.random.default_rng(2024).permutation(N)).cuda()
d_shuffled = d_planes[:, order].contiguous()
d_out, d_out2 = torch.empty((N, 4), dtype=torch.float32, device="cuda"), torch.empty((N, 4), dtype=torch.float32, device="cuda")
copy_bytes = N * 48
d_src, d_dst = torch.empty((copy_bytes,), dtype=torch.uint8, device="cuda"), torch.empty((copy_bytes,), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
hip = hip_runtime()
hip.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
hip.hipMemcpyDtoDAsync.restype = C.c_int


def copy_call():
    rc = hip.hipMemcpyDtoDAsync(d_dst.data_ptr(), d_src.data_ptr(), copy_bytes, stream.cuda_stream)
    assert rc == 0, rc


def lookup(grid, d_sh, d_points, out):
    return lambda: ctx.volume_irradiance_device(grid, d_sh, d_points[0], d_points[1], out=out)


lines = ["probe volumes on the dragon scene (tests/golden/ref_dragon.flxs.gz): the %d x %d frame's %d points, %.4f of them hits; %s, %d CUs" % (W, H, N, hit.mean(), info[0], info[1]),
         "grid from (%.3f, %.3f, %.3f) to (%.3f, %.3f, %.3f); baked with face size 4, 1 sample, 2 bounces" % (tuple(lo) + tuple(hi)),
         "GPU ms between two events around each call, the calls in turn, median of %d rounds after %d warm-up rounds [min .. max]" % (REPEATS, WARMUP)]
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for count in GRIDS:
    spacing = [(hi[a] - lo[a]) / (count[a] - 1) for a in range(3)]
    grid = capi.VolumeGrid(tuple(lo), spacing, count, normal_bias=0.25 * min(spacing), floor=0.05)
    d_sh = ctx.volume_bake_device(grid, t, q)
    ctx.sync()
    # ---- once, outside the timed region ----
    ctx.volume_irradiance_device(grid, d_sh, d_planes[0], d_planes[1], out=d_out)
    ctx.frame_irradiance_device(p, grid, d_sh, out=d_out2)
    ctx.sync()
    assert torch.equal(d_out.view(torch.int32), d_out2.view(torch.int32)), "the fused call against its two calls"
    ctx.volume_irradiance_device(grid, d_sh, d_shuffled[0], d_shuffled[1], out=d_out2)
    ctx.sync()
    assert torch.equal(d_out[order].view(torch.int32), d_out2.view(torch.int32)), "the shuffled points against the frame's"
    image = d_out.cpu().numpy()
    assert np.isfinite(image).all() and (image[hit][:, 3] > 0).all() and (image[~hit] == 0).all()

    calls = [("lookup, frame order", lookup(grid, d_sh, d_planes, d_out)), ("lookup, shuffled", lookup(grid, d_sh, d_shuffled, d_out)),
             ("hipMemcpyDtoDAsync, %d bytes" % copy_bytes, copy_call), ("flx_frame_surface_device, POSITION | NORMAL", lambda: ctx.frame_surface_device(p, SURFACE, d_planes)),
             ("flx_frame_irradiance_device", lambda: ctx.frame_irradiance_device(p, grid, d_sh, out=d_out))]
    ms = {name: [] for name, _ in calls}
    for k in range(WARMUP + REPEATS):
        for name, call in calls:
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            if k >= WARMUP:
                ms[name].append(e0.elapsed_time(e1))
    med = {name: float(np.median(v)) for name, v in ms.items()}
    lines += ["", "%d x %d x %d = %d probes (%d bytes of SH rows), spacing (%.3f, %.3f, %.3f)" % (tuple(count) + (grid.probes, grid.probes * 144) + tuple(spacing))]
    for name, _ in calls:
        lines.append("  %-58s %8.4f ms [%8.4f .. %8.4f]" % (name, med[name], min(ms[name]), max(ms[name])))
    names = [name for name, _ in calls]
    lines += ["  the copy moves %.1f GB/s (each byte read once and written once); lookup over copy: frame order %.2f, shuffled %.2f; shuffled over frame order %.2f" % (
                  copy_bytes / med[names[2]] / 1e6, med[names[0]] / med[names[2]], med[names[1]] / med[names[2]], med[names[1]] / med[names[0]]),
              "  the fused call less the surface call: %.4f ms" % (med[names[4]] - med[names[3]])]
lines.append("verified once per grid outside the timed region: the fused call equals the surface call followed by the lookup and the shuffled points' rows are the frame's, bit for bit")
if out_path:
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
print("\n".join(lines), flush=True)
ctx.close()
