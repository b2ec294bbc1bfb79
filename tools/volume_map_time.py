#!/usr/bin/env python3
"""What directional visibility costs (csrc/flx_volume_map.hip: k_probe_map; csrc/flx_volume.hip: k_volume_irradiance_map) beside what the volume cost without it.
The bake: profiles/probes.txt's configuration — a 16 x 16 x 8 grid of 2048 probes over the dragon scene, 2 samples, 3 bounces, face sizes 8 and 16 —, map sizes 8 and
16, exponent 32 (sharpness 5).  The lookup: the dragon's 1920 x 1080 frame over that grid baked with face size 8, with and without maps.
Timed with device events on the context's stream around each call, the calls in turn, round after round, median of REPEATS rounds after WARMUP [min .. max]:
  flx_volume_bake_device                   the bake without maps
  flx_volume_bake_map_device               the bake with maps: k_probe_map beside k_probe_sh on each chunk's radiance
  flx_probe_map_device                     k_probe_map alone, on radiance rows traced once for it
  flx_probe_reduce_device                  k_probe_sh alone, on the same rows
  hipMemcpyDtoDAsync                       the yardstick: the radiance rows' bytes, read and written by the copy
  flx_frame_irradiance_device              the frame's lookup without maps
  flx_frame_irradiance_map_device          ... with maps
  flx_volume_irradiance[_map]_device       the lookup kernels alone, on the frame's position and normal planes
THE BASELINE IS THE PARENT COMMIT'S LIBRARY, never the code under test: run the tool a second time with --baseline and FLX_LIB naming a library built from the parent
commit; it then times flx_volume_bake_device and flx_frame_irradiance_device alone, the same inputs, the same way.
Once, outside the timed region, the fused bake is held against the plain bake's SH rows and against flx_probe_map_device's rows, bit for bit.  GPU box.

usage: volume_map_time.py [--out FILE] [--repeats 15] [--baseline] [--small]      (its output is recorded in profiles/volume_map.txt; --small: a 4 x 4 x 2 grid and
256 x 144, to try the tool)"""
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
BASELINE = "--baseline" in sys.argv
SMALL = "--small" in sys.argv
WARMUP = 3
GRID = (4, 4, 2) if SMALL else (16, 16, 8)
W, H = (256, 144) if SMALL else (1920, 1080)
N = W * H
SHARPNESS = 5
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
info = ctx.device_info()
sc = Scene.golden("dragon")
ctx.update_scene(sc)
p = sc.frame_params(width=256, height=144, samples=2, max_reflections=3, use_filter=0)
t = capi.TraceParams.of_frame(p)
frame = sc.frame_params(width=W, height=H, samples=1, max_reflections=2, use_filter=0)
# the grid: over the first hits of the scene's own camera, as tools/probe_time.py lays it
eye = ctx.camera_rays_device(capi.Camera.pinhole(p), 256, 144)
d_hits = ctx.cast_rays_device(eye, what=capi.RAYS_CLOSEST)
ctx.sync()
hits = capi.unpack_hits(d_hits)
eye = eye.cpu().numpy()
seen = hits["entry"] >= 0
points = eye[seen, 0:3] + hits["suv"][seen, 0:1] * eye[seen, 4:7]
lo, hi = points.min(axis=0), points.max(axis=0)
lo, hi = lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo)
spacing = [(hi[a] - lo[a]) / (GRID[a] - 1) for a in range(3)]
grid = capi.VolumeGrid(tuple(lo), spacing, GRID, normal_bias=0.25 * min(spacing), floor=0.05)
n = grid.probes
hip = hip_runtime()
hip.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
hip.hipMemcpyDtoDAsync.restype = C.c_int
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(calls):
    """-> ({label: median ms}, the rows as printed)"""
    ms = {label: [] for label, _ in calls}
    for k in range(WARMUP + REPEATS):
        for label, call in calls:
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            if k >= WARMUP:
                ms[label].append(e0.elapsed_time(e1))
    med = {label: float(np.median(v)) for label, v in ms.items()}
    return med, ["  %-58s %9.4f ms [%9.4f .. %9.4f]" % (label, med[label], min(ms[label]), max(ms[label])) for label, _ in calls]


lines = ["directional visibility, %d x %d x %d = %d probes over the dragon, 2 samples, 3 bounces; %s, %d CUs%s" % (
             GRID + (n, info[0], info[1], "; THE BASELINE: FLX_LIB = %s" % os.environ.get("FLX_LIB") if BASELINE else "")),
         "grid from (%.3f, %.3f, %.3f) to (%.3f, %.3f, %.3f)" % (tuple(lo) + tuple(hi)),
         "GPU ms between two events around each call, the calls in turn, median of %d rounds after %d warm-up rounds [min .. max]" % (REPEATS, WARMUP)]
d_sh = torch.empty((n, 36), dtype=torch.float32, device="cuda")
d_image = torch.empty((N, 4), dtype=torch.float32, device="cuda")
for w in (8, 16):
    rays = 6 * w * w
    params = capi.ProbeParams(face_size=w)
    if BASELINE:
        med, rows = timed([("flx_volume_bake_device", lambda: ctx.volume_bake_device(grid, t, params, out=d_sh))])
        lines += ["face size %d (%d rays a probe, %d rays)" % (w, rays, n * rays)] + rows
        continue
    d_positions = ctx.volume_positions_device(grid)
    d_rays = ctx.probe_rays_device(d_positions, w)
    d_rows = torch.empty((n * rays, 32), dtype=torch.uint8, device="cuda")
    ctx.trace_rays_ordered_device(d_rays, t, out=d_rows, order=0)
    ctx.sync()
    del d_rays
    d_copy = torch.empty_like(d_rows)
    radiance_bytes = n * rays * 32

    def copy_call():
        rc = hip.hipMemcpyDtoDAsync(d_copy.data_ptr(), d_rows.data_ptr(), radiance_bytes, stream.cuda_stream)
        assert rc == 0, rc

    for m in (8, 16):
        vmap = capi.VolumeMap(m, SHARPNESS)
        d_maps, d_maps2, d_sh2 = torch.empty((n * m * m, 4), dtype=torch.float32, device="cuda"), torch.empty((n * m * m, 4), dtype=torch.float32, device="cuda"), torch.empty_like(d_sh)
        # ---- once, outside the timed region ----
        ctx.volume_bake_device(grid, t, params, out=d_sh)
        ctx.volume_bake_map_device(grid, t, params, vmap, out=d_sh2, maps=d_maps)
        ctx.probe_map_device(d_rows, n, w, vmap, out=d_maps2)
        ctx.sync()
        assert torch.equal(d_sh.view(torch.int32), d_sh2.view(torch.int32)), "the fused bake's SH rows against the plain bake's"
        assert torch.equal(d_maps.view(torch.int32), d_maps2.view(torch.int32)), "the fused bake's maps against flx_probe_map_device's"
        assert bool(torch.isfinite(d_maps).all())
        med, rows = timed([("flx_volume_bake_device", lambda: ctx.volume_bake_device(grid, t, params, out=d_sh)),
                           ("flx_volume_bake_map_device", lambda: ctx.volume_bake_map_device(grid, t, params, vmap, out=d_sh2, maps=d_maps)),
                           ("flx_probe_map_device", lambda: ctx.probe_map_device(d_rows, n, w, vmap, out=d_maps2)),
                           ("flx_probe_reduce_device", lambda: ctx.probe_reduce_device(d_rows, n, params, out=d_sh2)),
                           ("hipMemcpyDtoDAsync, %d bytes" % radiance_bytes, copy_call)])
        copy_ms = med["hipMemcpyDtoDAsync, %d bytes" % radiance_bytes]
        lines += ["", "face size %d (%d rays a probe, %d rays, %d bytes of radiance), map %d x %d, exponent %d (%d bytes of maps)" % (
                      w, rays, n * rays, radiance_bytes, m, m, 1 << SHARPNESS, n * m * m * 16)] + rows
        lines += ["  k_probe_map reads its rows at %.1f GB/s, the copy reads the same bytes at %.1f GB/s (and writes them): the map over the copy %.2f" % (
                      radiance_bytes / med["flx_probe_map_device"] / 1e6, radiance_bytes / copy_ms / 1e6, med["flx_probe_map_device"] / copy_ms),
                  "  the bake with maps less the bake without: %.4f ms, %.1f %% of the bake without; k_probe_map alone is %.1f %% of it, k_probe_sh alone %.1f %%" % (
                      med["flx_volume_bake_map_device"] - med["flx_volume_bake_device"], 100.0 * (med["flx_volume_bake_map_device"] / med["flx_volume_bake_device"] - 1.0),
                      100.0 * med["flx_probe_map_device"] / med["flx_volume_bake_device"], 100.0 * med["flx_probe_reduce_device"] / med["flx_volume_bake_device"])]
        if w == 8:
            # the lookup over this bake
            d_planes = ctx.frame_surface_device(frame, SURFACE)
            d_plain, d_with = torch.empty_like(d_image), torch.empty_like(d_image)
            ctx.frame_irradiance_device(frame, grid, d_sh, out=d_plain)
            ctx.frame_irradiance_map_device(frame, grid, d_sh, vmap, d_maps, out=d_with)
            ctx.sync()
            differ = float((d_plain != d_with).any(dim=1).float().mean())
            med, rows = timed([("flx_frame_irradiance_device", lambda: ctx.frame_irradiance_device(frame, grid, d_sh, out=d_image)),
                               ("flx_frame_irradiance_map_device", lambda: ctx.frame_irradiance_map_device(frame, grid, d_sh, vmap, d_maps, out=d_image)),
                               ("flx_volume_irradiance_device", lambda: ctx.volume_irradiance_device(grid, d_sh, d_planes[0], d_planes[1], out=d_image)),
                               ("flx_volume_irradiance_map_device", lambda: ctx.volume_irradiance_map_device(grid, d_sh, d_planes[0], d_planes[1], vmap, d_maps, out=d_image))])
            lines += ["  the %d x %d frame's lookup over this bake (%.4f of the pixels differ with maps)" % (W, H, differ)] + ["  " + r for r in rows]
            lines += ["    the maps cost the frame call %.4f ms, %.1f %% of it without; the lookup kernel alone %.4f ms, %.1f %%" % (
                          med["flx_frame_irradiance_map_device"] - med["flx_frame_irradiance_device"], 100.0 * (med["flx_frame_irradiance_map_device"] / med["flx_frame_irradiance_device"] - 1.0),
                          med["flx_volume_irradiance_map_device"] - med["flx_volume_irradiance_device"], 100.0 * (med["flx_volume_irradiance_map_device"] / med["flx_volume_irradiance_device"] - 1.0))]
            del d_planes, d_plain, d_with
        del d_maps, d_maps2, d_sh2
    del d_rows, d_copy
if BASELINE:
    ctx.volume_bake_device(grid, t, capi.ProbeParams(face_size=8), out=d_sh)
    ctx.sync()
    med, rows = timed([("flx_frame_irradiance_device", lambda: ctx.frame_irradiance_device(frame, grid, d_sh, out=d_image))])
    lines += ["the %d x %d frame's lookup over the bake of face size 8" % (W, H)] + rows
else:
    lines.append("verified once per setting outside the timed region: the fused bake's SH rows are the plain bake's and its maps are flx_probe_map_device's, bit for bit")
if out_path:
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
print("\n".join(lines), flush=True)
ctx.close()
