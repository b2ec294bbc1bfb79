#!/usr/bin/env python3
"""What probe relocation costs (csrc/flx_volume_relocate.hip: k_probe_relocate, k_volume_positions_offset; csrc/flx_volume.hip: the relocated lookups).
The setting: profiles/volume_update.txt's — a 16 x 16 x 8 grid of 2048 probes over the dragon scene, 2 samples, 3 bounces, face size 8 —, and the lookup of
profiles/volume.txt: the dragon's 1920 x 1080 frame, its position plane and its normal plane made once.
Timed with device events on the context's stream around each call, the calls in turn, round after round, median of REPEATS rounds after WARMUP [min .. max]:
  flx_probe_relocate_device                                k_probe_relocate alone over the planes of all 2048 probes, made once for it
  hipMemcpyDtoDAsync                                       the yardstick: as many bytes as the reduction reads (two planes of 2048 x 384 rows)
  flx_volume_relocate_device                               one whole pass: positions, rays, the cast with its surface rows, the reduction
  flx_volume_bake_device                                   the bake of the same grid and face size it is held against
  flx_volume_irradiance_device / _map_device               the plain lookups of the frame's 2 073 600 points
  flx_volume_irradiance_relocated_device, two ways         the same with offsets, without a map and with one
Once, outside the timed region, three passes and a frozen one are run and the states counted, and the relocated lookup with zero offsets is held against the plain
lookup's rows, bit for bit.  GPU box.

usage: volume_relocate_time.py [--out FILE] [--repeats 15] [--small]      (its output is recorded in profiles/volume_relocate.txt; --small: a 4 x 4 x 2 grid and a
256 x 144 frame, to try the tool)"""
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
GRID = (4, 4, 2) if SMALL else (16, 16, 8)
FRAME = (256, 144) if SMALL else (1920, 1080)
FACE, SIZE, SHARPNESS = 8, 8, 5


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
# the grid: over the first hits of the scene's own camera, as tools/volume_update_time.py lays it
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
n, rays = grid.probes, capi.probe_ray_count(FACE)
relocate = capi.VolumeRelocate(0.25, 0.2 * min(spacing), 2.0 * max(spacing), 0.45)
frozen = capi.VolumeRelocate(relocate.back_share, relocate.min_front, relocate.reach, relocate.limit, capi.RELOCATE_FREEZE)
hip = hip_runtime()
hip.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
hip.hipMemcpyDtoDAsync.restype = C.c_int
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(calls):
    """-> ({label: (median, min, max) ms}, the rows as printed)"""
    ms = {label: [] for label, _ in calls}
    for k in range(WARMUP + REPEATS):
        for label, call in calls:
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            if k >= WARMUP:
                ms[label].append(e0.elapsed_time(e1))
    med = {label: (float(np.median(v)), min(v), max(v)) for label, v in ms.items()}
    return med, ["  %-58s %9.4f ms [%9.4f .. %9.4f]" % ((label,) + med[label]) for label, _ in calls]


lines = ["probe relocation, %d x %d x %d = %d probes over the dragon, face size %d (%d rays a probe); lookups of a %d x %d frame; %s, %d CUs" % (
             GRID + (n, FACE, rays) + FRAME + (info[0], info[1])),
         "grid from (%.3f, %.3f, %.3f) to (%.3f, %.3f, %.3f); back_share %.2f, min_front %.3f, reach %.3f, limit %.2f" % (
             tuple(lo) + tuple(hi) + (relocate.back_share, relocate.min_front, relocate.reach, relocate.limit)),
         "GPU ms between two events around each call, the calls in turn, median of %d rounds after %d warm-up rounds [min .. max]" % (REPEATS, WARMUP)]
# ---- once, outside the timed region: three passes and a frozen one ----
d_offsets = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
for k in range(4):
    ctx.volume_relocate_device(grid, frozen if k == 3 else relocate, FACE, d_offsets, t.texture_width)
ctx.sync()
offsets = d_offsets.cpu().numpy()
states = capi.relocate_states(offsets)
moved = int((np.abs(offsets[:, :3]).max(axis=1) > 0).sum())
lines.append("after three passes and a frozen one: %d of %d probes moved, %d inactive, %d rejected; rules 1 / 2 / 3 of the frozen pass: %d / %d / %d" % (
    moved, n, int((states & 1 != 0).sum()), int((states & 8 != 0).sum()), int((capi.relocate_rule(states) == 1).sum()), int((capi.relocate_rule(states) == 2).sum()),
    int((capi.relocate_rule(states) == 3).sum())))
# the reduction alone: the planes of every probe, made once
d_positions = ctx.volume_positions_offset_device(grid, d_offsets)
d_rays = ctx.probe_rays_device(d_positions, FACE)
planes = ctx.surface_rays_device(d_rays.view(-1, 8), capi.SURFACE_HIT | capi.SURFACE_NORMAL, t.texture_width)
ctx.sync()
read = 2 * n * rays * 16
d_from, d_to = torch.empty((read,), dtype=torch.uint8, device="cuda"), torch.empty((read,), dtype=torch.uint8, device="cuda")
d_scratch = d_offsets.clone()
params = capi.ProbeParams(face_size=FACE)
d_sh = torch.empty((n, 36), dtype=torch.float32, device="cuda")


def copy_call():
    rc = hip.hipMemcpyDtoDAsync(d_to.data_ptr(), d_from.data_ptr(), read, stream.cuda_stream)
    assert rc == 0, rc


med, rows = timed([("flx_probe_relocate_device, %d probes" % n, lambda: ctx.probe_relocate_device(grid, frozen, planes[0], planes[1], n, FACE, d_scratch)),
                   ("hipMemcpyDtoDAsync, %d bytes" % read, copy_call),
                   ("flx_volume_relocate_device, one pass", lambda: ctx.volume_relocate_device(grid, frozen, FACE, d_scratch, t.texture_width)),
                   ("flx_volume_bake_device", lambda: ctx.volume_bake_device(grid, t, params, out=d_sh))])
lines += ["", "the reduction and the whole pass"] + rows
reduce_ms, copy_ms = med["flx_probe_relocate_device, %d probes" % n][0], med["hipMemcpyDtoDAsync, %d bytes" % read][0]
pass_ms, bake_ms = med["flx_volume_relocate_device, one pass"][0], med["flx_volume_bake_device"][0]
lines += ["  k_probe_relocate reads %d bytes of planes: %.1f GB/s; the copy reads and writes as many: %.1f GB/s moved; the reduction over the copy %.2f" % (
              read, read / reduce_ms / 1e6, 2.0 * read / copy_ms / 1e6, reduce_ms / copy_ms),
          "  one pass is %.3f of a bake of the same grid and face size; the reduction is %.2f %% of a pass" % (pass_ms / bake_ms, 100.0 * reduce_ms / pass_ms)]
# ---- the lookups ----
frame = sc.frame_params(width=FRAME[0], height=FRAME[1], samples=1, max_reflections=1, use_filter=0)
surface = ctx.frame_surface_device(frame, capi.SURFACE_POSITION | capi.SURFACE_NORMAL)
vmap = capi.VolumeMap(SIZE, SHARPNESS)
d_sh, d_maps = ctx.volume_bake_relocated_device(grid, t, params, d_offsets, vmap)
ctx.sync()
points_n = FRAME[0] * FRAME[1]
out = torch.empty((points_n, 4), dtype=torch.float32, device="cuda")
d_zero = torch.zeros_like(d_offsets)
torch.cuda.synchronize()                       # (torch fills it on its own stream: the context's must not read it sooner)
plain = ctx.volume_irradiance_device(grid, d_sh, surface[0], surface[1])
same = ctx.volume_irradiance_relocated_device(grid, d_sh, surface[0], surface[1], d_zero)
ctx.sync()
a, b = plain.view(torch.int32), same.view(torch.int32)
assert bool(((a == b) | (torch.isnan(plain) & torch.isnan(same))).all()), "zero offsets against the plain lookup"
med, rows = timed([("flx_volume_irradiance_device", lambda: ctx.volume_irradiance_device(grid, d_sh, surface[0], surface[1], out=out)),
                   ("flx_volume_irradiance_relocated_device", lambda: ctx.volume_irradiance_relocated_device(grid, d_sh, surface[0], surface[1], d_offsets, out=out)),
                   ("flx_volume_irradiance_relocated_device, zero offsets", lambda: ctx.volume_irradiance_relocated_device(grid, d_sh, surface[0], surface[1], d_zero, out=out)),
                   ("flx_volume_irradiance_map_device", lambda: ctx.volume_irradiance_map_device(grid, d_sh, surface[0], surface[1], vmap, d_maps, out=out)),
                   ("flx_volume_irradiance_relocated_device, map", lambda: ctx.volume_irradiance_relocated_device(grid, d_sh, surface[0], surface[1], d_offsets, vmap, d_maps, out=out))])
lines += ["", "the lookups of %d points" % points_n] + rows
for plain_name, moved_name in (("flx_volume_irradiance_device", "flx_volume_irradiance_relocated_device"), ("flx_volume_irradiance_map_device", "flx_volume_irradiance_relocated_device, map")):
    (pm, plo, phi), (rm, rlo, rhi) = med[plain_name], med[moved_name]
    lines.append("  %s over %s: %.3f (medians); the ranges %s" % (moved_name, plain_name, rm / pm, "overlap" if rlo <= phi and plo <= rhi else "do not overlap"))
lines.append("verified once outside the timed region: the relocated lookup with zero offsets is the plain lookup's rows, bit for bit")
if out_path:
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
print("\n".join(lines), flush=True)
ctx.close()
