#!/usr/bin/env python3
"""What a volume update costs (csrc/flx_volume_update.hip: k_volume_positions_list, k_volume_blend) beside the full bake it stands in for.
The setting: profiles/probes.txt's — a 16 x 16 x 8 grid of 2048 probes over the dragon scene, 2 samples, 3 bounces, face size 8 —, with maps of 8 x 8 bins
(exponent 32) and without.  AN UPDATE OF EVERY EIGHTH PROBE (first = round % 8, stride 8, 256 entries, hysteresis 0.97) is compared with the full bake of the same
library, and k_volume_blend with a device copy of the bytes it moves.
Timed with device events on the context's stream around each call, the calls in turn, round after round, median of REPEATS rounds after WARMUP [min .. max]:
  flx_volume_bake_device / flx_volume_bake_map_device     the full bake
  flx_volume_update_device, every eighth                  positions of the list, the bake of 256 probes, the blend
  flx_volume_update_device, every probe                   the same for all 2048: a bake and a blend
  flx_volume_blend_device, 256 and 2048 entries           k_volume_blend alone, on rows baked once for it
  hipMemcpyDtoDAsync                                      the yardstick: as many bytes as the blend of 2048 entries reads, read and written by the copy
THE BASELINE IS THE PARENT COMMIT'S LIBRARY, never the code under test: run the tool a second time with --baseline and FLX_LIB naming a library built from the parent
commit; it then times the two bakes alone, the same inputs, the same way.
Once, outside the timed region, an update with h = 0 of every probe onto zeroed rows is held against the bake's rows, bit for bit.  GPU box.

usage: volume_update_time.py [--out FILE] [--repeats 15] [--baseline] [--small]      (its output is recorded in profiles/volume_update.txt; --small: a 4 x 4 x 2 grid,
to try the tool)"""
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
FACE, SIZE, SHARPNESS, STRIDE, H = 8, 8, 5, 8, 0.97


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
some = n // STRIDE
hip = hip_runtime()
hip.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
hip.hipMemcpyDtoDAsync.restype = C.c_int
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
turn = [0]


def timed(calls):
    """-> ({label: median ms}, the rows as printed)"""
    ms = {label: [] for label, _ in calls}
    for k in range(WARMUP + REPEATS):
        turn[0] = k
        for label, call in calls:
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            if k >= WARMUP:
                ms[label].append(e0.elapsed_time(e1))
    med = {label: float(np.median(v)) for label, v in ms.items()}
    return med, ["  %-58s %9.4f ms [%9.4f .. %9.4f]" % (label, med[label], min(ms[label]), max(ms[label])) for label, _ in calls]


def seeded(k):
    return capi.TraceParams(t.samples, t.max_reflections, t.min_importancy, tuple(t.ambient), float(k), t.texture_width)


lines = ["volume updates, %d x %d x %d = %d probes over the dragon, 2 samples, 3 bounces, face size %d; %s, %d CUs%s" % (
             GRID + (n, FACE, info[0], info[1], "; THE BASELINE: FLX_LIB = %s" % os.environ.get("FLX_LIB") if BASELINE else "")),
         "grid from (%.3f, %.3f, %.3f) to (%.3f, %.3f, %.3f)" % (tuple(lo) + tuple(hi)),
         "GPU ms between two events around each call, the calls in turn, median of %d rounds after %d warm-up rounds [min .. max]" % (REPEATS, WARMUP)]
params = capi.ProbeParams(face_size=FACE)
d_sh = torch.empty((n, 36), dtype=torch.float32, device="cuda")
for m in (SIZE, None):
    vmap = capi.VolumeMap(m, SHARPNESS) if m else None
    bins = m * m if m else 0
    d_maps = torch.empty((n * bins, 4), dtype=torch.float32, device="cuda") if m else None
    bake = (lambda: ctx.volume_bake_map_device(grid, t, params, vmap, out=d_sh, maps=d_maps)) if m else (lambda: ctx.volume_bake_device(grid, t, params, out=d_sh))
    bake_name = "flx_volume_bake_map_device" if m else "flx_volume_bake_device"
    title = "maps of %d x %d bins, exponent %d" % (m, m, 1 << SHARPNESS) if m else "no maps"
    if BASELINE:
        med, rows = timed([(bake_name, bake)])
        lines += ["", title] + rows
        continue
    # ---- once, outside the timed region: h = 0 of every probe onto zeroed rows is the bake ----
    bake()
    r_sh, r_maps = torch.zeros_like(d_sh), torch.zeros_like(d_maps) if m else None
    torch.cuda.synchronize()
    state = ctx.volume_update_device(grid, t, params, vmap, capi.VolumeUpdate(0.0, 0, 1), r_sh, r_maps, None, n, state=True)
    ctx.sync()
    taken = state == 1                           # (a bake row that holds a NaN is kept out: its probe stays zeroed)
    kept = int((state == 2).sum())
    assert int(taken.sum()) + kept == n and bool(torch.isfinite(d_sh[taken]).all()) and not bool(torch.isfinite(d_sh[~taken]).all(dim=1).any())
    assert torch.equal(d_sh.view(torch.int32)[taken], r_sh.view(torch.int32)[taken]), "an update with h = 0 against the bake's SH rows"
    if m:
        fine = torch.isfinite(d_maps).all(dim=1) & taken.repeat_interleave(bins)
        assert torch.equal(d_maps.view(torch.int32)[fine], r_maps.view(torch.int32)[fine]), "an update with h = 0 against the bake's maps"
    # the blend alone: new rows baked once for it
    new_sh, new_maps = torch.empty_like(d_sh), torch.empty_like(d_maps) if m else None
    if m:
        ctx.volume_bake_map_device(grid, seeded(7), params, vmap, out=new_sh, maps=new_maps)
    else:
        ctx.volume_bake_device(grid, seeded(7), params, out=new_sh)
    ctx.sync()
    moved = n * (288 + 32 * bins)                # the bytes the blend of every probe reads; it writes half as many
    d_from, d_to = torch.empty((moved,), dtype=torch.uint8, device="cuda"), torch.empty((moved,), dtype=torch.uint8, device="cuda")

    def copy_call():
        rc = hip.hipMemcpyDtoDAsync(d_to.data_ptr(), d_from.data_ptr(), moved, stream.cuda_stream)
        assert rc == 0, rc

    every = capi.VolumeUpdate(H, 0, 1)
    med, rows = timed([(bake_name, bake),
                       ("flx_volume_update_device, every eighth (%d entries)" % some,
                        lambda: ctx.volume_update_device(grid, seeded(turn[0]), params, vmap, capi.VolumeUpdate(H, turn[0] % STRIDE, STRIDE), r_sh, r_maps, None, some)),
                       ("flx_volume_update_device, every probe (%d entries)" % n, lambda: ctx.volume_update_device(grid, seeded(turn[0]), params, vmap, every, r_sh, r_maps, None, n)),
                       ("flx_volume_blend_device, %d entries" % some,
                        lambda: ctx.volume_blend_device(grid, vmap, capi.VolumeUpdate(H, turn[0] % STRIDE, STRIDE), new_sh, r_sh, new_maps, r_maps, None, some)),
                       ("flx_volume_blend_device, %d entries" % n, lambda: ctx.volume_blend_device(grid, vmap, every, new_sh, r_sh, new_maps, r_maps, None, n)),
                       ("hipMemcpyDtoDAsync, %d bytes" % moved, copy_call)])
    update_ms, all_ms = med["flx_volume_update_device, every eighth (%d entries)" % some], med["flx_volume_update_device, every probe (%d entries)" % n]
    blend_ms, copy_ms = med["flx_volume_blend_device, %d entries" % n], med["hipMemcpyDtoDAsync, %d bytes" % moved]
    lines += ["", title + " (%d of %d bake rows hold a NaN and are kept out)" % (kept, n)] + rows
    lines += ["  an update of every eighth probe is %.3f of the full bake; of every probe %.3f of it" % (update_ms / med[bake_name], all_ms / med[bake_name]),
              "  k_volume_blend of %d entries is %.2f %% of an update of every eighth and %.2f %% of the full bake; of %d entries %.2f %% of the full bake" % (
                  some, 100.0 * med["flx_volume_blend_device, %d entries" % some] / update_ms, 100.0 * med["flx_volume_blend_device, %d entries" % some] / med[bake_name], n,
                  100.0 * blend_ms / med[bake_name]),
              "  k_volume_blend of %d entries reads %d bytes and writes %d: %.1f GB/s moved; the copy reads and writes %d each: %.1f GB/s moved; the blend over the copy %.2f" % (
                  n, moved, moved // 2, 1.5 * moved / blend_ms / 1e6, moved, 2.0 * moved / copy_ms / 1e6, blend_ms / copy_ms)]
    assert bool(torch.isfinite(r_sh).all())
    del r_sh, r_maps, new_sh, new_maps, d_from, d_to, d_maps
if not BASELINE:
    lines.append("verified once per setting outside the timed region: an update with h = 0 of every probe onto zeroed rows is the bake's rows, bit for bit")
if out_path:
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
print("\n".join(lines), flush=True)
ctx.close()
