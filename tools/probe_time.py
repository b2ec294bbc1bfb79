#!/usr/bin/env python3
"""What light probes cost when the device makes, traces and reduces their rays (flx_probes_sh_device, csrc/flx_probes.hip: k_probe_rays, k_probe_sh) against the
route an application had before: a 16 x 16 x 8 grid of 2048 probes over the dragon scene, face size 8 and 16, 2 samples, 3 bounces, order 0 and hits.
The grid spans the bounding box of the first hits of the scene's own camera (256 x 144 rays, flx_rays_cast), shrunk by a tenth on every side.
Timed, each call followed by a wait for the context's stream, on the host's clock (what the caller sees); the calls in turn, round after round, median of REPEATS
rounds after WARMUP [min .. max]:
  flx_probes_sh_device                      positions in, SH rows out: the fused call
  flx_probe_rays_device                     stage 1 alone, into a tensor
  flx_rays_trace_ordered_device             stage 2 alone, on those rays
  flx_probe_reduce_device                   stage 3 alone, on those rows
  hipMemcpyDtoDAsync                        the yardstick of stage 3: the bytes it reads, read and written by the copy engine's kernel
  baseline                                  six cube-face cameras a probe through flx_camera_rays_device (five probes, thirty cameras, a call: one launch),
                                            flx_rays_trace_ordered_device, the radiance rows downloaded, the same sums in numpy (float32, the basis and the
                                            weights made once outside the timed region)
  flx_probe_reduce_device, 1 probe w = 64   one wave alone on 24 576 rows: whether a wave per probe starves the machine for few, large probes
Once, outside the timed region, the fused call is held against the three stages bit for bit and the baseline's sums against the fused rows.  GPU box.

usage: probe_time.py [--out FILE] [--repeats 10] [--stages-only]      (its output is recorded in profiles/probes.txt; --stages-only: the three stages and the
copy alone, a few rounds, for a kernel trace)"""
import os
import sys
import time

import numpy as np
import torch                                   # (before the library: INTEGRATION.md, Build)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "web-ray-tracer_amd"))
from flexlight_hip import capi
from flexlight_hip.scene_io import Scene

out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
REPEATS = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 10
STAGES_ONLY = "--stages-only" in sys.argv
WARMUP = 2
GRID = (16, 16, 8)
K = (0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396)

ctx = capi.Context(0)
info = ctx.device_info()
sc = Scene.golden("dragon")
p = sc.frame_params(width=256, height=144, samples=2, max_reflections=3, use_filter=0)
t = capi.TraceParams.of_frame(p)
ctx.update_scene(sc)
# the grid: over the first hits of the scene's own camera
eye = ctx.camera_rays_device(capi.Camera.pinhole(p), 256, 144)
d_hits = ctx.cast_rays_device(eye, what=capi.RAYS_CLOSEST)
ctx.sync()
hits = capi.unpack_hits(d_hits)
eye = eye.cpu().numpy()
seen = hits["entry"] >= 0
points = eye[seen, 0:3] + hits["suv"][seen, 0:1] * eye[seen, 4:7]
lo, hi = points.min(axis=0), points.max(axis=0)
lo, hi = lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo)
axes = [np.linspace(lo[k], hi[k], GRID[k]) for k in range(3)]
positions = np.zeros((GRID[0] * GRID[1] * GRID[2], 4), np.float32)
positions[:, :3] = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
n = len(positions)
d_positions = torch.from_numpy(positions).cuda()
lines = ["light probes, %d x %d x %d = %d probes over the dragon, 2 samples, 3 bounces; %s, %d CUs" % (GRID + (n,) + (info[0], info[1])),
         "grid from (%.3f, %.3f, %.3f) to (%.3f, %.3f, %.3f)" % (tuple(lo) + tuple(hi)),
         "host ms of call + wait for the stream, the calls in turn, median of %d rounds after %d warm-up rounds [min .. max]" % (REPEATS, WARMUP)]


def weights_and_basis(w):
    """float32 [6 w w, 10]: b_i d_omega for i = 0 .. 8 and d_omega, from the generated rays' directions (the baseline's tables, made once)"""
    rays = ctx.probe_rays(np.zeros((1, 4), np.float32), w)
    x, y, z = rays[:, 4].astype(np.float64), rays[:, 5].astype(np.float64), rays[:, 6].astype(np.float64)
    px, row = np.meshgrid(np.arange(w), np.arange(w))
    sx, sy = ((px + 0.5) / w * 2 - 1).reshape(-1), ((w - 1 - row + 0.5) / w * 2 - 1).reshape(-1)
    q = np.tile(1 + sx * sx + sy * sy, 6)
    dw = (4.0 / (w * w)) / (q * np.sqrt(q))
    b = np.stack([K[0] * np.ones_like(x), K[1] * y, K[1] * z, K[1] * x, K[2] * x * y, K[2] * y * z, K[3] * (3 * z * z - 1), K[2] * x * z, K[4] * (x * x - y * y)], axis=-1)
    return np.concatenate([b * dw[:, None], dw[:, None]], axis=1).astype(np.float32)


def timed(calls, repeats, warmup):
    ms = {label: [] for label, _ in calls}
    for k in range(warmup + repeats):
        for label, call in calls:
            ctx.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            ctx.sync()
            if label.startswith("hipMemcpy"):
                torch.cuda.synchronize()
            if k >= warmup:
                ms[label].append((time.perf_counter() - t0) * 1e3)
    return ["  %-58s %9.3f ms [%9.3f .. %9.3f]" % (label, float(np.median(ms[label])), min(ms[label]), max(ms[label])) for label, _ in calls]


for w in (8, 16):
    rays = 6 * w * w
    d_rays = torch.empty((n * rays, 8), dtype=torch.float32, device="cuda")
    d_rows = torch.empty((n * rays, 32), dtype=torch.uint8, device="cuda")
    d_copy = torch.empty_like(d_rows)
    d_sh = torch.empty((n, 36), dtype=torch.float32, device="cuda")
    d_sh3 = torch.empty((n, 36), dtype=torch.float32, device="cuda")
    faces = [[capi.Camera.cube_face(tuple(positions[k, :3]), f) for k in range(first, min(n, first + 5)) for f in range(6)] for first in range(0, n, 5)]
    table = weights_and_basis(w)
    for order in (0, capi.TRACE_ORDER_HITS):
        params = capi.ProbeParams(face_size=w, order=order)
        # ---- once, outside the timed region: the fused call against its stages, the baseline's sums against the fused rows ----
        ctx.probes_sh_device(d_positions, t, params, out=d_sh)
        ctx.probe_rays_device(d_positions, w, out=d_rays)
        ctx.trace_rays_ordered_device(d_rays, t, out=d_rows, order=order)
        ctx.probe_reduce_device(d_rows, n, params, out=d_sh3)
        ctx.sync()
        assert torch.equal(d_sh.view(torch.int32), d_sh3.view(torch.int32))
        fused = d_sh.cpu().numpy()

        def baseline():
            for k, cams in enumerate(faces):
                ctx.camera_rays_device(cams, w, w, out=d_rays.data_ptr() + k * 5 * rays * 32)
            ctx.trace_rays_ordered_device(d_rays, t, out=d_rows, order=order)
            ctx.sync()
            rows = d_rows.cpu().numpy().view(np.float32).reshape(n, rays, 8)
            hit = rows[:, :, 3] != 0
            radiance = rows[:, :, 0:3] * hit[:, :, None]
            out = np.zeros((n, 9, 4), np.float32)
            out[:, :, 0:3] = np.einsum("prc,ri->pic", radiance, table[:, 0:9])
            out[:, 0, 3] = table[:, 9].sum()
            out[:, 1, 3] = (hit * table[:, 9]).sum(axis=1)
            out[:, 2, 3] = (hit * table[:, 9] * rows[:, :, 4]).sum(axis=1)
            out[:, 3, 3] = (hit * table[:, 9] * rows[:, :, 4] * rows[:, :, 4]).sum(axis=1)
            return out.reshape(n, 36)

        # (the baseline's rays carry the camera's noise words, six faces sharing one set: its radiance differs from the fused call's by noise, its weights do not)
        base = baseline()
        scale = np.abs(fused[:, 3]).max()
        assert np.abs(base[:, 3] - fused[:, 3]).max() <= 1e-5 * scale
        calls = [("flx_probe_rays_device", lambda: ctx.probe_rays_device(d_positions, w, out=d_rays)),
                 ("flx_rays_trace_ordered_device", lambda: ctx.trace_rays_ordered_device(d_rays, t, out=d_rows, order=order)),
                 ("flx_probe_reduce_device", lambda: ctx.probe_reduce_device(d_rows, n, params, out=d_sh3)),
                 ("hipMemcpyDtoDAsync, %d bytes" % (n * rays * 32), lambda: d_copy.copy_(d_rows))]
        if not STAGES_ONLY:
            calls = [("flx_probes_sh_device", lambda: ctx.probes_sh_device(d_positions, t, params, out=d_sh))] + calls + [("baseline: cameras, trace, download, numpy", baseline)]
        lines.append("face size %d (%d rays a probe, %d rays, %d bytes of radiance), order %s" % (w, rays, n * rays, n * rays * 32, "hits" if order else "0"))
        lines += timed(calls, 3 if STAGES_ONLY else REPEATS, 1 if STAGES_ONLY else WARMUP)
        if STAGES_ONLY:
            break
    del d_rays, d_rows, d_copy

# few, large probes: one wave alone
one = capi.ProbeParams(face_size=64)
d_one = torch.zeros((6 * 64 * 64, 32), dtype=torch.uint8, device="cuda")
d_one_sh = torch.empty((1, 36), dtype=torch.float32, device="cuda")
d_one_copy = torch.empty_like(d_one)
lines.append("one probe of face size 64 (24576 rays, %d bytes of radiance)" % (6 * 64 * 64 * 32))
lines += timed([("flx_probe_reduce_device, 1 probe w = 64", lambda: ctx.probe_reduce_device(d_one, 1, one, out=d_one_sh)),
                ("hipMemcpyDtoDAsync, %d bytes" % (6 * 64 * 64 * 32), lambda: d_one_copy.copy_(d_one))], 3 if STAGES_ONLY else REPEATS, 1 if STAGES_ONLY else WARMUP)
lines.append("  verified once per configuration outside the timed region: the fused call equals its three stages bit for bit")
if out_path:
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
print("\n".join(lines), flush=True)
ctx.close()
