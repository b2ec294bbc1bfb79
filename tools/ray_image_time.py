#!/usr/bin/env python3
"""What a denoised ray image costs (flx_rays_image_device, csrc/flx_rays_planes.hip) against the filtered frame of the same camera (flx_render_device with
use_filter = 1), on two frames of bench.py: cornell.obj 1080p 4 spp 3 bounces (configs[1]) and the dragon 1080p 8 spp 4 bounces.  The rays are the camera's, as
k_primary makes them (origin = the camera, direction = primary_dir_v's bits, noise = the pixel's NDC), row by row.
Timed, each call followed by a wait for the context's stream, on the host's clock (what the caller of the call sees); the calls in turn, round after round, median of
REPEATS rounds after WARMUP [min .. max]:
  flx_rays_image_device            first hits + planes kernel + chain
  flx_rays_planes_device (RGBA8)   first hits + planes kernel
  ... in 8 x 8 tile order          the same rays, permuted so that 64 consecutive rays are an 8 x 8 pixel tile: the coherence the frame kernel's waves have
  flx_rays_cast_device (closest)   first hits alone
  flx_filter_planes_device         the chain alone, over the planes the ray call made
  flx_render_device, use_filter 1  the frame: its per-pixel trace kernel (primary walk inside) + chain
  flx_render_planes_device         the frame's trace alone
  with --temporal N[,N..]: flx_rays_image_temporal_device at each depth N, with the chain and without (the ring keeps wrapping: every call has a full history)
from which the split: planes kernel = planes call - first hits.  Once, outside the timed region, the image is held against the frame bit for bit (they differ where
the frame's hit rule and rayTracer differ, and in what the chain spreads from there).  GPU box.

usage: ray_image_time.py [--out FILE] [--repeats 20] [--temporal N[,N..]] [--only NAME]      (its output is recorded in profiles/rays_planes.txt and, with
--temporal, in profiles/rays_temporal.txt; --only: one of the two frames, by its scene's name)"""
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
REPEATS = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 20
TEMPORAL = [int(x) for x in sys.argv[sys.argv.index("--temporal") + 1].split(",")] if "--temporal" in sys.argv else []
ONLY = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
WARMUP = 3
W, H = 1920, 1080
FRAMES = (("cornell_obj", 4, 3), ("dragon", 8, 4))


def camera_rows(p):
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


ctx = capi.Context(0)
info = ctx.device_info()
lines = ["denoised ray images against filtered frames, %d x %d, the camera's own rays in pixel order; %s, %d CUs" % (W, H, info[0], info[1]),
         "host ms of call + wait for the stream, the calls in turn, median of %d rounds after %d warm-up rounds [min .. max]" % (REPEATS, WARMUP)]
n = W * H
d_image = torch.empty((n, 4), dtype=torch.float32, device="cuda")
d_frame = torch.empty((n, 4), dtype=torch.float32, device="cuda")
d_planes = torch.empty((5, n), dtype=torch.int32, device="cuda")
d_frame_planes = torch.empty((5, n), dtype=torch.int32, device="cuda")
d_hits = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
for name, spp, bounces in FRAMES:
    if ONLY and name != ONLY:
        continue
    sc = Scene.golden(name)
    p = sc.frame_params(width=W, height=H, samples=spp, max_reflections=bounces, use_filter=1)
    t = capi.TraceParams.of_frame(p)
    ctx.update_scene(sc)
    rows = camera_rows(p)
    d_rays = torch.from_numpy(rows).cuda()
    ty, tx, y, x = np.meshgrid(np.arange(H // 8), np.arange(W // 8), np.arange(8), np.arange(8), indexing="ij")      # (1920 x 1080: whole tiles)
    d_tiled = torch.from_numpy(rows[((ty * 8 + y) * W + tx * 8 + x).reshape(-1)]).cuda()
    torch.cuda.synchronize()
    # ---- once, outside the timed region: the image against the library's own filtered frame ----
    ctx.ray_image_device(d_rays, W, H, t, hdr=p.hdr, out=d_image)
    ctx.render_device(p, d_frame.data_ptr())
    ctx.ray_planes_device(d_rays, t, planes8=d_planes)
    ctx.render_planes_device(p, d_frame_planes.data_ptr())
    ctx.sync()
    image, frame = d_image.cpu().numpy(), d_frame.cpu().numpy()
    same = ((image.view(np.uint32) == frame.view(np.uint32)) | (np.isnan(image) & np.isnan(frame))).all(axis=1)
    same_planes = (d_planes.cpu().numpy() == d_frame_planes.cpu().numpy()).all(axis=0)
    assert same_planes.mean() > 0.9 and same.mean() > 0.8, (same_planes.mean(), same.mean())      # (cornell.obj: back faces and shared edges, where the two hit rules part)
    last = ctx.last_ray_planes()
    calls = [("flx_rays_image_device", lambda: ctx.ray_image_device(d_rays, W, H, t, hdr=p.hdr, out=d_image)),
             ("flx_rays_planes_device (RGBA8)", lambda: ctx.ray_planes_device(d_rays, t, planes8=d_planes)),
             ("... in 8 x 8 tile order", lambda: ctx.ray_planes_device(d_tiled, t, planes8=d_frame_planes)),
             ("flx_rays_cast_device (closest)", lambda: ctx.cast_rays_device(d_rays, d_hits, capi.RAYS_CLOSEST)),
             ("flx_filter_planes_device", lambda: ctx.filter_planes_device(p, d_planes.data_ptr(), d_image.data_ptr())),
             ("flx_render_device, use_filter 1", lambda: ctx.render_device(p, d_frame.data_ptr())),
             ("flx_render_planes_device", lambda: ctx.render_planes_device(p, d_frame_planes.data_ptr()))]
    for depth in TEMPORAL:                          # (a history per depth and mode: none is re-keyed inside the timed region)
        for use_filter in (1, 0):
            temporal = capi.RayTemporal(history=(len(calls) - 7) % capi.RAY_HISTORIES, temporal_samples=depth, use_filter=use_filter, hdr=p.hdr)
            calls.append(("temporal N = %d, %s" % (depth, "chain" if use_filter else "no chain"),
                          lambda temporal=temporal: ctx.rays_image_temporal(d_rays, W, H, t, temporal, device=True, out=d_image)))
    ms = {label: [] for label, _ in calls}
    for k in range(WARMUP + REPEATS):
        for label, call in calls:
            ctx.sync()
            t0 = time.perf_counter()
            call()
            ctx.sync()
            if k >= WARMUP:
                ms[label].append((time.perf_counter() - t0) * 1e3)
    med = {label: float(np.median(v)) for label, v in ms.items()}
    lines += ["", "%s, %d spp, %d bounces (frame kernel: %s; planes kernel: %d workgroups of 256 lanes, lockstep %d, %d slab(s))" % (
        name, spp, bounces, ctx.last_trace_kernel(), last["groups"], last["lockstep"], last["slabs"])]
    for label, _ in calls:
        lines.append("  %-34s %8.3f ms [%8.3f .. %8.3f]" % (label, med[label], min(ms[label]), max(ms[label])))
    first, planes = med["flx_rays_cast_device (closest)"], med["flx_rays_planes_device (RGBA8)"]
    lines += ["  split of the ray image: first hits %.3f ms, planes kernel %.3f ms (the planes call less the first hits), chain %.3f ms" % (
                  first, planes - first, med["flx_filter_planes_device"]),
              "  ray image / filtered frame: %.3f;  planes kernel / the frame's trace: %.3f;  planes call / the frame's trace: %.3f" % (
                  med["flx_rays_image_device"] / med["flx_render_device, use_filter 1"], (planes - first) / med["flx_render_planes_device"], planes / med["flx_render_planes_device"]),
            ] + ["  %s - flx_rays_image_device: %+.3f ms" % (label, med[label] - med["flx_rays_image_device"]) for label, _ in calls if label.startswith("temporal")] + [
              "  verified once outside the timed region: the planes equal the frame's on %.4f %% of the pixels, the image the filtered frame bit for bit on %.4f %%" % (
                  100.0 * same_planes.mean(), 100.0 * same.mean())]
if out_path:
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
print("\n".join(lines), flush=True)
ctx.close()
