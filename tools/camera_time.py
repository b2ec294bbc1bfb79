#!/usr/bin/env python3
"""What the rays of a camera cost when the device makes them (flx_camera_rays_device, csrc/flx_camera.hip: k_camera_rays), 1920 x 1080, per projection, and what a
camera image saves against a ray image whose rays come from the host, on cornell.obj 1080p 4 spp 3 bounces (bench.py's configs[1]).
Timed, each call followed by a wait for the context's stream, on the host's clock (what the caller of the call sees); the calls in turn, round after round, median of
REPEATS rounds after WARMUP [min .. max]:
  flx_camera_rays_device, <projection>    one camera's 2 073 600 rows, 66 MB written
  ... six cube faces, one call            a probe's faces in one launch
  hipMemcpyDtoDAsync, 66 MB               the yardstick: the same bytes read and written by the copy engine's kernel
  flx_camera_image_device                 the rays made on the device + flx_rays_image_device
  flx_rays_image_device                   the same image from rays that are on the device already
  flx_rays_image                          the same image from rays in host memory: 66 MB up, 33 MB down
  flx_camera_image                        the camera's image into host memory: 33 MB down
Once, outside the timed region, the camera image is held against the ray image of the generated rays bit for bit.  GPU box.

usage: camera_time.py [--out FILE] [--repeats 20] [--rays-only]      (its output is recorded in profiles/camera_rays.txt; --rays-only: the ray calls alone, for a
kernel trace)"""
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
RAYS_ONLY = "--rays-only" in sys.argv
WARMUP = 3
W, H = 1920, 1080

ctx = capi.Context(0)
info = ctx.device_info()
n = W * H
sc = Scene.golden("cornell_obj")
p = sc.frame_params(width=W, height=H, samples=4, max_reflections=3, use_filter=1)
t = capi.TraceParams.of_frame(p)
basis = (0.8, 0.0, -0.6, 0.0, 1.0, 0.0, 0.6, 0.0, 0.8)
position = tuple(p.camera)
cameras = [("pinhole", capi.Camera.pinhole(p)), ("panorama", capi.Camera.panorama(position, basis)), ("fisheye", capi.Camera.fisheye(position, basis, fov=np.deg2rad(180.0))),
           ("orthographic", capi.Camera.orthographic(position, basis, width=4.0, height=2.25)), ("cube face 4", capi.Camera.cube_face(position, 4, basis))]
faces = [capi.Camera.cube_face(position, f, basis) for f in range(6)]
d_rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
d_copy = torch.empty((n, 8), dtype=torch.float32, device="cuda")
d_faces = torch.empty((6 * 1024 * 1024, 8), dtype=torch.float32, device="cuda")
d_image = torch.empty((n, 4), dtype=torch.float32, device="cuda")
d_want = torch.empty((n, 4), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
lines = ["cameras on the device, %d x %d; %s, %d CUs" % (W, H, info[0], info[1]),
         "host ms of call + wait for the stream, the calls in turn, median of %d rounds after %d warm-up rounds [min .. max]" % (REPEATS, WARMUP)]
calls = [("flx_camera_rays_device, %s" % name, lambda cam=cam: ctx.camera_rays_device(cam, W, H, out=d_rays)) for name, cam in cameras]
calls.append(("... six cube faces 1024 x 1024, one call", lambda: ctx.camera_rays_device(faces, 1024, 1024, out=d_faces)))
calls.append(("hipMemcpyDtoDAsync, %d bytes" % (n * 32), lambda: d_copy.copy_(d_rays)))      # (on torch's stream; the wait below is for it)
if not RAYS_ONLY:
    ctx.update_scene(sc)
    panorama = cameras[1][1]
    # ---- once, outside the timed region: the camera image against the ray image of the generated rays ----
    ctx.camera_rays_device(panorama, W, H, out=d_rays)
    ctx.ray_image_device(d_rays, W, H, t, hdr=p.hdr, out=d_want)
    ctx.camera_image_device(panorama, W, H, t, hdr=p.hdr, out=d_image)
    ctx.sync()
    assert torch.equal(d_image.view(torch.int32), d_want.view(torch.int32))
    host_rays = d_rays.cpu().numpy()
    d_panorama = d_rays.clone()
    calls += [("flx_camera_image_device, panorama", lambda: ctx.camera_image_device(panorama, W, H, t, hdr=p.hdr, out=d_image)),
              ("flx_rays_image_device, its rays on the device", lambda: ctx.ray_image_device(d_panorama, W, H, t, hdr=p.hdr, out=d_want)),
              ("flx_rays_image, its rays in host memory", lambda: ctx.ray_image(host_rays, W, H, t, hdr=p.hdr)),
              ("flx_camera_image, panorama", lambda: ctx.camera_image(panorama, W, H, t, hdr=p.hdr))]
ms = {label: [] for label, _ in calls}
for k in range(WARMUP + REPEATS):
    for label, call in calls:
        ctx.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        ctx.sync()
        if label.startswith("hipMemcpy"):
            torch.cuda.synchronize()
        if k >= WARMUP:
            ms[label].append((time.perf_counter() - t0) * 1e3)
for label, _ in calls:
    lines.append("  %-48s %8.3f ms [%8.3f .. %8.3f]" % (label, float(np.median(ms[label])), min(ms[label]), max(ms[label])))
if not RAYS_ONLY:
    lines.append("  verified once outside the timed region: the camera image equals the ray image of the generated rays bit for bit")
if out_path:
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
print("\n".join(lines), flush=True)
ctx.close()
