#!/usr/bin/env python3
"""What surface rows cost (flx_frame_surface_device, flx_rays_surface_device: csrc/flx_surface.hip) on the dragon scene at 1920 x 1080:
  frames   all eight planes, HIT | NORMAL | ALBEDO, HIT alone;
  rays     the camera's rays in pixel order (origin = the camera, direction = primary_dir_v's bits) and the same rays shuffled by a fixed seed, all planes;
  copy     the yardstick: one hipMemcpyDtoDAsync of as many bytes as k_surface reads and writes in the all-planes call — ray rows, hit rows and planes — on the same stream.
GPU ms between two events recorded on the context's stream around each call, the calls in turn, round after round (REPEATS rounds after 3 warm-up rounds), reported
as median [min .. max].  Once, outside the timed region, the frame call's planes are held against the rays call's on the pixel-ordered rays (equal rows wherever
the two hit rules name the same entry).  GPU box.

--trace: the same calls five times each and nothing else, for a `rocprofv3 --kernel-trace --stats` run of its own; --report DIR reads that run's kernel trace (no GPU)
and prints the kernels' times per call, in the order the calls were made.

usage: surface_time.py [--out profiles/surface_rows.txt] [--repeats 15] | --trace | --report DIR"""
import csv
import ctypes as C
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
N = W * H
ALL, SOME, ONE = 255, 1 | 8 | 32, 1
CALLS = ["flx_frame_surface_device, all planes", "flx_frame_surface_device, HIT | NORMAL | ALBEDO", "flx_frame_surface_device, HIT",
         "flx_rays_surface_device, pixel order, all planes", "flx_rays_surface_device, shuffled, all planes"]
TRACE_EACH = 5


def report(directory):
    """the kernel trace of a --trace run: per call the median [min .. max] of its launches' kernels"""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    short = lambda r: r["Kernel_Name"].split("(")[0].replace("void ", "").replace("flx::", "")
    ours = [(short(r), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6) for r in rows if any(k in r["Kernel_Name"] for k in ("k_surface", "k_primary", "k_ray_query"))]
    ours = ours[-2 * TRACE_EACH * len(CALLS):]                     # two kernels a call; what ran before the timed calls (the check) is in front
    assert len(ours) == 2 * TRACE_EACH * len(CALLS), len(ours)
    for k, call in enumerate(CALLS):
        seg = ours[2 * TRACE_EACH * k: 2 * TRACE_EACH * (k + 1)]
        for name in sorted({n for n, _ in seg}, key=lambda n: "k_surface" in n):
            ms = sorted(t for n, t in seg if n == name)
            print("  %-52s %-26s %7.3f ms [%7.3f .. %7.3f] of %d" % (call, name, ms[len(ms) // 2], ms[0], ms[-1], len(ms)))


if "--report" in sys.argv:
    report(sys.argv[sys.argv.index("--report") + 1])
    sys.exit(0)

import torch                                   # (before the library: INTEGRATION.md, Build)

sys.path.insert(0, os.path.join(ROOT, "web-ray-tracer_amd"))
from flexlight_hip import capi
from flexlight_hip.scene_io import Scene

out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "surface_rows.txt")
REPEATS = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 15
WARMUP = 3
TRACE = "--trace" in sys.argv

sc = Scene.golden("dragon")
p = sc.frame_params(width=W, height=H, samples=1, max_reflections=1, use_filter=0)
TW = p.texture_width


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
    rows = np.zeros((N, 8), np.float32)
    rows[:, 0:3] = list(p.camera)
    rows[:, 4], rows[:, 5], rows[:, 6] = (dx / length).reshape(-1), (dy / length).reshape(-1), (dz / length).reshape(-1)
    return rows


def hip_runtime():
    """the HIP runtime this process has loaded already (torch's), by the path it was mapped from"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime is loaded")


ctx = capi.Context(0)
stream = torch.cuda.Stream()
ctx.set_stream(stream.cuda_stream)
ctx.update_scene(sc)
rng = np.random.default_rng(2024)
a = camera_rows()
d_a, d_b = torch.from_numpy(a).cuda(), torch.from_numpy(a[rng.permutation(N)]).cuda()
d_out = torch.empty((8, N, 4), dtype=torch.float32, device="cuda")
d_out2 = torch.empty((8, N, 4), dtype=torch.float32, device="cuda")
# the bytes k_surface reads and writes in the all-planes call: a frame's 16-byte hit row and eight 16-byte rows; a ray's 32-byte ray row and 32-byte hit row more
frame_bytes, rays_bytes = N * (16 + 8 * 16), N * (32 + 32 + 8 * 16)
d_src = torch.empty((rays_bytes,), dtype=torch.uint8, device="cuda")
d_dst = torch.empty((rays_bytes,), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()

# ---- once, outside the timed region: the frame call against the rays call on the same rays ----
ctx.frame_surface_device(p, ALL, d_out)
ctx.surface_rays_device(d_a, ALL, TW, d_out2)
ctx.sync()
f_words, r_words = d_out.cpu().numpy().view(np.uint32), d_out2.cpu().numpy().view(np.uint32)
agree = f_words[0, :, 3] == r_words[0, :, 3]
same = (f_words[:, agree] == r_words[:, agree]).all()
hit = (f_words[0, :, 3].view(np.int32) != -1).mean()
assert agree.mean() > 0.995 and same, (agree.mean(), same)

hip = hip_runtime()
hip.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
hip.hipMemcpyDtoDAsync.restype = C.c_int


def copy_call(nbytes):
    def call():
        rc = hip.hipMemcpyDtoDAsync(d_dst.data_ptr(), d_src.data_ptr(), nbytes, stream.cuda_stream)
        assert rc == 0, rc
    return call


calls = [(CALLS[0], lambda: ctx.frame_surface_device(p, ALL, d_out)), (CALLS[1], lambda: ctx.frame_surface_device(p, SOME, d_out)),
         (CALLS[2], lambda: ctx.frame_surface_device(p, ONE, d_out)), (CALLS[3], lambda: ctx.surface_rays_device(d_a, ALL, TW, d_out)),
         (CALLS[4], lambda: ctx.surface_rays_device(d_b, ALL, TW, d_out))]
if TRACE:
    for name, call in calls:
        for _ in range(TRACE_EACH):
            call()
        ctx.sync()
    ctx.close()
    print("trace run: %d calls, %d of each, in the order of CALLS" % (TRACE_EACH * len(calls), TRACE_EACH))
    sys.exit(0)

calls += [("hipMemcpyDtoDAsync, %d bytes (a frame's k_surface)" % frame_bytes, copy_call(frame_bytes)),
          ("hipMemcpyDtoDAsync, %d bytes (a batch's k_surface)" % rays_bytes, copy_call(rays_bytes))]
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
info, last = ctx.device_info(), ctx.last_surface()
lines = ["surface rows on the dragon scene (tests/golden/ref_dragon.flxs.gz): the %d x %d camera's %d pixels / rays; %s, %d CUs" % (W, H, N, info[0], info[1]),
         "GPU ms between two events around each call (first hits and k_surface together), the seven calls in turn, median of %d rounds after %d warm-up rounds [min .. max]" % (REPEATS, WARMUP), ""]
med = {name: float(np.median(v)) for name, v in ms.items()}
for name, _ in calls:
    lines.append("  %-58s %8.3f ms [%8.3f .. %8.3f]" % (name, med[name], min(ms[name]), max(ms[name])))
copy_f, copy_r = med[calls[5][0]], med[calls[6][0]]
lines += ["", "the yardstick copies move %.1f and %.1f GB/s (each byte read once and written once)" % (frame_bytes / copy_f / 1e6, rays_bytes / copy_r / 1e6),
          "whole call over its copy: frame, all planes %.2f; rays, pixel order %.2f; rays, shuffled %.2f   (the kernel alone: see the trace run below)" % (
              med[CALLS[0]] / copy_f, med[CALLS[3]] / copy_r, med[CALLS[4]] / copy_r),
          "the last batch: %d slab(s) of at most %d rays, %d workgroups of 1024 lanes in the first-hit kernel; hit %.4f of the pixels" % (last["slabs"], last["slab"], last["query_groups"], hit),
          "verified once outside the timed region: the frame call's rows equal the rays call's on the pixel-ordered rays, all eight planes bit for bit, on the %d of %d pixels where the two hit rules name the same entry (%.4f %%)" % (
              agree.sum(), agree.size, 100.0 * agree.mean())]
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("\n".join(lines), flush=True)
ctx.close()
