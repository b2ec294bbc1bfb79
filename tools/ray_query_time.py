#!/usr/bin/env python3
"""What a ray query costs (flx_rays_cast_device, csrc/flx_query.hip) on the dragon scene of bench.py, about 2 M rays a set:
  (a) primary   the 1080p camera's primary rays in pixel order,
  (b) shuffled  the same rays in an order shuffled by a fixed seed,
  (c) bounce    origins on the hit points of (a), directions cosine-distributed about the direction back to the camera (bounce-like: no coherence of direction).
Per set and `what` = 1, 2, 3: GPU time between two events recorded on the context's stream around the call, after warm-up, the median of REPEATS with min and max,
and Mrays/s; from one counted run (what | 4) the mean entries a walk fetched.  Yardstick (i), the same rays in the same run: flx_debug_walk(0, ...) with its
copies and its allocation, on the host's clock (it waits for the device itself).
--trace [--set primary|shuffled|bounce]: no timing — flx_debug_walk(0, ...) and the query with what = 7 five times over one set, for a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/ray_query_time.py --trace`, whose kernel times (k_debug_walk<0> alone against k_ray_query) are yardstick (ii).
--trace-report FILE.csv [--set name]: the two kernels' rows of that run's kernel_stats.csv, appended to the file.  GPU box.

usage: ray_query_time.py [--out profiles/ray_query.txt] [--repeats 21] [--trace [--set name] | --trace-report kernel_stats.csv [--set name]]"""
import ctypes as C
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "ray_query.txt")
REPEATS = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 21
WARMUP = 3
W, H = 1920, 1080


def emit(lines, mode="a"):
    with open(out_path, mode) as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if "--trace-report" in sys.argv:
    rows = list(csv.DictReader(open(sys.argv[sys.argv.index("--trace-report") + 1])))
    keep = [r for r in rows if "k_debug_walk" in r["Name"] or "k_ray_query" in r["Name"]]
    assert len(keep) >= 2, [r["Name"] for r in rows]
    label = sys.argv[sys.argv.index("--set") + 1] if "--set" in sys.argv else "primary"
    lines = ["", "yardstick (ii): kernel times of a rocprofv3 --kernel-trace --stats run of its own (tools/ray_query_time.py --trace --set %s): set %s, what = 7" % (label, label),
             "%-60s %6s %12s %12s %12s" % ("kernel", "calls", "mean ms", "min ms", "max ms")]
    for r in keep:
        lines.append("%-60s %6s %12.3f %12.3f %12.3f" % (r["Name"][:60], r["Calls"], float(r["AverageNs"]) / 1e6, float(r["MinNs"]) / 1e6, float(r["MaxNs"]) / 1e6))
    emit(lines)
    sys.exit(0)

import torch                                   # (before the library: INTEGRATION.md, Build)

sys.path.insert(0, os.path.join(ROOT, "web-ray-tracer_amd"))
from flexlight_hip import capi
from flexlight_hip.scene_io import Scene

sc = Scene.golden("dragon")
p = sc.frame_params(width=W, height=H, use_filter=0)


def primary_rays():
    """the rays k_primary traces for the frame (flx_device.h: primary_dir_v), in pixel order, as ray rows [W * H, 8] with l = 25"""
    inv = np.linalg.inv(np.array(list(p.view_matrix), np.float64).reshape(3, 3))
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    nx, ny = (px + 0.5) / W * 2.0 - 1.0, (py + 0.5) / H * 2.0 - 1.0
    d = np.stack([inv[r, 0] * nx + inv[r, 1] * ny + inv[r, 2] for r in range(3)], axis=-1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rows = np.zeros((W * H, 8), np.float32)
    rows[:, 0:3], rows[:, 3], rows[:, 4:7] = list(p.camera), 25.0, d
    return rows


def bounce_rays(primary, hits, rng):
    """from the hit points of the primary rays (a miss keeps its ray), a cosine-distributed direction about the way back to the camera"""
    h = capi.unpack_hits(hits)
    hit = h["entry"] != -1
    rows = primary.copy()
    point = primary[:, 0:3] + h["suv"][:, 0:1] * primary[:, 4:7]
    normal = -primary[:, 4:7]
    a = np.where(np.abs(normal[:, 0:1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    t1 = np.cross(normal, a)
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(normal, t1)
    u1, u2 = rng.random(len(rows)), rng.random(len(rows))
    r, phi = np.sqrt(u1), 2.0 * np.pi * u2
    d = (r * np.cos(phi))[:, None] * t1 + (r * np.sin(phi))[:, None] * t2 + np.sqrt(1.0 - u1)[:, None] * normal
    rows[hit, 0:3] = (point + 1e-3 * normal)[hit]
    rows[hit, 4:7] = d[hit]
    rows[:, 3] = rng.uniform(0.5, 25.0, len(rows))
    return rows


ctx = capi.Context(0)
stream = torch.cuda.Stream()
ctx.set_stream(stream.cuda_stream)
ctx.update_scene(sc)
rng = np.random.default_rng(2024)
a = primary_rays()
sets = [("primary", a), ("shuffled", a[rng.permutation(len(a))]), ("bounce", bounce_rays(a, ctx.cast_rays(a, 1), rng))]


def seven(rows):
    """ray rows -> flx_debug_walk's rows (origin, direction, l)"""
    return np.ascontiguousarray(np.concatenate([rows[:, 0:3], rows[:, 4:7], rows[:, 3:4]], axis=1), np.float32)


if "--trace" in sys.argv:
    rows = dict(sets)[sys.argv[sys.argv.index("--set") + 1] if "--set" in sys.argv else "primary"]
    d_rays = torch.from_numpy(rows).cuda()
    d_hits = torch.empty((len(rows), 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for _ in range(5):
        ctx.debug_walk(0, seven(rows))
        ctx.cast_rays_device(d_rays, d_hits, 7)
        ctx.sync()
    ctx.close()
    sys.exit(0)

info = ctx.device_info()
lines = ["ray queries on the dragon scene (tests/golden/ref_dragon.flxs.gz), %d rays a set, %s, %d CUs; GPU ms between two events around flx_rays_cast_device:" % (len(a), info[0], info[1]),
         "median of %d after %d warm-up calls [min .. max]" % (REPEATS, WARMUP), ""]
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for name, rows in sets:
    d_rays = torch.from_numpy(rows).cuda()
    d_hits = torch.empty((len(rows), 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    counted = capi.unpack_hits(ctx.cast_rays(rows, 7))
    lines.append("set %-9s hit %.3f  occluded %.3f  mean entries per closest-hit walk %.1f (max %d), per shadow walk %.1f (max %d)" % (
        name, (counted["entry"] != -1).mean(), counted["occluded"].mean(), counted["visits_closest"].mean(), counted["visits_closest"].max(),
        counted["visits_shadow"].mean(), counted["visits_shadow"].max()))
    for what in (1, 2, 3):
        ms = []
        for k in range(WARMUP + REPEATS):
            e0.record(stream)
            ctx.cast_rays_device(d_rays, d_hits, what)
            e1.record(stream)
            e1.synchronize()
            if k >= WARMUP:
                ms.append(e0.elapsed_time(e1))
        med = float(np.median(ms))
        walks = len(rows) * (2 if what == 3 else 1)
        lines.append("  what %d   %8.3f ms [%8.3f .. %8.3f]   %8.1f Mrays/s   %8.1f Mwalks/s" % (what, med, min(ms), max(ms), len(rows) / med / 1e3, walks / med / 1e3))
    info_q = ctx.last_query()
    lines.append("  launch: %d workgroups, ldsCount %d, pre-transformed %d, %d waves had rays, %d rays to a wave at a time" % (info_q["groups"], info_q["lds_count"], info_q["pre"], info_q["waves"], info_q["chunk"]))
    r7 = seven(rows)
    wall = []
    for k in range(1 + 5):
        t0 = time.perf_counter()
        ctx.debug_walk(0, r7)
        if k >= 1:
            wall.append((time.perf_counter() - t0) * 1e3)
    lines.append("  yardstick (i) flx_debug_walk(0, ...), both walks counted, with its copies and allocation, host clock: %8.2f ms [%8.2f .. %8.2f] (median of 5)" % (float(np.median(wall)), min(wall), max(wall)))
    host = []
    for k in range(1 + 5):
        t0 = time.perf_counter()
        ctx.cast_rays(rows, 7)
        if k >= 1:
            host.append((time.perf_counter() - t0) * 1e3)
    lines.append("  the host call flx_rays_cast, what = 7, with its copies, host clock:                                            %8.2f ms [%8.2f .. %8.2f] (median of 5)" % (float(np.median(host)), min(host), max(host)))
    lines.append("")
emit(lines, "w")
ctx.close()
