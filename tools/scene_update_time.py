#!/usr/bin/env python3
"""What a vertex update costs: flx_scene_upload of the whole re-flattened scene (host validation, build_threaded with its sort, build_lockstep, five synchronous
copies) against flx_scene_update of the rows that moved (the monkey's; all rows), on the 174 276-triangle dragon scene (tests/golden/ref_dragon_100k.flxs.gz).
Per call: the host's wall clock inside the call, the wall clock until the device has finished (call + flx_sync), and the GPU time between two events recorded
on the context's stream around the call.  Warm-up, then REPEATS calls of each kind in turn (alternating, so that a drift of the machine hits all alike); median
and spread.  The yardsticks are measured in the same run: the full upload, and one 1080p frame of the scene.  GPU box.
--device-rows: flx_scene_update_device beside them, the rows in torch tensors on the device (made before the clock starts: that is where such an application
has them); the host-row kinds are measured again in the same run, and the lines are APPENDED to the file.  (The events stand on the context's stream: the check
kernel, which runs on a stream of its own and is waited for inside the call, shows in the host's columns.)
--device-upload: flx_scene_upload_device of the whole scene, its three arrays in torch tensors on the device (made before the clock starts), beside the host's
flx_scene_upload of the same scenes in the same run, alternating; only these two kinds, and the lines are APPENDED to the file.  (Its check runs on a stream of
its own like flx_scene_update_device's, and the call ends with a wait for the context's stream: the host's columns are the ones to read.)

usage: scene_update_time.py [--out profiles/scene_update.txt] [--repeats 25] [--device-rows | --device-upload]"""
import ctypes as C
import os
import sys
import time

import numpy as np

DEVICE_ROWS = "--device-rows" in sys.argv
DEVICE_UPLOAD = "--device-upload" in sys.argv
if DEVICE_ROWS or DEVICE_UPLOAD:
    import torch                               # (before the library: INTEGRATION.md, Build)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "web-ray-tracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from flexlight_hip import capi
from flexlight_hip.scene_io import Scene
from scene_update_util import reflatten_by_rule, with_geometry

out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "scene_update.txt")
REPEATS = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 25
WARMUP = 3

hip = C.CDLL("libamdhip64.so")
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]


def check(rc):
    if rc != 0:
        raise RuntimeError("HIP call failed: %d" % rc)


sc = Scene.golden("dragon_100k")
g0 = sc.arrays["geometry"].reshape(-1, 12)
n = g0.shape[0]
monkey = np.flatnonzero((g0[:, 10] != 0) & (g0[:, 9] == 2))          # the rows that stand in the monkey's transform
first, count = int(monkey[0]), int(monkey[-1] - monkey[0] + 1)
assert (g0[first:first + count, 9] == 2).all(), "the monkey's rows are one span"
rng = np.random.default_rng(1)


def moved(k):
    """the scene with the monkey's vertices moved (a different wobble per k), re-flattened on the host"""
    g = g0.copy()
    tri = np.zeros(n, bool)
    tri[first:first + count] = True
    tri &= g[:, 10] == 2
    g[tri, :9] += (0.01 * np.sin(k + np.arange(int(tri.sum()) * 9, dtype=np.float32))).reshape(-1, 9)
    return with_geometry(sc, reflatten_by_rule(g))


versions = [moved(k) for k in range(4)]
ctx = capi.Context(0)
stream, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
check(hip.hipStreamCreate(C.byref(stream)))
check(hip.hipEventCreate(C.byref(e0)))
check(hip.hipEventCreate(C.byref(e1)))
ctx.set_stream(stream.value)
ctx.update_scene(sc)
p = sc.frame_params(use_filter=0)


def timed(call):
    check(hip.hipEventRecord(e0, stream))
    t0 = time.perf_counter()
    call()
    t1 = time.perf_counter()
    check(hip.hipEventRecord(e1, stream))
    ctx.sync()
    t2 = time.perf_counter()
    check(hip.hipEventSynchronize(e1))
    ms = C.c_float()
    check(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
    return (t1 - t0) * 1e3, (t2 - t0) * 1e3, ms.value


def full(v):
    view = v.view()
    ctx._check(capi.LIB.flx_scene_upload(ctx._h, view.geometry, view.attributes, view.n_entries_padded, view.ids, view.n_ids), "flx_scene_upload")


def rows(v, lo, cnt, attributes=True):
    ctx.update_scene_rows(lo, v.arrays["geometry"].reshape(-1, 12)[lo:lo + cnt], v.arrays["attributes"].reshape(-1, 28)[lo:lo + cnt] if attributes else None)


kinds = [
    ("flx_scene_upload, the whole scene", lambda v: full(v)),
    ("flx_scene_update, the monkey's rows", lambda v: rows(v, first, count)),
    ("flx_scene_update, the monkey's rows, geometry only", lambda v: rows(v, first, count, False)),
    ("flx_scene_update, all rows", lambda v: rows(v, 0, n)),
]
if DEVICE_ROWS:
    on_device = [(torch.from_numpy(v.arrays["geometry"].reshape(-1, 12)).cuda(), torch.from_numpy(v.arrays["attributes"].reshape(-1, 28)).cuda()) for v in versions]

    def device_rows(v, lo, cnt, attributes=True):
        g, a = on_device[versions.index(v)]
        ctx.update_scene_rows_device(lo, g[lo:lo + cnt], a[lo:lo + cnt] if attributes else None)

    kinds += [
        ("flx_scene_update_device, the monkey's rows", lambda v: device_rows(v, first, count)),
        ("flx_scene_update_device, the monkey's rows, geometry only", lambda v: device_rows(v, first, count, False)),
        ("flx_scene_update_device, all rows", lambda v: device_rows(v, 0, n)),
        ("flx_scene_update_device, all rows, geometry only", lambda v: device_rows(v, 0, n, False)),
    ]
if DEVICE_UPLOAD:
    arrays_on_device = [(torch.from_numpy(v.arrays["geometry"].reshape(-1, 12)).cuda(), torch.from_numpy(v.arrays["attributes"].reshape(-1, 28)).cuda(),
                         torch.from_numpy(v.arrays["ids"]).cuda()) for v in versions]
    kinds = kinds[:1] + [("flx_scene_upload_device, the whole scene", lambda v: ctx.upload_scene_device(*arrays_on_device[versions.index(v)]))]
samples = {label: [] for label, _ in kinds}
for rep in range(WARMUP + REPEATS):
    v = versions[rep % len(versions)]
    for label, call in kinds:
        t = timed(lambda: call(v))
        if rep >= WARMUP:
            samples[label].append(t)
frame = []
for rep in range(WARMUP + 7):
    t0 = time.perf_counter()
    ctx.render(p)
    if rep >= WARMUP:
        frame.append((time.perf_counter() - t0) * 1e3)
gpu_frame = ctx.last_frame_ms()[0]

lines = ["%sscene updates on %s: %d entries (%d padded rows), the monkey's rows [%d, %d) = %d rows; %d calls of each kind after %d warm-up rounds, alternating"
         % ("\nrows in device memory (--device-rows), the host-row kinds measured again beside them\n" if DEVICE_ROWS else
            "\nthe whole scene from device memory (--device-upload), the host upload measured beside it\n" if DEVICE_UPLOAD else "", ctx.device_info()[0], sc.meta["textureLength"], n, first, first + count, count, REPEATS, WARMUP),
         "ms: median (min .. max)",
         "%-58s %-26s %-26s %-26s" % ("", "host, inside the call", "host, call + flx_sync", "GPU, events around the call")]
med = {}
for label, _ in kinds:
    a = np.array(samples[label])
    med[label] = np.median(a, axis=0)
    lines.append("%-58s " % label + " ".join("%-26s" % ("%.3f (%.3f .. %.3f)" % (np.median(a[:, k]), a[:, k].min(), a[:, k].max())) for k in range(3)))
lines.append("one 1920x1080 frame of the scene (flx_render, host wall clock incl. the copy out): median %.3f ms; GPU time of the last one %.3f ms" % (np.median(frame), gpu_frame))
if DEVICE_UPLOAD:
    host_ms, device_ms = med[kinds[0][0]][1], med[kinds[1][0]][1]
    lines.append("the whole scene from device memory takes %.3f ms against %.3f ms from host memory (call + sync): %.2f x; the frame's GPU time is %.3f ms"
                 % (device_ms, host_ms, host_ms / device_ms, gpu_frame))
else:
    up, mk, al = med[kinds[0][0]][1], med[kinds[1][0]][1], med[kinds[3][0]][1]
    lines.append("the monkey's rows take %.1f %% of the full upload's time (call + sync), all rows %.1f %%; the frame's GPU time is %.3f ms: the monkey update is %s it, the update of all rows %s it"
                 % (100 * mk / up, 100 * al / up, gpu_frame, "below" if mk < gpu_frame else "ABOVE", "below" if al < gpu_frame else "ABOVE"))
if DEVICE_ROWS:
    for what, host, dev in (("the monkey's rows", kinds[1][0], kinds[4][0]), ("all rows", kinds[3][0], kinds[6][0])):
        lines.append("%s from device memory take %.3f ms against %.3f ms from host memory (call + sync): %.2f x"
                     % (what, med[dev][1], med[host][1], med[host][1] / med[dev][1]))
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "a" if DEVICE_ROWS or DEVICE_UPLOAD else "w") as fh:
    fh.write(text)
ctx.close()
