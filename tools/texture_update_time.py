#!/usr/bin/env python3
"""What a texture costs on its way in (profiles/texture_update.txt).  Two workloads:
  1. one texture of a four-texture atlas of 1024 x 1024 cells replaced from a 1024 x 1024 RGBA8 source: flx_texture_update_device (the source in a torch tensor on
     the device, made before the clock starts), flx_texture_update (the source in host memory), and the only route before them: sceneFile.buildAtlas over the whole
     list under Node (tools/build_atlas_time.js) plus flx_atlas_upload of the whole atlas;
  2. the theater scene's albedo build, one 1600 x 2560 source into a 512 x 512 cell: flx_textures_upload_device, flx_textures_upload, and buildAtlas plus
     flx_atlas_upload.
Per call: the host's wall clock inside the call, the wall clock until the device has finished (call + flx_sync), and the GPU time between two events recorded on
the context's stream around the call (an update's resample runs on a stream of the context's own and is waited for inside the call: it shows in the host's columns).
Warm-up, then REPEATS calls of each kind in turn (alternating); median and spread.  The atlas read back is compared with the numpy atlas at the end.  GPU box.

usage: texture_update_time.py [--out profiles/texture_update.txt] [--repeats 25]"""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import torch                                   # (before the library: INTEGRATION.md, Build)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "web-ray-tracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from flexlight_hip import capi
import textures_util as tu

out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "texture_update.txt")
REPEATS = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 25
WARMUP = 3

hip = C.CDLL("libamdhip64.so")
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]


def check(rc):
    if rc != 0:
        raise RuntimeError("HIP call failed: %d" % rc)


ctx = capi.Context(0)
stream, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
check(hip.hipStreamCreate(C.byref(stream)))
check(hip.hipEventCreate(C.byref(e0)))
check(hip.hipEventCreate(C.byref(e1)))
ctx.set_stream(stream.value)


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


def atlas_upload(which, atlas):
    ctx._check(capi.LIB.flx_atlas_upload(ctx._h, which, atlas.ctypes.data_as(C.POINTER(C.c_uint8)), atlas.shape[1], atlas.shape[0]), "flx_atlas_upload")


def node_build(n, source, cell):
    out = subprocess.check_output([shutil.which("node"), os.path.join(ROOT, "tools", "build_atlas_time.js"), str(n), str(source[0]), str(source[1]), str(cell[0]), str(cell[1]), "9"])
    return np.array(json.loads(out.decode().splitlines()[-1])["ms"])


def measure(kinds, after=None):
    """after(label), if given, runs behind every call, outside the clock"""
    samples = {label: [] for label, _ in kinds}
    for rep in range(WARMUP + REPEATS):
        for label, call in kinds:
            t = timed(lambda: call(rep))
            if rep >= WARMUP:
                samples[label].append(t)
            if after:
                after(label)
    return {label: np.array(samples[label]) for label, _ in kinds}


def table(kinds, samples):
    rows = ["%-66s %-26s %-26s %-26s" % ("ms: median (min .. max)", "host, inside the call", "host, call + flx_sync", "GPU, events around the call")]
    for label, _ in kinds:
        a = samples[label]
        rows.append("%-66s " % label + " ".join("%-26s" % ("%.3f (%.3f .. %.3f)" % (np.median(a[:, k]), a[:, k].min(), a[:, k].max())) for k in range(3)))
    return rows


rng = np.random.default_rng(1)
lines = ["textures on %s; %d calls of each kind after %d warm-up rounds, alternating" % (ctx.device_info()[0], REPEATS, WARMUP), ""]

# 1. one texture of four replaced
cell = (1024, 1024)
images = [tu.random_image(rng, cell) for _ in range(4)]
spare = [tu.random_image(rng, cell) for _ in range(2)]
spare_dev = [torch.from_numpy(a).cuda() for a in spare]
atlases = [tu.build_atlas(images[:1] + [s] + images[2:], cell) for s in spare]       # what the old route uploads: the list with member 1 replaced, composited
ctx.upload_textures(0, images, cell)
kinds = [
    ("flx_texture_update_device, 1024^2 RGBA8 in device memory", lambda r: ctx.update_texture_device(0, 1, spare_dev[r % 2])),
    ("flx_texture_update, 1024^2 RGBA8 in host memory", lambda r: ctx.update_texture(0, 1, spare[r % 2])),
    ("flx_atlas_upload of the whole 2048 x 4096 atlas (32 MiB)", lambda r: atlas_upload(0, atlases[r % 2])),
]
# (a finished atlas has no known cells: the list is built again behind the old route's upload, outside the clock, so that the next update finds its cell)
samples = measure(kinds, after=lambda label: ctx.upload_textures(0, images, cell) if label.startswith("flx_atlas_upload") else None)
ctx.update_texture_device(0, 1, spare_dev[0])
assert np.array_equal(ctx.atlas_read(0), atlases[0]), "the updated atlas is not the composited one"
build = node_build(4, cell, cell)
lines += ["1. one texture of a four-texture atlas of 1024 x 1024 cells replaced from a 1024 x 1024 source (the atlas: 2048 x 4096)"] + table(kinds, samples)
old = np.median(build) + np.median(samples[kinds[2][0]][:, 1])
lines += ["sceneFile.buildAtlas over the four images under Node (host only): median %.1f ms (%.1f .. %.1f), 9 builds after 2" % (np.median(build), build.min(), build.max()),
          "the route before: buildAtlas + flx_atlas_upload = %.1f ms; flx_texture_update_device %.3f ms (%.0f x), flx_texture_update %.3f ms (%.0f x), call + sync"
          % (old, np.median(samples[kinds[0][0]][:, 1]), old / np.median(samples[kinds[0][0]][:, 1]), np.median(samples[kinds[1][0]][:, 1]), old / np.median(samples[kinds[1][0]][:, 1])), ""]

# 2. the theater's albedo build
cell, source = (512, 512), (1600, 2560)
image = tu.random_image(rng, source)
image_dev = torch.from_numpy(image).cuda()
atlas = tu.build_atlas([image], cell)
kinds = [
    ("flx_textures_upload_device, 1600 x 2560 RGBA8 in device memory", lambda r: ctx.upload_textures_device(0, [image_dev], cell)),
    ("flx_textures_upload, 1600 x 2560 RGBA8 in host memory (15.6 MiB)", lambda r: ctx.upload_textures(0, [image], cell)),
    ("flx_atlas_upload of the 2048 x 512 atlas (4 MiB)", lambda r: atlas_upload(0, atlas)),
]
samples = measure(kinds)
ctx.upload_textures_device(0, [image_dev], cell)
assert np.array_equal(ctx.atlas_read(0), atlas), "the built atlas is not the composited one"
build = node_build(1, source, cell)
lines += ["2. the theater scene's albedo atlas built: one 1600 x 2560 source into a 512 x 512 cell (the atlas: 2048 x 512)"] + table(kinds, samples)
old = np.median(build) + np.median(samples[kinds[2][0]][:, 1])
lines += ["sceneFile.buildAtlas of the one image under Node (host only): median %.1f ms (%.1f .. %.1f), 9 builds after 2" % (np.median(build), build.min(), build.max()),
          "the route before: buildAtlas + flx_atlas_upload = %.1f ms; flx_textures_upload_device %.3f ms, flx_textures_upload %.3f ms, call + sync"
          % (old, np.median(samples[kinds[0][0]][:, 1]), np.median(samples[kinds[1][0]][:, 1])), ""]
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write(text)
ctx.close()
