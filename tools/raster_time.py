#!/usr/bin/env python3
"""Time the rasterizer renderer's frame (flx_raster_render, k_raster): warm-up frames, then the median of repeated frames by
flx_last_frame_ms (HIP events around the launch on the context's stream), output left in device memory.

    python tools/raster_time.py [--scenes cornell_obj,dragon,theater] [--width 1920 --height 1080] [--frames 50] [--warmup 10]

One JSON line per scene: GPU ms (median, min, max), the work counters of one counted frame and what they are per pixel."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "web-ray-tracer_amd"))

import torch  # noqa: E402,F401  (torch's HIP runtime first, as in tests/conftest.py)
from flexlight_hip import capi  # noqa: E402
from flexlight_hip.scene_io import Scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_obj,dragon,theater")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    with capi.Context(0) as ctx:
        buf = torch.zeros((a.height, a.width, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        for name in a.scenes.split(","):
            sc = Scene.golden(name)
            ctx.update_scene(sc)
            p = sc.frame_params(width=a.width, height=a.height)
            _, cnt = ctx.raster_render(p, counters=True)
            for _ in range(a.warmup):
                ctx.raster_render_device(p, buf.data_ptr())
            ms = []
            for _ in range(a.frames):
                ctx.raster_render_device(p, buf.data_ptr())
                ms.append(ctx.last_frame_ms()[0])
            px = a.width * a.height
            print(json.dumps({"scene": name, "width": a.width, "height": a.height, "frames": a.frames, "ms_median": round(statistics.median(ms), 4),
                              "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "counters": cnt,
                              "per_pixel": {k: round(v / px, 3) for k, v in cnt.items() if v}}), flush=True)


if __name__ == "__main__":
    main()
