#!/usr/bin/env python3
"""Temporal frames: what the temporal pass costs, and what a rank of a group pays for a temporal frame (profiles/temporal_group.txt).  GPU box.

  passes  SCENE [--frames N]  1080p temporal frames, N = 4, of cornell_obj (with the filter) or dragon (without it), BASELINE spp / bounces, rendered
                             into device memory; run it under `rocprofv3 --kernel-trace --stats -d DIR -o run -- python3 tools/temporal_group_time.py passes dragon`
                             once with this library and once with another (FLX_LIB=...) to compare their kernels.
  report  NEW OLD [--frames N]  the temporal pass of both runs from their kernel_stats.csv or rocpd database: the fused kernel (k_temporal_frame)
                             against the launches it replaced (k_quantize, k_temporal and the ring copies' blit kernels), per frame.
  group   [--ranks 8]        a group of 8 contexts on device 0 at 1080p (dragon): a rank's share of a temporal frame against its share of the same
                             frame without temporal accumulation (flx_render of the rank's strips, GPU time), and flx_group_frame_begin's host time
                             for temporal float frames (the lanes path: nothing waits for a GPU)."""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "web-ray-tracer_amd"))

SCENES = {"cornell_obj": 1, "dragon": 0}      # scene -> use_filter


def passes(name, frames):
    import torch                                  # (before the library: torch's HIP runtime first)
    from flexlight_hip import capi
    from flexlight_hip.scene_io import Scene
    out = torch.empty((1080, 1920, 4), dtype=torch.float32, device="cuda")
    sc = Scene.golden(name)
    with capi.Context(0) as ctx:
        ctx.update_scene(sc)
        p = sc.frame_params(width=1920, height=1080, use_filter=SCENES[name])
        p.is_temporal, p.temporal_samples = 1, 4
        ms = []
        for f in range(frames):
            p.random_seed = float(f % 4)
            ctx.render_device(p, out.data_ptr())
            ctx.sync()
            ms.append(ctx.last_frame_ms()[0])
        print("%-12s filter %d: %d temporal frames, frame %.3f ms (median)" % (name, SCENES[name], frames, statistics.median(ms)), flush=True)


def kernel_stats(path):
    """kernel name -> (calls, total ns) of a rocprofv3 run: its kernel_stats.csv (--output-format csv --stats) or its rocpd database (*.db)"""
    rows = {}
    if path.endswith(".db"):
        import sqlite3
        with sqlite3.connect(path) as db:
            for name, calls, ns in db.execute("select name, count(*), sum(duration) from kernels group by name"):
                rows[name] = (int(calls), float(ns))
        return rows
    with open(path) as fh:
        for r in csv.DictReader(fh):
            rows[r["Name"]] = (int(r["Calls"]), float(r["TotalDurationNs"]))
    return rows


def short_name(name):
    return name.split("(")[0].split("<")[0].replace("void ", "").replace("flx::", "").strip()


def report(new_path, old_path, frames):
    """the temporal pass per frame: the fused kernel against k_temporal + k_quantize + the ring copies (the blit copies the other run does not have)"""
    runs = {}
    for label, path in (("this commit", new_path), ("parent", old_path)):
        runs[label] = {}
        for name, (c, ns) in kernel_stats(path).items():
            k = short_name(name)
            c0, ns0 = runs[label].get(k, (0, 0.0))
            runs[label][k] = (c0 + c, ns0 + ns)
    copies = {label: r.get("__amd_rocclr_copyBuffer", (0, 0.0)) for label, r in runs.items()}
    for label, r in runs.items():
        other = copies["parent" if label == "this commit" else "this commit"]
        extra_calls, extra_ns = max(0, copies[label][0] - other[0]), max(0.0, copies[label][1] - other[1])
        calls, ns = extra_calls, extra_ns
        print("%s (%d frames):" % (label, frames))
        for k in ("k_temporal_frame", "k_temporal", "k_quantize"):
            if k in r:
                c, t = r[k]
                calls += c; ns += t
                print("   %-20s %4d launches  %7.2f us each  %7.2f us per frame" % (k, c, t / 1e3 / c, t / 1e3 / frames))
        if extra_calls:
            print("   %-20s %4d launches  %7.2f us each  %7.2f us per frame  (the ring copies: blit kernels beyond the other run's)" % ("copyBuffer", extra_calls, extra_ns / 1e3 / extra_calls, extra_ns / 1e3 / frames))
        print("   temporal pass: %.1f launches, %.2f us per frame" % (calls / frames, ns / 1e3 / frames))


def group(ranks, frames):
    from flexlight_hip import capi
    from flexlight_hip.scene_io import Scene
    sc = Scene.golden("dragon")
    p = sc.frame_params(width=1920, height=1080, use_filter=0)
    with capi.Context(0) as ctx:
        ctx.update_scene(sc)
        for temporal in (0, 1):
            q = type(p).from_buffer_copy(p)
            q.is_temporal, q.temporal_samples = temporal, 4
            q.tile_rows, q.tile_index, q.tile_count = 8, 0, ranks
            ms, km = [], []
            for f in range(frames + 3):
                q.random_seed = float(f % 4) if temporal else 0.0
                ctx.render(q)
                if f >= 3:
                    a, b = ctx.last_frame_ms()
                    ms.append(a); km.append(b)
            print("rank 0 of %d, dragon 1080p (%d rows), temporal %d: frame %.3f ms, trace kernel %.3f ms (median of %d)"
                  % (ranks, capi.Context.tile_row_count(q), temporal, statistics.median(ms), statistics.median(km), frames), flush=True)
    with capi.Group([0] * ranks) as g:
        g.update_scene(sc)
        q = type(p).from_buffer_copy(p)
        q.is_temporal, q.temporal_samples = 1, 4
        host = []
        for f in range(frames + 3):
            q.random_seed = float(f % 4)
            if g.frames_in_flight() == 3:
                g.frame_end()
            t0 = time.perf_counter()
            g.frame_begin(q, tile_rows=8)
            if f >= 3:
                host.append((time.perf_counter() - t0) * 1e3)
        while g.frames_in_flight():
            g.frame_end()
        print("group of %d on device 0, dragon 1080p temporal float frames: flx_group_frame_begin %.3f ms host time (median of %d, max %.3f)"
              % (ranks, statistics.median(host), len(host), max(host)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("passes"); a.add_argument("scene", choices=sorted(SCENES)); a.add_argument("--frames", type=int, default=20)
    b = sub.add_parser("report"); b.add_argument("new"); b.add_argument("old"); b.add_argument("--frames", type=int, default=20)
    c = sub.add_parser("group"); c.add_argument("--ranks", type=int, default=8); c.add_argument("--frames", type=int, default=20)
    args = ap.parse_args()
    if args.cmd == "passes":
        passes(args.scene, args.frames)
    elif args.cmd == "report":
        report(args.new, args.old, args.frames)
    else:
        group(args.ranks, args.frames)


if __name__ == "__main__":
    main()
