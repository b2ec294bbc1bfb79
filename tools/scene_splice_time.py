#!/usr/bin/env python3
"""What it costs to give ONE mesh of the resident scene another shape when its triangles are in device memory: (a) Context.replace_mesh_device —
flx_tree_build_device + flx_tree_emit_device + flx_scene_splice_device, the scene's arrays staying where the context holds them — against (b) what a caller does
without the splice: build_tree_device, then its OWN assembly of the whole arrays in torch from a copy of the scene it keeps in device memory (the rows in front of
the block, the block, the tail, the padding; the root's skip count and its six floats; the id list), then flx_scene_upload_device of everything.
The scene: a root box over four triangles, the mesh's block and one triangle behind it.  The mesh is replaced by the same mesh rebuilt, so the result is known: the
arrays the scene was uploaded with, bit for bit, which both paths are checked against.  Two meshes: tests/golden/assets/objects/dragon_lp.obj.gz (43 569 triangles)
and tools/make_dragon_100k.py's 174 276-triangle mesh.  Per path the median of REPEATS runs, call + sync, alternating after a warm-up.  The lines go to
profiles/scene_splice.txt.  GPU box.

usage: scene_splice_time.py [--out profiles/scene_splice.txt] [--repeats 25]"""
import gzip
import os
import sys
import tempfile
import time

import numpy as np
import torch                                   # (before the library: INTEGRATION.md, Build)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "web-ray-tracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from flexlight_hip import capi
from scene_update_util import reflatten_by_rule
from tree_build_util import bits, block_of_text, face_order_rows, soup_of_obj
import make_dragon_100k

out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "scene_splice.txt")
REPEATS = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 25
WARMUP = 3


def meshes():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "assets", "objects", "dragon_lp.obj.gz"), "rt") as f:
        low = f.read()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "objects"))
        with open(os.path.join(tmp, "objects", "dragon_lp.obj"), "w") as f:
            f.write(low)
        argv, sys.argv = sys.argv, [sys.argv[0], tmp, tmp]
        try:
            make_dragon_100k.main()
        finally:
            sys.argv = argv
        with open(os.path.join(tmp, "objects", "dragon_100k.obj")) as f:
            high = f.read()
    return [("dragon_lp", low), ("dragon_100k", high)]


def scene_around(block):
    """root box [ four triangles, the block, one triangle ] -> (geometry [padded, 12], attributes [padded, 28], ids, the block's first entry)"""
    g, a, ids = block
    at = np.flatnonzero(g[:, 10] == 2)
    lead, tail = at[:4], at[-1:]
    first = 1 + lead.size
    end = first + g.shape[0] + tail.size
    n = (end + 255) // 256 * 256
    og, oa = np.zeros((n, 12), np.float32), np.zeros((n, 28), np.float32)
    og[0, 6], og[0, 10] = end - 1, 1
    og[1:first], oa[1:first] = g[lead] + np.float32([0.5] * 9 + [0] * 3), a[lead]
    og[first:first + g.shape[0]], oa[first:first + g.shape[0]] = g, a
    og[end - 1], oa[end - 1] = g[tail[0]] - np.float32([0.5] * 9 + [0] * 3), a[tail[0]]
    all_ids = np.concatenate([np.arange(1, first), ids + first, [end - 1]]).astype(np.int32)
    return reflatten_by_rule(og), oa, all_ids, first


def main():
    ctx = capi.Context(0)
    lines = ["one mesh of the resident scene rebuilt from triangles in device memory on %s: %d runs of each path after %d warm-up rounds, alternating; ms, call + sync: median (min .. max)"
             % (ctx.device_info()[0], REPEATS, WARMUP),
             "(a) Context.replace_mesh_device: build_tree_device (its three torch.empty and its synchronise of torch's stream included) + flx_scene_splice_device; the caller keeps no copy of the scene",
             "(b) build_tree_device + the caller's torch assembly of the whole arrays from its own copy in device memory (cat of rows, block, tail and padding; the root's skip count and bounds; the ids) + flx_scene_upload_device"]
    for name, text in meshes():
        soup = soup_of_obj(text)
        block = block_of_text(text)
        rows = face_order_rows(block, soup)
        triangles, attributes = torch.from_numpy(rows[0]).cuda(), torch.from_numpy(rows[1]).cuda()
        hg, ha, hids, first = scene_around(block)
        n_old, padded = block[0].shape[0], hg.shape[0]
        end = first + n_old + 1
        dg, da, dids = torch.from_numpy(hg).cuda(), torch.from_numpy(ha).cuda(), torch.from_numpy(hids).cuda()      # the caller's copy, for (b)

        def splice():
            ctx.replace_mesh_device(first, n_old, 0, triangles, attributes)
            ctx.sync()

        def by_hand():
            g, a, ids = ctx.build_tree_device(triangles, attributes)
            delta = g.shape[0] - n_old
            pad = (end + delta + 255) // 256 * 256 - (end + delta)
            new_g = torch.cat([dg[:first], g, dg[first + n_old:end], torch.zeros((pad, 12), device="cuda")])
            new_a = torch.cat([da[:first], a, da[first + n_old:end], torch.zeros((pad, 28), device="cuda")])
            new_g[0, 6] += delta
            vertices = new_g[:end + delta][new_g[:end + delta, 10] == 2][:, :9].reshape(-1, 3)
            new_g[0, 0:3], new_g[0, 3:6] = vertices.amin(0), vertices.amax(0)
            keep = dids[dids < first], dids[dids >= first + n_old] + delta
            new_ids = torch.cat([keep[0], ids + first, keep[1]]).to(torch.int32)
            ctx.upload_scene_device(new_g, new_a, new_ids, stream=torch.cuda.current_stream())
            ctx.sync()

        def same():
            return ((bits(ctx.scene_read("geometry", padded)) == bits(hg)).all() and (bits(ctx.scene_read("attributes", padded)) == bits(ha)).all()
                    and (ctx.scene_read("ids", hids.size) == hids).all())

        ctx.upload_scene_device(dg, da, dids)
        splice()
        ok_a = same()
        by_hand()
        ok_b = same()
        samples = {"splice": [], "by hand": []}
        for rep in range(WARMUP + REPEATS):
            for label, call in (("splice", splice), ("by hand", by_hand)):
                t0 = time.perf_counter()
                call()
                if rep >= WARMUP:
                    samples[label].append((time.perf_counter() - t0) * 1e3)
        ok_end = same()
        s, h = np.array(samples["splice"]), np.array(samples["by hand"])
        lines.append("%s: %d triangles, a block of %d entries in a scene of %d (%d padded); the resident arrays and ids equal the uploaded ones bit for bit after (a): %s, after (b): %s, after the runs: %s"
                     % (name, soup.shape[0], n_old, end, padded, *("yes" if ok else "NO" for ok in (ok_a, ok_b, ok_end))))
        lines.append("  (a) replace_mesh_device                                             %.3f (%.3f .. %.3f)" % (np.median(s), s.min(), s.max()))
        lines.append("  (b) build_tree_device + torch assembly + flx_scene_upload_device    %.3f (%.3f .. %.3f)" % (np.median(h), h.min(), h.max()))
        lines.append("  (a)'s median lies %s (b)'s: %.2f x; %s" % ("below" if np.median(s) < np.median(h) else "ABOVE", np.median(s) / np.median(h),
                                                                 "(a)'s median lies ABOVE (b)'s max" if np.median(s) > h.max() else "(a)'s median does not lie above (b)'s max"))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
