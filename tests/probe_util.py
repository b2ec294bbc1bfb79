"""Helpers of the light-probe tests (test_probes_cpu.py, test_probes_gpu.py, test_probe_seams_gpu.py, test_probes_js_gpu.py): the CPU reference built once per
session, synthetic radiance rows, poisoned device outputs, and a float64 restatement of include/flx_probe.h's quadrature."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "probe_ref"))
import flx_probe_ref  # noqa: E402

POSITION = (0.0, -1.5, 2.25)            # a zero and a negative component
K = (0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396)
A = (np.pi, 2.0 * np.pi / 3.0, np.pi / 4.0)
SPARE = 8               # rows behind the last one of a poisoned output that must keep their poison
EPSILON = {1: 0.910, 2: 0.0396, 3: 0.0281, 4: 0.0153, 8: 0.00383, 16: 0.00096, 32: 0.00024}      # sum d_omega = 4 pi (1 + e_w), as the header prints it

_ref = []


def reference(tmp_path_factory):
    """the CPU reference, built once per session"""
    if not _ref:
        _ref.append(flx_probe_ref.build(str(tmp_path_factory.mktemp("probe_ref"))))
    return _ref[0]


def poisoned(rows, row_bytes):
    """a device output of that many rows and SPARE rows behind them, every byte 0xA5"""
    import torch
    return torch.full(((rows + SPARE) * row_bytes,), 0xA5, dtype=torch.uint8, device="cuda")


def finished(ctx, out, rows, row_words):
    """a poisoned output after the call -> its uint32 [rows, row_words]: nothing past the last row was written"""
    ctx.sync()
    words = out.cpu().numpy().view(np.uint32)
    assert (words[rows * row_words:] == 0xA5A5A5A5).all()
    return words[:rows * row_words].reshape(rows, row_words)


def positions_of(n, seed=3):
    """n probe positions float32 [n, 4]: the first is POSITION, word 3 is junk that must be ignored"""
    rng = np.random.default_rng(seed)
    out = rng.uniform(-4.0, 4.0, size=(n, 4)).astype(np.float32)
    out[0, :3] = POSITION
    return out


def synthetic_radiance(n_probes, face_size, seed, all_miss=False):
    """radiance rows uint32 [n_probes * 6 w w, 8] with a fixed seed: about a third are miss rows (zeros, entry -1); colours and distances span 2^-20 .. 2^10"""
    rng = np.random.default_rng(seed)
    n = n_probes * 6 * face_size * face_size
    rows = np.zeros((n, 8), np.float32)
    rows[:, 0:3] = np.exp2(rng.uniform(-20.0, 10.0, size=(n, 3)))
    rows[:, 3] = 1.0
    rows[:, 4] = np.exp2(rng.uniform(-20.0, 10.0, size=n))
    words = rows.view(np.uint32)
    words[:, 5] = rng.integers(0, 1000, size=n)
    words[:, 6] = 2 * rng.integers(0, 3, size=n)
    words[:, 7] = rng.integers(1, 9, size=n)
    miss = np.ones(n, bool) if all_miss else rng.random(n) < 1.0 / 3.0
    words[miss] = 0
    words[miss, 5] = 0xffffffff
    return words


def cornell_probes(oracle, scenes):
    """-> (scene, trace params with 2 samples and 3 bounces, five positions float32 [5, 4] in the box's free space: 0.6 of the way from the camera to a first hit)"""
    from rays_trace_util import camera_rays, trace_params
    sc, p, rays, _, first = camera_rays(oracle, scenes, "cornell")
    hit = np.flatnonzero(first[:, 4] >= 0)
    pick = hit[np.linspace(0, len(hit) - 1, 5).astype(int)]
    positions = np.zeros((5, 4), np.float32)
    positions[:, :3] = rays[pick, 0:3] + 0.6 * first[pick, 0:1] * rays[pick, 4:7]
    t = trace_params(p)
    t.samples, t.max_reflections = 2, 3
    return sc, t, positions


def quadrature64(face_size):
    """the header's quadrature in float64 -> (directions [6 w w, 3], d_omega [6 w w], basis [6 w w, 9]) in texel order"""
    w = face_size
    px, row = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(w, dtype=np.float64))
    py = w - 1 - row
    sx, sy = ((px + 0.5) / w * 2.0 - 1.0).reshape(-1), ((py + 0.5) / w * 2.0 - 1.0).reshape(-1)
    one = np.ones_like(sx)
    local = [(one, sy, -sx), (-one, sy, sx), (sx, one, -sy), (sx, -one, sy), (sx, sy, one), (-sx, sy, -one)]      # flx_camera.h's faces 0 .. 5
    d = np.concatenate([np.stack(l, axis=-1) for l in local])
    d = d / np.sqrt((d * d).sum(axis=-1, keepdims=True))
    q = np.tile(1.0 + sx * sx + sy * sy, 6)
    dw = (4.0 / (w * w)) / (q * np.sqrt(q))
    return d, dw, basis64(d)


def basis64(d):
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([K[0] * np.ones_like(x), K[1] * y, K[1] * z, K[1] * x, K[2] * x * y, K[2] * y * z, K[3] * (3.0 * z * z - 1.0), K[2] * x * z, K[4] * (x * x - y * y)], axis=-1)


def sh64(face_size, radiance):
    """radiance float64 [6 w w, 3] of a probe whose every texel hits -> coefficients float64 [9, 3] by the same quadrature"""
    _, dw, b = quadrature64(face_size)
    return np.einsum("tc,ti,t->ic", radiance, b, dw)


def irradiance64(coefficients, normal):
    """coefficients float64 [9, 3] -> E float64 [3] for the normal"""
    b = basis64(np.asarray(normal, np.float64))
    p = coefficients * b[:, None]
    return A[0] * p[0] + A[1] * p[1:4].sum(axis=0) + A[2] * p[4:9].sum(axis=0)


def hit_rows(radiance, distance=1.0):
    """colours float [n, 3] -> radiance rows uint32 [n, 8] that all hit at that distance"""
    rows = np.zeros((len(radiance), 8), np.float32)
    rows[:, 0:3] = radiance
    rows[:, 3] = 1.0
    rows[:, 4] = distance
    return rows.view(np.uint32)


def assert_same_words(got, want, what=""):
    """float32 or uint32 [n, k] against the same, bit for bit"""
    got, want = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert got.shape == want.shape, "%s: %s against %s" % (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "%s: %d of %d rows differ, first %d: got %s want %s" % (
        what, bad.size, len(got), bad[0], ["%08x" % x for x in got[bad[0]]], ["%08x" % x for x in want[bad[0]]])
