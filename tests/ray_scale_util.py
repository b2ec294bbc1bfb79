"""Helpers of the ray-batch scale tests (test_ray_batches_scale_gpu.py): a batch of any size tiled from base rays whose reference rows exist.  Row i of the batch is
base ray (i * 977) mod m — 977 is prime and divides no base count used, so every base ray occurs and the 64 rays of a wave are 977 base rays apart —, and a row of
the result depends on its ray row and the scene alone, so the expected row i is the reference's row of that base ray.  Rays and expectations are gathered on the
device; rows that differ as bits come to the host, where the call's own comparison (its same_rows: the NaNs it lets pass) decides."""
import math
import time

import numpy as np
import torch

STEP = 977
SPARE = 8          # rows behind the last that must keep their poison
POISON = 0xA5


def index_map(n, m):
    """int64 [n] on the device: the base ray of every row"""
    assert math.gcd(STEP, m) == 1
    return (torch.arange(n, dtype=torch.int64, device="cuda") * STEP) % m


def base_of(row, m):
    return row * STEP % m


def as_words(a):
    """a numpy array of 32-bit elements -> an int32 tensor of the same shape on the device (bits kept)"""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4
    return torch.from_numpy(a.view(np.int32).copy()).cuda()


def tiled_rays(base_rays, idx):
    """float32 [n, 8] on the device: the base rays gathered by the index map (as words: no float is looked at)"""
    return as_words(base_rays)[idx].view(torch.float32).contiguous()


def rays_unchanged(d_rays, base_rays, idx):
    return torch.equal(d_rays.view(torch.int32), as_words(base_rays)[idx])


def poisoned(rows, row_bytes):
    """uint8 on the device, all 0xA5: `rows` rows and SPARE more"""
    return torch.full(((rows + SPARE) * row_bytes,), POISON, dtype=torch.uint8, device="cuda")


def rows_of(out, rows, row_bytes):
    """-> int32 [rows, row_bytes / 4] of a poisoned output whose spare rows kept their poison"""
    flat = out.view(-1)
    assert flat.dtype == torch.uint8 and flat.numel() == (rows + SPARE) * row_bytes
    assert bool((flat[rows * row_bytes:] == POISON).all()), "the spare rows behind row %d were written" % (rows - 1)
    return flat[:rows * row_bytes].view(torch.int32).view(rows, row_bytes // 4)


def exactly(got, want):
    """the comparison of a call whose rows allow no NaN to pass: every word"""
    return (got == want).all(axis=1)


def assert_tiled(got, want_base, idx, same, what):
    """got: int32 [n, w] on the device; want_base: the reference's rows of the base rays, 32-bit [m, w] numpy; same(got, want) -> bool per row over uint32 [k, w]
    numpy arrays: the existing comparison of the call.  Compared as bits on the device; only rows that differ there go through the host."""
    want_base = np.ascontiguousarray(want_base).view(np.uint32)
    n, m = got.shape[0], want_base.shape[0]
    assert got.shape == (n, want_base.shape[1]) and idx.shape == (n,), (what, tuple(got.shape), want_base.shape)
    want = as_words(want_base)[idx]
    differ = torch.nonzero((got != want).any(dim=1)).flatten()
    del want
    if differ.numel() == 0:
        return
    rows = differ.cpu().numpy()
    g = got[differ].cpu().numpy().view(np.uint32)
    w = want_base[rows * STEP % m]
    bad = np.flatnonzero(~same(g.copy(), w.copy()))
    hexed = lambda r: " ".join("%08x" % x for x in r)
    assert bad.size == 0, "%s: %d of %d rows differ, first row %d (base ray %d): got %s want %s" % (
        what, bad.size, n, rows[bad[0]], base_of(int(rows[bad[0]]), m), hexed(g[bad[0]]), hexed(w[bad[0]]))


class timed:
    """with timed(hip, "what"): the wall time of the calls inside, the context's stream drained, printed"""

    def __init__(self, hip, what):
        self.hip, self.what = hip, what

    def __enter__(self):
        torch.cuda.synchronize()
        self.began = time.perf_counter()

    def __exit__(self, kind, value, trace):
        if kind is None:
            self.hip.sync()
            print("%s: %.1f ms" % (self.what, 1e3 * (time.perf_counter() - self.began)))
