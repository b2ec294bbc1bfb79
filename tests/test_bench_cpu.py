"""bench.py --dump-outputs without a GPU: the frame as it is, every written value finite with the frame's NaN / inf listed beside it, and a frame
over the size limit as the same seeded sample of its pixels every time."""
import os

import numpy as np

import bench


def _frame(h, w, seed, nonfinite=0):
    f = np.random.default_rng(seed).standard_normal((h, w, 4)).astype(np.float32)
    if nonfinite:
        at = np.random.default_rng(seed + 100).choice(f.size, nonfinite, replace=False)
        f.reshape(-1)[at] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(nonfinite) % 3]
    return f


def _same(a, b):
    """equal bit for bit where finite, the same non-finite values in the same places"""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _total(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_a_frame_within_the_limit_is_written_whole(tmp_path):
    f = _frame(27, 48, 1)
    assert bench.dump_outputs(str(tmp_path), f) == ["frame", "frame_nonfinite"]
    got = np.load(str(tmp_path / "frame.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, f)
    nf = np.load(str(tmp_path / "frame_nonfinite.npy"))
    assert nf.dtype == np.float64 and nf.shape == (0, 2)
    assert sorted(os.listdir(str(tmp_path))) == ["frame.npy", "frame_nonfinite.npy"]


def test_the_frames_nan_and_infinities_are_listed_and_every_written_value_is_finite(tmp_path):
    f = _frame(27, 48, 4, nonfinite=30)
    bench.dump_outputs(str(tmp_path), f)
    got, nf = np.load(str(tmp_path / "frame.npy")), np.load(str(tmp_path / "frame_nonfinite.npy"))
    assert np.isfinite(got).all() and np.isfinite(nf).all()
    assert nf.shape == (30, 2) and set(nf[:, 1]) == {1.0, 2.0, 3.0}
    bad = ~np.isfinite(f)
    assert np.array_equal(got[~bad], f[~bad]) and (got[bad] == 0).all()
    assert _same(bench.join_nonfinite(got, nf), f)


def test_a_larger_frame_is_a_fixed_sample_of_its_pixels(tmp_path):
    h, w = 60, 80
    n = 1000
    limit = 24 * n + 3 * 128                          # 77 KB frame against a 24 KB limit: 1000 pixels at 16 + 8 bytes (+ the .npy headers)
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    np.save(str(tmp_path / "a" / "frame.npy"), np.zeros(3, np.float32))          # an earlier run's whole frame does not stay beside the sample
    fa, fb = _frame(h, w, 2), _frame(h, w, 3)
    assert bench.dump_outputs(str(tmp_path / "a"), fa, limit=limit, sample_pixels=n) == ["frame_sample", "frame_sample_nonfinite", "frame_sample_pixels"]
    bench.dump_outputs(str(tmp_path / "b"), fb, limit=limit, sample_pixels=n)
    assert sorted(os.listdir(str(tmp_path / "a"))) == ["frame_sample.npy", "frame_sample_nonfinite.npy", "frame_sample_pixels.npy"]
    assert _total(str(tmp_path / "a")) <= limit
    ia, ib = np.load(str(tmp_path / "a" / "frame_sample_pixels.npy")), np.load(str(tmp_path / "b" / "frame_sample_pixels.npy"))
    assert ia.dtype == np.float64 and ia.shape == (n,) and np.array_equal(ia, ib)
    assert np.all(np.diff(ia) > 0) and ia[0] >= 0 and ia[-1] < h * w
    sa = np.load(str(tmp_path / "a" / "frame_sample.npy"))
    assert sa.dtype == np.float32 and sa.shape == (n, 4)
    assert np.array_equal(sa, fa.reshape(-1, 4)[ia.astype(np.int64)])


def test_a_sample_keeps_its_nan_and_infinities_and_stays_within_the_limit(tmp_path):
    h, w = 60, 80
    n = 1000
    limit = 24 * n + 3 * 128
    f = _frame(h, w, 5, nonfinite=h * w * 4 // 2)      # half of all values non-finite: the sample's list would not fit, the sample halves
    bench.dump_outputs(str(tmp_path), f, limit=limit, sample_pixels=n)
    d = str(tmp_path)
    assert _total(d) <= limit
    s, nf, px = (np.load(os.path.join(d, x + ".npy")) for x in ("frame_sample", "frame_sample_nonfinite", "frame_sample_pixels"))
    assert np.isfinite(s).all() and np.isfinite(nf).all() and 0 < len(px) < n and len(nf) > 0
    assert _same(bench.join_nonfinite(s, nf), f.reshape(-1, 4)[px.astype(np.int64)])
