"""The GPU's denoise chain across tile borders and at its byte thresholds: flx_filter_planes_device (k_filter_first / _second / _final) against the vectorised literal
of the shaders and the pass schedule (tests/filter_util.py) over generated adversarial planes — bit for bit without the tone mapping, within assert_filter_kat's 2 ulp
with it (pow) — and against the oracle's chain bit for bit at both (they share flx_pow).

What the planes ask of the kernels is asserted from the literal's masks (filter_util.coverage) BEFORE the device's frame is looked at: 34 x 34 LDS tiles whose taps
land in all eight neighbours and beyond all four borders, a tile of uncovered texels over non-zero data, first-filter taps 42 texels away, the bytes 25 and 26 where
`>= 26u` decides, every outcome of the vote.  tests/test_filter_literal_cpu.py holds the literal itself."""
import numpy as np
import pytest

import filter_util as fu
from test_filter_literal_cpu import oracle_filter
from test_oracle_kat import assert_filter_kat

pytestmark = pytest.mark.gpu


def device_chain(hip, planes, hdr):
    import torch
    from flexlight_hip.capi import FrameParams
    H, W = planes[0].shape[:2]
    p = FrameParams()
    p.width, p.height, p.samples, p.max_reflections, p.use_filter, p.hdr, p.texture_width = W, H, 1, 1, 1, hdr, 1
    d_planes = torch.as_tensor(fu.pack_planes(planes).view(np.int32), device="cuda").contiguous()
    out = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")         # (every texel is written: none of this may survive)
    torch.cuda.synchronize()
    hip.filter_planes_device(p, d_planes.data_ptr(), out.data_ptr())
    hip.sync()
    return out.cpu().numpy()


def where_differs(got, want):
    bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1))
    if not len(bad): return "equal"
    tiles = sorted({(int(c) // 16, int(r) // 16) for r, c in bad})
    return "%d texels differ, first (row, x) = %s, in tiles (tx, ty) %s" % (len(bad), bad[0].tolist(), tiles[:12])


def check(hip, oracle, W, H, seed, hdr):
    planes, want, _ = fu.literal_case(W, H, seed, hdr)
    got = device_chain(hip, planes, hdr)
    what = "GPU, %d x %d hdr %d" % (W, H, hdr)
    assert_filter_kat(got, want, hdr, "%s against the literal (%s)" % (what, where_differs(got, want)))
    ora = oracle_filter(oracle, planes, hdr)
    assert_filter_kat(got, ora, 0, "%s against the oracle (%s)" % (what, where_differs(got, ora)))
    return got


@pytest.mark.parametrize("hdr", [0, 1])
def test_main_case(hip, oracle, scenes, hdr):
    """93 x 87: 6 x 6 tiles with a ragged last column and row, 3 x 11 first-filter workgroups, every coverage condition at once"""
    W, H, seed, _ = fu.CASES[0]
    assert (W, H, seed, hdr) in fu.CASES
    planes, want, masks = fu.literal_case(W, H, seed, hdr)
    cov = fu.coverage(planes, masks)
    missing = [k for k, v in cov.items() if v < 1]
    assert not missing, missing
    assert len(cov) >= 55
    hip.update_scene(scenes("cornell"))                  # (the chain reads no scene; a context renders only with one)
    check(hip, oracle, W, H, seed, hdr)


@pytest.mark.parametrize("W,H,seed,hdr", fu.CASES[1:-1])
def test_small_and_ragged_shapes(hip, oracle, scenes, W, H, seed, hdr):
    """one texel, one row, one column, one texel short of / past a tile and a first-filter workgroup, four tiles in a row"""
    hip.update_scene(scenes("cornell"))
    check(hip, oracle, W, H, seed, hdr)


def test_stale_state_between_frames(hip, oracle, scenes):
    """The main case, a smaller case, the main case again on one context: the planes the chain ping-pongs between are the context's and keep what the frame
    before left — the second filter's O[1], read at pass 4 before this frame wrote it, and every plane a pass must fully rewrite, the all-uncovered tile's zeros
    included (the 64 x 16 frame's texels lie where rows 0 .. 10 of the main case's do, across its uncovered tile)."""
    hip.update_scene(scenes("cornell"))
    W, H, seed, hdr = fu.CASES[0]
    small = next(c for c in fu.CASES if c[:2] == (64, 16))
    tx, ty = fu.UNCOVERED_TILE
    assert ty == 0 and small[0] * small[1] > 8 * W + 16 * tx + 16
    first = check(hip, oracle, W, H, seed, hdr)
    check(hip, oracle, *small)
    third = check(hip, oracle, W, H, seed, hdr)
    assert np.array_equal(first.view(np.uint32), third.view(np.uint32))
