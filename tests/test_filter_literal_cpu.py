"""The denoise chain's vectorised literal (tests/filter_util.py) held to everything that can hold it without a GPU, and the oracle's chain held to the literal.

The literal is first compared with the committed table (tests/golden/filter_kat.json.gz) and with the per-texel transcription that wrote it
(tests/analysis/make_filter_kat.py's chain) on a generated adversarial case; then the tap offsets of all three filters are tabulated for every byte they depend on,
once with the literal's correctly rounded tanh and once with include/flx_math.h's, together with the byte rules csrc/flx_filter.hip decides by; then
flx_oracle_filter is compared with the literal on every plane set tests/test_filter_tiles_gpu.py runs on the device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import filter_util as fu
from test_oracle_kat import _filter_kat_cases, assert_filter_kat, filter_kat_inputs

f32 = np.float32


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def oracle_filter(oracle, planes, hdr):
    """flx_oracle_filter over the float planes whose RGBA8 store is `planes`"""
    from flexlight_hip.capi import FrameParams, GBuffers
    H, W = planes[0].shape[:2]
    p = FrameParams()
    p.width, p.height, p.samples, p.max_reflections, p.use_filter, p.hdr, p.texture_width = W, H, 1, 1, 1, hdr, 1
    fl = [np.ascontiguousarray(fu.fetch(pl)) for pl in planes]
    assert all(np.array_equal(fu.quantise(a), pl) for a, pl in zip(fl, planes))
    gb = GBuffers(fp(fl[0]), fp(fl[1]), fp(fl[2]), fp(fl[3]), fp(fl[4]), None)
    got = np.zeros((H, W, 4), f32)
    assert oracle.lib().flx_oracle_filter(C.byref(p), C.byref(gb), fp(got), 1) == 0
    return got


@pytest.mark.parametrize("k", range(5))
def test_literal_equals_the_committed_table(k):
    case = _filter_kat_cases()[k]
    W, H = case["width"], case["height"]
    _, _, want = filter_kat_inputs(case)
    got, masks = fu.filter_literal([np.array(pl, np.uint8).reshape(H, W, 4) for pl in case["planes"]], case["hdr"])
    assert [m["kind"] for m in masks] == ["first"] * 4 + ["second"] * 2 + ["final"]
    assert_filter_kat(got, want, case["hdr"], "literal, case %d" % k)


def test_literal_equals_the_per_texel_transcription():
    """one generated adversarial case of 24 x 16: make_filter_kat.py's chain, texel by texel, gives the same bits — with the tone mapping too, both pows being correctly rounded"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "analysis"))
    import make_filter_kat as mk
    W, H = 24, 16
    planes = fu.make_planes(W, H, 5)
    assert (planes[1][..., 3] != 0).sum() > 40 and (planes[0][..., 3] == 0).any() and len(np.unique(planes[4][..., 3])) >= 6
    want = np.array(mk.chain(W, H, 1, [mk.Tex(W, H, p) for p in planes]), f32)
    got, _ = fu.filter_literal(planes, 1)
    assert (want[..., 3] == 1).sum() > 300
    assert_filter_kat(got, want, 0, "literal against the per-texel chain")


def test_tap_offsets_for_every_byte_and_the_byte_rules(oracle):
    """Exhaustive tables: the 36 / 37 tap offsets of the second / final filter for all 256 x 256 (OColor.w, OId.w), the first filter's 37 for all 256 OColor.w.  With
    flx_math.h's tanh (flx_oracle_math, function 7) every offset is what the correctly rounded tanh gives, so no byte pair has to stay out of generated planes; the
    greatest reach is 8 texels for the second and the final filter (the kernels' 34 x 34 tile, FILTER_HALO = 9, keeps a texel to spare) and 42 for the first."""
    lib = oracle.lib()
    lib.flx_oracle_math.argtypes = [C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32]

    def flx_tanh(x):
        x = np.ascontiguousarray(x, f32)
        out = np.empty_like(x)
        lib.flx_oracle_math(7, fp(x), None, fp(out), x.size)
        return out

    k = np.arange(256, dtype=np.uint8)
    ocw, oidw = np.meshgrid(fu.fetch(k), fu.fetch(k), indexing="ij")
    for what, scale, stencil in (("second", fu.second_scale, fu.STENCIL3_36), ("final", fu.final_scale, fu.STENCIL3_37)):
        lit = fu.scale_offsets(stencil, scale(ocw, oidw))
        flx = fu.scale_offsets(stencil, scale(ocw, oidw, tanh=flx_tanh))
        assert lit.shape == (len(stencil), 2, 256, 256)
        differ = np.argwhere((lit != flx).any(axis=(0, 1)))
        assert sorted(map(tuple, differ.tolist())) == sorted(fu.EXCLUDED_PAIRS), "%s filter: flx_tanh moves a tap at (OColor.w, OId.w) = %s" % (what, differ[:8].tolist())
        assert np.abs(lit).max() == 8 and np.abs(lit[:, :, 0, 0]).max() == (3 if what == "second" else 2), what
    first = fu.first_offsets(fu.fetch(k))
    assert first.shape == (37, 2, 256)
    assert np.abs(first).max() == 42 and np.abs(first[:, :, 0]).max() == 10 and np.abs(first[:, :, 255]).max() == 42
    assert (np.diff(np.abs(first).max(axis=(0, 1))) >= 0).all()
    kk = f32(1.0) + fu.fetch(k)                           # (stencil * (k * k) * 3.5 lands on the same texel for every byte: the product's association is free)
    assert all(np.array_equal(((f32(s) * (kk * kk)) * f32(3.5)).astype(np.int32), ((f32(s) * kk) * kk * f32(3.5)).astype(np.int32)) for s in (1, 2, 3))
    # the byte rules flx_filter.hip decides by, in float32
    x = fu.fetch(k)
    assert x.dtype == f32
    assert np.array_equal(x > f32(0.1), k >= 26)
    assert np.array_equal(x >= f32(0.1), k >= 26)
    assert np.array_equal((x * f32(255.0)).astype(np.int32), k.astype(np.int32))
    assert np.array_equal(x != 0, k != 0) and len(np.unique(x)) == 256
    assert np.array_equal(fu.quantise(x), k)


def test_generated_planes_keep_clear_of_excluded_pairs():
    for W, H, seed, _ in fu.CASES:
        planes = fu.make_planes(W, H, seed)
        pairs = set(zip(planes[2][..., 3].ravel().tolist(), planes[4][..., 3].ravel().tolist()))
        assert not pairs & set(fu.EXCLUDED_PAIRS)
        assert all(p.shape == (H, W, 4) and p.dtype == np.uint8 for p in planes)
        again = fu.make_planes(W, H, seed)
        assert all(np.array_equal(a, b) for a, b in zip(planes, again))


def test_main_case_meets_every_coverage_condition():
    """the same conditions test_filter_tiles_gpu.py asserts before it looks at the device's frame, here where they can be read without one"""
    W, H, seed, hdr = fu.CASES[0]
    planes, out, masks = fu.literal_case(W, H, seed, hdr)
    cov = fu.coverage(planes, masks)
    missing = [k for k, v in cov.items() if v < 1]
    assert not missing, missing


@pytest.mark.parametrize("W,H,seed,hdr", fu.CASES)
def test_oracle_equals_the_literal(oracle, W, H, seed, hdr):
    planes, want, _ = fu.literal_case(W, H, seed, hdr)
    got = oracle_filter(oracle, planes, hdr)
    if W * H > 1:                                        # (assert_filter_kat's hdr bound wants a share of exact floats: the literal frame must have some)
        assert (want[..., 3] == 1).any()
    assert_filter_kat(got, want, hdr, "oracle, %d x %d hdr %d" % (W, H, hdr))
