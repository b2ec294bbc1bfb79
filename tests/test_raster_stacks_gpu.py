"""k_raster on the hand-made layer stacks of tests/raster_stacks_util.py: frame and work counters equal the CPU reference (tests/raster_ref) bit for bit
on every case — every O / T pattern of up to four fragments with and without failing layers between, a tile of seven patterns, the wave going alone
inside a box with fragments pending, alpha at the opaque boundary, depth ties, the near plane, shadowed and lit fragments, saturating blends — in pure
lockstep (8 x 8), alone (3 x 3) and with two different tiles (16 x 8).  tests/test_raster_stacks_cpu.py shows that the cases reach what they claim and
that the reference equals the literal draw on them."""
import os
import sys

import numpy as np
import pytest

import raster_stacks_util as u
from frame_loop_util import run_loop

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "raster_ref"))
import flx_raster_ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(oracle, tmp_path_factory):
    return flx_raster_ref.build(str(tmp_path_factory.mktemp("raster_ref")))


@pytest.mark.parametrize("cid", [c.id for c in u.CASES])
def test_stack_matches_reference(hip, ref, cid):
    sc, p = u.case_scene(u.CASE[cid])
    hip.update_scene(sc)
    u.assert_same(hip, ref, sc, p, cid)


@pytest.mark.parametrize("cid", ["pattern-TTOT-8x8", "failing-OTTO-16x8", "mixed-8x8", "switch-BO-3", "switch-BT-3", "alpha-2^-23-8x8", "alpha-texel1-near-3x3",
                                 "near-half-9x9", "shadow-mixed-8x8"])
def test_stack_through_the_device_output_and_the_frame_loop(hip, ref, cid):
    """the frame into device memory, and the frame loop's RGBA8 frames (k_raster<false, uint32_t>): the reference frame and flx_present of it"""
    torch = pytest.importorskip("torch")
    sc, p = u.case_scene(u.CASE[cid])
    hip.update_scene(sc)
    want, _ = ref.render(sc, p)
    buf = torch.zeros((p.height, p.width, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    hip.raster_render_device(p, buf.data_ptr())
    hip.sync()
    assert np.array_equal(u.bits(buf.cpu().numpy()), u.bits(want)), cid
    got, _, _ = run_loop(hip, [(p, dict(rasterizer=True, rgba8=True)), (p, dict(rasterizer=True)), (p, dict(rasterizer=True, rgba8=True))])
    assert got[0].dtype == np.uint8 and np.array_equal(got[0], hip.present(want)) and np.array_equal(got[2], got[0]), cid
    assert np.array_equal(u.bits(got[1]), u.bits(want)), cid
