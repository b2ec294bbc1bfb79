"""The GPU's temporal pass (k_temporal_frame, the ring handling of run_post_frame) against the generated shader's text at every history depth and under
motion, with the tracing taken out of the comparison.

Every frame is rendered with gbuffers=True: flx_render copies back the six float G-buffers the trace wrote, the planes k_temporal_frame reads.  The test
pushes them into a ring of its own (temporal_util.TemporalRing) and requires the returned frame to equal temporal_util.temporal_literal — the shader
modules/pathtracerWGL2.js:571-662 generates, for any depth, written from the reference's text and not from the kernel or the oracle — under assert_filter_kat's rule:
bit for bit, within 2 ulp where the tone mapping's pow is in.  What the trace writes is held elsewhere (test_pixel_parity_gpu, test_parity_gpu).  Where the
oracle can render the run (flx_oracle_render_sequence / _frames), the frames equal its frames too, with no float differing.

The motion runs move the camera between two or three positions on a schedule without a period (temporal_util.SCHEDULE), so that history slots match some
pixels and not others, and assert from the literal's masks over the GPU's own G-buffers that they did (temporal_util.Coverage)."""
import ctypes as C

import numpy as np
import pytest

from frame_loop_util import run_loop
from parity_util import assert_parity
from temporal_util import (Coverage, TemporalRing, copy_params, effective_depth, far_frames, motion_frames, only_w_tells, quantise, still_frames, temporal_literal,
                           temporal_params)
from test_oracle_kat import assert_filter_kat

pytestmark = pytest.mark.gpu

W, H = 48, 32
DEPTHS = [1, 2, 3, 4, 5, 6, 8, 9, 13, 16, 0, 17, -1]
STILL = [("dragon", n, 0) for n in DEPTHS] + [("theater", 6, 0), ("theater", 16, 0), ("dragon", 6, 1)]
MOTION = [(name, n) for name in ("theater", "dragon") for n in (4, 6, 16)]


class Run:
    """frames of one context against the literal over a ring of the test's own"""

    def __init__(self, hip):
        self.hip, self.ring, self.gbuffers = hip, None, None
        hip.temporal_reset()

    def fresh(self):
        """the next temporal frame is expected to start from a zero history"""
        self.ring = None

    def frame(self, q, what, coverage=None):
        """render q; a temporal frame goes into the ring and equals the literal -> the frame"""
        if q.is_temporal != 1:
            return self.hip.render(q)[0]
        got, _, gb = self.hip.render(q, gbuffers=True)
        if self.ring is None:
            self.ring = TemporalRing(effective_depth(q.temporal_samples), got.shape[0], q.width)
        assert self.ring.depth == effective_depth(q.temporal_samples)
        self.ring.push(gb)
        self.gbuffers = gb
        want, masks = temporal_literal(self.ring, q.hdr, q.use_filter)
        if coverage is not None:
            coverage.add(self.ring, masks)
        if q.use_filter == 1:
            want = self.chain(q, want, gb)
        assert_filter_kat(np.ascontiguousarray(got), np.ascontiguousarray(want), 0 if q.use_filter == 1 else q.hdr, what)
        return got

    def chain(self, q, planes, gb):
        """the library's denoise chain over the literal's two planes and the stored original colour, id and original id of the frame"""
        import torch
        five = [planes[0], planes[1], quantise(gb["original_color"]), quantise(gb["id"]), quantise(gb["original_id"])]
        words = np.stack([np.ascontiguousarray(pl).view(np.uint32)[..., 0] for pl in five])                      # RGBA8: R in the low byte
        d_planes = torch.as_tensor(words.view(np.int32), device="cuda").contiguous()
        out = torch.zeros((q.height, q.width, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        self.hip.filter_planes_device(q, d_planes.data_ptr(), out.data_ptr())
        self.hip.sync()
        return out.cpu().numpy()


@pytest.mark.parametrize("name,n,hdr", STILL, ids=["%s_n%d_hdr%d" % c for c in STILL])
def test_every_depth_against_the_literal_and_the_oracle(hip, oracle, scenes, name, n, hdr):
    sc = scenes(name)
    hip.update_scene(sc)
    p = temporal_params(sc, W, H, n, hdr=hdr)
    frames = still_frames(p)
    want = oracle.render_sequence(sc, p, len(frames))
    run = Run(hip)
    for f, q in enumerate(frames):
        got = run.frame(q, "%s depth %d frame %d" % (name, n, f))
        rms, mism = assert_parity(got, want[f], "%s depth %d frame %d" % (name, n, f))
        assert mism == 0, "%s depth %d frame %d: %d floats differ from the oracle's (rms %s)" % (name, n, f, mism, rms)
    hip.temporal_reset()


@pytest.mark.parametrize("name,n", MOTION, ids=["%s_n%d" % c for c in MOTION])
def test_a_moving_camera_against_the_literal_and_the_oracle(hip, oracle, scenes, name, n):
    sc = scenes(name)
    hip.update_scene(sc)
    frames = motion_frames(temporal_params(sc, W, H, n), n + 4)
    want = oracle.render_sequence_frames(sc, frames)
    run, cov = Run(hip), Coverage(n)
    for f, q in enumerate(frames):
        got = run.frame(q, "%s depth %d frame %d" % (name, n, f), cov)
        rms, mism = assert_parity(got, want[f], "%s depth %d frame %d" % (name, n, f))
        assert mism == 0, "%s depth %d frame %d: %d floats differ from the oracle's (rms %s)" % (name, n, f, mism, rms)
    print(name, cov.figures())
    cov.check(uncovered=name == "theater")
    hip.temporal_reset()


def test_where_only_w_tells_a_pixel_from_a_zero_texel(hip, scenes):
    """cornell from far away (temporal_util.far_frames): covered pixels whose location id stores as (0, 0, 0, 1 / 255) over an empty history and beside the
    vec4(0) stand-ins: a comparison of three of the four bytes counts them in"""
    sc = scenes("cornell")
    hip.update_scene(sc)
    n = 6
    run, cov = Run(hip), Coverage(n)
    for f, q in enumerate(far_frames(sc, temporal_params(sc, W, H, n))):
        run.frame(q, "far cornell frame %d" % f, cov)
        if f == 0:
            assert only_w_tells(run.gbuffers).sum() >= 100
    assert cov.uncovered_stand_in >= 100 and set(range(1, n + 1)) <= cov.counters, cov.figures()
    hip.temporal_reset()


def centre_triangle(oracle, sc, p):
    """the geometry row of the triangle the centre pixel sees"""
    from flexlight_hip.scene_io import FrameParams, SceneView
    F3 = C.c_float * 3
    lib = oracle.lib()
    lib.flx_oracle_primary.argtypes = [C.POINTER(SceneView), C.POINTER(FrameParams), C.c_uint32, C.c_uint32, F3, C.POINTER(C.c_int), C.POINTER(C.c_int), F3]
    lib.flx_oracle_primary.restype = None
    view = sc.view()
    suv, d, tid, tri = F3(), F3(), C.c_int(), C.c_int()
    lib.flx_oracle_primary(C.byref(view), C.byref(p), p.width // 2, p.height // 2, suv, C.byref(tid), C.byref(tri), d)
    assert tri.value >= 0
    return tri.value


def test_a_triangle_that_leaves_and_returns_costs_only_its_pixels_their_history(hip, oracle, scenes):
    """the scene changes, not the camera: a triangle of cornell's back wall is moved out of view and back (flx_scene_update) on the motion schedule.  The
    literal over the GPU's G-buffers is the only reference here."""
    sc = scenes("cornell")
    hip.update_scene(sc)
    n = 6
    frames = still_frames(temporal_params(sc, W, H, n), 2 * n)
    entry = centre_triangle(oracle, sc, frames[0])
    here = sc.arrays["geometry"].reshape(-1, 12)[entry:entry + 1].copy()
    assert here[0, 10] == 2
    away = here.copy()
    away[0, [1, 4, 7]] += np.float32(500.0)
    gone = [0, 1, 0, 0, 1, 1, 0, 1, 0, 1, 1, 0]
    run, cov, ids = Run(hip), Coverage(n), []
    try:
        for f, q in enumerate(frames):
            if f and gone[f] != gone[f - 1]:
                hip.update_scene_rows(entry, away if gone[f] else here)
            run.frame(q, "frame %d" % f, cov)
            ids.append(quantise(run.gbuffers["location_id"]))
    finally:
        hip.update_scene(sc)
        hip.temporal_reset()
    print(cov.figures())
    present, absent = ids[0], ids[1]
    changed = (present != absent).any(axis=-1)
    covered = (present != 0).any(axis=-1)
    assert 0 < changed.sum() < covered.sum()                               # only the triangle's pixels lose their history
    assert np.array_equal(ids[2], present) and np.array_equal(ids[4], absent)
    assert cov.partial >= 100 and len(cov.patterns) >= 8, cov.figures()
    assert set(range(1, n + 1)) <= cov.counters, cov.figures()


@pytest.mark.parametrize("n", [4, 5])
def test_with_the_filter_the_chain_reads_the_planes_the_literal_writes(hip, scenes, n):
    """use_filter = 1 under motion: the frame equals the library's chain (flx_filter_planes_device) over the literal's dColor / dIp and the stored original colour,
    id and original id of the frame, bit for bit — the chain is on both sides, the temporal pass is not"""
    sc = scenes("dragon")
    hip.update_scene(sc)
    frames = motion_frames(temporal_params(sc, W, H, n, use_filter=1), n + 4)
    run, cov = Run(hip), Coverage(n)
    got = [run.frame(q, "filter depth %d frame %d" % (n, f), cov) for f, q in enumerate(frames)]
    assert cov.partial >= 100 and cov.id_miss_oid_hit >= 100, cov.figures()
    assert not np.array_equal(got[0], got[-1])
    hip.temporal_reset()


def test_history_boundaries_on_one_context(hip, scenes):
    """what keeps and what forgets the history, each frame against the literal over the ring the test expects: a frame without temporal accumulation (plain, and
    through the chain) leaves the ring as it was; another depth, another frame size and flx_temporal_reset start a zero ring; temporal_samples 0 then 4 and 16
    then 20 name the same depth and keep it"""
    sc = scenes("dragon")
    hip.update_scene(sc)
    base = temporal_params(sc, W, H, 0)
    other = temporal_params(sc, W + 8, H - 4, 4)
    run = Run(hip)
    f = 0

    def frames(p, count, **kw):
        nonlocal f
        depth = effective_depth(p.temporal_samples)
        for _ in range(count):
            q = copy_params(p, random_seed=float(f % depth), **kw)
            q.camera[0] = p.camera[0] + np.float32(0.05 * (f % 3 == 1))
            got = run.frame(q, "frame %d (temporal_samples %d, %d x %d)" % (f, q.temporal_samples, q.width, q.height))
            f += 1
        return got

    frames(base, 3)                                                        # temporal_samples 0: a depth of 4
    frames(base, 1, is_temporal=0)                                         # not a temporal frame: the ring stays
    frames(base, 1, is_temporal=0, use_filter=1)                           # nor one that runs the chain over the same G-buffers
    frames(base, 2, temporal_samples=4)                                    # 4 is the depth 0 meant: the history stays, and wraps
    assert run.ring.pushed == 5
    run.fresh()
    frames(base, 3, temporal_samples=5)                                    # another depth: zero ring
    run.fresh()
    frames(base, 2, temporal_samples=4)                                    # and back
    run.fresh()
    frames(other, 3)                                                       # another size
    hip.temporal_reset()                                                   # flx_temporal_reset
    run.fresh()
    frames(other, 2)
    run.fresh()
    frames(copy_params(other, height=H), 2)                                # another height alone
    run.fresh()
    frames(copy_params(other, width=W), 2)                                 # another width alone
    run.fresh()
    frames(base, 17, temporal_samples=16)                                  # the ring of 16 wraps ...
    frames(base, 3, temporal_samples=20)                                   # ... and 20 is still 16: the history stays
    assert run.ring.pushed == 20
    hip.temporal_reset()


def test_strips_of_a_moving_camera(hip, scenes):
    """tile = (8, 1, 3) of a frame 36 rows high: the context's packed strips (rows 8 - 15 and the ragged 32 - 35), history kept per strip"""
    sc = scenes("theater")
    hip.update_scene(sc)
    n = 6
    p = temporal_params(sc, W, 36, n, tile=(8, 1, 3))
    assert hip.tile_rows(p) == list(range(8, 16)) + list(range(32, 36))
    whole = temporal_params(sc, W, 36, n)
    run, cov = Run(hip), Coverage(n)
    for f, q in enumerate(motion_frames(p, n + 4)):
        got = run.frame(q, "strips frame %d" % f, cov)
        assert got.shape == (12, W, 4)
    assert cov.partial >= 100 and len(cov.patterns) >= 8, cov.figures()
    # the strips are those rows of the whole frame
    hip.temporal_reset()
    last = [hip.render(q)[0] for q in motion_frames(whole, n + 4)][-1]
    assert np.array_equal(got, last[hip.tile_rows(p)], equal_nan=True)
    hip.temporal_reset()


def test_the_frame_loop_gives_the_frames_of_render(hip, scenes):
    """the motion run at depth 6 through flx_frame_begin / flx_frame_end with two frames in flight: the frames flx_render gave (held against the literal here)"""
    sc = scenes("theater")
    hip.update_scene(sc)
    n = 6
    frames = motion_frames(temporal_params(sc, W, H, n), n + 4)
    run, cov = Run(hip), Coverage(n)
    want = [run.frame(q, "frame %d" % f, cov) for f, q in enumerate(frames)]
    cov.check(uncovered=True)
    hip.temporal_reset()
    got, _, _ = run_loop(hip, [(q, {}) for q in frames], depth=2)
    hip.temporal_reset()
    assert len(got) == len(want)
    for f, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b, equal_nan=True), "frame %d of the loop" % f
