"""Pipeline 1 — the per-pixel trace kernels — instantiation by instantiation against the CPU oracle.

launch_trace_pixels picks one of sixteen kernels: k_trace_pixels<COUNT, LOCK> (a pixel's samples one after the other) and k_trace_samples<COUNT, LOCK, S>
(the S samples of a pixel side by side, the shader's cross-sample globals replayed afterwards in its order) for S = 2, 4, 8.  Filter frames, temporal frames
and small scenes run them.  Every case here renders under flx_set_pipeline(1), with and without the work counters (COUNT), with the samples side by side
and one after the other, on a scene of the lockstep walk (LOCK) and on the dragon; it holds the frame (and a filter frame's G-buffers) bit for bit
against the oracle with equal counters, and flx_debug_last_trace_kernel against the dispatch rule written out below — so that a change of the rule
cannot send every case to the fallback unseen."""
import numpy as np
import pytest

from parity_util import bit_mismatches

pytestmark = pytest.mark.gpu

TS_MAX_BOUNCES = 4                 # FLX_TS_MAX_BOUNCES of flx_kernels.hip
LDS_BYTES = 64 * 1024
LOCK_SCENES = ("cornell", "cornell_obj", "theater")      # at most 128 entries, all in transform 0: the wave's lockstep walk


def side_by_side(spp, bounces, sample_parallel=True):
    """the rule of launch_trace_pixels: S = spp for k_trace_samples, 0 for k_trace_pixels.  Side by side: 2, 4 or 8 samples, at most
    FLX_TS_MAX_BOUNCES bounces, and the workgroup's LDS — 64 hits, 64 last originalColors, S x 64 results of 32 B, a 24 B log entry per
    bounce, sample and lane — within 64 KB"""
    if not sample_parallel or spp not in (2, 4, 8) or bounces > TS_MAX_BOUNCES:
        return 0
    lds = (128 + 2 * spp * 64) * 16 + max(bounces, 1) * spp * 64 * 24
    return spp if lds <= LDS_BYTES else 0


def test_the_dispatch_rule_at_its_boundaries():
    """the cells either side of the rule's edges, pinned: 8 x 3 fits its log, 8 x 4 (67 584 B) does not; 4 x 4 fits, 4 x 5 has too many bounces"""
    assert side_by_side(8, 3) == 8
    assert side_by_side(8, 4) == 0
    assert (128 + 2 * 8 * 64) * 16 + 4 * 8 * 64 * 24 == 67584
    assert side_by_side(4, 4) == 4
    assert side_by_side(4, 5) == 0
    assert side_by_side(2, 4) == 2 and side_by_side(2, 5) == 0
    assert [side_by_side(s, 3) for s in (1, 3, 16)] == [0, 0, 0]
    assert side_by_side(8, 0) == 8                     # (no bounce: a log of one)
    assert side_by_side(4, 3, sample_parallel=False) == 0


@pytest.fixture
def px(hip):
    """the context under pipeline 1; every knob the tests turn is put back"""
    hip.set_pipeline(1)
    try:
        yield hip
    finally:
        hip.set_sample_parallel(1)
        hip.set_pipeline(0)
        hip.set_lockstep(True)
        hip.set_angle_table(True)


def test_the_boundary_cells_run_the_kernels_they_should(px, scenes):
    """the same four cells on the GPU, the kernels written out literally rather than through side_by_side()"""
    for name, lock in (("cornell", 1), ("dragon", 0)):
        sc = scenes(name)
        px.update_scene(sc)
        for (spp, bounces), s in {(8, 3): 8, (8, 4): 0, (4, 4): 4, (4, 5): 0}.items():
            px.render(sc.frame_params(width=24, height=16, samples=spp, max_reflections=bounces, use_filter=0))
            assert px.last_trace_kernel() == (s, lock, 0), (name, spp, bounces)


_ORACLE_CACHE = {}


def _oracle(oracle, sc, name, p, gbuffers=False):
    """the oracle's frame once per (scene, parameters)"""
    key = (name, bytes(p), gbuffers)
    if key not in _ORACLE_CACHE:
        _ORACLE_CACHE[key] = oracle.render(sc, p, gbuffers=gbuffers)
    return _ORACLE_CACHE[key]


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    mism = bit_mismatches(got, want)
    assert mism == 0, "%s: %d of %d floats differ in bits" % (what, mism, got.size)


def _lock_of(name, lockstep=True):
    return 1 if (name in LOCK_SCENES and lockstep) else 0


def _check_frame(hip, oracle, sc, name, p, tag, lockstep=True, gbuffers=False, modes=(1, 0), ran=None):
    """p under every (sample_parallel, counters) pair: frame (and G-buffers) and counters equal to the oracle's, the kernel the rule names"""
    want, want_cnt, want_gb = _oracle(oracle, sc, name, p, gbuffers=gbuffers)
    hip.set_lockstep(lockstep)
    for sp in modes:
        hip.set_sample_parallel(sp)
        for counted in (True, False):
            what = "%s sample_parallel %d counters %d" % (tag, sp, counted)
            got, cnt, gb = hip.render(p, gbuffers=gbuffers, counters=counted)
            kernel = hip.last_trace_kernel()
            assert hip.last_pipeline() == 1, what
            assert kernel == (side_by_side(p.samples, p.max_reflections, sp), _lock_of(name, lockstep), int(counted)), (what, kernel)
            if ran is not None:
                ran.add(kernel)
            _same(got, want, what)
            if counted:
                assert cnt == want_cnt, what
            if gbuffers:
                for key in want_gb:
                    _same(gb[key], want_gb[key], "%s G-buffer %s" % (what, key))
    return want, want_cnt, want_gb


# ---- the dispatch matrix --------------------------------------------------------------------------------------------------------------------------------------
SPPS = (1, 2, 3, 4, 8, 16)
BOUNCES = (0, 1, 3, 4, 5)
MATRIX_SIZE = (61, 37)             # ragged against the 8 x 8 tile of k_trace_samples and the 16 x 16 workgroup of k_trace_pixels


@pytest.mark.parametrize("bounces", BOUNCES)
@pytest.mark.parametrize("spp", SPPS)
def test_dispatch_matrix(px, oracle, scenes, spp, bounces):
    """every (samples, bounces) cell: the lockstep scene with both walks and the dragon, samples side by side and one after the other, counted and not"""
    for name, lockstep in (("cornell", True), ("cornell", False), ("dragon", True)):
        sc = scenes(name)
        px.update_scene(sc)
        p = sc.frame_params(width=MATRIX_SIZE[0], height=MATRIX_SIZE[1], samples=spp, max_reflections=bounces, use_filter=0)
        p.random_seed = float((spp + bounces) % 5)
        _check_frame(px, oracle, sc, name, p, "%s lockstep %d %d spp %d bounces" % (name, lockstep, spp, bounces), lockstep=lockstep)


def test_every_instantiation_runs(px, scenes):
    """the union of (S, LOCK, COUNT) over the matrix's cells is all sixteen kernels: k_trace_pixels<COUNT, LOCK> and k_trace_samples<COUNT, LOCK, S>
    for S = 2, 4, 8 (the dispatch alone, on frames of one 8 x 8 tile; the matrix above holds each frame against the oracle)"""
    ran = set()
    for name, lockstep in (("cornell", True), ("cornell", False), ("dragon", True)):
        sc = scenes(name)
        px.update_scene(sc)
        px.set_lockstep(lockstep)
        for spp in SPPS:
            for bounces in BOUNCES:
                p = sc.frame_params(width=8, height=8, samples=spp, max_reflections=bounces, use_filter=0)
                for sp in (1, 0):
                    px.set_sample_parallel(sp)
                    for counted in (True, False):
                        px.render(p, counters=counted)
                        kernel = px.last_trace_kernel()
                        assert kernel == (side_by_side(spp, bounces, sp), _lock_of(name, lockstep), int(counted)), (name, lockstep, spp, bounces, sp, counted, kernel)
                        ran.add(kernel)
    assert ran == {(s, lock, count) for s in (0, 2, 4, 8) for lock in (0, 1) for count in (0, 1)}, sorted(ran)


def test_other_pipelines_report_no_trace_kernel(px, scenes):
    sc = scenes("cornell")
    px.update_scene(sc)
    p = sc.frame_params(width=16, height=16, samples=2, max_reflections=2, use_filter=0)
    px.render(p)
    assert px.last_trace_kernel() == (2, 1, 0)
    for pipeline in (2, 3):
        px.set_pipeline(pipeline)
        px.render(p)
        assert px.last_pipeline() == pipeline
        assert px.last_trace_kernel() == (-1, -1, -1), pipeline


# ---- filter frames: the five G-buffers at S = 8 and S = 4 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h,spp,bounces,lockstep", [
    ("dragon", 130, 75, 8, 3, True),          # glass: the glassFilter / dontFilter bits of the replay
    ("cornell_obj", 100, 60, 4, 3, True),     # configs[1]'s samples and bounces (and many tiles of sky)
    ("cornell_obj", 100, 60, 4, 3, False),
    ("cornell", 45, 29, 8, 3, True),
    ("dragon", 45, 29, 2, 4, True),
])
def test_filter_frames_with_gbuffers(px, oracle, scenes, name, w, h, spp, bounces, lockstep):
    sc = scenes(name)
    px.update_scene(sc)
    p = sc.frame_params(width=w, height=h, samples=spp, max_reflections=bounces, use_filter=1)
    _, _, want_gb = _check_frame(px, oracle, sc, name, p, "%s %dx%d %d spp %d bounces filter" % (name, w, h, spp, bounces), lockstep=lockstep, gbuffers=True)
    if name == "dragon" and spp == 8:
        assert (want_gb["color_ip"][..., 3] > 0).sum() > 0, "no glass path in the frame"


# ---- temporal frames without the filter (k_trace_samples' is_temporal epilogue) -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,spp,bounces,sample_parallel", [
    ("cornell", 2, 3, 1), ("dragon", 4, 3, 1), ("cornell_obj", 8, 3, 1), ("dragon", 8, 2, 0),
])
def test_temporal_frames_without_filter(px, oracle, scenes, name, spp, bounces, sample_parallel):
    """six frames over a history of four (the ring wraps), counted and not, against flx_oracle_render_sequence"""
    sc = scenes(name)
    px.update_scene(sc)
    p = sc.frame_params(width=53, height=35, samples=spp, max_reflections=bounces, use_filter=0)
    p.is_temporal, p.temporal_samples = 1, 4
    frames = 6
    want = oracle.render_sequence(sc, p, frames)
    px.set_sample_parallel(sample_parallel)
    try:
        for counted in (True, False):
            px.temporal_reset()
            for f in range(frames):
                p.random_seed = float(f % 4)
                got, _, _ = px.render(p, counters=counted)
                what = "%s %d spp temporal frame %d counters %d" % (name, spp, f, counted)
                assert px.last_trace_kernel() == (spp if sample_parallel else 0, _lock_of(name), int(counted)), what
                _same(got, want[f], what)
    finally:
        px.temporal_reset()


# ---- edge shapes at S = 2, 4, 8 -------------------------------------------------------------------------------------------------------------------------------
EDGE_SIZES = [(1, 1), (1, 13), (13, 1), (7, 7), (8, 8), (9, 9), (65, 33)]


@pytest.mark.parametrize("spp", [2, 4, 8])
def test_edge_shapes(px, oracle, scenes, spp):
    """frames of one pixel, one column, one row, smaller than a tile, one tile, one tile and a pixel, and a ragged frame"""
    for name in ("cornell", "dragon"):
        sc = scenes(name)
        px.update_scene(sc)
        for w, h in EDGE_SIZES:
            p = sc.frame_params(width=w, height=h, samples=spp, max_reflections=3, use_filter=0)
            _check_frame(px, oracle, sc, name, p, "%s %dx%d %d spp" % (name, w, h, spp))


@pytest.mark.parametrize("spp", [2, 4, 8])
def test_strips_of_tiled_frames(px, oracle, scenes, spp):
    """a rank's strips (rows of 1 over 3 ranks, of 8 over 5): every strip equals the oracle's strip and the rows of the whole frame"""
    for name in ("cornell", "dragon"):
        sc = scenes(name)
        px.update_scene(sc)
        whole = sc.frame_params(width=45, height=43, samples=spp, max_reflections=3, use_filter=0)
        want_whole = _oracle(oracle, sc, name, whole)[0]
        for tr, tc in ((1, 3), (8, 5)):
            for r in range(tc):
                p = sc.frame_params(width=45, height=43, samples=spp, max_reflections=3, use_filter=0, tile=(tr, r, tc))
                got = _check_frame(px, oracle, sc, name, p, "%s %d spp strip (%d, %d, %d)" % (name, spp, tr, r, tc))[0]
                _same(got, want_whole[px.tile_rows(p)], "%s %d spp strip (%d, %d, %d) against the whole frame" % (name, spp, tr, r, tc))


def _moved(sc, p, i):
    """frame i of a camera move: another position, view direction, seed and ambient"""
    from flexlight_hip.scene_io import view_matrix
    cam = sc.meta["camera"]
    q = type(p).from_buffer_copy(p)
    q.camera[:] = [cam["x"] + 0.35 * i, cam["y"] + 0.1 * i, cam["z"] - 0.2 * i]
    q.view_matrix[:] = view_matrix(cam["fx"] + 0.07 * i, cam["fy"] - 0.03 * i, cam["fov"], p.width, p.height).tolist()
    q.random_seed = float(i % 3)
    q.ambient[:] = [a * (1.0 + 0.25 * i) for a in sc.meta["ambient"]]
    return q


@pytest.mark.parametrize("spp", [2, 4, 8])
def test_batch_of_moved_cameras(px, oracle, scenes, spp):
    """three frames of a camera move in one launch (frame_index inside the kernel): each against its own oracle frame, the counters the sum"""
    for name in ("cornell", "dragon"):
        sc = scenes(name)
        px.update_scene(sc)
        p = sc.frame_params(width=37, height=27, samples=spp, max_reflections=3, use_filter=0)
        frames = [_moved(sc, p, i) for i in range(3)]
        wants = [_oracle(oracle, sc, name, q) for q in frames]
        for sp in (1, 0):
            px.set_sample_parallel(sp)
            for counted in (True, False):
                what = "%s %d spp batch sample_parallel %d counters %d" % (name, spp, sp, counted)
                got, cnt = px.render_batch(frames, counters=counted)
                assert px.last_trace_kernel() == (spp if sp else 0, _lock_of(name), int(counted)), what
                for i, (want, _, _) in enumerate(wants):
                    _same(got[i], want, "%s frame %d" % (what, i))
                if counted:
                    assert cnt == {k: sum(c[k] for _, c, _ in wants) for k in cnt}, what


def _sky_view(px, sc):
    """the dragon from far outside its room, looking away from it: no primary ray hits anything"""
    from flexlight_hip import scene_io
    cam = sc.meta["camera"]
    for dy, fy in ((1.0e3, 1.4), (1.0e3, -1.4), (-1.0e3, 1.4), (-1.0e3, -1.4)):
        q = sc.frame_params(width=40, height=24, samples=2, max_reflections=3, use_filter=0)
        q.camera[1] += dy
        q.view_matrix[:] = scene_io.view_matrix(cam["fx"], fy, cam["fov"], q.width, q.height).tolist()
        if px.render(q, counters=True)[1]["primary_hits"] == 0:
            return q
    return None


@pytest.mark.parametrize("spp", [2, 4, 8])
def test_all_sky_frame(px, oracle, scenes, spp):
    """every tile of the frame is sky: the waves of samples 1 .. S - 1 leave at once, wave 0 writes the tile (k_trace_samples' !anyCovered return)"""
    sc = scenes("dragon")
    px.update_scene(sc)
    p = _sky_view(px, sc)
    assert p is not None
    p.samples = spp
    for filt in (0, 1):
        p.use_filter = filt
        want, want_cnt, _ = _check_frame(px, oracle, sc, "dragon", p, "sky %d spp filter %d" % (spp, filt), gbuffers=bool(filt))
        assert want_cnt["primary_hits"] == 0


@pytest.mark.parametrize("spp", [2, 4, 8])
@pytest.mark.parametrize("min_importancy", [0.0, 1.01])
def test_min_importancy(px, oracle, scenes, spp, min_importancy):
    """0: every path runs all its bounces; 1.01: even bounce 0 is switched off while max_reflections > 0 (no sample shades, the globals stay as main() set them)"""
    for name in ("cornell", "dragon"):
        sc = scenes(name)
        px.update_scene(sc)
        for filt in (0, 1):
            p = sc.frame_params(width=29, height=19, samples=spp, max_reflections=3, use_filter=filt, min_importancy=min_importancy)
            _, want_cnt, _ = _check_frame(px, oracle, sc, name, p, "%s %d spp min_importancy %g filter %d" % (name, spp, min_importancy, filt), gbuffers=bool(filt))
            if min_importancy > 1.0:
                assert want_cnt["shades"] == 0


def test_without_the_angle_table(px, oracle, scenes):
    """S = 8 with every shade computing the per-triangle angles itself"""
    px.set_angle_table(False)
    for name in ("cornell", "dragon"):
        sc = scenes(name)
        px.update_scene(sc)
        for filt in (0, 1):
            p = sc.frame_params(width=45, height=29, samples=8, max_reflections=3, use_filter=filt)
            _check_frame(px, oracle, sc, name, p, "%s 8 spp no angle table filter %d" % (name, filt), gbuffers=bool(filt))
