"""Traced batches with a volume on the GPU (flx_rays_trace_gather, flx_rays_trace_gather_device: csrc/flx_rays_gather.hip) against the CPU reference
(tests/rays_gather_ref, which test_rays_gather_cpu.py pins): every word of every row, a NaN equal to a NaN.  The volumes are baked on the device (face size 4: 96
rays a probe), copied down once and handed to both sides as the same floats."""
import numpy as np
import pytest
import torch

import rays_trace_util
from flexlight_hip import capi
from rays_gather_util import GAIN, assert_rows, batch, inactive_offsets, pinhole_rays, reference, small_grid, spanning_grid, trace_params, wanted, words_of
from volume_map_util import map_of
from volume_relocate_util import relocate_of

pytestmark = pytest.mark.gpu

SCENES = ("cornell", "dragon")            # the lockstep walk; the lane walk
GRIDS = ("span", "small")                 # 3 x 3 x 3 over the scene; 2 x 1 x 2 that the scene overhangs
FORMS = ("plain", "map", "offsets", "map_offsets")
FACE, MAP = 4, 4
# samples, max_reflections, min_importancy (None: the scene's), gain, visibility: S in {1, 3}, bounces in {0, 1, 2, 4}, a high threshold, gain in {0, 1 / pi}, the flag on and off
PARAMS = ((1, 0, None, GAIN, True), (3, 1, None, GAIN, False), (1, 2, None, 0.0, True), (3, 4, None, GAIN, True), (3, 4, 0.8, GAIN, False), (3, 2, None, GAIN, True))

_volumes = {}


@pytest.fixture(scope="module")
def ref(tmp_path_factory, oracle):
    return reference(tmp_path_factory)


def grid_of(points, which, visibility=True):
    return spanning_grid(points, visibility=visibility) if which == "span" else small_grid(points, visibility=visibility)


def volume(hip, oracle, scenes, name, which):
    """the scene uploaded; -> (scene, rays, points, {form: (vmap, sh, maps, offsets) as host arrays}), baked once per (scene, grid): the map forms with a map of size
    4, the offset forms after one relocateVolume pass from the lattice"""
    sc, rays = batch(oracle, scenes, name)
    points = pinhole_rays(oracle, scenes, name)[2]
    hip.update_scene(sc)
    if (name, which) not in _volumes:
        grid, vmap = grid_of(points, which), map_of(MAP, 3)
        t, probe = trace_params(sc, 1, 2), capi.ProbeParams(FACE)
        down = lambda x: x.detach().cpu().numpy().copy()      # noqa: E731
        sh, maps = hip.volume_bake_map_device(grid, t, probe, vmap)
        offsets = torch.zeros((grid.probes, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        hip.volume_relocate_device(grid, relocate_of(), FACE, offsets, t.texture_width)
        sh_moved, maps_moved = hip.volume_bake_relocated_device(grid, t, probe, offsets, vmap)
        hip.sync()
        sh, maps, offsets, sh_moved, maps_moved = down(sh), down(maps), down(offsets), down(sh_moved), down(maps_moved)
        assert np.isfinite(sh).all() and np.isfinite(maps).all() and np.isfinite(sh_moved).all() and np.isfinite(maps_moved).all() and np.isfinite(offsets[:, 0:3]).all()
        _volumes[(name, which)] = {"plain": (None, sh, None, None), "map": (vmap, sh, maps, None), "offsets": (None, sh_moved, None, offsets),
                                   "map_offsets": (vmap, sh_moved, maps_moved, offsets)}
    return sc, rays, points, _volumes[(name, which)]


def on_device(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def gathered(hip, rays, t, grid, form, gain=GAIN, order=0, stream=None, n=None):
    """rays (numpy [n, 8]) through trace_rays_gather_device into a poisoned buffer with eight rows behind the last -> words [n, 8]; nothing else is written"""
    vmap, sh, maps, offsets = form
    d = torch.from_numpy(np.ascontiguousarray(rays[:n] if n is not None else rays)).cuda()
    arrays = [on_device(sh), on_device(maps), on_device(offsets)]
    keep = [d.clone()] + [a.clone() for a in arrays if a is not None]
    n = d.shape[0]
    out = torch.full((n + 8, 32), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert hip.trace_rays_gather_device(d, t, grid, arrays[0], vmap, arrays[1], arrays[2], gain, out, order, stream) is out
    hip.sync()
    got = words_of(out)
    assert (got[n:] == 0xA5A5A5A5).all()                                          # nothing beyond row n - 1 is written; the inputs are read only
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip([d] + [a for a in arrays if a is not None], keep))      # (as words: a dead probe's rows are NaN)
    return got[:n]


def expected(ref, key, sc, t, rays, grid, form, gain=GAIN):
    vmap, sh, maps, offsets = form
    return wanted(key, lambda: ref.gather(sc, t, rays, grid, sh, gain, vmap=vmap, maps=maps, offsets=offsets))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("which", GRIDS)
@pytest.mark.parametrize("name", SCENES)
def test_every_form_equals_its_reference(hip, oracle, scenes, ref, name, which, form):
    """pinhole rays, their shuffle, rays that miss and rays whose paths leave the scene, over the parameters of PARAMS"""
    sc, rays, points, forms = volume(hip, oracle, scenes, name, which)
    for samples, bounces, importancy, gain, visibility in PARAMS:
        t, grid = trace_params(sc, samples, bounces, importancy), grid_of(points, which, visibility)
        want = expected(ref, (name, which, form, samples, bounces, importancy, gain, visibility), sc, t, rays, grid, forms[form], gain)
        what = "%s %s %s S %d K %d min %s gain %s visibility %s" % (name, which, form, samples, bounces, importancy, gain, visibility)
        print(what, "rows that hit:", int((want[:, 5] != 0xffffffff).sum()), "of", len(want))
        assert_rows(gathered(hip, rays, t, grid, forms[form], gain), want, what)
    info = hip.last_gather()
    assert (info["n"], info["slabs"], info["flags"], info["ordered"], info["record_bytes"]) == (len(rays), 1, FORMS.index(form), 0, 64)
    assert hip.last_trace()["lockstep"] in (0, 1)


@pytest.mark.parametrize("name", SCENES)
def test_the_inputs_are_what_the_issue_asks_for(hip, oracle, scenes, ref, name):
    """most hits lie inside the spanning grid; the small grid is overhung; some rays miss; some paths end on a miss before their last bounce; the volume changes rows"""
    sc, rays, points, forms = volume(hip, oracle, scenes, name, "span")
    grid, small = grid_of(points, "span"), grid_of(points, "small")
    lo = np.array(list(grid.origin)); hi = lo + np.array(list(grid.spacing)) * 2.0
    assert ((points >= lo) & (points <= hi)).all(axis=1).mean() > 0.9
    slo = np.array(list(small.origin)); shi = slo + np.array(list(small.spacing))
    assert ((points < slo) | (points > shi)).any(axis=1).mean() > 0.5
    t = trace_params(sc, 3, 4)
    want = expected(ref, (name, "span", "plain", 3, 4, None, GAIN, True), sc, t, rays, grid, forms["plain"])
    hit = want[:, 5] != 0xffffffff
    assert 8 <= (~hit).sum() and (want[hit, 7] < 12).any() and (want[hit, 7] == 12).any()
    constant = wanted((name, "constant", 3, 4), lambda: ref.gather(sc, t, rays, grid, forms["plain"][1], GAIN, offsets=inactive_offsets(grid.probes)))
    assert (want[hit, 0:3] != constant[hit, 0:3]).any(axis=1).mean() > 0.5


def test_a_dead_probe_poisons_nothing(hip, oracle, scenes, ref):
    """with offsets, the probe in the middle of the grid made inactive and its SH row and map rows filled with NaN: none of it is read"""
    sc, rays, points, forms = volume(hip, oracle, scenes, "cornell", "span")
    grid, t = grid_of(points, "span"), trace_params(sc, 3, 2)
    vmap, sh, maps, offsets = forms["map_offsets"]
    sh, maps, offsets = sh.copy(), maps.copy(), offsets.copy()
    dead = 13
    offsets.view(np.uint32)[dead, 3] |= capi.RELOCATE_INACTIVE
    sh[dead] = np.nan
    maps.reshape(grid.probes, -1)[dead] = np.nan
    for form in ((vmap, sh, maps, offsets), (None, sh, None, offsets)):
        want = ref.gather(sc, t, rays, grid, form[1], GAIN, vmap=form[0], maps=form[2], offsets=form[3])
        got = gathered(hip, rays, t, grid, form)
        nan = lambda rows: np.isnan(rows[:, 0:3].view(np.float32)).any(axis=1)      # noqa: E731
        assert not nan(want).any() and not (nan(got) & ~nan(want)).any()
        assert_rows(got, want, "dead probe, map %s" % (form[0] is not None))
    alive = offsets.copy()
    alive.view(np.uint32)[dead, 3] &= ~np.uint32(capi.RELOCATE_INACTIVE)
    poisoned = ref.gather(sc, t, rays, grid, sh, GAIN, offsets=alive)
    assert np.isnan(poisoned[:, 0:3].view(np.float32)).any(), "the dead probe is a corner of no path's last point: the test shows nothing"


@pytest.mark.parametrize("name", SCENES)
def test_seams(hip, oracle, scenes, ref, name):
    """slabs of 64 rays with a partial last one, one workgroup and the natural grid, one ray, 65 rays"""
    sc, rays, points, forms = volume(hip, oracle, scenes, name, "span")
    grid, t, form = grid_of(points, "span"), trace_params(sc, 3, 2), forms["map_offsets"]
    want = expected(ref, (name, "span", "map_offsets", 3, 2, None, GAIN, True), sc, t, rays, grid, form)
    part = slice(3072 - 200, 3072 + 157)                    # 357 rays across the end of the image and the start of its shuffle: five slabs of 64 and one of 37
    try:
        for groups in (1, 0):
            hip.set_query_groups(groups)
            hip.set_trace_slab(64)
            for order in (0, capi.TRACE_ORDER_HITS):
                assert_rows(gathered(hip, rays[part], t, grid, form, order=order), want[part], "%s slabs of 64, groups %d, order %d" % (name, groups, order))
                info = hip.last_gather()
                assert (info["n"], info["slabs"], info["slab"], info["ordered"]) == (357, 6, 64, order)
                assert info["lookup_groups"] == 1 and (info["path_groups"] == 1 or groups == 0)      # the last slab: 37 rays x 3 samples
            hip.set_trace_slab(0)
            for n in (1, 65):
                assert_rows(gathered(hip, rays, t, grid, form, n=n), want[:n], "%s n %d groups %d" % (name, n, groups))
                assert hip.last_gather()["lookup_groups"] == (n * 3 + 255) // 256
    finally:
        hip.set_query_groups(0)
        hip.set_trace_slab(0)
    assert_rows(gathered(hip, rays, t, grid, form), want, name)


def test_call_variants(hip, oracle, scenes, ref):
    """first-hit order, the host call, a producer stream, the same call twice"""
    sc, rays, points, forms = volume(hip, oracle, scenes, "dragon", "span")
    grid, t = grid_of(points, "span"), trace_params(sc, 3, 2)
    for name in FORMS:
        form = forms[name]
        want = expected(ref, ("dragon", "span", name, 3, 2, None, GAIN, True), sc, t, rays, grid, form)
        first = gathered(hip, rays, t, grid, form)
        assert_rows(first, want, name)
        assert np.array_equal(gathered(hip, rays, t, grid, form), first)                                   # the scratch is reused
        ordered = gathered(hip, rays, t, grid, form, order=capi.TRACE_ORDER_HITS)
        assert np.array_equal(ordered, first) and hip.last_gather()["ordered"] == 1
        vmap, sh, maps, offsets = form
        assert np.array_equal(words_of(hip.trace_rays_gather(rays, t, grid, sh, vmap, maps, offsets)), first)      # the host call
        assert np.array_equal(words_of(hip.trace_rays_gather(rays, t, grid, sh, vmap, maps, offsets, order=capi.TRACE_ORDER_HITS)), first)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        made = torch.from_numpy(rays).cuda(non_blocking=False) * 1.0                                            # written on the side stream
    arrays = [on_device(x) for x in forms["map"][1:3]]
    torch.cuda.current_stream().synchronize()
    out = hip.trace_rays_gather_device(made, t, grid, arrays[0], forms["map"][0], arrays[1], None, GAIN, None, 0, side)
    hip.sync()
    assert_rows(words_of(out), expected(ref, ("dragon", "span", "map", 3, 2, None, GAIN, True), sc, t, rays, grid, forms["map"]), "producer stream")
    assert hip.trace_rays_gather_device((0, 0), t, grid, arrays[0], out=0) == 0                                # n == 0: nothing is looked at but the scene and the params
    assert hip.trace_rays_gather(np.zeros((0, 8), np.float32), t, grid, forms["plain"][1]).shape == (0, 32)


def test_the_plain_trace_is_unchanged(hip, oracle, scenes, ref, tmp_path_factory):
    """flx_rays_trace_device on the same rays, after batches with a volume have used the shared scratch: flx_rays_trace_ref's rows"""
    plain = rays_trace_util.reference(tmp_path_factory)
    for name in SCENES:
        sc, rays, points, forms = volume(hip, oracle, scenes, name, "span")
        t = trace_params(sc, 3, 4)
        gathered(hip, rays, t, grid_of(points, "span"), forms["map"])
        d = torch.from_numpy(rays).cuda()
        torch.cuda.synchronize()
        for order in (0, capi.TRACE_ORDER_HITS):
            out = hip.trace_rays_ordered_device(d, t, order=order)
            hip.sync()
            assert_rows(words_of(out), wanted((name, "trace", 3, 4), lambda: plain.trace(sc, t, rays)), "%s order %d" % (name, order))


def test_refusals(hip, oracle, scenes, ref):
    """each refusal's status and message through the library, nothing written"""
    sc, rays_host, points, forms = volume(hip, oracle, scenes, "cornell", "span")
    grid, t = grid_of(points, "span"), trace_params(sc, 1, 1)
    vmap, sh_host, maps_host, offsets_host = forms["map_offsets"]
    n = 256
    rays_host = rays_host[:n]
    rays, sh, maps, offsets = on_device(rays_host), on_device(sh_host), on_device(maps_host), on_device(offsets_host)
    out = torch.full((n, 32), 0xA5, dtype=torch.uint8, device="cuda")
    host = np.zeros((n, 8), np.float32)
    torch.cuda.synchronize()
    with capi.Context(0) as fresh:
        with pytest.raises(capi.FlexLightHipError, match=r"failed \(3\): flx_rays_trace_gather: no scene and transforms uploaded"):
            fresh.trace_rays_gather_device(rays, t, grid, sh, out=out)
        assert fresh.last_gather()["slabs"] == 0
    before = hip.last_gather()

    def with_(**kw):
        q = trace_params(sc, 1, 1)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def grid_with(**kw):
        g = grid_of(points, "span")
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    def go(params=t, g=grid, s=sh.data_ptr(), m=vmap, d=maps.data_ptr(), f=offsets.data_ptr(), r=rays, o=out, **kw):      # (addresses: the library judges them, not the binding)
        return lambda: hip.trace_rays_gather_device(r, params, g, s, m, d, f, out=o, **kw)

    both = torch.zeros((2 * n, 8), dtype=torch.float32, device="cuda")
    big = torch.zeros((grid.probes * 16 + n * 2, 4), dtype=torch.float32, device="cuda")      # room for the maps, then for n rows of 32 bytes
    dev = "flx_rays_trace_gather_device: "
    refused = [
        # 1. the scene's and the trace params' own, an unknown order bit, the rays and the radiance
        (go(params=None), "flx_rays_trace_gather: params is NULL"),
        (go(params=with_(samples=0)), "flx_rays_trace_gather: samples is less than 1"),
        (go(params=with_(max_reflections=-1), r=(0, 0), o=0), "flx_rays_trace_gather: max_reflections is negative"),      # for n == 0 too
        (go(params=with_(texture_width=0)), "flx_rays_trace_gather: texture_width is less than 1"),
        (go(order=2), "flx_rays_trace_gather: order has a bit beyond FLX_TRACE_ORDER_HITS"),
        (go(r=(0, n)), dev + "an array is NULL"),
        (go(r=(host.ctypes.data, n)), dev + "the rays are not n rows in memory of the context's device"),
        (go(o=out.data_ptr() + 8), dev + "the radiance is not n rows in memory of the context's device, 16-byte aligned"),
        (go(r=(both.data_ptr(), n), o=both.data_ptr() + 32 * (n - 1)), dev + "the rays and the radiance overlap"),
        # 2. the volume: NULL, its grid, its map, its arrays, in the volume calls' words
        (go(volume=False), dev + "the volume is NULL"),
        (go(g=None), dev + "the grid is NULL"),
        (go(g=grid_with(count=(3, 0, 3))), dev + "a count of the grid is 0"),
        (go(g=grid_with(spacing=(1.0, -1.0, 1.0))), dev + "a spacing is not greater than 0"),
        (go(g=grid_with(normal_bias=float("nan"))), dev + "normal_bias is negative or not finite"),
        (go(g=grid_with(flags=2)), dev + "flags has a bit beyond FLX_VOLUME_VISIBILITY"),
        (go(g=grid_with(reserved=1)), dev + "reserved is not 0"),
        (go(m=capi.VolumeMap(17, 3)), dev + "the map's size is not one of 1 .. 16"),
        (go(m=capi.VolumeMap(4, 9)), dev + "the map's sharpness is above 8"),
        (go(s=None), dev + "an array is NULL"),
        (go(s=sh_host.ctypes.data), dev + "the SH rows are not nx \\* ny \\* nz rows of 144 bytes in memory of the context's device"),
        (go(s=sh.data_ptr() + 4), dev + "the SH rows are not nx \\* ny \\* nz rows of 144 bytes in memory of the context's device, 16-byte aligned"),
        (go(d=maps_host.ctypes.data), dev + "the maps are not n_probes \\* size \\* size rows of 16 bytes in memory of the context's device"),
        (go(s=big.data_ptr(), d=big.data_ptr() + 16), dev + "the maps overlap another array"),
        (go(f=offsets_host.ctypes.data), dev + "the offsets are not nx \\* ny \\* nz rows of 16 bytes"),
        (go(f=sh.data_ptr() + 144), dev + "the arrays overlap"),
        # 3. this call's own
        (go(gain=-1.0), dev + "gain is negative or not finite"),
        (go(gain=float("inf")), dev + "gain is negative or not finite"),
        (go(gain=float("nan")), dev + "gain is negative or not finite"),
        (go(reserved=1), dev + "the volume's reserved word is not 0"),
        (go(d=None), dev + "map and maps are not both given or both NULL"),
        (go(m=None), dev + "map and maps are not both given or both NULL"),
        (go(f=rays.data_ptr()), dev + "an array of the volume overlaps the rays or the radiance"),
        (go(s=both.data_ptr(), r=(both.data_ptr() + grid.probes * 144 - 16, n)), dev + "an array of the volume overlaps the rays or the radiance"),
        (go(d=big.data_ptr(), o=big.data_ptr() + grid.probes * 256 - 32), dev + "an array of the volume overlaps the rays or the radiance"),
        # the host call, under its own name
        (lambda: hip.trace_rays_gather(rays_host, t, grid, sh_host, gain=-0.5), "flx_rays_trace_gather: gain is negative or not finite"),
        (lambda: hip.trace_rays_gather(rays_host, t, grid, sh_host, vmap, None), "flx_rays_trace_gather: map and maps are not both given or both NULL"),
        (lambda: hip.trace_rays_gather(rays_host, t, grid_with(floor=2.0), sh_host), "flx_rays_trace_gather: floor is not one of 0 .. 1"),
        (lambda: hip.trace_rays_gather(rays_host, t, grid, None), "flx_rays_trace_gather: an array is NULL"),
        (lambda: hip.trace_rays_gather(rays_host, t, grid, sh_host, reserved=5), "flx_rays_trace_gather: the volume's reserved word is not 0"),
    ]
    for call, message in refused:
        status = r"failed \(1\): "
        with pytest.raises(capi.FlexLightHipError, match=status + message):
            call()
    hip.sync()
    assert (words_of(out) == 0xA5A5A5A5).all() and hip.last_gather() == before      # nothing was enqueued
    # the accepted borders: gain 0 and the largest gain
    for gain in (0.0, float(np.finfo(np.float32).max)):
        hip.trace_rays_gather_device(rays, t, grid, sh, vmap, maps, offsets, gain, out)
    hip.sync()
    assert (words_of(out)[:, 3].view(np.float32) == 1.0).any()
