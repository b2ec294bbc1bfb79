"""Light probes on the device (include/flexlight_hip_debug.h, "light probes"): k_probe_rays' rows and k_probe_sh's SH rows are the CPU reference's bits
(tests/probe_ref, the same include/flx_probe.h) for every size and count at which the kernels take another path; flx_probes_sh_device is the three calls one after
the other, bit for bit, whatever the chunk and the order; the ray call needs no scene; every refusal says its words and leaves the output as it was."""
import numpy as np
import pytest
import torch

from flexlight_hip import capi
from probe_util import assert_same_words, cornell_probes, finished, poisoned, positions_of, reference, synthetic_radiance
from rays_trace_util import trace_params

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 4, 5, 8, 11)       # w w below 256 (the face is the lane's own), 8: 64; R below 64 for 1 .. 3 (slots without a texel), 4: one or two texels a slot, 8: exactly six, 11: w w = 121 across workgroups
COUNTS = (1, 3, 4, 5, 9)             # 1, 3, 5: the last workgroup of the reduction has waves without a probe
WIDE = (16, 32)                      # w w = 256 and 1024: a workgroup of k_probe_rays lies within one face, which one or four workgroups cover


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return reference(tmp_path_factory)


def device_rays(ctx, positions, w):
    n = len(positions) * 6 * w * w
    out = poisoned(n, 32)
    d_positions = torch.from_numpy(positions).cuda()
    torch.cuda.synchronize()
    assert ctx.probe_rays_device(d_positions, w, out=out) is out
    return finished(ctx, out, n, 8)


def device_reduce(ctx, radiance, n, params):
    out = poisoned(n, 144)
    d_radiance = torch.from_numpy(radiance.view(np.uint8)).cuda()
    torch.cuda.synchronize()
    assert ctx.probe_reduce_device(d_radiance, n, params, out=out) is out
    return finished(ctx, out, n, 36)


@pytest.mark.parametrize("w", SIZES + WIDE)
def test_ray_rows_are_the_references_bits(hip, ref, w):
    for n in COUNTS if w not in WIDE else (3,):
        positions = positions_of(n, seed=n)
        want = ref.rays(positions, w)
        assert_same_words(device_rays(hip, positions, w), want, "%d probes of w = %d" % (n, w))
        if n in (1, 5):
            assert_same_words(hip.probe_rays(positions, w), want, "the host variant, %d probes of w = %d" % (n, w))
            assert_same_words(hip.probe_rays(positions[:, :3], w), want, "the host variant, three floats a position")


def test_rays_need_no_scene(ref):
    positions = positions_of(5)
    with capi.Context(0) as fresh:
        assert_same_words(device_rays(fresh, positions, 5), ref.rays(positions, 5), "a context without a scene")
        assert_same_words(fresh.probe_rays(positions, 3), ref.rays(positions, 3), "its host variant")


@pytest.mark.parametrize("w", SIZES)
def test_the_reduction_is_the_references_bits(hip, ref, w):
    for n in COUNTS:
        radiance = synthetic_radiance(n, w, seed=100 * w + n)
        sky = (0.25, 0.5, 4.0)
        params = capi.ProbeParams(face_size=w, sky=sky)
        want = ref.reduce(radiance, n, w, sky)
        assert np.isfinite(want).all() and (want[:, 3] > 0).all()
        assert_same_words(device_reduce(hip, radiance, n, params), want, "%d probes of w = %d" % (n, w))
        if n in (1, 5):
            assert_same_words(hip.probe_reduce(radiance, n, params), want, "the host variant, %d probes of w = %d" % (n, w))


def test_all_misses_under_a_sky(hip, ref):
    for w, n in ((3, 3), (8, 5)):
        radiance = synthetic_radiance(n, w, seed=7, all_miss=True)
        sky = (3.0, 0.125, 1.0e-3)
        want = ref.reduce(radiance, n, w, sky)
        assert (want[:, 0:3] > 0).all() and (want[:, (7, 11, 15)] == 0).all()
        assert_same_words(device_reduce(hip, radiance, n, capi.ProbeParams(face_size=w, sky=sky)), want, "w = %d" % w)
        dark = device_reduce(hip, radiance, n, capi.ProbeParams(face_size=w))
        assert (dark[:, [k for k in range(36) if k != 3]] == 0).all() and (dark[:, 3] != 0).all()      # sky = 0: only the sum of d_omega is left


def test_end_to_end_is_the_three_calls(hip, oracle, scenes):
    sc, t, positions = cornell_probes(oracle, scenes)
    hip.update_scene(sc)
    w, n, rays = 8, 5, 384
    d_positions = torch.from_numpy(positions).cuda()
    torch.cuda.synchronize()
    sky = (0.5, 0.25, 0.125)
    generated = hip.probe_rays_device(d_positions, w)
    radiance = hip.trace_rays_ordered_device(generated, t, order=capi.TRACE_ORDER_HITS)
    want = hip.probe_reduce_device(radiance, n, capi.ProbeParams(face_size=w, sky=sky))
    hip.sync()
    want = want.cpu().numpy()
    assert np.isfinite(want).all()
    for order in (0, capi.TRACE_ORDER_HITS):
        params = capi.ProbeParams(face_size=w, order=order, sky=sky)
        for chunk, chunks in ((2, 3), (0, 1)):
            hip.set_probe_chunk(chunk)
            out = poisoned(n, 144)
            torch.cuda.synchronize()
            hip.probes_sh_device(d_positions, t, params, out=out)
            assert_same_words(finished(hip, out, n, 36), want, "order %d, chunk %d" % (order, chunk))
            last = hip.last_probes()
            assert last == {"chunks": chunks, "chunk": chunk or (1 << 21) // rays, "face_size": w, "n": n, "order": order, "rays": rays,
                            "reduce_groups": 1 if chunk else 2}, last
        hip.set_probe_chunk(0)
        assert_same_words(hip.probes_sh(positions, t, params), want, "the host variant, order %d" % order)
    params = capi.ProbeParams(face_size=w, sky=sky)
    for k in range(n):                                     # a probe's row depends on nothing else in the call
        assert_same_words(hip.probes_sh(positions[k:k + 1], t, params), want[k:k + 1], "probe %d alone" % k)
    parts = capi.unpack_sh(want)
    assert ((parts["coverage"] > 0) & (parts["coverage"] <= parts["weight"])).all()
    assert (parts["mean_distance"] > 0).all() and (parts["coefficients"][:, 0] > 0).all()
    assert np.array_equal(capi.probe_irradiance(want, np.tile(np.array([0, 1, 0], np.float32), (n, 1)))[2], capi.probe_irradiance(want[2], np.array([0, 1, 0], np.float32)))


def test_probes_between_two_frames_of_the_loop(hip, oracle, scenes):
    sc, t, positions = cornell_probes(oracle, scenes)
    hip.update_scene(sc)
    params = capi.ProbeParams(face_size=8)
    want = hip.probes_sh(positions, t, params)
    frames = [sc.frame_params(width=48, height=36, samples=2, max_reflections=3, use_filter=0) for _ in range(2)]
    frames[1].random_seed = frames[0].random_seed + 1.0
    oracle_frames = [oracle.render(sc, q)[0] for q in frames]
    d_positions = torch.from_numpy(positions).cuda()
    out = poisoned(5, 144)
    torch.cuda.synchronize()
    for q in frames:
        hip.frame_begin(q)
    assert hip.frames_in_flight() == 2
    hip.probes_sh_device(d_positions, t, params, out=out)
    got = [hip.frame_end()[0] for _ in frames]
    assert_same_words(finished(hip, out, 5, 36), want, "between the frames")
    for image, frame in zip(got, oracle_frames):
        image = np.asarray(image).reshape(frame.shape)
        assert ((image.view(np.uint32) == frame.view(np.uint32)) | (np.isnan(image) & np.isnan(frame))).all()
    assert not np.array_equal(got[0], got[1])


def test_refusals(hip, oracle, scenes):
    sc, t, positions = cornell_probes(oracle, scenes)
    hip.update_scene(sc)
    torch.cuda.empty_cache()                                        # (the allocations below are then the device's own, of exactly these sizes)
    good = capi.ProbeParams(face_size=2)
    hip.probes_sh(positions, t, good)
    before = hip.last_probes()
    d_positions = torch.from_numpy(positions).cuda()
    rows, sh = poisoned(5 * 24, 32), poisoned(5, 144)
    host = np.zeros((64, 36), np.float32)
    short = torch.full((20 << 20,), 0xA5, dtype=torch.uint8, device="cuda")     # 20 MB, an allocation of its own: too short for 2 probes of w = 256 (24 MB of rows) and for 1 400 000 positions
    torch.cuda.synchronize()
    P, R, S = d_positions.data_ptr(), rows.data_ptr(), sh.data_ptr()

    def with_(**kw):
        q = trace_params(sc.frame_params(width=8, height=8, samples=2, max_reflections=3, use_filter=0))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    nan, inf = float("nan"), float("inf")
    rays_device = lambda p=(P, 5), w=2, out=R: hip.probe_rays_device(p, w, out=out)
    reduce_device = lambda r=R, n=5, q=good, out=S: hip.probe_reduce_device(r, n, q, out=out)
    sh_device = lambda p=(P, 5), q=good, tt=t, out=S: hip.probes_sh_device(p, tt, q, out=out)
    refused = [
        (lambda: rays_device(w=0), "flx_probe_rays_device: face_size is not one of 1 .. 256"),
        (lambda: rays_device(w=257), "flx_probe_rays_device: face_size is not one of 1 .. 256"),
        (lambda: hip.probe_rays(positions, 0), "flx_probe_rays: face_size is not one of 1 .. 256"),
        (lambda: rays_device(p=(P, 10923), w=256), "flx_probe_rays_device: n_probes \\* 6 \\* face_size \\* face_size is 2\\^32 or more"),
        (lambda: rays_device(p=(0, 5)), "flx_probe_rays_device: an array is NULL"),
        (lambda: rays_device(out=0), "flx_probe_rays_device: an array is NULL"),
        (lambda: rays_device(p=(positions.ctypes.data, 5)), "the positions are not n_probes rows of 16 bytes in memory of the context's device"),      # host memory
        (lambda: rays_device(p=(P + 4, 4)), "the positions are not n_probes rows of 16 bytes in memory of the context's device, 16-byte aligned"),
        (lambda: rays_device(p=(short.data_ptr(), 1400000), w=1), "the positions are not n_probes rows of 16 bytes"),                        # an allocation too short
        (lambda: rays_device(out=host.ctypes.data), "the rays are not n_probes \\* 6 \\* face_size \\* face_size rows in memory of the context's device"),
        (lambda: rays_device(out=R + 8), "the rays are not .* rows in memory of the context's device, 16-byte aligned"),
        (lambda: rays_device(p=(P, 2), w=256, out=short.data_ptr()), "the rays are not n_probes \\* 6 \\* face_size \\* face_size rows"),
        (lambda: rays_device(p=(R, 5), out=R), "flx_probe_rays_device: the arrays overlap"),
        (lambda: reduce_device(q=None), "flx_probe_reduce_device: the probe params are NULL"),
        (lambda: hip.probe_reduce(np.zeros(8, np.uint32), 1, None), "flx_probe_reduce: the probe params are NULL"),
        (lambda: reduce_device(q=capi.ProbeParams(face_size=0)), "flx_probe_reduce_device: face_size is not one of 1 .. 256"),
        (lambda: reduce_device(q=capi.ProbeParams(face_size=2, order=2)), "flx_probe_reduce_device: order has a bit beyond FLX_TRACE_ORDER_HITS"),
        (lambda: reduce_device(q=capi.ProbeParams(face_size=2, sky=(0, nan, 0))), "flx_probe_reduce_device: sky or reserved holds a value that is not finite"),
        (lambda: reduce_device(q=capi.ProbeParams(face_size=2, reserved=inf)), "sky or reserved holds a value that is not finite"),
        (lambda: reduce_device(n=10923, q=capi.ProbeParams(face_size=256)), "flx_probe_reduce_device: n_probes \\* 6 \\* face_size \\* face_size is 2\\^32 or more"),
        (lambda: reduce_device(r=0), "flx_probe_reduce_device: an array is NULL"),
        (lambda: reduce_device(out=0), "flx_probe_reduce_device: an array is NULL"),
        (lambda: reduce_device(r=host.ctypes.data), "the radiance is not n_probes \\* 6 \\* face_size \\* face_size rows in memory of the context's device"),
        (lambda: reduce_device(n=2, q=capi.ProbeParams(face_size=256), r=short.data_ptr()), "the radiance is not n_probes \\* 6 \\* face_size \\* face_size rows"),
        (lambda: reduce_device(out=S + 8), "the SH rows are not n_probes rows of 144 bytes in memory of the context's device, 16-byte aligned"),
        (lambda: reduce_device(out=host.ctypes.data), "the SH rows are not n_probes rows of 144 bytes"),
        (lambda: reduce_device(out=R + 32), "flx_probe_reduce_device: the arrays overlap"),
        # the whole path: the trace params in the trace call's words, then the probe params, then the arrays
        (lambda: sh_device(tt=None), "flx_rays_trace_ordered: params is NULL"),
        (lambda: sh_device(tt=with_(samples=0)), "flx_rays_trace_ordered: samples is less than 1"),
        (lambda: sh_device(tt=with_(max_reflections=-1)), "max_reflections is negative"),
        (lambda: hip.probes_sh(positions, with_(texture_width=0), good), "texture_width is less than 1"),
        (lambda: sh_device(q=None), "flx_probes_sh_device: the probe params are NULL"),
        (lambda: hip.probes_sh(positions, t, None), "flx_probes_sh: the probe params are NULL"),
        (lambda: sh_device(q=capi.ProbeParams(face_size=300)), "flx_probes_sh_device: face_size is not one of 1 .. 256"),
        (lambda: sh_device(q=capi.ProbeParams(face_size=2, order=4)), "flx_probes_sh_device: order has a bit beyond FLX_TRACE_ORDER_HITS"),
        (lambda: hip.probes_sh(positions, t, capi.ProbeParams(face_size=2, sky=(inf, 0, 0))), "flx_probes_sh: sky or reserved holds a value that is not finite"),
        (lambda: sh_device(q=capi.ProbeParams(face_size=2, reserved=nan)), "flx_probes_sh_device: sky or reserved holds a value that is not finite"),
        (lambda: sh_device(p=(0, 5)), "flx_probes_sh_device: an array is NULL"),
        (lambda: sh_device(out=0), "flx_probes_sh_device: an array is NULL"),
        (lambda: sh_device(p=(positions.ctypes.data, 5)), "the positions are not n_probes rows of 16 bytes in memory of the context's device"),
        (lambda: sh_device(p=(short.data_ptr(), 1400000)), "the positions are not n_probes rows of 16 bytes"),
        (lambda: sh_device(out=S + 4), "the SH rows are not n_probes rows of 144 bytes in memory of the context's device, 16-byte aligned"),
        (lambda: sh_device(p=(S, 5), out=S + 16), "flx_probes_sh_device: the arrays overlap"),
    ]
    for call, words in refused:
        with pytest.raises(capi.FlexLightHipError, match=r"failed \(1\): .*(" + words + ")"):      # FLX_ERR_INVALID
            call()
    hip.sync()
    for buffer in (rows, sh, short):
        assert bool((buffer == 0xA5).all())                        # nothing was written
    assert hip.last_probes() == before                             # ... and nothing traced
    # no probes: FLX_OK and nothing enqueued, the params looked at first
    hip.probes_sh_device((0, 0), t, good, out=0)
    hip.probe_rays_device((0, 0), 2, out=0)
    hip.probe_reduce_device(0, 0, good, out=0)
    with pytest.raises(capi.FlexLightHipError, match="flx_probes_sh_device: face_size is not one of 1 .. 256"):
        hip.probes_sh_device((0, 0), t, capi.ProbeParams(face_size=0), out=0)
    assert hip.last_probes() == before
    with capi.Context(0) as fresh:                                 # the whole path needs a scene, in the trace call's words
        with pytest.raises(capi.FlexLightHipError, match=r"failed \(3\): flx_rays_trace_ordered: no scene and transforms uploaded"):      # FLX_ERR_NO_SCENE
            fresh.probes_sh(positions, t, good)
    # the calls still work
    assert np.isfinite(hip.probes_sh(positions, t, good)).all()
