"""Traced ray batches without a GPU: the CPU reference (tests/rays_trace_ref) is held against the oracle's own frames on a camera's rays — words 0..3 of a row are
the frame's pixel bit for bit, the rows' bounce iterations add up to the frame's `shades` counter —; the calls are declared, exported and bound; the helpers of
capi read and make what the header lays out; and the argument checks that need no device (csrc/flx_query_args.h) hold in a stand-alone program under the address
and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from rays_trace_util import FRAMES, camera_rays, free_rays, reference, trace_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("flx_rays_trace_device", "flx_rays_trace", "flx_debug_set_trace_slab", "flx_debug_last_trace")


@pytest.fixture(scope="module")
def ref(tmp_path_factory, oracle):
    return reference(tmp_path_factory)


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_the_reference_on_a_cameras_rays_is_the_oracles_frame(oracle, scenes, ref, name):
    sc, p, rays, compares, first = camera_rays(oracle, scenes, name)
    w, h, samples, bounces, must = FRAMES[name]
    print("%s: %d of %d pixels compare, %d hits" % (name, compares.sum(), compares.size, (first[:, 4] != -1).sum()))
    assert compares.sum() >= must and compares.size == w * h                  # the condition on the inputs
    frame, counters, _ = oracle.render(sc, p)
    rows = ref.trace(sc, trace_params(p), rays)
    pixels = np.ascontiguousarray(frame, np.float32).reshape(-1, 4).view(np.uint32)
    differ = np.flatnonzero((rows[:, 0:4] != pixels).any(axis=1) & compares)
    assert differ.size == 0, (name, differ[:8], rows[differ[:1], 0:4], pixels[differ[:1]])
    hit = rows[:, 5].view(np.int32) != -1
    assert np.array_equal(hit, first[:, 4] != -1) and np.array_equal(rows[hit, 5].view(np.int32), first[hit, 4].astype(np.int32))
    assert np.array_equal(rows[hit, 6].view(np.int32), first[hit, 3].astype(np.int32)) and np.array_equal(rows[hit, 4].view(np.float32), first[hit, 0].astype(np.float32))
    assert (rows[~hit] == np.array([0, 0, 0, 0, 0, 0xffffffff, 0, 0], np.uint32)).all()      # a miss row: zeros, entry -1
    assert (rows[hit, 3].view(np.float32) == 1.0).all() and (rows[hit, 7] >= samples).all() and (rows[hit, 7] <= samples * bounces).all()
    if compares.all():
        assert int(rows[:, 7].sum()) == counters["shades"]


@pytest.mark.parametrize("name", ["dragon", "theater"])
def test_the_free_rays_meet_their_conditions(oracle, scenes, ref, name):
    """what test_rays_trace_gpu.py asks of the rays no camera makes, asserted on the reference's rows"""
    sc, p, _, _, _ = camera_rays(oracle, scenes, name)
    rows = ref.trace(sc, trace_params(p), free_rays(oracle, scenes, name))
    hit = rows[:, 5].view(np.int32) != -1
    deep = rows[:, 7] > p.samples                                             # more bounce iterations than samples: some sample shaded two or more
    print("%s: %.3f hit, %.3f miss, %.3f shade two or more bounces in some sample" % (name, hit.mean(), 1 - hit.mean(), deep.mean()))
    assert hit.mean() >= 0.30 and (~hit).mean() >= 0.05 and deep.mean() >= 0.10


def test_the_loop_guard_cases_of_the_reference(oracle, scenes, ref):
    sc, p, rays, _, first = camera_rays(oracle, scenes, "cornell")
    from flexlight_hip import capi
    hit = first[:, 4] != -1
    ambient = np.array(p.ambient[:], np.float32).view(np.uint32)
    for kw in (dict(max_reflections=0), dict(min_importancy=2.0)):
        t = capi.TraceParams.of_frame(p)
        for k, v in kw.items():
            setattr(t, k, v)
        rows = ref.trace(sc, t, rays)
        assert (rows[hit, 0:3] == ambient).all() and (rows[hit, 7] == 0).all() and (rows[hit, 3].view(np.float32) == 1.0).all(), kw
        assert (rows[~hit, 0:5] == 0).all()


def test_the_calls_are_declared_exported_and_bound():
    from flexlight_hip import capi
    from test_capi_cpu import declared_functions
    debug, boundary = declared_functions(headers=("flexlight_hip_debug.h",)), declared_functions(headers=("flexlight_hip.h",))
    for name in CALLS:
        assert name in debug and name not in boundary, name          # in the instrumentation header: the boundary keeps its size
        assert name in capi.EXPORTS and hasattr(capi.LIB, name), name
        assert getattr(capi.LIB, name).argtypes is not None, name
    text = open(os.path.join(ROOT, "include", "flexlight_hip_debug.h")).read()
    struct = text.split("typedef struct flx_trace_params {")[1].split("}")[0]
    assert [f.strip() for f in struct.replace("\n", " ").split(";") if f.strip()] == [
        "int32_t samples, max_reflections", "float min_importancy", "float ambient[3]", "float random_seed", "int32_t texture_width"]
    import ctypes as C
    assert C.sizeof(capi.TraceParams) == 32 and [f[0] for f in capi.TraceParams._fields_] == ["samples", "max_reflections", "min_importancy", "ambient", "random_seed", "texture_width"]
    t = capi.TraceParams(samples=3, max_reflections=7, min_importancy=0.25, ambient=(0.5, 0.25, 0.125), random_seed=2.0, texture_width=64)
    assert (t.samples, t.max_reflections, t.min_importancy, tuple(t.ambient), t.random_seed, t.texture_width) == (3, 7, 0.25, (0.5, 0.25, 0.125), 2.0, 64)
    args = open(os.path.join(ROOT, "web-ray-tracer_amd", "csrc", "flx_query_args.h")).read()
    assert "flx_trace_args_check" in args and "flx_query_args_check" in args


def test_unpack_radiance_reads_a_hand_packed_buffer():
    from flexlight_hip import capi
    words = np.zeros((3, 8), np.uint32)
    words[0, 0:5] = np.array([1.5, 0.25, 3.0e9, 1.0, 7.75], np.float32).view(np.uint32)
    words[0, 5:8] = [123456789, 6, 0xfffffff0]
    words[1, 5] = 0xffffffff                                           # a miss row
    words[2, 0] = 0xffc12345                                           # a NaN with a sign and a payload: its bits come back
    words[2, 3:8] = [np.array([1.0], np.float32).view(np.uint32)[0], 0, 0, 2 ** 20, 17]
    buf = words.view(np.uint8).reshape(3, 32)
    import torch
    for source in (buf, buf.reshape(-1), torch.from_numpy(buf.copy())):
        got = capi.unpack_radiance(source)
        assert sorted(got) == ["alpha", "entry", "rgb", "s", "shades", "transform2"]
        assert got["rgb"].dtype == np.float32 and got["rgb"].shape == (3, 3) and np.array_equal(got["rgb"].view(np.uint32), words[:, 0:3])
        assert got["alpha"].tolist() == [1.0, 0.0, 1.0] and got["s"].tolist() == [7.75, 0.0, 0.0]
        assert got["entry"].dtype == np.int32 and got["entry"].tolist() == [123456789, -1, 0]
        assert got["transform2"].dtype == np.int32 and got["transform2"].tolist() == [6, 0, 2 ** 20]
        assert got["shades"].dtype == np.uint32 and got["shades"].tolist() == [0xfffffff0, 0, 17]
    assert capi.unpack_radiance(np.zeros((0, 32), np.uint8))["rgb"].shape == (0, 3)


def test_noise_coordinates_are_spread_and_all_different():
    from flexlight_hip import capi
    for n in (0, 1, 2, 63, 64, 65, 2160, 100000):
        xy = capi.noise_coordinates(n)
        assert xy.shape == (n, 2) and xy.dtype == np.float32
        assert ((xy >= -1.0) & (xy < 1.0)).all()
        assert len(set(map(tuple, xy.tolist()))) == n
    xy = capi.noise_coordinates(2160)
    assert abs(xy.mean()) < 0.05 and xy[:, 0].min() < -0.9 and xy[:, 0].max() > 0.9 and xy[:, 1].min() < -0.9 and xy[:, 1].max() > 0.9
    # a 4 x 4 batch has a 4 x 4 frame's pixel centres, as primary_hit computes them
    centres = ((np.arange(4, dtype=np.float32) + np.float32(0.5)) / np.float32(4) * np.float32(2) - np.float32(1)).tolist()
    assert capi.noise_coordinates(16)[:, 0].tolist() == centres * 4 and capi.noise_coordinates(16)[::4, 1].tolist() == centres


def test_trace_rays_device_refuses_a_bad_tensor_before_any_library_call(monkeypatch):
    import torch
    from flexlight_hip import capi

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError("the library was called: %s" % name)

    ctx = capi.Context.__new__(capi.Context)                                  # no flx_context_create: nothing below may need one
    ctx._h, ctx._device = None, 0
    monkeypatch.setattr(capi, "LIB", NoLibrary())
    params = capi.TraceParams()
    good = torch.zeros((16, 8), dtype=torch.float32)
    with pytest.raises(ValueError, match="trace_rays_device: rays is on cpu"):
        ctx.trace_rays_device(good, params)
    with pytest.raises(ValueError, match="trace_rays_device: rays is a contiguous float32 tensor"):
        ctx.trace_rays_device(good.double(), params)
    with pytest.raises(ValueError, match="contiguous float32 tensor"):
        ctx.trace_rays_device(torch.zeros((16, 7), dtype=torch.float32), params)
    with pytest.raises(TypeError, match="torch tensor or"):
        ctx.trace_rays_device(np.zeros((16, 8), np.float32), params)
    with pytest.raises(TypeError, match="params is a TraceParams"):
        ctx.trace_rays_device((4096, 16), {"samples": 1})
    ctx._h = None


def test_argument_checks_in_a_stand_alone_program_under_the_sanitizers(tmp_path):
    """every refusal and the accepting cases at the edges (an array that ends at the top of the address space, arrays that touch), and the slab rule:
    flx_trace_args_check and flx_trace_slab_rays with a main of their own, built with -fsanitize=address,undefined, run directly"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is part of the image (the oracle is built with gcc)"
    exe = tmp_path / "rays_trace_args"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "web-ray-tracer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "rays_trace_args_main.cc"), "-o", str(exe)])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) >= 90
