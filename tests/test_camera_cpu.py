"""Cameras without a GPU (include/flexlight_hip_debug.h, "cameras"; include/flx_camera.h): the CPU reference the GPU tests compare against is itself held against
the oracle's primary rays (the pinhole, bit for bit) and against float64 restatements of the header's formulas (the other four projections, within a bound worked
out from the number format); the exact properties the header promises hold; the calls are declared, exported and bound; and the argument rules that need no device
(csrc/flx_camera_args.h) hold in a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from camera_util import JITTER, POSITION, SIZES, assert_same_rows, cameras_of, expected64, reference, rotated_basis, skewed_basis
from rays_trace_util import FRAMES, camera_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("flx_camera_rays_device", "flx_camera_rays", "flx_camera_image_device", "flx_camera_image", "flx_camera_image_temporal_device", "flx_camera_image_temporal")
ARGS_CASES = 141        # the cases tests/camera_args_main.cc runs
BOUND = 2.0 ** -18      # fewer than 64 roundings of relative 2^-24 on magnitudes <= 1


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return reference(tmp_path_factory)


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_the_pinhole_is_the_oracles_primary_ray(oracle, scenes, ref, name):
    """origin, direction and both noise words of every pixel equal flx_oracle_primary's, which shares no code with include/flx_camera.h"""
    from flexlight_hip import capi
    sc, p, rays, _, _ = camera_rays(oracle, scenes, name)
    w, h = FRAMES[name][0], FRAMES[name][1]
    assert_same_rows(ref.rays(capi.Camera.pinhole(p), w, h), rays, "the pinhole of %s" % name)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_other_projections_against_float64(ref, size):
    from flexlight_hip import capi
    w, h = size
    worst = {}
    for name, cam in cameras_of(capi, rotated_basis()).items():
        got = ref.rays(cam, w, h).astype(np.float64)
        origin, direction, noise = expected64(cam, w, h)
        scale = max(1.0, float(np.abs(origin).max()))                      # an orthographic origin: the bound scaled by the largest |coordinate|
        worst[name] = (float(np.abs(got[:, 4:7] - direction).max()), float(np.abs(got[:, 0:3] - origin).max()) / scale, float(np.abs(got[:, (3, 7)] - noise).max()))
    say = ", ".join("%s %.2f / %.2f / %.2f" % (k, v[0] * 2.0 ** 24, v[1] * 2.0 ** 24, v[2] * 2.0 ** 24) for k, v in worst.items())
    assert all(max(v) <= BOUND for v in worst.values()), "%d x %d, worst direction / origin / noise error in units of 2^-24 (the bound: 64): %s" % (w, h, say)
    print("%d x %d, worst direction / origin / noise error in units of 2^-24: %s" % (w, h, say))


def test_edge_samples(ref):
    """jitter +0.5 at the last pixel gives exactly 1, jitter -0.5 at the first exactly -1: an orthographic window of 2 x 2 units around the origin in the identity basis
    shows sx and sy as the origin's x and y"""
    from flexlight_hip import capi
    for w, h in SIZES + ((1, 1),):
        hi = ref.rays(capi.Camera.orthographic((0, 0, 0), width=2.0, height=2.0, jitter=(0.5, 0.5)), w, h).reshape(h, w, 8)
        lo = ref.rays(capi.Camera.orthographic((0, 0, 0), width=2.0, height=2.0, jitter=(-0.5, -0.5)), w, h).reshape(h, w, 8)
        assert (hi[:, w - 1, 0] == 1.0).all() and (hi[0, :, 1] == 1.0).all()            # row 0 is the top: py = h - 1
        assert (lo[:, 0, 0] == -1.0).all() and (lo[h - 1, :, 1] == -1.0).all()
        assert (hi[:, :, 4:7] == np.array([0, 0, 1], np.float32)).all()


def test_cube_seams(ref):
    """the right edge of face 4 is the left edge of face 0 and the top edge of face 4 the bottom edge of face 2, bit for bit, for a basis that is no rotation"""
    from flexlight_hip import capi
    basis, w, h = skewed_basis(), 9, 9
    face = lambda f, jitter: ref.rays(capi.Camera.cube_face(POSITION, f, basis, jitter=jitter), w, h).reshape(h, w, 8)
    bits = lambda rows: np.ascontiguousarray(rows[:, 4:7]).view(np.uint32)
    right_of_4, left_of_0 = face(4, (0.5, 0.2))[:, w - 1], face(0, (-0.5, 0.2))[:, 0]
    assert np.array_equal(bits(right_of_4), bits(left_of_0))
    top_of_4, bottom_of_2 = face(4, (-0.1, 0.5))[0], face(2, (-0.1, -0.5))[h - 1]
    assert np.array_equal(bits(top_of_4), bits(bottom_of_2))
    assert not np.array_equal(bits(face(4, (0.5, 0.2))[:, 0]), bits(left_of_0))      # (the comparison compares something)


def test_regions_are_the_whole_images_rows(ref):
    from flexlight_hip import capi
    w, h = 33, 31
    cams = list(cameras_of(capi, skewed_basis()).values())
    whole = ref.rays(cams, w, h).reshape(len(cams), h, w, 8)
    for x0, y0, rw, rh in ((5, 7, 13, 9), (0, 0, 33, 31), (32, 30, 1, 1), (0, 29, 33, 2), (31, 0, 2, 31)):
        part = ref.rays(cams, w, h, region=(x0, y0, rw, rh)).reshape(len(cams), rh, rw, 8)
        assert np.array_equal(part.view(np.uint32), whole[:, y0:y0 + rh, x0:x0 + rw].view(np.uint32)), (x0, y0, rw, rh)


def test_noise_words_do_not_change_with_jitter(ref):
    from flexlight_hip import capi
    w, h = 65, 3
    still = ref.rays(list(cameras_of(capi, rotated_basis(), jitter=(0.0, 0.0)).values()), w, h)
    moved = ref.rays(list(cameras_of(capi, rotated_basis(), jitter=JITTER).values()), w, h)
    assert np.array_equal(still[:, (3, 7)].view(np.uint32), moved[:, (3, 7)].view(np.uint32))
    assert not np.array_equal(still[:, 4:7], moved[:, 4:7])
    one, half, two = np.float32(1.0), np.float32(0.5), np.float32(2.0)
    px, py = np.arange(w, dtype=np.float32), (h - 1 - np.arange(h)).astype(np.float32)
    first = still[:w * h].reshape(h, w, 8)
    assert np.array_equal(first[0, :, 3], (px + half) / np.float32(w) * two - one) and np.array_equal(first[:, 0, 7], (py + half) / np.float32(h) * two - one)


def test_fisheye_centre(ref):
    """q == 0 at the centre pixel of an odd image without jitter: the direction is normalize3(forward), which is the orthographic camera's"""
    from flexlight_hip import capi
    basis, w, h = skewed_basis(), 7, 5
    eye = ref.rays(capi.Camera.fisheye(POSITION, basis, fov=3.0), w, h).reshape(h, w, 8)
    flat = ref.rays(capi.Camera.orthographic(POSITION, basis), w, h).reshape(h, w, 8)
    assert eye[h // 2, w // 2, 3] == 0.0 and eye[h // 2, w // 2, 7] == 0.0
    assert np.array_equal(eye[h // 2, w // 2, 4:7].view(np.uint32), flat[0, 0, 4:7].view(np.uint32))
    assert np.isfinite(eye).all() and not np.array_equal(eye[0, 0, 4:7], flat[0, 0, 4:7])


def test_the_calls_are_declared_exported_and_bound():
    from flexlight_hip import capi
    header = open(os.path.join(ROOT, "include", "flexlight_hip_debug.h")).read()
    public = open(os.path.join(ROOT, "include", "flexlight_hip.h")).read()
    for name in CALLS:
        assert name in capi.EXPORTS and hasattr(capi.LIB, name) and name + "(" in header and name not in public, name
    for k, name in enumerate(("PINHOLE", "PANORAMA", "FISHEYE", "ORTHOGRAPHIC", "CUBE_FACE")):
        assert "#define FLX_CAMERA_%s" % name in header and getattr(capi, "CAMERA_" + name) == k
    for method in ("camera_rays", "camera_rays_device", "camera_image", "camera_image_device", "camera_image_temporal", "camera_image_temporal_device"):
        assert callable(getattr(capi.Context, method))


def test_the_camera_structure_matches_the_c_compiler(tmp_path):
    from flexlight_hip import capi
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stdio.h>
#include <stddef.h>
#include "flexlight_hip_debug.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(flx_camera), offsetof(flx_camera, projection), offsetof(flx_camera, face), offsetof(flx_camera, position),
         offsetof(flx_camera, basis), offsetof(flx_camera, extent), offsetof(flx_camera, jitter));
  return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)]).decode().split()))
    cam = capi.Camera
    assert got == [C.sizeof(cam), cam.projection.offset, cam.face.offset, cam.position.offset, cam.basis.offset, cam.extent.offset, cam.jitter.offset]


def test_the_constructors(scenes):
    from flexlight_hip import capi
    p = scenes("cornell").frame_params(width=32, height=24, samples=1, max_reflections=1, use_filter=0)
    c = capi.Camera.pinhole(p, jitter=(0.25, -0.25))
    assert c.projection == capi.CAMERA_PINHOLE and list(c.position) == list(p.camera) and list(c.basis) == list(p.view_matrix) and list(c.jitter) == [0.25, -0.25]
    c = capi.Camera.panorama((1, 2, 3))
    assert c.projection == capi.CAMERA_PANORAMA and list(c.extent) == [np.float32(2 * np.pi), np.float32(np.pi)] and list(c.basis) == list(capi.IDENTITY_BASIS)
    c = capi.Camera.fisheye((1, 2, 3), fov=2.0)
    assert c.projection == capi.CAMERA_FISHEYE and list(c.extent) == [2.0, 0.0]
    c = capi.Camera.orthographic((1, 2, 3), width=4.0, height=3.0)
    assert c.projection == capi.CAMERA_ORTHOGRAPHIC and list(c.extent) == [4.0, 3.0] and list(c.position) == [1.0, 2.0, 3.0]
    c = capi.Camera.cube_face((0, 0, 0), 5, skewed_basis())
    assert c.projection == capi.CAMERA_CUBE_FACE and c.face == 5 and np.array_equal(np.array(list(c.basis), np.float32), skewed_basis())
    ctx = capi.Context.__new__(capi.Context)      # no device: the checks made before the library is asked
    ctx._h, ctx._device = None, 0
    with pytest.raises(TypeError, match="camera_rays: cameras is a Camera or a sequence of them"):
        ctx.camera_rays([1, 2], 4, 4)
    with pytest.raises(TypeError, match="camera_image: camera is a Camera"):
        ctx.camera_image(p, 4, 4, capi.TraceParams())


def test_argument_rules_in_a_stand_alone_program_under_the_sanitizers(tmp_path):
    """every refusal of flx_camera_args.h, the 2^32 product, a region touching each border and the address wraps: the header with a main of its own, built with
    -fsanitize=address,undefined, run directly"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is part of the image (the oracle is built with gcc)"
    exe = tmp_path / "camera_args"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "web-ray-tracer_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "camera_args_main.cc"), "-o", str(exe)])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) == ARGS_CASES
