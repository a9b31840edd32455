"""The shaped trace kernel: small LDS-geometry scenes of the shallow fast build run a kernel with the scene's sphere, plane and light
counts compiled in (wt_shape in csrc/whitted_trace.inc).  It must give the generic kernel's frame bit for bit, and every other scene must keep
the generic kernel.  This module holds the bench-sized frames and the scenes just outside the compiled set; every compiled count pair, in every
sampling mode, is swept by tests/test_gpu_shape_modes.py.  Variant 8192 forces the generic kernel, so both run in one process.
(The strict build has no shaped flavour: its small scenes always take the generic kernel, checked below.)"""
import numpy as np
import pytest

from conftest import CAM
from render_common import R  # noqa: F401  (the fixture)
from shape_common import F_DEEP, F_GEOM_LDS, F_SHAPE, V_GENERIC, frame, shape_of

pytestmark = pytest.mark.gpu


def check_pair(R, sc, tex, sky, w, h, depth, cam=CAM, shaped=True):
    gen, gen_rgb, gflags = frame(R, sc, tex, sky, w, h, depth, V_GENERIC, cam)
    out, rgb, flags = frame(R, sc, tex, sky, w, h, depth, 0, cam)
    assert not gflags & F_SHAPE
    if shaped:
        assert flags & F_SHAPE and flags & F_GEOM_LDS, flags
        assert shape_of(flags) == sc.counts
    else:
        assert not flags & F_SHAPE, flags
    assert np.array_equal(out, gen)
    assert np.array_equal(rgb.view(np.uint32), gen_rgb.view(np.uint32))     # the un-clamped radiance too, bit for bit


def test_render_map_c2(R, demo_scene, tex, sky):
    """Config C2's frame: 1920x1080, depth 4, the raypng camera."""
    from example_gui_opencl_raytracer_amd import CAMERA_RAYPNG
    check_pair(R, demo_scene, tex, sky, 1920, 1080, 4, CAMERA_RAYPNG)


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_render_map_720p(R, demo_scene, tex, sky, depth):
    check_pair(R, demo_scene, tex, sky, 1280, 720, depth)


def test_deep_launch_keeps_generic_kernel(R, demo_scene, tex, sky):
    _, _, flags = frame(R, demo_scene, tex, sky, 160, 120, 5, 0)
    assert flags & F_DEEP and not flags & F_SHAPE


def test_strict_build_keeps_generic_kernel(R, demo_scene, tex, sky):
    _, _, flags = frame(R, demo_scene, tex, sky, 160, 120, 4, 0, strict=True)
    assert flags == F_GEOM_LDS


def _variants(sc):
    """render.map with its counts moved inside and just outside the compiled set"""
    from example_gui_opencl_raytracer_amd.scene import Scene
    s, p, l = sc.spheres, sc.planes, sc.lights
    inside = {"1 sphere": Scene(s[:1], p, l), "2 spheres": Scene(s[:2], p, l), "3 spheres": Scene(s[1:], p, l),
              "1 plane": Scene(s, p[1:], l), "no planes": Scene(s, p[:0], l), "3 spheres 1 plane": Scene(s[:3], p[:1], l),
              "1 sphere 1 plane": Scene(s[2:3], p[:1], l), "2 spheres no planes": Scene(s[1:3], p[:0], l), "2 spheres 1 plane": Scene(s[2:], p[1:], l),
              "3 spheres no planes": Scene(s[:3], p[:0], l)}
    s5 = np.concatenate([s, s[:1]])
    s5[4]["origin"] = (-3.0, 0.6, 2.0)
    l4 = np.concatenate([l, l[:1]])
    l4[3]["origin"] = (2.0, 4.0, 1.0)
    p3 = np.concatenate([p, p[:1]])
    p3[2]["normal"] = (1.0, 0.0, 0.0)
    p3[2]["point_in_plane"] = (-6.0, 0.0, 0.0)
    outside = {"5 spheres": Scene(s5, p, l), "3 planes": Scene(s, p3, l), "2 lights": Scene(s, p, l[:2]),
               "4 lights": Scene(s, p, l4), "no spheres": Scene(s[:0], p, l)}
    return inside, outside


@pytest.mark.parametrize("depth", [1, 4])
def test_render_map_shapes(R, demo_scene, tex, sky, depth):
    inside, outside = _variants(demo_scene)
    for name, sc in inside.items():
        check_pair(R, sc, tex, sky, 256, 192, depth, shaped=True)
    for name, sc in outside.items():
        check_pair(R, sc, tex, sky, 256, 192, depth, shaped=False)


# tests/fuzz_scenes.py seeds: (spheres, planes, lights) inside the compiled set, and just outside it
FUZZ_INSIDE = [1, 11, 24, 37]            # (4, 2, 3), (1, 0, 3), (3, 1, 3), (1, 2, 3)
FUZZ_OUTSIDE = [14, 16, 43, 42, 7]       # (1, 3, 3), (4, 2, 4), (4, 2, 2), (0, 3, 3), (8, 2, 3)


@pytest.mark.parametrize("seed", FUZZ_INSIDE + FUZZ_OUTSIDE)
def test_fuzz_scenes(R, tex, sky, seed):
    from fuzz_scenes import random_scene
    sc, cam, depth = random_scene(seed)
    for d in sorted({1, min(depth, 4), 4}):
        check_pair(R, sc, tex, sky, 96, 64, d, cam, shaped=seed in FUZZ_INSIDE)
