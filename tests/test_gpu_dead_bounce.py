"""The trimmed trace loop: on a path's last level (depth + 1 >= MAX_DEPTH) the Fresnel / reflection block is skipped -- no child can be
pushed there and whitted_pop.inc overwrites or retires everything the block would compute (csrc/whitted_bounce.inc) -- and the tile cost
is reduced over the wave by DPP row operations instead of the shuffle butterfly (wt_wave_reduce in csrc/whitted_trace.inc).  Variant
16384 runs the kernel the old way (a wave-uniform launch parameter, same kernels), so both run in one process: the packed frame, the float
radiance, the per-tile costs and the work counters must be equal, bit for bit, in every flavour of the kernel."""
import numpy as np
import pytest

from conftest import CAM
from flags_common import F_COUNT, F_DEEP, F_GEOM_LDS, F_GRID, F_SHAPE
from render_common import R, rendering  # noqa: F401  (R: the fixture)
from shape_common import frame

pytestmark = pytest.mark.gpu

V_GENERIC, V_UNTRIMMED = 8192, 16384
GLASS_CAM = dict(origin=(3.5, 3.0, -6.0), look=(0.0, -2.5, 9.5), fov=90.0, focal=1.0)
GRID_CAM = dict(origin=(0.0, 12.0, -10.0), look=(0.0, -0.45, 1.0), fov=90.0, focal=1.0)
# Fuzz seed 11 is left out, as tests/test_gpu_parity.py::test_random_scenes_against_the_oracle leaves it out: the scene hits an undefined
# float -> int conversion / image read in the reference, so there is no defined frame to hold either variant to.  Every other seed runs.
FUZZ_SKIPPED = (11,)
FUZZ_SEEDS = [s for s in range(40) if s not in FUZZ_SKIPPED]


def check_pair(R, sc, tex, sky, w, h, depth, cam=CAM, strict=False, base=0):
    """variant `base` (trimmed) against `base | 16384` (untrimmed): same kernel, same bits.  -> the launch's flags"""
    old, old_rgb, oflags = frame(R, sc, tex, sky, w, h, depth, base | V_UNTRIMMED, cam, strict)
    new, new_rgb, flags = frame(R, sc, tex, sky, w, h, depth, base, cam, strict)
    assert flags == oflags, (flags, oflags)          # the bit is a launch parameter: it must not pick another kernel
    assert np.array_equal(new, old)
    assert np.array_equal(new_rgb.view(np.uint32), old_rgb.view(np.uint32))     # the un-clamped radiance too, bit for bit
    return flags


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5, 8])
def test_render_map(R, demo_scene, tex, sky, depth, strict):
    """render.map at shallow and deep depths, fast and strict build; the fast build's shallow launches in the shaped and the generic kernel."""
    flags = check_pair(R, demo_scene, tex, sky, 640, 360, depth, strict=strict)
    assert bool(flags & F_DEEP) == (depth > 4)
    assert bool(flags & F_SHAPE) == (not strict and depth <= 4)
    if flags & F_SHAPE:
        gflags = check_pair(R, demo_scene, tex, sky, 640, 360, depth, strict=strict, base=V_GENERIC)
        assert not gflags & F_SHAPE and gflags & F_GEOM_LDS


@pytest.mark.parametrize("base", [0, V_GENERIC])
def test_render_map_c2(R, demo_scene, tex, sky, base):
    """Config C2's frame: 1920x1080, depth 4, the raypng camera."""
    from example_gui_opencl_raytracer_amd import CAMERA_RAYPNG
    flags = check_pair(R, demo_scene, tex, sky, 1920, 1080, 4, CAMERA_RAYPNG, base=base)
    assert bool(flags & F_SHAPE) == (base == 0)


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_scenes(R, tex, sky, seed):
    """The scenes of tests/fuzz_scenes.py at their own depth (1-15) and at depths 1 and 4, fast and strict, shaped (where the scene's counts
    are in the compiled set) and generic."""
    from fuzz_scenes import random_scene
    sc, cam, depth = random_scene(seed)
    for strict in (False, True):
        for d in sorted({1, 4, depth}):
            flags = check_pair(R, sc, tex, sky, 96, 64, d, cam, strict=strict)
            if flags & F_SHAPE:
                check_pair(R, sc, tex, sky, 96, 64, d, cam, strict=strict, base=V_GENERIC)


def test_fuzz_scenes_skip_one_seed_at_most():
    assert len(FUZZ_SKIPPED) <= 1 and len(FUZZ_SEEDS) == 40 - len(FUZZ_SKIPPED)


@pytest.mark.parametrize("strict", [False, True])
def test_glass_field_depth_8(R, tex, sky, strict):
    """The deep flavours: the glass field at depth 8 with the tree-parallel tail (whose own bounce is untouched), without it (variant 16:
    the per-lane loop runs every refraction tree to the end) and in the low-occupancy flavour (variant 64)."""
    from example_gui_opencl_raytracer_amd import scene
    sc = scene.dielectric_field_scene(8)
    for base in (0, 16, 64):
        flags = check_pair(R, sc, tex, sky, 256, 192, 8, GLASS_CAM, strict=strict, base=base)
        assert flags & F_DEEP


@pytest.mark.parametrize("strict", [False, True])
def test_grid_scene(R, tex, sky, strict):
    """C4's scene (10 000 spheres through the uniform grid) on a small frame."""
    from example_gui_opencl_raytracer_amd import scene
    flags = check_pair(R, scene.sphere_grid_scene(100, 100), tex, sky, 320, 180, 4, GRID_CAM, strict=strict)
    assert flags & F_GRID


def _costs(R, sc, tex, sky, w, h, depth, variant, cam, frames=3):
    """The per-tile cost buffer after `frames` frames (the later ones dispatched in the order the earlier ones' costs gave), read back as
    tools/tile_costs.py reads it."""
    with rendering(R, sc, tex, sky, w, h, setup=lambda wrap: wrap.set_variant(variant), cam=cam, depth=depth) as r:
        for _ in range(frames):
            r.render(readback=False)
        r.w.sync()
        return r.w.read_tile_costs().copy(), r.w.last_trace_flags()


@pytest.mark.parametrize("base", [0, V_GENERIC])
def test_tile_costs_are_equal(R, demo_scene, tex, sky, base):
    """render.map depth 4 (a tile reports the maximum over its lanes): the costs wt_sched_build sorts by are the same numbers."""
    from example_gui_opencl_raytracer_amd import CAMERA_RAYPNG
    w, h = 1920, 1080
    new, flags = _costs(R, demo_scene, tex, sky, w, h, 4, base, CAMERA_RAYPNG)
    old, oflags = _costs(R, demo_scene, tex, sky, w, h, 4, base | V_UNTRIMMED, CAMERA_RAYPNG)
    assert flags == oflags and bool(flags & F_SHAPE) == (base == 0)
    assert new.size == ((w + 7) // 8) * ((h + 7) // 8) and new.max() > new.min() > 0
    assert np.array_equal(new, old)


def test_tile_costs_are_equal_on_a_deep_launch(R, tex, sky):
    """The glass field at depth 8.  With the tail on a tile's cost is the SUM over its lanes, added up over the wavefronts that share the
    tile (the other form of the reduction); without it (variant 16) the maximum over the lanes of a per-lane loop that runs to the end."""
    from example_gui_opencl_raytracer_amd import scene
    sc = scene.dielectric_field_scene(8)
    for base in (0, 16):
        new, flags = _costs(R, sc, tex, sky, 256, 192, 8, base, GLASS_CAM, frames=1)
        old, oflags = _costs(R, sc, tex, sky, 256, 192, 8, base | V_UNTRIMMED, GLASS_CAM, frames=1)
        assert flags == oflags and flags & F_DEEP
        assert new.max() > 0
        assert np.array_equal(new, old), base


WORK_KEYS = ("segments", "shadow_rays", "light_probes", "sky_fetches", "texel_fetches", "pushes", "shadow_rays_traced")
LOOP_KEYS = WORK_KEYS + ("lane_iters", "wave_iters_x64", "lights_classified", "vis_mismatches")


def _counted(R, sc, tex, sky, w, h, depth, variant, cam, strict):
    with rendering(R, sc, tex, sky, w, h, setup=lambda wrap: wrap.set_variant(variant), cam=cam, depth=depth, strict=strict) as r:
        r.w.enable_counters(1)
        img = r.render()
        c = r.w.read_counters()
        assert r.w.last_trace_flags() & F_COUNT
        return img, c


@pytest.mark.parametrize("strict", [False, True])
def test_counters_are_equal(R, demo_scene, tex, sky, strict):
    """A counting run's counters: nothing is pushed on the level whose bounce is skipped, so `pushes` cannot move; neither may anything else.
    Shallow launches and the deep per-lane loop (variant 16) compare every counter of the loop; with the tail on, the work counters are
    compared (as test_tree_parallel_tail_equals_the_per_lane_loop does)."""
    from example_gui_opencl_raytracer_amd import scene
    glass = scene.dielectric_field_scene(8)
    for sc, w, h, depth, cam, base, keys in ((demo_scene, 640, 360, 4, CAM, 0, LOOP_KEYS), (demo_scene, 640, 360, 1, CAM, 0, LOOP_KEYS),
                                             (demo_scene, 320, 200, 8, CAM, 16, LOOP_KEYS), (glass, 256, 192, 8, GLASS_CAM, 16, LOOP_KEYS),
                                             (glass, 256, 192, 8, GLASS_CAM, 0, WORK_KEYS)):
        new, cn = _counted(R, sc, tex, sky, w, h, depth, base, cam, strict)
        old, co = _counted(R, sc, tex, sky, w, h, depth, base | V_UNTRIMMED, cam, strict)
        assert np.array_equal(new, old)
        assert cn["segments"] > 0 and (depth == 1 or cn["pushes"] > 0)
        assert {k: cn[k] for k in keys} == {k: co[k] for k in keys}, (depth, base)
