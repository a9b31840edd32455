"""Shared by test_shape_scenes_host.py, test_gpu_shape_specialised.py and test_gpu_shape_modes.py: the count pairs the shaped trace kernel is
compiled for, the flag word of each (WT_SHAPE_FLAGS of csrc/whitted_params.h, read back with clw_ext_last_trace_flags), and the frame
sizes, depths, factor and threshold at which the twelve scenes of fuzz_scenes.SHAPED_SEEDS are rendered."""
from conftest import CAM
from fuzz_scenes import SHAPED_SEEDS, shaped_scene
from render_common import rendering, take

from flags_common import F_DEEP, F_GEOM_LDS, F_SHAPE, F_SS, F_MOVE, F_LIST, shape_flags      # noqa: F401
V_GENERIC = 8192                        # clw_ext_set_variant: small scenes of the fast build keep the generic kernel
SHAPES = [(ns, npl) for ns in (1, 2, 3, 4) for npl in (0, 1, 2)]          # x 3 lights: the switch of WT_LAUNCH_TRACE (csrc/whitted_launch.inc)
FRAME, RAGGED = (72, 48), (61, 43)      # 9 x 6 whole tiles; the smallest size with a partial tile in both directions next to more than one whole one
DEPTHS = (1, 4)                         # the shaped kernel drops the dead last bounce by depth
ADAPTIVE = (2, 16)                      # factor and contrast threshold of the adaptive cases (the threshold of test_gpu_adaptive.py)


def shape_of(flags):
    return (flags >> 9) & 7, (flags >> 12) & 3, (flags >> 14) & 7


def scene_of(ns, npl):
    """-> (scene, camera, displacement) of the committed seed of this shape"""
    return shaped_scene(ns, npl, SHAPED_SEEDS[ns, npl])


def frame(R, sc, tex, sky, w, h, depth, variant, cam=CAM, strict=False):
    """-> (packed frame, float radiance, flags of the trace launch)"""
    with rendering(R, sc, tex, sky, w, h, setup=lambda wrap: wrap.set_variant(variant), cam=cam, depth=depth, strict=strict) as r:
        return (*take(r)[0], r.w.last_trace_flags())


def empty_list_scenes(demo_scene):
    """render.map without its spheres, its planes, its lights, and without all three"""
    from example_gui_opencl_raytracer_amd.scene import Scene
    return {
        "no spheres": Scene(demo_scene.spheres[:0], demo_scene.planes, demo_scene.lights),
        "no planes": Scene(demo_scene.spheres, demo_scene.planes[:0], demo_scene.lights),
        "no lights": Scene(demo_scene.spheres, demo_scene.planes, demo_scene.lights[:0]),
        "sky only": Scene(demo_scene.spheres[:0], demo_scene.planes[:0], demo_scene.lights[:0]),
    }
