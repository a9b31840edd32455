"""Shared by test_sphere_motion_host.py and test_gpu_sphere_motion.py: the displacements the tests use and the numpy side of the definition of
moving spheres.

With factor n, a displacement table disp[spheres, 3] and sample times t[0 .. n*n), the sample at virtual pixel (vx, vy) is pixel (vx, vy) of
the 1-sample render of the n*W x n*H frame of the scene S(t[(vy mod n) * n + (vx mod n)]), whose sphere i has centre fma(t, disp[i], c[i])
(api.spheres_at = clw_host_spheres_at); clamp, add and scale as plain supersampling (sample_cameras_common.resolve)."""
import numpy as np

# the demo scene (scene.render_map_scene): sphere 0 (red plastic) and 3 (green glass) stand still, 1 (blue plastic, opaque) and 2 (glass) move
# by a few tenths of a unit while the shutter is open
DISP = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, -0.3], [-0.4, 0.2, 0.0], [0.0, 0.0, 0.0]], np.float32)


def field_disp(count):
    """a displacement for scene.dielectric_field_scene: every third sphere moves, the others stand still"""
    d = np.zeros((count, 3), np.float32)
    d[0::3] = (0.25, 0.1, 0.0)
    d[1::6] = (0.0, 0.0, -0.3)
    return d


def moved_scene(api, sc, disp, t):
    """the scene S(t)"""
    from example_gui_opencl_raytracer_amd.scene import Scene
    return Scene(api.spheres_at(sc.spheres, disp, t), sc.planes, sc.lights)


def fma32(t, d, c):
    """float32 fma(t, d, c) with ONE rounding, in numpy: the product of two float32 is exact in float64; the float64 sum is made round-to-odd
    with the error term of the two-sum, which rounds to float32 as the exact sum does (53 >= 24 + 2 bits)"""
    t, d, c = (np.asarray(v, np.float32).astype(np.float64) for v in (t, d, c))
    p = t * d                                   # exact
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)             # two-sum: p + c == s + err exactly
    odd = (s.view(np.uint64) & np.uint64(1)).astype(bool)
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & ~odd, np.nextafter(s, toward), s)
    return s.astype(np.float32)
