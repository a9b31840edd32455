"""Shared by test_sphere_motion_host.py and test_gpu_sphere_motion.py: the displacements the tests use and the numpy side of the definition of
moving spheres.

With factor n, a displacement table disp[spheres, 3] and sample times t[0 .. n*n), the sample at virtual pixel (vx, vy) is pixel (vx, vy) of
the 1-sample render of the n*W x n*H frame of the scene S(t[(vy mod n) * n + (vx mod n)]), whose sphere i has centre fma(t, disp[i], c[i])
(api.spheres_at = clw_host_spheres_at); clamp, add and scale as plain supersampling (render_common.resolve)."""
import numpy as np

from conftest import CAM
from render_common import assert_same_frames, rendering, take
from sample_cameras_common import composed, rows_of, virtual_camera

from flags_common import F_SS      # noqa: F401  (clw_ext_last_trace_flags)
LENS = (0.2, 8.0)
CAM2 = dict(origin=(1.6, 3.1, -6.5), look=(0.05, -0.15, 1.0), fov=90.0, focal=1.0)      # the other end of a camera shutter

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


# ---- the GPU side of the definition (R = renderer.Renderer, api = the api module; `cam`, `cam2`: the launch camera and the shutter's other end)
def camera_table(api, W, H, n, kind, cam=CAM, cam2=CAM2):
    """kind None: n*n copies of the launch camera; (aperture, focus): the lens table; "shutter": cam -> cam2 -> (base camera, float32 [n*n, 12])"""
    base = api.perspective(**cam, width=W, height=H)
    if kind is None:
        return base, np.tile(rows_of(base), (n * n, 1))
    if kind == "shutter":
        return base, api.shutter_cameras(base, api.perspective(**cam2, width=W, height=H), n)
    return base, api.lens_cameras(base, kind[0], kind[1], n)


def gpu_virtual(R, api, sc, tex, sky, disp, t, base, row, n, depth, strict, what="rgb", setup=None):
    """the GPU's own 1-sample render of the n*W x n*H frame of S(t) through the camera `row` of a table"""
    with rendering(R, moved_scene(api, sc, disp, float(t)), tex, sky, n * base.width, n * base.height, setup=setup,
                   cam=virtual_camera(api.clw_camera, row, base, n), depth=depth, strict=strict) as r:
        (p, f), = take(r, rgb=what == "rgb")
        return (p if f is None else f), r.w.last_trace_flags()


def gpu_composed(R, api, sc, tex, sky, disp, times, W, H, n, depth, strict, cams=None, setup=None, cam=CAM, cam2=CAM2):
    """`composed` over the GPU's own 1-sample virtual frames of the moved scenes -> (packed, float)"""
    base, table = camera_table(api, W, H, n, cams, cam, cam2)

    def render_virtual(k):
        f, flags = gpu_virtual(R, api, sc, tex, sky, disp, times[k], base, table[k], n, depth, strict, setup=setup)
        assert not flags & F_SS
        return f
    return composed(render_virtual, table, W, H, n)


def moving(R, sc, tex, sky, W, H, n, depth, strict, disp, times=None, cams=None, count=1, setup=None, rgb=True, cam=CAM, **kw):
    """`count` frames of one supersampled renderer with a displacement table (None = none), optional explicit times and a lens
    (cams = (aperture, focus)) or a table of cameras (cams = float32 [n*n, 12]) -> [(packed, float)], flags, the times the last launch used"""
    lens = cams if isinstance(cams, tuple) else None

    def knobs_then_tables(w):
        if setup:
            setup(w)
        if times is not None:
            w.set_sphere_motion(disp, times)
        if cams is not None and lens is None:
            w.set_sample_cameras(cams)
    with rendering(R, sc, tex, sky, W, H, setup=knobs_then_tables, cam=cam, depth=depth, strict=strict, supersample=n, lens=lens,
                   motion=disp if times is None else None, **kw) as r:
        return take(r, count, rgb), r.w.last_trace_flags(), r.w.get_sample_times()


def check_self_consistent(R, api, sc, tex, sky, W, H, n, depth, strict, disp=DISP, times=None, cams=None, count=1, setup=None, cam=CAM, cam2=CAM2):
    used_times = api.sample_times(n) if times is None else np.asarray(times, np.float32)
    want_p, want_f = gpu_composed(R, api, sc, tex, sky, disp, used_times, W, H, n, depth, strict, cams=cams, setup=setup, cam=cam, cam2=cam2)
    table = None if cams is None or isinstance(cams, tuple) else camera_table(api, W, H, n, cams, cam, cam2)[1]
    got, flags, used = moving(R, sc, tex, sky, W, H, n, depth, strict, disp, times=times, cams=cams if table is None else table, count=count, setup=setup, cam=cam)
    assert flags & F_SS
    assert used.tobytes() == used_times.tobytes()
    for p, f in got:
        assert p.shape == (W * H,) and f.shape == (W * H, 3)
    assert_same_frames(got, want_p, want_f, f"{W}x{H} n={n} depth {depth} strict={int(strict)} cams={cams}")
    # and the moving frame is not the static supersampled one
    static = moving(R, sc, tex, sky, W, H, n, depth, strict, None, cams=cams if table is None else table, rgb=False, setup=setup, cam=cam)[0][0][0]
    print(f"  {100 * float((static != want_p).mean()):.1f} % of the pixels differ from the static supersampled frame")
    assert not np.array_equal(static, want_p)
    return flags, want_p
