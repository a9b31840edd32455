"""The primary-ray cull table on the GPU (include/hip_wrap_ext.h: clw_host_primary_cull, clw_ext_read_primary_cull; csrc/whitted_cull.inc builds it,
csrc/whitted_hit.inc reads it): a tile whose primary rays all fail the line test of every sphere / every light skips that group of tests in its
first loop iteration.  Skipping a test that fails in every lane may not change a bit, so every frame here is compared with the frame of the same
renderer under variant 32768 (no table), packed and float, fast and strict build (cull_common.on_and_off); the device table is held to the host
definition; and the launches that must not use a table are shown to run without one.

This module is about the table's life: when it is built, what it follows, which launches take none, strips and band shares.  Its views are
render.map and one-sphere cuts of it, so of the 22 twin kernels `wt_trace_cull<FLAGS>` it launches five: the shaped twins of (4 spheres, 2 planes)
and (1, 2), the strict LDS twin (flag word 4) and the two counting twins (word 5 of either build).  tests/test_gpu_cull_twins.py runs all 22."""
import numpy as np
import pytest

from conftest import CAM
from cull_common import NO_CULL, no_table, on_and_off
from render_common import R, api, released, rendering, take  # noqa: F401

pytestmark = pytest.mark.gpu

SIZES = [(64, 40), (72, 44)]      # the second has tiles cut by the right and the bottom edge


def one_sphere(demo_scene, centre, radius, material=None):
    from example_gui_opencl_raytracer_amd import scene
    s = demo_scene.spheres[:1].copy()
    s[0]["origin"], s[0]["radius"] = centre, radius
    if material is not None:
        s[0]["material"] = material
    return scene.Scene(s, demo_scene.planes, demo_scene.lights)


def corner_scene(api, demo_scene, W, H):
    """one small sphere on the ray of the pixel where four tiles meet, so that it covers one corner of a tile and little else"""
    cam = api.perspective(CAM["origin"], CAM["look"], CAM["fov"], CAM["focal"], W, H)
    px, py = 24, 16
    v = np.array([cam.im_corner[a] + cam.right[a] * cam.w_factor * (px - 0.5) - cam.up[a] * cam.h_factor * (py - 0.5) for a in range(3)])
    v /= np.linalg.norm(v)
    return one_sphere(demo_scene, tuple(np.array(cam.origin[:]) + 6.0 * v), 0.12)


def scenes(api, demo_scene, W, H):
    from example_gui_opencl_raytracer_amd import scene
    return {
        "demo": (demo_scene, CAM),
        "corner": (corner_scene(api, demo_scene, W, H), CAM),
        "inside glass": (one_sphere(demo_scene, (0.8, 2.3, -7.6), 1.5, scene.glass()), CAM),
        "light in view": (demo_scene, dict(origin=(2.0, 1.5, -2.5), look=(0.0, 0.0, 1.0), fov=60.0, focal=1.0)),
    }


@pytest.mark.parametrize("strict", [False, True], ids=["fast", "strict"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_table_on_is_table_off(R, api, demo_scene, tex, sky, size, strict):
    W, H = size
    for name, (sc, cam) in scenes(api, demo_scene, W, H).items():
        for depth in (1, 4):
            with rendering(R, sc, tex, sky, W, H, cam=cam, depth=depth, strict=strict) as r:
                what = f"{name} {W}x{H} depth {depth} {'strict' if strict else 'fast'}"
                _, table = on_and_off(r, what)
                # the device table is the host definition's: it may set fewer bits, never more -- and it is the same arithmetic, so the same table
                c = api.perspective(cam["origin"], cam["look"], cam["fov"], cam["focal"], W, H)
                host = api.host_primary_cull(c, sc.spheres, sc.lights).reshape(-1)
                print(f"{what}: {table.size} tiles, device bits set {int((table & 1).astype(bool).sum())} / {int((table & 2).astype(bool).sum())}, "
                      f"host {int((host & 1).astype(bool).sum())} / {int((host & 2).astype(bool).sum())}")
                assert table.shape == host.shape and not (table & ~host).any(), what
                assert np.array_equal(table, host), what
                if name == "inside glass":
                    assert not (table & 1).any()
                if name == "light in view":
                    assert (table & 2).any() and not (table & 2).all(), what      # a light's line crosses some tiles: they keep the probe
                if name in ("demo", "corner"):
                    assert (table & 1).any() and not (table & 1).all() and (table & 2).any(), what      # not vacuous: tiles skip, tiles do not


@pytest.mark.parametrize("strict", [False, True], ids=["fast", "strict"])
def test_row_strip_and_band_share(R, api, demo_scene, tex, sky, strict):
    W, H = 72, 44
    cam = api.perspective(CAM["origin"], CAM["look"], CAM["fov"], CAM["focal"], W, H)
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict) as r:
        whole, _ = on_and_off(r, "whole frame")
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict, first_row=19, rows=21) as r:      # a strip that starts inside a tile row
        strip, table = on_and_off(r, "rows 19..39")
        assert np.array_equal(strip[0], whole[0][19 * W:40 * W])
        assert np.array_equal(table, api.host_primary_cull(cam, demo_scene.spheres, demo_scene.lights, rows=21, row_offset=19).reshape(-1))
        assert (table & 1).any() and not (table & 1).all()
    W, H = 64, 40
    cam = api.perspective(CAM["origin"], CAM["look"], CAM["fov"], CAM["focal"], W, H)
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict) as r:
        whole = take(r, 1)[0]
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict, bands=(5, 2)) as r:      # the 8-row band 2 of 5
        band, table = on_and_off(r, "band 2 of 5")
        assert np.array_equal(band[0], whole[0][16 * W:24 * W])
        assert np.array_equal(table, api.host_primary_cull(cam, demo_scene.spheres, demo_scene.lights, rows=8, band_stride=5, band_phase=2).reshape(-1))


def test_table_follows_the_camera_and_the_scene(R, api, demo_scene, tex, sky):
    """a still view builds its table once; a new camera and a rewritten scene each build it again, and the frame is the table-off frame"""
    import torch
    from example_gui_opencl_raytracer_amd.scene import RAY, Scene
    W, H, depth = 64, 40, 4
    other = dict(origin=(-2.0, 1.5, -6.0), look=(0.4, 0.0, 1.0), fov=70.0, focal=1.0)
    moved = demo_scene.spheres.copy()
    moved["origin"][0] = (1.5, 0.5, -2.0)
    want = {}
    for key, sc, cam in (("first", demo_scene, CAM), ("camera", demo_scene, other), ("scene", Scene(moved, demo_scene.planes, demo_scene.lights), other)):
        with rendering(R, sc, tex, sky, W, H, cam=cam, depth=depth, setup=lambda w: w.set_variant(NO_CULL)) as r:
            want[key] = r.render().copy()
            assert no_table(r.w, 0)
    assert not np.array_equal(want["camera"], want["scene"])
    sph = torch.from_numpy(np.frombuffer(demo_scene.spheres.tobytes(), np.uint8).copy()).cuda()      # a caller-owned sphere array, rewritten in place
    with released(api.ClWrap()) as cw:
        cw.set_depth(depth)
        f3 = lambda v: np.array([v[0], v[1], v[2], 0.0], np.float32)

        def look(cam):
            c = api.perspective(cam["origin"], cam["look"], cam["fov"], cam["focal"], W, H)
            for a, v in enumerate((f3(c.im_corner), f3(c.origin), f3(c.up), f3(c.right), np.float32(c.w_factor), np.float32(c.h_factor))):
                cw.load_single_data(0, a, v)
            return c
        look(CAM)
        cw.load_single_data(0, 6, np.uint32(W)); cw.load_single_data(0, 7, np.uint32(H))
        cw.load_global_data(0, 8, None, RAY.itemsize * W * H)
        cw.load_single_data(1, 0, cw.buffer_handle(0, 8))
        cw.bind_device_buffer(1, 1, sph.data_ptr(), sph.numel())
        cw.load_global_data(1, 2, demo_scene.planes)
        cw.load_global_data(1, 3, demo_scene.lights)
        for a, n in ((4, len(demo_scene.spheres)), (5, len(demo_scene.planes)), (6, len(demo_scene.lights))):
            cw.load_single_data(1, a, np.uint8(n))
        cw.load_single_data(1, 7, np.uint32(W * H))
        cw.load_images_raw(1, 8, tex); cw.load_images_raw(1, 9, sky)
        cw.load_global_data(1, 10, None, 4 * W * H)

        def frame():
            out = np.empty(W * H, np.uint32)
            cw.output(W * H, 0, 0, 0, 0, None)
            cw.output(W * H, out.nbytes, 1, 1, 10, out)
            return out
        for k in range(4):      # a still view: no table for its first frame, then one build
            assert np.array_equal(frame(), want["first"])
            table, builds = cw.read_primary_cull()
            assert builds == min(k, 1) and (table is not None) == (k > 0)
        first_table = table
        c = look(other)
        assert np.array_equal(frame(), want["camera"])      # the frame after a camera change never reads the old view's table: it reads none
        assert no_table(cw, 1)
        assert np.array_equal(frame(), want["camera"])
        table, builds = cw.read_primary_cull()
        assert builds == 2 and not np.array_equal(table, first_table)
        assert np.array_equal(table, api.host_primary_cull(c, demo_scene.spheres, demo_scene.lights).reshape(-1))
        sph.copy_(torch.from_numpy(np.frombuffer(moved.tobytes(), np.uint8).copy()))
        torch.cuda.synchronize()
        cw.invalidate_scene()
        assert np.array_equal(frame(), want["scene"])       # ... and so the frame after a scene upload
        assert no_table(cw, 2)
        assert np.array_equal(frame(), want["scene"])
        scene_table, builds = cw.read_primary_cull()
        assert builds == 3 and not np.array_equal(scene_table, table)
        assert np.array_equal(scene_table, api.host_primary_cull(c, moved, demo_scene.lights).reshape(-1))
        assert np.array_equal(frame(), want["scene"]) and cw.read_primary_cull()[1] == 3
        # a camera that moves every frame builds nothing and reads nothing
        for k in range(4):
            look(dict(other, origin=(-1.9 + 0.1 * k, 1.5, -6.0)))
            frame()
            assert no_table(cw, 3)


@pytest.mark.parametrize("strict", [False, True], ids=["fast", "strict"])
def test_ray_counters_do_not_see_the_table(R, api, demo_scene, tex, sky, strict):
    W, H = 72, 44
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict, setup=lambda w: w.enable_counters(1)) as r:
        r.render()      # (the view's first frame: no table yet)
        r.w.read_counters()
        on = r.render().copy()
        assert r.w.read_primary_cull()[0] is not None
        c_on = r.w.read_counters()
        r.w.set_variant(NO_CULL)
        off = r.render().copy()
        c_off = r.w.read_counters()
    print(c_on)
    assert np.array_equal(on, off) and c_on == c_off and c_on["segments"] > W * H


def test_launches_that_take_no_table(R, api, demo_scene, tex, sky):
    from example_gui_opencl_raytracer_amd import scene
    W, H = 64, 40
    disp = np.zeros((4, 3), np.float32); disp[0] = (0.5, 0.0, 0.0)
    cases = {
        "lens camera": dict(supersample=2, lens=(0.05, 6.0), depth=4),
        "moving spheres": dict(supersample=2, motion=disp, depth=4),
        "ray buffer": dict(fuse=False, depth=4),
        "supersampled": dict(supersample=2, depth=4),      # (left on a null table: the table would have to be built over the virtual tiles)
        "deep": dict(depth=6),
    }
    for name, kw in cases.items():
        with rendering(R, demo_scene, tex, sky, W, H, **kw) as r:
            for _ in range(3):
                r.render()
                assert no_table(r.w, 0), name
    with rendering(R, scene.sphere_grid_scene(20, 20), tex, sky, W, H, depth=4) as r:      # 400 spheres: the uniform grid
        for _ in range(3):
            r.render()
            assert r.w.last_trace_flags() & 16 and no_table(r.w, 0)
    with rendering(R, demo_scene, tex, sky, W, H, depth=4) as r:      # ... and the launch they are not
        for _ in range(3):
            r.render()
        table, builds = r.w.read_primary_cull()
        assert table is not None and table.size == 5 * 8 and builds == 1
