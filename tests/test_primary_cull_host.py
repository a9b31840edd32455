"""The primary-ray cull table on the CPU (include/hip_wrap_ext.h: clw_host_primary_cull; csrc/primary_cull_host.h states the rule): one byte per
8x8 tile, bit 0 = no primary ray of the tile passes the line test (D >= 0) of any sphere, bit 1 = of any light.

SOUNDNESS is what the trace kernel relies on: wherever a bit is set, every pixel ray of the tile -- the oracle's raygen, bit for bit the kernel's
wt_primary_dir_xy -- must have D < 0 for every primitive of the group, D being the discriminant of the oracle's intersect_sphere evaluated in
float32.  Beyond that sign the test holds the MARGIN the rule promises: in float64, D / |c - o|^2 <= -4e-6 for those rays (the header derives
-9e-6 and bounds the kernel's float32 rounding, fused or not, a = 1 or d.d, by 4e-6), so that the fast build's differently rounded discriminant
has the same sign.  Families: random scenes with spheres in front, beside and behind the camera; a camera inside a sphere; spheres grazing a tile
corner; frames whose width and rows are no multiples of 8, with a row offset, and 8-row band shares; terms that are not finite.  Every family
must produce set AND clear bits (printed as shares), or the test would hold nothing.

The demo view (tests/conftest.py: CAM over render.map) at 1920x1080, 135 x 240 = 32 400 tiles, measured here: bit 0 (spheres) set in 30 673 tiles
= 94.7 %, bit 1 (lights) set in 32 349 = 99.8 %, both in 30 622 = 94.5 %; the line of some sphere really crosses 1 600 tiles (4.9 %), so the
margin costs 127 tiles (test_demo_view_shares asserts the counts)."""
import ctypes as C

import numpy as np
import pytest

from conftest import CAM
from cull_common import check_case, disc32, disc64_rel, launch_rays, oracle_camera, shares, tile_any, tile_max  # noqa: F401
from example_gui_opencl_raytracer_amd import api, scene

F = np.float32


def rand_scene(rng, o, look, ns, behind=False):
    """ns spheres and 3 lights scattered in front of, beside and (behind=True: only) behind the camera"""
    look = look / np.linalg.norm(look)
    s = np.zeros(ns, scene.SPHERE)
    for k in range(ns):
        dist = rng.uniform(2.0, 12.0)
        side = rng.normal(size=3) * rng.choice([0.2, 1.0, 3.0])
        sign = -1.0 if behind or rng.random() < 0.25 else 1.0
        s[k]["origin"] = o + sign * dist * look + side
        s[k]["radius"] = rng.uniform(0.2, 1.5)
        s[k]["material"] = scene.plastic()
    l = scene.render_map_scene().lights.copy()
    for k in range(3):
        l[k]["origin"] = o + rng.uniform(3.0, 10.0) * look + rng.normal(size=3) * rng.choice([0.3, 2.0])
        l[k]["radius"] = rng.choice([0.1, 0.3])
    return scene.Scene(s, scene.render_map_scene().planes, l)


def rand_camera(rng, W, H):
    o = rng.uniform(-5, 5, 3)
    look = rng.normal(size=3)
    look[1] *= 0.3      # (the reference rejects a view straight up)
    return o, look, api.perspective(tuple(o), tuple(look), float(rng.choice([40.0, 60.0, 90.0, 110.0])), 1.0, W, H)


FRAMES = [(64, 40), (72, 44), (37, 29), (50, 23)]      # width x height; the last three have tiles cut by the frame edge


def test_random_scenes(oracle):
    rng = np.random.default_rng(1)
    tables = []
    for k in range(160):
        W, H = FRAMES[k % 4]
        o, look, cam = rand_camera(rng, W, H)
        sc = rand_scene(rng, o, look, 1 + k % 4)
        row_offset = int(rng.integers(0, H - 9)) if k % 2 else 0      # any row, not only tile rows
        rows = int(rng.integers(9, H - row_offset + 1))
        tables.append(check_case(oracle, cam, sc, rows=rows, row_offset=row_offset)[0])
    s0, s1 = shares("random scenes, row strips", tables)
    assert 0.05 < s0 < 0.95 and 0.05 < s1 < 0.95


def test_spheres_behind_the_camera(oracle):
    """the line test passes for a sphere BEHIND the camera: its tiles must stay clear"""
    rng = np.random.default_rng(2)
    tables, hit_tiles = [], 0
    for k in range(60):
        W, H = FRAMES[k % 4]
        o, look, cam = rand_camera(rng, W, H)
        table, ps, _ = check_case(oracle, cam, rand_scene(rng, o, look, 1 + k % 4, behind=True))
        tables.append(table)
        hit_tiles += int(ps.sum())
    s0, _ = shares("spheres behind the camera", tables)
    print(f"  tiles with a pixel whose line meets a sphere behind the camera: {hit_tiles}")
    assert hit_tiles > 100 and 0.05 < s0 < 0.95


def test_camera_inside_a_sphere(oracle):
    rng = np.random.default_rng(3)
    tables = []
    for k in range(40):
        W, H = FRAMES[k % 4]
        o, look, cam = rand_camera(rng, W, H)
        sc = rand_scene(rng, o, look, 1 + k % 4)
        j = k % len(sc.spheres)
        sc.spheres[j]["radius"] = 2.0
        off = rng.normal(size=3)
        off *= (0.0 if k % 5 == 0 else rng.uniform(0.1, 1.99)) / np.linalg.norm(off)      # (every fifth: the origin IS the centre; else up to 0.5 % inside)
        sc.spheres[j]["origin"] = o + off
        table = check_case(oracle, cam, sc)[0]
        assert not (table & api.CULL_SPHERES).any()      # never, whatever the other spheres do
        tables.append(table)
    _, s1 = shares("camera inside a sphere", tables)
    assert 0.05 < s1 < 0.95      # (bit 0 is all clear by the rule; the lights' bit must still show both)


def test_spheres_grazing_a_tile_corner(oracle):
    """a sphere tangent to the ray of a tile's corner pixel: the silhouette runs through the corner where four tiles meet"""
    rng = np.random.default_rng(4)
    tables = []
    for k in range(80):
        W, H = FRAMES[k % 4]
        o, look, cam = rand_camera(rng, W, H)
        rays = oracle.raygen(oracle_camera(cam))
        px, py = 8 * int(rng.integers(1, W // 8)) - (k & 1), 8 * int(rng.integers(1, H // 8)) - ((k >> 1) & 1)      # the corner's four pixels in turn
        d = rays[py * W + px, 4:7].astype(np.float64)
        n = np.cross(d, rng.normal(size=3)); n /= np.linalg.norm(n)
        r, t = rng.uniform(0.3, 1.2), rng.uniform(3.0, 9.0)
        sc = rand_scene(rng, o, look, 1)
        sc.spheres[0]["origin"] = o + t * d + n * r * (1.0 + rng.choice([-1e-3, 0.0, 1e-3, 1e-5]))
        sc.spheres[0]["radius"] = r
        tables.append(check_case(oracle, cam, sc)[0])
    s0, _ = shares("spheres grazing a tile corner", tables)
    assert 0.05 < s0 < 0.95


def test_band_shares(oracle):
    rng = np.random.default_rng(5)
    tables = []
    for k in range(24):
        W, H = (64, 48) if k % 2 else (37, 32)
        stride = 2 if H == 32 or k % 4 == 1 else 3
        o, look, cam = rand_camera(rng, W, H)
        sc = rand_scene(rng, o, look, 1 + k % 4)
        for phase in range(stride):
            tables.append(check_case(oracle, cam, sc, rows=H // stride, bands=(stride, phase))[0])
        # the shares of a frame are the rows of its whole table, dealt out
        whole = api.host_primary_cull(cam, sc.spheres, sc.lights)
        got = np.stack(tables[-stride:], 1).reshape(whole.shape)
        assert np.array_equal(got, whole)
    s0, s1 = shares("8-row band shares", tables)
    assert 0.05 < s0 < 0.95 and 0.05 < s1 < 0.95
    with pytest.raises(ValueError):
        api.host_primary_cull(cam, sc.spheres, sc.lights, rows=16, band_stride=2, band_phase=2)


def test_nothing_is_set_for_terms_that_are_not_finite(oracle, demo_scene):
    cam = api.perspective(CAM["origin"], CAM["look"], CAM["fov"], CAM["focal"], 64, 40)
    good = api.host_primary_cull(cam, demo_scene.spheres, demo_scene.lights)
    assert (good & 1).any() and (good & 2).any() and not (good & 1).all()
    for field in ("im_corner", "origin", "up", "right", "w_factor", "h_factor"):
        for bad in (np.nan, np.inf, -np.inf):
            c = api.clw_camera.from_buffer_copy(bytes(cam))
            if field.endswith("factor"):
                setattr(c, field, bad)
            else:
                getattr(c, field)[1] = bad
            assert not api.host_primary_cull(c, demo_scene.spheres, demo_scene.lights).any(), (field, bad)
    for bad in (np.nan, np.inf):
        for what in ("origin", "radius"):
            sc = scene.Scene(demo_scene.spheres.copy(), demo_scene.planes, demo_scene.lights.copy())
            if what == "origin": sc.spheres[2]["origin"][0] = bad
            else: sc.spheres[2]["radius"] = bad
            t = api.host_primary_cull(cam, sc.spheres, sc.lights)
            assert not (t & 1).any() and np.array_equal(t & 2, good & 2), (what, bad)
            sc = scene.Scene(demo_scene.spheres.copy(), demo_scene.planes, demo_scene.lights.copy())
            if what == "origin": sc.lights[1]["origin"][2] = bad
            else: sc.lights[1]["radius"] = bad
            t = api.host_primary_cull(cam, sc.spheres, sc.lights)
            assert not (t & 2).any() and np.array_equal(t & 1, good & 1), (what, bad)
    # an empty group has nothing to test: its bit is set everywhere
    t = api.host_primary_cull(cam, None, demo_scene.lights)
    assert (t & 1).all() and np.array_equal(t & 2, good & 2)
    # refused: no tiles, a missing array
    L = api.load_library()
    out = np.zeros(64, np.uint8)
    assert L.clw_host_primary_cull(C.byref(cam), 0, 0, 1, 0, None, 0, None, 0, api._ptr(out)) == 0
    assert L.clw_host_primary_cull(C.byref(cam), 0, 8, 1, 0, None, 2, None, 0, api._ptr(out)) == 0
    assert L.clw_host_primary_cull(None, 0, 8, 1, 0, None, 0, None, 0, api._ptr(out)) == 0


def test_no_bit_where_float32_would_overflow(demo_scene):
    """a sphere so far away (or so large) that v.v overflows the kernel's float32: there D is inf - inf = NaN, which the kernel's `D < 0` does not
    reject -- every ray "hits", so the group may not be skipped although the sphere is far outside every tile's cone in float64"""
    cam = api.perspective(CAM["origin"], CAM["look"], CAM["fov"], CAM["focal"], 64, 40)
    good = api.host_primary_cull(cam, demo_scene.spheres, demo_scene.lights)
    for far, clear in ((1e18, True), (3e18, True), (4e18, False), (1e19, False), (3e19, False)):      # squares 1e36 .. 9e38; the limit is 1e37
        sc = scene.Scene(demo_scene.spheres.copy(), demo_scene.planes, demo_scene.lights.copy())
        sc.spheres[0]["origin"] = (far, 0.0, 0.0)
        t = api.host_primary_cull(cam, sc.spheres[:1], sc.lights)
        assert bool((t & 1).any()) == clear, far
        sc.lights[2]["origin"] = (0.0, far, 0.0)
        t = api.host_primary_cull(cam, demo_scene.spheres, sc.lights)
        assert bool((t & 2).any()) == clear and np.array_equal(t & 1, good & 1), far
    sc = scene.Scene(demo_scene.spheres.copy(), demo_scene.planes, demo_scene.lights)
    sc.spheres[1]["origin"], sc.spheres[1]["radius"] = (1e19, 0.0, 0.0), 4e18      # r^2 = 1.6e37
    assert not (api.host_primary_cull(cam, sc.spheres, sc.lights) & 1).any()


def test_the_planner_gives_a_table_to_the_launches_that_read_one():
    """csrc/launch_plan.c: wt_plan_cull -- a shallow, tiled, fused 1-sample launch of the pinhole camera over a linearly scanned scene, and nothing
    else; each condition is shown by the launch that differs in it alone (sample cameras and moving spheres only exist with samples in the
    planner, so their conditions are shown on a plan whose table counts are set by hand)"""
    import plan_common as pc
    from plan_common import plan, plan_in
    L = pc.seam()
    L.wt_plan_cull.argtypes = [C.POINTER(pc.PlanIn), C.POINTER(pc.PlanOut)]
    L.wt_plan_cull.restype = C.c_int
    cull = lambda i, o=None: L.wt_plan_cull(C.byref(i), C.byref(plan(L, i) if o is None else o))
    for strict in (0, 1):
        for depth in (1, 4):
            for sc in ((4, 2, 3), (1, 0, 3), (7, 1, 2), (200, 2, 3)):
                assert cull(plan_in(scene=sc, strict=strict, depth=depth)) == 1
    base = plan_in()
    assert cull(plan_in(variant=32768)) == 0
    assert cull(plan_in(depth=5)) == 0 and cull(plan_in(depth=15)) == 0
    assert cull(plan_in(supersample=2)) == 0
    assert cull(plan_in(rays="own")) == 0 and cull(plan_in(rays="caller")) == 0 and cull(plan_in(rays="exposed")) == 0
    assert cull(plan_in(variant=2)) == 0                                     # linear ids: no tiles
    assert cull(plan_in(scene=(400, 0, 3), grid_usable=1)) == 0              # the uniform grid
    assert cull(plan_in(array_size=0)) == 0                                  # an empty range: no launch at all
    assert cull(plan_in(counting=1)) == 1 and cull(plan_in(variant=8192)) == 1 and cull(plan_in(variant=1)) == 1
    o = plan(L, base)
    assert cull(base, o) == 1
    for field, value in (("n_cams", 4), ("motion_floats", 768), ("ss", 2), ("fused", 0), ("status", pc.REFUSED)):
        o = plan(L, base)
        setattr(o, field, value)
        assert cull(base, o) == 0, field
    o = plan(L, base)
    o.P.ss_lg = 1
    assert cull(base, o) == 0
    o = plan(L, base)
    o.P.tiled = 0
    assert cull(base, o) == 0


def test_demo_view_shares(oracle, demo_scene):
    """the flagship frame: what share of its tiles skips which group (the figures the docstring and DESIGN.md quote)"""
    cam = api.perspective(CAM["origin"], CAM["look"], CAM["fov"], CAM["focal"], 1920, 1080)
    table, ps, pl = check_case(oracle, cam, demo_scene)
    s0, s1 = shares("demo view 1920x1080", [table])
    n0, n1, both = int((table & 1).astype(bool).sum()), int((table & 2).astype(bool).sum()), int((table == 3).sum())
    print(f"  tiles: {table.size}; bit 0 set {n0}, bit 1 set {n1}, both {both}; tiles some sphere's line really crosses {int(ps.sum())}, some light's {int(pl.sum())}")
    assert table.shape == (135, 240)
    assert s0 > 0.5, "fewer than half of the demo view's tiles skip the sphere loop: the estimate of the gain rests on it"
    assert (n0, n1, both) == (30673, 32349, 30622)
