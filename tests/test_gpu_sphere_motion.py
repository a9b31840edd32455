"""Moving spheres (clw_ext_set_sphere_motion; Renderer(motion=...), Renderer.set_sphere_motion) on a real GPU.

The definition every test uses (sphere_motion_common.py): with factor n, a displacement table and sample times t[0 .. n*n), the sample at
virtual pixel (vx, vy) is pixel (vx, vy) of the 1-sample render of the n*W x n*H frame of the scene S(t[(vy mod n) * n + (vx mod n)])
(api.spheres_at) -- through the launch camera, or through camera k of a table of sample cameras; the samples are clamped, added and
scaled as in plain supersampling (render_common.resolve)."""
import numpy as np
import pytest

from flags_common import F_DEEP, F_GEOM_LDS, F_GRID, F_OCC, F_SHAPE
from render_common import R, api, queued_on, rendering, run_child, same_floats, take  # noqa: F401  (R, api: the fixtures)
from sample_cameras_common import composed, pick, virtual_camera
from sphere_motion_common import DISP, F_SS, LENS, camera_table, check_self_consistent, field_disp, gpu_virtual, moved_scene, moving

pytestmark = pytest.mark.gpu

COUNTED = ("segments", "shadow_rays", "light_probes", "sky_fetches", "texel_fetches", "pushes")


# ------------------------------------------------------------------ 1. self-consistency, exact, both builds
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("W,H,n", [(320, 240, 2), (200, 152, 4), (96, 64, 8), (101, 75, 2)])
def test_shallow_moving_frame_is_composed_of_the_gpus_own_frames_of_the_moved_scenes(R, api, demo_scene, tex, sky, W, H, n, strict):
    flags, _ = check_self_consistent(R, api, demo_scene, tex, sky, W, H, n, 4, strict)
    assert not flags & F_DEEP
    if not strict:
        assert flags & F_SHAPE          # the shaped shallow kernel of the fast build really ran with the table


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("W,H,n", [(400, 300, 2), (96, 64, 8)])
def test_deep_moving_frames_are_composed_of_the_gpus_own_frames_of_the_moved_scenes(R, api, demo_scene, tex, sky, W, H, n, strict):
    """Three frames in a row: the second and third run with the cost-sorted order (moving launches run without the tail and the split)."""
    flags, _ = check_self_consistent(R, api, demo_scene, tex, sky, W, H, n, 15, strict, count=3)
    assert flags & F_DEEP and not flags & F_OCC


def test_glass_field(R, api, tex, sky):
    from example_gui_opencl_raytracer_amd import scene
    sc = scene.dielectric_field_scene()
    for strict in (True, False):
        flags, _ = check_self_consistent(R, api, sc, tex, sky, 256, 256, 2, 8, strict, disp=field_disp(len(sc.spheres)), count=3)
        assert flags & F_DEEP


def test_high_occupancy_deep_flavour(R, api, demo_scene, tex, sky):
    """A big deep launch of the fast build takes the high-occupancy flavour: 1024x768 n = 4 at depth 6 is 196 608 virtual tiles."""
    flags, _ = check_self_consistent(R, api, demo_scene, tex, sky, 1024, 768, 4, 6, False, count=2)
    assert flags & F_OCC


def scene_just_over_the_staging_limit():
    """256 spheres, 254 planes, 3 lights: 256 + 2 * 254 + 2 * 3 = 770 float4 of prepared geometry (no light / plane side table at this many
    planes) fit the 1024 float4 (16 KiB) that are staged in LDS, and 770 + 256 with the displacement table do not.  The planes are the
    floor and 253 copies of it below, where no ray gets; every third sphere moves."""
    from example_gui_opencl_raytracer_amd import scene
    sc = scene.sphere_grid_scene(16, 16)
    planes = np.repeat(sc.planes[:1], 254)
    planes["point_in_plane"][1:, 1] = -1.0 - 0.01 * np.arange(253, dtype=np.float32)
    disp = np.zeros((256, 3), np.float32)
    disp[0::3] = (0.25, 0.1, 0.0)
    disp[1::6] = (0.0, 0.0, -0.3)
    return scene.Scene(sc.spheres, planes, sc.lights), disp


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_a_table_that_does_not_fit_the_staged_16_kib_is_read_from_global_memory(R, api, tex, sky, strict):
    """The 16 KiB staging rule counts the table: the moving launch of this scene runs the kernels that read geometry and displacements from
    global memory, its static launch (and every 1-sample frame it is composed of) the ones that stage the scene in LDS."""
    sc, disp = scene_just_over_the_staging_limit()
    W, H, n, depth = 96, 64, 2, 4
    flags, _ = check_self_consistent(R, api, sc, tex, sky, W, H, n, depth, strict, disp=disp)
    assert not flags & F_GEOM_LDS and not flags & F_GRID
    static_flags = moving(R, sc, tex, sky, W, H, n, depth, strict, None, rgb=False)[1]
    assert static_flags & F_GEOM_LDS and static_flags & F_SS


# ------------------------------------------------------------------ 2. against the oracle, strict build
@pytest.mark.parametrize("W,H,n,depth", [(320, 240, 2, 4), (200, 152, 4, 4), (400, 300, 2, 15)])
def test_strict_moving_frame_is_composed_of_the_oracles_frames_of_the_moved_scenes(R, api, oracle, demo_scene, tex, sky, W, H, n, depth):
    """The strict build differs from glibc on isolated 1-ulp sinf / cosf / powf inputs (profiles/r03_libm_divergence.jsonl), so the output
    pixels whose footprint holds a SELECTED virtual pixel at which the strict 1-sample render of S(t[k]) itself differs from the oracle's
    are left out: at most 4 per configuration (the cap of tests/test_gpu_sample_cameras.py for these sizes).  Displacement: DISP of
    sphere_motion_common.py."""
    from oracle.oracle_py import Camera
    times = api.sample_times(n)
    base, table = camera_table(api, W, H, n, None)
    oracle_frames = {}

    def oracle_virtual(k):
        p, f, _ = oracle.render(virtual_camera(Camera, table[k], base, n), moved_scene(api, demo_scene, DISP, float(times[k])), tex, sky, depth, want_rgb=True)
        oracle_frames[k] = p
        return f
    want_p, want_f = composed(oracle_virtual, table, W, H, n)

    def differs(k):
        return gpu_virtual(R, api, demo_scene, tex, sky, DISP, times[k], base, table[k], n, depth, True, what="packed")[0] != oracle_frames[k]
    selected = pick(differs, W, H, n)
    left_out = selected.reshape(H, n, W, n).any((1, 3)).reshape(-1)
    print(f"{W}x{H} n={n} depth {depth}: {int(selected.sum())} selected virtual pixels differ from the oracle, {int(left_out.sum())} output pixels left out")
    assert left_out.sum() <= 4
    ((p, f),), flags, _ = moving(R, demo_scene, tex, sky, W, H, n, depth, True, DISP)
    assert flags & F_SS
    keep = ~left_out
    print(f"  {int((p[keep] != want_p[keep]).sum())} kept packed pixels differ, {int((f[keep].view(np.uint32) != want_f[keep].view(np.uint32)).any(1).sum())} float")
    assert np.array_equal(p[keep], want_p[keep])


# ------------------------------------------------------------------ 3. with sample cameras; explicit times
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("W,H,n,depth,cams", [(200, 152, 4, 4, LENS), (400, 300, 2, 15, LENS), (200, 152, 4, 4, "shutter"), (400, 300, 2, 15, "shutter")])
def test_motion_with_a_lens_or_a_camera_shutter(R, api, demo_scene, tex, sky, W, H, n, depth, cams, strict):
    """sample k looks through cams[k] at S(t[k]): spheres and a shutter-blurred camera move on one clock"""
    check_self_consistent(R, api, demo_scene, tex, sky, W, H, n, depth, strict, cams=cams)


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_explicit_times_are_honoured(R, api, demo_scene, tex, sky, strict):
    W, H, n, depth = 200, 152, 4, 4
    default = api.sample_times(n)
    times = default[::-1].copy()                      # a permutation of the default times
    _, want_p = check_self_consistent(R, api, demo_scene, tex, sky, W, H, n, depth, strict, times=times)
    got, _, used = moving(R, demo_scene, tex, sky, W, H, n, depth, strict, DISP, rgb=False)
    assert used.tobytes() == default.tobytes()
    assert not np.array_equal(got[0][0], want_p)      # not the frame of the default times
    # ... and times outside the shutter's [0, 1] are times like any other
    check_self_consistent(R, api, demo_scene, tex, sky, 96, 64, 2, depth, strict, times=np.array([-0.5, 0.0, 1.0, 2.25], np.float32))


# ------------------------------------------------------------------ 4. degenerate tables
def counted_frames(R, sc, tex, sky, W, H, n, depth, strict, prepare):
    with rendering(R, sc, tex, sky, W, H, depth=depth, strict=strict, supersample=n) as r:
        prepare(r)
        (p, f), = take(r)
        p2 = r.render().copy()
        flags, costs, used = r.w.last_trace_flags(), r.w.read_tile_costs(), r.w.get_sample_times()
        r.w.enable_counters(1)
        r.render()
        c = r.w.read_counters()
        return p, f, p2, flags, costs, [c[k] for k in COUNTED], used


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("W,H,n,depth", [(200, 152, 4, 4), (400, 300, 2, 15)])
def test_degenerate_tables_give_the_plain_supersampled_frame(R, api, demo_scene, tex, sky, W, H, n, depth, strict):
    plain = counted_frames(R, demo_scene, tex, sky, W, H, n, depth, strict, lambda r: None)
    assert plain[6].size == 0
    ways = dict(all_zero=lambda r: r.set_sphere_motion(np.zeros_like(DISP)),
                negative_zero=lambda r: r.set_sphere_motion(-np.zeros_like(DISP), api.sample_times(n)),
                set_and_cleared=lambda r: (r.set_sphere_motion(DISP), r.set_sphere_motion(None)))
    for name, prepare in ways.items():
        got = counted_frames(R, demo_scene, tex, sky, W, H, n, depth, strict, prepare)
        assert np.array_equal(got[0], plain[0]) and same_floats(got[1], plain[1]) and np.array_equal(got[2], plain[2]), name
        assert got[3] == plain[3] and np.array_equal(got[4], plain[4]) and got[5] == plain[5] and got[6].size == 0, name
    # every time equal to tau: the plain supersampled frame of the static scene S(tau)
    tau = 0.375
    got = counted_frames(R, demo_scene, tex, sky, W, H, n, depth, strict, lambda r: r.set_sphere_motion(DISP, np.full(n * n, tau, np.float32)))
    want = counted_frames(R, moved_scene(api, demo_scene, DISP, tau), tex, sky, W, H, n, depth, strict, lambda r: None)
    assert np.array_equal(got[0], want[0]) and same_floats(got[1], want[1]) and np.array_equal(got[2], want[2])
    # the work counters, like against like: a moving launch runs without the tree-parallel tail and the tile split, so does this static one
    want = counted_frames(R, moved_scene(api, demo_scene, DISP, tau), tex, sky, W, H, n, depth, strict, lambda r: (r.w.set_tpt(0), r.w.set_variant(4096)))
    assert np.array_equal(got[0], want[0]) and got[5] == want[5]
    assert got[6].tolist() == [tau] * (n * n)
    assert not np.array_equal(got[0], plain[0])


# ------------------------------------------------------------------ 5. life cycle
def test_changing_displacement_times_factor_and_lens_between_frames(R, api, demo_scene, tex, sky):
    W, H, depth = 160, 120, 15
    half = (DISP * np.float32(0.5)).astype(np.float32)
    rev = lambda n: api.sample_times(n)[::-1].copy()
    # (factor, displacement, times, lens)
    steps = [(2, "full", None, None), (2, "full", None, None), (2, "half", None, None), (2, "half", "rev", None), (4, "half", None, None), (4, "full", None, LENS),
             (4, "full", None, LENS), (4, None, None, LENS), (4, None, None, None), (2, "full", "rev", None), (2, "full", None, LENS), (1, None, None, None),
             (8, "full", None, None), (2, "full", None, None)]
    disp_of = {"full": DISP, "half": half, None: None}
    for strict in (True, False):
        want = {}
        for n, d, t, lens in set(steps):
            want[(n, d, t, lens)] = moving(R, demo_scene, tex, sky, W, H, n, depth, strict, disp_of[d], times=rev(n) if t else None, cams=lens, rgb=False)[0][0][0]
        assert len({v.tobytes() for v in want.values()}) == len(want)
        with rendering(R, demo_scene, tex, sky, W, H, depth=depth, strict=strict) as r:
            for n, d, t, lens in steps:
                r.w.set_supersample(n)
                r.set_sphere_motion(disp_of[d], rev(n) if t else None)
                r.w.set_lens(*(lens or (0.0, 1.0)))
                assert np.array_equal(r.render(), want[(n, d, t, lens)]), (strict, n, d, t, lens)
                assert r.w.get_sample_times().tobytes() == (b"" if d is None else (rev(n) if t else api.sample_times(n)).tobytes())


def test_tables_that_change_under_queued_launches(R, demo_scene, tex, sky):
    """Asynchronous launches on a caller's stream into a torch-owned framebuffer, the displacement changed after every launch and nothing waited
    for until the end (the frames are copied aside in stream order): every copy holds the frame of the table its launch was given."""
    import torch
    W, H, n, depth = 640, 480, 2, 4
    scales = [1.0, 0.25, 0.5, 0.25, 0.25, 0.0, 1.0, 0.75]
    disp = {s: (DISP * np.float32(s)).astype(np.float32) for s in set(scales)}
    want = {s: moving(R, demo_scene, tex, sky, W, H, n, depth, False, disp[s], rgb=False)[0][0][0] for s in set(scales)}
    assert len({v.tobytes() for v in want.values()}) == len(want)
    fb = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with rendering(R, demo_scene, tex, sky, W, H, setup=queued_on(side), depth=depth, supersample=n, framebuffer_ptr=fb.data_ptr()) as r:
        outs = []
        for s in scales:
            r.set_sphere_motion(disp[s])
            r.render(readback=False)
            with torch.cuda.stream(side):
                outs.append(fb.clone())
        side.synchronize()
        for k, s in enumerate(scales):
            assert np.array_equal(outs[k].cpu().numpy().view(np.uint32), want[s]), (k, s)


def test_changing_the_stream_between_moving_frames(R, demo_scene, tex, sky):
    """The table was written in the order of the stream that was current then: a launch on another stream still reads the right one."""
    import torch
    W, H, n, depth = 320, 240, 2, 4
    disp = {s: (DISP * np.float32(s)).astype(np.float32) for s in (0.5, 1.0)}
    want = {s: moving(R, demo_scene, tex, sky, W, H, n, depth, True, disp[s], rgb=False)[0][0][0] for s in disp}
    side = torch.cuda.Stream()
    with rendering(R, demo_scene, tex, sky, W, H, depth=depth, strict=True, supersample=n) as r:
        for stream, s in ((0, 0.5), (side.cuda_stream, 0.5), (side.cuda_stream, 1.0), (0, 1.0), (0, 0.5), (side.cuda_stream, 1.0), (0, 1.0)):
            r.w.set_stream(stream)
            r.set_sphere_motion(disp[s])
            assert np.array_equal(r.render(), want[s]), (stream != 0, s)


@pytest.mark.parametrize("n", [2, 4])
def test_row_strips_compose(R, demo_scene, tex, sky, n):
    from example_gui_opencl_raytracer_amd.renderer import strip_rows
    W, H, depth = 400, 300, 4
    for strict in (True, False):
        full = moving(R, demo_scene, tex, sky, W, H, n, depth, strict, DISP, rgb=False)[0][0][0]
        static = moving(R, demo_scene, tex, sky, W, H, n, depth, strict, None, rgb=False)[0][0][0]
        assert not np.array_equal(full, static)
        parts = []
        for rank in range(3):
            r0, rows = strip_rows(H, 3, rank)
            part = moving(R, demo_scene, tex, sky, W, H, n, depth, strict, DISP, rgb=False, first_row=r0, rows=rows)[0][0][0]
            assert part.shape == (rows * W,)
            parts.append(part)
        assert np.array_equal(np.concatenate(parts), full)


# ------------------------------------------------------------------ 6. refusals: message + exit(1)
def _run(snippet, env=None):
    return run_child("from sphere_motion_common import DISP\n" + snippet, env)


BAD = "d = DISP.copy(); d[2, 1] = float(%r); "
REFUSED = {
    "factor_1": "r = Renderer(sc, tex, sky, 64, 48, depth=2, motion=DISP); r.look(**CAM); r.render()",
    "count_16_with_factor_2": "r = Renderer(sc, tex, sky, 64, 48, depth=2, supersample=2); r.set_sphere_motion(DISP, api.sample_times(4)); r.look(**CAM); r.render()",
    "count_3_with_factor_2": "r = Renderer(sc, tex, sky, 64, 48, depth=2, supersample=2); r.set_sphere_motion(DISP, api.sample_times(2)[:3]); r.look(**CAM); r.render()",
    # times given, none of them: only times == NULL makes the count irrelevant
    "count_0_with_factor_2": "t = np.zeros(4, np.float32)\n"
                             "r = Renderer(sc, tex, sky, 64, 48, depth=2, supersample=2); r.look(**CAM)\n"
                             "r.w.L.clw_ext_set_sphere_motion(api.C.byref(r.w.w), api._ptr(DISP), 4, api._ptr(t), 0); r.render()",
    "three_spheres_of_four": "r = Renderer(sc, tex, sky, 64, 48, depth=2, supersample=2, motion=DISP[:3]); r.look(**CAM); r.render()",
    "five_spheres_of_four": "r = Renderer(sc, tex, sky, 64, 48, depth=2, supersample=2, motion=np.concatenate([DISP, DISP[1:2]])); r.look(**CAM); r.render()",
    "nan_displacement": BAD % "nan" + "w = api.ClWrap(); w.set_sphere_motion(d)",
    "infinite_displacement": BAD % "-inf" + "w = api.ClWrap(); w.set_sphere_motion(d)",
    "nan_time": "w = api.ClWrap(); w.set_sphere_motion(DISP, np.array([0.1, float('nan'), 0.3, 0.4], np.float32))",
    "infinite_time": "w = api.ClWrap(); w.set_sphere_motion(DISP, np.array([0.1, 0.2, float('inf'), 0.4], np.float32))",
    "grid_scene": "big = scene.sphere_grid_scene(24, 24); d = np.zeros((576, 3), np.float32); d[5] = (0.2, 0, 0)\n"
                  "r = Renderer(big, tex, sky, 64, 48, depth=2, supersample=2, motion=d); r.look(**CAM); r.render()",
    "the_two_kernel_path": "r = Renderer(sc, tex, sky, 64, 48, depth=2, fuse=False, supersample=2, motion=DISP); r.look(**CAM); r.render()",
    # the life cycle: the scene's sphere count changes under a table that stays
    "another_sphere_count_under_the_same_table": "r = Renderer(sc, tex, sky, 64, 48, depth=2, supersample=2, motion=DISP); r.look(**CAM); r.render(); print('first frame')\n"
                                                 "r.w.load_single_data(1, 4, np.uint8(3)); r.render()",
}


# what the message of each refusal says (csrc/hip_wrap.cpp): the test asks for THIS refusal, not for any
SAYS = {
    "factor_1": "with supersampling factor 1",
    "count_16_with_factor_2": "16 sample times, but supersampling factor 2 needs 4",
    "count_3_with_factor_2": "3 sample times, but supersampling factor 2 needs 4",
    "count_0_with_factor_2": "0 sample times, but supersampling factor 2 needs 4",
    "three_spheres_of_four": "the displacement table is for 3 spheres, the scene has 4",
    "five_spheres_of_four": "the displacement table is for 5 spheres, the scene has 4",
    "nan_displacement": "displacement 1 of sphere 2 is not finite",
    "infinite_displacement": "displacement 1 of sphere 2 is not finite",
    "nan_time": "sample time 1 is not finite",
    "infinite_time": "sample time 2 is not finite",
    "grid_scene": "scenes of more than 256 spheres",
    "the_two_kernel_path": "Supersampling needs the fused raygen + trace launch",
    "another_sphere_count_under_the_same_table": "the displacement table is for 4 spheres, the scene has 3",
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_unsupported_combinations_exit_with_a_message(case):
    p = _run(REFUSED[case] + "\nprint('unreachable')")
    assert p.returncode == 1 and "ERROR:\t" in p.stdout and "unreachable" not in p.stdout, p.stdout + p.stderr
    assert SAYS[case] in p.stdout.split("ERROR:\t", 1)[1], p.stdout
    if case == "another_sphere_count_under_the_same_table":
        assert "first frame" in p.stdout


def test_resetting_the_motion_with_the_sphere_count_is_accepted():
    p = _run("r = Renderer(sc, tex, sky, 64, 48, depth=2, supersample=2, motion=DISP); r.look(**CAM); a = r.render().copy()\n"
             "r.w.load_single_data(1, 4, np.uint8(3)); r.set_sphere_motion(DISP[:3]); b = r.render().copy()\n"
             "r.set_sphere_motion(None); c = r.render().copy()\n"
             "assert not np.array_equal(a, b) and not np.array_equal(b, c)\nprint('three frames')")
    assert p.returncode == 0 and "three frames" in p.stdout, p.stdout + p.stderr
