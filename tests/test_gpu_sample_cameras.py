"""Per-sample cameras (clw_ext_set_sample_cameras, clw_ext_set_lens; Renderer(lens=...), Renderer.set_sample_cameras) on a real GPU.

The definition every test uses (sample_cameras_common.py): with factor n and a table cams[0 .. n*n), the sample at virtual pixel (vx, vy)
is pixel (vx, vy) of a 1-sample render of the n*W x n*H frame through cams[(vy mod n) * n + (vx mod n)] with w_factor / n, h_factor / n;
the samples are clamped, added and scaled as in plain supersampling (`resolve`)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import CAM, ROOT
from flags_common import F_DEEP, F_GRID, F_OCC, F_SHAPE, F_SS
from render_common import R, api, assert_same_frames, queued_on, rendering, run_child, same_floats, take  # noqa: F401  (R, api: the fixtures)
from sample_cameras_common import CAM2, composed, gpu_composed, make_table, pick, rows_of, sampled, virtual_camera

pytestmark = pytest.mark.gpu

LENS = (0.2, 8.0)
COUNTED = ("segments", "shadow_rays", "light_probes", "sky_fetches", "texel_fetches", "pushes")


def check_self_consistent(R, api, sc, tex, sky, W, H, n, depth, strict, kind=LENS, count=1, setup=None):
    base, table = make_table(api, W, H, n, kind)
    (want_p, want_f), vflags = gpu_composed(R, api, sc, tex, sky, base, table, W, H, n, depth, strict, setup=setup)
    got, flags, used = sampled(R, sc, tex, sky, W, H, n, depth, strict, kind, table=table, count=count, setup=setup)
    assert flags & F_SS and not vflags & F_SS
    assert used.tobytes() == table.tobytes()
    for p, f in got:
        assert p.shape == (W * H,) and f.shape == (W * H, 3)
    assert_same_frames(got, want_p, want_f, f"{W}x{H} n={n} depth {depth} strict={int(strict)} {kind}")
    return flags, want_p


# ------------------------------------------------------------------ 5. self-consistency, exact, both builds
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("W,H,n", [(320, 240, 2), (200, 152, 4), (96, 64, 8), (101, 75, 2)])
def test_shallow_lens_frame_is_composed_of_the_gpus_own_virtual_frames(R, api, demo_scene, tex, sky, W, H, n, strict):
    flags, want_p = check_self_consistent(R, api, demo_scene, tex, sky, W, H, n, 4, strict)
    assert not flags & F_DEEP
    if not strict:
        assert flags & F_SHAPE          # the shaped shallow kernel of the fast build really ran with the table
    # and the lens frame is not the plain supersampled one
    plain = sampled(R, demo_scene, tex, sky, W, H, n, 4, strict, None, rgb=False)[0][0][0]
    print(f"  {100 * float((plain != want_p).mean()):.1f} % of the pixels differ from the plain supersampled frame")
    assert not np.array_equal(plain, want_p)


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("W,H,n", [(400, 300, 2), (96, 64, 8)])
def test_deep_lens_frames_are_composed_of_the_gpus_own_virtual_frames(R, api, demo_scene, tex, sky, W, H, n, strict):
    """Three frames in a row: the second and third run with the cost-sorted order and (n < 8) split heavy tiles."""
    flags, _ = check_self_consistent(R, api, demo_scene, tex, sky, W, H, n, 15, strict, count=3)
    assert flags & F_DEEP and not flags & F_OCC


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("W,H,n,depth", [(200, 152, 4, 4), (400, 300, 2, 15)])
def test_explicit_shutter_table(R, api, demo_scene, tex, sky, W, H, n, depth, strict):
    flags, want_p = check_self_consistent(R, api, demo_scene, tex, sky, W, H, n, depth, strict, kind="shutter", count=2)
    for cam in (CAM, CAM2):      # neither end of the shutter
        assert not np.array_equal(want_p, sampled(R, demo_scene, tex, sky, W, H, n, depth, strict, None, cam=cam, rgb=False)[0][0][0])


def test_glass_field(R, api, tex, sky):
    from example_gui_opencl_raytracer_amd import scene
    for strict in (True, False):
        flags, _ = check_self_consistent(R, api, scene.dielectric_field_scene(), tex, sky, 256, 256, 2, 8, strict, count=3)
        assert flags & F_DEEP


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_uniform_grid_scene(R, api, tex, sky, strict):
    from example_gui_opencl_raytracer_amd import scene
    sc = scene.sphere_grid_scene(24, 24)          # 576 spheres
    flags, _ = check_self_consistent(R, api, sc, tex, sky, 160, 120, 2, 4, strict, count=3)
    assert flags & F_GRID
    flags, _ = check_self_consistent(R, api, sc, tex, sky, 160, 120, 2, 6, strict, count=3)
    assert flags & F_GRID and flags & F_DEEP


def test_high_occupancy_deep_flavour(R, api, demo_scene, tex, sky):
    """A big deep launch of the fast build takes the high-occupancy flavour (no tail): 1024x768 n = 4 at depth 6 is 196 608 virtual tiles."""
    flags, _ = check_self_consistent(R, api, demo_scene, tex, sky, 1024, 768, 4, 6, False, count=2)
    assert flags & F_OCC


# ------------------------------------------------------------------ 6. against the oracle, strict build
@pytest.mark.parametrize("W,H,n,depth", [(320, 240, 2, 4), (200, 152, 4, 4), (400, 300, 2, 15)])
def test_strict_lens_frame_is_composed_of_the_oracles_virtual_frames(R, api, oracle, demo_scene, tex, sky, W, H, n, depth):
    """The strict build differs from glibc on isolated 1-ulp sinf / cosf / powf inputs (profiles/r03_libm_divergence.jsonl), so the output
    pixels whose footprint holds a SELECTED virtual pixel at which the strict 1-sample render of that sample's camera itself differs from
    the oracle's are left out: at most 4 per configuration (the cap of tests/test_gpu_supersample.py for these sizes)."""
    from oracle.oracle_py import Camera
    base, table = make_table(api, W, H, n, LENS)
    oracle_frames = {}

    def oracle_virtual(k):
        p, f, _ = oracle.render(virtual_camera(Camera, table[k], base, n), demo_scene, tex, sky, depth, want_rgb=True)
        oracle_frames[k] = p
        return f
    want_p, want_f = composed(oracle_virtual, table, W, H, n)

    with R(demo_scene, tex, sky, n * W, n * H, depth=depth, strict=True) as r:
        def differs(k):
            r.set_camera(virtual_camera(api.clw_camera, table[k], base, n))
            return r.render() != oracle_frames[k]
        selected = pick(differs, W, H, n)
    left_out = selected.reshape(H, n, W, n).any((1, 3)).reshape(-1)
    print(f"{W}x{H} n={n} depth {depth}: {int(selected.sum())} selected virtual pixels differ from the oracle, {int(left_out.sum())} output pixels left out")
    assert left_out.sum() <= 4
    ((p, f),), flags, _ = sampled(R, demo_scene, tex, sky, W, H, n, depth, True, LENS)
    assert flags & F_SS
    keep = ~left_out
    print(f"  {int((p[keep] != want_p[keep]).sum())} kept packed pixels differ, {int((f[keep].view(np.uint32) != want_f[keep].view(np.uint32)).any(1).sum())} float")
    assert np.array_equal(p[keep], want_p[keep])


# ------------------------------------------------------------------ 7. degenerate tables
def counted_frames(R, sc, tex, sky, W, H, n, depth, strict, prepare, cam=CAM):
    with R(sc, tex, sky, W, H, depth=depth, strict=strict, supersample=n) as r:
        camera = r.look(**cam)
        prepare(r, camera)
        (p, f), = take(r)
        p2 = r.render().copy()
        flags, costs = r.w.last_trace_flags(), r.w.read_tile_costs()
        r.w.enable_counters(1)
        r.render()
        c = r.w.read_counters()
        return p, f, p2, flags, costs, [c[k] for k in COUNTED]


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("W,H,n,depth", [(200, 152, 4, 4), (400, 300, 2, 15)])
def test_degenerate_tables_give_the_plain_supersampled_frame(R, api, demo_scene, tex, sky, W, H, n, depth, strict):
    plain = counted_frames(R, demo_scene, tex, sky, W, H, n, depth, strict, lambda r, cam: None)
    ways = dict(aperture_0=lambda r, cam: r.w.set_lens(0.0, 8.0),
                copies=lambda r, cam: r.set_sample_cameras(np.tile(rows_of(cam), (n * n, 1))))
    for name, prepare in ways.items():
        got = counted_frames(R, demo_scene, tex, sky, W, H, n, depth, strict, prepare)
        assert np.array_equal(got[0], plain[0]) and same_floats(got[1], plain[1]) and np.array_equal(got[2], plain[2]), name
        assert got[3] == plain[3] and np.array_equal(got[4], plain[4]) and got[5] == plain[5], name
    # n * n copies of ANOTHER camera: that camera's plain supersampled frame
    other = api.perspective(**CAM2, width=W, height=H)
    got = counted_frames(R, demo_scene, tex, sky, W, H, n, depth, strict, lambda r, cam: r.set_sample_cameras(np.tile(rows_of(other), (n * n, 1))))
    want = counted_frames(R, demo_scene, tex, sky, W, H, n, depth, strict, lambda r, cam: None, cam=CAM2)
    assert np.array_equal(got[0], want[0]) and same_floats(got[1], want[1]) and got[5] == want[5]
    assert not np.array_equal(got[0], plain[0])


# ------------------------------------------------------------------ 8. the table a launch used; a moving camera
def test_the_launch_uses_the_host_helpers_table_under_a_moving_camera(R, api, demo_scene, tex, sky):
    W, H, n, depth = 320, 240, 2, 4
    for strict in (True, False):
        with R(demo_scene, tex, sky, W, H, depth=depth, strict=strict, supersample=n, lens=(0.1, 8.0)) as r:
            assert r.w.get_sample_cameras().shape == (0, 12)          # no launch yet
            frames = []
            for k in range(5):
                cam = dict(CAM, origin=(0.8 + 0.3 * k, 2.5, -8.0 + 0.2 * k))
                camera = r.look(**cam)
                frames.append(r.render().copy())
                assert r.w.get_sample_cameras().tobytes() == api.lens_cameras(camera, 0.1, 8.0, n).tobytes(), k
                fresh = sampled(R, demo_scene, tex, sky, W, H, n, depth, strict, (0.1, 8.0), cam=cam, rgb=False)[0][0][0]
                assert np.array_equal(frames[-1], fresh), (strict, k)
        assert not np.array_equal(frames[0], frames[1])


# ------------------------------------------------------------------ 9. strips, pipelined read-back
@pytest.mark.parametrize("n", [2, 4])
def test_row_strips_compose(R, demo_scene, tex, sky, n):
    from example_gui_opencl_raytracer_amd.renderer import strip_rows
    W, H, depth = 400, 300, 4
    for strict in (True, False):
        full = sampled(R, demo_scene, tex, sky, W, H, n, depth, strict, LENS, rgb=False)[0][0][0]
        plain = sampled(R, demo_scene, tex, sky, W, H, n, depth, strict, None, rgb=False)[0][0][0]
        assert not np.array_equal(full, plain)
        parts = []
        for rank in range(3):
            r0, rows = strip_rows(H, 3, rank)
            part = sampled(R, demo_scene, tex, sky, W, H, n, depth, strict, LENS, rgb=False, first_row=r0, rows=rows)[0][0][0]
            assert part.shape == (rows * W,)
            parts.append(part)
        assert np.array_equal(np.concatenate(parts), full)


def test_pipelined_readback_returns_the_same_frame(R, demo_scene, tex, sky):
    W, H, n, depth = 2048, 2048, 2, 2
    outs = []
    for on in (1, 0):
        got, _, _ = sampled(R, demo_scene, tex, sky, W, H, n, depth, False, LENS, count=2, rgb=False, setup=lambda w: w.set_pipeline(on))
        outs.append((got[0][0], got[1][0]))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][0], outs[0][1])
    plain = sampled(R, demo_scene, tex, sky, W, H, n, depth, False, None, rgb=False)[0][0][0]
    assert not np.array_equal(outs[0][0], plain)


# ------------------------------------------------------------------ 10. changing everything between frames of one wrapper
def test_changing_aperture_focus_table_and_factor_between_frames(R, api, demo_scene, tex, sky):
    W, H, depth = 160, 120, 15
    for strict in (True, False):
        steps = [(2, (0.2, 8.0)), (2, (0.2, 8.0)), (2, (0.05, 8.0)), (2, (0.05, 4.0)), (4, (0.05, 4.0)), (4, "shutter"), (4, "shutter"), (4, None), (2, None),
                 (2, "shutter"), (2, (0.2, 8.0)), (1, None), (1, None), (8, (0.2, 8.0)), (2, (0.2, 8.0))]
        want = {}
        for n, kind in set(steps):
            table = make_table(api, W, H, n, kind)[1] if kind == "shutter" else None
            want[(n, kind)] = sampled(R, demo_scene, tex, sky, W, H, n, depth, strict, kind, table=table, rgb=False)[0][0][0]
        with rendering(R, demo_scene, tex, sky, W, H, depth=depth, strict=strict) as r:
            for n, kind in steps:
                r.w.set_supersample(n)
                if kind == "shutter":
                    r.set_sample_cameras(make_table(api, W, H, n, kind)[1])
                elif kind is None:
                    r.w.set_lens(0.0, 1.0)
                    r.set_sample_cameras(None)
                else:
                    r.w.set_lens(*kind)
                assert np.array_equal(r.render(), want[(n, kind)]), (strict, n, kind)
        assert len({v.tobytes() for v in want.values()}) == len(want)


def test_tables_that_change_under_queued_launches(R, demo_scene, tex, sky):
    """Asynchronous launches on a caller's stream into a torch-owned framebuffer, the lens changed after every launch and nothing waited for
    until the end (the frames are copied aside in stream order): every copy holds the frame of the table its launch was given."""
    import torch
    W, H, n, depth = 640, 480, 2, 4
    lenses = [(0.05, 8.0), (0.2, 8.0), (0.1, 4.0), (0.2, 8.0), (0.2, 8.0), (0.05, 8.0), (0.3, 6.0)]
    want = {l: sampled(R, demo_scene, tex, sky, W, H, n, depth, False, l, rgb=False)[0][0][0] for l in set(lenses)}
    assert len({v.tobytes() for v in want.values()}) == len(want)
    fb = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with rendering(R, demo_scene, tex, sky, W, H, setup=queued_on(side), depth=depth, supersample=n, framebuffer_ptr=fb.data_ptr()) as r:
        outs = []
        for lens in lenses:
            r.w.set_lens(*lens)
            r.render(readback=False)
            with torch.cuda.stream(side):
                outs.append(fb.clone())
        side.synchronize()
        for k, lens in enumerate(lenses):
            assert np.array_equal(outs[k].cpu().numpy().view(np.uint32), want[lens]), (k, lens)


def test_changing_the_stream_between_lens_frames(R, demo_scene, tex, sky):
    """The table was written in the order of the stream that was current then: a launch on another stream still reads the right one."""
    import torch
    W, H, n, depth = 320, 240, 2, 4
    want = {a: sampled(R, demo_scene, tex, sky, W, H, n, depth, True, (a, 8.0), rgb=False)[0][0][0] for a in (0.05, 0.2)}
    side = torch.cuda.Stream()
    with rendering(R, demo_scene, tex, sky, W, H, depth=depth, strict=True, supersample=n, lens=(0.05, 8.0)) as r:
        for stream, aperture in ((0, 0.05), (side.cuda_stream, 0.05), (side.cuda_stream, 0.2), (0, 0.2), (0, 0.05), (side.cuda_stream, 0.2), (0, 0.2)):
            r.w.set_stream(stream)
            r.w.set_lens(aperture, 8.0)
            assert np.array_equal(r.render(), want[aperture]), (stream != 0, aperture)


# ------------------------------------------------------------------ 11. the reference's own driver, unchanged
REF_RAYPNG = os.path.join(ROOT, "oracle", "_ref", "raypng_hip")


@pytest.mark.skipif(not os.path.exists(REF_RAYPNG), reason="oracle/_ref/raypng_hip not built (needs the reference's sources)")
def test_unchanged_raypng_driver_gets_the_lens_from_the_environment(R, api, tmp_path):
    import shutil
    from example_gui_opencl_raytracer_amd.scene import Scene
    FIX = os.path.join(ROOT, "tests", "golden", "reference_scene")
    names = ("cobblestone", "sand", "check", "grass")
    for d in ("scenes", "assets/bg", "out"):
        os.makedirs(tmp_path / d)
    shutil.copy(os.path.join(FIX, "render.map"), tmp_path / "scenes" / "render.map")
    for nm in names:
        shutil.copy(os.path.join(FIX, nm + ".png"), tmp_path / "assets" / (nm + ".png"))
    shutil.copy(os.path.join(FIX, "stormydays.png"), tmp_path / "assets" / "bg" / "stormydays.png")

    def driver(**env):
        p = subprocess.run([REF_RAYPNG], cwd=tmp_path, env=dict(os.environ, CLWRAP_SUPERSAMPLE="2", CLWRAP_STRICT="1", **env), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "Done, took:" in p.stdout, p.stdout + p.stderr
        img = api.read_png(str(tmp_path / "out" / "scene.png"))
        assert img.shape == (600, 800, 4)
        return (img[..., 0].astype(np.uint32) << 16 | img[..., 1].astype(np.uint32) << 8 | img[..., 2]).reshape(-1)
    got = driver(CLWRAP_APERTURE="0.1", CLWRAP_FOCUS="8")
    with rendering(R, Scene.load(os.path.join(FIX, "render.map")), None, None, 800, 600, depth=15, strict=True, supersample=2, lens=(0.1, 8),
                   texture_paths=[os.path.join(FIX, nm + ".png") for nm in names], skybox_path=os.path.join(FIX, "stormydays.png")) as r:
        want = r.render().copy()
    assert np.array_equal(got, want), int((got != want).sum())
    assert not np.array_equal(driver(), got)          # and it is not the frame without the lens


# ------------------------------------------------------------------ 12. refusals: message + exit(1)
def _run(snippet, env=None):
    return run_child("table = lambda n: api.lens_cameras(api.perspective(**CAM, width=64, height=48), 0.1, 8.0, n)\n" + snippet, env)


REFUSED = {
    "count_16_with_factor_2": "r = Renderer(sc, tex, sky, 64, 48, depth=2, supersample=2); r.set_sample_cameras(table(4)); r.look(**CAM); r.render()",
    "count_4_with_factor_4": "r = Renderer(sc, tex, sky, 64, 48, depth=2, supersample=4); r.set_sample_cameras(table(2)); r.look(**CAM); r.render()",
    "count_3_with_factor_2": "r = Renderer(sc, tex, sky, 64, 48, depth=2, supersample=2); r.set_sample_cameras(table(2)[:3]); r.look(**CAM); r.render()",
    "table_with_factor_1": "r = Renderer(sc, tex, sky, 64, 48, depth=2); r.set_sample_cameras(table(2)); r.look(**CAM); r.render()",
    "one_camera_with_factor_1": "r = Renderer(sc, tex, sky, 64, 48, depth=2); r.set_sample_cameras(table(2)[:1]); r.look(**CAM); r.render()",
    "lens_with_factor_1": "r = Renderer(sc, tex, sky, 64, 48, depth=2, lens=(0.1, 8.0)); r.look(**CAM); r.render()",
    "lens_on_the_two_kernel_path": "r = Renderer(sc, tex, sky, 64, 48, depth=2, fuse=False, supersample=2, lens=(0.1, 8.0)); r.look(**CAM); r.render()",
    "negative_aperture": "w = api.ClWrap(); w.set_lens(-0.1, 8.0)",
    "nan_aperture": "w = api.ClWrap(); w.set_lens(float('nan'), 8.0)",
    "infinite_aperture": "w = api.ClWrap(); w.set_lens(float('inf'), 8.0)",
    "focus_0": "w = api.ClWrap(); w.set_lens(0.1, 0.0)",
    "negative_focus": "w = api.ClWrap(); w.set_lens(0.1, -2.0)",
    "nan_focus": "w = api.ClWrap(); w.set_lens(0.0, float('nan'))",
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_unsupported_combinations_exit_with_a_message(case):
    p = _run(REFUSED[case] + "\nprint('unreachable')")
    assert p.returncode == 1 and "ERROR:\t" in p.stdout and "unreachable" not in p.stdout, p.stdout + p.stderr


@pytest.mark.parametrize("name,value", [("CLWRAP_APERTURE", "-0.5"), ("CLWRAP_APERTURE", "nan"), ("CLWRAP_APERTURE", "wide"), ("CLWRAP_FOCUS", "0"),
                                        ("CLWRAP_FOCUS", "-3"), ("CLWRAP_FOCUS", "inf")])
def test_bad_environment_value_exits(name, value):
    p = _run("api.ClWrap()\nprint('unreachable')", env=dict(os.environ, **{name: value}))
    assert p.returncode == 1 and "ERROR:\t" in p.stdout and name in p.stdout and "unreachable" not in p.stdout, p.stdout + p.stderr


def test_good_environment_values_are_taken(R, demo_scene, tex, sky):
    code = ("r = Renderer(sc, tex, sky, 64, 48, depth=2, supersample=2); cam = r.look(**CAM); r.render()\n"
            "assert r.w.get_sample_cameras().tobytes() == api.lens_cameras(cam, 0.25, 6.0, 2).tobytes()\nprint('lens taken')")
    p = _run(code, env=dict(os.environ, CLWRAP_APERTURE="0.25", CLWRAP_FOCUS="6"))
    assert p.returncode == 0 and "lens taken" in p.stdout, p.stdout + p.stderr


# ------------------------------------------------------------------ 13. defaults untouched
@pytest.mark.parametrize("W,H,depth", [(1280, 720, 4), (800, 600, 15)])
def test_aperture_zero_and_no_table_set_explicitly_are_the_default(R, demo_scene, tex, sky, W, H, depth):
    for strict in (False, True):
        for n in (1, 2):
            res = []
            for explicit in (False, True):
                def prepare(r, cam):
                    if explicit:
                        r.w.set_lens(0.0, 1.0)
                        r.set_sample_cameras(None)
                res.append(counted_frames(R, demo_scene, tex, sky, W, H, n, depth, strict, prepare))
                assert bool(res[-1][3] & F_SS) == (n > 1)
            a, b = res
            assert np.array_equal(a[0], b[0]) and same_floats(a[1], b[1]) and np.array_equal(a[2], b[2])
            assert a[3] == b[3] and np.array_equal(a[4], b[4]) and a[5] == b[5]
