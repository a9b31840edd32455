"""In-kernel n x n supersampling (clw_ext_set_supersample, Renderer(supersample=n)) on a real GPU.

The definition every test uses: sub-sample (sx, sy) of output pixel (x, y) is pixel (n x + sx, n y + sy) of the n*W x n*H frame the same
camera gives, traced exactly as a 1-sample launch of that frame traces it; the samples are clamped to [0, 1], added in float32 -- adjacent
pairs along x (log2 n rounds), then adjacent pairs along y -- scaled by 1 / n^2 and packed like any pixel: render_common.resolve."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import CAM, ROOT
from flags_common import F_DEEP, F_GRID, F_OCC, F_SHAPE, F_SS
from render_common import R, assert_same_frames, frames, released, rendering, resolve, run_child, same_floats, take  # noqa: F401  (R: the fixture)

pytestmark = pytest.mark.gpu


def check_self_consistent(R, sc, tex, sky, W, H, n, depth, strict, count=1, setup=None):
    """supersampled frame(s) == resolve(the GPU's own 1-sample render of n*W x n*H); -> flags of the supersampled launch"""
    (virt,), vflags = frames(R, sc, tex, sky, n * W, n * H, depth, strict, setup=setup)
    want_p, want_f = resolve(virt[1], W, H, n)
    got, flags = frames(R, sc, tex, sky, W, H, depth, strict, n=n, count=count, setup=setup)
    assert flags & F_SS and not vflags & F_SS
    for p, f in got:
        assert p.shape == (W * H,) and f.shape == (W * H, 3)
    assert_same_frames(got, want_p, want_f, f"{W}x{H} n={n} depth {depth} strict={int(strict)}")
    return flags


# ------------------------------------------------------------------ the setter
def test_get_returns_what_set_and_the_environment_set():
    from example_gui_opencl_raytracer_amd import api
    with released(api.ClWrap()) as w:
        assert w.get_supersample() == 1
        for n in (2, 4, 8, 1):
            w.set_supersample(n)
            assert w.get_supersample() == n
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from example_gui_opencl_raytracer_amd import api\n"
            "w = api.ClWrap(); print('supersample', w.get_supersample()); w.release()\n" % ROOT)
    for n in ("1", "2", "4", "8"):
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, CLWRAP_SUPERSAMPLE=n), timeout=300)
        assert p.returncode == 0 and f"supersample {n}" in p.stdout, p.stdout + p.stderr


# ------------------------------------------------------------------ 1. self-consistency, exact, both builds
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("W,H,n", [(320, 240, 2), (200, 152, 4), (96, 64, 8), (101, 75, 2)])
def test_shallow_frame_is_the_resolve_of_the_gpus_own_virtual_frame(R, demo_scene, tex, sky, W, H, n, strict):
    flags = check_self_consistent(R, demo_scene, tex, sky, W, H, n, 4, strict)
    assert not flags & F_DEEP
    if not strict:
        assert flags & F_SHAPE          # the shaped shallow kernel of the fast build really ran supersampled


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("W,H,n", [(400, 300, 2), (96, 64, 8)])
def test_deep_frames_are_the_resolve_of_the_gpus_own_virtual_frame(R, demo_scene, tex, sky, W, H, n, strict):
    """Three frames in a row: the second and third run with the cost-sorted order and (n < 8) split heavy tiles."""
    flags = check_self_consistent(R, demo_scene, tex, sky, W, H, n, 15, strict, count=3)
    assert flags & F_DEEP and not flags & F_OCC


# ------------------------------------------------------------------ 2. against the oracle, strict build
@pytest.mark.parametrize("W,H,n,depth", [(320, 240, 2, 4), (200, 152, 4, 4), (96, 64, 8, 4), (101, 75, 2, 4), (400, 300, 2, 15)])
def test_strict_frame_is_the_resolve_of_the_oracles_virtual_frame(R, oracle, demo_scene, tex, sky, W, H, n, depth):
    """The strict build differs from glibc on isolated 1-ulp sinf / cosf / powf inputs (profiles/r03_libm_divergence.jsonl), so the output
    pixels whose footprint holds a virtual pixel where the strict 1-sample virtual frame itself differs from the oracle's are left out: at
    most 4 per configuration.  The frames are the packed ones; how far the float radiance agrees is printed."""
    cam = oracle.camera(CAM["origin"], CAM["look"], CAM["fov"], CAM["focal"], n * W, n * H)
    want_virt_p, want_virt_f, _ = oracle.render(cam, demo_scene, tex, sky, depth, want_rgb=True)
    want_p, want_f = resolve(want_virt_f, W, H, n)
    (virt,), _ = frames(R, demo_scene, tex, sky, n * W, n * H, depth, True)
    differs = virt[0] != want_virt_p
    clamped = lambda a: np.clip(a, np.float32(0), np.float32(1))
    print(f"{W}x{H} n={n} depth {depth}: clamped float radiance of {int((clamped(virt[1]) != clamped(want_virt_f)).any(1).sum())} virtual pixels differs from the oracle's")
    left_out = differs.reshape(H, n, W, n).any((1, 3)).reshape(-1)
    print(f"{W}x{H} n={n} depth {depth}: {int(differs.sum())} virtual pixels differ from the oracle, {int(left_out.sum())} output pixels left out")
    assert left_out.sum() <= 4
    ((p, f),), flags = frames(R, demo_scene, tex, sky, W, H, depth, True, n=n)
    assert flags & F_SS
    keep = ~left_out
    print(f"  {int((p[keep] != want_p[keep]).sum())} kept packed pixels differ, {int((f[keep].view(np.uint32) != want_f[keep].view(np.uint32)).any(1).sum())} float")
    assert np.array_equal(p[keep], want_p[keep])


# ------------------------------------------------------------------ 3. other flavours
def test_glass_field(R, tex, sky):
    from example_gui_opencl_raytracer_amd import scene
    for strict in (True, False):
        flags = check_self_consistent(R, scene.dielectric_field_scene(), tex, sky, 256, 256, 2, 8, strict, count=3)
        assert flags & F_DEEP


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_uniform_grid_scene(R, tex, sky, strict):
    from example_gui_opencl_raytracer_amd import scene
    sc = scene.sphere_grid_scene(24, 24)          # 576 spheres
    flags = check_self_consistent(R, sc, tex, sky, 160, 120, 2, 4, strict, count=3)
    assert flags & F_GRID
    flags = check_self_consistent(R, sc, tex, sky, 160, 120, 2, 6, strict, count=3)
    assert flags & F_GRID and flags & F_DEEP


def test_tail_wide_tail_off_and_split_off_give_the_same_frame(R, demo_scene, tex, sky):
    W, H, n, depth = 400, 300, 2, 15
    for strict in (True, False):
        (virt,), _ = frames(R, demo_scene, tex, sky, n * W, n * H, depth, strict)
        want_p, want_f = resolve(virt[1], W, H, n)
        ways = dict(default=None, tail_wide=lambda w: w.set_tpt(64), tail_off=lambda w: w.set_tpt(0), split_off=lambda w: w.set_variant(4096),
                    unsorted=lambda w: w.set_tile_sched(0))
        for name, setup in ways.items():
            got, flags = frames(R, demo_scene, tex, sky, W, H, depth, strict, n=n, count=3, setup=setup)
            assert flags & F_DEEP and flags & F_SS
            for k, (p, f) in enumerate(got):
                assert np.array_equal(p, want_p) and same_floats(f, want_f), (name, strict, k, int((p != want_p).sum()))


def test_high_occupancy_deep_flavour(R, demo_scene, tex, sky):
    """A big deep launch of the fast build takes the high-occupancy flavour (no tail): 1024x768 n = 4 at depth 6 is 196 608 virtual tiles."""
    W, H, n, depth = 1024, 768, 4, 6
    (virt,), vflags = frames(R, demo_scene, tex, sky, n * W, n * H, depth, False)
    want_p, want_f = resolve(virt[1], W, H, n)
    got, flags = frames(R, demo_scene, tex, sky, W, H, depth, False, n=n, count=2)
    assert flags & F_OCC and vflags & F_OCC and flags & F_SS
    for p, f in got:
        assert np.array_equal(p, want_p) and same_floats(f, want_f)


def test_counters_and_tile_costs_describe_the_virtual_frame(R, demo_scene, tex, sky):
    W, H, n = 200, 152, 2
    for depth in (4, 15):
        res = []
        for (w, h, k) in ((W, H, n), (n * W, n * H, 1)):
            with rendering(R, demo_scene, tex, sky, w, h, depth=depth, strict=True, supersample=k) as r:
                r.w.enable_counters(1)
                r.render()
                c = r.w.read_counters()
                costs = r.w.read_tile_costs()
            res.append(({x: c[x] for x in ("segments", "shadow_rays", "sky_fetches", "texel_fetches", "pushes")}, costs))
        assert res[0][0] == res[1][0] and res[0][0]["segments"] >= n * n * W * H
        assert len(res[0][1]) == ((n * W + 7) // 8) * ((n * H + 7) // 8) and np.array_equal(res[0][1], res[1][1])


def test_changing_the_factor_between_frames(R, demo_scene, tex, sky):
    """The cost / order buffers follow the virtual tile grid: one wrapper, factor changed between frames of a deep launch."""
    from example_gui_opencl_raytracer_amd.renderer import Renderer
    W, H, depth = 160, 120, 15
    want = {n: frames(R, demo_scene, tex, sky, W, H, depth, True, n=n, rgb=False)[0][0][0] for n in (1, 2, 4, 8)}
    with rendering(Renderer, demo_scene, tex, sky, W, H, depth=depth, strict=True) as r:
        for n in (2, 2, 2, 8, 8, 1, 1, 4, 4, 4, 2):
            r.w.set_supersample(n)
            assert np.array_equal(r.render(), want[n]), n
    assert not np.array_equal(want[1], want[2])


# ------------------------------------------------------------------ 4. strips
@pytest.mark.parametrize("n", [2, 4])
def test_row_strips_compose(R, demo_scene, tex, sky, n):
    from example_gui_opencl_raytracer_amd.renderer import strip_rows
    W, H, depth = 400, 300, 4
    for strict in (True, False):
        full = frames(R, demo_scene, tex, sky, W, H, depth, strict, n=n, rgb=False)[0][0][0]
        parts = []
        for rank in range(3):
            r0, rows = strip_rows(H, 3, rank)
            with rendering(R, demo_scene, tex, sky, W, H, depth=depth, strict=strict, first_row=r0, rows=rows, supersample=n) as r:
                parts.append(r.render().copy())
                assert parts[-1].shape == (rows * W,)
        assert np.array_equal(np.concatenate(parts), full)


def test_pipelined_readback_returns_the_same_frame(R, demo_scene, tex, sky):
    W, H, n, depth = 2048, 2048, 2, 2
    outs = []
    for on in (1, 0):
        with rendering(R, demo_scene, tex, sky, W, H, setup=lambda w: w.set_pipeline(on), depth=depth, supersample=n) as r:
            (a, _), (b, _) = take(r, 2, rgb=False)
            outs.append((a, b))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][0], outs[0][1])


def test_ray_buffer_keeps_its_one_ray_per_pixel_meaning(R, demo_scene, tex, sky):
    W, H = 96, 64
    rays = []
    for n in (1, 2):
        with rendering(R, demo_scene, tex, sky, W, H, depth=2, supersample=n) as r:
            r.render()
            rays.append(r.read_rays().copy())
    assert rays[0].shape == (W * H, 16) and np.array_equal(rays[0], rays[1])


# ------------------------------------------------------------------ 5. the reference's own driver, unchanged
REF_RAYPNG = os.path.join(ROOT, "oracle", "_ref", "raypng_hip")


@pytest.mark.skipif(not os.path.exists(REF_RAYPNG), reason="oracle/_ref/raypng_hip not built (needs /root/reference)")
def test_unchanged_raypng_driver_is_supersampled_by_the_environment(R, tmp_path):
    import shutil
    from example_gui_opencl_raytracer_amd import api
    from example_gui_opencl_raytracer_amd.scene import Scene
    FIX = os.path.join(ROOT, "tests", "golden", "reference_scene")
    names = ("cobblestone", "sand", "check", "grass")
    for d in ("scenes", "assets/bg", "out"):
        os.makedirs(tmp_path / d)
    shutil.copy(os.path.join(FIX, "render.map"), tmp_path / "scenes" / "render.map")
    for nm in names:
        shutil.copy(os.path.join(FIX, nm + ".png"), tmp_path / "assets" / (nm + ".png"))
    shutil.copy(os.path.join(FIX, "stormydays.png"), tmp_path / "assets" / "bg" / "stormydays.png")
    env = dict(os.environ, CLWRAP_SUPERSAMPLE="2", CLWRAP_STRICT="1")
    p = subprocess.run([REF_RAYPNG], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "Done, took:" in p.stdout, p.stdout + p.stderr
    img = api.read_png(str(tmp_path / "out" / "scene.png"))
    assert img.shape == (600, 800, 4)
    got = (img[..., 0].astype(np.uint32) << 16 | img[..., 1].astype(np.uint32) << 8 | img[..., 2]).reshape(-1)
    with rendering(R, Scene.load(os.path.join(FIX, "render.map")), None, None, 800, 600, depth=15, strict=True, supersample=2,
                   texture_paths=[os.path.join(FIX, nm + ".png") for nm in names], skybox_path=os.path.join(FIX, "stormydays.png")) as r:
        want = r.render().copy()
    assert np.array_equal(got, want), int((got != want).sum())
    # and it is not the 1-sample frame
    env1 = dict(os.environ, CLWRAP_STRICT="1")
    p = subprocess.run([REF_RAYPNG], cwd=tmp_path, env=env1, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    img1 = api.read_png(str(tmp_path / "out" / "scene.png"))
    assert not np.array_equal(img1, img)


# ------------------------------------------------------------------ 6. refusals: message + exit(1)
_run = run_child


REFUSED = {
    "two_kernel_path": "r = Renderer(sc, tex, sky, 64, 48, depth=2, fuse=False, supersample=2); r.look(**CAM); r.render()",
    "caller_written_rays": ("r = Renderer(sc, tex, sky, 64, 48, depth=2, supersample=2); r.look(**CAM); r.w.output(r.pixels, 0, 0, 0, 0, None)\n"
                            "r.w.device_ptr(0, 8)\nr.w.output(r.pixels, 0, 1, 1, 10, None)"),
    "not_whole_rows": ("r = Renderer(sc, tex, sky, 64, 48, depth=2, supersample=2); r.look(**CAM); r.w.output(r.pixels, 0, 0, 0, 0, None)\n"
                       "r.w.load_single_data(1, 7, np.uint32(64 * 10 + 32))\nr.w.output(r.pixels, 0, 1, 1, 10, None)"),
    "id_offset_inside_a_row": ("r = Renderer(sc, tex, sky, 64, 48, depth=2, supersample=2); r.look(**CAM); r.w.set_id_offset(32)\n"
                               "r.w.load_single_data(1, 7, np.uint32(64 * 10)); r.w.output(64 * 10, 0, 0, 0, 0, None)\nr.w.output(64 * 10, 0, 1, 1, 10, None)"),
    "row_bands": "r = Renderer(sc, tex, sky, 64, 48, depth=2, bands=(2, 1), supersample=2); r.look(**CAM); r.render()",
    "linear_ids": "r = Renderer(sc, tex, sky, 64, 48, depth=2, supersample=2); r.w.set_variant(2); r.look(**CAM); r.render()",
    "ids_beyond_32_bits": "r = Renderer(sc, tex, sky, 8192, 8192, depth=1, supersample=8); r.look(**CAM); r.render(readback=False)",
    "factor_3": "w = api.ClWrap(); w.set_supersample(3)",
    "factor_16": "w = api.ClWrap(); w.set_supersample(16)",
    "factor_0": "w = api.ClWrap(); w.set_supersample(0)",
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_unsupported_combinations_exit_with_a_message(case):
    p = _run(REFUSED[case] + "\nprint('unreachable')")
    assert p.returncode == 1 and "ERROR:\t" in p.stdout and "upersampl" in p.stdout and "unreachable" not in p.stdout, p.stdout + p.stderr


@pytest.mark.parametrize("value", ["3", "16", "0", "-2"])
def test_bad_environment_value_exits(value):
    p = _run("api.ClWrap()\nprint('unreachable')", env=dict(os.environ, CLWRAP_SUPERSAMPLE=value))
    assert p.returncode == 1 and "ERROR:\t" in p.stdout and "CLWRAP_SUPERSAMPLE" in p.stdout and "unreachable" not in p.stdout, p.stdout + p.stderr


# ------------------------------------------------------------------ 7. default untouched
@pytest.mark.parametrize("W,H,depth", [(1280, 720, 4), (800, 600, 15)])
def test_factor_one_set_explicitly_is_the_default(R, demo_scene, tex, sky, W, H, depth):
    from example_gui_opencl_raytracer_amd.renderer import Renderer
    for strict in (False, True):
        res = []
        for explicit in (False, True):
            with rendering(Renderer, demo_scene, tex, sky, W, H, setup=(lambda w: w.set_supersample(1)) if explicit else None, depth=depth, strict=strict) as r:
                (frame, _), (frame2, _) = take(r, 2, rgb=False)
                flags = r.w.last_trace_flags()
                costs = r.w.read_tile_costs()
                r.w.enable_counters(1)
                r.render()
                c = r.w.read_counters()
            res.append((frame, frame2, costs, [c[k] for k in ("segments", "shadow_rays", "light_probes", "sky_fetches", "texel_fetches", "pushes")], flags))
        assert not res[0][4] & F_SS and res[0][4] == res[1][4]
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
        assert np.array_equal(res[0][2], res[1][2]) and res[0][3] == res[1][3]
