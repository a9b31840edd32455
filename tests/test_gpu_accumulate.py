"""The seed offset (clw_ext_set_seed_offset) and progressive frame accumulation (clw_ext_set_accumulate, Renderer(accumulate=N)) on a real GPU.

Everything is bit-exact.  A frame with seed offset s is the oracle's frame traced with ids shifted by s (strict build), and the same frame on
every launch path.  Frame K-1 of an accumulated view is `accumulate_common.fold` of K plain frames -- the GPU's own, each rendered by a fresh
renderer with the mode off, seed offset frame_seed(f) and camera jitter_camera(cam, f, n), or the oracle's (strict build)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from accumulate_common import accumulated, base_camera, fold, jittered, own_frames, plain
from conftest import CAM, ROOT
from render_common import R, api, released, rendering, resolve, run_child, take  # noqa: F401  (R, api: the fixtures)
from sample_cameras_common import rows_of, virtual_camera

pytestmark = pytest.mark.gpu

SEEDS = [1, 0x9E3779B1, 2 ** 32 - 5]          # the last makes in-frame pixel 5 the stuck generator
# (W, H, n, depth): partial tiles both ways; the supersampled resolves; the deep build (cost-sorted order, split tiles, the tail) on three lights and glass
SHAPES = [(101, 75, 1, 4), (96, 64, 2, 4), (64, 48, 4, 4), (96, 64, 1, 15)]


def oracle_frame(oracle, cam, sc, tex, sky, depth, seed):
    """the oracle's rays of `cam` traced with ids (RNG seeds) shifted by `seed` -> (packed, float radiance)"""
    from oracle.oracle_py import Counters, _Inputs, _p
    rays = oracle.raygen(cam)
    inp = _Inputs(sc, tex, sky)
    n = rays.shape[0]
    out, rgb, cnt = np.zeros(n, np.uint32), np.zeros((n, 3), np.float32), Counters()
    assert oracle.lib.wo_trace_rays(_p(rays), C.byref(inp.c), depth, seed, seed + n, _p(out), _p(rgb), C.byref(cnt), 0) == 0
    return out, rgb


# ------------------------------------------------------------------ 1. the seed offset, strict, against the oracle
@pytest.mark.parametrize("W,H,depth", [(101, 75, 4), (96, 64, 15)])
def test_seed_offset_is_the_oracles_shifted_ids(R, api, oracle, demo_scene, tex, sky, W, H, depth):
    cam = base_camera(api, W, H)
    ocam = oracle.camera(CAM["origin"], CAM["look"], 90.0, 1.0, W, H)
    rays = oracle.raygen(ocam)
    zero, _ = plain(R, demo_scene, tex, sky, W, H, depth, True, cam)
    explicit, _ = plain(R, demo_scene, tex, sky, W, H, depth, True, cam, seed=0, setup=lambda w: w.set_seed_offset(0))
    want0, _ = oracle.trace_rays(rays, demo_scene, tex, sky, depth)
    assert np.array_equal(zero, want0) and np.array_equal(explicit, zero)
    for s in SEEDS:
        got, _ = plain(R, demo_scene, tex, sky, W, H, depth, True, cam, seed=s)
        want, _ = oracle.trace_rays(rays, demo_scene, tex, sky, depth, id_begin=s)
        print(f"{W}x{H} depth {depth} seed offset {s:#x}: {int((got != want).sum())} pixels differ from the oracle, {int((got != zero).sum())} from offset 0")
        assert np.array_equal(got, want), s
        if s == 1:
            assert not np.array_equal(got, zero)              # the offset is not a no-op


def test_seed_offset_get_returns_what_set(api):
    with released(api.ClWrap()) as w:
        assert w.get_seed_offset() == 0 and w.get_accumulated() == 0
        for s in (1, 0x9E3779B1, 2 ** 32 - 1, 0):
            w.set_seed_offset(s)
            assert w.get_seed_offset() == s


# ------------------------------------------------------------------ 2. the offset reaches every path, both builds
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_seed_offset_reaches_every_path(R, api, demo_scene, tex, sky, strict):
    W, H, s = 96, 64, 0x9E3779B1
    cam = base_camera(api, W, H)
    for depth in (4, 15):
        want, _ = plain(R, demo_scene, tex, sky, W, H, depth, strict, cam, seed=s)
        unseeded, _ = plain(R, demo_scene, tex, sky, W, H, depth, strict, cam)
        assert not np.array_equal(want, unseeded)
        two, _ = plain(R, demo_scene, tex, sky, W, H, depth, strict, cam, seed=s, fuse=False)
        linear, _ = plain(R, demo_scene, tex, sky, W, H, depth, strict, cam, seed=s, setup=lambda w: w.set_variant(2))
        assert np.array_equal(two, want) and np.array_equal(linear, want), depth
        bands = [plain(R, demo_scene, tex, sky, W, H, depth, strict, cam, seed=s, bands=(2, k))[0].reshape(-1, 8 * W) for k in range(2)]
        full = want.reshape(H // 8, 8 * W)
        assert np.array_equal(bands[0], full[0::2]) and np.array_equal(bands[1], full[1::2]), depth
        strips = [plain(R, demo_scene, tex, sky, W, H, depth, strict, cam, seed=s, first_row=r0, rows=32)[0] for r0 in (0, 32)]
        assert np.array_equal(np.concatenate(strips), want), depth
    loop, _ = plain(R, demo_scene, tex, sky, W, H, 15, strict, cam, seed=s, setup=lambda w: w.set_variant(16))
    assert np.array_equal(loop, want)
    through_the_tail = lambda w: w.set_tpt(64, 1, -1)         # everything through the tail (as tests/test_gpu_parity.py forces it)
    with rendering(R, demo_scene, tex, sky, W, H, setup=through_the_tail, cam=cam, depth=15, strict=strict, seed_offset=s) as r:
        tail = r.render().copy()
        r.w.enable_counters(1)                               # the counting flavour of the same launch tells whether the tail ran
        counted = r.render().copy()
        c = r.w.read_counters()
    assert c["tpt_tiles"] > 0 and c["tpt_nodes"] > 0, "the tail did not run"
    assert np.array_equal(tail, want) and np.array_equal(counted, want)


def test_the_strict_twins_that_carry_the_seed_and_the_sum(R, api, demo_scene, tex, sky):
    """The strict build's shallow counting and grid kernels read the seed offset and accumulate only as their WT_F_ACC twin (1 << 20): same
    frames as the kernels that carry both unflagged, and no twin while the offset is 0 and the mode off."""
    from example_gui_opencl_raytracer_amd import scene
    from flags_common import F_COUNT, F_GRID, F_ACC
    W, H, depth, s = 96, 64, 4, 0x9E3779B1
    cam = base_camera(api, W, H)
    flags = {}

    def one(sc, name, acc=0, seed=0, setup=None):
        with rendering(R, sc, tex, sky, W, H, setup=setup, cam=cam, depth=depth, strict=True, seed_offset=seed, accumulate=acc) as r:
            frames = take(r, max(acc, 1), rgb=False)
            flags[name] = r.w.last_trace_flags()
            return frames[-1][0]

    on = lambda w: w.enable_counters(1)
    assert np.array_equal(one(demo_scene, "count_seed", seed=s, setup=on), one(demo_scene, "seed", seed=s))
    assert np.array_equal(one(demo_scene, "count_acc", acc=3, setup=on), one(demo_scene, "acc", acc=3))
    one(demo_scene, "count", setup=on)
    assert flags["count_seed"] & F_ACC and flags["count_acc"] & F_ACC and flags["count"] & F_COUNT and not flags["count"] & F_ACC
    assert not flags["seed"] & F_ACC and not flags["acc"] & F_ACC
    big = scene.sphere_grid_scene(20, 20)                       # 400 spheres: the uniform grid
    linear = lambda w: w.set_variant(8)
    assert np.array_equal(one(big, "grid_seed", seed=s), one(big, "linear_seed", seed=s, setup=linear))
    assert np.array_equal(one(big, "grid_acc", acc=3), one(big, "linear_acc", acc=3, setup=linear))
    assert not np.array_equal(one(big, "grid"), one(big, "grid_seed", seed=s))
    assert flags["grid_seed"] & F_ACC and flags["grid_acc"] & F_ACC and flags["grid"] & F_GRID and not flags["grid"] & F_ACC
    assert not flags["linear_seed"] & (F_ACC | F_GRID)


# ------------------------------------------------------------------ 3. accumulation is the fold of the GPU's own frames, both builds
@pytest.mark.parametrize("jitter", [True, False], ids=["jitter", "still"])
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("W,H,n,depth", SHAPES)
def test_accumulated_frame_is_the_fold_of_the_gpus_own_frames(R, api, demo_scene, tex, sky, W, H, n, depth, strict, jitter):
    K = 5
    own = own_frames(R, api, demo_scene, tex, sky, W, H, n, depth, strict, jitter, K)
    got = accumulated(R, api, demo_scene, tex, sky, W, H, n, depth, strict, jitter, K)
    assert not np.array_equal(own[1][0], own[0][0])             # frame 1 is a frame of its own
    for k, (p, f, count) in enumerate(got, start=1):
        want_p, want_f = fold([c for _, c in own[:k]])
        print(f"{W}x{H} n={n} depth {depth} strict={int(strict)} jitter={int(jitter)} frame {k - 1}: {int((p != want_p).sum())} packed pixels differ, "
              f"{int((f != want_f).any(1).sum())} float")
        assert count == k
        assert np.array_equal(p, want_p), k
        assert np.array_equal(f, want_f), k
    assert np.array_equal(got[0][0], own[0][0])                 # frame 0 is the plain frame
    if n > 1:
        assert np.array_equal(got[0][1], own[0][1])             # ... float too where the plain launch resolves


# ------------------------------------------------------------------ 4. strict against the oracle
@pytest.mark.parametrize("W,H,n,depth", [SHAPES[0], SHAPES[1], SHAPES[3]])
def test_strict_accumulation_is_the_fold_of_the_oracles_frames(R, api, oracle, demo_scene, tex, sky, W, H, n, depth):
    from oracle.oracle_py import Camera
    K = 3
    ocam = oracle.camera(CAM["origin"], CAM["look"], 90.0, 1.0, W, H)
    cs = []
    for f in range(K):
        cam_f = jittered(ocam, f, n, Camera)
        if n > 1:
            cam_f = virtual_camera(Camera, rows_of(cam_f), ocam, n)
        _, rgb = oracle_frame(oracle, cam_f, demo_scene, tex, sky, depth, api.frame_seed(f))
        cs.append(resolve(rgb, W, H, n)[1] if n > 1 else rgb)
    want_p, want_f = fold(cs)
    p, f, count = accumulated(R, api, demo_scene, tex, sky, W, H, n, depth, True, True, K)[-1]
    print(f"{W}x{H} n={n} depth {depth}: {int((p != want_p).sum())} packed pixels differ from the oracle's fold, {int((f != want_f).any(1).sum())} float "
          f"(largest |difference| {float(np.abs(f - want_f).max()):.3g})")
    # The frame is held to the oracle bit for bit.  The float means cannot be: the strict build follows the oracle to within the ulp by which the
    # device's sinf / cosf / powf differ from glibc's (the pinned residual).  Bound: a light's term is a product of such a
    # result with factors both sides compute alike, so it carries a relative error of about one ulp from powf and one from the sample's
    # direction; the terms of a pixel are non-negative and what is compared is clamped to [0, 1], so an unclamped pixel's terms are each at
    # most 1 and their errors add up to a few ulps of 1.0 at most -- 8 x 2^-23 allows four times the two sources; the mean of K frames keeps it.
    # (The float output is held bit for bit to the GPU's own constituent frames in the test above.)
    assert count == K and np.array_equal(p, want_p)
    assert float(np.abs(f - want_f).max()) <= 8 * 2.0 ** -23


# ------------------------------------------------------------------ 5. strips compose
@pytest.mark.parametrize("n", [1, 2])
def test_strips_compose(R, api, demo_scene, tex, sky, n):
    W, H, depth, K = 96, 64, 4, 4
    full = accumulated(R, api, demo_scene, tex, sky, W, H, n, depth, False, True, K)[-1]
    strips = [accumulated(R, api, demo_scene, tex, sky, W, H, n, depth, False, True, K, first_row=r0, rows=32)[-1] for r0 in (0, 32)]
    assert all(s[2] == K for s in strips) and full[2] == K
    assert np.array_equal(np.concatenate([s[0] for s in strips]), full[0])
    assert np.array_equal(np.concatenate([s[1] for s in strips]), full[1])


# ------------------------------------------------------------------ 6. restart and hold
def test_restart_and_hold(R, api, demo_scene, tex, sky):
    W, H, depth = 96, 64, 4
    cam = base_camera(api, W, H)
    other = dict(CAM, origin=(0.3, 2.0, -7.0))
    cam2 = api.perspective(other["origin"], other["look"], 90.0, 1.0, W, H)
    plain1, _ = plain(R, demo_scene, tex, sky, W, H, depth, False, cam)
    plain2, _ = plain(R, demo_scene, tex, sky, W, H, depth, False, cam2)
    plain1_d3, _ = plain(R, demo_scene, tex, sky, W, H, 3, False, cam)
    with rendering(R, demo_scene, tex, sky, W, H, cam=cam, depth=depth, accumulate=64) as r:
        frames = [p for p, _ in take(r, 3, rgb=False)]
        assert r.accumulated == 3 and np.array_equal(frames[0], plain1) and not np.array_equal(frames[2], plain1)
        r.look(**other)                                      # another camera: its plain frame, one frame in the sum
        assert np.array_equal(r.render(), plain2) and r.accumulated == 1
        r.render()
        r.look(**other)                                      # the same values again: the view goes on
        r.render()
        assert r.accumulated == 3
        r.w.set_tile_sched(0)                                # a scheduling knob: the image is the same
        r.render()
        assert r.accumulated == 4
        r.set_camera(cam)
        r.render(); r.render()
        assert r.accumulated == 2
        r.w.set_depth(3)
        assert np.array_equal(r.render(), plain1_d3) and r.accumulated == 1
        r.w.set_depth(depth)
        r.render(); r.render()
        r.w.invalidate_scene()
        assert np.array_equal(r.render(), plain1) and r.accumulated == 1
        r.render()
        r.reset_accumulation()
        assert np.array_equal(r.render(), plain1) and r.accumulated == 1
        r.render()
        r.w.set_seed_offset(7)
        r.render()
        assert r.accumulated == 1
    with rendering(R, demo_scene, tex, sky, W, H, cam=cam, depth=depth, accumulate=3) as r:
        r.w.timing_reset()
        got = [p for p, _ in take(r, 3, rgb=False)]
        assert r.accumulated == 3 and r.w.timing_get(1)[0] == 3
        assert np.array_equal(got[2], frames[2])
        flags = r.w.last_trace_flags()
        for _ in range(2):                                   # converged: no launch, the same frame
            assert np.array_equal(r.render(), got[2]) and r.accumulated == 3
        assert r.w.timing_get(1)[0] == 3 and r.w.last_trace_flags() == flags


# ------------------------------------------------------------------ 7. it converges
def test_it_converges(R, api, demo_scene, tex, sky):
    W, H, depth = 160, 120, 4
    with rendering(R, demo_scene, tex, sky, W, H, cam=base_camera(api, W, H), depth=depth, accumulate=64, jitter=False) as r:
        at = {}
        for k in range(1, 65):
            p = r.render()
            if k in (1, 16, 64):
                at[k] = np.stack([(p >> 16) & 255, (p >> 8) & 255, p & 255], 1).astype(np.int64)
        assert r.accumulated == 64
    d1, d16 = int(np.abs(at[1] - at[64]).sum()), int(np.abs(at[16] - at[64]).sum())
    print(f"summed channel distance to the 64-frame result: 1 frame {d1}, 16 frames {d16}")
    assert d16 < d1 and (at[16] != at[1]).any()


# ------------------------------------------------------------------ 8. refusals: message + exit(1); the environment
_run = run_child


REFUSED = {
    "two_kernel_path": ("r = Renderer(sc, tex, sky, 64, 48, depth=2, fuse=False, accumulate=4); r.look(**CAM); r.render()", "fused"),
    "caller_written_rays": ("r = Renderer(sc, tex, sky, 64, 48, depth=2, accumulate=4); r.look(**CAM); r.w.output(r.pixels, 0, 0, 0, 0, None)\n"
                            "r.w.device_ptr(0, 8)\nr.w.output(r.pixels, 0, 1, 1, 10, None)", "fused"),
    "sample_cameras": ("r = Renderer(sc, tex, sky, 64, 48, depth=2, supersample=2, accumulate=4); c = r.look(**CAM)\n"
                       "r.set_sample_cameras(api.lens_cameras(c, 0.0, 1.0, 2)); r.render()", "sample cameras"),
    "lens": ("r = Renderer(sc, tex, sky, 64, 48, depth=2, supersample=2, lens=(0.1, 5.0), accumulate=4); r.look(**CAM); r.render()", "lens"),
    "moving_spheres": ("r = Renderer(sc, tex, sky, 64, 48, depth=2, supersample=2, motion=np.ones((4, 3), np.float32), accumulate=4); r.look(**CAM); r.render()",
                       "moving spheres"),
    "adaptive": ("r = Renderer(sc, tex, sky, 64, 48, depth=2, supersample=2, adaptive=16, accumulate=4); r.look(**CAM); r.render()", "adaptive"),
    "max_frames_negative": ("w = api.ClWrap(); w.set_accumulate(-1, 1)", "[0, 65536]"),
    "max_frames_too_many": ("w = api.ClWrap(); w.set_accumulate(65537, 1)", "[0, 65536]"),
    "jitter_2": ("w = api.ClWrap(); w.set_accumulate(4, 2)", "jitter"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_unsupported_combinations_exit_with_a_message(case):
    snippet, word = REFUSED[case]
    p = _run(snippet + "\nprint('unreachable')")
    assert p.returncode == 1 and "ERROR:\t" in p.stdout and "ccumulation" in p.stdout and word in p.stdout and "unreachable" not in p.stdout, p.stdout + p.stderr


@pytest.mark.parametrize("jitter,seed", [("0", "11"), ("1", None)])
def test_environment_is_read(jitter, seed):
    """q is the same view with the mode set by hand, jitter off: the environment's renderer equals it iff CLWRAP_ACC_JITTER=0 was read"""
    snippet = ("r = Renderer(sc, tex, sky, 64, 48, depth=2); r.look(**CAM)\n"
               "for _ in range(9): r.render()\n"
               "print('accumulated', r.accumulated, 'seed', r.w.get_seed_offset())\n"
               "a = r.render().copy()\n"
               "q = Renderer(sc, tex, sky, 64, 48, depth=2); q.w.set_accumulate(7, 0); q.look(**CAM)\n"
               "for _ in range(7): b = q.render().copy()\n"
               "print('same', int(np.array_equal(a, b)))\n")
    env = dict(os.environ, CLWRAP_ACCUMULATE="7", CLWRAP_ACC_JITTER=jitter)
    if seed:
        env["CLWRAP_SEED_OFFSET"] = seed
    p = _run(snippet, env=env)
    assert p.returncode == 0 and f"accumulated 7 seed {seed or 0}" in p.stdout and f"same {1 - int(jitter)}" in p.stdout, p.stdout + p.stderr


@pytest.mark.parametrize("name,value", [("CLWRAP_ACCUMULATE", "65537"), ("CLWRAP_ACCUMULATE", "-1"), ("CLWRAP_ACC_JITTER", "2"),
                                        ("CLWRAP_SEED_OFFSET", "abc"), ("CLWRAP_SEED_OFFSET", "4294967296"), ("CLWRAP_SEED_OFFSET", "-1")])
def test_bad_environment_value_exits(name, value):
    code = ("import sys; sys.path.insert(0, %r)\nimport torch\nfrom example_gui_opencl_raytracer_amd import api\napi.ClWrap()\nprint('unreachable')\n" % ROOT)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, **{name: value}))
    assert p.returncode == 1 and "ERROR:\t" in p.stdout and name in p.stdout and "unreachable" not in p.stdout, p.stdout + p.stderr


# ------------------------------------------------------------------ 9. the reference's unchanged interactive driver
REF_INTERACTIVE = os.path.join(ROOT, "oracle", "_ref", "rayinteractive_hip")


@pytest.mark.skipif(not os.path.exists(REF_INTERACTIVE), reason="oracle/_ref/rayinteractive_hip not built (needs /root/reference)")
def test_unchanged_interactive_driver_accumulates(R, api, demo_scene, tex, tmp_path):
    from example_gui_opencl_raytracer_amd import textures
    sky = textures.skybox_cross(1024)
    for d in ("scenes", "assets/bg", "out"):
        os.makedirs(tmp_path / d, exist_ok=True)
    demo_scene.save(tmp_path / "scenes" / "render.map")
    for i, name in enumerate(("cobblestone", "sand", "check", "grass")):
        api.write_png_rgba(str(tmp_path / "assets" / f"{name}.png"), tex[i])
    api.write_png_rgba(str(tmp_path / "assets" / "bg" / "stormydays.png"), sky[0])

    def run(keys, frames, dump, accumulate):
        env = dict(os.environ, CLWRAP_ACCUMULATE=accumulate, MFB_STUB_FRAMES=str(frames), MFB_STUB_KEYS=keys, MFB_STUB_DUMP=str(tmp_path / dump))
        p = subprocess.run([REF_INTERACTIVE], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and f"minifb-stub: {frames} frames" in p.stdout, p.stdout + p.stderr
        img = api.read_png(str(tmp_path / dump))
        return (img[..., 0].astype(np.uint32) << 16 | img[..., 1].astype(np.uint32) << 8 | img[..., 2]).reshape(-1)

    W, H, depth = 800, 600, 15
    still = run("", 6, "still.png", "4")                     # six frames of a still view: four accumulate, two hold
    with R(demo_scene, tex, sky, W, H, depth=depth, accumulate=4) as r:
        r.look((0.8, 2.5, -8.0), (0.0, 0.0, 1.0))           # the camera of rayinteractive.c:111-115
        for _ in range(4):
            want = r.render().copy()
    assert np.array_equal(still, want)
    # a key on the last frame: the sum starts again, the dump is the PLAIN frame of the moved camera -- the one the driver shows with the mode off
    moved = run(".....W", 6, "moved.png", "4")
    moved_plain = run(".....W", 6, "moved_plain.png", "0")
    assert np.array_equal(moved, moved_plain) and not np.array_equal(moved, still)
