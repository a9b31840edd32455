"""Every compiled shaped trace kernel in every sampling mode, and the modes on the generic kernels of scenes outside the shaped set.

The fast build runs a small scene with a kernel that has the scene's counts compiled in (wt_shape in csrc/whitted_trace.inc).  The switch of
WT_LAUNCH_TRACE (csrc/whitted_launch.inc) holds 1..4 spheres x 0..2 planes x 3 lights = 12 shapes in four flavours each: 48 kernels, whose
sphere, plane and light loops are unrolled by count.  Each case group of that switch, and the test here that launches it for all 12 shapes
(scenes: fuzz_scenes.SHAPED_SEEDS, held to their conditions by test_shape_scenes_host.py; every test asserts the exact flag word):

    WT_SHAPE_FLAGS(ns, np, 3)                           test_plain                      (and the 1-sample frames of every other test)
    WT_SHAPE_FLAGS(ns, np, 3) | WT_F_SS                 test_supersampled, test_seed_offset_and_accumulation (n = 2), test_shutter_cameras,
                                                        and the static frame of test_moving_spheres
    WT_SHAPE_FLAGS(ns, np, 3) | WT_F_SS | WT_F_LIST     test_adaptive                   (the refine pass; last_trace_flags reports it)
    WT_SHAPE_FLAGS(ns, np, 3) | WT_F_SS | WT_F_MOVE     test_moving_spheres

The seed offset and the accumulation are run-time branches of the plain and the supersampled flavour: test_seed_offset_and_accumulation.
Every shaped frame is compared bit for bit, packed and float, with the generic kernel's (variant 8192) and held to the mode's definition in
the *_common.py module of its suite; the plain flavour also to the CPU oracle.  The second half runs the modes on the generic kernels, in
both builds, for the counts just outside the compiled set and for empty primitive lists."""
import numpy as np
import pytest

import accumulate_common as acc
import adaptive_common as ada
import sample_cameras_common as cams
import sphere_motion_common as motion
from conftest import CAM, channel_diff
from fuzz_scenes import random_scene, sphere_displacement
from parity_common import check_exact, report
from render_common import R, api, frames, resolve, run_child, same_floats  # noqa: F401  (R, api: the fixtures)
from shape_common import (ADAPTIVE, DEPTHS, F_GEOM_LDS, F_LIST, F_MOVE, F_SHAPE, F_SS, FRAME, RAGGED, SHAPES, V_GENERIC, empty_list_scenes, frame,
                          scene_of, shape_flags)

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B1
shapes = pytest.mark.parametrize("ns,npl", SHAPES, ids=[f"{s}s{p}p" for s, p in SHAPES])


def generic(w):
    w.set_variant(V_GENERIC)


def other_end(cam):
    """the camera at the other end of a shutter that opens on `cam`"""
    o, l = cam["origin"], cam["look"]
    return dict(cam, origin=(o[0] + 0.4, o[1] + 0.3, o[2] + 0.5), look=(l[0] - 0.1, l[1] - 0.05, l[2]))


LAUNCHED = set()      # the flag words of the shaped launches the sweep asserted


@pytest.fixture(scope="module", autouse=True)
def launched_report():
    """after the module: how many shaped flag words were asserted, next to the 48 of the switch, in the log of measured figures"""
    yield
    want = {shape_flags(s, p) | m for s, p in SHAPES for m in (0, F_SS, F_SS | F_LIST, F_SS | F_MOVE)}
    report(dict(test="shaped flag words asserted", count=len(LAUNCHED), in_switch=len(want), equal=LAUNCHED == want))


def check_flags(ns, npl, mode, shaped, generic_flags):
    """the shaped launch ran exactly this case of the switch, the forced-generic one the plain LDS-geometry kernel of the same mode"""
    assert shaped == shape_flags(ns, npl) | mode, (hex(shaped), hex(shape_flags(ns, npl) | mode))
    assert generic_flags == F_GEOM_LDS | mode, hex(generic_flags)
    LAUNCHED.add(shaped)


def same_frames(a, b):
    """(packed, float) pairs, bit for bit"""
    return np.array_equal(a[0], b[0]) and same_floats(a[1], b[1])


# =========================================================================================== the 12 shapes x 4 flavours, shaped and generic
@shapes
@pytest.mark.parametrize("W,H", [FRAME, RAGGED], ids=["72x48", "61x43"])
def test_plain(R, oracle, tex, sky, ns, npl, W, H):
    sc, cam, _ = scene_of(ns, npl)
    for depth in (1, 2, 3, 4):
        out, rgb, flags = frame(R, sc, tex, sky, W, H, depth, 0, cam)
        gen, gen_rgb, gflags = frame(R, sc, tex, sky, W, H, depth, V_GENERIC, cam)
        check_flags(ns, npl, 0, flags, gflags)
        assert same_frames((out, rgb), (gen, gen_rgb)), depth
        want, _, cnt = oracle.render(oracle.camera(cam["origin"], cam["look"], cam["fov"], cam["focal"], W, H), sc, tex, sky, depth)
        assert cnt.int_cast_oor == 0 and cnt.oob_reads == 0
        strict, _, sflags = frame(R, sc, tex, sky, W, H, depth, 0, cam, strict=True)
        assert sflags == F_GEOM_LDS
        le1 = float((channel_diff(out, want) <= 1).mean())
        print(f"{ns} spheres {npl} planes {W}x{H} depth {depth}: strict {int((strict != want).sum())} pixels off the oracle, fast {le1:.4f} within 1 LSB")
        check_exact(strict, want, f"shape ({ns}, {npl}) {W}x{H} d{depth} strict")
        assert le1 >= 0.97, depth


@shapes
@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("W,H", [FRAME, RAGGED], ids=["72x48", "61x43"])
def test_supersampled(R, tex, sky, ns, npl, W, H, n):
    sc, cam, _ = scene_of(ns, npl)
    for depth in DEPTHS:
        (virt,), vflags = frames(R, sc, tex, sky, n * W, n * H, depth, False, cam=cam)
        want = resolve(virt[1], W, H, n)
        (got,), flags = frames(R, sc, tex, sky, W, H, depth, False, n=n, cam=cam)
        (gen,), gflags = frames(R, sc, tex, sky, W, H, depth, False, n=n, cam=cam, setup=generic)
        assert vflags == shape_flags(ns, npl)
        check_flags(ns, npl, F_SS, flags, gflags)
        print(f"{ns} spheres {npl} planes {W}x{H} n={n} depth {depth}: {int((got[0] != want[0]).sum())} packed pixels differ from the resolve")
        assert same_frames(got, gen), depth
        assert got[0].shape == (W * H,) and same_frames(got, want), depth


@shapes
@pytest.mark.parametrize("n,depth,lens", [(2, 1, None), (2, 4, None), (2, 1, motion.LENS), (2, 4, motion.LENS), (4, 4, None)],
                         ids=["n2-d1", "n2-d4", "n2-d1-lens", "n2-d4-lens", "n4-d4"])
def test_moving_spheres(R, api, tex, sky, ns, npl, n, depth, lens):
    sc, cam, disp = scene_of(ns, npl)
    W, H = FRAME
    # == `composed` of the GPU's own 1-sample frames of the moved scenes, != the static supersampled frame
    flags, want_p = motion.check_self_consistent(R, api, sc, tex, sky, W, H, n, depth, False, disp=disp, cams=lens, cam=cam)
    ((p, f),), flags2, _ = motion.moving(R, sc, tex, sky, W, H, n, depth, False, disp, cams=lens, cam=cam)
    ((gp, gf),), gflags, _ = motion.moving(R, sc, tex, sky, W, H, n, depth, False, disp, cams=lens, cam=cam, setup=generic)
    _, sflags, _ = motion.moving(R, sc, tex, sky, W, H, n, depth, False, None, cams=lens, cam=cam, rgb=False)
    assert flags2 == flags
    check_flags(ns, npl, F_SS | F_MOVE, flags, gflags)
    check_flags(ns, npl, F_SS, sflags, F_GEOM_LDS | F_SS)          # (the static frame it was told apart from)
    assert np.array_equal(p, want_p) and same_frames((p, f), (gp, gf))


@shapes
def test_adaptive(R, api, tex, sky, ns, npl):
    sc, cam, _ = scene_of(ns, npl)
    W, H = FRAME
    n, T = ADAPTIVE
    for depth in DEPTHS:
        ((bp, bf),), bflags = frames(R, sc, tex, sky, W, H, depth, False, cam=cam)
        ((fp, ff),), fflags = frames(R, sc, tex, sky, W, H, depth, False, n=n, cam=cam)
        got, flags = ada.adaptive(R, sc, tex, sky, W, H, depth, False, n, T, cam=cam)
        gen, gflags = ada.adaptive(R, sc, tex, sky, W, H, depth, False, n, T, cam=cam, setup=generic)
        assert bflags == shape_flags(ns, npl) and fflags == shape_flags(ns, npl) | F_SS
        check_flags(ns, npl, F_SS | F_LIST, flags, gflags)
        mask = ada.check_composite(api, (bp, bf, fp, ff, fflags), got, W, H, n, T, f"shape ({ns}, {npl}) depth {depth}")
        assert np.array_equal(mask, ada.refine_mask_np(bp, W, H, n, T))
        assert 0 < mask.sum() < mask.size
        assert same_frames(got[0], gen[0]) and np.array_equal(got[0][2], gen[0][2])
        ((p, f, m),), flags = ada.adaptive(R, sc, tex, sky, W, H, depth, False, n, 0, cam=cam)
        assert flags == shape_flags(ns, npl) | F_SS | F_LIST and m.all() and same_frames((p, f), (fp, ff))
        ((p, f, m),), flags = ada.adaptive(R, sc, tex, sky, W, H, depth, False, n, 256, cam=cam)
        assert flags == shape_flags(ns, npl) | F_SS | F_LIST and not m.any() and same_frames((p, f), (bp, bf))


@shapes
@pytest.mark.parametrize("depth", DEPTHS)
def test_seed_offset_and_accumulation(R, api, tex, sky, ns, npl, depth):
    sc, cam, _ = scene_of(ns, npl)
    W, H = FRAME
    (seeded,), flags = frames(R, sc, tex, sky, W, H, depth, False, cam=cam, seed_offset=SEED)
    (gen,), gflags = frames(R, sc, tex, sky, W, H, depth, False, cam=cam, seed_offset=SEED, setup=generic)
    (unseeded,), _ = frames(R, sc, tex, sky, W, H, depth, False, cam=cam)
    check_flags(ns, npl, 0, flags, gflags)
    assert same_frames(seeded, gen) and not np.array_equal(seeded[0], unseeded[0])
    K = 3
    for n in (1, 2):
        own = acc.own_frames(R, api, sc, tex, sky, W, H, n, depth, False, True, K, cam=cam, name=("shape", ns, npl))
        flags, gflags = [], []
        got = acc.accumulated(R, api, sc, tex, sky, W, H, n, depth, False, True, K, cam=cam, flags=flags)
        gen = acc.accumulated(R, api, sc, tex, sky, W, H, n, depth, False, True, K, cam=cam, flags=gflags, setup=generic)
        check_flags(ns, npl, F_SS if n > 1 else 0, flags[0], gflags[0])
        assert not np.array_equal(own[1][0], own[0][0])
        for k in range(1, K + 1):
            want_p, want_f = acc.fold([c for _, c in own[:k]])
            p, f, count = got[k - 1]
            assert count == k and np.array_equal(p, want_p) and np.array_equal(f, want_f), (n, k)
            assert gen[k - 1][2] == k and same_frames((p, f), gen[k - 1][:2]), (n, k)


@shapes
@pytest.mark.parametrize("depth", DEPTHS)
def test_shutter_cameras(R, api, tex, sky, ns, npl, depth):
    sc, cam, _ = scene_of(ns, npl)
    W, H = FRAME
    n = 2
    base, table = cams.make_table(api, W, H, n, "shutter", cam, other_end(cam))
    want, vflags = cams.gpu_composed(R, api, sc, tex, sky, base, table, W, H, n, depth, False)
    (got,), flags, used = cams.sampled(R, sc, tex, sky, W, H, n, depth, False, "shutter", table=table, cam=cam)
    (gen,), gflags, _ = cams.sampled(R, sc, tex, sky, W, H, n, depth, False, "shutter", table=table, cam=cam, setup=generic)
    (still,), _ = frames(R, sc, tex, sky, W, H, depth, False, n=n, cam=cam, rgb=False)
    assert vflags == shape_flags(ns, npl) and used.tobytes() == table.tobytes()
    check_flags(ns, npl, F_SS, flags, gflags)
    assert same_frames(got, gen) and same_frames(got, want)
    assert not np.array_equal(got[0], still[0])                   # the table is not a no-op


# =========================================================================================== the modes on the generic kernels of other counts
OTHER_SEEDS = [14, 16, 43, 42, 7]         # (1, 3, 3), (4, 2, 4), (4, 2, 2), (0, 3, 3), (8, 2, 3): just outside the compiled set
EMPTY = ["no spheres", "no planes", "no lights", "sky only"]


def other_scene(which, demo_scene):
    """-> (scene, camera, depth <= 8, displacement or None where there is no sphere)"""
    if which in EMPTY:
        sc = empty_list_scenes(demo_scene)[which]
        return sc, CAM, 4, motion.DISP if len(sc.spheres) else None
    sc, cam, depth = random_scene(which)
    ns = len(sc.spheres)
    return sc, cam, min(depth, 8), sphere_displacement(np.random.default_rng(which), ns, first=1) if ns else None


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("which", OTHER_SEEDS + EMPTY)
def test_modes_on_the_generic_kernels(R, api, demo_scene, tex, sky, which, strict):
    """(render.map without its planes has counts the fast build compiles: variant 8192 keeps every launch here on the generic kernels)"""
    sc, cam, depth, disp = other_scene(which, demo_scene)
    W, H = FRAME
    n, T = ADAPTIVE
    # supersampled == resolve of the 1-sample virtual frame
    (virt,), vflags = frames(R, sc, tex, sky, n * W, n * H, depth, strict, cam=cam, setup=generic)
    ((bp, bf),), bflags = frames(R, sc, tex, sky, W, H, depth, strict, cam=cam, setup=generic)
    ((fp, ff),), fflags = frames(R, sc, tex, sky, W, H, depth, strict, n=n, cam=cam, setup=generic)
    assert not (vflags | bflags) & (F_SHAPE | F_SS) and fflags & F_SS and not fflags & (F_SHAPE | F_MOVE | F_LIST)
    assert same_frames((fp, ff), resolve(virt[1], W, H, n))
    # adaptive == composite
    got, flags = ada.adaptive(R, sc, tex, sky, W, H, depth, strict, n, T, cam=cam, setup=generic)
    assert flags & F_LIST and flags & F_SS and not flags & (F_SHAPE | F_MOVE)
    ada.check_composite(api, (bp, bf, fp, ff, fflags), got, W, H, n, T, f"{which} strict={int(strict)}")
    # accumulation == fold
    K = 3
    own = acc.own_frames(R, api, sc, tex, sky, W, H, 1, depth, strict, True, K, cam=cam, name=("other", which), setup=generic)
    flags = []
    for k, (p, f, count) in enumerate(acc.accumulated(R, api, sc, tex, sky, W, H, 1, depth, strict, True, K, cam=cam, flags=flags, setup=generic), start=1):
        want_p, want_f = acc.fold([c for _, c in own[:k]])
        assert count == k and np.array_equal(p, want_p) and np.array_equal(f, want_f), k
    assert not flags[0] & (F_SHAPE | F_SS)
    # moving spheres == composed
    if disp is not None:
        flags, _ = motion.check_self_consistent(R, api, sc, tex, sky, W, H, n, depth, strict, disp=disp, cam=cam, setup=generic)
        assert flags & F_MOVE and flags & F_SS and not flags & (F_SHAPE | F_LIST)


@pytest.mark.parametrize("moves", [True, False], ids=["moving", "static"])
@pytest.mark.parametrize("seed", [16, 7])
def test_strict_modes_against_the_oracle(R, api, oracle, demo_scene, tex, sky, seed, moves):
    """As test_strict_moving_frame_is_composed_of_the_oracles_frames_of_the_moved_scenes (test_gpu_sphere_motion.py), on 4 spheres with 4 lights
    and on 8 spheres: the output pixels whose footprint holds a selected virtual pixel at which the strict 1-sample render itself differs from
    the oracle's (the device libm's 1-ulp sinf / cosf / powf differences) are left out, at most 4."""
    from oracle.oracle_py import Camera
    sc, cam, depth, disp = other_scene(seed, demo_scene)
    if not moves:
        disp = np.zeros_like(disp)              # S(t) = S: plain supersampling
    W, H = FRAME
    n = 2
    times = api.sample_times(n)
    base, table = motion.camera_table(api, W, H, n, None, cam)
    oracle_frames = {}

    def oracle_virtual(k):
        p, f, cnt = oracle.render(cams.virtual_camera(Camera, table[k], base, n), motion.moved_scene(api, sc, disp, float(times[k])), tex, sky, depth, want_rgb=True)
        assert cnt.int_cast_oor == 0 and cnt.oob_reads == 0
        oracle_frames[k] = p
        return f
    want_p, _ = cams.composed(oracle_virtual, table, W, H, n)

    def differs(k):
        return motion.gpu_virtual(R, api, sc, tex, sky, disp, times[k], base, table[k], n, depth, True, what="packed")[0] != oracle_frames[k]
    selected = cams.pick(differs, W, H, n)
    left_out = selected.reshape(H, n, W, n).any((1, 3)).reshape(-1)
    print(f"seed {seed} moves={int(moves)} depth {depth}: {int(selected.sum())} selected virtual pixels differ from the oracle, {int(left_out.sum())} output pixels left out")
    assert left_out.sum() <= 4
    ((p, _),), flags, _ = motion.moving(R, sc, tex, sky, W, H, n, depth, True, disp if moves else None, cam=cam)
    assert flags & F_SS and bool(flags & F_MOVE) == moves and not flags & F_SHAPE
    keep = ~left_out
    print(f"  {int((p[keep] != want_p[keep]).sum())} kept packed pixels differ")
    assert np.array_equal(p[keep], want_p[keep])


# =========================================================================================== a displacement table and a scene without spheres
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_an_empty_table_on_a_scene_without_spheres_is_no_motion(R, demo_scene, tex, sky, strict):
    """clw_ext_set_sphere_motion stores a table in which nothing moves as none: 0 rows are the plain supersampled launch"""
    sc = empty_list_scenes(demo_scene)["no spheres"]
    W, H = FRAME
    (want,), wflags, _ = motion.moving(R, sc, tex, sky, W, H, 2, 4, strict, None)
    (got,), flags, used = motion.moving(R, sc, tex, sky, W, H, 2, 4, strict, np.zeros((0, 3), np.float32), times=np.array([0.1, 0.2, 0.3, 0.4], np.float32))
    assert used.size == 0 and flags == wflags and flags & F_SS and not flags & F_MOVE
    assert same_frames(got, want)


def test_a_table_for_a_scene_without_spheres_is_refused():
    p = run_child("sc = scene.Scene(sc.spheres[:0], sc.planes, sc.lights)\n"
                  "r = Renderer(sc, tex, sky, 64, 48, depth=2, supersample=2, motion=np.full((1, 3), 0.25, np.float32))\n"
                  "r.look(**CAM); r.render()\nprint('unreachable')\n")
    assert p.returncode == 1 and "ERROR:\t" in p.stdout and "unreachable" not in p.stdout, p.stdout + p.stderr
    assert "the displacement table is for 1 spheres, the scene has 0" in p.stdout.split("ERROR:\t", 1)[1], p.stdout
