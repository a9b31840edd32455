"""Every twin kernel of the primary-ray cull table, launched with a table.

A trace launch that is given a table runs `wt_trace_cull<FLAGS>` (csrc/whitted_trace.inc), compiled once for every flavour wt_cull_flavour
admits.  wt_find_trace (csrc/whitted_launch.inc) holds 22 of them that the planner can reach with a table (csrc/launch_plan.c: wt_plan_cull):

    fast build      the generic flag words 0, 1, 4, 5 and the 12 shaped words WT_SHAPE_FLAGS(1..4, 0..2, 3)
    strict build    0, 1, 4, 5, 1 | WT_F_ACC and 5 | WT_F_ACC

A twin's only contract is that skipping a group of tests that fails in every lane changes no bit.  The shaped loops are unrolled by count, the
probe of the lights runs in chunks of four with a switch for the last one, the sphere loop clamps its last block: a fault can sit in one twin
alone, so each one is run (cull_common.on_and_off: table on == table off, packed and float; the device table == the host definition, byte for
byte; the flag word == the word the case names) on views whose tables hold set AND clear bits.  TWINS collects every (build, flag word) a case
asserted; `twin_report` holds it to the 22 after the module."""
import numpy as np
import pytest

import accumulate_common as acc
from conftest import CAM
from cull_common import NO_CULL, check_case, on_and_off
from flags_common import F_ACC, F_COUNT, F_GEOM_LDS, SHAPE_LIGHTS, SHAPE_MAX_PLANES, SHAPE_MAX_SPHERES, shape_flags
from fuzz_scenes import random_scene
from parity_common import report
from render_common import R, api, assert_same_frames, rendering, take  # noqa: F401  (R, api: the fixtures)
from shape_common import FRAME, RAGGED, SHAPES, V_GENERIC, scene_of

pytestmark = pytest.mark.gpu

V_GEOM_GLOBAL = 1                       # clw_ext_set_variant: geometry read from global memory although it would fit LDS
builds = pytest.mark.parametrize("strict", [False, True], ids=["fast", "strict"])
TWINS = set()                           # the (build, flag word) pairs whose launch with a table a case here asserted


def build_of(strict):
    return "strict" if strict else "fast"


def expected_twins():
    """the twins of wt_find_trace that wt_plan_cull gives a table, from the vocabulary of flags_common: the four generic words of either build,
    the fast build's shaped words, the strict build's WT_F_ACC words (wt_acc_flagged: the shallow counting kernels read the seed offset as
    their WT_F_ACC twin; the grid kernels, the other WT_F_ACC words, take no table)"""
    generic = {0, F_COUNT, F_GEOM_LDS, F_GEOM_LDS | F_COUNT}
    shaped = {shape_flags(ns, npl) for ns in range(1, SHAPE_MAX_SPHERES + 1) for npl in range(SHAPE_MAX_PLANES + 1)}
    acc_twins = {F_COUNT | F_ACC, F_GEOM_LDS | F_COUNT | F_ACC}
    return {("fast", f) for f in generic | shaped} | {("strict", f) for f in generic | acc_twins}


def whole_module(request):
    """the run selects this module as a whole (no -k expression, no single test named): only then do the sums over its cases hold"""
    return not request.config.option.keyword and not any("::" in str(a) for a in request.config.args)


@pytest.fixture(scope="module", autouse=True)
def twin_report(request):
    """after the module: the twins launched with a table next to the 22 the launcher holds, in the log of measured figures"""
    yield
    want = expected_twins()
    print(f"cull twins launched with a table: {len(TWINS & want)} of {len(want)} flag words; missing {sorted(want - TWINS)}, beyond {sorted(TWINS - want)}")
    report(dict(test="cull twins launched with a table", count=len(TWINS), compiled=len(want), equal=TWINS == want,
                missing=[list(x) for x in sorted(want - TWINS)]))
    assert len(want) == 22 and TWINS <= want
    if whole_module(request):
        assert TWINS == want


def fast_word(sc):
    """the flag word of a shallow fused 1-sample launch of a small scene in the fast build (csrc/launch_plan.c: wt_plan): its shaped word where
    the counts are compiled, else the generic LDS word"""
    ns, npl, nl = sc.counts
    return shape_flags(ns, npl) if 1 <= ns <= SHAPE_MAX_SPHERES and npl <= SHAPE_MAX_PLANES and nl == SHAPE_LIGHTS else F_GEOM_LDS


def bits_of(table):
    return (table & 1) != 0, (table & 2) != 0


# ---------------------------------------------------------------------------- 1. the 12 shaped twins, and the generic LDS twin on their views
_premise = {}


def shaped_premise(oracle, api, ns, npl, W, H):
    """the host table of the shape's view, held to what makes a twin that reads a neighbouring tile's byte lose a sphere: bit 0 set in some
    tiles and clear in others, bit 1 set somewhere, and a tile that some sphere's line really crosses (computed once per view)"""
    key = (ns, npl, W, H)
    if key not in _premise:
        sc, cam, _ = scene_of(ns, npl)
        c = api.perspective(cam["origin"], cam["look"], cam["fov"], cam["focal"], W, H)
        table, ps, _ = check_case(oracle, c, sc)
        s, l = bits_of(table)
        print(f"shape ({ns}, {npl}) {W}x{H}: bit 0 set in {int(s.sum())} of {s.size} tiles, bit 1 in {int(l.sum())}; a sphere's line crosses {int(ps.sum())}")
        assert s.any() and not s.all() and l.any() and ps.any(), key
        _premise[key] = table.reshape(-1)
    return _premise[key]


@pytest.mark.parametrize("W,H", [FRAME, RAGGED], ids=["72x48", "61x43"])
@pytest.mark.parametrize("ns,npl", SHAPES, ids=[f"{s}s{p}p" for s, p in SHAPES])
def test_shaped_twins(R, api, oracle, tex, sky, ns, npl, W, H):
    sc, cam, _ = scene_of(ns, npl)
    host = shaped_premise(oracle, api, ns, npl, W, H)
    for depth in (1, 4):
        with rendering(R, sc, tex, sky, W, H, cam=cam, depth=depth) as r:
            _, table = on_and_off(r, f"shape ({ns}, {npl}) {W}x{H} depth {depth}", cam=cam, flags=shape_flags(ns, npl), asserted=TWINS, build="fast")
            assert np.array_equal(table, host)


@builds
@pytest.mark.parametrize("W,H", [FRAME, RAGGED], ids=["72x48", "61x43"])
@pytest.mark.parametrize("ns,npl", SHAPES, ids=[f"{s}s{p}p" for s, p in SHAPES])
def test_generic_lds_twin_on_the_shaped_views(R, api, oracle, tex, sky, ns, npl, W, H, strict):
    """variant 8192 keeps the fast build on the generic kernel; the strict build has no other"""
    sc, cam, _ = scene_of(ns, npl)
    host = shaped_premise(oracle, api, ns, npl, W, H)
    for depth in (1, 4):
        with rendering(R, sc, tex, sky, W, H, cam=cam, depth=depth, strict=strict) as r:
            _, table = on_and_off(r, f"shape ({ns}, {npl}) {W}x{H} depth {depth} generic {build_of(strict)}", cam=cam, flags=F_GEOM_LDS, variant=V_GENERIC,
                                  asserted=TWINS, build=build_of(strict))
            assert np.array_equal(table, host)


# ---------------------------------------------------------------------------- 2. global geometry, counting, the strict WT_F_ACC twins
@builds
@pytest.mark.parametrize("variant,counting,word", [(V_GEOM_GLOBAL, False, 0), (V_GEOM_GLOBAL, True, F_COUNT), (0, True, F_GEOM_LDS | F_COUNT)],
                         ids=["global", "global-counting", "lds-counting"])
def test_global_geometry_and_counting_twins(R, api, demo_scene, tex, sky, variant, counting, word, strict):
    W, H = 72, 44
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict, setup=lambda w: w.enable_counters(1) if counting else None) as r:
        _, table = on_and_off(r, f"render.map {W}x{H} variant {variant} counting {counting} {build_of(strict)}", cam=CAM, flags=word, variant=variant,
                              counting=counting, asserted=TWINS, build=build_of(strict))
        s, l = bits_of(table)
        assert s.any() and not s.all() and l.any()


@pytest.mark.parametrize("variant,word", [(0, F_GEOM_LDS | F_COUNT | F_ACC), (V_GEOM_GLOBAL, F_COUNT | F_ACC)], ids=["lds", "global"])
def test_strict_seeded_counting_twins(R, api, demo_scene, tex, sky, variant, word):
    """the strict build's shallow counting kernels read the seed offset only as their WT_F_ACC twin"""
    W, H = 72, 44
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=True, seed_offset=1, setup=lambda w: w.enable_counters(1)) as r:
        off, table = on_and_off(r, f"render.map {W}x{H} variant {variant} seeded counting strict", cam=CAM, flags=word, variant=variant, counting=True,
                                asserted=TWINS, build="strict")
        s, _ = bits_of(table)
        assert s.any() and not s.all()
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=True) as r:
        assert not np.array_equal(r.render(), off[0])      # (the seed offset is read)


# ---------------------------------------------------------------------------- 3. a still view that accumulates
@builds
def test_accumulating_still_view(R, api, demo_scene, tex, sky, strict):
    """jitter off: the camera stands, so frames 1 to 3 are given the table built behind frame 0; their running means are the table-off ones"""
    W, H, depth, K = 64, 40, 4, 4
    cam = acc.base_camera(api, W, H)
    tables = lambda r: r.w.read_primary_cull()
    with rendering(R, demo_scene, tex, sky, W, H, setup=lambda w: w.set_variant(NO_CULL), cam=cam, depth=depth, strict=strict, accumulate=K, jitter=False) as r:
        want = take(r, K, extra=lambda r: (r.accumulated, tables(r)))
    assert [f[2][0] for f in want] == [1, 2, 3, 4] and all(f[2][1] == (None, 0) for f in want)
    with rendering(R, demo_scene, tex, sky, W, H, cam=cam, depth=depth, strict=strict, accumulate=K, jitter=False) as r:
        got = take(r, K, extra=lambda r: (r.accumulated, tables(r), r.w.last_trace_flags()))
    host = api.host_primary_cull(cam, demo_scene.spheres, demo_scene.lights).reshape(-1)
    word = F_GEOM_LDS if strict else fast_word(demo_scene)
    for k in range(K):
        count, (table, n), flags = got[k][2]
        assert count == k + 1 and flags == word, (k, count, hex(flags))
        assert (table is None and n == 0) if k == 0 else (n == 1 and table is not None and table.tobytes() == host.tobytes()), (k, n)
        assert_same_frames([got[k]], want[k][0], want[k][1], f"accumulating still view {build_of(strict)} frame {k}")
    assert not np.array_equal(got[0][0], got[K - 1][0])      # (the frames differ: each has its own seeds)
    TWINS.add((build_of(strict), word))


@builds
def test_accumulating_jittered_view_takes_no_table(R, api, demo_scene, tex, sky, strict):
    """jitter on: the trace's camera moves by a sub-pixel every frame, so no view comes twice in a row -- bind_primary_cull (csrc/hip_wrap.cpp)
    builds nothing and hands out nothing.  (Were a table reported, it would have to be the jittered camera's: api.jitter_camera.)"""
    W, H, depth, K = 64, 40, 4, 4
    cam = acc.base_camera(api, W, H)
    frames = {}
    for variant in (NO_CULL, 0):
        with rendering(R, demo_scene, tex, sky, W, H, setup=lambda w: w.set_variant(variant), cam=cam, depth=depth, strict=strict, accumulate=K, jitter=True) as r:
            frames[variant] = take(r, K, extra=lambda r: (r.accumulated, r.w.read_primary_cull()))
    for k in range(K):
        count, (table, n) = frames[0][k][2]
        assert count == k + 1
        if table is not None:      # the failure path: whose table is it?
            jit = api.jitter_camera(cam, k, 1)
            assert table.tobytes() == api.host_primary_cull(jit, demo_scene.spheres, demo_scene.lights).tobytes(), ("a table of another camera", k)
        assert table is None and n == 0, (k, n)
        assert_same_frames([frames[0][k]], frames[NO_CULL][k][0], frames[NO_CULL][k][1], f"accumulating jittered view {build_of(strict)} frame {k}")
    assert not np.array_equal(api.jitter_camera(cam, 1, 1).im_corner[:], cam.im_corner[:])


# ---------------------------------------------------------------------------- 4. fuzz views: 0 to 8 spheres, 0 to 4 lights
SEEDS = range(40)
_fuzz = {False: [], True: []}      # build -> [(seed, ns, nl, table, the launch was given it)]


@builds
@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_views(R, api, tex, sky, seed, strict):
    """the counts around the 4-wide chunks of the light probe and the sphere loop, the empty groups whose bit is set in every tile (the scene's
    own depth is ignored: deep launches take no table)"""
    sc, cam, _ = random_scene(seed)
    W, H = (64, 40) if seed % 2 == 0 else (61, 43)
    ns, _, nl = sc.counts
    for depth in (1, 4):
        with rendering(R, sc, tex, sky, W, H, cam=cam, depth=depth, strict=strict) as r:
            _, table = on_and_off(r, f"fuzz seed {seed} {W}x{H} depth {depth} {build_of(strict)}", cam=cam, flags=F_GEOM_LDS if strict else fast_word(sc),
                                  asserted=TWINS, build=build_of(strict))
    s, l = bits_of(table)
    if ns == 0:
        assert s.all()      # an empty group has nothing to test: its bit is set everywhere
    if nl == 0:
        assert l.all()
    _fuzz[strict].append((seed, ns, nl, table))


@builds
def test_fuzz_views_cover_the_counts(request, strict):
    """(behind the seeds of its build) over their union: both bits set and clear, an empty sphere group and an empty light group, the light
    counts 1 to 4 -- every size of the probe's last chunk and a whole one -- and a clamped last block of spheres, each in a launch with a table"""
    rows = _fuzz[strict]
    if not whole_module(request) and len(rows) < len(SEEDS):
        return      # (a run of single cases: the union is not there to be judged)
    assert sorted(r[0] for r in rows) == list(SEEDS), "run behind test_fuzz_views of the same build"
    every = np.concatenate([r[3] for r in rows])
    s, l = bits_of(every)
    print(f"fuzz views {build_of(strict)}: {every.size} tiles, bit 0 set in {int(s.sum())}, bit 1 in {int(l.sum())}; "
          f"sphere counts {sorted({r[1] for r in rows})}, light counts {sorted({r[2] for r in rows})}")
    assert s.any() and not s.all() and l.any() and not l.all()
    assert any(r[1] == 0 for r in rows) and any(r[2] == 0 for r in rows)
    assert {1, 2, 3, 4} <= {r[2] for r in rows} and any(r[1] > 4 for r in rows)
    assert any(4 < r[1] < 8 for r in rows)      # a last block of 1 to 3 spheres: the clamped fetch


# ---------------------------------------------------------------------------- 5. ragged frames: tile counts that are no multiple of the word
@pytest.mark.parametrize("W,H,tiles", [(1, 1, 1), (7, 3, 1), (33, 9, 10), (257, 8, 33), (150, 101, 247)], ids=lambda v: str(v))
def test_ragged_frames(R, api, demo_scene, tex, sky, W, H, tiles):
    """the kernel loads the table a word of four tiles at a time"""
    with rendering(R, demo_scene, tex, sky, W, H, depth=4) as r:
        _, table = on_and_off(r, f"render.map {W}x{H}", cam=CAM, flags=fast_word(demo_scene), asserted=TWINS, build="fast")
        assert table.size == tiles == ((W + 7) // 8) * ((H + 7) // 8)
