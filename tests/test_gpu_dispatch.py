"""GPU tests of what a deep launch decides on the device, where an image comparison cannot see it: the dispatch order wt_sched_build writes
(against the host model and checker of tests/sched_common.py), the split of heavy tiles over several wavefronts (shown to happen, and to change
no bit), and the scratch-stack flavours at the depths where a stack is exactly full.  Everything here is bit for bit: no tolerance."""
import numpy as np
import pytest

import sched_common as sc
from conftest import CAM
from flags_common import F_COUNT, F_DEEP, F_OCC, F_D8, F_D16
from parity_common import check_exact
from render_common import R, released, rendering, resolve, same_floats, take  # noqa: F401  (R: the fixture)

pytestmark = pytest.mark.gpu

# render.map from close by: the glass sphere fills the middle tiles of a small frame and floor and mirror the rest, so that tile costs spread
# over more than the factor 16 a split at every lg needs (from the far camera the tiles of a 61x43 frame cost within a factor of 8 of their share's quota)
CLOSE_CAM = dict(origin=(0.8, 0.9, -0.6), look=(0.0, -0.05, 1.0), fov=90.0, focal=1.0)
GLASS_CAM = dict(origin=(3.5, 3.0, -6.0), look=(0.0, -2.5, 9.5), fov=90.0, focal=1.0)
TAIL_KEYS = ("segments", "shadow_rays", "light_probes", "sky_fetches", "texel_fetches", "pushes", "shadow_rays_traced")


@pytest.fixture(scope="module")
def wrap(R):
    """A wrapper to run the builder on: clw_ext_unit_sched needs no scene."""
    from example_gui_opencl_raytracer_amd import api
    with released(api.ClWrap("src/cl/raygen.cl", "raygen", "src/cl/raytracing.cl", "raytracer")) as w:
        yield w


# ------------------------------------------------------------ C. wt_sched_build on synthetic cost tables
# (split_slots, max_lg, min_quota): without slots nothing else is read
SPLITS = [(0, 4, 1500), (512, 4, 1), (512, 4, 1500), (512, 2, 1), (512, 2, 1500), (512, 1, 1), (512, 1, 1500)]


def run_builder(wrap, cost, clamp, cap, slots, min_quota, max_lg):
    trows, tpr = cost.shape
    words = wrap.unit_sched(cost, tpr, trows, clamp, cap, slots, min_quota, max_lg)
    assert words.size == 8 * (sc.per_share_of(tpr, trows) << max_lg) + 8 * cap
    shares = sc.model(cost, clamp, cap, slots, min_quota, max_lg)
    return sc.check_order(words, shares, cap), shares, words


@pytest.mark.parametrize("values", sc.VALUES)
@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_sched_build_against_the_model(wrap, shape, values):
    """The builder's whole output -- the list, and the sentinels behind it -- for every split setting, both min_quota, with and without the outlier
    clamp, with a list that has room for parts (per_share + 1024) and one that has none (per_share: the quota doubles until nothing is split, or
    only as far as a share with fewer tiles than per_share has room)."""
    tpr, trows = sc.SHAPES[shape]
    cost = sc.value_table(values, tpr, trows)
    ps = sc.per_share_of(tpr, trows)
    split_seen = doubled = 0
    for slots, max_lg, min_quota in SPLITS:
        for clamp in (0, 1):
            for cap in (ps, ps + 1024):
                errs, shares, _ = run_builder(wrap, cost, clamp, cap, slots, min_quota, max_lg)
                assert errs == [], (shape, values, dict(slots=slots, max_lg=max_lg, min_quota=min_quota, clamp=clamp, cap=cap), errs[:4])
                split_seen += sum(sc.lg_histogram(shares)[1:])
                if slots:
                    start = [max(min(int(cost[k::8].astype(np.uint64).sum()) // slots, 0x7FFFFFFF), min_quota, 1) for k in range(8)]
                    doubled += sum(1 for k in range(8) if shares[k]["tiles"] and shares[k]["quota"] != start[k])
    if cost.max() > 1:
        assert split_seen > 0, "no setting split any tile of this table"
    if values in ("all equal", "around the quota", ">= 2^31") and shape != "1x1":
        assert doubled > 0, "the quota never had to double on this table"


@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_sched_build_when_the_parts_never_fit(wrap, shape):
    """min_quota 1, every cost 2^31, a list with room for ONE part more than the tiles: the quota doubles up to "never split" (split_slots 512;
    max_lg 4, 2, 1): no entry beyond the list, at most one tile of a share served by two wavefronts."""
    tpr, trows = sc.SHAPES[shape]
    cost, cap = sc.overflow_table(tpr, trows)
    for max_lg in (4, 2, 1):
        for clamp in (0, 1):
            errs, shares, _ = run_builder(wrap, cost, clamp, cap, 512, 1, max_lg)
            assert errs == [], (shape, max_lg, clamp, errs[:4])
            assert all(sh["nvalid"] - len(sh["tiles"]) <= 1 for sh in shares)       # room for one part more: at most one tile in two


@pytest.mark.parametrize("tpr,trows,slots", sc.OVERFLOW_CASES)
def test_sched_build_ends_at_never_split_when_24_trials_are_not_enough(wrap, tpr, trows, slots):
    """The inputs the trial loop, as it was, left with more entries than the list holds (tests/test_sched_host.py shows it with the model): a
    share whose sum / split_slots is below 2^7.  The builder ends at "never split" by itself: no tile split, nothing behind the list touched."""
    cost, cap = sc.overflow_table(tpr, trows)
    for max_lg in (4, 2, 1):
        errs, shares, words = run_builder(wrap, cost, 0, cap, slots, 1, max_lg)
        assert errs == [], (tpr, trows, slots, max_lg, errs[:4])
        old = sc.model(cost, 0, cap, slots, 1, max_lg, fixed=False)
        for k in range(8):
            if not old[k]["fits"]:          # (max_lg 4 everywhere; a single tile split in two still fits its list of two)
                assert shares[k]["quota"] == 0xFFFFFFFF and shares[k]["nvalid"] == len(shares[k]["tiles"]), (k, max_lg)
                assert not sc.order_lgs(words[k:8 * cap:8], cap).any()
        if max_lg == 4:
            assert not any(sh["fits"] for sh in old if sh["tiles"])


# ------------------------------------------------------------ D. the split really happens, and changes nothing
def choose_slots(cost, cap, max_lg):
    """The split_slots (min_quota 1) for which the model serves the most tiles at its rarest lg, 0..max_lg -> (slots, histogram)."""
    best = (0, None, None)
    for slots in sorted({int(round(1.05 ** e)) for e in range(0, 285)}):         # 1 .. 2^20 in steps of 5 %
        h = sc.lg_histogram(sc.model(cost, 0, cap, slots, 1, max_lg), max_lg)
        if best[1] is None or min(h) > best[0]:
            best = (min(h), slots, h)
    return best[1], best[2]


def counted(r, one_launch=False):
    """(packed, float, counters) of a still view: the float frame first (two trace launches), then one counted launch.  one_launch: all three from
    ONE launch of the counting build, the float frame read back behind the raygen launch, which in fused mode only latches the camera again (for
    frames that take seconds, at depths where the counting build has no flavour to lose)."""
    if one_launch:
        if r._rgb_dev is None:
            from example_gui_opencl_raytracer_amd import api
            r.w.load_global_data(1, 31, None, 12 * r.pixels, api.CL_MEM_WRITE_ONLY)
            r._rgb_dev = r.w.device_ptr(1, 31)
        r.w.set_debug_rgb(r._rgb_dev)
        r.w.enable_counters(1)
        img = r.render().copy()
        c = r.w.read_counters()
        r.w.enable_counters(0)
        rgb = np.empty((r.pixels, 3), np.float32)
        r.w.output(r.pixels, rgb.nbytes, 0, 1, 31, rgb)
        r.w.set_debug_rgb(0)
        return img, rgb, c
    img, rgb = r.render_rgb()
    img, rgb = img.copy(), rgb.copy()
    r.w.enable_counters(1)
    again = r.render()
    c = r.w.read_counters()
    r.w.enable_counters(0)
    assert np.array_equal(again, img)
    return img, rgb, c


def forced_split(r, max_lg, tpt=(-1, -1)):
    """Still camera, tail on: a first frame in the default order, `slots` chosen from its costs so that the model splits tiles at every lg up to
    max_lg, the schedulers reset, a frame whose costs the order is built from (once: the view stands still), then the frames under test, which
    read that order -> (packed, float, counters, order words, per_share_cap, the model's shares)."""
    w = r.w
    w.set_variant(0)
    w.set_tpt(tpt[0], tpt[1], -1)
    w.set_split(-1, 1)
    r.render(readback=False)
    vw, vh = r.width * w.get_supersample(), r.height * w.get_supersample()
    tpr, trows = (vw + 7) // 8, (vh + 7) // 8
    cap = sc.per_share_of(tpr, trows) + (w.get_split()[2] if max_lg else 0)
    first = w.read_tile_costs()
    assert first.size == tpr * trows
    slots, _ = choose_slots(first.reshape(trows, tpr), cap, max_lg)
    w.set_split(slots, 1)
    r.render(readback=False)
    assert w.read_tile_order()[0].size == 0, "the frame after a reset runs in the default order"
    cost = w.read_tile_costs().reshape(trows, tpr)
    shares = sc.model(cost, 0, cap, slots if max_lg else 0, 1, max_lg)
    h = sc.lg_histogram(shares, max_lg)
    print(f"{vw}x{vh}: split_slots {slots}, costs {int(cost.min())}..{int(cost.max())}, quotas {[sh['quota'] for sh in shares]}, tiles per lg {h}")
    if cost.size <= 64:
        print(cost)
    assert all(x > 0 for x in h), f"the model does not split at every lg 0..{max_lg}: {h}"
    img, rgb, c = counted(r)
    order, got_cap = w.read_tile_order()
    assert got_cap == cap and order.size == 8 * cap
    return img, rgb, c, order, cap, shares


def per_lane(r):
    r.w.set_variant(16)
    return counted(r)


def check_split_frame(what, got, ref, max_lg):
    img, rgb, c, order, cap, shares = got
    rimg, rrgb, rc = ref
    errs = sc.check_order(order, shares, cap)
    assert errs == [], (what, errs[:4])
    lgs = sc.order_lgs(order, cap)
    assert lgs.max() == max_lg, (what, int(lgs.max()))
    assert c["tpt_tiles"] > 0 and rc["tpt_tiles"] == 0, what
    print(f"{what}: {int((img != rimg).sum())} packed pixels, {int((rgb.view(np.uint32) != rrgb.view(np.uint32)).any(1).sum())} float pixels differ from the per-lane loop")
    assert np.array_equal(img, rimg), what
    assert same_floats(rgb, rrgb), what
    assert all(c[k] == rc[k] for k in TAIL_KEYS), (what, {k: (c[k], rc[k]) for k in TAIL_KEYS})


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("w,h", [(61, 43), (160, 120)])
def test_forced_split_on_render_map(R, oracle, demo_scene, tex, sky, w, h, strict):
    """render.map at depth 15 (61x43 from close by, 160x120 from the usual camera): tiles served by 1, 2, 4, 8 and 16 wavefronts (61x43: parts of
    the edge tiles own no pixel), the order the launch read
    is the one the contract gives for the costs it was built from, and frame, radiance and ray counters are the per-lane loop's."""
    cam = CLOSE_CAM if w < 100 else CAM
    with rendering(R, demo_scene, tex, sky, w, h, cam=cam, depth=15, strict=strict) as r:
        ref = per_lane(r)
        for tpt in ((-1, -1), (64, 1)):
            check_split_frame(f"render.map {w}x{h} strict={strict} tail at {tpt[0]}", forced_split(r, 4, tpt), ref, 4)
    if strict:
        want, _, _ = oracle.render(oracle.camera(cam["origin"], cam["look"], 90.0, 1.0, w, h), demo_scene, tex, sky, 15)
        check_exact(ref[0], want, f"forced split / per-lane loop vs oracle: render.map {w}x{h}")


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_forced_split_with_a_pool_the_tail_gives_up_on(R, oracle, tex, sky, strict):
    """The glass field at depth 15 with split tiles and a pool whose slots hold 192 nodes: a part gives up like a whole tile does, and the
    per-lane loop finishes it."""
    from example_gui_opencl_raytracer_amd import scene
    field = scene.dielectric_field_scene(4)
    with rendering(R, field, tex, sky, 160, 120, cam=GLASS_CAM, depth=15, strict=strict) as r:
        ref = per_lane(r)
        per_node = (29 + 4 * 3) if strict else (27 + 3)
        words = (25 + 36) * 64 + 15 * 192 + per_node * 192 + 63
        r.w.set_tpt(-1, -1, max(1, (words * 8192 * 4) >> 20))
        for tpt in ((24, -1), (64, 1)):
            got = forced_split(r, 4, tpt)
            assert got[2]["tpt_gave_up"] > 0, got[2]
            check_split_frame(f"glass field, small pool, strict={strict}, tail at {tpt[0]}", got, ref, 4)
    if strict:
        want, _, _ = oracle.render(oracle.camera(GLASS_CAM["origin"], GLASS_CAM["look"], 90.0, 1.0, 160, 120), field, tex, sky, 15)
        check_exact(ref[0], want, "forced split with a small pool / per-lane loop vs oracle: glass field 160x120")


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("n,W,H,max_lg", [(2, 80, 60, 2), (4, 40, 30, 1)])
def test_forced_split_of_supersampled_launches(R, oracle, demo_scene, tex, sky, n, W, H, max_lg, strict):
    """A part of a split tile must hold whole n x n sample groups: at most 4 parts with n = 2, 2 with n = 4.  The frame is the resolve of the
    1-sample per-lane frame of the n*W x n*H view."""
    with rendering(R, demo_scene, tex, sky, n * W, n * H, depth=15, strict=strict) as v:
        v.w.set_variant(16)
        (virt_p, virt), = take(v)
    if strict:      # the virtual frame is the oracle's, so the supersampled frame is the resolve of the oracle's samples
        want, _, _ = oracle.render(oracle.camera(CAM["origin"], CAM["look"], 90.0, 1.0, n * W, n * H), demo_scene, tex, sky, 15)
        check_exact(virt_p, want, f"virtual frame {n * W}x{n * H} of the supersampled forced split vs oracle")
    want_p, want_f = resolve(virt, W, H, n)
    with rendering(R, demo_scene, tex, sky, W, H, depth=15, strict=strict, supersample=n) as r:
        img, rgb, c, order, cap, shares = forced_split(r, max_lg, (64, 1))
    errs = sc.check_order(order, shares, cap)
    assert errs == [], errs[:4]
    assert sc.order_lgs(order, cap).max() == max_lg
    assert c["tpt_tiles"] > 0
    assert np.array_equal(img, want_p)
    assert same_floats(rgb, want_f)


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("case", ["n = 8", "moving spheres"])
def test_launches_that_must_not_split(R, demo_scene, tex, sky, case, strict):
    """n = 8 (a part would have to hold 8 tile rows) and moving spheres (no tail): however small the quota, every entry of the order has lg 0, and
    the order is the unsplit one of the costs it was built from."""
    from sphere_motion_common import DISP
    n, W, H, kw = (8, 20, 15, {}) if case == "n = 8" else (2, 80, 60, dict(motion=DISP))
    with rendering(R, demo_scene, tex, sky, W, H, depth=15, strict=strict, supersample=n, **kw) as r:
        r.w.set_split(4096, 1)
        r.render(readback=False)
        tpr, trows = (n * W + 7) // 8, (n * H + 7) // 8
        cost = r.w.read_tile_costs().reshape(trows, tpr)
        r.render(readback=False)
        r.render(readback=False)
        order, cap = r.w.read_tile_order()
    assert cap == sc.per_share_of(tpr, trows) and order.size == 8 * cap
    assert cost.max() > 16, "costs a quota of 1 would split"
    assert sc.check_order(order, sc.model(cost, 0, cap, 0, 1, 0), cap) == []
    assert not sc.order_lgs(order, cap).any()


# ------------------------------------------------------------ F. the scratch-stack flavours where a stack is exactly full
@pytest.fixture(scope="module")
def glass8():
    from example_gui_opencl_raytracer_amd import scene
    return scene.dielectric_field_scene(8)


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("depth", [8, 9, 16, 17])
def test_stack_flavours_at_their_edges(R, oracle, glass8, tex, sky, depth, strict):
    """WT_F_D8 / WT_F_D16 carry scratch for 7 / 15 parents; at depth 8 / 16 the glass field fills them to the last entry (the oracle's max_stack
    counts the current ray too), at 9 / 17 the next flavour takes over.  The flavour sized for the depth, the full 31-parent stack (variant
    2048), the low-occupancy flavour (64) and both give the same bits; the strict frame is the oracle's."""
    w, h = 64, 48
    want, _, cnt = oracle.render(oracle.camera(GLASS_CAM["origin"], GLASS_CAM["look"], 90.0, 1.0, w, h), glass8, tex, sky, depth)
    assert cnt.max_stack == depth, (depth, int(cnt.max_stack))
    outs = []
    for variant in (0, 2048, 64, 64 | 2048):
        with rendering(R, glass8, tex, sky, w, h, setup=lambda wrap: wrap.set_variant(variant), cam=GLASS_CAM, depth=depth, strict=strict) as r:
            outs += take(r)
            flags = r.w.last_trace_flags()
        want_flavour = 0 if variant & 2048 else (F_D8 if depth <= 8 else (F_D16 if depth <= 16 else 0))
        assert flags & F_DEEP and not flags & (F_COUNT | F_OCC) and flags & (F_D8 | F_D16) == want_flavour, (depth, variant, flags)
    for p, f in outs[1:]:
        assert np.array_equal(p, outs[0][0]) and same_floats(f, outs[0][1]), depth
    if strict:
        check_exact(outs[0][0], want, f"glass field 64x48 depth {depth}, stack exactly full / one past")


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_the_top_of_the_full_stack(R, oracle, tex, sky, strict):
    """Depth 32 on the deep scene whose refraction trees climb highest under the ray cap: 28 of the 32 stack entries (a straight row of glass
    spheres would fill all of them, but its tree doubles per level).  Only the full flavour runs at this depth.  One pixel of this frame holds
    660 000 of its 1.6 M rays, a serial chain no mode shortens: a launch was measured at 2.5 s on an MI355X, whichever mode.  So this scene runs at
    depth 32 here only, in the two modes that differ most and with one launch per compared frame: the per-lane loop, and everything through the
    tail with tiles split -- an order built from a first frame's costs, read back and shown to hold split entries, the tail shown to have run.
    Packed frame, float radiance and ray counters are equal; the strict per-lane frame is the oracle's."""
    import time
    import fuzz_scenes as F
    sc_, cam = F.deep_scene(F.DEEP_TOP_SEED)
    with rendering(R, sc_, tex, sky, F.DEEP_W, F.DEEP_H, cam=cam, depth=32, strict=strict) as r:
        t0 = time.time()
        ref = mode_frame(r, "per-lane loop", one_launch=True)
        t1 = time.time()
        got = mode_frame(r, "tail at 64, forced split", one_launch=True)
        print(f"deep scene {F.DEEP_TOP_SEED} depth 32 strict={strict}: per-lane launch {t1 - t0:.2f} s, two launches through the split tail {time.time() - t1:.2f} s; "
              f"tail tiles {got[2]['tpt_tiles']}, gave up {got[2]['tpt_gave_up']}, split entries {int((got[3] > 0).sum())}")
        flags = r.w.last_trace_flags()
    assert flags & F_DEEP and not flags & (F_D8 | F_D16)
    assert ref[2]["tpt_tiles"] == 0 and got[2]["tpt_tiles"] > 0 and (got[3] > 0).any()
    assert np.array_equal(got[0], ref[0]) and same_floats(got[1], ref[1])
    assert all(got[2][k] == ref[2][k] for k in TAIL_KEYS), {k: (got[2][k], ref[2][k]) for k in TAIL_KEYS}
    if strict:
        want, _, cnt = oracle.render(oracle.camera(cam["origin"], cam["look"], 90.0, 1.0, F.DEEP_W, F.DEEP_H), sc_, tex, sky, 32)
        assert cnt.max_stack == F.DEEP_TOP_STACK and cnt.int_cast_oor == 0 and cnt.oob_reads == 0
        check_exact(ref[0], want, f"deep scene {F.DEEP_TOP_SEED} at depth 32, stack {F.DEEP_TOP_STACK} deep")


# ------------------------------------------------------------ E. the tail on scenes that differ, in both builds
def mode_frame(r, mode, one_launch=False):
    """(packed, float, counters, lg of the order's entries) of one mode of a still view: the schedulers reset, one frame whose costs the order is
    built from where the mode is about the order, then the frames under test."""
    if not hasattr(r, "library_defaults"):       # what the library starts with (its constants, or the environment's values), read before any mode changes it
        r.library_defaults = (r.w.get_tpt()[:2], r.w.get_split()[:2])
    tpt0, split0 = r.library_defaults
    variant, tpt, split = {"per-lane loop": (16, tpt0, split0), "tail": (0, tpt0, split0), "tail at 64": (0, (64, 1), split0),
                           "tail at 64, forced split": (0, (64, 1), (1 << 20, 1)), "full stack": (2048, tpt0, split0)}[mode]
    r.w.set_variant(variant)
    r.w.set_tpt(tpt[0], tpt[1], -1)
    r.w.set_split(*split)
    if split != split0:
        r.render(readback=False)         # the frame whose costs the order is built from
    img, rgb, c = counted(r, one_launch)
    order, cap = r.w.read_tile_order()
    return img, rgb, c, sc.order_lgs(order, cap)


MODES = ["per-lane loop", "tail", "tail at 64", "tail at 64, forced split", "full stack"]


def check_modes(r, what, gave_up=False, modes=MODES):
    """Every mode gives the per-lane loop's bits and ray counters; the tail ran wherever it is on; with `gave_up`, wherever everything goes
    through it unsplit, it also gave up on some tile -> the per-lane frame."""
    ref = mode_frame(r, modes[0])
    assert ref[2]["tpt_tiles"] == 0
    for mode in modes[1:]:
        img, rgb, c, lgs = mode_frame(r, mode)
        print(f"{what}, {mode}: {int((img != ref[0]).sum())} packed / {int((rgb.view(np.uint32) != ref[1].view(np.uint32)).any(1).sum())} float pixels differ, "
              f"tail tiles {c['tpt_tiles']}, gave up {c['tpt_gave_up']}, split entries {int((lgs > 0).sum())}")
        assert c["tpt_tiles"] > 0, (what, mode)
        if gave_up and mode == "tail at 64":          # (not with the forced split: a part holds a sixteenth of its tile's trees)
            assert c["tpt_gave_up"] > 0, (what, mode, c)
        if mode == "tail at 64, forced split":
            assert (lgs > 0).any(), (what, mode)
        assert np.array_equal(img, ref[0]), (what, mode)
        assert same_floats(rgb, ref[1]), (what, mode)
        assert all(c[k] == ref[2][k] for k in TAIL_KEYS), (what, mode, {k: (c[k], ref[2][k]) for k in TAIL_KEYS})
    return ref[0]


def _deep_seeds():
    import fuzz_scenes as F
    return list(F.DEEP_SEEDS)


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("seed", _deep_seeds())
def test_tail_modes_on_deep_scenes(R, oracle, tex, sky, seed, strict):
    """Fields of glass, mirror and opaque spheres with 0, 1, 2, 3, 4 and 7 lights (a tail node has 27 + nl words in the fast build, 29 + 4 nl in the
    strict one), at depth 5, on both sides of the stack-flavour switches and, where the ray count allows, at 32: one renderer per scene and build,
    five modes per depth, all bit-equal in the packed frame, the float radiance and the ray counters; the strict frames are the oracle's."""
    import fuzz_scenes as F
    sc_, cam = F.deep_scene(seed)
    with rendering(R, sc_, tex, sky, F.DEEP_W, F.DEEP_H, cam=cam, depth=5, strict=strict) as r:
        for depth in F.DEEP_SEEDS[seed]:
            r.w.set_depth(depth)
            what = f"deep scene {seed} ({len(sc_.lights)} lights) depth {depth} strict={strict}"
            frame = check_modes(r, what)
            if strict:
                want, _, _ = oracle.render(oracle.camera(cam["origin"], cam["look"], cam["fov"], cam["focal"], F.DEEP_W, F.DEEP_H), sc_, tex, sky, depth)
                check_exact(frame, want, what)


def test_fast_tail_on_the_uniform_grid(R, tex, sky):
    """The fast build's tail with segments that walk the uniform grid: 576 spheres at depth 8, everything through the tail."""
    from example_gui_opencl_raytracer_amd import scene
    cam = dict(origin=(0.0, 6.0, -8.0), look=(0.0, -0.45, 1.0), fov=90.0, focal=1.0)
    with rendering(R, scene.sphere_grid_scene(24, 24), tex, sky, 160, 96, cam=cam, depth=8, strict=False) as r:
        ref = mode_frame(r, "per-lane loop")
        for mode in ("tail", "tail at 64"):
            img, rgb, c, _ = mode_frame(r, mode)
            assert c["tpt_tiles"] > 0 and np.array_equal(img, ref[0]) and same_floats(rgb, ref[1]), mode
            assert all(c[k] == ref[2][k] for k in TAIL_KEYS), (mode, {k: (c[k], ref[2][k]) for k in TAIL_KEYS})
        assert r.w.last_trace_flags() & 16, "the launch did not walk the grid"


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_tail_with_255_lights(R, oracle, demo_scene, tex, sky, strict):
    """255 lights at depth 5 on a 24x16 frame of render.map from close by: a node carries a weight per light (strict: four), so 192 nodes fit a
    slot -- the tail runs, and where whole tiles go through it from the first segment on, it gives up on those whose trees outgrow that."""
    from example_gui_opencl_raytracer_amd import scene
    rng = np.random.default_rng(255)
    lights = np.tile(demo_scene.lights, 85)
    lights["origin"][:, :3] += rng.uniform(-1.5, 1.5, (255, 3)).astype(np.float32)
    lights["intensity"] *= np.float32(1 / 40)
    many = scene.Scene(demo_scene.spheres, demo_scene.planes, lights)
    with rendering(R, many, tex, sky, 24, 16, cam=CLOSE_CAM, depth=5, strict=strict) as r:
        if not strict:
            # a slot of the default pool holds 192 strict nodes of 29 + 4 * 255 words, but 896 fast ones of 27 + 255: the fast build gets the pool
            # that gives its slots 192 nodes as well (the sizes of the give-up test of test_gpu_parity.py)
            words = (25 + 36) * 64 + 5 * 192 + (27 + 255) * 192 + 63
            r.w.set_tpt(-1, -1, (words * 8192 * 4) >> 20)
        frame = check_modes(r, f"255 lights strict={strict}", gave_up=True)
    if strict:
        want, _, cnt = oracle.render(oracle.camera(CLOSE_CAM["origin"], CLOSE_CAM["look"], 90.0, 1.0, 24, 16), many, tex, sky, 5)
        assert cnt.int_cast_oor == 0 and cnt.oob_reads == 0
        check_exact(frame, want, "255 lights, 24x16, depth 5")
