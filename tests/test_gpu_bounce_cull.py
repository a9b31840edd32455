"""The bounce cull table on the GPU (include/hip_wrap_ext.h: clw_host_bounce_cull, clw_ext_read_bounce_cull, clw_ext_set_bounce_cull;
csrc/whitted_cull.inc builds it beside the primary table, wt_trace_cull reads both from one 16-bit entry per tile).

Every twin kernel (the 22 of test_gpu_cull_twins.py) through cull_common.on_and_off -- table on == table off bit for bit, packed and float, the
primary bytes == their host definition -- and on top: the device's bounce bytes == clw_host_bounce_cull byte for byte, at depths 1, 2 and 4 (the
reflected bits exist from depth 2 on), with views whose bounce tables hold set AND clear bits of both parts.  The counting twins: segments,
probes, shadow rays drawn and rays traced are the same with and without the table.  The parts (clw_ext_set_bounce_cull 0 / 1 / 2 / 3): the
table rebuilt with only those bits, the same frame.

Mutation checks on scratch builds (not committed): without the clear after the second iteration (cullb kept), and with the shadow mask applied
to every shade instead of the first, the on == off comparisons here fail (see the commit message)."""
import numpy as np
import pytest

from conftest import CAM
from cull_common import on_and_off
from flags_common import F_ACC, F_COUNT, F_GEOM_LDS, shape_flags
from render_common import R, api, rendering, take  # noqa: F401  (R, api: the fixtures)
from shape_common import RAGGED, SHAPES, V_GENERIC, scene_of

pytestmark = pytest.mark.gpu

V_GEOM_GLOBAL = 1
builds = pytest.mark.parametrize("strict", [False, True], ids=["fast", "strict"])
DEPTHS = (1, 2, 4)


def host_bounce(api, r, cam, depth, parts=3):
    c = api.perspective(cam["origin"], cam["look"], cam["fov"], cam["focal"], r.width, r.height)
    return api.host_bounce_cull(c, r.scene.spheres, r.scene.planes, r.scene.lights, depth=depth, parts=parts).reshape(-1)


def both_tables(api, r, what, cam, depth, **kw):
    """on_and_off, then the bounce bytes of the view's table against the host definition -> them"""
    on_and_off(r, what, cam=cam, **kw)
    got = r.w.read_bounce_cull()
    want = host_bounce(api, r, cam, depth)
    assert got is not None and got.shape == want.shape and got.tobytes() == want.tobytes(), (what, int((got != want).sum()))
    return got


@pytest.mark.parametrize("ns,npl", SHAPES, ids=[f"{s}s{p}p" for s, p in SHAPES])
def test_shaped_twins(R, api, tex, sky, ns, npl):
    sc, cam, _ = scene_of(ns, npl)
    W, H = RAGGED
    for depth in DEPTHS:
        with rendering(R, sc, tex, sky, W, H, cam=cam, depth=depth) as r:
            t = both_tables(api, r, f"shape ({ns}, {npl}) depth {depth}", cam, depth, flags=shape_flags(ns, npl))
            if npl == 0:
                assert not t.any()


@builds
@pytest.mark.parametrize("ns,npl", SHAPES, ids=[f"{s}s{p}p" for s, p in SHAPES])
def test_generic_lds_twin_on_the_shaped_views(R, api, tex, sky, ns, npl, strict):
    sc, cam, _ = scene_of(ns, npl)
    W, H = RAGGED
    for depth in DEPTHS:
        with rendering(R, sc, tex, sky, W, H, cam=cam, depth=depth, strict=strict) as r:
            both_tables(api, r, f"shape ({ns}, {npl}) depth {depth} generic strict={strict}", cam, depth, flags=F_GEOM_LDS, variant=V_GENERIC)


@builds
@pytest.mark.parametrize("variant,counting,word", [(V_GEOM_GLOBAL, False, 0), (V_GEOM_GLOBAL, True, F_COUNT), (0, True, F_GEOM_LDS | F_COUNT)],
                         ids=["global", "global-counting", "lds-counting"])
def test_global_geometry_and_counting_twins(R, api, demo_scene, tex, sky, variant, counting, word, strict):
    """counting: on_and_off holds every counter of the launches -- segments, probes, shadow rays drawn, rays traced -- equal with and without"""
    W, H = 72, 44
    for depth in DEPTHS:
        with rendering(R, demo_scene, tex, sky, W, H, depth=depth, strict=strict, setup=lambda w: w.enable_counters(1) if counting else None) as r:
            t = both_tables(api, r, f"render.map variant {variant} counting {counting} strict={strict} depth {depth}", CAM, depth, flags=word,
                            variant=variant, counting=counting)
            assert (t & 15).any() and ((t & 48).any() == (depth >= 2))


@pytest.mark.parametrize("variant,word", [(0, F_GEOM_LDS | F_COUNT | F_ACC), (V_GEOM_GLOBAL, F_COUNT | F_ACC)], ids=["lds", "global"])
def test_strict_seeded_counting_twins(R, api, demo_scene, tex, sky, variant, word):
    W, H = 72, 44
    for depth in DEPTHS:
        with rendering(R, demo_scene, tex, sky, W, H, depth=depth, strict=True, seed_offset=1, setup=lambda w: w.enable_counters(1)) as r:
            both_tables(api, r, f"render.map variant {variant} seeded counting strict depth {depth}", CAM, depth, flags=word, variant=variant, counting=True)


@builds
def test_the_parts(R, api, demo_scene, tex, sky, strict):
    """clw_ext_set_bounce_cull: a table with the primary bits only, + the shadow bits, + the reflected bits, all -- the same frame each time, the
    table rebuilt (once) when the parts change"""
    W, H, depth = 150, 101, 4
    with rendering(R, demo_scene, tex, sky, W, H, depth=depth, strict=strict) as r:
        w = r.w
        r.render()                              # (a view is built for when it comes the second time)
        want = take(r, 1)[0]
        full = w.read_bounce_cull()
        builds_ = w.read_primary_cull()[1]
        assert np.array_equal(full, host_bounce(api, r, CAM, depth)) and (full & 15).any() and (full & 48).any() and builds_ == 1
        for parts in (0, 1, 2, 3):
            w.set_bounce_cull(parts)
            got = take(r, 1)[0]
            t = w.read_bounce_cull()
            assert np.array_equal(t, host_bounce(api, r, CAM, depth, parts)), parts
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), parts
            builds_ += 1
            assert w.read_primary_cull()[1] == builds_, parts      # (the setter drops the table even when the parts stay: one build per call)


def test_two_fixed_views_hold_set_and_clear_bits(R, api, demo_scene, tex, sky):
    """the premise of the comparisons above, on two views of its own: the device's bounce bytes of render.map at 72x44 and at 150x101 hold
    every bit of the byte set somewhere and clear somewhere, and nothing in bits 6-7"""
    tables = []
    for W, H in ((72, 44), (150, 101)):
        with rendering(R, demo_scene, tex, sky, W, H, depth=4) as r:
            r.render()
            r.render()                      # (a view is built for when it comes the second time)
            t = r.w.read_bounce_cull()
            assert t is not None and np.array_equal(t, host_bounce(api, r, CAM, 4))
            tables.append(t)
    every = np.concatenate(tables)
    shares = [float(((every >> b) & 1).mean()) for b in range(6)]
    print("bounce bytes of the two views:", every.size, "tiles; bits 0-5 set in", " ".join(f"{100 * s:.1f}%" for s in shares))
    assert all(0.0 < s < 1.0 for s in shares) and not (every & 0xC0).any()
