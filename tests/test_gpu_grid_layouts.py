"""The uniform grid on layouts that decide something (fuzz_scenes.grid_layout), with BOTH of its shadow walks named and checked.

The claim: the grid changes how many tests a ray makes, never their results.  For every layout, both builds and a
camera outside and one inside the sphere set, at 96 x 72 and depth 4:
  small lights   the frame of the paired walk (wt_grid_shadow_pair), of the single walk (wt_grid_shadow, forced with set_grid_pair(0)) and of
                 the linear scan (set_grid(0)) are equal bit for bit, packed and float;
  large lights   (one of radius 1.5 inside the sphere set: the shim's 0.3-of-a-cell rule refuses pairing) grid == linear scan;
  strict build   every one of these frames equals the oracle's, every pixel;
and get_grid() / last_trace_flags() say which walk ran: a scene that does not take the walk a test names FAILS it.  No pixel is masked or
excused: the layouts stay inside the float sphere test's domain (every sphere within 40 units of every camera and light, radii >= 0.05;
test_grid_host.py holds them to it).  The primary-hit pass and the tree-parallel tail (whose shadow rays always walk singly) run on the
same scenes, and a scene with spheres that are not finite runs without a grid."""
import numpy as np
import pytest

import gbuffer_common as gc
from flags_common import F_GRID
from fuzz_scenes import GRID_3D, GRID_LAYOUTS, grid_layout
from parity_common import check_exact
from render_common import R, assert_same_frames, bits, rendering, take  # noqa: F401  (R: the fixture)

pytestmark = pytest.mark.gpu

W, H, DEPTH = 96, 72, 4
GW, GH = gc.WD, gc.HD                    # the primary-hit pass: its expected buffers come from a per-pixel Python loop over every sphere
TW, TH, TDEPTH = 64, 48, 8               # the tail
# light probes that ended ON a light sphere (light_probes - segments of the oracle's counters) with the large lights, both cameras of a
# layout together at W x H, depth DEPTH: the floor asserted below is about half of what the oracle counts (test_grid_host.py prints them)
LIGHT_ENDS_MIN = {"cloud": 400, "giants": 120, "coincident": 750, "touching": 300, "tower": 1900, "offset": 400}


def _oracle_cam(oracle, cam, w, h):
    return oracle.camera(cam["origin"], cam["look"], cam["fov"], cam["focal"], w, h)


def _grid_state(r, pair):
    """the grid of the scene as last prepared and the flags of the last trace launch: built, on, and on the walk the test names"""
    g = r.w.get_grid()
    assert g is not None and g["built"] == 1, g
    assert g["pair"] == pair, f"the scene took the {'paired' if g['pair'] else 'single'} shadow walk: {g}"
    assert (g["reg_pad"] > 0) == bool(pair) and g["ncells"] == g["res"][0] * g["res"][1] * g["res"][2] and g["pairs"] > 0
    assert r.w.last_trace_flags() & F_GRID
    return g


@pytest.mark.parametrize("lights", ["small", "large"])
@pytest.mark.parametrize("name", GRID_LAYOUTS)
def test_both_shadow_walks_equal_the_linear_scan_and_the_oracle(R, oracle, tex, sky, name, lights):
    sc, cams = grid_layout(name, lights)
    wants, ends = [], 0
    for cam in cams:
        want, _, cnt = oracle.render(_oracle_cam(oracle, cam, W, H), sc, tex, sky, DEPTH)
        wants.append(want)
        ends += cnt.light_probes - cnt.segments
    if lights == "large":
        print(f"{name}: {ends} light probes end on a light")
        assert ends >= LIGHT_ENDS_MIN[name]
    for strict in (True, False):
        build = "strict" if strict else "fast"
        with rendering(R, sc, tex, sky, W, H, cam=None, depth=DEPTH, strict=strict) as r:
            assert r.w.get_grid() is None                                   # no scene prepared yet
            for k, cam in enumerate(cams):
                what = f"{name} {lights} {build} camera {k}"
                r.look(**cam)
                r.w.set_grid(1)
                r.w.set_grid_pair(-1)
                got = take(r)                                               # the default setting
                g = _grid_state(r, 1 if lights == "small" else 0)
                if name in GRID_3D:
                    assert min(g["res"]) > 1, g
                if lights == "small":
                    r.w.set_grid_pair(0)
                    got += take(r)
                    assert _grid_state(r, 0)["pairs"] <= g["pairs"]            # no pad: no sphere is listed in more cells than with it
                r.w.set_grid(0)
                (lin_p, lin_f), = take(r)
                assert not r.w.last_trace_flags() & F_GRID
                assert_same_frames(got, lin_p, lin_f, what)
                if strict:
                    check_exact(lin_p, wants[k], what)


def test_the_seam_forces_a_preparation_and_reports_what_came_of_it(R, tex, sky):
    """set_grid_pair(1) pairs where the rule allows it and not where it forbids it; every call prepares the scene again; a scene of at most
    256 spheres has no grid."""
    from example_gui_opencl_raytracer_amd import scene
    for lights, pair in (("small", 1), ("large", 0)):
        sc, cams = grid_layout("touching", lights)
        with rendering(R, sc, tex, sky, 32, 24, cam=cams[0], depth=2, strict=True) as r:
            r.w.set_grid_pair(1)
            (p1, _), = take(r, rgb=False)
            g1 = _grid_state(r, pair)
            r.w.set_grid_pair(0)
            assert r.w.get_grid() == g1                                     # as last prepared: the setting waits for the next launch
            (p0, _), = take(r, rgb=False)
            g0 = _grid_state(r, 0)
            assert np.array_equal(p0, p1) and g0["pairs"] <= g1["pairs"]
            r.w.set_grid_pair(-1)
            take(r, rgb=False)
            assert r.w.get_grid() == g1
    with rendering(R, scene.render_map_scene(), tex, sky, 32, 24, depth=2, strict=True) as r:
        take(r, rgb=False)
        g = r.w.get_grid()
        assert g is not None and g["built"] == 0 and g["pair"] == 0 and g["pairs"] == 0 and g["res"] == (0, 0, 0)


_expected = {}


def _expected_gbuffer(oracle, tex, sky, name, k):
    if (name, k) not in _expected:
        sc, cams = grid_layout(name)
        _expected[name, k] = gc.expected_gbuffer(oracle, sc, tex, sky, _oracle_cam(oracle, cams[k], GW, GH))
    return _expected[name, k]


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("name", ["giants", "coincident", "tower"])
def test_primary_hits_by_object_id_on_three_dimensional_grids(R, oracle, tex, sky, name, strict):
    """wt_grid_nearest / wt_grid_occluded by object id: ids, depth and normal of the primary-hit pass with the grid on equal those with the
    grid off in both builds, and the strict build's equal the oracle's primary hit (equal-t ties of coincident spheres included)."""
    sc, cams = grid_layout(name)
    with rendering(R, sc, tex, sky, GW, GH, cam=None, depth=DEPTH, strict=strict) as r:
        for k, cam in enumerate(cams):
            r.look(**cam)
            r.w.set_grid(1)
            on = r.gbuffer()
            assert r.w.get_grid()["built"] == 1
            r.w.set_grid(0)
            off = r.gbuffer()
            e = _expected_gbuffer(oracle, tex, sky, name, k)
            spheres = int((gc.kind_of(e["id"]) == gc.KIND_SPHERE).sum())
            print(f"{name} camera {k}: {spheres} sphere pixels, {len(np.unique(e['id']))} distinct ids")
            assert spheres >= 100
            for ch in ("id", "depth", "normal"):
                assert np.array_equal(bits(on[ch]) if ch != "id" else on[ch], bits(off[ch]) if ch != "id" else off[ch]), (name, k, ch)
                if strict:
                    bad = (bits(on[ch]) != bits(e[ch])) if ch != "id" else (on[ch] != e[ch])
                    assert not bad.any(), f"{name} camera {k}: {int(bad.reshape(len(e['id']), -1).any(1).sum())} pixels differ from the oracle in {ch}"


@pytest.mark.parametrize("name", ["cloud", "giants"])
def test_the_tail_walks_three_dimensional_grids(R, oracle, tex, sky, name):
    """Everything through the tree-parallel tail (set_tpt(64, 1, -1)) at depth 8: its shadow rays always take the single walk, whatever the
    scene pairs.  Grid == linear scan in both builds, strict == oracle."""
    sc, cams = grid_layout(name)
    cam = cams[1]
    want, _, _ = oracle.render(_oracle_cam(oracle, cam, TW, TH), sc, tex, sky, TDEPTH)
    for strict in (True, False):
        with rendering(R, sc, tex, sky, TW, TH, cam=cam, depth=TDEPTH, strict=strict) as r:
            r.w.set_tpt(64, 1, -1)
            r.w.enable_counters(1)
            (p, f), = take(r)
            c = r.w.read_counters()
            assert c["tpt_tiles"] > 0 and c["tpt_nodes"] > 0, "the tail did not run"
            _grid_state(r, 1)
            r.w.set_grid(0)
            lin = take(r)
            assert not r.w.last_trace_flags() & F_GRID
            assert_same_frames(lin, p, f, f"{name} tail {'strict' if strict else 'fast'}")
            if strict:
                check_exact(p, want, f"{name} through the tail")


def test_spheres_that_are_not_finite_run_without_a_grid(R, oracle, tex, sky):
    """cloud with one NaN-centre sphere and one of infinite radius: the builder refuses the scene (no float of it reaches a float -> int
    conversion), so no grid is built and the strict frame of the linear scan equals the oracle's."""
    sc, cams = grid_layout("cloud")
    sp = sc.spheres.copy()
    sp["origin"][7] = (np.nan, 3.0, 9.0)
    sp["radius"][11] = np.inf
    sc = type(sc)(sp, sc.planes, sc.lights)
    want, _, cnt = oracle.render(_oracle_cam(oracle, cams[0], W, H), sc, tex, sky, DEPTH)
    assert cnt.int_cast_oor == 0 and cnt.oob_reads == 0                 # the reference itself is defined on this frame
    with rendering(R, sc, tex, sky, W, H, cam=cams[0], depth=DEPTH, strict=True) as r:
        (p, _), = take(r, rgb=False)
        g = r.w.get_grid()
        assert g is not None and g["built"] == 0 and g["pair"] == 0
        assert not r.w.last_trace_flags() & F_GRID
        check_exact(p, want, "cloud with spheres that are not finite")
