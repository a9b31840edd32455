"""The uniform-grid builder (csrc/scene_prep.c: wprep_grid_plan / wprep_grid_fill), called through the library, against the float64 model
of its contract in grid_common.py -- CPU only.  The per-axis clamp to 1..1024, the 10-bit boxes on both sides of bit 9 and the coarsening
loop above 2^22 cells are pinned HERE alone: no scene inside the float sphere test's domain reaches them on the GPU."""
import numpy as np
import pytest

import grid_common as G
from fuzz_scenes import GRID_3D, GRID_LAYOUTS, grid_layout

PAD = 0.25          # the positive reg_pad every layout is also built with


@pytest.mark.parametrize("reg_pad", [0.0, PAD])
@pytest.mark.parametrize("name", sorted(G.HOST_LAYOUTS))
def test_builder_meets_its_contract(name, reg_pad):
    # the slowest case is "cube" (600 000 spheres, about 5.3 M cell-list entries): 1.3 s with either pad, builder and checker together
    origin, radius = G.HOST_LAYOUTS[name]()
    sp = G.spheres_of(origin, radius)
    grid = G.build_grid(sp, reg_pad)
    assert grid["pairs"] <= G.GRID_MAX_PAIRS, f"{name}: the builder refused a finite scene"
    assert grid["reg_pad"] >= reg_pad and (grid["reg_pad"] == 0.0) == (reg_pad == 0.0)
    G.check_grid(origin, radius, reg_pad, grid)
    res = tuple(int(x) for x in grid["res"])
    print(f"{name} pad {reg_pad}: res {res}, {grid['pairs']} pairs, longest cell list {int(np.diff(grid['start'].astype(np.int64)).max())}")
    if name == "line":
        assert res == (1024, 1, 1)
        hi_x = G.unpack_box(grid["box"][1::2])[:, 0]
        assert hi_x.min() < 512 and hi_x.max() > 1000                         # box indices on both sides of bit 9
    if name == "plane":
        assert res == (1024, 1, 1024) if reg_pad == 0.0 else (res[1] == 1 and min(res[0], res[2]) > 512)    # (the pad thickens the slab: wider cells)
    if name == "cube":
        # the resolution the builder wants (cells about side_lo wide: 8 cells per sphere) is beyond 2^22 cells; what it returns is not
        assert 8 * len(radius) > 1 << 22 and (1 << 21) < grid["ncells"] <= 1 << 22 and min(res) > 64
    if name in ("apart", "huge"):
        assert min(res) >= 1 and np.isfinite(grid["cell"]).all()
    if name == "repeated":
        lens = np.diff(grid["start"].astype(np.int64))
        assert set(lens.tolist()) <= {0, 300}                                    # one sphere 300 times: every cell of its box lists all of them
    if name in GRID_3D:
        assert min(res) > 1, f"{name}: a layout named three-dimensional has a flat grid {res}"
    if name == "tower":
        assert res[1] >= 10 * max(res[0], res[2])
    if name == "coincident":
        lens = set(np.diff(grid["start"].astype(np.int64)).tolist())
        assert any(k > 100 and k % 2 for k in lens) and any(k > 100 and k % 2 == 0 for k in lens), sorted(lens)   # long lists of odd and of even length
    if name == "giants":
        lo, hi = G.unpack_box(grid["box"][-2]), G.unpack_box(grid["box"][-1])       # the r 10 giant: its box is the whole grid
        assert (lo == 0).all() and (hi == np.array(res) - 1).all() and np.diff(grid["start"].astype(np.int64)).min() >= 1
        span = G.unpack_box(grid["box"][-3]) - G.unpack_box(grid["box"][-4])        # the r 8 glass giant: a dozen cells across on every axis
        assert span.min() >= 11, span


def _small():
    origin, radius = G.HOST_LAYOUTS["ns257"]()
    return origin, radius, G.build_grid(G.spheres_of(origin, radius), PAD)


def _corrupt(name):
    """-> (origin, radius, a grid that breaks ONE clause of the contract, a word of the message that must name it)"""
    origin, radius, g = _small()
    lens = np.diff(g["start"].astype(np.int64))
    lo, hi = G.unpack_box(g["box"][0::2]), G.unpack_box(g["box"][1::2])
    if name == "missing":                     # a sphere missing from one cell of its box (start stays a consistent prefix sum)
        cell = int(np.argmax(lens))
        k = int(g["start"][cell])
        g["items"] = np.delete(g["items"], k)
        g["start"] = g["start"].copy()
        g["start"][cell + 1:] -= 1
        g["pairs"] -= 1
        return origin, radius, g, "not listed in every cell"
    if name == "descending":
        cell = int(np.argmax(lens >= 2))
        k = int(g["start"][cell])
        g["items"][[k, k + 1]] = g["items"][[k + 1, k]]
        return origin, radius, g, "strictly ascending"
    if name == "duplicate":                   # an entry listed twice in a cell in place of its neighbour: counts per cell stay right
        cell = int(np.argmax(lens >= 2))
        k = int(g["start"][cell])
        g["items"][k + 1] = g["items"][k]
        return origin, radius, g, "strictly ascending"
    if name == "small box":                   # a box one cell too small, with tables that agree with it: only containment can notice
        need = np.floor((origin[:, 0].astype(np.float64) + radius + PAD - float(g["gmin"][0])) / float(g["cell"][0]))
        i = int(np.argmax((hi[:, 0] > lo[:, 0]) & (hi[:, 0] == need)))     # a sphere whose last cell the model itself requires
        hi = hi.copy()
        hi[i, 0] -= 1
        g["start"], g["items"], g["box"] = G.tables_from_boxes(lo, hi, g["res"])
        g["pairs"] = len(g["items"])
        return origin, radius, g, "misses a cell"
    if name == "start end":
        g["start"] = g["start"].copy()
        g["start"][-1] += 1
        return origin, radius, g, "start\\[ncells\\]"
    if name == "bounds":                      # the low corner moved into the spheres
        g["gmin"] = g["gmin"].copy()
        g["gmin"][0] = np.float32((origin[:, 0] - radius).min() + 0.01)
        return origin, radius, g, "bounds cut"
    if name == "overflow":                    # hi.x = 1024: the eleventh bit spills into the y field
        i = int(np.argmax(lo[:, 0] > 0))
        g["box"] = g["box"].copy()
        g["box"][2 * i + 1] += np.uint32(1024 - hi[i, 0])
        return origin, radius, g, "box fields"
    if name == "top bits":
        g["box"] = g["box"].copy()
        g["box"][1] |= np.uint32(1 << 30)
        return origin, radius, g, "top bits"
    if name == "stray":                       # a sphere listed in a cell outside its box, in place of the cell's own last entry
        cell = int(np.argmax(lens >= 1))
        inside = set(g["items"][g["start"][cell]:g["start"][cell + 1]].tolist())
        x, y, z = cell % g["res"][0], (cell // g["res"][0]) % g["res"][1], cell // (g["res"][0] * g["res"][1])
        out = [i for i in range(len(radius)) if i not in inside and i > max(inside) and not ((lo[i] <= (x, y, z)).all() and (hi[i] >= (x, y, z)).all())]
        g["items"][g["start"][cell + 1] - 1] = out[0]
        return origin, radius, g, "outside its box"
    if name == "inv":
        g["inv"] = g["inv"].copy()
        g["inv"][1] = np.nextafter(g["inv"][1], np.float32(np.inf))
        return origin, radius, g, "inv is not"
    raise KeyError(name)


CORRUPTIONS = ["missing", "descending", "duplicate", "small box", "start end", "bounds", "overflow", "top bits", "stray", "inv"]


def test_the_model_accepts_the_grid_it_then_rejects_corrupted():
    origin, radius, g = _small()
    G.check_grid(origin, radius, PAD, g)
    assert min(g["res"]) > 1
    start, items, box = G.tables_from_boxes(G.unpack_box(g["box"][0::2]), G.unpack_box(g["box"][1::2]), g["res"])
    assert np.array_equal(start, g["start"]) and np.array_equal(items, g["items"]) and np.array_equal(box, g["box"])


@pytest.mark.parametrize("name", CORRUPTIONS)
def test_the_model_rejects_a_corrupted_grid(name):
    origin, radius, g, message = _corrupt(name)
    with pytest.raises(AssertionError, match=message):
        G.check_grid(origin, radius, PAD, g)


# ---- spheres that are not finite: the builder refuses the scene before any float reaches a float -> int conversion
def _poisoned(what):
    origin, radius = G.HOST_LAYOUTS["ns257"]()
    origin, radius = origin.copy(), radius.copy()
    if what == "nan centre":
        origin[17, 1] = np.nan
    elif what == "inf centre":
        origin[200, 2] = -np.inf
    elif what == "inf radius":
        radius[5] = np.inf
    elif what == "nan radius":
        radius[256] = np.nan
    elif what == "bounds overflow":           # finite, but c + r is not
        radius[5] = 3e38
        origin[5, 0] = 3e38
    return G.spheres_of(origin, radius)


@pytest.mark.parametrize("reg_pad", [0.0, PAD])
@pytest.mark.parametrize("what", ["nan centre", "inf centre", "inf radius", "nan radius", "bounds overflow"])
def test_a_scene_that_is_not_finite_gets_no_grid(what, reg_pad):
    pairs, g = G.plan(_poisoned(what), reg_pad)
    assert pairs == G.SIZE_MAX and pairs > G.GRID_MAX_PAIRS          # above any limit: the shim builds no grid and the scene takes the linear scan
    assert tuple(g["res"]) == (1, 1, 1) and g["ncells"] == 1 and np.isfinite(g["cell"]).all()


# ---- which shadow walk the GPU layouts take (the shim's rule restated in grid_common.expected_pair; the GPU tests read the shim's own answer)
@pytest.mark.parametrize("name", GRID_LAYOUTS)
def test_gpu_layouts_take_the_walk_they_name_and_stay_inside_the_domain(oracle, name):
    for lights, pair in (("small", 1), ("large", 0)):
        sc, cams = grid_layout(name, lights)
        assert 300 <= len(sc.spheres) <= 600 and len(sc.planes) == 1 and len(cams) == 2
        assert G.expected_pair(sc) == pair, (name, lights)
        assert sc.spheres["radius"].min() >= 0.05
        r = sc.lights["radius"]
        assert (r.max() <= 0.1) if lights == "small" else (r[0] >= 1.0)
        c, rad = sc.spheres["origin"].astype(np.float64), sc.spheres["radius"].astype(np.float64)
        for p in [cam["origin"] for cam in cams] + [tuple(o) for o in sc.lights["origin"]]:
            far = (np.linalg.norm(c - np.asarray(p, np.float64), axis=1) + rad).max()
            assert far <= 40.0, (name, lights, p, far)                     # every sphere, whole, within 40 units of every camera and light
        for cam in cams:                                                   # the floor, where shadow rays start, is not seen from afar either
            rays = oracle.raygen(oracle.camera(cam["origin"], cam["look"], cam["fov"], cam["focal"], 96, 72))
            height, dy = rays[:, 1].astype(np.float64) - float(sc.planes["point_in_plane"][0][1]), rays[:, 5].astype(np.float64)
            far = (dy < 0) & (height > -300.0 * dy)                        # the ray meets the floor more than 300 units away
            assert far.sum() <= 96, (name, cam, int(far.sum()))            # at most the pixel row at the horizon
        if lights == "large":                                              # the large light sits INSIDE the sphere set
            o = sc.lights["origin"][0].astype(np.float64)
            assert ((o > (c - rad[:, None]).min(0)) & (o < (c + rad[:, None]).max(0))).all()


# shadow rays from the primary hit points (gbuffer_common.expected_gbuffer at its 40 x 24 frame, both cameras) to the centres of the small
# lights whose factor (the oracle's wo_shadow) lies strictly between 0 and 1 -- glass in the way and nothing opaque: the single walk's
# "a transparent sphere counts once" rule and the paired walk's decide such samples.  The oracle counts 1731 (giants) and 2104 (coincident).
PARTIAL_MIN = {"giants": 850, "coincident": 1000}


@pytest.mark.parametrize("name", sorted(PARTIAL_MIN))
def test_layouts_with_glass_in_the_way_have_partially_shadowed_samples(oracle, tex, sky, name):
    import ctypes as C
    import gbuffer_common as gc
    from oracle.oracle_py import _Inputs
    sc, cams = grid_layout(name)
    inp = _Inputs(sc, tex, sky)
    f3 = C.c_float * 3
    lights = [f3(*l["origin"]) for l in sc.lights]
    partial = 0
    for cam in cams:
        e = gc.expected_gbuffer(oracle, sc, tex, sky, oracle.camera(cam["origin"], cam["look"], cam["fov"], cam["focal"], gc.WD, gc.HD))
        for i in np.nonzero(e["solid"])[0]:
            p = f3(*e["point"][i])
            partial += sum(0.0 < oracle.lib.wo_shadow(l, p, C.byref(inp.c)) < 1.0 for l in lights)
    print(f"{name}: {partial} partially shadowed samples")
    assert partial >= PARTIAL_MIN[name]
