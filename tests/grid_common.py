"""Shared by test_grid_host.py and test_gpu_grid_layouts.py: the uniform-grid builder of csrc/scene_prep.c called through the library, a
float64 numpy model of its CONTRACT (`check_grid`), the shim's pairing rule restated, and the layouts the host tests run.

The contract (scene_prep.h; hip_wrap_ext.h, clw_ext_get_grid), for n spheres (centre c, radius r) and a requested pad p >= 0:
  * res is in 1..1024 per axis, ncells their product and <= 2^22, cell finite and positive, inv the fp32 value of 1 / cell;
  * the bounds [gmin, gmin + cell * res] contain every box [c - |r| - p, c + |r| + p];
  * start has ncells + 1 entries, begins at 0, never decreases, and start[ncells] is the returned pair count;
  * the items of a cell are sphere indices < n in strictly ascending order;
  * box[2i], box[2i + 1] unpack (10 bits per axis, the top two bits clear) to lo <= hi <= res - 1;
  * sphere i is listed in exactly the cells of its box;
  * that box holds every cell whose (closed) extent meets the sphere's box above -- conservative containment: more cells are allowed.
A scene the builder refuses (a sphere that is not finite, bounds beyond a float) returns SIZE_MAX pairs and gets no tables."""
import ctypes as C

import numpy as np

from example_gui_opencl_raytracer_amd import scene as S

SIZE_MAX = (1 << 64) - 1
GRID_MAX_PAIRS = 1 << 25          # csrc/hip_wrap.cpp
GRID_MIN_SPHERES = 256            # csrc/whitted_params.h, WT_GRID_MIN_SPHERES: scenes above it get a grid
DENSITY = 1.6                     # what the shim passes
PAIR_RULE = 0.3                   # the shim pairs while the largest light radius is at most this share of the smallest cell side


class wprep_grid(C.Structure):
    _fields_ = [("gmin", C.c_float * 3), ("inv", C.c_float * 3), ("cell", C.c_float * 3), ("res", C.c_int32 * 3), ("ncells", C.c_uint32),
                ("reg_pad", C.c_float)]


def _lib():
    from example_gui_opencl_raytracer_amd import api
    L = api.load_library()
    L.wprep_grid_plan.restype = C.c_size_t
    L.wprep_grid_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.POINTER(wprep_grid)]
    L.wprep_grid_fill.restype = None
    L.wprep_grid_fill.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(wprep_grid), C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def spheres_of(origin, radius):
    """a wire-format sphere array (96 B each, plastic) from float centres [n, 3] and radii [n]"""
    origin = np.asarray(origin, np.float32).reshape(-1, 3)
    sp = np.zeros(len(origin), S.SPHERE)
    sp["origin"] = origin
    sp["radius"] = np.asarray(radius, np.float32)
    return sp


def plan(spheres, reg_pad=0.0, density=DENSITY):
    """wprep_grid_plan alone -> (pairs, dict of the planned grid)"""
    spheres = np.ascontiguousarray(spheres, S.SPHERE)
    g = wprep_grid()
    pairs = int(_lib().wprep_grid_plan(spheres.ctypes.data, len(spheres), density, reg_pad, C.byref(g)))
    G = dict(pairs=pairs, res=np.array(g.res[:], np.int64), ncells=int(g.ncells), cell=np.array(g.cell[:], np.float32),
             inv=np.array(g.inv[:], np.float32), gmin=np.array(g.gmin[:], np.float32), reg_pad=float(g.reg_pad), _c=g)
    return pairs, G


def build_grid(spheres, reg_pad=0.0, density=DENSITY):
    """plan + fill -> the grid as a dict (res, ncells, cell, inv, gmin, reg_pad, pairs, start, items, box); a refused scene has no tables"""
    spheres = np.ascontiguousarray(spheres, S.SPHERE)
    pairs, G = plan(spheres, reg_pad, density)
    g = G.pop("_c")
    if pairs > GRID_MAX_PAIRS:
        return G
    G["start"] = np.full(G["ncells"] + 1, 0xDEADBEEF, np.uint32)
    G["items"] = np.full(max(pairs, 1), 0xDEADBEEF, np.uint32)
    G["box"] = np.full(2 * len(spheres), 0xDEADBEEF, np.uint32)
    _lib().wprep_grid_fill(spheres.ctypes.data, len(spheres), C.byref(g), G["start"].ctypes.data, G["items"].ctypes.data, G["box"].ctypes.data)
    G["items"] = G["items"][:pairs]
    return G


def expected_pair(scene):
    """The walk the shim chooses for a grid scene (csrc/hip_wrap.cpp, prepare_scene), restated: 1 = the paired shadow walk, 0 = the single
    one, None = no grid at all."""
    if len(scene.spheres) <= GRID_MIN_SPHERES:
        return None
    r = np.abs(scene.lights["radius"].astype(np.float32))
    maxr = np.float32(r.max()) if len(r) else np.float32(0)
    pair = 0
    if maxr > 0 and np.isfinite(maxr):
        pairs, G = plan(scene.spheres, float(maxr))
        pair = int(maxr <= np.float32(PAIR_RULE) * G["cell"].min() and pairs <= GRID_MAX_PAIRS)
    if not pair:
        pairs, G = plan(scene.spheres, 0.0)
    return pair if pairs <= GRID_MAX_PAIRS else None


def unpack_box(word):
    word = np.asarray(word, np.uint32).astype(np.int64)
    return np.stack([word & 1023, (word >> 10) & 1023, (word >> 20) & 1023], -1)


def tables_from_boxes(lo, hi, res):
    """start / items / box of the cell lists that list sphere i in exactly the cells lo[i] .. hi[i] (a plain loop: small scenes only)"""
    res = [int(x) for x in res]
    cells = [[] for _ in range(res[0] * res[1] * res[2])]
    for i in range(len(lo)):
        for z in range(lo[i][2], hi[i][2] + 1):
            for y in range(lo[i][1], hi[i][1] + 1):
                for x in range(lo[i][0], hi[i][0] + 1):
                    cells[(z * res[1] + y) * res[0] + x].append(i)
    start = np.zeros(len(cells) + 1, np.uint32)
    start[1:] = np.cumsum([len(c) for c in cells])
    items = np.array([i for c in cells for i in c], np.uint32)
    pack = lambda v: (v[:, 0] | v[:, 1] << 10 | v[:, 2] << 20).astype(np.uint32)
    box = np.zeros(2 * len(lo), np.uint32)
    box[0::2], box[1::2] = pack(np.asarray(lo, np.int64)), pack(np.asarray(hi, np.int64))
    return start, items, box


def check_grid(origin, radius, reg_pad, G):
    """Hold a built grid to the contract at the top of this file; AssertionError names the clause that fails."""
    c = np.asarray(origin, np.float64).reshape(-1, 3)
    r = np.abs(np.asarray(radius, np.float64)).reshape(-1)
    n = len(c)
    res, cell, gmin = np.asarray(G["res"], np.int64), np.asarray(G["cell"], np.float32), np.asarray(G["gmin"], np.float32)
    assert ((res >= 1) & (res <= 1024)).all(), f"resolution outside 1..1024: {res}"
    assert G["ncells"] == int(res.prod()) and G["ncells"] <= 1 << 22, f"cell count: {G['ncells']} for {res}"
    assert np.isfinite(cell).all() and (cell > 0).all() and np.isfinite(gmin).all(), f"cell sides / corner: {cell} {gmin}"
    assert np.array_equal(np.asarray(G["inv"], np.float32).view(np.uint32), (np.float32(1) / cell).view(np.uint32)), "inv is not the fp32 value of 1 / cell"
    lo_w, hi_w = c - r[:, None] - reg_pad, c + r[:, None] + reg_pad                      # every sphere's box, widened
    g0, cs = gmin.astype(np.float64), cell.astype(np.float64)
    g1 = g0 + cs * res
    assert (lo_w >= g0).all() and (hi_w <= g1).all(), "the bounds cut a sphere's box"
    start, items, box = G["start"], G["items"], G["box"]
    assert len(start) == G["ncells"] + 1 and start[0] == 0 and (np.diff(start.astype(np.int64)) >= 0).all(), "start is not a prefix sum from 0"
    assert int(start[-1]) == G["pairs"] == len(items), f"start[ncells] {int(start[-1])}, returned pairs {G['pairs']}, items {len(items)}"
    assert len(box) == 2 * n and (box >> np.uint32(30) == 0).all(), "box words: count or top bits"
    lo, hi = unpack_box(box[0::2]), unpack_box(box[1::2])
    assert (lo <= hi).all() and (hi <= res - 1).all(), "box fields: lo <= hi <= res - 1 violated"
    if len(items):
        assert int(items.max()) < n, "item out of range"
        first = np.zeros(len(items) + 1, bool)
        first[start] = True                                                            # entries that open a cell's list
        assert ((items[1:] > items[:-1]) | first[1:-1]).all(), "items of a cell are not strictly ascending"
    cells_of = np.repeat(np.arange(G["ncells"], dtype=np.int64), np.diff(start.astype(np.int64)))
    xyz = np.stack([cells_of % res[0], (cells_of // res[0]) % res[1], cells_of // (res[0] * res[1])], -1)
    assert ((xyz >= lo[items]) & (xyz <= hi[items])).all(), "a sphere is listed in a cell outside its box"
    listed = np.bincount(items, minlength=n) if len(items) else np.zeros(n, np.int64)
    assert np.array_equal(listed, (hi - lo + 1).prod(1)), "a sphere is not listed in every cell of its box"
    # every cell whose closed extent [g0 + k cs, g0 + (k + 1) cs] meets [lo_w, hi_w]: k >= (lo_w - g0) / cs - 1 and k <= (hi_w - g0) / cs
    k_min = np.clip(np.ceil((lo_w - g0) / cs - 1.0), 0, res - 1).astype(np.int64)
    k_max = np.clip(np.floor((hi_w - g0) / cs), 0, res - 1).astype(np.int64)
    assert (lo <= k_min).all() and (hi >= k_max).all(), "a box misses a cell its sphere's widened bounding box meets"


# ---- the layouts of the host tests: name -> (centres [n, 3], radii [n]); built on demand, none of them cached
def _flat():
    sp = S.sphere_grid_scene(24, 24).spheres
    return sp["origin"], sp["radius"]


def _gpu_layout(name):
    def make():
        from fuzz_scenes import grid_layout
        sp = grid_layout(name)[0].spheres
        return sp["origin"], sp["radius"]
    return make


def _line():
    """600 spheres of r 0.3 over 1 500 units: 1024 x 1 x 1, box indices on both sides of bit 9"""
    o = np.zeros((600, 3), np.float32)
    o[:, 0] = np.linspace(0.0, 1500.0, 600)
    return o, np.full(600, 0.3, np.float32)


def _plane():
    """tiny spheres spread wide on a plane: 1024 x 1 x 1024, capped on both axes"""
    rng = np.random.default_rng(5)
    o = np.zeros((2000, 3), np.float32)
    o[:, 0], o[:, 2] = rng.uniform(0, 12000, 2000), rng.uniform(0, 12000, 2000)
    return o, np.full(2000, 0.05, np.float32)


def _cube():
    """about 600 000 small spheres in a cube: the resolution wanted exceeds 2^22 cells, so the coarsening loop runs"""
    rng = np.random.default_rng(6)
    return rng.uniform(0, 100, (600_000, 3)).astype(np.float32), np.full(600_000, 0.05, np.float32)


def _ns257():
    rng = np.random.default_rng(7)
    return rng.uniform(-5, 5, (257, 3)).astype(np.float32), rng.uniform(0.05, 0.5, 257).astype(np.float32)


def _repeated():
    return np.tile(np.float32([1.5, 2.5, -3.5]), (300, 1)), np.full(300, 0.7, np.float32)


def _radius0():
    rng = np.random.default_rng(8)
    return rng.uniform(-5, 5, (300, 3)).astype(np.float32), np.zeros(300, np.float32)


def _negative():
    """a negative radius is the sphere of its magnitude (the sphere test only reads r * r)"""
    o, r = _ns257()
    return o, -r


def _apart():
    """two groups of small spheres 1e30 apart: cells per axis beyond any int before the clamp"""
    o, r = _ns257()
    o = o.copy()
    o[::2, 0] += np.float32(1e30)
    return o, r


def _huge():
    """one finite radius of 1e30 among small spheres"""
    o, r = _ns257()
    r = r.copy()
    r[100] = 1e30
    return o, r


HOST_LAYOUTS = {"flat": _flat, "line": _line, "plane": _plane, "cube": _cube, "ns257": _ns257, "repeated": _repeated, "radius0": _radius0,
                "negative": _negative, "apart": _apart, "huge": _huge}
HOST_LAYOUTS.update({name: _gpu_layout(name) for name in ("cloud", "giants", "coincident", "touching", "tower", "offset")})
