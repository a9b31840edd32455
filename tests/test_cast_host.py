"""The ray queries on the CPU (include/hip_wrap_ext.h: clw_host_cast_rays, clw_host_occluded_rays; csrc/cast_host.c): the C ABI against the header
and the ctypes mirror, the host definition against the numpy restatement of tests/cast_common.py -- bit for bit, no tolerance anywhere --,
closed forms, the oracle's primary hits, every refusal, and the host-side choice of the kernel instantiation (csrc/launch_plan.c: wt_plan_cast)."""
import ctypes as C
import re

import numpy as np
import pytest

import cast_common as cc
import gbuffer_common as gc
from example_gui_opencl_raytracer_amd import api
from render_common import header_text

F = np.float32
NEW_SYMBOLS = ["clw_host_cast_rays", "clw_host_occluded_rays", "clw_ext_cast_rays", "clw_ext_occluded_rays", "clw_ext_cast_rays_device"]
SEED = 17


# ------------------------------------------------------------------ 1. header, library and mirror
def test_header_library_and_mirror_agree():
    code = header_text(comments=False)
    L = api.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), f"hip_wrap_ext.h does not declare {name}"
        assert name in api.SYMBOLS
        assert hasattr(L, name), f"the library does not export {name}"
        assert getattr(L, name).argtypes is not None
    assert L.clw_host_cast_rays.restype is C.c_int and L.clw_ext_cast_rays.restype is C.c_uint32 and L.clw_ext_cast_rays_device.restype is C.c_uint32
    # both structures: 32 bytes, the header's fields at the header's offsets, in ctypes and in numpy
    for struct, dtype, name, fields in ((api.clw_ray, api.RAY_QUERY, "clw_ray", [("origin", 0, 12), ("tmax", 12, 4), ("dir", 16, 12), ("ignore", 28, 4)]),
                                        (api.clw_hit, api.HIT, "clw_hit", [("t", 0, 4), ("id", 4, 4), ("normal", 8, 12), ("point", 20, 12)])):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), code, flags=re.S)
        assert m, f"hip_wrap_ext.h does not define {name}"
        declared = [re.sub(r"\[\d+\]", "", decl.split()[-1]) for decl in m.group(1).split(";") if decl.strip()]
        assert declared == [f[0] for f in fields] == [f[0] for f in struct._fields_] == list(dtype.names)
        assert C.sizeof(struct) == 32 and dtype.itemsize == 32
        assert [(getattr(struct, f).offset, getattr(struct, f).size) for f, _, _ in fields] == [(o, s) for _, o, s in fields]
        assert [(dtype.fields[f][1], dtype.fields[f][0].itemsize) for f, _, _ in fields] == [(o, s) for _, o, s in fields]
    defs = dict(re.findall(r"#define\s+(CLW_\w+)\s+(0x[0-9A-Fa-f]+|\d+)u\b", header_text()))
    want = dict(CLW_CAST_SPHERES=api.CAST_SPHERES, CLW_CAST_PLANES=api.CAST_PLANES, CLW_CAST_LIGHTS=api.CAST_LIGHTS, CLW_CAST_KINDS=api.CAST_KINDS,
                CLW_CAST_OPAQUE=api.CAST_OPAQUE, CLW_TIMING_CAST=api.TIMING_CAST)
    for name, value in want.items():
        assert int(defs[name], 0) == value, name
    assert (api.CAST_SPHERES, api.CAST_PLANES, api.CAST_LIGHTS, api.CAST_KINDS, api.CAST_OPAQUE, api.TIMING_CAST) == (1, 2, 4, 7, 8, 0x43415354)
    assert (cc.SPHERES, cc.PLANES, cc.LIGHTS, cc.KINDS, cc.OPAQUE) == (1, 2, 4, 7, 8)
    text = header_text()
    for word in ("NOT normalised", "NOT the trace kernel's", "equal t keeps the earlier primitive", "WITHOUT the EPSILON offset", "never flipped",
                 "sorting incoherent rays by grid cell", "per-ray flags", "the texel or the material", 'a latched "bounce"'):
        assert word in text, word
    from example_gui_opencl_raytracer_amd.renderer import Renderer
    for name in ("cast_rays", "cast_rays_device", "line_of_sight"):
        assert callable(getattr(Renderer, name))
    for name in ("cast_rays", "occluded_rays", "cast_rays_device"):
        assert callable(getattr(api.ClWrap, name))


# ------------------------------------------------------------------ 2. and 3. the C definition equals the numpy model
def check_case(scene, rays, flags, what):
    """the definition against the model, nearest and any; -> the expected hits"""
    want, want_blocked = cc.cast_model(rays, flags, scene.spheres, scene.planes, scene.lights)
    got = api.cast_rays_host(rays, flags, scene.spheres, scene.planes, scene.lights)
    blocked = api.occluded_rays_host(rays, flags, scene.spheres, scene.planes, scene.lights)
    differ = int((got.view(np.uint8).reshape(-1, 32) != want.view(np.uint8).reshape(-1, 32)).any(1).sum())
    print(f"{what}: {differ} of {rays.size} hits differ from the model; {int(blocked.sum())} blocked")
    assert got.dtype == api.HIT and got.tobytes() == want.tobytes(), what
    assert blocked.dtype == np.uint8 and np.array_equal(blocked, want_blocked), what
    assert np.array_equal(blocked != 0, got["id"] != cc.ID_NONE), what          # 3. occluded == (nearest.id != CLW_ID_NONE)
    return got


@pytest.mark.parametrize("opaque", [0, cc.OPAQUE], ids=["all", "opaque"])
@pytest.mark.parametrize("kinds", cc.KIND_COMBOS)
@pytest.mark.parametrize("name", ["small", "planes", "spheres"])
def test_the_definition_equals_the_numpy_model(name, kinds, opaque):
    scene, flags = cc.scene_of(name), kinds | opaque
    base, info = cc.make_rays(scene, cc.N_HOST, SEED)
    for tmax in cc.TMAX:
        for per_ray in (False, True):
            rays = cc.with_tmax(base, tmax, per_ray)
            what = f"{name} flags {flags} tmax {tmax} {'per ray' if per_ray else 'scalar'}"
            hits = check_case(scene, rays, flags, what)
            if cc.kinds_present(scene, flags):
                cc.assert_decides(scene, rays, flags, hits, what)
            else:                                                      # (lights alone... every scene has lights; a kind the scene lacks)
                assert (hits["id"] == cc.ID_NONE).all()


@pytest.mark.parametrize("flags", [cc.SPHERES | cc.PLANES, cc.KINDS | cc.OPAQUE])
@pytest.mark.parametrize("name", ["cloud", "ns257"])
def test_the_definition_equals_the_numpy_model_on_the_big_scenes(name, flags):
    scene = cc.scene_of(name)
    base, info = cc.make_rays(scene, cc.N_HOST, SEED)
    for tmax, per_ray in ((np.inf, False), (3.0, True)):
        rays = cc.with_tmax(base, tmax, per_ray)
        what = f"{name} flags {flags} tmax {tmax} {'per ray' if per_ray else 'scalar'}"
        cc.assert_decides(scene, rays, flags, check_case(scene, rays, flags, what), what)


@pytest.mark.parametrize("name", list(cc.SCENES))
def test_the_ray_sets_hold_what_they_are_made_for(name):
    scene = cc.scene_of(name)
    rays, info = cc.make_rays(scene, cc.N_HOST, SEED)
    hits = api.cast_rays_host(rays, cc.KINDS, scene.spheres, scene.planes, scene.lights)
    assert rays.size == cc.N_HOST and all(len(info[k]) for k in ("away", "odd", "bounce", "edge_at", "edge_below"))
    assert (hits["id"][info["away"]] == cc.ID_NONE).all() and np.isinf(hits["t"][info["away"]]).all()      # certain misses
    assert (hits["id"][info["odd"]] == cc.ID_NONE).all()                 # a zero direction, a NaN, an infinite direction meet nothing
    odd = rays[info["odd"]]
    assert (odd["dir"] == 0).all(1).any() and np.isnan(odd["origin"]).any() and np.isnan(odd["tmax"]).any() and np.isinf(odd["dir"]).any()
    assert (np.abs(np.linalg.norm(rays["dir"][:20].astype(np.float64), axis=1) - 1) > 1e-3).all()      # directions are not unit
    # tmax = t exactly still meets the primitive; one ulp less meets it no more
    assert np.array_equal(hits["id"][info["edge_at"]], info["edge_id"]) and np.array_equal(hits["t"][info["edge_at"]], rays["tmax"][info["edge_at"]])
    assert (hits["id"][info["edge_below"]] != info["edge_id"]).all()
    # a second bounce leaves the primitive it starts on alone
    assert (hits["id"][info["bounce"]] != rays["ignore"][info["bounce"]]).all()
    if len(scene.spheres):                                              # rays that start inside a sphere meet its far side
        inside = info["inside"]
        assert len(inside) and (hits["id"][inside] != cc.ID_NONE).all() and (hits["t"][inside] > 0).all()


def test_coincident_spheres_the_lower_index_wins():
    scene = cc.scene_of("small")
    assert np.array_equal(scene.spheres["origin"][1], scene.spheres["origin"][3]) and scene.spheres["radius"][1] == scene.spheres["radius"][3]
    rng = np.random.default_rng(3)
    c = scene.spheres["origin"][1]
    o = (c + rng.normal(size=(40, 3)) * 3).astype(F)
    rays = api.make_rays(o, c - o)
    hits = api.cast_rays_host(rays, cc.SPHERES, scene.spheres, None, None)
    assert (hits["id"] != 3).all() and (hits["id"] == 1).sum() > 20
    rays = api.make_rays(o, c - o, ignore=1)                              # ... and with it ignored, its twin answers with the same t
    again = api.cast_rays_host(rays, cc.SPHERES, scene.spheres, None, None)
    sel = hits["id"] == 1
    assert (again["id"][sel] == 3).all() and np.array_equal(again["t"][sel], hits["t"][sel])


@pytest.mark.parametrize("reg_pad", [0.0, 0.1])
@pytest.mark.parametrize("name", list(cc.TANGENT_VARIANTS))
def test_the_tangent_pair_ties_across_cells(name, reg_pad):
    """The premise of the GPU tests of the tie rule (test_gpu_cast.py, test_gpu_layers.py: wt_sink_nearest::grid_take takes an equal t only from
    a lower index): A and B give the same t bits, the definition keeps the lower index, and on the grid the library builds -- without a pad
    and with the pad of the scene's lights -- the ray is in a cell that lists B and not A before it is in the cell of the hit, which lists
    both.  Without that cell the walk would meet the pair in one cell's ascending order and the GPU tests would prove nothing."""
    import layers_common as lc
    sc = cc.scene_of(name)
    a, b = cc.tangent_ids(name)
    lo, hi = min(a, b), max(a, b)
    assert len(sc.spheres) == cc.TANGENT_FILLERS + 2 > 256
    assert bool(sc.spheres["material"]["transperent"][a]) == cc.TANGENT_VARIANTS[name].get("glass", True) and not sc.spheres["material"]["transperent"][b]
    rays = cc.tangent_exact_rays(name)
    one, below = F(1), np.nextafter(F(1), F(0))
    for only in (a, b):                                                  # each alone: t = 1, bit for bit
        h = api.cast_rays_host(rays[0::5], cc.SPHERES, sc.spheres[only:only + 1], None, None)
        assert (h["id"] == 0).all() and np.array_equal(h["t"].view(np.uint32), np.full(len(h), one).view(np.uint32)), only
    for flags, planes, lights in ((cc.SPHERES, None, None), (cc.SPHERES | cc.PLANES, sc.planes, sc.lights), (cc.KINDS, sc.planes, sc.lights)):
        hits = api.cast_rays_host(rays, flags, sc.spheres, planes, lights)
        model = cc.cast_model(rays, flags, sc.spheres, planes, lights)[0]
        assert hits.tobytes() == model.tobytes()
        for k in range(len(cc.TANGENT_EXACT)):
            h = hits[5 * k:5 * k + 5]
            assert h["id"].tolist() == [lo, b, a, lo, cc.ID_NONE], (name, flags, k, h["id"])      # plain, ignore A, ignore B, tmax 1, tmax below 1
            assert h["t"][:4].tolist() == [1.0] * 4 and np.isposinf(h["t"][4])
        two = api.cast_layers_host(rays, flags, 2, sc.spheres, planes, lights)
        assert two["id"][:, 0::5].T.tolist() == [[lo, hi]] * len(cc.TANGENT_EXACT) and (two["t"][:, 0::5] == one).all()
        t, ids, count = lc.candidates(rays, flags, sc.spheres, planes, lights)
        assert np.array_equal(two["id"], lc.layers_of(t, ids, 2)["id"])
    opaque = api.cast_rays_host(rays, cc.SPHERES | cc.OPAQUE, sc.spheres, None, None)
    assert opaque["id"][0] == (b if sc.spheres["material"]["transperent"][a] else lo)
    assert rays["tmax"][4] == below and below < one
    cells, G = cc.tangent_cells(name, reg_pad)
    print(f"{name} pad {reg_pad}: grid {G['res'].tolist()} cells of {G['cell'].tolist()}; cells before the hit that list B alone: {[len(c) for c, _ in cells]}")
    assert (G["res"] > 1).all()
    for k, (b_only, both_at_hit) in enumerate(cells):
        assert both_at_hit, (name, k)
        if k == 0:                       # the ray along x: 5.5 units of B's box before A's
            assert len(b_only) >= 2, (name, reg_pad, b_only)
        # (the ray along z has 1.75 units of B's box before A's, about one cell: it rides along, and decides where it finds such a cell)


# ------------------------------------------------------------------ 4. closed forms with dyadic values
def test_closed_forms():
    sc = cc.scene_of("small")
    floor = sc.planes[:1]
    h = api.cast_rays_host(api.make_rays([(0, 5, 0)], [(0, -1, 0)]), cc.PLANES, None, floor, None)[0]
    assert h["t"] == 5 and h["id"] == cc.KIND_PLANE and h["point"].tolist() == [0, 0, 0] and h["normal"].tolist() == [0, 1, 0]
    ball = sc.spheres[:1].copy()
    ball["origin"], ball["radius"] = (0, 0, 4), 1.0
    h = api.cast_rays_host(api.make_rays([(0, 0, 0)], [(0, 0, 1)]), cc.SPHERES, ball, None, None)[0]
    assert h["t"] == 3 and h["id"] == 0 and h["point"].tolist() == [0, 0, 3] and h["normal"].tolist() == [0, 0, -1]
    h = api.cast_rays_host(api.make_rays([(0, 0, 4)], [(0, 0, 1)]), cc.SPHERES, ball, None, None)[0]
    assert h["t"] == 1 and h["point"].tolist() == [0, 0, 5] and h["normal"].tolist() == [0, 0, 1]           # from the centre: the far root
    # t is in units of |d|: twice the direction, half the t, the same point; and a -> b with tmax = 1 ends exactly at b
    h = api.cast_rays_host(api.make_rays([(0, 0, 0)], [(0, 0, 2)]), cc.SPHERES, ball, None, None)[0]
    assert h["t"] == 1.5 and h["point"].tolist() == [0, 0, 3]
    rays = api.make_rays([(0, 0, 0), (0, 0, 0)], [(0, 0, 3), (0, 0, 2.75)], tmax=1.0)
    assert api.occluded_rays_host(rays, cc.SPHERES, ball, None, None).tolist() == [1, 0]


# ------------------------------------------------------------------ 5. against the oracle's primary hits
@pytest.mark.parametrize("name", ["A", "B", "D0", "E"])
def test_a_cast_of_the_camera_rays_reproduces_the_primary_hits(oracle, tex, sky, name):
    key, w, h, cam, _ = gc.CASES[name]
    e = gc.expected_case(oracle, name, tex, sky)
    sc = gc.case_scene(name)
    ocam = oracle.camera(cam["origin"], cam["look"], cam["fov"], cam["focal"], w, h)
    records = api.projection_rays(api.clw_camera.from_buffer_copy(bytes(ocam)), api.projection(api.PROJ_PERSPECTIVE))
    hits = api.cast_rays_host(api.make_rays(records[:, 0:3], records[:, 4:7]), cc.SPHERES | cc.PLANES, sc.spheres, sc.planes, sc.lights)
    lit = (e["id"] != gc.ID_NONE) & (gc.kind_of(e["id"]) == gc.KIND_LIGHT)
    assert lit.sum() < w * h / 4
    sel = ~lit
    with np.errstate(invalid="ignore"):
        point = hits["normal"] * F(0.001) + hits["point"]                     # the EPSILON offset, in float32: n * eps + p
    bad = {k: int((a[sel].view(np.uint32) != b[sel].view(np.uint32)).sum()) for k, a, b in
           (("depth", hits["t"], e["depth"]), ("id", hits["id"], e["id"]), ("normal", hits["normal"], e["normal"]), ("point", point, e["point"]))}
    print(f"case {name}: {int(sel.sum())} of {w * h} pixels compared, differing words {bad}")
    assert not any(bad.values())


# ------------------------------------------------------------------ 6. refusals: 0, nothing written
def test_every_refusal():
    L = api.load_library()
    sc = cc.scene_of("small")
    rays = np.ascontiguousarray(cc.make_rays(sc, 12, 1)[0])
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(which, rays=rays, n=12, flags=3, sp=sc.spheres, ns=4, pl=sc.planes, npl=2, li=sc.lights, nl=3, out=True):
        o = np.full(12 * (32 if which == "cast" else 1), 0xA5, np.uint8)
        f = L.clw_host_cast_rays if which == "cast" else L.clw_host_occluded_rays
        r = f(P(rays), n, flags, P(sp), ns, P(pl), npl, P(li), nl, P(o) if out else None)
        assert (o == 0xA5).all() or r == 1
        return r

    for which in ("cast", "occluded"):
        assert call(which) == 1 and call(which, flags=15) == 1 and call(which, n=1) == 1
        assert call(which, sp=None, ns=0) == 1 and call(which, pl=None, npl=0) == 1 and call(which, li=None, nl=0) == 1
        for kw in (dict(rays=None), dict(out=False), dict(sp=None), dict(pl=None), dict(li=None), dict(n=0), dict(n=1 << 30), dict(n=0xFFFFFFFF),
                   dict(flags=0), dict(flags=8), dict(flags=16 | 3), dict(flags=0x80000001)):
            assert call(which, **kw) == 0, (which, kw)
    with pytest.raises(ValueError):
        api.cast_rays_host(rays, 0, sc.spheres, sc.planes, sc.lights)
    with pytest.raises(ValueError):
        api.occluded_rays_host(rays[:0], 3, sc.spheres, sc.planes, sc.lights)


# ------------------------------------------------------------------ 7. the plan: which instantiation runs
class wt_cast_class(C.Structure):
    _fields_ = [("flags", C.c_int32), ("dyn_lds", C.c_uint32), ("groups", C.c_uint32), ("batches", C.c_uint32)]


WT_F_GEOM_LDS, WT_F_GRID = 4, 16                      # csrc/whitted_params.h
WT_V_GEOM_GLOBAL, WT_V_NO_GRID = 1, 8                 # csrc/launch_plan.h
WT_CAST_BATCHES_LDS = 1                               # csrc/launch_plan.h: batches of 64 rays a wave serves per staging (the measured optimum)


def plan_cast(variant, ns, geom_f4, grid_usable, n, batches_req=0):
    L = api.load_library()
    L.wt_plan_cast.restype = wt_cast_class
    L.wt_plan_cast.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32]
    c = L.wt_plan_cast(variant, ns, geom_f4, grid_usable, n, batches_req)
    return c.flags, c.dyn_lds, c.groups, c.batches


def test_the_plan_picks_lds_global_or_grid():
    small = 4 + 2 * 2 + 2 * 3 + 2                     # the small scene's float4s: spheres, planes, lights, the side table
    assert plan_cast(0, 4, small, 0, 4099) == (WT_F_GEOM_LDS, small * 16, -(-65 // WT_CAST_BATCHES_LDS), WT_CAST_BATCHES_LDS)
    assert plan_cast(WT_V_GEOM_GLOBAL, 4, small, 0, 4099) == (0, 0, 65, 1)
    big = 257 + 2 + 6 + 1
    assert plan_cast(0, 257, big, 1, 193) == (WT_F_GRID, 0, 4, 1)
    assert plan_cast(WT_V_NO_GRID, 257, big, 1, 193) == (0, 0, 4, 1)               # grid built, switched off by the variant
    assert plan_cast(0, 257, big, 0, 193) == (0, 0, 4, 1)                          # ... or not usable: more than 256 spheres are never staged
    assert plan_cast(0, 200, 1024, 0, 64)[:2] == (WT_F_GEOM_LDS, 16384)            # exactly 16 KiB is staged
    assert plan_cast(0, 200, 1025, 0, 64)[:2] == (0, 0)                            # a float4 more is not
    # the launch shape: one wave per `batches` batches of 64 rays, the last one ragged
    for n in (1, 63, 64, 65, 193, 4099, (1 << 30) - 1):
        for req in (0, 1, 2, 8, 1000):
            flags, lds, groups, batches = plan_cast(0, 4, small, 0, n, req)
            assert batches == (min(req, 64) if req else WT_CAST_BATCHES_LDS)
            assert groups * batches * 64 >= n > (groups - 1) * batches * 64
    assert plan_cast(0, 4, small, 0, 0)[2] == 0 and plan_cast(0, 4, small, 0, 1 << 30)[2] == 0      # counts the queries refuse
