"""The proximity queries' definition on the host (include/hip_wrap_ext.h: clw_host_nearest_surface, clw_host_within_reach,
clw_host_near_surfaces; csrc/near_host.c) against the numpy model of tests/near_common.py -- bit for bit --, its own properties (prefix, layer 0,
within), closed forms against a float64 restatement, every refusal, the host-side choice of the kernel instantiation (csrc/launch_plan.c:
wt_plan_near) and the lattice scene, exactly.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import cast_common as cc
import near_common as nc
from example_gui_opencl_raytracer_amd import api

F = np.float32
_sets = {}


def probe_set(name):
    """(scene, probes, ignore, info) of a scene: built once, never written to"""
    if name not in _sets:
        sc = cc.scene_of(name)
        _sets[name] = (sc,) + nc.make_probes(sc, nc.N_HOST, seed=nc.N_HOST)
    return _sets[name]


def host(probes, ignore, flags, sc, K=nc.KMAX):
    hits = api.nearest_surface_host(probes, flags, sc.spheres, sc.planes, sc.lights, ignore)
    within = api.within_reach_host(probes, flags, sc.spheres, sc.planes, sc.lights, ignore)
    lists = api.near_surfaces_host(probes, flags, K, sc.spheres, sc.planes, sc.lights, ignore)
    return hits, within, lists


# ------------------------------------------------------------------ 1. against the model, and what the probe sets decide
@pytest.mark.parametrize("name", nc.SCENE_NAMES)
def test_the_definition_equals_the_model(name):
    sc, probes, ignore, info = probe_set(name)
    for flags in nc.KIND_COMBOS + (nc.KINDS | nc.OPAQUE, nc.SPHERES | nc.OPAQUE):
        hits, within, lists = host(probes, ignore, flags, sc)
        m_hits, m_within, m_d, m_id = nc.near_model(probes, ignore, flags, sc.spheres, sc.planes, sc.lights)
        assert hits.tobytes() == m_hits.tobytes(), (name, flags)
        assert np.array_equal(within, m_within), (name, flags)
        assert lists["d"].tobytes() == m_d.tobytes() and np.array_equal(lists["id"], m_id), (name, flags)
        if flags == nc.KINDS:
            s = nc.assert_decides(probes, hits, within, api.near_surfaces_host(probes, flags, 4, sc.spheres, sc.planes, sc.lights, ignore)["d"], 4, name)
            print(f"{name}: {s}, inside a sphere or light {float((hits['t'] < 0).mean()):.2f}")
            assert s["negative"] == bool(len(sc.spheres)), name                 # some probe lies inside a sphere wherever there are spheres
            # the odd probes are there, and the edge pairs decide: reach = d keeps the surface, the float below it loses it
            odd = probes[info["odd"]]
            assert np.isnan(odd["point"]).any() and np.isnan(odd["reach"]).any() and np.isinf(odd["point"]).any()
            assert (len(info["centre"]) > 0) == bool(len(sc.spheres)) and (len(info["faces"]) > 0) == (len(sc.spheres) > 256)
            at, below = hits[info["edge_at"]], hits[info["edge_below"]]
            assert len(at) > 100 and (at["t"] == probes["reach"][info["edge_at"]]).all() and (at["id"] != nc.ID_NONE).all()
            assert not (below["t"] == at["t"]).any()
            assert (ignore[info["ignoring"]] != nc.ID_NONE).all() and not (hits["id"][info["ignoring"]] == ignore[info["ignoring"]]).any()
            if len(info["centre"]):              # at a centre: d = -r and the NaNs stored as computed (unless a larger sphere around it is nearer)
                c = hits[info["centre"]]
                assert (c["t"] < 0).any() and (np.isnan(c["normal"]).all(1) & np.isnan(c["point"]).all(1) & (c["t"] < 0)).any()


# ------------------------------------------------------------------ 2. the definition's own properties
@pytest.mark.parametrize("name", ["small", "cloud", "coincident", "tangent"])
def test_prefix_layer0_and_within(name):
    sc, probes, ignore, _ = probe_set(name)
    for flags in (nc.KINDS, nc.SPHERES | nc.OPAQUE):
        hits, within, full = host(probes, ignore, flags, sc)
        for K in range(1, nc.KMAX):
            part = api.near_surfaces_host(probes, flags, K, sc.spheres, sc.planes, sc.lights, ignore)
            assert part["d"].tobytes() == full["d"][:K].tobytes() and np.array_equal(part["id"], full["id"][:K]), (name, flags, K)
        finite = np.isfinite(hits["t"]) | (hits["t"] == -np.inf)
        assert finite.any() and (~finite).any()
        assert np.array_equal(full["d"][0][finite].view(np.uint32), hits["t"][finite].view(np.uint32)) and np.array_equal(full["id"][0][finite], hits["id"][finite])
        assert (full["id"][0][~finite] == nc.ID_NONE).all()
        # within <=> a candidate exists: every hit is within; a probe that is not within has the miss record and an empty list
        assert (within[hits["id"] != nc.ID_NONE] == 1).all()
        out = within == 0
        assert (hits["id"][out] == nc.ID_NONE).all() and np.isposinf(hits["t"][out]).all() and (full["id"][:, out] == nc.ID_NONE).all()
        # ... and a candidate at d = +inf raises within but keeps the miss record
        far = api.make_probes([(np.inf, 0, 0)], np.inf)
        assert api.within_reach_host(far, flags, sc.spheres, sc.planes, sc.lights).tolist() == [1]
        assert api.nearest_surface_host(far, flags, sc.spheres, sc.planes, sc.lights)["id"].tolist() == [nc.ID_NONE]
        # every primitive at most once, keys ascending
        d, ids = full["d"], full["id"]
        assert ((d[1:] > d[:-1]) | ((d[1:] == d[:-1]) & (ids[1:] > ids[:-1])) | (ids[1:] == nc.ID_NONE)).all()


# ------------------------------------------------------------------ 3. closed forms
def test_closed_forms_with_dyadic_values():
    sc = cc.scene_of("small")
    floor = sc.planes[:1]                                                       # y = 0, normal +y
    h = api.nearest_surface_host(api.make_probes([(3, 5, -2), (3, -5, -2)]), nc.PLANES, None, floor, None)
    assert h["t"].tolist() == [5, 5] and (h["id"] == nc.KIND_PLANE).all()      # the two-sided sheet
    assert h["point"].tolist() == [[3, 0, -2]] * 2 and h["normal"].tolist() == [[0, 1, 0]] * 2      # the stored normal, never flipped
    ball = sc.spheres[:1].copy()
    ball["origin"], ball["radius"] = (0, 0, 4), 1.0
    pr = api.make_probes([(0, 0, 0), (0, 0, 3.5), (0, 0, 4)], [3.0, np.inf, np.inf])
    h = api.nearest_surface_host(pr, nc.SPHERES, ball, None, None)
    assert h["t"].tolist() == [3, -0.5, -1] and (h["id"] == 0).all()
    assert h["normal"][:2].tolist() == [[0, 0, -1]] * 2 and h["point"][:2].tolist() == [[0, 0, 3]] * 2
    assert np.isnan(h["normal"][2]).all() and np.isnan(h["point"][2]).all()     # at the centre: 0 / 0, stored as computed
    # d <= reach: reach 3 exactly reaches it, the float below does not; a negative reach asks for that deep a penetration
    pr = api.make_probes([(0, 0, 0), (0, 0, 0), (0, 0, 3.5), (0, 0, 3.5), (0, 0, 3.5)], [3.0, np.nextafter(F(3), F(0)), -0.5, -0.25, -0.75])
    assert api.within_reach_host(pr, nc.SPHERES, ball, None, None).tolist() == [1, 0, 1, 1, 0]
    # a NaN anywhere meets nothing; ignore skips the one primitive
    pr = api.make_probes([(np.nan, 0, 0), (0, 0, 0), (0, 0, 0)], [np.inf, np.nan, np.inf])
    assert api.within_reach_host(pr, nc.KINDS, ball, floor, sc.lights, ignore=[nc.ID_NONE, nc.ID_NONE, nc.KIND_PLANE]).tolist() == [0, 0, 1]
    assert api.nearest_surface_host(pr[2:], nc.SPHERES | nc.PLANES, ball, floor, None, ignore=nc.KIND_PLANE)["id"].tolist() == [0]
    assert api.nearest_surface_host(pr[2:], nc.SPHERES | nc.PLANES, ball, floor, None)["id"].tolist() == [nc.KIND_PLANE]      # d = 0 < 3


@pytest.mark.parametrize("name", ["small", "cloud", "giants"])
def test_distances_against_float64(name):
    """|d - d64| <= 8 * 2^-24 * (|p - c| + r) for a sphere or light, and the same bound on |p - p0| * |n| for a plane, d64 the same expressions
    in float64 on the float32 inputs.  Derived: p - c is rounded per component (relative 2^-24 of each), the three products and the two sums of
    v.v add at most 2.5 more on the way through the root, the root one: at most four roundings of relative size 2^-24 act on m; r =
    sqrtf(fl(r * r)) carries two halves and one, the difference one of its own -- about 6.5 in all, 8 with slack.  The plane: three differences,
    three products and two sums, each at most 2^-24 of |p - p0| |n|."""
    sc, probes, ignore, _ = probe_set(name)
    u = 2.0 ** -24
    lists = api.near_surfaces_host(probes, nc.KINDS, nc.KMAX, sc.spheres, sc.planes, sc.lights, None)
    d, ids = lists["d"].astype(np.float64), lists["id"]
    p = probes["point"].astype(np.float64)
    checked = 0
    for j in range(nc.KMAX):
        ok = np.isfinite(d[j]) & (ids[j] != nc.ID_NONE)
        kind, index = ids[j] >> np.uint32(30), (ids[j] & np.uint32(0x3FFFFFFF)).astype(np.int64)
        for k in np.flatnonzero(ok):
            i = index[k]
            if kind[k] == 1:
                nn, p0 = sc.planes["normal"][i].astype(np.float64), sc.planes["point_in_plane"][i].astype(np.float64)
                d64, scale = abs(np.dot(p[k] - p0, nn)), np.linalg.norm(p[k] - p0) * np.linalg.norm(nn)
            else:
                rec = sc.spheres[i] if kind[k] == 0 else sc.lights[i]
                c, r = rec["origin"].astype(np.float64), abs(float(rec["radius"]))
                m = np.linalg.norm(p[k] - c)
                if m == 0:
                    continue                                                    # at a centre
                d64, scale = m - r, m + r
            assert abs(d[j][k] - d64) <= 8 * u * scale, (name, j, k, d[j][k], d64, scale)
            checked += 1
    assert checked > 1000


# ------------------------------------------------------------------ 4. refusals: 0, nothing written
def test_every_refusal():
    L = api.load_library()
    sc = cc.scene_of("small")
    probes = np.ascontiguousarray(nc.make_probes(sc, 12, 1)[0])
    ign = np.full(12, nc.ID_NONE, np.uint32)
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(which, probes=probes, ignore=ign, n=12, flags=3, sp=sc.spheres, ns=4, pl=sc.planes, npl=2, li=sc.lights, nl=3, out=True, K=4, out2=True):
        o = np.full(12 * 32, 0xA5, np.uint8)
        o2 = np.full(12 * 32, 0xA5, np.uint8)
        head = (P(probes), P(ignore), n, flags, P(sp), ns, P(pl), npl, P(li), nl)
        if which == "nearest":
            r = L.clw_host_nearest_surface(*head, P(o) if out else None)
        elif which == "within":
            r = L.clw_host_within_reach(*head, P(o) if out else None)
        else:
            r = L.clw_host_near_surfaces(*head, K, P(o) if out else None, P(o2) if out2 else None)
        assert ((o == 0xA5).all() and (o2 == 0xA5).all()) or r == 1
        return r

    for which in ("nearest", "within", "list"):
        assert call(which) == 1 and call(which, flags=15) == 1 and call(which, n=1) == 1 and call(which, ignore=None) == 1
        assert call(which, sp=None, ns=0) == 1 and call(which, pl=None, npl=0) == 1 and call(which, li=None, nl=0) == 1
        for kw in (dict(probes=None), dict(out=False), dict(sp=None), dict(pl=None), dict(li=None), dict(n=0), dict(n=1 << 30), dict(n=0xFFFFFFFF),
                   dict(flags=0), dict(flags=8), dict(flags=16 | 3), dict(flags=0x80000001)):
            assert call(which, **kw) == 0, (which, kw)
    assert call("list", K=1) == 1 and call("list", K=8) == 1
    for kw in (dict(K=0), dict(K=9), dict(K=0xFFFFFFFF), dict(out2=False)):
        assert call("list", **kw) == 0, kw
    with pytest.raises(ValueError):
        api.nearest_surface_host(probes, 0, sc.spheres, sc.planes, sc.lights)
    with pytest.raises(ValueError):
        api.within_reach_host(probes[:0], 3, sc.spheres, sc.planes, sc.lights)
    with pytest.raises(ValueError):
        api.near_surfaces_host(probes, 3, 9, sc.spheres, sc.planes, sc.lights)


# ------------------------------------------------------------------ 5. the plan: which instantiation runs
class wt_near_class(C.Structure):
    _fields_ = [("flags", C.c_int32), ("dyn_lds", C.c_uint32), ("groups", C.c_uint32), ("box_cells", C.c_uint32)]


WT_F_GEOM_LDS, WT_F_GRID = 4, 16                      # csrc/whitted_params.h
WT_V_GEOM_GLOBAL, WT_V_NO_GRID = 1, 8                 # csrc/launch_plan.h
WT_NEAR_BOX_CELLS = 512                               # csrc/launch_plan.h


def plan_near(variant, ns, geom_f4, grid_usable, n, box_cells_req=-1):
    L = api.load_library()
    L.wt_plan_near.restype = wt_near_class
    L.wt_plan_near.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_int32]
    c = L.wt_plan_near(variant, ns, geom_f4, grid_usable, n, box_cells_req)
    return c.flags, c.dyn_lds, c.groups, c.box_cells


def test_the_plan_picks_lds_global_or_grid():
    small = 4 + 2 * 2 + 2 * 3 + 2                     # the small scene's float4s: spheres, planes, lights, the side table
    assert plan_near(0, 4, small, 0, 4099) == (WT_F_GEOM_LDS, small * 16, 65, WT_NEAR_BOX_CELLS)
    assert plan_near(WT_V_GEOM_GLOBAL, 4, small, 0, 4099) == (0, 0, 65, WT_NEAR_BOX_CELLS)
    big = 257 + 2 + 6 + 1
    assert plan_near(0, 257, big, 1, 193) == (WT_F_GRID, 0, 4, WT_NEAR_BOX_CELLS)
    assert plan_near(WT_V_NO_GRID, 257, big, 1, 193)[:3] == (0, 0, 4)              # grid built, switched off by the variant
    assert plan_near(0, 257, big, 0, 193)[:3] == (0, 0, 4)                         # ... or not usable (no grid, or an r * r that is not finite)
    assert plan_near(0, 200, 1024, 0, 64)[:2] == (WT_F_GEOM_LDS, 16384) and plan_near(0, 200, 1025, 0, 64)[:2] == (0, 0)
    for n in (1, 63, 64, 65, 193, 4099, (1 << 30) - 1):                             # one wave per 64 probes, the last one ragged
        assert plan_near(0, 4, small, 0, n)[2] == -(-n // 64)
    assert plan_near(0, 4, small, 0, 0)[2] == 0 and plan_near(0, 4, small, 0, 1 << 30)[2] == 0
    for req, want in ((0, 0), (1, 1), (7, 7), (1 << 30, 1 << 30), (-1, WT_NEAR_BOX_CELLS), (-5, WT_NEAR_BOX_CELLS)):
        assert plan_near(0, 257, big, 1, 193, req)[3] == want


# ------------------------------------------------------------------ 6. the lattice, exactly
def test_touching_spheres_of_the_lattice():
    sc = nc.lattice_scene()
    probes, ignore, r = nc.touching_probes(sc, 0.0)
    got = api.near_surfaces_host(probes, nc.SPHERES, 8, sc.spheres, None, None, ignore)
    ids, gap = got["id"], got["d"] - r[None, :]
    counts = set()
    for i in range(len(sc.spheres)):
        want = nc.lattice_neighbours(i)
        counts.add(len(want))
        assert ids[:len(want), i].tolist() == want and (gap[:len(want), i] == 0).all(), i
        assert (ids[len(want):, i] == nc.ID_NONE).all() and np.isposinf(gap[len(want):, i]).all(), i
    assert counts == {3, 4, 5, 6}                      # corners, edges, faces, the interior
    model = nc.near_model(probes, ignore, nc.SPHERES, sc.spheres, None, None)
    assert got["d"].tobytes() == model[2].tobytes() and np.array_equal(ids, model[3])
    # a hair of margin changes nothing; half a diagonal's gap adds the 12 edge-diagonal neighbours: an interior sphere then fills K = 8
    probes, ignore, r = nc.touching_probes(sc, 0.5)
    more = api.near_surfaces_host(probes, nc.SPHERES, 8, sc.spheres, None, None, ignore)
    assert (more["id"][7] != nc.ID_NONE).any()
