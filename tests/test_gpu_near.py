"""Proximity queries on the GPU (include/hip_wrap_ext.h: clw_ext_nearest_surface, clw_ext_within_reach, clw_ext_near_surfaces,
clw_ext_probe_device, clw_ext_near_surfaces_device; csrc/whitted_near.inc) against the host definition (csrc/near_host.c) -- bit for bit, in both
builds, no tolerance anywhere.  The scenes reach each geometry source of wt_near (staged in LDS, read from global memory, the boxes of the
uniform grid); the probe sets are those of tests/near_common.py."""
import numpy as np
import pytest

import cast_common as cc
import grid_common as gridc
import near_common as nc
from render_common import R, api, released, rendering  # noqa: F401  (R, api: the fixtures)

pytestmark = pytest.mark.gpu

WT_V_GEOM_GLOBAL = 1                     # csrc/launch_plan.h: geometry read from global memory although it would fit LDS
SIZES = (1, 63, 64, 65, 193, 4099)      # one lane, a ragged wave, a whole one, one and a lane, several workgroups, many with a ragged tail
LIST_KS = (3, 8)                         # a list of the capacity-4 kernel that is not full to capacity, and the capacity-8 kernel's largest
S, P, L, O = nc.SPHERES, nc.PLANES, nc.LIGHTS, nc.OPAQUE
FLAG_SETS = {"planes": (P, P | L), "spheres": (S | O, S | L), "small": (S | P, S | P | L | O), "ns257": (S | P, S | P | L), "cloud": (S | P | O, S | P | L),
             "tangent": (S | O, S | P | L)}
FLAG_SETS.update({name: (S | P, S | P | L | O) for name in cc.GRID_SCENES})
# name -> (setup of the wrapper, the geometry the pass must take: "lds" | "global" | "grid")
UNIT_SCENES = {"planes": (None, "lds"), "spheres": (None, "lds"), "small": (None, "lds"), "small-global": (lambda w: w.set_variant(WT_V_GEOM_GLOBAL), "global")}
for _name in ("ns257", "cloud") + cc.GRID_SCENES + ("tangent",):      # each through its boxes and scanned: grid == linear == the definition
    UNIT_SCENES.update({_name + "-grid": (None, "grid"), _name + "-linear": (lambda w: w.set_grid(0), "global")})
_expected = {}


@pytest.fixture(scope="module", params=[True, False], ids=["strict", "fast"])
def strict(request):
    import torch  # noqa: F401
    return request.param


def api_mod():
    from example_gui_opencl_raytracer_amd import api as a
    return a


def expected(name):
    """[(n, flags, probes, ignore, hits, within, {K: lists}) ...] of one scene: the host definition, computed once, shared by both builds and
    by the scene's grid and linear flavours, never written to; the largest set over every kind decides something (near_common.assert_decides)"""
    base = name.split("-")[0]
    if base not in _expected:
        a, sc, rows = api_mod(), cc.scene_of(base), []
        for n in SIZES:
            probes, ignore, info = nc.make_probes(sc, n, seed=n)
            if n == SIZES[-1]:
                every = (a.nearest_surface_host(probes, nc.KINDS, sc.spheres, sc.planes, sc.lights, ignore),
                         a.within_reach_host(probes, nc.KINDS, sc.spheres, sc.planes, sc.lights, ignore),
                         a.near_surfaces_host(probes, nc.KINDS, 4, sc.spheres, sc.planes, sc.lights, ignore)["d"])
                s = nc.assert_decides(probes, every[0], every[1], every[2], 4, base)
                assert s["negative"] == bool(len(sc.spheres)) and len(info["odd"]) and len(info["edge_at"]) and len(info["ignoring"])
                assert (len(info["faces"]) > 0) == (len(sc.spheres) > gridc.GRID_MIN_SPHERES) and not np.isfinite(probes["reach"]).all()
            for flags in FLAG_SETS[base]:
                hits = a.nearest_surface_host(probes, flags, sc.spheres, sc.planes, sc.lights, ignore)
                within = a.within_reach_host(probes, flags, sc.spheres, sc.planes, sc.lights, ignore)
                lists = {K: a.near_surfaces_host(probes, flags, K, sc.spheres, sc.planes, sc.lights, ignore) for K in LIST_KS}
                for arr in [hits, within] + [v for l in lists.values() for v in l.values()]:
                    arr.setflags(write=False)
                rows.append((n, flags, probes, ignore, hits, within, lists))
        _expected[base] = rows
    return _expected[base]


def differing(got, want):
    return int((np.ascontiguousarray(got).reshape(-1).view(np.uint8) != np.ascontiguousarray(want).reshape(-1).view(np.uint8)).sum())


def run_case(w, case):
    """all three queries of one expected case on the wrapper -> the differing bytes of (hits, within, the lists' d and id per K ...)"""
    n, flags, probes, ignore, hits, within, lists = case
    got, got_within = w.nearest_surface(probes, flags, ignore), w.within_reach(probes, flags, ignore)
    assert got is not None and got.shape == hits.shape and got.dtype == api_mod().HIT
    assert got_within is not None and got_within.shape == within.shape and got_within.dtype == np.uint8
    d = [differing(got, hits), differing(got_within, within)]
    for K, want in lists.items():
        g = w.near_surfaces(probes, flags, K, ignore)
        assert g is not None and g["d"].shape == (K, n) and g["id"].shape == (K, n)
        d += [differing(g["d"], want["d"]), differing(g["id"], want["id"])]
        listed = np.sort(np.where(g["id"] == nc.ID_NONE, np.arange(K, dtype=np.uint32)[:, None] | np.uint32(0xC0000000), g["id"]), 0)
        assert not (listed[1:] == listed[:-1]).any()                      # a primitive appears once in a list
    return d


def took_geometry(name, sc, grid):
    """the geometry the pass took: the grid when one is built and on, LDS for a small scene unless the variant says global"""
    if grid and grid["built"] and "linear" not in name:
        return "grid"
    return "lds" if len(sc.spheres) <= gridc.GRID_MIN_SPHERES and "global" not in name else "global"


# ------------------------------------------------------------------ 1. against the definition
@pytest.mark.parametrize("name", list(UNIT_SCENES))
def test_probes_equal_the_definition(R, api, tex, sky, strict, name):
    sc, (setup, geometry) = cc.scene_of(name.split("-")[0]), UNIT_SCENES[name]
    bad = []
    with rendering(R, sc, tex, sky, 8, 8, setup=setup, cam=None, strict=strict) as r:
        for case in expected(name):
            d = run_case(r.w, case)
            if any(d):
                bad.append(case[:2] + tuple(d))
        grid = r.w.get_grid()
        assert bool(grid and grid["built"]) == (len(sc.spheres) > gridc.GRID_MIN_SPHERES)
        assert took_geometry(name, sc, grid) == geometry
    print(f"{name} {'strict' if strict else 'fast'}: {len(expected(name))} cases x nearest, within and K in {LIST_KS}, differing bytes "
          f"{sum(sum(b[2:]) for b in bad)} {bad[:8]}")
    assert not bad


# ------------------------------------------------------------------ 2. both sides of the box-cell cap
@pytest.mark.parametrize("cap", [0, 1, 1 << 30])
@pytest.mark.parametrize("name", ["cloud-grid", "coincident-grid", "tangent-grid"])
def test_the_cap_does_not_change_the_answer(R, api, tex, sky, strict, monkeypatch, name, cap):
    """CLWRAP_NEAR_BOX_CELLS (read on every call): 0 sends every probe of finite reach to the in-order scan, 1 those whose box is more than one
    cell, a huge value none -- the same bytes each time.  The coincident and the tangent scene hold equal keys met from several cells."""
    monkeypatch.setenv("CLWRAP_NEAR_BOX_CELLS", str(cap))
    sc = cc.scene_of(name.split("-")[0])
    bad = []
    with rendering(R, sc, tex, sky, 8, 8, cam=None, strict=strict) as r:
        for case in expected(name):
            if case[0] in (65, 193, 4099):
                d = run_case(r.w, case)
                if any(d):
                    bad.append(case[:2] + tuple(d))
        grid = r.w.get_grid()
        assert grid and grid["built"]
    print(f"{name} {'strict' if strict else 'fast'} cap {cap}: differing bytes {bad[:8]}")
    assert not bad


def test_equal_keys_from_several_cells(R, api, tex, sky, strict):
    """the tangent pair: the small sphere A touches the large B from inside at the origin, so a probe there is equally far from both (d = 0,
    exactly) -- the lower index wins the nearest query and the list holds both once, in index order, whichever cell presents which first"""
    name = "tangent"
    sc = cc.scene_of(name)
    a, b = cc.tangent_ids(name)
    probes = api.make_probes(np.float32([(0.0, 0.0, 0.0)] * 3), [np.inf, 0.0, 0.25])      # the point of contact: |A's centre| = 1.25, |B's| = 10, exactly
    want = api.nearest_surface_host(probes, S, sc.spheres, sc.planes, sc.lights)
    lists = api.near_surfaces_host(probes, S, 4, sc.spheres, sc.planes, sc.lights)
    assert want["id"].tolist() == [min(a, b)] * 3 and (want["t"] == 0).all()
    assert lists["id"][:2, 0].tolist() == sorted((a, b)) and (lists["d"][:2, 0] == 0).all()
    for setup in (None, lambda w: w.set_grid(0)):
        with rendering(R, sc, tex, sky, 8, 8, setup=setup, cam=None, strict=strict) as r:
            assert r.w.nearest_surface(probes, S).tobytes() == want.tobytes()
            got = r.w.near_surfaces(probes, S, 4)
            assert got["d"].tobytes() == lists["d"].tobytes() and np.array_equal(got["id"], lists["id"])


# ------------------------------------------------------------------ 3. the device path
@pytest.mark.parametrize("name", ["small", "cloud-grid"])
def test_device_path_equals_the_host_array_calls(R, api, tex, sky, strict, name):
    import torch
    sc = cc.scene_of(name.split("-")[0])
    n, flags, probes, ignore, hits, within, lists = [e for e in expected(name) if e[0] == 4099][1]
    K = 8
    with rendering(R, sc, tex, sky, 8, 8, cam=None, strict=strict) as r:
        d_probes = torch.from_numpy(np.frombuffer(probes.tobytes(), np.float32).reshape(n, 4).copy()).cuda()
        d_ignore = torch.from_numpy(ignore.view(np.int32).copy()).cuda()
        kinds, opaque = flags & nc.KINDS, bool(flags & O)
        for own_stream in (True, False):
            d_hits = torch.full((n, 8), float("nan"), dtype=torch.float32, device="cuda")
            d_within = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
            d_d = torch.full((K, n), float("nan"), dtype=torch.float32, device="cuda")
            d_id = torch.full((K, n), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def launch():
                assert r.probe_device(d_probes, n, hits=d_hits, ignore=d_ignore, kinds=kinds, opaque_only=opaque) == n
                assert r.w.probe_device(d_probes.data_ptr(), n, flags, d_ignore.data_ptr(), within_ptr=d_within.data_ptr()) == n
                assert r.near_surfaces_device(d_probes, n, K, d_d, d_id, ignore=d_ignore, kinds=kinds, opaque_only=opaque) == n
            if own_stream:                                     # the wrapper's stream
                launch()
                r.w.sync()
            else:                                              # torch's current stream, after set_stream
                stream = torch.cuda.Stream()
                with torch.cuda.stream(stream):
                    r.w.set_stream(torch.cuda.current_stream().cuda_stream)
                    launch()
                    early = d_hits.cpu()                       # (ordered behind the launches on that stream)
                stream.synchronize()
                assert early.numpy().tobytes() == hits.tobytes()
            torch.cuda.synchronize()
            got = (d_hits.cpu().numpy(), d_within.cpu().numpy(), d_d.cpu().numpy(), d_id.cpu().numpy().view(np.uint32))
            d = (differing(got[0], hits), differing(got[1], within), differing(got[2], lists[K]["d"]), differing(got[3], lists[K]["id"]))
            print(f"{name} {'strict' if strict else 'fast'} {'wrapper stream' if own_stream else 'torch stream'}: differing bytes {d}")
            assert not any(d)
        r.w.set_stream(0)
        # without ignore words: the same as ignoring nothing
        d_within = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert r.probe_device(d_probes, n, within=d_within, kinds=kinds, opaque_only=opaque) == n
        r.w.sync()
        assert np.array_equal(d_within.cpu().numpy(), api.within_reach_host(probes, flags, sc.spheres, sc.planes, sc.lights))
        # refusals: both or neither output, no probes, K out of range -- 0, nothing written
        assert r.w.probe_device(d_probes.data_ptr(), n, flags) == 0
        assert r.w.probe_device(d_probes.data_ptr(), n, flags, None, d_hits.data_ptr(), d_within.data_ptr()) == 0
        assert r.w.probe_device(0, n, flags, None, d_hits.data_ptr()) == 0 and r.w.probe_device(d_probes.data_ptr(), n, 16 | 3, None, d_hits.data_ptr()) == 0
        assert r.w.near_surfaces_device(d_probes.data_ptr(), n, flags, 9, d_d.data_ptr(), d_id.data_ptr()) == 0
        assert r.w.near_surfaces_device(d_probes.data_ptr(), n, flags, 0, d_d.data_ptr(), d_id.data_ptr()) == 0
        assert r.w.near_surfaces(probes, flags, 9) is None and r.w.nearest_surface(probes, 0) is None and r.w.within_reach(probes[:0], flags) is None
    with released(api.ClWrap()) as w:                          # no scene bound
        assert w.nearest_surface(probes, flags) is None and w.within_reach(probes, flags) is None and w.near_surfaces(probes, flags, 4) is None


# ------------------------------------------------------------------ 4. a rewritten scene, and nothing else moves
def test_a_rewritten_scene_is_seen_after_invalidate(api, strict):
    import torch
    from test_gpu_cast import bare_scene_wrapper
    sc = cc.scene_of("ns257")
    n, flags, probes, ignore, hits, within, lists = [e for e in expected("ns257") if e[0] == 193][0]
    sph = torch.from_numpy(np.frombuffer(sc.spheres.tobytes(), np.uint8).copy()).cuda()
    with released(bare_scene_wrapper(api, sc, sph)) as cw:
        cw.set_strict(strict)
        assert cw.nearest_surface(probes, flags, ignore).tobytes() == hits.tobytes()
        moved = sc.spheres.copy()
        victim = int(np.bincount(hits["id"][hits["id"] >> 30 == 0]).argmax())            # the sphere most probes are nearest to
        moved["origin"][victim] += np.float32([0.75, 0.5, -0.25])
        sph.copy_(torch.from_numpy(np.frombuffer(moved.tobytes(), np.uint8).copy()))
        torch.cuda.synchronize()
        cw.invalidate_scene()
        want = api.nearest_surface_host(probes, flags, moved, sc.planes, sc.lights, ignore)
        got = cw.nearest_surface(probes, flags, ignore)
        assert (want["id"] != hits["id"]).any() or (want["t"] != hits["t"]).any()
        assert got.tobytes() == want.tobytes()
        assert np.array_equal(cw.within_reach(probes, flags, ignore), api.within_reach_host(probes, flags, moved, sc.planes, sc.lights, ignore))


def test_a_probe_leaves_everything_else_alone(R, api, demo_scene, tex, sky, strict):
    from test_gpu_cast import read_framebuffer
    W = H = 16
    probes, ignore, _ = nc.make_probes(demo_scene, 193, 5)
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict, accumulate=4) as r:
        first = r.render()
        g = r.gbuffer(api.GB_ID)
        flags_before = r.w.last_trace_flags()
        r.w.timing_reset()
        hits = r.nearest_surface(probes["point"], probes["reach"], ignore, kinds=("sphere", "plane", "light"))
        assert hits.tobytes() == api.nearest_surface_host(probes, nc.KINDS, demo_scene.spheres, demo_scene.planes, demo_scene.lights, ignore).tobytes()
        assert r.within_reach(probes["point"], probes["reach"]).dtype == bool
        assert r.near_surfaces(probes["point"], 4, probes["reach"])["id"].shape == (4, 193)
        assert r.w.timing_get(api.TIMING_NEAR)[0] == 3 and r.w.timing_get(api.TIMING_CAST)[0] == 0
        assert np.array_equal(r.w.read_gbuffer(api.GB_ID), g["id"])
        assert r.w.last_trace_flags() == flags_before and r.accumulated == 1
        assert np.array_equal(read_framebuffer(r), first)                    # the framebuffer rendered before the probes: byte-equal after
        with pytest.raises(RuntimeError):
            r.nearest_surface(probes["point"], kinds=())
        with pytest.raises(RuntimeError):
            r.near_surfaces(probes["point"], 9)


# ------------------------------------------------------------------ 5. Renderer.touching_spheres on the lattice
def test_touching_spheres_of_the_lattice(R, api, tex, sky, strict):
    sc = nc.lattice_scene()
    for setup in (None, lambda w: w.set_grid(0)):
        with rendering(R, sc, tex, sky, 8, 8, setup=setup, cam=None, strict=strict) as r:
            ids, gap = r.touching_spheres(0.0)
            grid = r.w.get_grid()
            assert bool(grid and grid["built"])
        assert ids.shape == gap.shape == (8, len(sc.spheres)) and gap.dtype == np.float32
        for i in range(len(sc.spheres)):
            want = nc.lattice_neighbours(i)
            assert ids[:len(want), i].tolist() == want and (gap[:len(want), i] == 0).all(), i
            assert (ids[len(want):, i] == nc.ID_NONE).all() and np.isposinf(gap[len(want):, i]).all(), i
