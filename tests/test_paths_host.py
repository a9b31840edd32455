"""The path queries on the CPU (include/hip_wrap_ext.h: clw_host_cast_paths; csrc/paths_host.c): the C ABI against the header and the ctypes
mirror, every refusal, the status byte and `next`, every segment against clw_host_cast_rays of the ray before it, the paths against the ORACLE
(oracle/whitted_oracle.c: wo_find_solid, wo_reflect, wo_refract) -- bit for bit, no tolerance anywhere --, the census of what the rays decide,
and the sanitizer build of the definition on the census rays (tools/paths_sanitize.c, a child process)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cast_common as cc
import paths_common as pc
from conftest import ROOT
from example_gui_opencl_raytracer_amd import api
from render_common import header_text

F = np.float32
NEW_SYMBOLS = ["clw_host_cast_paths", "clw_ext_cast_paths", "clw_ext_cast_paths_device", "clw_ext_pick_path"]
SEED = 7
B_SET = (1, 2, 8)
ORACLE_SCENES = ("hall", "demo")


def hits_bytes(h):
    return np.frombuffer(np.ascontiguousarray(h).tobytes(), np.uint8)


# ------------------------------------------------------------------ 1. header, library and mirror
def test_header_library_and_mirror_agree():
    code = header_text(comments=False)
    L = api.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), f"hip_wrap_ext.h does not declare {name}"
        assert name in api.SYMBOLS and hasattr(L, name), f"the library does not export {name}"
        assert getattr(L, name).argtypes is not None
    assert L.clw_host_cast_paths.restype is C.c_int and L.clw_ext_pick_path.restype is C.c_int
    assert L.clw_ext_cast_paths.restype is C.c_uint32 and L.clw_ext_cast_paths_device.restype is C.c_uint32
    defs = dict(re.findall(r"#define\s+(CLW_\w+)\s+(0x[0-9A-Fa-f]+|\d+)u\b", header_text()))
    assert int(defs["CLW_PATH_TRANSMIT"]) == api.PATH_TRANSMIT == pc.TRANSMIT == 16
    assert int(defs["CLW_PATH_ALL_SURFACES"]) == api.PATH_ALL_SURFACES == pc.ALL_SURFACES == 32
    assert int(defs["CLW_PATH_MAX_BOUNCES"]) == api.PATH_MAX_BOUNCES == pc.B_MAX == 8
    assert (int(defs["CLW_PATH_REASON_BOUNCES"]), int(defs["CLW_PATH_REASON_MISSED"]), int(defs["CLW_PATH_REASON_ENDED"])) == (0, 1, 2) \
        == (api.PATH_REASON_BOUNCES, api.PATH_REASON_MISSED, api.PATH_REASON_ENDED) == (pc.BOUNCES, pc.MISSED, pc.ENDED)
    assert int(defs["CLW_TIMING_PATHS"], 0) == api.TIMING_PATHS == 0x50415448
    # the new flags sit beside the ray queries', which keep their values
    assert (int(defs["CLW_CAST_SPHERES"]), int(defs["CLW_CAST_PLANES"]), int(defs["CLW_CAST_LIGHTS"]), int(defs["CLW_CAST_OPAQUE"])) == (1, 2, 4, 8)
    assert api.PATH_TRANSMIT & 15 == 0 and api.PATH_ALL_SURFACES & (15 | api.PATH_TRANSMIT) == 0
    assert api.RAY_QUERY.itemsize == api.HIT.itemsize == 32 and api.PATH_EPSILON == pc.EPSILON == F(0.001)
    text = header_text()
    for word in ("count | reason << 4", "hits[k * n + i]", "CLW_PATH_COUNT(status)  ((status) & 15u)", "CLW_PATH_REASON(status) ((status) >> 4)",
                 "refract assumes a UNIT direction", "per-ray flags", "total path length", "Schlick-weighted branching", "total internal"):
        assert word in text, word
    from example_gui_opencl_raytracer_amd.renderer import Renderer
    for name in ("cast_paths", "cast_paths_device", "pick_path"):
        assert callable(getattr(Renderer, name)) and callable(getattr(api.ClWrap, name))
    assert api.path_flags() == 7 and api.path_flags(("sphere",), True, True, True) == 1 | 8 | 16 | 32


# ------------------------------------------------------------------ 2. refusals: 0, nothing written
def test_every_refusal():
    L = api.load_library()
    sc = pc.scene_of("hall")
    rays = np.ascontiguousarray(pc.unit_rays(sc, 12, 1))
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    ns, npl, nl = len(sc.spheres), len(sc.planes), len(sc.lights)

    def call(rays=rays, n=12, flags=7, B=3, sp=sc.spheres, ns=ns, pl=sc.planes, npl=npl, li=sc.lights, nl=nl, hits=True, status=True, nxt=True):
        oh, os_, on = np.full(12 * 8 * 32, 0xA5, np.uint8), np.full(12, 0xA5, np.uint8), np.full(12 * 32, 0xA5, np.uint8)
        r = L.clw_host_cast_paths(P(rays), n, flags, B, P(sp), ns, P(pl), npl, P(li), nl, P(oh) if hits else None, P(os_) if status else None,
                                  P(on) if nxt else None)
        assert r == 1 or ((oh == 0xA5).all() and (os_ == 0xA5).all() and (on == 0xA5).all())
        if r == 1:                                                  # exactly B * n hits, n bytes and n rays are written
            assert (oh[32 * B * n:] == 0xA5).all() and (os_[n:] == 0xA5).all() and (on[32 * n:] == 0xA5).all() and (os_[:n] != 0xA5).all()
            assert (on == 0xA5).all() if not nxt else (on[:32 * n] != 0xA5).any()
        return r

    assert call() == 1 and call(flags=63) == 1 and call(n=1) == 1 and call(B=1) == 1 and call(B=8) == 1 and call(nxt=False) == 1
    assert call(flags=1 | 16) == 1 and call(flags=2 | 32) == 1 and call(flags=4) == 1
    assert call(sp=None, ns=0) == 1 and call(pl=None, npl=0) == 1 and call(li=None, nl=0) == 1
    for kw in (dict(rays=None), dict(hits=False), dict(status=False), dict(sp=None), dict(pl=None), dict(li=None), dict(n=0), dict(n=1 << 30),
               dict(n=0xFFFFFFFF), dict(flags=0), dict(flags=8), dict(flags=16), dict(flags=32), dict(flags=8 | 16 | 32), dict(flags=64 | 7),
               dict(flags=0x80000007), dict(B=0), dict(B=9), dict(B=0xFFFFFFFF)):
        assert call(**kw) == 0, kw
    for B in (0, 9):
        with pytest.raises(ValueError):
            api.cast_paths_host(rays, 7, B, sc.spheres, sc.planes, sc.lights)
    for flags in (0, 16, 64 | 7):
        with pytest.raises(ValueError):
            api.cast_paths_host(rays, flags, 2, sc.spheres, sc.planes, sc.lights)
    with pytest.raises(ValueError):
        api.cast_paths_host(rays[:0], 7, 2, sc.spheres, sc.planes, sc.lights)


# ------------------------------------------------------------------ 3. chaining: a segment is clw_host_cast_rays of the ray before it
@pytest.mark.parametrize("name", ["hall", "small", "cloud"])
def test_every_segment_is_the_nearest_hit_of_the_ray_before_it(name):
    """on cast_common's ray set -- directions that are not unit, `ignore`, tmax at and below a hit's t, zero, NaN and infinite rays --: segment
    0 is clw_host_cast_rays of the input; segment k of a path that went on is clw_host_cast_rays of `next` of the same query with k segments;
    the layers of a path that ended hold the miss record; B segments are a prefix of B + 1"""
    sc = pc.scene_of(name)
    rays = cc.with_tmax(cc.make_rays(sc, 193, SEED)[0], 3.0, per_ray=True)
    assert (rays["ignore"] != cc.ID_NONE).sum() > 10 and np.isnan(rays["origin"]).any() and (np.abs(np.linalg.norm(rays["dir"], axis=1) - 1) > 0.1).sum() > 50
    miss = np.zeros(1, api.HIT)
    miss["t"], miss["id"] = np.inf, cc.ID_NONE
    for flags in pc.FLAG_COMBOS:
        cast_flags = flags & 15
        full = api.cast_paths_host(rays, flags, pc.B_MAX, sc.spheres, sc.planes, sc.lights)
        first = api.cast_rays_host(rays, cast_flags, sc.spheres, sc.planes, sc.lights)
        assert full["hits"][0].tobytes() == first.tobytes()
        went_on = 0
        for k in range(1, pc.B_MAX + 1):
            part = api.cast_paths_host(rays, flags, k, sc.spheres, sc.planes, sc.lights)
            assert part["hits"].tobytes() == full["hits"][:k].tobytes()                       # a prefix
            assert np.array_equal(np.minimum(full["count"], k), part["count"])
            on = part["reason"] == pc.BOUNCES
            assert np.array_equal(part["next"]["tmax"][on].view(np.uint32), rays["tmax"][on].view(np.uint32)) and (part["next"]["ignore"][on] == cc.ID_NONE).all()
            if k < pc.B_MAX:
                again = api.cast_rays_host(part["next"], cast_flags, sc.spheres, sc.planes, sc.lights)
                assert again[on].tobytes() == full["hits"][k][on].tobytes()
                assert all(h.tobytes() == miss.tobytes() for h in full["hits"][k][~on])
                went_on += int(on.sum())
        assert went_on > 50, (name, flags, went_on)


# ------------------------------------------------------------------ 4. the status byte and `next`
def test_the_status_byte_and_next_for_each_reason():
    sc = pc.scene_of("hall")
    rays = pc.unit_rays(sc, pc.N_RAYS, SEED)
    for flags in (7, 7 | pc.TRANSMIT, 7 | pc.ALL_SURFACES):
        for B in B_SET:
            got = api.cast_paths_host(rays, flags, B, sc.spheres, sc.planes, sc.lights)
            status, count, reason, nxt, hits = got["status"], got["count"], got["reason"], got["next"], got["hits"]
            assert np.array_equal(status, count | reason << 4) and np.array_equal(count, status & 15) and np.array_equal(reason, status >> 4)
            assert count.max() <= B and set(reason.tolist()) <= {0, 1, 2}
            assert ((reason == pc.BOUNCES) <= (count == B)).all() and ((reason == pc.MISSED) <= (count < B)).all() and ((reason == pc.ENDED) <= (count >= 1)).all()
            assert np.array_equal((hits["id"] != cc.ID_NONE).sum(0), count) and np.array_equal(np.isfinite(hits["t"]).sum(0), count)
            for i in range(rays.size):                                                    # hits first, misses behind them
                assert (hits["id"][:count[i], i] != cc.ID_NONE).all()
            last = hits[np.maximum(count.astype(np.int64) - 1, 0), np.arange(rays.size)]
            start = last["point"] + last["normal"] * pc.EPSILON                            # where the next segment starts
            ended, missed, on = reason == pc.ENDED, reason == pc.MISSED, reason == pc.BOUNCES
            assert ended.any() and missed.any() and (on.any() or B == 8)
            # ended: a zero direction from the last hit's shading point -- a ray that meets nothing
            assert (nxt["dir"][ended] == 0).all() and nxt["origin"][ended].tobytes() == start[ended].tobytes() and (nxt["ignore"][ended] == cc.ID_NONE).all()
            assert (api.cast_rays_host(nxt[ended], 7, sc.spheres, sc.planes, sc.lights)["id"] == cc.ID_NONE).all()
            on_light = ended & (last["id"] >> 30 == 2)
            assert on_light.any() and (~on_light & ended).any() == (not flags & pc.ALL_SURFACES)
            # missed: the ray that missed; at count 0 the caller's own record
            assert nxt[missed & (count == 0)].tobytes() == rays[missed & (count == 0)].tobytes()
            assert (api.cast_rays_host(nxt[missed], flags & 15, sc.spheres, sc.planes, sc.lights)["id"] == cc.ID_NONE).all()
            later = missed & (count > 0)
            assert later.any() == (B > 1) and (np.abs(np.linalg.norm(nxt["dir"][later], axis=1) - 1) < 1e-3).all()
            # went on: the outgoing ray of the last hit, from its shading point or 2 EPSILON inside the surface
            inside = start - last["normal"] * (F(2) * pc.EPSILON)
            from_start = (nxt["origin"] == start).all(1)
            from_inside = (nxt["origin"] == inside).all(1)
            assert (from_start | from_inside)[on | later].all()
            if B < 8:                                                                     # (at B = 8 a handful of paths are still under way)
                assert from_inside[on].any() == bool(flags & pc.TRANSMIT)
            assert np.array_equal(nxt["tmax"].view(np.uint32), rays["tmax"].view(np.uint32))


# ------------------------------------------------------------------ 5. held to the oracle
def _no_ties_no_nan(rays, sc, flags):
    """the choice of rays on which the trace's and the query's tie and NaN rules cannot differ: finite rays, and the two nearest candidates
    of the ray at different t"""
    assert np.isfinite(rays["origin"]).all() and np.isfinite(rays["dir"]).all()
    two = api.cast_layers_host(rays, flags & 15, 2, sc.spheres, sc.planes, sc.lights)
    hit = two["id"][0] != cc.ID_NONE
    assert not np.isnan(two["t"]).any() and (two["t"][0][hit] < two["t"][1][hit]).all()


@pytest.mark.parametrize("name", ORACLE_SCENES)
def test_the_reflected_path_is_the_oracles_find_solid_chain(oracle, tex, sky, name):
    """spheres and planes, no transmission: per segment wo_find_solid of the current ray gives the normal, the shading point (point + normal *
    EPSILON: where the next segment starts) and the material; t is wo_intersect_* of the primitive the id names; the next direction is
    wo_reflect.  Everything the definition answers is compared with these, bit for bit."""
    from oracle.oracle_py import _Inputs
    sc = pc.scene_of(name)
    rays = pc.unit_rays(sc, pc.N_RAYS, SEED)
    flags, B = cc.SPHERES | cc.PLANES | pc.ALL_SURFACES, 5
    got = api.cast_paths_host(rays, flags, B, sc.spheres, sc.planes, sc.lights)
    inp = _Inputs(sc, tex, sky)
    lib = oracle.lib
    cur_o, cur_d = rays["origin"].copy(), rays["dir"].copy()
    alive = np.ones(rays.size, bool)
    compared = 0
    for k in range(B):
        seg_rays = api.make_rays(cur_o[alive], cur_d[alive])
        _no_ties_no_nan(seg_rays, sc, flags)
        for i in np.flatnonzero(alive):
            point, normal, mat = pc._f3((0, 0, 0)), pc._f3((0, 0, 0)), np.zeros(1, sc.spheres["material"].dtype)
            hit = lib.wo_find_solid(pc._f3(cur_o[i]), pc._f3(cur_d[i]), C.byref(inp.c), point, normal, mat.ctypes.data_as(C.c_void_p))
            h = got["hits"][k, i]
            assert bool(hit) == (h["id"] != cc.ID_NONE) == (got["count"][i] > k), (k, i)
            if not hit:
                assert got["reason"][i] == pc.MISSED and got["count"][i] == k
                alive[i] = False
                continue
            idw = int(h["id"])
            t = C.c_float(0)
            if idw >> 30 == 0:
                s = sc.spheres[idw]
                assert lib.wo_intersect_sphere(pc._f3(cur_o[i]), pc._f3(cur_d[i]), pc._f3(s["origin"]), float(s["radius"]), C.byref(t))
            else:
                p = sc.planes[idw & 0x3FFFFFFF]
                assert lib.wo_intersect_plane(pc._f3(cur_o[i]), pc._f3(cur_d[i]), pc._f3(p["normal"]), pc._f3(p["point_in_plane"]), C.byref(t))
            assert F(t.value).tobytes() == h["t"].tobytes(), (k, i)
            assert np.array(normal[:], F).tobytes() == h["normal"].tobytes(), (k, i)
            start = h["point"] + h["normal"] * pc.EPSILON
            assert np.array(point[:], F).tobytes() == start.tobytes(), (k, i)
            m = pc.material_of(sc, idw)
            assert all(mat[0][f] == m[f] for f in ("transperent", "dielectric", "n", "reflectivity", "shininess")), (k, i)
            cur_o[i], cur_d[i] = start, pc.oracle_reflect(oracle, cur_d[i], np.array(normal[:], F))
            compared += 1
    on = got["reason"] == pc.BOUNCES
    assert on.sum() >= 5 and got["next"]["origin"][on].tobytes() == cur_o[on].tobytes() and got["next"]["dir"][on].tobytes() == cur_d[on].tobytes()
    print(f"{name}: {compared} hits held to wo_find_solid, {int(on.sum())} outgoing rays to wo_reflect")
    assert compared > 300


_census = {}


@pytest.mark.parametrize("name", ORACLE_SCENES)
def test_the_paths_are_the_oracles_reflect_and_refract(oracle, name):
    """every flag combination, B = 1, 2, 8: the definition equals the chain built in Python from clw_host_cast_rays per segment and
    wo_reflect / wo_refract with the n1 / n2 rule restated from the oracle (paths_common.chain_model) -- hits, status and next, bit for bit"""
    sc = pc.scene_of(name)
    rays = pc.unit_rays(sc, pc.N_RAYS, SEED)
    _no_ties_no_nan(rays, sc, pc.SPL)
    rows = []
    for flags in pc.FLAG_COMBOS:
        for B in B_SET:
            want, events = pc.chain_model(oracle, rays, flags, B, sc)
            got = api.cast_paths_host(rays, flags, B, sc.spheres, sc.planes, sc.lights)
            assert not np.isnan(want["next"]["dir"]).any() and not np.isnan(want["hits"]["point"]).any()
            d = pc.differing(got, want)
            rows.append(pc.census(want, events, B))
            assert d == (0, 0, 0), (name, flags, B, d)
    _census[name] = rows
    total = {k: sum(r[k] for r in rows) for k in pc.CENSUS}
    print(f"{name}: census over {len(rows)} cases of {pc.N_RAYS} rays: {total}")
    if name == "hall":
        pc.assert_census(rows)
    else:                                                           # the demo scene has no matte surface: everything else happens there too
        assert total["stop_matte"] == 0 and total["all_surfaces_goes_on"] == 0 and total["tir"] == 0
        assert all(total[k] > 0 for k in pc.CENSUS if k not in ("stop_matte", "all_surfaces_goes_on", "tir"))


def test_all_surfaces_goes_on_where_the_default_stops():
    sc = pc.scene_of("hall")
    rays = pc.unit_rays(sc, pc.N_RAYS, SEED)
    stop = api.cast_paths_host(rays, 7, 4, sc.spheres, sc.planes, sc.lights)
    goes = api.cast_paths_host(rays, 7 | pc.ALL_SURFACES, 4, sc.spheres, sc.planes, sc.lights)
    last = stop["hits"][np.maximum(stop["count"].astype(np.int64) - 1, 0), np.arange(rays.size)]
    matte = (stop["reason"] == pc.ENDED) & (last["id"] >> 30 != 2)
    assert matte.sum() > 20 and (goes["count"][matte] >= stop["count"][matte]).all() and (goes["count"][matte] > stop["count"][matte]).any()
    assert not ((goes["reason"] == pc.ENDED) & (goes["hits"][np.maximum(goes["count"].astype(np.int64) - 1, 0), np.arange(rays.size)]["id"] >> 30 != 2)).any()
    same = ~matte
    assert goes["hits"][:, same].tobytes() == stop["hits"][:, same].tobytes() and np.array_equal(goes["status"][same], stop["status"][same])


# ------------------------------------------------------------------ 6. the definition under the sanitizers
def test_the_definition_under_the_sanitizers(tmp_path):
    """tools/paths_sanitize.c: csrc/paths_host.c built with -fsanitize=address,undefined as a stand-alone program, run once as a child process
    over the census rays of both scenes with degenerate rays behind them (host code only)"""
    cc_ = shutil.which(os.environ.get("CC") or "gcc")
    assert cc_, "no C compiler"
    files = []
    for name in ORACLE_SCENES:
        sc = pc.scene_of(name)
        odd = cc.make_rays(sc, 48, SEED)[0]
        rays = np.concatenate([pc.unit_rays(sc, pc.N_RAYS, SEED), odd])
        assert np.isnan(odd["origin"]).any() and (odd["dir"] == 0).all(1).any()
        path = str(tmp_path / (name + ".bin"))
        with open(path, "wb") as f:
            f.write(np.array([rays.size, len(sc.spheres), len(sc.planes), len(sc.lights)], "<u4").tobytes())
            for a in (rays, sc.spheres, sc.planes, sc.lights):
                f.write(np.ascontiguousarray(a).tobytes())
        files.append(path)
    csrc = os.path.join(ROOT, "example_gui_opencl_raytracer_amd", "csrc")
    exe = str(tmp_path / "paths_sanitize")
    cmd = [cc_, "-O1", "-g", "-std=c99", "-ffp-contract=off", "-D_DEFAULT_SOURCE", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I", csrc, os.path.join(ROOT, "tools", "paths_sanitize.c")] + [os.path.join(csrc, f) for f in ("paths_host.c", "cast_host.c", "scene_prep.c")] + ["-lm", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    p = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0 and "0 failures" in p.stdout
