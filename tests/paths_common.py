"""Shared by test_paths_host.py and test_gpu_paths.py: the `hall` scene of mirrors, glass and matte surfaces, the unit-direction ray sets, the
path rule (include/hip_wrap_ext.h: clw_host_cast_paths) restated in Python over the ORACLE's reflect and refract (oracle/whitted_oracle.c:
wo_reflect, wo_refract; the n1 / n2 rule from its lines 481-508) with a segment's hit taken from the ray queries' definition, and the census a
ray set has to pass before anything is compared on it.  Everything is compared for equality of bits."""
import numpy as np

import cast_common as cc
from example_gui_opencl_raytracer_amd import api
from example_gui_opencl_raytracer_amd import scene as S

F = np.float32
TRANSMIT, ALL_SURFACES = 16, 32
BOUNCES, MISSED, ENDED = 0, 1, 2
EPSILON, DEFAULT_N = F(0.001), F(1.0)                  # whitted_oracle.c:39, 73
B_MAX = 8
SPL = cc.SPHERES | cc.PLANES | cc.LIGHTS
# every combination of TRANSMIT x ALL_SURFACES x OPAQUE on top of all three kinds
FLAG_COMBOS = tuple(SPL | t | a | o for t in (0, TRANSMIT) for a in (0, ALL_SURFACES) for o in (0, cc.OPAQUE))
N_RAYS = 257
CENSUS = ("reaches_B", "miss_first", "miss_later", "stop_matte", "stop_light", "enter_glass", "leave_glass", "tir", "all_surfaces_goes_on")


def _set_material(rec, m):
    for name in ("ambient", "diffuse", "specular", "shininess", "transperent", "dielectric", "n", "reflectivity"):
        rec["material"][name] = m[name]


def matte():
    """neither reflective, dielectric nor transparent: the reference sends nothing on from it"""
    m = S.plastic()
    m["reflectivity"] = 0.0
    return m


def hall_scene():
    """6 spheres -- 0 a mirror, 1 glass, 2 matte, 3 plastic (reflectivity 0.1), 4 glass overlapping sphere 1 (a path inside 1 meets it at
    any angle: total internal reflection), 5 a small mirror --, 3 planes -- a matte floor, a mirror wall across z = 7, a stone wall across
    x = -6 --, 3 lights of radius 0.3 that paths do meet.  33 float4: staged in LDS."""
    base = S.render_map_scene()
    sp = np.repeat(base.spheres[:1], 6).copy()
    sp["origin"] = [(-2.0, 1.0, 3.0), (1.0, 1.0, 2.0), (3.5, 0.7, 3.5), (-0.5, 0.5, 0.5), (1.9, 1.2, 2.6), (0.5, 2.6, 4.0)]
    sp["radius"] = (1.0, 1.0, 0.7, 0.5, 0.6, 0.4)
    for i, m in enumerate((S.mirror(), S.glass(), matte(), S.plastic(), S.glass(), S.mirror())):
        _set_material(sp[i:i + 1], m)
    pl = np.repeat(base.planes[1:2], 3).copy()
    pl["normal"] = [(0.0, 1.0, 0.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0)]
    pl["point_in_plane"] = [(0.0, 0.0, 0.0), (0.0, 0.0, 7.0), (-6.0, 0.0, 0.0)]
    for i, m in enumerate((matte(), S.mirror(), S.stone())):
        _set_material(pl[i:i + 1], m)
    li = base.lights.copy()
    li["origin"] = [(-2.0, 3.2, 2.0), (2.0, 2.8, 0.2), (1.0, 4.0, 5.0)]
    li["radius"] = 0.3
    return S.Scene(sp, pl, li)


_scenes = {}


def scene_of(name):
    """`hall`, `demo` (the demo scene) or a scene of cast_common (small, cloud ...), built once"""
    if name not in _scenes:
        _scenes[name] = hall_scene() if name == "hall" else S.render_map_scene() if name == "demo" else cc.scene_of(name)
    return _scenes[name]


def unit_rays(scene, n, seed, eye=(0.8, 2.5, -8.0)):
    """api.RAY_QUERY [n] of UNIT directions (normalised in float32: what a camera hands out), tmax = inf, ignore = ID_NONE, cycling through:
    from the eye toward a point on or near a primitive; from a random point above the floor in a random direction; from inside a sphere;
    from the eye up and away from everything; toward a light."""
    rng = np.random.default_rng(seed)
    tg = cc._targets(scene)
    lights = [t for t in tg if t[0] >> 30 == 2]
    pts = np.array([t[1] for t in tg], F)
    lo, hi = pts.min(0) - 1, pts.max(0) + 1
    rays = np.zeros(n, api.RAY_QUERY)
    rays["tmax"], rays["ignore"] = np.inf, cc.ID_NONE
    eye = np.asarray(eye, F)
    for k in range(n):
        what = k % 8
        r = rays[k]
        if what in (0, 1, 2):
            _, c, rad = tg[int(rng.integers(len(tg)))]
            o = eye + rng.uniform(-1, 1, 3).astype(F) * F(what)
            d = c + rng.normal(size=3).astype(F) * F(0.6 * max(rad, 0.5)) - o
        elif what in (3, 4):
            o = rng.uniform(lo, hi).astype(F)
            o[1] = abs(o[1]) + F(0.05)
            d = rng.normal(size=3).astype(F)
        elif what == 5 and len(scene.spheres):
            i = int(rng.integers(len(scene.spheres)))
            u = rng.normal(size=3)
            o = scene.spheres["origin"][i] + (u / np.linalg.norm(u) * rng.uniform(0, 0.9) * abs(float(scene.spheres["radius"][i]))).astype(F)
            d = rng.normal(size=3).astype(F)
        elif what == 6 or not lights:
            o = eye
            d = np.array([rng.uniform(-1, 1), rng.uniform(0.5, 2), rng.uniform(-3, -1)], F)
        else:
            _, c, rad = lights[int(rng.integers(len(lights)))]
            o = eye + rng.uniform(-2, 2, 3).astype(F)
            d = c + rng.normal(size=3).astype(F) * F(0.3 * rad) - o
        d = np.asarray(d, F)
        r["origin"], r["dir"] = o, d / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    rays.setflags(write=False)
    return rays


# ---- the rule, over the oracle's reflect and refract
def _f3(v):
    import ctypes as C
    return (C.c_float * 3)(*[float(x) for x in v])


def oracle_reflect(oracle, d, n):
    out = _f3((0, 0, 0))
    oracle.lib.wo_reflect(_f3(d), _f3(n), out)
    return np.array(out[:], F)


def oracle_refract(oracle, n1, n2, d, n):
    out = _f3((0, 0, 0))
    oracle.lib.wo_refract(float(n1), float(n2), _f3(d), _f3(n), out)
    return np.array(out[:], F)


def material_of(scene, idw):
    arr = scene.spheres if idw >> 30 == 0 else scene.planes
    return arr["material"][idw & 0x3FFFFFFF]


def chain_model(oracle, rays, flags, B, scene):
    """-> (result as api.paths_result, events): every path followed in Python.  A segment's hit is the ray queries' definition
    (api.cast_rays_host) of the path's current ray; the next ray is built from wo_reflect / wo_refract with the n1 / n2 rule of
    whitted_oracle.c:481-508 restated here: n2 = material n if n1 == DEFAULT_N else DEFAULT_N; n1 < n2: the origin steps 2 EPSILON inside, else
    the normal is negated; a NaN x falls back to the reflected ray, n1 unchanged.  events: per ray, a list per recorded hit of one of
    "reflect", "enter", "leave", "tir", "stop_matte", "stop_light", plus "matte_goes_on" where ALL_SURFACES continued off a matte surface."""
    rays = np.ascontiguousarray(rays, api.RAY_QUERY).reshape(-1)
    n = rays.size
    cast_flags = flags & (cc.KINDS | cc.OPAQUE)
    hits = np.zeros((B, n), api.HIT)
    hits["t"], hits["id"] = np.inf, cc.ID_NONE
    status = np.zeros(n, np.uint8)
    cur = rays.copy()
    n1 = np.full(n, DEFAULT_N, F)
    alive = np.ones(n, bool)
    events = [[] for _ in range(n)]
    for k in range(B):
        if not alive.any():
            break
        idx = np.flatnonzero(alive)
        seg = api.cast_rays_host(cur[idx], cast_flags, scene.spheres, scene.planes, scene.lights)
        for j, i in enumerate(idx):
            h = seg[j]
            idw = int(h["id"])
            if idw == cc.ID_NONE:
                status[i] = k | MISSED << 4
                alive[i] = False
                continue
            hits[k, i] = h
            nrm, d = h["normal"].astype(F), cur[i]["dir"].astype(F)
            p = h["point"] + nrm * EPSILON
            m = None if idw >> 30 == 2 else material_of(scene, idw)
            matte_hit = m is not None and m["reflectivity"] == 0 and not m["dielectric"] and not m["transperent"]
            if m is None or (matte_hit and not flags & ALL_SURFACES):
                events[i].append("stop_light" if m is None else "stop_matte")
                cur[i]["origin"], cur[i]["dir"], cur[i]["ignore"] = p, 0, cc.ID_NONE
                status[i] = (k + 1) | ENDED << 4
                alive[i] = False
                continue
            o, out, what = p, oracle_reflect(oracle, d, nrm), "matte_goes_on" if matte_hit else "reflect"
            if flags & TRANSMIT and m["transperent"]:
                n2 = F(m["n"]) if n1[i] == DEFAULT_N else DEFAULT_N
                entering = n1[i] < n2
                through = oracle_refract(oracle, n1[i], n2, d, nrm if entering else nrm * F(-1))
                if np.isnan(through[0]):
                    what = "tir"
                else:
                    o, out, what = (p - nrm * (F(2) * EPSILON) if entering else p), through, "enter" if entering else "leave"
                    n1[i] = n2
            events[i].append(what)
            cur[i]["origin"], cur[i]["dir"], cur[i]["ignore"] = o, out, cc.ID_NONE
            if k + 1 == B:
                status[i] = B | BOUNCES << 4
    return api.paths_result(hits, status, cur), events


def census(result, events, B):
    """name -> number of rays of one case on which the thing happens (CENSUS; all_surfaces_goes_on: a matte surface sent the path on)"""
    count, reason = result["count"], result["reason"]
    flat = [set(e) for e in events]
    return {"reaches_B": int((reason == BOUNCES).sum()), "miss_first": int(((reason == MISSED) & (count == 0)).sum()),
            "miss_later": int(((reason == MISSED) & (count > 0)).sum()), "stop_matte": sum("stop_matte" in e for e in flat),
            "stop_light": sum("stop_light" in e for e in flat), "enter_glass": sum("enter" in e for e in flat),
            "leave_glass": sum("leave" in e for e in flat), "tir": sum("tir" in e for e in flat),
            "all_surfaces_goes_on": sum("matte_goes_on" in e for e in flat), "rays": len(events)}


def assert_census(censuses):
    """over the cases of one ray set: each thing of CENSUS happens on some ray and does not happen on some ray"""
    for name in CENSUS:
        hit = sum(c[name] for c in censuses)
        total = sum(c["rays"] for c in censuses)
        assert 0 < hit < total, (name, hit, total)


def differing(got, want):
    """differing bytes of the three arrays of two path results"""
    return tuple(int((np.frombuffer(got[k].tobytes(), np.uint8) != np.frombuffer(want[k].tobytes(), np.uint8)).sum()) for k in ("hits", "status", "next"))
