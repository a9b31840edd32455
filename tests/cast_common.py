"""Shared by test_cast_host.py and test_gpu_cast.py: the ray queries (include/hip_wrap_ext.h: clw_ray, clw_hit, clw_host_cast_rays,
clw_host_occluded_rays) restated in numpy from the header's text -- float32, one rounding per operation, dot products left to right --, the
scenes both test modules run and the seeded maker of their ray sets.  Everything is compared for equality of bits."""
import numpy as np

import ao_common as ac
from example_gui_opencl_raytracer_amd import api
from example_gui_opencl_raytracer_amd import scene as S

F = np.float32
SPHERES, PLANES, LIGHTS, KINDS, OPAQUE = 1, 2, 4, 7, 8
KIND_PLANE, KIND_LIGHT, ID_NONE = 1 << 30, 2 << 30, 0xFFFFFFFF
TMAX = (0.25, 3.0, np.inf)
N_HOST = 193
KIND_COMBOS = (1, 2, 3, 4, 5, 6, 7)


# ---- the rule, float32, one rounding per operation, in the header's order
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _sphere(o, d, A, c, q):
    v = o - c
    Cq = _dot(v, v) - q
    B = _dot(v, d)
    D = B * B + (-(A * Cq))
    s = np.sqrt(D)
    t0 = (-B - s) / A
    t = np.where(t0 < 0, (-B + s) / A, t0)
    return ~(D < 0) & ~(t <= 0), t


def _plane(o, d, n, p0):
    num = _dot(p0 - o, n)
    B = _dot(d, n)
    t = num / B
    return ~(B == 0) & ~(t <= 0), t


def cast_model(rays, flags, spheres, planes, lights):
    """-> (api.HIT [n], uint8 [n]): the nearest hit and the any-hit answer of every ray, by the header's rules"""
    rays = np.ascontiguousarray(rays, api.RAY_QUERY).reshape(-1)
    n = rays.size
    o, d, tmax, ignore = rays["origin"].astype(F), rays["dir"].astype(F), rays["tmax"].astype(F), rays["ignore"]
    ns, npl, nl = (0 if a is None else len(a) for a in (spheres, planes, lights))
    tbest, best, blocked = np.full(n, np.inf, F), np.full(n, ID_NONE, np.uint32), np.zeros(n, bool)
    centre, normal = np.zeros((n, 3), F), np.zeros((n, 3), F)          # of the best so far: a sphere's or light's centre, a plane's normal

    def take(hit, t, idw, c=None, nn=None):
        nonlocal tbest, best, blocked, centre, normal
        cand = hit & (t <= tmax) & (ignore != np.uint32(idw))
        blocked |= cand
        better = cand & (t < tbest)
        tbest = np.where(better, t, tbest)
        best = np.where(better, np.uint32(idw), best)
        if c is not None:
            centre = np.where(better[:, None], c, centre)
        else:
            normal = np.where(better[:, None], nn, normal)

    with np.errstate(all="ignore"):
        A = _dot(d, d)
        if flags & SPHERES:
            for i in range(ns):
                r = F(spheres["radius"][i])
                if (flags & OPAQUE) and spheres["material"]["transperent"][i] != 0:
                    continue
                c = spheres["origin"][i].astype(F)
                take(*_sphere(o, d, A, c, np.abs(r * r)), i, c=c)
        if flags & PLANES:
            for i in range(npl):
                nn = planes["normal"][i].astype(F)
                take(*_plane(o, d, nn, planes["point_in_plane"][i].astype(F)), KIND_PLANE | i, nn=nn)
        if flags & LIGHTS:
            for i in range(nl):
                r = F(lights["radius"][i])
                c = lights["origin"][i].astype(F)
                take(*_sphere(o, d, A, c, np.abs(r * r)), KIND_LIGHT | i, c=c)
        hits = np.zeros(n, api.HIT)
        hits["t"], hits["id"] = tbest, best
        found = best != ID_NONE
        point = d * tbest[:, None] + o
        w = point - centre
        length = np.sqrt(_dot(w, w))
        round_normal = w / length[:, None]
        is_plane = (best >> np.uint32(30)) == 1
        hits["point"] = np.where(found[:, None], point, F(0))
        hits["normal"] = np.where(found[:, None], np.where(is_plane[:, None], normal, round_normal), F(0))
    return hits, blocked.astype(np.uint8)


# ---- scenes
def small_scene(spheres=True, planes=True):
    """ao_common's small scene -- two opaque spheres, a glass one of negative radius, a floor, a slanted plane with a normal that is not unit,
    three lights -- and a fourth sphere that coincides with sphere 1: equal t, the lower index must win"""
    sc = ac.small_scene(spheres, planes)
    if not spheres:
        return sc
    sp = np.concatenate([sc.spheres, sc.spheres[1:2]])
    return S.Scene(sp, sc.planes, sc.lights)


def ns257_scene():
    import grid_common as gridc
    base = S.render_map_scene()
    o, r = gridc.HOST_LAYOUTS["ns257"]()
    return S.Scene(gridc.spheres_of(o, r), base.planes[:1], base.lights)


def cloud_scene():
    from fuzz_scenes import grid_layout
    return grid_layout("cloud")[0]


# ---- the tangent pair: an equal t met from two cells of the grid
TANGENT_A = ((0.75, 0.0, 1.0), 1.25)                 # the small sphere (centre, radius) ...
TANGENT_B = ((6.0, 0.0, 8.0), 10.0)                  # ... and the large one it touches from inside at (0, 0, 0)
TANGENT_FILLERS = 300
# (origin, direction): both meet A and B at t = 1 exactly in float32 -- along x: b = -70, D = 36 and b = -112, D = 2304; along z: b = -20, D = 16
# and b = -48, D = 1024 -- after a stretch inside B's box alone (5.5 units along x, 1.75 along z)
TANGENT_EXACT = (((-8.0, 0.0, 0.0), (8.0, 0.0, 0.0)), ((0.0, 0.0, -4.0), (0.0, 0.0, 4.0)))
TANGENT_SHIFT = (3.0, 12.0, 5.0)                     # moves the whole construction; every term above stays exact
TANGENT_VARIANTS = {"tangent": {}, "tangent_opaque": dict(glass=False), "tangent_swapped": dict(swapped=True),
                    "tangent_shifted": dict(shift=TANGENT_SHIFT)}


def tangent_scene(glass=True, swapped=False, shift=(0.0, 0.0, 0.0)):
    """Two spheres that touch internally where a ray meets them, so that both give the same t bits, with more than 256 spheres around them
    so that the scene takes the uniform grid: the small sphere A at index 0 (glass, or opaque), the large B (opaque) at the last index --
    `swapped`: the other way round, the control in which a cell's ascending order alone gives the answer.  B's box is (nearly) the grid's
    bounds, so B is listed in every cell and a ray from outside A's box walks cells that list B alone before the cell of the hit, which
    lists both: the walk holds B when it meets A, the LOWER index, at an equal t.  The fillers (r 0.1 .. 0.3, inside B's box, |y| >= 1.5) keep
    off both exact rays; the floor lies below B's box, parallel to both."""
    rng = np.random.default_rng(0x7A96)
    n = TANGENT_FILLERS
    sp = S.sphere_grid_scene(n + 2, 1).spheres.copy()          # plastic spheres with hashed colours: the geometry is overwritten
    fill = rng.uniform([-3.7, 1.5, -1.7], [15.7, 9.7, 17.7], (n, 3))
    fill[:, 1] *= rng.choice([-1.0, 1.0], n)
    a, b = (n + 1, 0) if swapped else (0, n + 1)
    sp["origin"][1:n + 1] = fill.astype(F)
    sp["radius"][1:n + 1] = rng.uniform(0.1, 0.3, n).astype(F)
    sp["origin"][a], sp["radius"][a] = TANGENT_A
    sp["origin"][b], sp["radius"][b] = TANGENT_B
    if glass:
        g = S.glass()
        for name in ("ambient", "diffuse", "specular", "shininess", "transperent", "dielectric", "n", "reflectivity"):
            sp["material"][name][a] = g[name]
    base = S.render_map_scene()
    planes, li = base.planes[:1].copy(), base.lights.copy()
    planes["normal"], planes["point_in_plane"] = (0.0, 1.0, 0.0), (0.0, -12.0, 0.0)
    li["origin"] = [(3.0, 4.0, 2.0), (-2.0, 6.0, 9.0), (9.0, -3.0, 5.0)]
    li["radius"] = (0.1, 0.08, 0.1)
    shift = np.asarray(shift, F)
    sp["origin"] += shift
    li["origin"] += shift
    planes["point_in_plane"] += shift
    return S.Scene(sp, planes, li)


def tangent_ids(name):
    """(index of A, index of B) in a variant of the tangent scene"""
    n = TANGENT_FILLERS
    return (n + 1, 0) if TANGENT_VARIANTS[name].get("swapped") else (0, n + 1)


def tangent_exact_rays(name):
    """api.RAY_QUERY [5 * len(TANGENT_EXACT)]: each exact ray as it stands, ignoring A, ignoring B, ending at tmax = 1 and at nextafter(1, 0)"""
    shift = np.asarray(TANGENT_VARIANTS[name].get("shift", (0.0, 0.0, 0.0)), F)
    a, b = tangent_ids(name)
    rays = np.zeros(5 * len(TANGENT_EXACT), api.RAY_QUERY)
    rays["tmax"], rays["ignore"] = np.inf, ID_NONE
    for k, (o, d) in enumerate(TANGENT_EXACT):
        rays["origin"][5 * k:5 * k + 5] = np.asarray(o, F) + shift
        rays["dir"][5 * k:5 * k + 5] = d
        rays["ignore"][5 * k + 1], rays["ignore"][5 * k + 2] = a, b
        rays["tmax"][5 * k + 3], rays["tmax"][5 * k + 4] = F(1), np.nextafter(F(1), F(0))
    return rays


def tangent_rays(name, seed, n=N_HOST):
    """-> (api.RAY_QUERY [n + 10], where the exact rays sit): make_rays' set of the scene with the exact rays spread among it, so that their
    lanes share waves with rays of other walk lengths"""
    base = make_rays(scene_of(name), n, seed)[0]
    exact = tangent_exact_rays(name)
    at = (np.arange(exact.size) * (n // exact.size) + 7).astype(np.int64)      # positions in `base` in front of which they go
    rays = np.insert(base, at, exact)
    where = at + np.arange(exact.size)
    assert rays[where].tobytes() == exact.tobytes()
    rays.setflags(write=False)
    return rays, where


def tangent_cells(name, reg_pad=0.0):
    """The premise of the tangent scenes on the grid the library builds for them (grid_common.build_grid, the shim's density and `reg_pad`):
    per exact ray -> (cells the ray is in before the cell of the hit that list B and not A, whether the cell of the hit lists both).  The
    cells are taken from points 1 / 64 of a unit apart along the ray, in float64: a cell crossed for less than that may be missed, which can
    only lose a B-only cell, never invent one."""
    import grid_common as gridc
    sc = scene_of(name)
    G = gridc.build_grid(sc.spheres, reg_pad)
    gridc.check_grid(sc.spheres["origin"], sc.spheres["radius"], reg_pad, G)
    a, b = tangent_ids(name)
    res, gmin, cell = G["res"], G["gmin"].astype(np.float64), G["cell"].astype(np.float64)
    shift = np.asarray(TANGENT_VARIANTS[name].get("shift", (0.0, 0.0, 0.0)), np.float64)

    def listed(p):
        k = np.floor((p - gmin) / cell).astype(np.int64)
        if (k < 0).any() or (k >= res).any():
            return None, None
        c = int((k[2] * res[1] + k[1]) * res[0] + k[0])
        return c, set(G["items"][G["start"][c]:G["start"][c + 1]].tolist())
    out = []
    for o, d in TANGENT_EXACT:
        o, d = np.asarray(o, np.float64) + shift, np.asarray(d, np.float64)
        hit_cell, at_hit = listed(o + d)
        steps = int(np.linalg.norm(d) * 64)
        before = {}
        for t in np.arange(steps) / steps:
            c, items = listed(o + t * d)
            if c is not None and c != hit_cell:
                before[c] = items
        out.append((sorted(c for c, items in before.items() if b in items and a not in items), a in at_hit and b in at_hit))
    return out, G


SCENES = {"planes": lambda: small_scene(spheres=False), "spheres": lambda: small_scene(planes=False), "small": small_scene, "ns257": ns257_scene,
          "cloud": cloud_scene, "tangent": tangent_scene}
_scenes = {}


GRID_SCENES = ("giants", "coincident", "touching", "tower")      # fuzz_scenes.grid_layout: more than 256 spheres each


def scene_of(name):
    """a scene of SCENES, a variant of the tangent scene (TANGENT_VARIANTS) or a grid layout (GRID_SCENES), built once"""
    if name not in _scenes:
        if name in SCENES:
            _scenes[name] = SCENES[name]()
        elif name in TANGENT_VARIANTS:
            _scenes[name] = tangent_scene(**TANGENT_VARIANTS[name])
        else:
            from fuzz_scenes import grid_layout
            assert name in GRID_SCENES, name
            _scenes[name] = grid_layout(name)[0]
    return _scenes[name]


# ---- ray sets
def _targets(scene):
    """(id word, centre or point in the plane, radius or 0) of every primitive"""
    out = [(i, s["origin"].astype(F), abs(float(s["radius"]))) for i, s in enumerate(scene.spheres)]
    out += [(KIND_PLANE | i, p["point_in_plane"].astype(F), 0.0) for i, p in enumerate(scene.planes)]
    out += [(KIND_LIGHT | i, l["origin"].astype(F), abs(float(l["radius"]))) for i, l in enumerate(scene.lights)]
    return out


def make_rays(scene, n, seed):
    """-> (api.RAY_QUERY [n], info): a seeded ray set for a scene.  About two thirds of it are base rays, cycling through: random origins inside
    and outside the scene's bounds with random directions that are not unit; rays that start inside a sphere; rays aimed at a primitive's centre
    (a plane's point) from nearby with d = (target - origin) * scale, every other one ignoring its target; rays aimed away from everything; rays
    with a zero direction, a NaN origin, a NaN tmax, an infinite direction (the unwalkable ones).  Behind them, from the model's unlimited cast
    of the base rays against every kind: second-bounce rays (origin = a hit's point, direction = its normal, ignore = its id) and, for a
    quarter of the hits, the same ray once with tmax = t exactly and once with tmax = nextafter(t, 0).  info: index arrays `away`, `odd`,
    `inside`, `bounce`, `edge_at`, `edge_below` and `edge_id` (the id the edge rays' originals met)."""
    rng = np.random.default_rng(seed)
    sp = scene.spheres
    tg = _targets(scene)
    by_kind = [g for g in ([t for t in tg if t[0] >> 30 == kind] for kind in range(3)) if g]
    pts = np.array([t[1] for t in tg], F)
    lo, hi = pts.min(0) - 2, pts.max(0) + 2
    nb = n if n < 12 else (2 * n) // 3
    rays = np.zeros(nb, api.RAY_QUERY)
    rays["tmax"], rays["ignore"] = np.inf, ID_NONE
    away, odd, inside = [], [], []
    rnd = lambda: (rng.normal(size=3) * 10.0 ** rng.uniform(-0.7, 0.7)).astype(F)
    for k in range(nb):
        what = k % 12
        r = rays[k]
        if what in (0, 1, 10):
            r["origin"], r["dir"] = rng.uniform(lo, hi), rnd()
        elif what == 2:
            r["origin"], r["dir"] = rng.uniform(3 * lo, 3 * hi), rnd()
            if k % 24 == 2:                                     # ... half of them toward the scene
                r["dir"] = (pts[rng.integers(len(pts))] - r["origin"]) * F(rng.uniform(0.2, 2.0))
        elif what == 3 and len(sp):
            i = int(rng.integers(len(sp)))
            u = rng.normal(size=3)
            r["origin"] = sp["origin"][i] + (u / np.linalg.norm(u) * rng.uniform(0, 0.9) * abs(float(sp["radius"][i]))).astype(F)
            r["dir"] = rnd()
            inside.append(k)
        elif what in (3, 4, 5, 6, 9, 11):
            group = by_kind[(k // 12 + what) % len(by_kind)]      # the kinds in turn, then any primitive of the kind
            idw, c, rad = group[int(rng.integers(len(group)))]
            u = rng.normal(size=3)
            r["origin"] = c + (u / np.linalg.norm(u) * (rad + rng.uniform(0.05, 2.5))).astype(F)
            r["dir"] = (c - r["origin"]) * F(10.0 ** rng.uniform(-0.5, 1.0))
            if k % 2:
                r["ignore"] = idw
        elif what == 7:
            r["origin"] = hi + F(5) + rng.uniform(0, 3, 3).astype(F)
            r["dir"] = (r["origin"] - (lo + hi) / 2) * F(rng.uniform(0.2, 2.0))      # straight away from the middle of the scene
            away.append(k)
        else:                                                   # what == 8
            r["origin"], r["dir"] = rng.uniform(lo, hi), rnd()
            kind = (k // 12) % 4
            if kind == 0:
                r["dir"] = 0
            elif kind == 1:
                r["origin"][int(rng.integers(3))] = np.nan
            elif kind == 2:
                r["tmax"] = np.nan
            else:
                r["dir"][int(rng.integers(3))] = np.inf
            odd.append(k)
    first, _ = cast_model(rays, KINDS, scene.spheres, scene.planes, scene.lights)
    hit = np.flatnonzero(first["id"] != ID_NONE)
    extra = np.zeros(n - nb, api.RAY_QUERY)
    extra["tmax"], extra["ignore"] = np.inf, ID_NONE
    extra["origin"], extra["dir"] = hi + F(5), F(1)            # what is left over: more rays away from everything
    info = dict(away=list(away), odd=list(odd), inside=list(inside), bounce=[], edge_at=[], edge_below=[], edge_id=[])
    k = 0
    n_bounce = min(len(hit), (n - nb) // 3)
    for h in hit[rng.permutation(len(hit))[:n_bounce]]:
        extra[k]["origin"], extra[k]["dir"], extra[k]["ignore"] = first["point"][h], first["normal"][h], first["id"][h]
        info["bounce"].append(nb + k)
        k += 1
    for h in hit[rng.permutation(len(hit))[:len(hit) // 4]]:
        if k + 2 > n - nb:
            break
        for which, tm in (("edge_at", first["t"][h]), ("edge_below", np.nextafter(first["t"][h], F(0)))):
            extra[k] = rays[h]
            extra[k]["tmax"] = tm
            info[which].append(nb + k)
            k += 1
        info["edge_id"].append(int(first["id"][h]))
    info["away"] += list(range(nb + k, n))
    out = np.concatenate([rays, extra])
    out.setflags(write=False)
    return out, {key: np.asarray(v, np.int64) for key, v in info.items()}


def with_tmax(rays, tmax, per_ray):
    """the ray set with another tmax: everywhere (scalar), or the values of TMAX dealt over the rays with `tmax` first (per ray); the edge
    rays and the NaN ones keep theirs"""
    out = rays.copy()
    keep = np.isnan(rays["tmax"]) | np.isfinite(rays["tmax"])
    new = np.roll(np.asarray(TMAX, F), -TMAX.index(tmax))[np.arange(rays.size) % 3] if per_ray else np.full(rays.size, tmax, F)
    out["tmax"] = np.where(keep, rays["tmax"], new)
    return out


def spread(scene, rays, flags, hits):
    """what a case decides, from its expected hits: the kinds hit, whether a ray misses, how many rays `ignore` changed and how many a
    transparent sphere let pass (against the model without ignore / without OPAQUE)"""
    kinds = set((hits["id"][hits["id"] != ID_NONE] >> np.uint32(30)).tolist())
    plain = rays.copy()
    plain["ignore"] = ID_NONE
    no_ignore = cast_model(plain, flags, scene.spheres, scene.planes, scene.lights)[0]
    passed = 0
    if flags & OPAQUE:
        passed = int((cast_model(rays, flags & ~OPAQUE, scene.spheres, scene.planes, scene.lights)[0]["id"] != hits["id"]).sum())
    return dict(kinds=kinds, miss=bool((hits["id"] == ID_NONE).any()), ignored=int((no_ignore["id"] != hits["id"]).sum()), passed=passed)


def kinds_present(scene, flags):
    """the enabled kinds the scene has primitives of, as id kinds 0 / 1 / 2"""
    return {k for k, (bit, arr) in enumerate(((SPHERES, scene.spheres), (PLANES, scene.planes), (LIGHTS, scene.lights))) if flags & bit and len(arr)}


def assert_decides(scene, rays, flags, hits, what=""):
    """a case may not pass on empty ground"""
    s = spread(scene, rays, flags, hits)
    assert s["kinds"] == kinds_present(scene, flags), (what, s)
    assert s["miss"] and s["ignored"] > 0, (what, s)
    transparent = len(scene.spheres) and (scene.spheres["material"]["transperent"] != 0).any()
    if flags & OPAQUE:
        assert (s["passed"] > 0) == bool(flags & SPHERES and transparent), (what, s)
    return s


def dump_cases(directory, n=N_HOST, seed=17):
    """the host test's ray set of every scene as a binary file for tools/cast_sanitize.c: four u32 { rays, spheres, planes, lights }, then the
    records"""
    import os
    os.makedirs(directory, exist_ok=True)
    for name in SCENES:
        sc = scene_of(name)
        rays, _ = make_rays(sc, n, seed)
        with open(os.path.join(directory, name + ".bin"), "wb") as f:
            f.write(np.array([rays.size, len(sc.spheres), len(sc.planes), len(sc.lights)], "<u4").tobytes())
            for a in (rays, sc.spheres, sc.planes, sc.lights):
                f.write(np.ascontiguousarray(a).tobytes())
