"""Shared by test_near_host.py and test_gpu_near.py: the proximity queries (include/hip_wrap_ext.h: clw_probe, clw_host_nearest_surface,
clw_host_within_reach, clw_host_near_surfaces) restated in numpy from the header's text -- float32, one rounding per operation, dot products left
to right --, the seeded maker of their probe sets over cast_common's scenes, and the lattice scene.  Everything is compared for equality of
bits."""
import numpy as np

import cast_common as cc
import grid_common as gridc
from example_gui_opencl_raytracer_amd import api
from example_gui_opencl_raytracer_amd import scene as S

F = np.float32
SPHERES, PLANES, LIGHTS, KINDS, OPAQUE = cc.SPHERES, cc.PLANES, cc.LIGHTS, cc.KINDS, cc.OPAQUE
KIND_PLANE, KIND_LIGHT, ID_NONE = cc.KIND_PLANE, cc.KIND_LIGHT, cc.ID_NONE
KMAX = 8
N_HOST = 4099
SCENE_NAMES = ("planes", "spheres", "small", "ns257", "cloud") + cc.GRID_SCENES + ("tangent",)
KIND_COMBOS = (1, 2, 3, 4, 5, 6, 7)


# ---- the rule, float32, one rounding per operation, in the header's order
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _round(r):
    """the prepared word's magnitude |r * r| of a radius, and the radius the definition takes from it"""
    r = F(r)
    return np.sqrt(np.abs(r * r))


def near_model(probes, ignore, flags, spheres, planes, lights):
    """-> (api.HIT [n], uint8 [n], d float32 [KMAX, n], id uint32 [KMAX, n]): the nearest surface, the within answer and the KMAX nearest
    surfaces of every probe, by the header's rules"""
    probes = np.ascontiguousarray(probes, api.PROBE).reshape(-1)
    n = probes.size
    p, reach = probes["point"].astype(F), probes["reach"].astype(F)
    ignore = np.full(n, ID_NONE, np.uint32) if ignore is None else np.broadcast_to(np.asarray(ignore, np.uint32), (n,))
    ns, npl, nl = (0 if a is None else len(a) for a in (spheres, planes, lights))
    best, best_id, within = np.full(n, np.inf, F), np.full(n, ID_NONE, np.uint32), np.zeros(n, bool)
    normal, point = np.zeros((n, 3), F), np.zeros((n, 3), F)          # of the best so far
    ld, li = np.full((KMAX, n), np.inf, F), np.full((KMAX, n), ID_NONE, np.uint32)

    def take(d, idw, nrm, pt):
        nonlocal best, best_id, within, normal, point
        cand = (d <= reach) & (ignore != np.uint32(idw))
        within |= cand
        better = cand & (d < best)
        best = np.where(better, d, best)
        best_id = np.where(better, np.uint32(idw), best_id)
        normal = np.where(better[:, None], nrm, normal)
        point = np.where(better[:, None], pt, point)
        # the list, ordered by the key (d, id word): the candidate goes in, what it displaces is carried on
        cd, ci = np.where(cand & (d < np.inf), d, F(np.inf)).astype(F), np.full(n, idw, np.uint32)
        for j in range(KMAX):
            before = (cd < ld[j]) | ((cd == ld[j]) & (ci < li[j]))
            ld[j], cd = np.where(before, cd, ld[j]), np.where(before, ld[j], cd)
            li[j], ci = np.where(before, ci, li[j]), np.where(before, li[j], ci)

    def ball(c, radius, idw):
        v = p - c
        m = np.sqrt(_dot(v, v))
        r = _round(radius)
        nrm = v / m[:, None]
        take(m - r, idw, nrm, nrm * r + c)

    with np.errstate(all="ignore"):
        if flags & SPHERES:
            for i in range(ns):
                if (flags & OPAQUE) and spheres["material"]["transperent"][i] != 0:
                    continue
                ball(spheres["origin"][i].astype(F), spheres["radius"][i], i)
        if flags & PLANES:
            for i in range(npl):
                nn, p0 = planes["normal"][i].astype(F), planes["point_in_plane"][i].astype(F)
                s = _dot(p - p0, nn)
                take(np.abs(s), KIND_PLANE | i, np.broadcast_to(nn, (n, 3)), p - nn * s[:, None])
        if flags & LIGHTS:
            for i in range(nl):
                ball(lights["origin"][i].astype(F), lights["radius"][i], KIND_LIGHT | i)
    hits = np.zeros(n, api.HIT)
    hits["t"], hits["id"] = best, best_id
    found = best_id != ID_NONE
    hits["normal"] = np.where(found[:, None], normal, F(0))
    hits["point"] = np.where(found[:, None], point, F(0))
    li = np.where(ld < np.inf, li, np.uint32(ID_NONE))
    return hits, within.astype(np.uint8), ld, li


# ---- probe sets
def mean_radius(scene):
    r = np.abs(scene.spheres["radius"]) if len(scene.spheres) else np.abs(scene.lights["radius"])
    return F(r.mean()) if len(r) else F(1)


def grid_faces(scene):
    """points on the cell faces, gmin + k * cell, of the grids the library may build for the scene (the plain one and the one padded by the
    largest light radius) -> float32 [m, 3]; empty for a scene without a grid"""
    if len(scene.spheres) <= gridc.GRID_MIN_SPHERES:
        return np.zeros((0, 3), F)
    out = []
    pads = {0.0} | ({float(np.abs(scene.lights["radius"]).max())} if len(scene.lights) else set())
    for pad in sorted(pads):
        G = gridc.build_grid(scene.spheres, pad)
        gmin, cell, res = G["gmin"], G["cell"], G["res"]
        for k in range(8):
            idx = np.array([(3 * k + 1) % max(int(res[0]), 1), (5 * k + 2) % max(int(res[1]), 1), (7 * k) % max(int(res[2]), 1)])
            out.append((gmin + idx.astype(F) * cell).astype(F))
    return np.array(out, F)


def make_probes(scene, n, seed):
    """-> (api.PROBE [n], ignore uint32 [n], info): a seeded probe set for a scene.  About two thirds of it are base probes, cycling through:
    points in and around the scene's bounds; points inside spheres; points 0 to 3 mean radii off the surface of a primitive of each kind; the odd
    ones (a NaN coordinate, a NaN reach, an infinite coordinate, a point exactly at a sphere's centre); on grid scenes, points on cell faces.
    Their reaches cycle through {0, 0.5, 2, -0.25} mean radii; every fifth probe reaches +inf.  Behind them, from the model's unlimited first
    pass of the base probes against every kind: the same point with reach = d exactly and with nextafter(d, -inf), and the same point ignoring
    the id the first pass found.  info: index arrays `odd`, `inside`, `centre`, `edge_at`, `edge_below`, `ignoring`, `faces`."""
    rng = np.random.default_rng(seed)
    sp = scene.spheres
    tg = cc._targets(scene)
    by_kind = [g for g in ([t for t in tg if t[0] >> 30 == kind] for kind in range(3)) if g]
    pts = np.array([t[1] for t in tg], F)
    rbar = mean_radius(scene)
    lo, hi = pts.min(0) - 2 * rbar, pts.max(0) + 2 * rbar
    faces = grid_faces(scene)
    nb = n if n < 12 else (2 * n) // 3
    probes = np.zeros(nb, api.PROBE)
    reaches = (F(0), F(0.5) * rbar, F(2) * rbar, F(-0.25) * rbar)
    info = dict(odd=[], inside=[], centre=[], edge_at=[], edge_below=[], ignoring=[], faces=[])
    for k in range(nb):
        what = k % 12
        q = probes[k]
        q["reach"] = np.inf if k % 5 == 4 else reaches[(k // 3) % 4]
        if what in (0, 1):
            q["point"] = rng.uniform(lo, hi)
        elif what in (2, 3) and len(sp):
            i = int(rng.integers(len(sp)))
            u = rng.normal(size=3)
            q["point"] = sp["origin"][i] + (u / np.linalg.norm(u) * rng.uniform(0, 0.95) * abs(float(sp["radius"][i]))).astype(F)
            info["inside"].append(k)
        elif what == 10 and len(faces) and (k // 12) % 2 == 0:
            q["point"] = faces[(k // 24) % len(faces)]
            if (k // 24) % 3:                                  # ... some of them on one face only
                q["point"][1:] += rng.uniform(0, 1, 2).astype(F) * rbar
            info["faces"].append(k)
        elif what == 8 and (k // 12) % 2 == 0:
            q["point"] = rng.uniform(lo, hi)
            kind = (k // 24) % 4
            if kind == 0:
                q["point"][int(rng.integers(3))] = np.nan
            elif kind == 1:
                q["reach"] = np.nan
            elif kind == 2:
                q["point"][int(rng.integers(3))] = np.inf * (1 if k % 48 < 24 else -1)
            elif len(sp):
                q["point"] = sp["origin"][int(rng.integers(len(sp)))]
                info["centre"].append(k)
            info["odd"].append(k)
        else:                                                  # 0 to 3 mean radii off a surface, the kinds in turn
            group = by_kind[(k // 12 + what) % len(by_kind)]
            idw, c, rad = group[int(rng.integers(len(group)))]
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            off = rng.uniform(0, 3) * float(rbar)
            if idw >> 30 == 1:                                 # a plane: somewhere on it, then off along its normal, either side
                nn = scene.planes["normal"][idw & 0x3FFFFFFF].astype(np.float64)
                nn /= np.linalg.norm(nn)
                t = np.cross(nn, u)
                q["point"] = (c + t * rng.uniform(0, 4) + nn * off * rng.choice([-1.0, 1.0])).astype(F)
            else:
                q["point"] = (c + u * (rad + off)).astype(F)
    first = near_model(make_reach(probes, np.inf), None, KINDS, scene.spheres, scene.planes, scene.lights)[0]
    found = np.flatnonzero((first["id"] != ID_NONE) & np.isfinite(first["t"]))
    extra = np.zeros(n - nb, api.PROBE)
    extra["point"], extra["reach"] = hi + F(50) * rbar, rbar       # what is left over: probes away from everything
    ignore = np.full(n, ID_NONE, np.uint32)
    k = 0
    for h in found[rng.permutation(len(found))]:
        if k + 3 > n - nb:
            break
        d = first["t"][h]
        for which, value in (("edge_at", d), ("edge_below", np.nextafter(d, F(-np.inf))), ("ignoring", np.inf if k % 2 else F(2) * rbar + np.abs(d))):
            extra[k]["point"], extra[k]["reach"] = probes[h]["point"], value
            if which == "ignoring":
                ignore[nb + k] = first["id"][h]
            info[which].append(nb + k)
            k += 1
    out = np.concatenate([probes, extra])
    out.setflags(write=False)
    ignore.setflags(write=False)
    return out, ignore, {key: np.asarray(v, np.int64) for key, v in info.items()}


def make_reach(probes, reach):
    out = probes.copy()
    out["reach"] = reach
    return out


def spread(probes, hits, within, ld, K):
    """what a case decides, from the definition's output: the share of the finite-reach probes that have a candidate, whether some probe is
    inside a sphere or light (a negative d), whether some list is full and some holds between 1 and K - 1 entries"""
    finite = np.isfinite(probes["reach"])
    filled = (ld[:K] < np.inf).sum(0)
    return dict(share=float(np.asarray(within, bool)[finite].mean()), negative=bool((hits["t"] < 0).any()), full=bool((filled == K).any()),
                partial=bool(((filled >= 1) & (filled < K)).any()))


def assert_decides(probes, hits, within, ld, K, what=""):
    """a case over every kind may not pass on empty ground: among the probes of finite reach at least 20 % have a candidate and at least 20 %
    have none; some list is full and some is partly filled"""
    s = spread(probes, hits, within, ld, K)
    assert 0.2 <= s["share"] <= 0.8 and s["full"] and s["partial"], (what, s)
    return s


# ---- the lattice: radius-0.5 spheres at integer centres touch their axis neighbours exactly
LATTICE = (7, 7, 6)


def lattice_scene():
    nx, ny, nz = LATTICE
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    centres = np.stack([x, y, z], -1).reshape(-1, 3).astype(F)
    base = S.render_map_scene()
    return S.Scene(gridc.spheres_of(centres, np.full(len(centres), 0.5, F)), base.planes[:1], base.lights)


def lattice_neighbours(i):
    """the indices of sphere i's axis neighbours in the lattice, ascending"""
    nx, ny, nz = LATTICE
    x, y, z = i % nx, (i // nx) % ny, i // (nx * ny)
    out = []
    for dx, dy, dz in ((0, 0, -1), (0, -1, 0), (-1, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        a, b, c = x + dx, y + dy, z + dz
        if 0 <= a < nx and 0 <= b < ny and 0 <= c < nz:
            out.append((c * ny + b) * nx + a)
    return sorted(out)


def touching_probes(scene, margin=0.0):
    """touching_spheres' probes on the host: probe i at sphere i's centre, reach |r_i| + margin, ignoring sphere i"""
    sp = scene.spheres
    r = np.abs(sp["radius"].astype(F))
    return api.make_probes(sp["origin"], r + F(margin)), np.arange(len(sp), dtype=np.uint32), r
