"""Shared by test_layers_host.py and test_gpu_layers.py: the layered ray queries (include/hip_wrap_ext.h: clw_layer, clw_host_cast_layers)
restated in numpy from the header's text on top of cast_common's tests, the `stack` scene both test modules run, the ray sets, and what a case
has to decide before it may compare anything.  Everything is compared for equality of bits."""
import numpy as np

import cast_common as cc
from example_gui_opencl_raytracer_amd import api
from example_gui_opencl_raytracer_amd import scene as S

F = np.float32
K_MAX = 8
K_ALL = tuple(range(1, K_MAX + 1))
GRID_SCENES = cc.GRID_SCENES                                      # fuzz_scenes.grid_layout: more than 256 spheres each
TIE_SCENES = ("small", "stack", "coincident")                     # built with coincident spheres: two ids at one t
TRUNCATES_AT_8 = ("stack", "cloud", "coincident", "touching", "tower")      # some ray has more than 8 candidates; elsewhere more than K <= 4


# ---- the rule
def candidates(rays, flags, spheres, planes, lights):
    """-> (t float32 [n, m], ids uint32 [n, m], count [n]) over the m primitives that take part: every ray's LISTED candidates in the order
    (t ascending, id word ascending) -- a candidate (hit && t <= tmax, its id word not `ignore`, a transparent sphere not with OPAQUE) is
    listed iff t < inf --, the entries of the unlisted primitives, {inf, ID_NONE}, behind them; count = how many are listed"""
    rays = np.ascontiguousarray(rays, api.RAY_QUERY).reshape(-1)
    n = rays.size
    o, d, tmax, ignore = rays["origin"].astype(F), rays["dir"].astype(F), rays["tmax"].astype(F), rays["ignore"]
    ns, npl, nl = (0 if a is None else len(a) for a in (spheres, planes, lights))
    cols_t, cols_id = [], []

    def take(hit, t, idw):
        listed = hit & (t <= tmax) & (ignore != np.uint32(idw)) & (t < np.inf)
        cols_t.append(np.where(listed, t, F(np.inf)).astype(F))
        cols_id.append(np.where(listed, np.uint32(idw), np.uint32(cc.ID_NONE)))

    with np.errstate(all="ignore"):
        A = cc._dot(d, d)
        if flags & cc.SPHERES:
            for i in range(ns):
                r = F(spheres["radius"][i])
                if (flags & cc.OPAQUE) and spheres["material"]["transperent"][i] != 0:
                    continue
                take(*cc._sphere(o, d, A, spheres["origin"][i].astype(F), np.abs(r * r)), i)
        if flags & cc.PLANES:
            for i in range(npl):
                take(*cc._plane(o, d, planes["normal"][i].astype(F), planes["point_in_plane"][i].astype(F)), cc.KIND_PLANE | i)
        if flags & cc.LIGHTS:
            for i in range(nl):
                r = F(lights["radius"][i])
                take(*cc._sphere(o, d, A, lights["origin"][i].astype(F), np.abs(r * r)), cc.KIND_LIGHT | i)
    if not cols_t:
        return np.full((n, 1), np.inf, F), np.full((n, 1), cc.ID_NONE, np.uint32), np.zeros(n, np.int64)
    t, ids = np.stack(cols_t, 1), np.stack(cols_id, 1)
    order = np.argsort(t, axis=1, kind="stable")             # the columns are in id order: a stable sort by t is the sort by (t, id)
    t, ids = np.take_along_axis(t, order, 1), np.take_along_axis(ids, order, 1)
    return t, ids, (ids != cc.ID_NONE).sum(1)


def layers_of(sorted_t, sorted_id, K):
    """the first K columns of candidates(), padded with empty entries -> {"t": [K, n], "id": [K, n]} as the definition lays them out"""
    n, m = sorted_t.shape
    t, ids = np.full((K, n), np.inf, F), np.full((K, n), cc.ID_NONE, np.uint32)
    k = min(K, m)
    t[:k], ids[:k] = sorted_t[:, :k].T, sorted_id[:, :k].T
    return {"t": t, "id": ids}


# ---- scenes
def stack_scene():
    """12 spheres of radius 0.5 centred on the line y = 1, z = 0 at x = 0, 2, 4 ... -- sphere 7 coincides with sphere 3, sphere 5 is glass --,
    2 planes across the line (one with a normal that is not unit), 3 lights of which light 1 sits on the line.  46 float4: staged in LDS."""
    base = S.render_map_scene()
    sp = np.repeat(base.spheres[:1], 12).copy()
    sp["origin"] = [(2.0 * i, 1.0, 0.0) for i in range(12)]
    sp["origin"][7] = sp["origin"][3]
    sp["radius"] = 0.5
    g = S.glass()
    for name in ("ambient", "diffuse", "specular", "shininess", "transperent", "dielectric", "n", "reflectivity"):
        sp["material"][name][5] = g[name]
    pl = np.repeat(base.planes[:1], 2).copy()
    pl["normal"] = [(1.0, 0.0, 0.0), (-1.5, 0.25, 0.0)]
    pl["point_in_plane"] = [(-3.0, 0.0, 0.0), (25.0, 1.0, 0.0)]
    li = np.resize(base.lights, 3).copy()
    li["origin"] = [(4.0, 6.0, 3.0), (15.0, 1.0, 0.0), (-2.0, 3.0, -4.0)]
    li["radius"] = (0.3, 0.25, 0.2)
    return S.Scene(sp, pl, li)


def _grid(name):
    from fuzz_scenes import grid_layout
    return grid_layout(name)[0]


SCENES = dict(cc.SCENES, stack=stack_scene, **{name: (lambda name=name: _grid(name)) for name in GRID_SCENES})
_scenes = {}


def scene_of(name):
    if name in cc.SCENES or name in cc.TANGENT_VARIANTS or name in cc.GRID_SCENES:
        return cc.scene_of(name)
    if name not in _scenes:
        _scenes[name] = SCENES[name]()
    return _scenes[name]


# ---- ray sets
def line_rays(m, seed):
    """m rays along and near the stack's line, from either end and from inside a sphere: more than 8 candidates on one ray.  Every third keeps
    the line exactly (the coincident pair at one t), every fourth ignores a sphere on it, every fifth ends half way."""
    rng = np.random.default_rng(seed)
    rays = np.zeros(m, api.RAY_QUERY)
    rays["tmax"], rays["ignore"] = np.inf, cc.ID_NONE
    for k in range(m):
        r = rays[k]
        side = -1.0 if k % 2 else 1.0
        start = (-6.0 - rng.uniform(0, 2)) if side > 0 else (30.0 + rng.uniform(0, 2))
        if k % 7 == 6:
            start = 2.0 * int(rng.integers(12)) + rng.uniform(-0.3, 0.3)      # inside a sphere: its far side is listed
        exact = k % 3 == 0
        off = np.zeros(2) if exact else rng.uniform(-0.25, 0.25, 2)
        r["origin"] = (start, 1.0 + off[0], off[1])
        tilt = np.zeros(2) if exact else rng.uniform(-0.004, 0.004, 2)
        r["dir"] = np.array([side, tilt[0], tilt[1]]) * 10.0 ** rng.uniform(-0.5, 0.5)
        if k % 4 == 3:
            r["ignore"] = int(rng.integers(12))
        if k % 5 == 4:
            r["tmax"] = F(12.0 / np.linalg.norm(r["dir"]))
    return rays


def rays_for(name, n, seed):
    """the ray set of a scene: cast_common.make_rays', and for `stack` a third of it (at most 64) replaced by line_rays"""
    sc = scene_of(name)
    m = min(n // 3, 64) if name == "stack" else 0
    rays = cc.make_rays(sc, n - m, seed)[0]
    if m:
        rays = np.concatenate([rays, line_rays(m, seed)])
    rays.setflags(write=False)
    return rays


# ---- what a case decides
def spread(scene, rays, flags, count, sorted_t, sorted_id):
    """from the expected lists of one case: the largest count, how many rays hold none / an equal-t pair, how many lists `ignore` changed and
    how many OPAQUE changed (against the model without ignore / without OPAQUE)"""
    finite = sorted_id[:, 1:] != cc.ID_NONE
    ties = int(((sorted_t[:, 1:] == sorted_t[:, :-1]) & finite).any(1).sum()) if sorted_t.shape[1] > 1 else 0
    plain = rays.copy()
    plain["ignore"] = cc.ID_NONE
    no_ignore = candidates(plain, flags, scene.spheres, scene.planes, scene.lights)
    ignored = int((no_ignore[2] != count).sum())
    passed = 0
    if flags & cc.OPAQUE:
        passed = int((candidates(rays, flags & ~cc.OPAQUE, scene.spheres, scene.planes, scene.lights)[2] != count).sum())
    return dict(most=int(count.max()), none=int((count == 0).sum()), ties=ties, ignored=ignored, passed=passed, counts=count)


def assert_decides(name, K, spreads, opaque_spreads=()):      # noqa: C901
    """over the cases of one scene at one K (a spread per case): some ray has more than K listed candidates (at K = 8 on the scenes that
    reach it, at K <= 4 everywhere), some between 1 and K - 1, some none; an equal-t pair on the scenes built with coincident spheres;
    `ignore` changes some list; OPAQUE changes some list of the cases that set it, where the scene has a transparent sphere"""
    counts = np.concatenate([s["counts"] for s in spreads])
    if K <= 4 or name in TRUNCATES_AT_8:
        assert (counts > K).any(), (name, K, int(counts.max()))
    if K >= 2:
        assert ((counts >= 1) & (counts <= K - 1)).any(), (name, K)
    assert (counts == 0).any(), (name, K)
    if name in TIE_SCENES:
        assert sum(s["ties"] for s in spreads) > 0, name
    assert sum(s["ignored"] for s in spreads) > 0, name
    if opaque_spreads:
        assert (sum(s["passed"] for s in opaque_spreads) > 0) == bool((scene_of(name).spheres["material"]["transperent"] != 0).any()), name
