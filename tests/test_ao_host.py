"""The ambient occlusion pass on the CPU (include/hip_wrap_ext.h: clw_host_ao_dirs, clw_host_ao_open, clw_host_ao_resolve; csrc/ao_host.c): the
host definitions against the numpy restatement of tests/ao_common.py -- the direction table within 1 float32 ulp of the float64 formulas, the
open-ray counts and the resolve bit for bit -- closed forms between a floor and a ceiling, what ids and normals outside the ordinary yield,
and every refusal."""
import ctypes as C

import numpy as np
import pytest

import ao_common as ac
from example_gui_opencl_raytracer_amd import api
from example_gui_opencl_raytracer_amd import scene as S

F = np.float32


# ------------------------------------------------------------------ (a) the direction table
@pytest.mark.parametrize("K", ac.RAYS)
def test_dirs_follow_the_formulas(K):
    got = api.ao_dirs(K)
    exact, want = ac.dirs_model(K)
    assert got.shape == (16, K, 4) and got.dtype == np.float32
    worst = int(ac.ulps(got[..., :3], want[..., :3]).max())
    length = np.sqrt((got[..., :3].astype(np.float64) ** 2).sum(-1))
    print(f"K = {K}: at most {worst} ulp from the float64 formulas; | |l| - 1 | <= {np.abs(length - 1).max():.3g}; min z {got[..., 2].min():.6g}")
    assert worst <= 1
    assert (got[..., 3] == 0).all()
    assert (np.abs(length - 1) <= 2.0 ** -22).all()
    assert (got[..., 2] > 0).all() and (exact[..., 2] >= np.sqrt(0.03125 / K) * (1 - 1e-12)).all()
    # stratified in elevation: ray i of every pattern lies in stratum i of u1 = x^2 + y^2
    u1 = (exact[..., 0] ** 2 + exact[..., 1] ** 2) * K
    assert (np.floor(u1 + 1e-9).astype(int) == np.arange(K)[None, :]).all()


# ------------------------------------------------------------------ (b) the open rays
@pytest.mark.parametrize("radius", [0.25, 3.0, np.inf])
@pytest.mark.parametrize("K", ac.RAYS)
def test_open_equals_the_numpy_model(K, radius):
    W, H, first_row = 13, 7, 3
    sc = ac.small_scene()
    point, normal, ids = ac.channels(sc, W, H, seed=11)
    ao = api.ao_params(K, radius)
    dirs = api.ao_dirs(K)
    got = api.ao_open(point, normal, ids, W, H, first_row, sc.spheres, sc.planes, ao, dirs)
    want = ac.open_model(point, normal, ids, W, H, first_row, sc.spheres, sc.planes, K, radius, dirs)
    print(f"K = {K}, radius {radius}: {int((got != want).sum())} of {W * H} counts differ; histogram of the counts {np.bincount(got, minlength=K + 1).tolist()}")
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    if K == 32 and radius == 3.0:
        assert got.min() == 0 and got.max() == K and len(np.unique(got)) > 8      # the scene decides something
    # another first row is another pattern row: the counts follow the model there too
    assert np.array_equal(api.ao_open(point, normal, ids, W, H, 0, sc.spheres, sc.planes, ao, dirs),
                          ac.open_model(point, normal, ids, W, H, 0, sc.spheres, sc.planes, K, radius, dirs))


def slab(h):
    """a floor at y = 0 with normal +y and a ceiling plane at height h"""
    base = S.render_map_scene()
    pl = base.planes[:2].copy()
    pl["normal"] = [(0.0, 1.0, 0.0), (0.0, 1.0, 0.0)]
    pl["point_in_plane"] = [(0.0, 0.0, 0.0), (0.0, h, 0.0)]
    return S.Scene(base.spheres[:0], pl, base.lights)


@pytest.mark.parametrize("h,want", [(0.01, 0), (2.0, 32)])
def test_closed_forms_under_a_ceiling(h, want):
    """K = 32, radius 1: every ray of a floor point meets the ceiling at t = h / l.z; l.z >= sqrt(0.03125 / 32) = 1 / 32, so h = 0.01 gives
    t <= 0.32 <= 1 -- all occluded -- and h = 2 gives t >= 2 > 1 -- all open.  (The floor itself is met at t = 0: no hit.)"""
    W, H, K = 9, 5, 32
    sc = slab(h)
    rng = np.random.default_rng(3)
    point = np.zeros((W * H, 3), F)
    point[:, 0], point[:, 2] = rng.uniform(-50, 50, W * H), rng.uniform(-50, 50, W * H)
    normal = np.tile(F([0, 1, 0]), (W * H, 1))
    ids = np.full(W * H, ac.KIND_PLANE | 0, np.uint32)
    got = api.ao_open(point, normal, ids, W, H, 0, None, sc.planes, api.ao_params(K, 1.0))
    assert (got == want).all(), np.unique(got)


def test_ids_that_are_no_surface_are_open():
    W, H, K = 6, 2, 5
    sc = ac.small_scene()
    ns, npl = len(sc.spheres), len(sc.planes)
    point = np.tile(F([0.0, 1.0, 0.0]), (W * H, 1))                # the middle of sphere 0: every ray of a surface id is occluded
    normal = np.tile(F([0, 1, 0]), (W * H, 1))
    ids = np.array([0, ac.KIND_PLANE, ac.ID_NONE, ac.KIND_LIGHT, ac.KIND_LIGHT | 2, (3 << 30) | 1, ns, ns + 100, ac.KIND_PLANE | npl, 0x3FFFFFFF,
                    1, ac.KIND_PLANE | 1], np.uint32)
    got = api.ao_open(point, normal, ids, W, H, 0, sc.spheres, sc.planes, api.ao_params(K, 10.0))
    assert got.tolist() == [0, 0, K, K, K, K, K, K, K, K, 0, 0]


def test_zero_and_nan_normals_yield_the_models_value():
    W, H, K = 8, 4, 32
    sc = ac.small_scene()
    rng = np.random.default_rng(5)
    point = rng.uniform(-1.5, 1.5, (W * H, 3)).astype(F)
    normal = np.zeros((W * H, 3), F)
    normal[1::2] = np.nan
    normal[3::4, 1] = 0.5                                           # NaN in some components only
    normal[2::8] = (0.0, 0.0, -0.0)
    ids = np.where(np.arange(W * H) % 3 == 0, ac.KIND_PLANE, 0).astype(np.uint32)
    dirs = api.ao_dirs(K)
    for radius in (0.5, np.inf):
        got = api.ao_open(point, normal, ids, W, H, 1, sc.spheres, sc.planes, api.ao_params(K, radius), dirs)
        want = ac.open_model(point, normal, ids, W, H, 1, sc.spheres, sc.planes, K, radius, dirs)
        assert np.array_equal(got, want)
        assert (got[np.isnan(normal).all(1)] == K).all()           # a NaN direction is never occluded
    assert (want[::2] < K).any()                                    # ... while a zero normal still has directions (its basis is t, u)


# ------------------------------------------------------------------ (c) the resolve
@pytest.mark.parametrize("size", ac.RESOLVE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_resolve_equals_the_integer_model(size):
    bad, cases = [], ac.resolve_cases([size])
    for (w, h, name, flags, strength, K) in cases:
        counts, frame = ac.resolve_inputs(w, h, K)
        ids = ac.id_field(name, w, h)
        ao = api.clw_ao(flags, K, 1.0, strength)
        got = api.ao_resolve(counts, ids, frame if flags & ac.AO_COMPOSE else None, w, h, ao)
        if not np.array_equal(got, ac.resolve_model(counts, ids, frame, w, h, flags, K, strength)):
            bad.append((w, h, name, flags, strength, K))
    print(f"{size[0]} x {size[1]}: {len(cases)} cases, {len(bad)} differ from the model {bad[:8]}")
    assert not bad


def test_resolve_endpoints():
    """all rays open = white (the frame itself with COMPOSE) at any strength; none open = black at strength 256, white at strength 0"""
    w, h, K = 9, 9, 5
    ids, frame = ac.id_field("checker", w, h), ac.resolve_inputs(w, h, K)[1]
    full, none = np.full(w * h, K, np.uint8), np.zeros(w * h, np.uint8)
    for flags in (0, ac.AO_FILTER):
        assert (api.ao_resolve(full, ids, None, w, h, api.clw_ao(flags, K, 1.0, 200)) == 0xFFFFFF).all()
        assert (api.ao_resolve(none, ids, None, w, h, api.clw_ao(flags, K, 1.0, 256)) == 0).all()
        assert (api.ao_resolve(none, ids, None, w, h, api.clw_ao(flags, K, 1.0, 0)) == 0xFFFFFF).all()
        assert np.array_equal(api.ao_resolve(full, ids, frame, w, h, api.clw_ao(flags | ac.AO_COMPOSE, K, 1.0, 256)), frame & 0xFFFFFF)
        assert (api.ao_resolve(none, ids, frame, w, h, api.clw_ao(flags | ac.AO_COMPOSE, K, 1.0, 256)) == 0).all()


# ------------------------------------------------------------------ refusals: 0, nothing written
def test_every_refusal():
    L = api.load_library()
    W, H, K = 4, 3, 5
    n = W * H
    sc = ac.small_scene()
    point, normal, ids = ac.channels(sc, W, H, seed=2)
    point, normal = np.ascontiguousarray(point), np.ascontiguousarray(normal)
    dirs = api.ao_dirs(K)
    counts, frame = ac.resolve_inputs(W, H, K)
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    SENT = 0xA5

    def open_(ao, point=point, normal=normal, ids=ids, w=W, h=H, sp=sc.spheres, ns=3, pl=sc.planes, npl=2, dirs=dirs, out=True):
        o = np.full(n, SENT, np.uint8)
        r = L.clw_host_ao_open(P(point), P(normal), P(ids), w, h, 0, P(sp), ns, P(pl), npl, None if ao is None else C.byref(ao), P(dirs), P(o) if out else None)
        assert (o == SENT).all() or r == 1
        return r

    def resolve_(ao, counts=counts, ids=ids, frame=frame, w=W, h=H, out=True):
        o = np.full(n, 0xA5A5A5A5, np.uint32)
        r = L.clw_host_ao_resolve(P(counts), P(ids), P(frame), w, h, None if ao is None else C.byref(ao), P(o) if out else None)
        assert (o == 0xA5A5A5A5).all() or r == 1
        return r

    good = api.clw_ao(3, K, 1.0, 256)
    assert open_(good) == 1 and resolve_(good) == 1 and open_(api.clw_ao(0, K, np.inf, 0)) == 1 and resolve_(api.clw_ao(0, K, np.inf, 0), frame=None) == 1
    assert open_(good, sp=None, ns=0) == 1 and open_(good, pl=None, npl=0) == 1      # a scene without spheres, without planes
    bad_params = [None, api.clw_ao(4, K, 1.0, 256), api.clw_ao(0x80000001, K, 1.0, 256), api.clw_ao(0, 0, 1.0, 256), api.clw_ao(0, 33, 1.0, 256),
                  api.clw_ao(0, K, np.nan, 256), api.clw_ao(0, K, 0.0, 256), api.clw_ao(0, K, -0.0, 256), api.clw_ao(0, K, -1.0, 256),
                  api.clw_ao(0, K, -np.inf, 256), api.clw_ao(0, K, 1.0, 257)]
    for ao in bad_params:
        assert open_(ao) == 0 and resolve_(ao) == 0, None if ao is None else (ao.flags, ao.rays, ao.radius, ao.strength)
    for kw in (dict(point=None), dict(normal=None), dict(ids=None), dict(dirs=None), dict(out=False), dict(sp=None), dict(pl=None), dict(w=0), dict(h=0),
               dict(w=1 << 15, h=1 << 15), dict(w=1 << 30, h=1)):
        assert open_(good, **kw) == 0, kw
    for kw in (dict(counts=None), dict(ids=None), dict(frame=None), dict(out=False), dict(w=0), dict(h=0), dict(w=1 << 15, h=1 << 15), dict(w=1, h=1 << 30)):
        assert resolve_(good, **kw) == 0, kw
    assert resolve_(api.clw_ao(1, K, 1.0, 256), frame=None) == 1                    # no COMPOSE: the frame is not read
    # the table
    tab = np.full((16, 33, 4), 9.0, np.float32)
    for k in (0, 33, 1 << 31):
        assert L.clw_host_ao_dirs(k, P(tab)) == 0 and (tab == 9.0).all()
    assert L.clw_host_ao_dirs(K, None) == 0
    with pytest.raises(ValueError):
        api.ao_dirs(0)
    with pytest.raises(ValueError):
        api.ao_open(point, normal, ids, W, H, 0, sc.spheres, sc.planes, api.ao_params(0))
    with pytest.raises(ValueError):
        api.ao_resolve(counts, ids, None, W, H, api.ao_params(K, compose=True))


def test_the_header_states_the_definition_and_what_is_not_built():
    from render_common import header_text
    text = header_text()
    for word in ("CLW_AO_FILTER", "CLW_AO_COMPOSE", "clw_host_ao_dirs", "0.6180339887498949", "copysignf", "CLW_TIMING_AO_RESOLVE", "a latched mode",
                 "toward the viewer", "accumulation of AO over frames"):
        assert word in text, word
    assert C.sizeof(api.clw_ao) == 16 and (api.TIMING_AO, api.TIMING_AO_RESOLVE) == (0x414F5452, 0x414F5253)
