"""Layered ray queries on the GPU (include/hip_wrap_ext.h: clw_ext_cast_layers, clw_ext_cast_layers_device, clw_ext_camera_rays,
clw_ext_render_layers, clw_ext_pick_layers; csrc/whitted_layers.inc) against the host definition (csrc/layers_host.c: clw_host_cast_layers,
clw_host_camera_rays) -- bit for bit, in both builds, no tolerance anywhere.  The scenes reach each geometry source of wt_cast_layers (staged in
LDS, read from global memory, walked through the uniform grid) and both compiled list capacities; the ray sets are those of
tests/layers_common.py."""
import ctypes as C

import numpy as np
import pytest

import cast_common as cc
import grid_common as gridc
import layers_common as lc
from conftest import CAM
from render_common import R, api, bits, released, rendering  # noqa: F401  (R, api: the fixtures)
from test_gpu_cast import FLAG_SETS as CAST_FLAG_SETS
from test_gpu_cast import SIZES, WT_V_GEOM_GLOBAL, assert_tangent_premise, bare_scene_wrapper, read_framebuffer
from test_gpu_cast import UNIT_SCENES as CAST_UNIT_SCENES

pytestmark = pytest.mark.gpu

S, P, L, O = cc.SPHERES, cc.PLANES, cc.LIGHTS, cc.OPAQUE
K_EVERY_SIZE = (1, 4, 8)                 # the smaller kernel alone, full, the larger one full
K_AT_193 = (2, 3, 5, 7)
FLAG_SETS = dict({name: sets for name, sets in CAST_FLAG_SETS.items() if name not in lc.GRID_SCENES}, stack=(S | P, S | P | L | O), **{name: (S | P, S | P | L | O) for name in lc.GRID_SCENES})
# name -> (setup of the wrapper, the geometry the pass must take: "lds" | "global" | "grid")
SCENES = {name: how for name, how in CAST_UNIT_SCENES.items() if name.split("-")[0] not in lc.GRID_SCENES}
SCENES.update({"stack": (None, "lds"), "stack-global": (lambda w: w.set_variant(WT_V_GEOM_GLOBAL), "global")})
for _name in lc.GRID_SCENES:             # each grid layout walked and scanned: grid == linear == the definition
    SCENES.update({_name + "-grid": (None, "grid"), _name + "-linear": (lambda w: w.set_grid(0), "global")})
DECIDING = ("small", "stack", "ns257", "cloud") + lc.GRID_SCENES      # the scenes whose cases are held to layers_common.assert_decides
FRAMES = ((9, 9), (61, 43))
MODELS = ("perspective", "ortho", "equirect")
_expected = {}


@pytest.fixture(scope="module", params=[True, False], ids=["strict", "fast"])
def strict(request):
    import torch  # noqa: F401
    return request.param


def api_mod():
    from example_gui_opencl_raytracer_amd import api as a
    return a


def expected(name):
    """[(n, flags, K, rays, {"t", "id"}) ...] of one scene: the host definition, computed once, shared by both builds and by the scene's
    flavours, never written to.  Before anything is compared the cases are held to what they must decide (layers_common.assert_decides, from
    the numpy model's candidate counts of the sets of 193 and 4099 rays)."""
    base = name.split("-")[0]
    if base not in _expected:
        a, sc, rows, spreads, opaque_spreads = api_mod(), lc.scene_of(base), [], [], []
        for flags in FLAG_SETS[base]:
            for n in SIZES:
                rays = lc.rays_for(base, n, seed=n)
                for K in K_EVERY_SIZE + (K_AT_193 if n == 193 else ()):
                    want = a.cast_layers_host(rays, flags, K, sc.spheres, sc.planes, sc.lights)
                    want["t"].setflags(write=False)
                    want["id"].setflags(write=False)
                    rows.append((n, flags, K, rays, want))
                if n >= 193:
                    t, ids, count = lc.candidates(rays, flags, sc.spheres, sc.planes, sc.lights)
                    (opaque_spreads if flags & O else spreads).append(lc.spread(sc, rays, flags, count, t, ids))
        if base in DECIDING:
            for K in sorted(set(K_EVERY_SIZE + K_AT_193)):
                lc.assert_decides(base, K, spreads + opaque_spreads, opaque_spreads)
        _expected[base] = rows
    return _expected[base]


def differing(got, want):
    return int((got["t"].view(np.uint32) != want["t"].view(np.uint32)).sum() + (got["id"] != want["id"]).sum())


def view(model, W, H):
    """(camera structure, projection or None) of a camera model over a W x H frame"""
    a = api_mod()
    if model == "ortho":
        return a.ortho_camera((0.8, 2.5, -8.0), (0.2, -0.1, 1.0), 14.0, W, H)
    cam = a.perspective(CAM["origin"], CAM["look"], CAM["fov"], CAM["focal"], W, H)
    return cam, (a.projection(a.PROJ_EQUIRECT, (0.2, 0.0, 1.0)) if model == "equirect" else None)


def look_through(r, cam, proj):
    r.set_camera(cam)
    r.w.set_projection(proj)


# ------------------------------------------------------------------ 1. against the definition
@pytest.mark.parametrize("name", list(SCENES))
def test_layers_equal_the_definition(R, api, tex, sky, strict, name):
    base = name.split("-")[0]
    sc, (setup, geometry) = lc.scene_of(base), SCENES[name]
    bad = []
    with rendering(R, sc, tex, sky, 8, 8, setup=setup, cam=None, strict=strict) as r:
        for (n, flags, K, rays, want) in expected(name):
            got = r.w.cast_layers(rays, flags, K)
            assert got is not None and got["t"].shape == got["id"].shape == (K, n) and got["t"].dtype == np.float32 and got["id"].dtype == np.uint32
            d = differing(got, want)
            if d:
                bad.append((n, flags, K, d))
        grid = r.w.get_grid()
        assert bool(grid and grid["built"]) == (len(sc.spheres) > gridc.GRID_MIN_SPHERES)
        # the geometry the pass took: the grid when one is built and on, LDS for a small scene unless the variant says global
        took = "grid" if grid and grid["built"] and "linear" not in name else ("lds" if len(sc.spheres) <= gridc.GRID_MIN_SPHERES and "global" not in name else "global")
        assert took == geometry
    print(f"{name} {'strict' if strict else 'fast'}: {len(expected(name))} cases, differing words {sum(b[3] for b in bad)} {bad[:8]}")
    assert not bad


# ------------------------------------------------------------------ 1b. an equal t met from two cells of the grid
TANGENT_FLAGS = (S, S | P | L, S | P | L | O)
TANGENT_K = (1, 2, 8)


@pytest.mark.parametrize("name", list(cc.TANGENT_VARIANTS))
def test_an_equal_t_across_cells_is_listed_in_id_order(R, api, tex, sky, strict, monkeypatch, name):
    """test_gpu_cast.py's tangent pair under the list sink: the walk holds the large sphere B from the cells that list it alone when it meets
    the small sphere A at the same t.  At K = 1 the list's worst entry is B itself and A, the lower index, must replace it (the rule
    `t == worst_t && !(i < worst_i)` of wt_layers_insert); at K = 2 both are listed, lower index first; both compiled capacities."""
    sc = cc.scene_of(name)
    a, b = cc.tangent_ids(name)
    rays, where = cc.tangent_rays(name, seed=193)
    bad = []
    with rendering(R, sc, tex, sky, 8, 8, cam=None, strict=strict) as r:
        for capacity in (None, "8"):
            if capacity:
                monkeypatch.setenv("CLWRAP_LAYERS_CAPACITY", capacity)      # (read on every call)
            for flags in TANGENT_FLAGS:
                for K in TANGENT_K:
                    want = api.cast_layers_host(rays, flags, K, sc.spheres, sc.planes, sc.lights)
                    if not flags & O:
                        assert want["id"][0][where[0::5]].tolist() == [min(a, b)] * len(cc.TANGENT_EXACT)
                        assert K < 2 or want["id"][1][where[0::5]].tolist() == [max(a, b)] * len(cc.TANGENT_EXACT)
                    got = r.w.cast_layers(rays, flags, K)
                    d = differing(got, want)
                    if d:
                        bad.append((capacity, flags, K, d, got["id"][:, where[0::5]].tolist()))
        assert_tangent_premise(name, r.w.get_grid())
    print(f"{name} {'strict' if strict else 'fast'}: capacities 4 / 8 and 8 x {len(TANGENT_FLAGS)} flag sets x K {TANGENT_K}; (capacity, flags, K, differing words, ids of the exact rays) {bad}")
    assert not bad


# ------------------------------------------------------------------ 2. the device path
@pytest.mark.parametrize("name", ["stack", "cloud-grid"])
def test_device_path_equals_the_host_array_call(R, api, tex, sky, strict, name):
    import torch
    sc = lc.scene_of(name.split("-")[0])
    with rendering(R, sc, tex, sky, 8, 8, cam=None, strict=strict) as r:
        for K in (3, 8):
            n, flags, _, rays, want = [e for e in expected(name) if e[0] == (193 if K == 3 else 4099) and e[2] == K][1]
            host = r.w.cast_layers(rays, flags, K)
            d_rays = torch.from_numpy(np.frombuffer(rays.tobytes(), np.uint8).copy()).cuda()
            for own_stream in (True, False):
                d_t = torch.full((K * n,), -1.0, dtype=torch.float32, device="cuda")
                d_id = torch.full((K * n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                if own_stream:                                     # the wrapper's stream
                    assert r.cast_layers_device(d_rays.data_ptr(), n, K, d_t.data_ptr(), d_id.data_ptr(), kinds=flags & cc.KINDS, opaque_only=bool(flags & O)) == n
                    r.w.sync()
                else:                                              # torch's current stream, after set_stream
                    stream = torch.cuda.Stream()
                    with torch.cuda.stream(stream):
                        r.w.set_stream(torch.cuda.current_stream().cuda_stream)
                        assert r.w.cast_layers_device(d_rays.data_ptr(), n, flags, K, d_t.data_ptr(), d_id.data_ptr()) == n
                        early_t, early_id = d_t.cpu(), d_id.cpu()          # (ordered behind the launch on that stream)
                    stream.synchronize()
                torch.cuda.synchronize()
                got = {"t": d_t.cpu().numpy().reshape(K, n), "id": d_id.cpu().numpy().view(np.uint32).reshape(K, n)}
                print(f"{name} {'strict' if strict else 'fast'} K {K} {'wrapper stream' if own_stream else 'torch stream'}: differing words "
                      f"{differing(got, host)} from the host-array call, {differing(got, want)} from the definition")
                assert differing(got, host) == 0 and differing(got, want) == 0
                if not own_stream:
                    assert early_t.numpy().tobytes() == want["t"].tobytes() and early_id.numpy().tobytes() == want["id"].tobytes()
            r.w.set_stream(0)


# ------------------------------------------------------------------ 3. layer 0 is the nearest-hit query
@pytest.mark.parametrize("name", ["small", "stack", "cloud-grid", "coincident-grid"])
def test_layer_0_is_the_nearest_hit(R, api, tex, sky, strict, name):
    sc = lc.scene_of(name.split("-")[0])
    with rendering(R, sc, tex, sky, 8, 8, cam=None, strict=strict) as r:
        for (n, flags, K, rays, want) in [e for e in expected(name) if e[0] == 4099 and e[2] in (1, 8)]:
            hits = r.w.cast_rays(rays, flags)
            got = r.w.cast_layers(rays, flags, K)
            finite = np.isfinite(hits["t"])
            assert finite.sum() > 100 and (~finite).sum() > 100
            assert np.array_equal(got["t"][0][finite].view(np.uint32), hits["t"][finite].view(np.uint32)) and np.array_equal(got["id"][0][finite], hits["id"][finite])
            assert (got["id"][0][~finite] == cc.ID_NONE).all() and np.isposinf(got["t"][0][~finite]).all()


# ------------------------------------------------------------------ 4. the camera rays
@pytest.mark.parametrize("model", MODELS)
def test_camera_rays_equal_the_definition(R, api, demo_scene, tex, sky, strict, model):
    import torch
    for W, H in FRAMES:
        cam, proj = view(model, W, H)
        want = api.camera_rays_host(cam, proj)
        assert want.size == W * H and np.isfinite(want["dir"]).all()
        with rendering(R, demo_scene, tex, sky, W, H, cam=None, strict=strict) as r:
            assert r.w.camera_rays(W * H) is None                        # no camera latched yet
            look_through(r, cam, proj)
            got = r.camera_rays()
            assert got.dtype == api.RAY_QUERY and got.tobytes() == want.tobytes(), (model, W, H, int((got.view(np.uint8) != want.view(np.uint8)).sum()))
            assert r.w.camera_rays(W * H - 1) is None                    # too small a capacity
            d = torch.full((W * H * 32 + 32,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert r.w.camera_rays_device(d.data_ptr(), W * H - 1) == 0 and r.w.camera_rays_device(0, W * H) == 0
            assert r.w.camera_rays_device(d.data_ptr(), W * H) == W * H
            r.w.sync()
            back = d.cpu().numpy()
            assert back[:W * H * 32].tobytes() == want.tobytes() and (back[W * H * 32:] == 0xA5).all()
    # a strip -- an id offset of whole rows -- holds the frame's rows
    W, H = FRAMES[1]
    cam, proj = view(model, W, H)
    want = api.camera_rays_host(cam, proj)
    for first_row, rows in ((8, 16), (40, 3)):
        with rendering(R, demo_scene, tex, sky, W, H, cam=None, strict=strict, first_row=first_row, rows=rows) as r:
            look_through(r, cam, proj)
            got = r.camera_rays()
            assert got.size == rows * W and got.tobytes() == want[first_row * W:(first_row + rows) * W].tobytes()
            assert got.tobytes() == api.camera_rays_host(cam, proj, first_row * W, (first_row + rows) * W).tobytes()


# ------------------------------------------------------------------ 5. and 6. the layers of the view, and the pick through them
@pytest.mark.parametrize("model", MODELS)
def test_layers_of_the_view_and_pick_through(R, api, demo_scene, tex, sky, strict, model):
    W, H = FRAMES[1]
    cam, proj = view(model, W, H)
    rays = api.camera_rays_host(cam, proj)
    sc = demo_scene
    with rendering(R, sc, tex, sky, W, H, cam=None, strict=strict) as r:
        look_through(r, cam, proj)
        assert r.w.read_layers(api.LAYERS_T).size == 0 and not r.w.layers_device_ptr(api.LAYERS_ID)
        for K, kinds, opaque_only, flags in ((4, ("sphere", "plane"), False, S | P), (8, ("sphere", "plane", "light"), False, S | P | L),
                                             (2, ("sphere", "plane"), True, S | P | O), (1, ("sphere",), False, S)):
            want = api.cast_layers_host(rays, flags, K, sc.spheres, sc.planes, sc.lights)
            got = r.layers(K, kinds, opaque_only)
            assert got["t"].shape == got["id"].shape == (K, H, W)
            d = differing({"t": got["t"].reshape(K, -1), "id": got["id"].reshape(K, -1)}, want)
            print(f"{model} {'strict' if strict else 'fast'} K {K} flags {flags}: {d} differing words; deepest list {int((want['id'] != cc.ID_NONE).sum(0).max())}")
            assert d == 0
            assert r.w.layers_device_ptr(api.LAYERS_T) and r.w.layers_device_ptr(api.LAYERS_ID) and not r.w.layers_device_ptr(2)
        full = r.layers(8)
        depth = (full["id"] != cc.ID_NONE).sum(0)
        assert depth.max() >= 3 and depth.min() < depth.max()                  # the view shows depth
        # 6. a pick is that pixel's column, at the corners and inside
        for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2), (17, 29), (44, 31)):
            for K in (1, 5, 8):
                p = r.w.pick_layers(x, y, S | P, K)
                assert p is not None and p.dtype == api.LAYER and p.size == K
                assert np.array_equal(p["t"].view(np.uint32), full["t"][:K, y, x].view(np.uint32)) and np.array_equal(p["id"], full["id"][:K, y, x]), (x, y, K)
            through = r.pick_through(x, y)
            assert [e["id"] for e in through] == [int(i) for i in full["id"][:, y, x] if i != cc.ID_NONE]
            assert all(e["kind"] == e["id"] >> 30 and e["index"] == e["id"] & 0x3FFFFFFF for e in through)
            assert [bits(e["depth"])[()] for e in through] == [bits(t)[()] for t, i in zip(full["t"][:, y, x], full["id"][:, y, x]) if i != cc.ID_NONE]
        assert r.w.pick_layers(W, 0, S | P, 4) is None and r.w.pick_layers(0, H, S | P, 4) is None and r.pick_through(W, H) is None
    # a strip picks its own rows only
    with rendering(R, sc, tex, sky, W, H, cam=None, strict=strict, first_row=8, rows=16) as r:
        look_through(r, cam, proj)
        strip = r.layers(8)
        assert strip["t"].tobytes() == full["t"][:, 8:24].tobytes() and strip["id"].tobytes() == full["id"][:, 8:24].tobytes()
        assert r.w.pick_layers(5, 7, S | P, 8) is None and r.w.pick_layers(5, 24, S | P, 8) is None
        assert r.w.pick_layers(5, 8, S | P, 8)["id"].tolist() == full["id"][:, 8, 5].tolist()


# ------------------------------------------------------------------ 7. scene changes
@pytest.mark.parametrize("name", ["stack", "ns257-grid"])
def test_a_rewritten_scene_is_seen_after_invalidate(api, strict, name):
    import torch
    sc = lc.scene_of(name.split("-")[0])
    n, flags, K, rays, want = [e for e in expected(name) if e[0] == 193 and e[2] == 8][0]
    sph = torch.from_numpy(np.frombuffer(sc.spheres.tobytes(), np.uint8).copy()).cuda()
    with released(bare_scene_wrapper(api, sc, sph)) as cw:
        cw.set_strict(strict)
        assert differing(cw.cast_layers(rays, flags, K), want) == 0
        moved = sc.spheres.copy()
        listed = want["id"][want["id"] >> 30 == 0]
        victim = int(np.bincount(listed).argmax())                                        # the sphere most lists hold
        moved["origin"][victim] += np.float32([0.75, 0.5, -0.25])
        sph.copy_(torch.from_numpy(np.frombuffer(moved.tobytes(), np.uint8).copy()))
        torch.cuda.synchronize()
        cw.invalidate_scene()
        again = api.cast_layers_host(rays, flags, K, moved, sc.planes, sc.lights)
        got = cw.cast_layers(rays, flags, K)
        print(f"{name} {'strict' if strict else 'fast'}: sphere {victim} moved, {int((again['id'] != want['id']).any(0).sum())} lists change, "
              f"{differing(got, again)} words differ from the definition")
        assert (again["id"] != want["id"]).any() and differing(got, again) == 0
        grid = cw.get_grid()
        assert bool(grid and grid["built"]) == ("grid" in name)


# ------------------------------------------------------------------ 8. refusals: 0, the outputs untouched, and the process goes on
def test_refusals_return_zero_and_the_wrapper_works_on(R, api, tex, sky, strict):
    import torch
    sc = lc.scene_of("stack")
    n, flags, K, rays, want = [e for e in expected("stack") if e[0] == 65 and e[2] == 4][0]
    Lib = api.load_library()
    P_ = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rays_c = np.ascontiguousarray(rays)

    def refused(cw):
        out_t, out_i = np.full(n * 8 * 4, 0xA5, np.uint8), np.full(n * 8 * 4, 0xA5, np.uint8)
        for kw in (dict(n=0), dict(n=1 << 30), dict(flags=0), dict(flags=O), dict(flags=16 | 3), dict(flags=0x80000003), dict(rays=None), dict(t=None),
                   dict(ids=None), dict(K=0), dict(K=9), dict(K=0xFFFFFFFF)):
            assert Lib.clw_ext_cast_layers(C.byref(cw.w), P_(kw.get("rays", rays_c)), kw.get("n", n), kw.get("flags", flags), kw.get("K", K),
                                           None if "t" in kw else P_(out_t), None if "ids" in kw else P_(out_i)) == 0, kw
        assert (out_t == 0xA5).all() and (out_i == 0xA5).all()
        d = torch.full((2 * n * 8 * 4,), 0xA5, dtype=torch.uint8, device="cuda")
        d_rays = torch.from_numpy(np.frombuffer(rays.tobytes(), np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        dt, di = d.data_ptr(), d.data_ptr() + n * 8 * 4
        for args in ((0, n, flags, K, dt, di), (d_rays.data_ptr(), 0, flags, K, dt, di), (d_rays.data_ptr(), n, 16 | 3, K, dt, di), (d_rays.data_ptr(), n, O, K, dt, di),
                     (d_rays.data_ptr(), n, flags, 0, dt, di), (d_rays.data_ptr(), n, flags, 9, dt, di), (d_rays.data_ptr(), n, flags, K, 0, di),
                     (d_rays.data_ptr(), n, flags, K, dt, 0)):
            assert cw.cast_layers_device(*args) == 0, args
        assert cw.render_layers(0, 4) == 0 and cw.render_layers(S | P, 0) == 0 and cw.render_layers(S | P, 9) == 0 and cw.render_layers(16, 4) == 0
        assert cw.pick_layers(1, 1, 0, 4) is None and cw.pick_layers(1, 1, S | P, 9) is None
        lay = np.full(8, 0xA5A5A5A5, np.uint32).view(np.uint8).copy()
        assert Lib.clw_ext_pick_layers(C.byref(cw.w), 1, 1, S | P, 0, P_(lay)) == 0 and Lib.clw_ext_pick_layers(C.byref(cw.w), 1, 1, S | P, 4, None) == 0
        assert (lay == 0xA5).all()
        torch.cuda.synchronize()
        assert (d.cpu().numpy() == 0xA5).all()
        return d_rays, d

    with released(api.ClWrap()) as w:                                            # no scene bound, no camera latched
        w.set_strict(strict)
        d_rays, d = refused(w)
        assert w.cast_layers(rays, flags, K) is None and w.render_layers(S | P, 4) == 0 and w.pick_layers(0, 0, S | P, 4) is None
        assert w.camera_rays(64) is None and w.camera_rays_device(d.data_ptr(), 64) == 0
        assert w.cast_layers_device(d_rays.data_ptr(), n, flags, K, d.data_ptr(), d.data_ptr() + n * 32) == 0
        assert w.read_layers(api.LAYERS_T).size == 0 and w.read_layers(api.LAYERS_ID).size == 0 and not w.layers_device_ptr(0)
        torch.cuda.synchronize()
        assert (d.cpu().numpy() == 0xA5).all()
    with rendering(R, sc, tex, sky, 16, 16, depth=4, strict=strict, bands=(2, 1)) as r:      # row bands: no camera rays, so no layers of the view
        frame = r.render()
        assert r.w.camera_rays(16 * 16) is None and r.w.render_layers(S | P, 4) == 0 and r.w.pick_layers(3, 9, S | P, 4) is None
        with pytest.raises(RuntimeError):
            r.layers(4)
        assert differing(r.w.cast_layers(rays, flags, K), want) == 0                          # ... the caller's rays are served all the same
        assert np.array_equal(r.render(), frame)
    with rendering(R, sc, tex, sky, 16, 16, depth=4, strict=strict) as r:
        frame = r.render()
        refused(r.w)
        r.w.set_projection(api.projection(api.PROJ_EQUIRECT, (0.0, 1.0, 0.0)))                  # an axis along the camera's up: does not resolve
        assert r.w.camera_rays(16 * 16) is None and r.w.render_layers(S | P, 4) == 0 and r.w.pick_layers(3, 9, S | P, 4) is None
        r.w.set_projection(None)
        for call in (lambda: r.cast_layers(rays["origin"], rays["dir"], 4, kinds=()), lambda: r.cast_layers(np.zeros((0, 3)), np.zeros((0, 3))),
                     lambda: r.cast_layers(rays["origin"], rays["dir"], 9), lambda: r.layers(0)):
            with pytest.raises(RuntimeError):
                call()
        assert differing(r.w.cast_layers(rays, flags, K), want) == 0              # ... and the wrapper works behind them
        assert r.layers(4)["id"].shape == (4, 16, 16) and r.w.pick_layers(3, 9, S | P, 4) is not None
        assert np.array_equal(r.render(), frame)


# ------------------------------------------------------------------ 9. nothing else moves; the timing ids count the launches
def test_layers_leave_everything_else_alone(R, api, demo_scene, tex, sky, strict):
    W = H = 16
    rays = cc.make_rays(demo_scene, 193, 5)[0]
    state = {}
    for with_layers in (False, True):
        with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict, accumulate=4) as r:
            first = r.render()
            g = r.gbuffer()
            ao = r.ambient_occlusion(8, 1.0)
            counts = r.ao_counts().copy()
            picked = r.pick(5, 9)["id"]
            overlay = r.highlight([picked])
            table = r.objects()
            flags_before = r.w.last_trace_flags()
            if with_layers:
                got = r.cast_layers(rays["origin"], rays["dir"], 8, rays["tmax"], rays["ignore"], kinds=("sphere", "plane", "light"))
                assert differing(got, api.cast_layers_host(rays, cc.KINDS, 8, demo_scene.spheres, demo_scene.planes, demo_scene.lights)) == 0
                assert r.camera_rays().size == W * H and r.layers(8)["id"].shape == (8, H, W) and len(r.pick_through(5, 9)) >= 1
                for name, (bit, _, _) in api.GB_CHANNELS.items():
                    assert np.array_equal(bits(r.w.read_gbuffer(bit)) if name != "id" else r.w.read_gbuffer(bit), bits(g[name]) if name != "id" else g[name]), name
                assert np.array_equal(r.w.read_ao(api.AO_FRAME).reshape(H, W), ao) and np.array_equal(r.ao_counts(), counts)
                assert np.array_equal(r.w.read_overlay(), overlay) and r.objects().tobytes() == table.tobytes()
                assert r.w.last_trace_flags() == flags_before and r.accumulated == 1
                assert np.array_equal(read_framebuffer(r), first)
            second = r.render_rgb()
            state[with_layers] = (first, second[0], second[1], r.accumulated, r.w.read_tile_order())
    a, b = state[False], state[True]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2]))
    assert a[3] == b[3] == 2 and np.array_equal(a[4][0], b[4][0]) and a[4][1] == b[4][1]


def test_the_timing_ids_count_the_launches(R, api, demo_scene, tex, sky, strict):
    import torch
    rays = cc.make_rays(demo_scene, 193, 5)[0]
    with rendering(R, demo_scene, tex, sky, 64, 40, depth=4, strict=strict) as r:
        r.render()
        r.w.timing_reset()
        r.gbuffer(api.GB_ID)
        r.w.cast_rays(rays, cc.KINDS)
        r.render()
        for K in (1, 4, 8):
            r.w.cast_layers(rays, cc.KINDS, K)                                   # 3 layer launches
        r.layers(4)                                                             # 1 camera-ray launch, 1 layer launch
        r.camera_rays()                                                         # 1 camera-ray launch
        d_rays = torch.empty(64 * 40 * 32, dtype=torch.uint8, device="cuda")
        d_t = torch.empty(2 * 64 * 40, dtype=torch.float32, device="cuda")
        d_id = torch.empty(2 * 64 * 40, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert r.w.camera_rays_device(d_rays.data_ptr(), 64 * 40) == 64 * 40    # 1 camera-ray launch
        assert r.w.cast_layers_device(d_rays.data_ptr(), 64 * 40, S | P, 2, d_t.data_ptr(), d_id.data_ptr()) == 64 * 40      # 1 layer launch
        r.w.sync()
        assert r.w.pick_layers(3, 3, S | P, 8) is not None                       # a pick is not logged, as clw_ext_pick's is not
        assert r.w.cast_layers(rays, 0, 4) is None and r.w.render_layers(S | P, 9) == 0      # a refused call launches nothing
        n_layers, ms_layers = r.w.timing_get(api.TIMING_LAYERS)
        n_cam, ms_cam = r.w.timing_get(api.TIMING_CAMRAYS)
        assert n_layers == 5 and ms_layers > 0 and n_cam == 3 and ms_cam > 0
        # the parent's ids count what they counted
        assert r.w.timing_get(api.TIMING_GBUFFER)[0] == 1 and r.w.timing_get(api.TIMING_CAST)[0] == 1 and r.w.timing_get(1)[0] == 1
        assert r.w.timing_get(api.TIMING_AO)[0] == 0 and r.w.timing_get(api.TIMING_OVERLAY)[0] == 0


# ------------------------------------------------------------------ 10. the larger compiled capacity at a small K
@pytest.mark.parametrize("name", ["stack", "coincident-grid"])
def test_capacity_8_at_small_K_equals_the_definition(R, api, tex, sky, strict, monkeypatch, name):
    """CLWRAP_LAYERS_CAPACITY=8 (read on every call) runs the C = 8 kernel where K <= 4 would take C = 4: the worst entry, and the entry the grid
    walk ends on, is K - 1, not C - 1."""
    monkeypatch.setenv("CLWRAP_LAYERS_CAPACITY", "8")
    sc, (setup, geometry) = lc.scene_of(name.split("-")[0]), SCENES[name]
    cases = [e for e in expected(name) if e[2] in (1, 3, 4)]
    assert {e[2] for e in cases} == {1, 3, 4}
    bad = []
    with rendering(R, sc, tex, sky, 8, 8, setup=setup, cam=None, strict=strict) as r:
        for (n, flags, K, rays, want) in cases:
            d = differing(r.w.cast_layers(rays, flags, K), want)
            if d:
                bad.append((n, flags, K, d))
        grid = r.w.get_grid()
        assert bool(grid and grid["built"]) == (geometry == "grid")
    print(f"{name} {'strict' if strict else 'fast'} capacity 8: {len(cases)} cases, differing words {bad[:8]}")
    assert not bad
