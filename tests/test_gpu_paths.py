"""Path queries on the GPU (include/hip_wrap_ext.h: clw_ext_cast_paths, clw_ext_cast_paths_device, clw_ext_pick_path; csrc/whitted_paths.inc)
against the host definition (csrc/paths_host.c: clw_host_cast_paths) -- hits, status and next, bit for bit, in both builds, no tolerance
anywhere.  The scenes reach each geometry source of wt_cast_paths (staged in LDS, read from global memory, walked through the uniform grid);
the ray sets and the `hall` scene are those of tests/paths_common.py."""
import ctypes as C

import numpy as np
import pytest

import cast_common as cc
import grid_common as gridc
import paths_common as pc
from render_common import R, api, bits, released, rendering  # noqa: F401  (R, api: the fixtures)
from test_gpu_cast import WT_V_GEOM_GLOBAL, read_framebuffer
from test_gpu_layers import FRAMES, MODELS, look_through, view

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257)             # one lane, a ragged wave, a whole one, one and a lane, several workgroups with a ragged tail
B_SET = (1, 2, 8)
# name -> (setup of the wrapper, the geometry the pass must take: "lds" | "global" | "grid")
SCENES = {
    "hall": (None, "lds"),
    "small": (None, "lds"),
    "demo": (None, "lds"),
    "small-global": (lambda w: w.set_variant(WT_V_GEOM_GLOBAL), "global"),
    "hall-global": (lambda w: w.set_variant(WT_V_GEOM_GLOBAL), "global"),
    "cloud-grid": (None, "grid"),
    "ns257-grid": (None, "grid"),
    "cloud-linear": (lambda w: w.set_grid(0), "global"),
}
_expected = {}


@pytest.fixture(scope="module", params=[True, False], ids=["strict", "fast"])
def strict(request):
    import torch  # noqa: F401
    return request.param


def api_mod():
    from example_gui_opencl_raytracer_amd import api as a
    return a


def rays_for(base, n):
    """the ray set of a size: unit directions at 1, 64 and 257; at 63 and 65 cast_common's set -- directions that are not unit, `ignore`, tmax at
    and below a hit's t, zero, NaN and infinite rays"""
    sc = pc.scene_of(base)
    return pc.unit_rays(sc, n, seed=n) if n in (1, 64, 257) else cc.make_rays(sc, n, seed=n)[0]


def expected(name):
    """[(n, flags, B, rays, result) ...] of one scene: the host definition over SIZES x B_SET x every flag combination, computed once, shared by
    both builds and by the scene's flavours, never written to"""
    base = name.split("-")[0]
    if base not in _expected:
        a, sc, rows = api_mod(), pc.scene_of(base), []
        for n in SIZES:
            rays = rays_for(base, n)
            for flags in pc.FLAG_COMBOS:
                for B in B_SET:
                    want = a.cast_paths_host(rays, flags, B, sc.spheres, sc.planes, sc.lights)
                    for key in ("hits", "status", "next"):
                        want[key].setflags(write=False)
                    rows.append((n, flags, B, rays, want))
        big = [w for (n, _, B, _, w) in rows if n == 257 and B == 8]
        reasons = np.concatenate([w["reason"] for w in big])
        assert {0, 1, 2} <= set(reasons.tolist()) or base in ("ns257", "small"), (base, set(reasons.tolist()))      # the cases decide something
        assert max(int(w["count"].max()) for w in big) >= 3
        _expected[base] = rows
    return _expected[base]


def took_geometry(r, sc, name):
    grid = r.w.get_grid()
    assert bool(grid and grid["built"]) == (len(sc.spheres) > gridc.GRID_MIN_SPHERES)
    return "grid" if grid and grid["built"] and "linear" not in name else ("lds" if len(sc.spheres) <= gridc.GRID_MIN_SPHERES and "global" not in name else "global")


# ------------------------------------------------------------------ 1. against the definition
@pytest.mark.parametrize("name", list(SCENES))
def test_paths_equal_the_definition(R, api, tex, sky, strict, name):
    base = name.split("-")[0]
    sc, (setup, geometry) = pc.scene_of(base), SCENES[name]
    bad = []
    with rendering(R, sc, tex, sky, 8, 8, setup=setup, cam=None, strict=strict) as r:
        for (n, flags, B, rays, want) in expected(name):
            got = r.w.cast_paths(rays, flags, B)
            assert got is not None and got["hits"].shape == (B, n) and got["hits"].dtype == api.HIT and got["status"].shape == (n,) and got["next"].dtype == api.RAY_QUERY
            d = pc.differing(got, want)
            if any(d):
                bad.append((n, flags, B, d))
        assert took_geometry(r, sc, name) == geometry
    print(f"{name} {'strict' if strict else 'fast'}: {len(expected(name))} cases; (n, flags, B, differing bytes of hits / status / next) {bad[:8]}")
    assert not bad


# ------------------------------------------------------------------ 2. incoherent rays
@pytest.mark.parametrize("name", ["hall", "cloud-grid"])
def test_permuted_rays_give_the_ordered_answer(R, api, tex, sky, strict, name):
    sc = pc.scene_of(name.split("-")[0])
    rays = pc.unit_rays(sc, 1031, seed=3)
    perm = np.random.default_rng(11).permutation(rays.size)
    with rendering(R, sc, tex, sky, 8, 8, cam=None, strict=strict) as r:
        for flags in (pc.SPL, pc.SPL | pc.TRANSMIT | pc.ALL_SURFACES):
            want = api.cast_paths_host(rays, flags, 8, sc.spheres, sc.planes, sc.lights)
            ordered = r.w.cast_paths(rays, flags, 8)
            mixed = r.w.cast_paths(rays[perm], flags, 8)
            back = {"hits": np.empty_like(mixed["hits"]), "status": np.empty_like(mixed["status"]), "next": np.empty_like(mixed["next"])}
            back["hits"][:, perm], back["status"][perm], back["next"][perm] = mixed["hits"], mixed["status"], mixed["next"]
            assert pc.differing(ordered, want) == (0, 0, 0) and pc.differing(back, ordered) == (0, 0, 0)
            assert len(set(want["count"].tolist())) >= 4                              # neighbours in a wave go different ways


# ------------------------------------------------------------------ 3. the device path
@pytest.mark.parametrize("name", ["hall", "cloud-grid"])
def test_device_path_equals_the_host_array_call(R, api, tex, sky, strict, name):
    import torch
    sc = pc.scene_of(name.split("-")[0])
    with rendering(R, sc, tex, sky, 8, 8, cam=None, strict=strict) as r:
        for B, flags in ((2, pc.SPL), (8, pc.SPL | pc.TRANSMIT)):
            n, _, _, rays, want = [e for e in expected(name) if e[0] == 257 and e[1] == flags and e[2] == B][0]
            host = r.w.cast_paths(rays, flags, B)
            d_rays = torch.from_numpy(np.frombuffer(rays.tobytes(), np.uint8).copy()).cuda()
            for own_stream in (True, False):
                d_hits = torch.full((B * n * 32,), 0x5A, dtype=torch.uint8, device="cuda")
                d_status = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
                d_next = torch.full((n * 32,), 0x5A, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                if own_stream:                                     # the wrapper's stream
                    assert r.cast_paths_device(d_rays.data_ptr(), n, d_hits.data_ptr(), d_status.data_ptr(), d_next.data_ptr(), bounces=B,
                                               transmit=bool(flags & pc.TRANSMIT)) == n
                    r.w.sync()
                else:                                              # torch's current stream, after set_stream: launched behind work that
                    stream = torch.cuda.Stream()                   # is still running there, and the call comes back before it has finished
                    with torch.cuda.stream(stream):
                        r.w.set_stream(torch.cuda.current_stream().cuda_stream)
                        torch.cuda._sleep(4_000_000)
                        assert r.w.cast_paths_device(d_rays.data_ptr(), n, flags, B, d_hits.data_ptr(), d_status.data_ptr(), d_next.data_ptr()) == n
                        pending = not stream.query()
                        early = (d_hits.cpu(), d_status.cpu(), d_next.cpu())          # (ordered behind the launch on that stream)
                    stream.synchronize()
                    assert pending, "clw_ext_cast_paths_device waited for the stream"
                torch.cuda.synchronize()
                got = {"hits": d_hits.cpu().numpy(), "status": d_status.cpu().numpy(), "next": d_next.cpu().numpy()}
                d = (pc.differing(got, host), pc.differing(got, want))
                print(f"{name} {'strict' if strict else 'fast'} B {B} {'wrapper stream' if own_stream else 'torch stream'}: differing bytes {d[0]} from the host-array call, {d[1]} from the definition")
                assert d == ((0, 0, 0), (0, 0, 0))
                if not own_stream:
                    assert all(e.numpy().tobytes() == want[k].tobytes() for e, k in zip(early, ("hits", "status", "next")))
            r.w.set_stream(0)
            # without `next`: nothing is written there, the rest is the same
            d_hits = torch.full((B * n * 32,), 0x5A, dtype=torch.uint8, device="cuda")
            d_status = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert r.w.cast_paths_device(d_rays.data_ptr(), n, flags, B, d_hits.data_ptr(), d_status.data_ptr(), None) == n
            r.w.sync()
            assert d_hits.cpu().numpy().tobytes() == want["hits"].tobytes() and d_status.cpu().numpy().tobytes() == want["status"].tobytes()


# ------------------------------------------------------------------ 4. the pick along a path
@pytest.mark.parametrize("model", MODELS)
def test_pick_path_starts_with_the_pick(R, api, demo_scene, tex, sky, strict, model):
    W, H = FRAMES[1]
    cam, proj = view(model, W, H)
    rays = api.camera_rays_host(cam, proj)
    sc = demo_scene
    want = api.cast_paths_host(rays, pc.SPL, 4, sc.spheres, sc.planes, sc.lights)
    through = api.cast_paths_host(rays, pc.SPL | pc.TRANSMIT, 4, sc.spheres, sc.planes, sc.lights)
    kind0 = want["id"][0] >> 30
    pixels = [int(np.flatnonzero(kind0 == k)[len(np.flatnonzero(kind0 == k)) // 2]) for k in (0, 1)]      # one on a sphere, one on a plane
    pixels.append(int(np.flatnonzero(want["count"] == want["count"].max())[0]))                            # ... and the longest path
    with rendering(R, sc, tex, sky, W, H, cam=None, strict=strict) as r:
        assert r.pick_path(3, 3) is None                                     # no camera latched yet
        look_through(r, cam, proj)
        for p in pixels:
            x, y = p % W, p // W
            first = r.pick(x, y)
            for B, transmit, host in ((1, False, want), (4, False, want), (4, True, through)):
                path = r.pick_path(x, y, B, transmit)
                count = min(int(host["count"][p]), B)
                assert path is not None and len(path) == count >= 1
                assert [e["id"] for e in path] == [int(i) for i in host["id"][:count, p]]
                assert [bits(e["depth"])[()] for e in path] == [bits(t)[()] for t in host["t"][:count, p]]
                assert all(e["kind"] == e["id"] >> 30 and e["index"] == e["id"] & 0x3FFFFFFF for e in path)
                e = path[0]
                assert e["id"] == first["id"] and bits(e["depth"]) == bits(first["depth"]), (model, x, y)
                assert np.array_equal(bits(e["point"]), bits(first["point"])) and np.array_equal(bits(e["normal"]), bits(first["normal"])), (model, x, y)
            got = r.w.pick_path(x, y, 4, pc.SPL | pc.TRANSMIT)
            assert got[0].tobytes() == through["hits"][:, p].tobytes() and got[1] == int(through["status"][p])
        assert r.w.pick_path(W, 0, 4, pc.SPL) is None and r.w.pick_path(0, H, 4, pc.SPL) is None and r.pick_path(W, H) is None
        assert r.w.pick_path(1, 1, 0, pc.SPL) is None and r.w.pick_path(1, 1, 9, pc.SPL) is None and r.w.pick_path(1, 1, 4, 0) is None and r.w.pick_path(1, 1, 4, 64 | 7) is None
    with rendering(R, sc, tex, sky, W, H, cam=None, strict=strict, first_row=8, rows=16) as r:      # a strip picks its own rows only
        look_through(r, cam, proj)
        assert r.pick_path(5, 7) is None and r.pick_path(5, 24) is None          # (the renderer's call latches the camera)
        assert r.w.pick_path(5, 8, 4, pc.SPL)[0].tobytes() == want["hits"][:, 8 * W + 5].tobytes()


def test_a_click_on_a_reflection_names_the_reflected_sphere(R, api, demo_scene, tex, sky, strict):
    """the demo view: a pixel on a sphere in which ANOTHER sphere is reflected, found from the host definition -- pick() names the sphere the
    pixel is on, pick_path() that sphere and then the reflected one"""
    W, H = 160, 120
    cam, proj = view("perspective", W, H)
    sc = demo_scene
    want = api.cast_paths_host(api.camera_rays_host(cam, proj), pc.SPL, 2, sc.spheres, sc.planes, sc.lights)
    id0, id1 = want["id"][0], want["id"][1]
    found = np.flatnonzero((id0 >> 30 == 0) & (id1 >> 30 == 0) & (id0 != id1))
    assert found.size >= 3, "the demo view shows no sphere reflected in another"
    with rendering(R, sc, tex, sky, W, H, cam=None, strict=strict) as r:
        look_through(r, cam, proj)
        for p in found[[0, found.size // 2, -1]]:
            x, y = int(p) % W, int(p) // W
            path = r.pick_path(x, y, 2)
            assert r.pick(x, y)["id"] == int(id0[p]) == path[0]["id"] and path[1]["id"] == int(id1[p]) and path[1]["kind"] == 0
            assert path[1]["index"] != path[0]["index"]


# ------------------------------------------------------------------ 5. refusals: 0, the outputs untouched, and the process goes on
def test_refusals_return_zero_and_the_wrapper_works_on(R, api, tex, sky, strict):
    import torch
    sc = pc.scene_of("hall")
    n, flags, B, rays, want = [e for e in expected("hall") if e[0] == 65 and e[1] == pc.SPL | pc.TRANSMIT and e[2] == 2][0]
    Lib = api.load_library()
    P_ = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rays_c = np.ascontiguousarray(rays)

    def refused(cw):
        oh, os_, on = np.full(n * 8 * 32, 0xA5, np.uint8), np.full(n, 0xA5, np.uint8), np.full(n * 32, 0xA5, np.uint8)
        for kw in (dict(n=0), dict(n=1 << 30), dict(flags=0), dict(flags=8), dict(flags=16), dict(flags=64 | 7), dict(flags=0x80000007), dict(rays=None),
                   dict(hits=None), dict(status=None), dict(B=0), dict(B=9), dict(B=0xFFFFFFFF)):
            assert Lib.clw_ext_cast_paths(C.byref(cw.w), P_(kw.get("rays", rays_c)), kw.get("n", n), kw.get("flags", flags), kw.get("B", B),
                                          None if "hits" in kw else P_(oh), None if "status" in kw else P_(os_), P_(on)) == 0, kw
        assert (oh == 0xA5).all() and (os_ == 0xA5).all() and (on == 0xA5).all()
        d = torch.full((n * 8 * 32 + n + n * 32,), 0xA5, dtype=torch.uint8, device="cuda")
        d_rays = torch.from_numpy(np.frombuffer(rays.tobytes(), np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        dr, dh, ds, dn = d_rays.data_ptr(), d.data_ptr(), d.data_ptr() + n * 8 * 32, d.data_ptr() + n * 8 * 32 + n
        for args in ((0, n, flags, B, dh, ds, dn), (dr, 0, flags, B, dh, ds, dn), (dr, n, 64 | 7, B, dh, ds, dn), (dr, n, 16, B, dh, ds, dn),
                     (dr, n, flags, 0, dh, ds, dn), (dr, n, flags, 9, dh, ds, dn), (dr, n, flags, B, 0, ds, dn), (dr, n, flags, B, dh, 0, dn)):
            assert cw.cast_paths_device(*args) == 0, args
        hit, st = np.full(8 * 32, 0xA5, np.uint8), np.full(1, 0xA5, np.uint8)
        assert Lib.clw_ext_pick_path(C.byref(cw.w), 1, 1, 0, pc.SPL, P_(hit), P_(st)) == 0 and Lib.clw_ext_pick_path(C.byref(cw.w), 1, 1, 4, 64 | 7, P_(hit), P_(st)) == 0
        assert Lib.clw_ext_pick_path(C.byref(cw.w), 1, 1, 4, pc.SPL, None, P_(st)) == 0 and Lib.clw_ext_pick_path(C.byref(cw.w), 1, 1, 4, pc.SPL, P_(hit), None) == 0
        assert (hit == 0xA5).all() and (st == 0xA5).all()
        torch.cuda.synchronize()
        assert (d.cpu().numpy() == 0xA5).all()
        return d_rays, d

    with released(api.ClWrap()) as w:                                            # no scene bound, no camera latched
        w.set_strict(strict)
        d_rays, d = refused(w)
        assert w.cast_paths(rays, flags, B) is None and w.pick_path(0, 0, 4, pc.SPL) is None
        assert w.cast_paths_device(d_rays.data_ptr(), n, flags, B, d.data_ptr(), d.data_ptr() + n * 8 * 32, None) == 0
        torch.cuda.synchronize()
        assert (d.cpu().numpy() == 0xA5).all()
    with rendering(R, sc, tex, sky, 16, 16, depth=4, strict=strict, bands=(2, 1)) as r:      # row bands: no camera rays, so no pick along a path
        frame = r.render()
        assert r.w.pick_path(3, 9, 4, pc.SPL) is None and r.pick_path(3, 9) is None
        assert pc.differing(r.w.cast_paths(rays, flags, B), want) == (0, 0, 0)                  # ... the caller's rays are served all the same
        assert np.array_equal(r.render(), frame)
    with rendering(R, sc, tex, sky, 16, 16, depth=4, strict=strict) as r:
        frame = r.render()
        refused(r.w)
        for call in (lambda: r.cast_paths(rays["origin"], rays["dir"], 4, kinds=()), lambda: r.cast_paths(np.zeros((0, 3)), np.zeros((0, 3))),
                     lambda: r.cast_paths(rays["origin"], rays["dir"], 9), lambda: r.cast_paths(rays["origin"], rays["dir"], 0)):
            with pytest.raises(RuntimeError):
                call()
        assert pc.differing(r.w.cast_paths(rays, flags, B), want) == (0, 0, 0)      # ... and the wrapper works behind them
        assert r.pick_path(3, 9) is not None
        assert np.array_equal(r.render(), frame)


# ------------------------------------------------------------------ 6. nothing else moves; the timing id counts the launches
def test_paths_leave_everything_else_alone(R, api, demo_scene, tex, sky, strict):
    W = H = 16
    rays = pc.unit_rays(demo_scene, 193, 5)
    state = {}
    for with_paths in (False, True):
        with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict, accumulate=4) as r:
            first = r.render()
            g = r.gbuffer()
            ao = r.ambient_occlusion(8, 1.0)
            counts = r.ao_counts().copy()
            picked = r.pick(5, 9)["id"]
            overlay = r.highlight([picked])
            table = r.objects()
            layers = r.layers(4)
            flags_before = r.w.last_trace_flags()
            if with_paths:
                got = r.cast_paths(rays["origin"], rays["dir"], 8, transmit=True, tmax=rays["tmax"], ignore=rays["ignore"])
                want = api.cast_paths_host(rays, pc.SPL | pc.TRANSMIT, 8, demo_scene.spheres, demo_scene.planes, demo_scene.lights)
                assert pc.differing(got, want) == (0, 0, 0)
                assert got["t"].shape == got["id"].shape == (8, 193) and got["point"].shape == got["normal"].shape == (8, 193, 3)
                assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["reason"], want["reason"])
                assert len(r.pick_path(5, 9)) >= 1
                for name, (bit, _, _) in api.GB_CHANNELS.items():
                    assert np.array_equal(bits(r.w.read_gbuffer(bit)) if name != "id" else r.w.read_gbuffer(bit), bits(g[name]) if name != "id" else g[name]), name
                assert np.array_equal(r.w.read_ao(api.AO_FRAME).reshape(H, W), ao) and np.array_equal(r.ao_counts(), counts)
                assert np.array_equal(r.w.read_overlay(), overlay) and r.objects().tobytes() == table.tobytes()
                assert r.w.read_layers(api.LAYERS_T).tobytes() == layers["t"].tobytes() and r.w.read_layers(api.LAYERS_ID).tobytes() == layers["id"].tobytes()
                assert r.w.last_trace_flags() == flags_before and r.accumulated == 1
                assert np.array_equal(read_framebuffer(r), first)
            second = r.render_rgb()
            state[with_paths] = (first, second[0], second[1], r.accumulated, r.w.read_tile_order())
    a, b = state[False], state[True]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2]))
    assert a[3] == b[3] == 2 and np.array_equal(a[4][0], b[4][0]) and a[4][1] == b[4][1]


def test_the_timing_id_counts_the_launches(R, api, demo_scene, tex, sky, strict):
    import torch
    rays = pc.unit_rays(demo_scene, 193, 5)
    with rendering(R, demo_scene, tex, sky, 64, 40, depth=4, strict=strict) as r:
        r.render()
        r.w.timing_reset()
        r.w.cast_rays(rays, cc.KINDS)
        r.w.cast_layers(rays, cc.KINDS, 4)
        for B in B_SET:
            assert r.w.cast_paths(rays, pc.SPL, B) is not None                    # 3 launches
        d_rays = torch.from_numpy(np.frombuffer(rays.tobytes(), np.uint8).copy()).cuda()
        d_hits = torch.empty(2 * 193 * 32, dtype=torch.uint8, device="cuda")
        d_status = torch.empty(193, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert r.w.cast_paths_device(d_rays.data_ptr(), 193, pc.SPL, 2, d_hits.data_ptr(), d_status.data_ptr(), None) == 193      # 1 launch
        r.w.sync()
        assert r.w.pick_path(3, 3, 8, pc.SPL) is not None                        # a pick is not logged, as clw_ext_pick's is not
        assert r.w.cast_paths(rays, 0, 4) is None and r.w.cast_paths(rays, pc.SPL, 9) is None      # a refused call launches nothing
        n_paths, ms_paths = r.w.timing_get(api.TIMING_PATHS)
        assert n_paths == 4 and ms_paths > 0
        # the parent's ids count what they counted
        assert r.w.timing_get(api.TIMING_CAST)[0] == 1 and r.w.timing_get(api.TIMING_LAYERS)[0] == 1 and r.w.timing_get(api.TIMING_CAMRAYS)[0] == 0
