"""Ray queries on the GPU (include/hip_wrap_ext.h: clw_ext_cast_rays, clw_ext_occluded_rays, clw_ext_cast_rays_device; csrc/whitted_cast.inc)
against the host definition (csrc/cast_host.c: clw_host_cast_rays, clw_host_occluded_rays) -- bit for bit, in both builds, no tolerance
anywhere.  The scenes reach each geometry source of wt_cast (staged in LDS, read from global memory, walked through the uniform grid); the ray
sets are those of tests/cast_common.py."""
import numpy as np
import pytest

import cast_common as cc
import grid_common as gridc
from conftest import CAM
from render_common import R, api, bits, released, rendering  # noqa: F401  (R, api: the fixtures)

pytestmark = pytest.mark.gpu

WT_V_GEOM_GLOBAL = 1                     # csrc/launch_plan.h: geometry read from global memory although it would fit LDS
SIZES = (1, 63, 64, 65, 193, 4099)      # one lane, a ragged wave, a whole one, one and a lane, several workgroups, many with a ragged tail
S, P, L, O = cc.SPHERES, cc.PLANES, cc.LIGHTS, cc.OPAQUE
FLAG_SETS = {"planes": (P, P | L), "spheres": (S | O, S | L), "small": (S | P, S | P | L | O), "ns257": (S | P, S | P | L), "cloud": (S | P | O, S | P | L)}
# the grid layouts of fuzz_scenes.grid_layout but `offset` (make_rays draws origins up to three times the scene's bounds away: thousands of units
# from the spheres, outside the domain where the float sphere test decides)
FLAG_SETS.update({name: (S | P, S | P | L | O) for name in cc.GRID_SCENES})
# name -> (setup of the wrapper, the geometry the pass must take: "lds" | "global" | "grid")
UNIT_SCENES = {
    "planes": (None, "lds"),
    "spheres": (None, "lds"),
    "small": (None, "lds"),
    "small-global": (lambda w: w.set_variant(WT_V_GEOM_GLOBAL), "global"),
    "ns257-grid": (None, "grid"),
    "ns257-linear": (lambda w: w.set_grid(0), "global"),
    "cloud-grid": (None, "grid"),
    "cloud-linear": (lambda w: w.set_grid(0), "global"),
}
for _name in cc.GRID_SCENES:             # each walked and scanned: grid == linear == the definition
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
    """[(n, flags, rays, hits, blocked) ...] of one scene: the host definition, computed once, shared by both builds and by the scene's grid and
    linear flavours, never written to; the union of a flag set's cases decides something (cast_common.assert_decides) and holds unwalkable rays"""
    base = name.split("-")[0]
    if base not in _expected:
        a, sc, rows = api_mod(), cc.scene_of(base), []
        for flags in FLAG_SETS[base]:
            mine = []
            for n in SIZES:
                rays, info = cc.make_rays(sc, n, seed=n)
                hits = a.cast_rays_host(rays, flags, sc.spheres, sc.planes, sc.lights)
                blocked = a.occluded_rays_host(rays, flags, sc.spheres, sc.planes, sc.lights)
                hits.setflags(write=False)
                blocked.setflags(write=False)
                mine.append((n, flags, rays, hits, blocked))
                if n >= 193:
                    odd = rays[info["odd"]]
                    assert (odd["dir"] == 0).all(1).any() and np.isnan(odd["origin"]).any() and np.isinf(odd["dir"]).any()      # the unwalkable ones
            cc.assert_decides(sc, np.concatenate([m[2] for m in mine]), flags, np.concatenate([m[3] for m in mine]), f"{base} flags {flags}")
            rows += mine
        _expected[base] = rows
    return _expected[base]


def differing(got, want):
    return int((np.ascontiguousarray(got).view(np.uint8) != np.ascontiguousarray(want).view(np.uint8)).sum())


# ------------------------------------------------------------------ 1. against the definition
@pytest.mark.parametrize("name", list(UNIT_SCENES))
def test_casts_equal_the_definition(R, api, tex, sky, strict, name):
    sc, (setup, geometry) = cc.scene_of(name.split("-")[0]), UNIT_SCENES[name]
    bad = []
    with rendering(R, sc, tex, sky, 8, 8, setup=setup, cam=None, strict=strict) as r:
        for (n, flags, rays, hits, blocked) in expected(name):
            got = r.w.cast_rays(rays, flags)
            got_blocked = r.w.occluded_rays(rays, flags)
            assert got is not None and got.shape == hits.shape and got.dtype == api.HIT
            assert got_blocked is not None and got_blocked.shape == blocked.shape and got_blocked.dtype == np.uint8
            d = (differing(got, hits), differing(got_blocked, blocked))
            if any(d):
                bad.append((n, flags) + d)
        grid = r.w.get_grid()
        assert bool(grid and grid["built"]) == (len(sc.spheres) > gridc.GRID_MIN_SPHERES)
        # the geometry the pass took: the grid when one is built and on, LDS for a small scene unless the variant says global
        took = "grid" if grid and grid["built"] and "linear" not in name else ("lds" if len(sc.spheres) <= gridc.GRID_MIN_SPHERES and "global" not in name else "global")
        assert took == geometry
    print(f"{name} {'strict' if strict else 'fast'}: {len(expected(name))} cases x nearest and any, differing bytes {sum(b[2] + b[3] for b in bad)} {bad[:8]}")
    assert not bad


# ------------------------------------------------------------------ 1b. an equal t met from two cells of the grid
TANGENT_FLAGS = (S, S | P, S | P | L, S | O, S | P | L | O)
_tangent = {}


def tangent_expected(name):
    """(rays, where the exact rays sit, {flags: (hits, blocked)}) of a variant of the tangent scene: the host definition, computed once"""
    if name not in _tangent:
        a, sc = api_mod(), cc.scene_of(name)
        rays, where = cc.tangent_rays(name, seed=193)
        want = {}
        for flags in TANGENT_FLAGS:
            hits = a.cast_rays_host(rays, flags, sc.spheres, sc.planes, sc.lights)
            blocked = a.occluded_rays_host(rays, flags, sc.spheres, sc.planes, sc.lights)
            hits.setflags(write=False)
            blocked.setflags(write=False)
            want[flags] = (hits, blocked)
        _tangent[name] = (rays, where, want)
    return _tangent[name]


def assert_tangent_premise(name, grid):
    """the pass took the grid, and on the grid of ITS pad the exact ray along x is in cells that list B alone before the cell that lists both.
    The wrapper reports the pad the builder derived (scene_prep.c: wprep_grid_plan widens the one it is asked for), so the host builder is
    asked for the pad the shim asks for -- the largest light radius of a paired walk, else none -- and must arrive at the reported one."""
    assert grid and grid["built"], name
    asked = float(np.abs(cc.scene_of(name).lights["radius"]).max()) if grid["pair"] else 0.0
    cells, G = cc.tangent_cells(name, asked)
    assert G["reg_pad"] == grid["reg_pad"] and (grid["reg_pad"] > 0) == bool(grid["pair"])
    assert tuple(G["res"].tolist()) == grid["res"] and G["pairs"] == grid["pairs"], (G["res"], grid["res"], G["pairs"], grid["pairs"])
    assert np.array_equal(bits(G["cell"]), bits(grid["cell"])) and np.array_equal(bits(G["gmin"]), bits(grid["gmin"]))
    assert len(cells[0][0]) >= 2 and all(both for _, both in cells), (name, cells)


@pytest.mark.parametrize("name", list(cc.TANGENT_VARIANTS))
def test_an_equal_t_across_cells_keeps_the_lower_index(R, api, tex, sky, strict, name):
    """wt_query_grid presents a cell's spheres in cell order and the cells in ray order, so the nearest sink meets the large sphere B, listed
    in every cell, before the small sphere A at the same t: with A at the lower index the sink's rule for an equal t from a lower index
    (wt_sink_nearest::grid_take) decides the id, with the indices swapped the rule must NOT fire.  The premise is asserted on the CPU
    (test_cast_host.py: test_the_tangent_pair_ties_across_cells) and again here for the pad the wrapper reports."""
    sc = cc.scene_of(name)
    a, b = cc.tangent_ids(name)
    rays, where, want = tangent_expected(name)
    plain = want[S | P][0][where]
    assert plain["id"][0::5].tolist() == [min(a, b)] * len(cc.TANGENT_EXACT) and plain["id"][1::5].tolist() == [b] * len(cc.TANGENT_EXACT)
    bad = []
    with rendering(R, sc, tex, sky, 8, 8, cam=None, strict=strict) as r:
        for flags, (hits, blocked) in want.items():
            got, got_blocked = r.w.cast_rays(rays, flags), r.w.occluded_rays(rays, flags)
            d = (differing(got, hits), differing(got_blocked, blocked), differing(got[where], hits[where]))
            print(f"{name} {'strict' if strict else 'fast'} flags {flags}: ids of the exact rays {got['id'][where].tolist()}")
            if any(d):
                bad.append((flags,) + d)
        assert_tangent_premise(name, r.w.get_grid())
    with rendering(R, sc, tex, sky, 8, 8, setup=lambda w: w.set_grid(0), cam=None, strict=strict) as r:      # ... and the linear scan agrees
        for flags, (hits, blocked) in want.items():
            if differing(r.w.cast_rays(rays, flags), hits) or differing(r.w.occluded_rays(rays, flags), blocked):
                bad.append((flags, "linear"))
    print(f"{name} {'strict' if strict else 'fast'}: {len(want)} flag sets x nearest and any, (flags, differing bytes: hits, blocked, hits of the exact rays) {bad}")
    assert not bad


# ------------------------------------------------------------------ 2. the device path
@pytest.mark.parametrize("name", ["small", "cloud-grid"])
def test_device_path_equals_the_host_array_calls(R, api, tex, sky, strict, name):
    import torch
    sc = cc.scene_of(name.split("-")[0])
    n, flags, rays, hits, blocked = [e for e in expected(name) if e[0] == 4099][1]
    with rendering(R, sc, tex, sky, 8, 8, cam=None, strict=strict) as r:
        want, want_blocked = r.w.cast_rays(rays, flags), r.w.occluded_rays(rays, flags)
        d_rays = torch.from_numpy(np.frombuffer(rays.tobytes(), np.uint8).copy()).cuda()
        for own_stream in (True, False):
            d_hits = torch.full((n * 32,), 0xA5, dtype=torch.uint8, device="cuda")
            d_blocked = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            if own_stream:                                     # the wrapper's stream
                assert r.w.cast_rays_device(d_rays.data_ptr(), n, flags, hits_ptr=d_hits.data_ptr()) == n
                assert r.cast_rays_device(d_rays.data_ptr(), n, blocked_ptr=d_blocked.data_ptr(), kinds=flags & cc.KINDS, opaque_only=bool(flags & O)) == n
                r.w.sync()
            else:                                              # torch's current stream, after set_stream
                stream = torch.cuda.Stream()
                with torch.cuda.stream(stream):
                    r.w.set_stream(torch.cuda.current_stream().cuda_stream)
                    assert r.w.cast_rays_device(d_rays.data_ptr(), n, flags, hits_ptr=d_hits.data_ptr()) == n
                    assert r.w.cast_rays_device(d_rays.data_ptr(), n, flags, blocked_ptr=d_blocked.data_ptr()) == n
                    got_t, got_b = d_hits.cpu(), d_blocked.cpu()          # (ordered behind the launches on that stream)
                stream.synchronize()
            torch.cuda.synchronize()
            got = d_hits.cpu().numpy().view(api.HIT)
            got_blocked = d_blocked.cpu().numpy()
            print(f"{name} {'strict' if strict else 'fast'} {'wrapper stream' if own_stream else 'torch stream'}: differing bytes "
                  f"{differing(got, want)} hits, {differing(got_blocked, want_blocked)} blocked")
            assert got.tobytes() == want.tobytes() == hits.tobytes() and np.array_equal(got_blocked, want_blocked) and np.array_equal(got_blocked, blocked)
            if not own_stream:
                assert got_t.numpy().tobytes() == want.tobytes() and np.array_equal(got_b.numpy(), want_blocked)
        r.w.set_stream(0)


# ------------------------------------------------------------------ 3. scene changes
def bare_scene_wrapper(api, sc, sph):
    """a wrapper with nothing but the raytracer's arguments 1-6 bound: no camera, no ray buffer, no images, no framebuffer; the sphere array is
    the caller's device tensor `sph`"""
    cw = api.ClWrap()
    cw.bind_device_buffer(1, 1, sph.data_ptr(), sph.numel())
    cw.load_global_data(1, 2, sc.planes)
    cw.load_global_data(1, 3, sc.lights)
    for a, n in ((4, len(sc.spheres)), (5, len(sc.planes)), (6, len(sc.lights))):
        cw.load_single_data(1, a, np.uint32(n))
    return cw


@pytest.mark.parametrize("name", ["small", "ns257-grid"])
def test_a_rewritten_scene_is_seen_after_invalidate(api, strict, name):
    import torch
    from example_gui_opencl_raytracer_amd.scene import Scene
    sc = cc.scene_of(name.split("-")[0])
    n, flags, rays, hits, blocked = [e for e in expected(name) if e[0] == 193][0]
    sph = torch.from_numpy(np.frombuffer(sc.spheres.tobytes(), np.uint8).copy()).cuda()
    with released(bare_scene_wrapper(api, sc, sph)) as cw:
        cw.set_strict(strict)
        assert cw.cast_rays(rays, flags).tobytes() == hits.tobytes()
        moved = sc.spheres.copy()
        victim = int(np.bincount(hits["id"][hits["id"] >> 30 == 0]).argmax())            # the sphere most rays meet
        moved["origin"][victim] += np.float32([0.75, 0.5, -0.25])
        sph.copy_(torch.from_numpy(np.frombuffer(moved.tobytes(), np.uint8).copy()))
        torch.cuda.synchronize()
        cw.invalidate_scene()
        want = api.cast_rays_host(rays, flags, moved, sc.planes, sc.lights)
        got = cw.cast_rays(rays, flags)
        print(f"{name} {'strict' if strict else 'fast'}: sphere {victim} moved, {int((want['id'] != hits['id']).sum())} rays answer differently, "
              f"{differing(got, want)} bytes differ from the definition")
        assert (want["id"] != hits["id"]).any() and got.tobytes() == want.tobytes()
        assert np.array_equal(cw.occluded_rays(rays, flags), api.occluded_rays_host(rays, flags, moved, sc.planes, sc.lights))
        grid = cw.get_grid()
        assert bool(grid and grid["built"]) == ("grid" in name)


# ------------------------------------------------------------------ 4. nothing else moves
def read_framebuffer(r):
    """the framebuffer as it lies, without tracing: the read-back rides on the raygen launch, which in fused mode only latches the camera"""
    out = np.empty(r.pixels, np.uint32)
    r.w.output(r.pixels, out.nbytes, 0, 1, 10, out)
    return out


def test_a_cast_leaves_everything_else_alone(R, api, demo_scene, tex, sky, strict):
    W = H = 16
    rays = cc.make_rays(demo_scene, 193, 5)[0]
    state = {}
    for with_cast in (False, True):
        with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict, accumulate=4) as r:
            first = r.render()
            g = r.gbuffer()
            ao = r.ambient_occlusion(8, 1.0)
            flags_before = r.w.last_trace_flags()
            if with_cast:
                hits = r.cast_rays(rays["origin"], rays["dir"], rays["tmax"], rays["ignore"], kinds=("sphere", "plane", "light"))
                assert hits.tobytes() == api.cast_rays_host(rays, cc.KINDS, demo_scene.spheres, demo_scene.planes, demo_scene.lights).tobytes()
                assert r.cast_rays(rays["origin"], rays["dir"], any_hit=True).dtype == bool
                for name, (bit, _, _) in api.GB_CHANNELS.items():
                    assert np.array_equal(bits(r.w.read_gbuffer(bit)) if name != "id" else r.w.read_gbuffer(bit), bits(g[name]) if name != "id" else g[name]), name
                assert np.array_equal(r.w.read_ao(api.AO_FRAME).reshape(H, W), ao)
                assert r.w.last_trace_flags() == flags_before and r.accumulated == 1
                assert np.array_equal(read_framebuffer(r), first)
            second = r.render_rgb()
            state[with_cast] = (first, second[0], second[1], r.accumulated, r.w.read_tile_order())
    a, b = state[False], state[True]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2]))
    assert a[3] == b[3] == 2 and np.array_equal(a[4][0], b[4][0]) and a[4][1] == b[4][1]


# ------------------------------------------------------------------ 5. refusals: 0, the outputs untouched, and the process goes on
def test_refusals_return_zero_and_the_wrapper_works_on(R, api, tex, sky, strict):
    import torch
    sc = cc.scene_of("small")
    n, flags, rays, hits, blocked = [e for e in expected("small") if e[0] == 65][0]
    L = api.load_library()
    import ctypes as C
    P_ = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rays_c = np.ascontiguousarray(rays)

    def refused(cw):
        out_h, out_b = np.full(n * 32, 0xA5, np.uint8), np.full(n, 0xA5, np.uint8)
        for kw in (dict(n=0), dict(n=1 << 30), dict(flags=0), dict(flags=O), dict(flags=16 | 3), dict(flags=0x80000003), dict(rays=None), dict(out=None)):
            nn, ff, rr = kw.get("n", n), kw.get("flags", flags), kw.get("rays", rays_c)
            assert L.clw_ext_cast_rays(C.byref(cw.w), P_(rr), nn, ff, None if "out" in kw else P_(out_h)) == 0, kw
            assert L.clw_ext_occluded_rays(C.byref(cw.w), P_(rr), nn, ff, None if "out" in kw else P_(out_b)) == 0, kw
        assert (out_h == 0xA5).all() and (out_b == 0xA5).all()
        d = torch.full((n * 32,), 0xA5, dtype=torch.uint8, device="cuda")
        d_rays = torch.from_numpy(np.frombuffer(rays.tobytes(), np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        assert cw.cast_rays_device(d_rays.data_ptr(), n, flags) == 0                                     # neither output
        assert cw.cast_rays_device(d_rays.data_ptr(), n, flags, d.data_ptr(), d.data_ptr()) == 0          # both
        assert cw.cast_rays_device(0, n, flags, d.data_ptr()) == 0 and cw.cast_rays_device(d_rays.data_ptr(), 0, flags, d.data_ptr()) == 0
        assert cw.cast_rays_device(d_rays.data_ptr(), n, 16 | 3, d.data_ptr()) == 0 and cw.cast_rays_device(d_rays.data_ptr(), n, O, d.data_ptr()) == 0
        torch.cuda.synchronize()
        assert (d.cpu().numpy() == 0xA5).all()
        return d_rays, d

    with released(api.ClWrap()) as w:                                            # no scene bound
        w.set_strict(strict)
        d_rays, d = refused(w)
        assert w.cast_rays(rays, flags) is None and w.occluded_rays(rays, flags) is None
        assert w.cast_rays_device(d_rays.data_ptr(), n, flags, d.data_ptr()) == 0
        torch.cuda.synchronize()
        assert (d.cpu().numpy() == 0xA5).all()
    with rendering(R, sc, tex, sky, 16, 16, depth=4, strict=strict) as r:
        frame = r.render()
        refused(r.w)
        with pytest.raises(RuntimeError):
            r.cast_rays(rays["origin"], rays["dir"], kinds=())
        with pytest.raises(RuntimeError):
            r.cast_rays(np.zeros((0, 3)), np.zeros((0, 3)))
        assert r.w.cast_rays(rays, flags).tobytes() == hits.tobytes()           # ... and the wrapper works behind them
        assert np.array_equal(r.w.occluded_rays(rays, flags), blocked)
        assert np.array_equal(r.render(), frame)


# ------------------------------------------------------------------ 6. the timing log
def test_the_timing_id_counts_the_launches(R, api, demo_scene, tex, sky, strict):
    import torch
    rays = cc.make_rays(demo_scene, 193, 5)[0]
    with rendering(R, demo_scene, tex, sky, 64, 40, depth=4, strict=strict) as r:
        r.render()
        r.w.timing_reset()
        r.gbuffer(api.GB_ID)
        r.ambient_occlusion(4, 1.0)
        r.render()
        for k in range(3):
            r.w.cast_rays(rays, cc.KINDS)
        r.w.occluded_rays(rays, S | P)
        d_rays = torch.from_numpy(np.frombuffer(rays.tobytes(), np.uint8).copy()).cuda()
        d = torch.empty(193, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert r.w.cast_rays_device(d_rays.data_ptr(), 193, S | P, blocked_ptr=d.data_ptr()) == 193
        assert r.w.cast_rays(rays, 0) is None                                     # a refused call launches nothing
        n_cast, ms_cast = r.w.timing_get(api.TIMING_CAST)
        assert n_cast == 5 and ms_cast > 0
        # the parent's ids count what they counted: one id pass and the AO's own, one AO trace, one resolve, no overlay
        assert r.w.timing_get(api.TIMING_GBUFFER)[0] == 2 and r.w.timing_get(api.TIMING_AO)[0] == 1 and r.w.timing_get(api.TIMING_AO_RESOLVE)[0] == 1
        assert r.w.timing_get(api.TIMING_OVERLAY)[0] == 0 and r.w.timing_get(1)[0] == 1


# ------------------------------------------------------------------ 7. Renderer.line_of_sight
def test_line_of_sight(R, api, tex, sky, strict):
    sc = cc.scene_of("small")
    a = np.float32([(-2.5, 1.0, 0.0), (-0.9, 0.4, -2.0), (5.0, 2.0, 5.0), (5.0, 2.0, 5.0), (5.0, 2.0, 5.0)])
    b = np.float32([(2.5, 1.0, 0.0), (-0.9, 0.4, -0.5), (5.0, 0.5, 5.0), (5.0, -0.5, 5.0), (5.0, 0.0, 5.0)])
    assert sc.spheres["material"]["transperent"].tolist() == [0, 0, 1, 0]
    with rendering(R, sc, tex, sky, 8, 8, cam=None, strict=strict) as r:
        opaque = r.line_of_sight(a, b)
        everything = r.line_of_sight(a, b, opaque_only=False)
    assert opaque.dtype == bool and opaque.shape == (5,)
    # either side of the opaque sphere 0: blocked; either side of the glass sphere 2: free for opaque_only, blocked without; a target in front of
    # the floor: free; behind it: blocked
    assert opaque[:4].tolist() == [False, True, True, False] and everything[:4].tolist() == [False, False, True, False]
    # a target exactly on the floor: as the definition decides it
    rays = api.make_rays(a, b - a, tmax=1.0)
    for got, flags in ((opaque, S | P | O), (everything, S | P)):
        assert np.array_equal(got, api.occluded_rays_host(rays, flags, sc.spheres, sc.planes, sc.lights) == 0)


# ------------------------------------------------------------------ 8. more than one batch per wave
@pytest.mark.parametrize("batches", [2, 3])
@pytest.mark.parametrize("name", ["small", "ns257-grid"])
def test_several_batches_per_wave_equal_the_definition(R, api, tex, sky, strict, monkeypatch, name, batches):
    """CLWRAP_CAST_BATCHES (read on every call): a wave serves 2 or 3 batches of 64 rays per staging.  The sizes hold ragged counts, and 193 rays
    under 3 batches leave the second workgroup one valid lane in its first batch and nothing for the others (base >= n)."""
    assert 193 in SIZES and any(n % 64 for n in SIZES)
    monkeypatch.setenv("CLWRAP_CAST_BATCHES", str(batches))
    sc, (setup, geometry) = cc.scene_of(name.split("-")[0]), UNIT_SCENES[name]
    bad = []
    with rendering(R, sc, tex, sky, 8, 8, setup=setup, cam=None, strict=strict) as r:
        for (n, flags, rays, hits, blocked) in expected(name):
            d = (differing(r.w.cast_rays(rays, flags), hits), differing(r.w.occluded_rays(rays, flags), blocked))
            if any(d):
                bad.append((n, flags) + d)
        grid = r.w.get_grid()
        assert bool(grid and grid["built"]) == (geometry == "grid")
    print(f"{name} {'strict' if strict else 'fast'} {batches} batches: {len(expected(name))} cases x nearest and any, differing bytes {bad[:8]}")
    assert not bad
