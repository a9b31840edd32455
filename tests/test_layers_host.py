"""The layered ray queries on the CPU (include/hip_wrap_ext.h: clw_host_cast_layers, clw_host_camera_rays; csrc/layers_host.c): the C ABI against
the header and the ctypes mirror, every refusal, the host definition against the numpy restatement of tests/layers_common.py -- bit for bit, no
tolerance anywhere --, layer 0 against clw_host_cast_rays, the prefix property, the camera rays against the repacked projection records, and
the sanitizer build of the definition on degenerate rays (tools/layers_sanitize.c, a child process)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cast_common as cc
import layers_common as lc
from conftest import ROOT
from example_gui_opencl_raytracer_amd import api
from render_common import header_text

F = np.float32
NEW_SYMBOLS = ["clw_host_cast_layers", "clw_host_camera_rays", "clw_ext_cast_layers", "clw_ext_cast_layers_device", "clw_ext_camera_rays",
               "clw_ext_camera_rays_device", "clw_ext_render_layers", "clw_ext_read_layers", "clw_ext_layers_device_ptr", "clw_ext_pick_layers"]
SEED = 7
HOST_SCENES = ("small", "stack", "ns257", "cloud")
_cases = {}


# ------------------------------------------------------------------ 1. header, library and mirror
def test_header_library_and_mirror_agree():
    code = header_text(comments=False)
    L = api.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), f"hip_wrap_ext.h does not declare {name}"
        assert name in api.SYMBOLS
        assert hasattr(L, name), f"the library does not export {name}"
        assert getattr(L, name).argtypes is not None
    assert L.clw_host_cast_layers.restype is C.c_int and L.clw_host_camera_rays.restype is C.c_int and L.clw_ext_pick_layers.restype is C.c_int
    assert L.clw_ext_cast_layers.restype is C.c_uint32 and L.clw_ext_render_layers.restype is C.c_uint32 and L.clw_ext_layers_device_ptr.restype is C.c_void_p
    m = re.search(r"typedef struct clw_layer \{(.*?)\} clw_layer;", code, flags=re.S)
    assert m, "hip_wrap_ext.h does not define clw_layer"
    declared = [decl.split()[-1] for decl in m.group(1).split(";") if decl.strip()]
    assert declared == ["t", "id"] == [f[0] for f in api.clw_layer._fields_] == list(api.LAYER.names)
    assert C.sizeof(api.clw_layer) == 8 == api.LAYER.itemsize
    assert (api.clw_layer.t.offset, api.clw_layer.id.offset) == (0, 4) == (api.LAYER.fields["t"][1], api.LAYER.fields["id"][1])
    defs = dict(re.findall(r"#define\s+(CLW_\w+)\s+(0x[0-9A-Fa-f]+|\d+)u\b", header_text()))
    assert int(defs["CLW_TIMING_LAYERS"], 0) == api.TIMING_LAYERS == 0x4C415952 and int(defs["CLW_TIMING_CAMRAYS"], 0) == api.TIMING_CAMRAYS == 0x43524159
    assert api.LAYERS_MAX == lc.K_MAX == 8 and (api.LAYERS_T, api.LAYERS_ID) == (0, 1)
    text = header_text()
    for word in ("LISTED iff additionally t < +inf", "planar, layer-major", "t[k * n + i]", "asks for K + 1", "K == 0 or K > 8", "exits", "X-ray outline",
                 "a total candidate count", "through-selection", "per-ray flags"):
        assert word in text, word
    from example_gui_opencl_raytracer_amd.renderer import Renderer
    for name in ("cast_layers", "cast_layers_device", "camera_rays", "layers", "pick_through"):
        assert callable(getattr(Renderer, name))
    for name in ("cast_layers", "cast_layers_device", "camera_rays", "camera_rays_device", "render_layers", "read_layers", "layers_device_ptr", "pick_layers"):
        assert callable(getattr(api.ClWrap, name))


# ------------------------------------------------------------------ 2. refusals: 0, nothing written
def test_every_refusal():
    L = api.load_library()
    sc = cc.scene_of("small")
    rays = np.ascontiguousarray(cc.make_rays(sc, 12, 1)[0])
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(rays=rays, n=12, flags=3, K=3, sp=sc.spheres, ns=4, pl=sc.planes, npl=2, li=sc.lights, nl=3, t=True, ids=True):
        ot, oi = np.full(12 * 8 * 4, 0xA5, np.uint8), np.full(12 * 8 * 4, 0xA5, np.uint8)
        r = L.clw_host_cast_layers(P(rays), n, flags, K, P(sp), ns, P(pl), npl, P(li), nl, P(ot) if t else None, P(oi) if ids else None)
        assert r == 1 or ((ot == 0xA5).all() and (oi == 0xA5).all())
        if r == 1:                                                  # exactly K * n words of each are written
            assert (ot[4 * K * n:] == 0xA5).all() and (oi[4 * K * n:] == 0xA5).all()
        return r

    assert call() == 1 and call(flags=15) == 1 and call(n=1) == 1 and call(K=1) == 1 and call(K=8) == 1
    assert call(sp=None, ns=0) == 1 and call(pl=None, npl=0) == 1 and call(li=None, nl=0) == 1
    for kw in (dict(rays=None), dict(t=False), dict(ids=False), dict(sp=None), dict(pl=None), dict(li=None), dict(n=0), dict(n=1 << 30),
               dict(n=0xFFFFFFFF), dict(flags=0), dict(flags=8), dict(flags=16 | 3), dict(flags=0x80000001), dict(K=0), dict(K=9), dict(K=0xFFFFFFFF)):
        assert call(**kw) == 0, kw
    for K in (0, 9):
        with pytest.raises(ValueError):
            api.cast_layers_host(rays, 3, K, sc.spheres, sc.planes, sc.lights)
    with pytest.raises(ValueError):
        api.cast_layers_host(rays[:0], 3, 2, sc.spheres, sc.planes, sc.lights)
    # the camera rays refuse what clw_host_projection_rays refuses
    cam = api.perspective((0, 1, -5), (0, 0, 1), 90.0, 1.0, 9, 7)
    out = np.zeros(63, api.RAY_QUERY)
    out.view(np.uint8)[:] = 0xA5
    for proj, b, e in ((api.projection(3), 0, 63), (api.projection(api.PROJ_EQUIRECT, span=(400, 180)), 0, 63), (api.projection(0), 5, 4),
                       (api.projection(0), 0, 64), (api.projection(api.PROJ_ORTHO, axis=(np.nan, 0, 0)), 0, 63)):
        assert L.clw_host_camera_rays(C.byref(cam), C.byref(proj), b, e, P(out)) == 0
        assert L.clw_host_projection_rays(C.byref(cam), C.byref(proj), b, e, P(np.zeros((64, 16), F))) == 0
    assert L.clw_host_camera_rays(C.byref(cam), C.byref(api.projection(0)), 0, 63, None) == 0
    assert (out.view(np.uint8) == 0xA5).all()
    with pytest.raises(ValueError):
        api.camera_rays_host(cam, api.projection(3))


# ------------------------------------------------------------------ 3. the C definition equals the numpy model
def case(name, kinds, opaque):
    """(rays, sorted t, sorted id, count, spread) of one scene and flag word at cast_common.N_HOST rays: the model, computed once, never written to"""
    key = (name, kinds, opaque)
    if key not in _cases:
        sc, flags = lc.scene_of(name), kinds | opaque
        rays = lc.rays_for(name, cc.N_HOST, SEED)
        t, ids, count = lc.candidates(rays, flags, sc.spheres, sc.planes, sc.lights)
        for a in (t, ids, count):
            a.setflags(write=False)
        _cases[key] = (rays, t, ids, count, lc.spread(sc, rays, flags, count, t, ids))
    return _cases[key]


@pytest.mark.parametrize("K", lc.K_ALL)
@pytest.mark.parametrize("name", HOST_SCENES)
def test_the_definition_equals_the_numpy_model(name, K):
    sc = lc.scene_of(name)
    lc.assert_decides(name, K, [case(name, kinds, 0)[4] for kinds in cc.KIND_COMBOS], [case(name, kinds, cc.OPAQUE)[4] for kinds in cc.KIND_COMBOS])
    bad = []
    for kinds in cc.KIND_COMBOS:
        for opaque in (0, cc.OPAQUE):
            rays, t, ids, count, _ = case(name, kinds, opaque)
            want = lc.layers_of(t, ids, K)
            got = api.cast_layers_host(rays, kinds | opaque, K, sc.spheres, sc.planes, sc.lights)
            assert got["t"].shape == got["id"].shape == (K, cc.N_HOST) and got["t"].dtype == F and got["id"].dtype == np.uint32
            d = int((got["t"].view(np.uint32) != want["t"].view(np.uint32)).sum() + (got["id"] != want["id"]).sum())
            if d:
                bad.append((kinds, opaque, d))
            # a primitive appears at most once, the keys ascend strictly, and the empty entries follow the listed ones
            listed = got["id"] != cc.ID_NONE
            assert (np.isinf(got["t"]) == ~listed).all() and (listed[1:] <= listed[:-1]).all()
            after = (got["t"][1:] > got["t"][:-1]) | ((got["t"][1:] == got["t"][:-1]) & (got["id"][1:] > got["id"][:-1]))
            assert after[listed[1:]].all()
    print(f"{name} K {K}: 14 flag words x {cc.N_HOST} rays, most candidates on a ray {max(case(name, k, 0)[4]['most'] for k in cc.KIND_COMBOS)}, differing words {bad}")
    assert not bad


@pytest.mark.parametrize("name", HOST_SCENES)
def test_layer_0_is_the_nearest_hit_and_the_layers_are_prefixes(name):
    sc = lc.scene_of(name)
    for kinds in cc.KIND_COMBOS:
        for opaque in (0, cc.OPAQUE):
            rays, flags = case(name, kinds, opaque)[0], kinds | opaque
            hits = api.cast_rays_host(rays, flags, sc.spheres, sc.planes, sc.lights)
            full = api.cast_layers_host(rays, flags, lc.K_MAX, sc.spheres, sc.planes, sc.lights)
            finite = np.isfinite(hits["t"])
            assert finite.any() and (~finite).any()
            assert np.array_equal(full["t"][0][finite].view(np.uint32), hits["t"][finite].view(np.uint32)) and np.array_equal(full["id"][0][finite], hits["id"][finite])
            assert (full["id"][0][~finite] == cc.ID_NONE).all() and np.isinf(full["t"][0][~finite]).all()
            for K in lc.K_ALL[:-1]:
                part = api.cast_layers_host(rays, flags, K, sc.spheres, sc.planes, sc.lights)
                assert part["t"].tobytes() == full["t"][:K].tobytes() and part["id"].tobytes() == full["id"][:K].tobytes(), (kinds, opaque, K)


def test_closed_forms():
    sc = lc.scene_of("stack")
    assert len(sc.spheres) == 12 and len(sc.planes) == 2 and len(sc.lights) == 3 and sc.spheres["material"]["transperent"].tolist() == [0] * 5 + [1] + [0] * 6
    # along the line from x = -6: plane 0 at 3, then every sphere's near side at 2 i + 5.5, the pair 3 / 7 at one t, light 1 at 20.75, plane 1 at 31
    rays = api.make_rays([(-6.0, 1.0, 0.0)], [(1.0, 0.0, 0.0)])
    got = api.cast_layers_host(rays, cc.KINDS, 8, sc.spheres, sc.planes, sc.lights)
    assert got["id"][:, 0].tolist() == [cc.KIND_PLANE, 0, 1, 2, 3, 7, 4, 5]
    assert got["t"][:, 0].tolist() == [3.0] + [5.5 + 2 * i for i in (0, 1, 2, 3, 3, 4, 5)]
    opaque = api.cast_layers_host(rays, cc.SPHERES | cc.OPAQUE, 8, sc.spheres, None, None)
    assert opaque["id"][:, 0].tolist() == [0, 1, 2, 3, 7, 4, 6, 8]                       # the glass sphere 5 lets the ray pass
    ignoring = api.cast_layers_host(api.make_rays([(-6.0, 1.0, 0.0)], [(1.0, 0.0, 0.0)], ignore=3), cc.SPHERES, 5, sc.spheres, None, None)
    assert ignoring["id"][:, 0].tolist() == [0, 1, 2, 7, 4]                             # ... and with 3 ignored its twin stays, once
    # twice the direction, half the t; tmax ends the list; from inside sphere 2 its far side is its one entry
    half = api.cast_layers_host(api.make_rays([(-6.0, 1.0, 0.0)], [(2.0, 0.0, 0.0)], tmax=4.0), cc.KINDS, 8, sc.spheres, sc.planes, sc.lights)
    assert half["id"][:, 0].tolist() == [cc.KIND_PLANE, 0, 1, cc.ID_NONE, cc.ID_NONE, cc.ID_NONE, cc.ID_NONE, cc.ID_NONE] and half["t"][0, 0] == 1.5
    inside = api.cast_layers_host(api.make_rays([(4.0, 1.0, 0.0)], [(1.0, 0.0, 0.0)]), cc.SPHERES, 2, sc.spheres, None, None)
    assert inside["id"][:, 0].tolist() == [2, 3] and inside["t"][:, 0].tolist() == [0.5, 1.5]
    # a candidate at t = +inf is not listed, though the any-hit query counts it
    floor = sc.planes[:1].copy()
    floor["normal"], floor["point_in_plane"] = (0.0, 1.0, 0.0), (0.0, -3e38, 0.0)
    far = api.make_rays([(0.0, 3e38, 0.0)], [(0.0, -1.0, 0.0)])
    assert api.occluded_rays_host(far, cc.PLANES, None, floor, None)[0] == 1
    assert api.cast_layers_host(far, cc.PLANES, 1, None, floor, None)["id"][0, 0] == cc.ID_NONE


# ------------------------------------------------------------------ 4. the camera rays
@pytest.mark.parametrize("model", ["perspective", "ortho", "equirect"])
def test_camera_rays_are_the_repacked_projection_records(model):
    W, H = 61, 43
    if model == "ortho":
        cam, proj = api.ortho_camera((0.0, 4.0, -6.0), (0.0, -0.2, 1.0), 12.0, W, H)
    else:
        cam = api.perspective((0.0, 4.0, -6.0), (0.0, -0.2, 1.0), 80.0, 1.0, W, H)
        proj = api.projection(model, axis=(0.0, 0.0, 1.0) if model == "equirect" else None)
    for b, e in ((0, W * H), (3 * W, 11 * W), (W + 5, W + 6), (7, 7)):
        rec = api.projection_rays(cam, proj, b, e)
        got = api.camera_rays_host(cam, proj, b, e)
        assert got.dtype == api.RAY_QUERY and got.size == e - b
        assert np.array_equal(got["origin"].view(np.uint32), rec[:, 0:3].view(np.uint32)) and np.array_equal(got["dir"].view(np.uint32), rec[:, 4:7].view(np.uint32))
        assert np.isposinf(got["tmax"]).all() and (got["ignore"] == cc.ID_NONE).all()
    whole = api.camera_rays_host(cam, proj)
    assert whole[3 * W:11 * W].tobytes() == api.camera_rays_host(cam, proj, 3 * W, 11 * W).tobytes()
    assert np.isfinite(whole["dir"]).all() and (len(np.unique(whole["dir"], axis=0)) > 1) == (model != "ortho")
    if model == "perspective":
        assert whole.tobytes() == api.camera_rays_host(cam).tobytes()              # no projection = the pinhole


# ------------------------------------------------------------------ 5. the definition under the sanitizers
def test_the_definition_under_the_sanitizers(tmp_path):
    """tools/layers_sanitize.c: csrc/layers_host.c built with -fsanitize=address,undefined as a stand-alone program, run as a child process on
    degenerate rays (host code only)"""
    cc_ = shutil.which(os.environ.get("CC") or "gcc")
    assert cc_, "no C compiler"
    csrc = os.path.join(ROOT, "example_gui_opencl_raytracer_amd", "csrc")
    exe = str(tmp_path / "layers_sanitize")
    cmd = [cc_, "-O1", "-g", "-std=c99", "-ffp-contract=off", "-D_DEFAULT_SOURCE", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I", csrc, os.path.join(ROOT, "tools", "layers_sanitize.c")] + [os.path.join(csrc, f) for f in ("layers_host.c", "cast_host.c", "projection_host.c", "host_camera.c", "scene_prep.c")] + ["-lm", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "0 failures" in p.stdout
