"""The camera models beside the pinhole on the GPU (include/hip_wrap_ext.h: clw_ext_set_projection; csrc/whitted_projection.inc): the
orthographic view and the equirectangular panorama, through every pass that looks through the camera.

  G1  the generated records (Renderer.read_rays, clw_ext_unit_projection) equal the host definition (api.projection_rays) bit for bit
  G2  strict build: the frame equals oracle.trace_rays on the host definition's records, every pixel
  G3  fast build: the frame equals the frame the same library traces from the same records uploaded as a caller's ray buffer, bit for bit
  G4  strict build: gbuffer() equals the buffers tests/gbuffer_common.py's recipe gives for the host records, every bit; pick() their entries
  G5  fast build: where its id is the expected one, depth, point and normal have the expected bits; a pixel whose id differs lies on an id
      boundary of the expected image and carries a neighbour's id
  G6  objects(), highlight() and select_rect() under the orthographic view equal the host models fed with G4's channels and G2's frame
  G7  setting and clearing a projection leaves the pinhole what it was; a still view generates its records once
  G8  what needs the fused launch is refused naming the projection; the environment variables

No tolerance anywhere: every comparison is on bit patterns.  Expected frames and buffers are computed once per module and shared.

Measured on the MI355X: every case passes with 0 differing words -- records, strict frames (0 of up to 3015 pixels at depth 1 and 5), the 60
fast frames against the uploaded records, the strict buffers (8 distinct ids on the demo scene under both models, 179 on the 324-sphere
scene under the orthographic view), and the fast buffers, in which no id differs from the expected one in any of the six cases (the
boundary rule of G5 was not needed)."""
import os

import numpy as np
import pytest

import flags_common as F
import gbuffer_common as gc
import projection_common as prj
from parity_common import check_exact
from render_common import R, api, bits, released, rendering, run_child  # noqa: F401  (R, api: the fixtures)

pytestmark = pytest.mark.gpu

SCENE_SIZE = {"demo": "67x45", "grid324": "40x24", "glass16": "40x24"}      # the size each scene's inspection passes run at
SIZES = dict(prj.SIZES)
SIZES["40x24"] = (gc.WD, gc.HD, 0, None, None)


@pytest.fixture(scope="module", params=[True, False], ids=["strict", "fast"])
def strict(request):
    import torch  # noqa: F401
    return request.param


_scenes, _views, _frames, _buffers = {}, {}, {}, {}


def scene_of(name):
    if name not in _scenes:
        _scenes[name] = gc._scene(name)
    return _scenes[name]


def view(api, model, size):
    """(camera, projection, host records of the renderer's work-items) of a model at a size: computed once, never written to"""
    if (model, size) not in _views:
        W, H, first_row, rows, bands = SIZES[size]
        cam, proj = prj.view_of(api, model, W, H)
        rays = prj.host_rays(api, cam, proj, W, H, first_row, rows, bands)
        rays.setflags(write=False)
        _views[model, size] = (cam, proj, rays)
    return _views[model, size]


def projected(R, api, scene, tex, sky, model, size, strict, depth=1, **kw):
    """`with projected(...) as r:` -- a renderer of the size's range that looks through the model"""
    W, H, first_row, rows, bands = SIZES[size]
    cam, proj, _ = view(api, model, size)
    return rendering(R, scene_of(scene), tex, sky, W, H, cam=cam, depth=depth, strict=strict, first_row=first_row, rows=rows, bands=bands,
                     projection=proj, **kw)


def expected_frame(oracle, api, scene, tex, sky, model, size, depth):
    key = (scene, model, size, depth)
    if key not in _frames:
        W, H, first_row, _, bands = SIZES[size]
        assert bands is None
        want, _ = oracle.trace_rays(view(api, model, size)[2], scene_of(scene), tex, sky, depth, id_begin=first_row * W)
        want.setflags(write=False)
        _frames[key] = want
    return _frames[key]


def expected_buffers(oracle, api, scene, tex, sky, model):
    key = (scene, model)
    if key not in _buffers:
        _buffers[key] = prj.expected_gbuffer(oracle, scene_of(scene), tex, sky, view(api, model, SCENE_SIZE[scene])[2])
    return _buffers[key]


# ------------------------------------------------------------------ G1. the records
@pytest.mark.parametrize("size", list(prj.SIZES))
@pytest.mark.parametrize("model", prj.MODELS)
def test_generated_records_equal_the_host_definition(R, api, tex, sky, strict, model, size):
    W, H, first_row, rows, bands = SIZES[size]
    cam, proj, want = view(api, model, size)
    with projected(R, api, "demo", tex, sky, model, size, strict) as r:
        got = r.read_rays()
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
        ids = prj.global_ids(W, H, first_row, rows, bands)
        unit = r.w.unit_projection(cam, proj, int(ids.min()), int(ids.max()) + 1)
        assert unit is not None and np.array_equal(bits(unit[ids - ids.min()]), bits(want))
        assert r.w.unit_projection(cam, proj, 0, W * H + 1) is None and r.w.unit_projection(cam, api.projection(3)) is None
        assert r.w.unit_projection(cam, api.projection(api.PROJ_PERSPECTIVE)) is None


@pytest.mark.parametrize("model", prj.MODELS)
def test_records_of_the_unfused_protocol(R, api, tex, sky, strict, model):
    """CLWRAP_FUSE=0: the raygen launch itself runs wt_raygen_proj"""
    with projected(R, api, "demo", tex, sky, model, "strip", strict, fuse=False) as r:
        assert np.array_equal(bits(r.read_rays()), bits(view(api, model, "strip")[2]))


# ------------------------------------------------------------------ G2. the strict frame against the oracle
G2_CASES = [(scene, model, "67x45", depth) for scene in ("demo", "grid324") for model in prj.MODELS for depth in (1, 5)]
G2_CASES += [("demo", model, "strip", depth) for model in prj.MODELS for depth in (1, 5)]
G2_CASES += [("demo", "equirect", "64x32", 1), ("demo", "equirect", "64x32", 5), ("demo", "ortho", "9x1", 5), ("demo", "equirect", "9x1", 5),
             ("demo", "ortho", "1x1", 5), ("demo", "equirect", "1x1", 5)]


@pytest.mark.parametrize("scene,model,size,depth", G2_CASES)
def test_strict_frame_equals_the_oracle_on_the_host_records(R, api, oracle, tex, sky, scene, model, size, depth):
    import torch  # noqa: F401
    want = expected_frame(oracle, api, scene, tex, sky, model, size, depth)
    with projected(R, api, scene, tex, sky, model, size, True, depth) as r:
        got = r.render()
        flags = r.w.last_trace_flags()
    assert flags & F.F_RAYS and not flags & F.F_SS
    if size not in ("1x1", "9x1"):
        assert len(np.unique(want)) > 16      # (the view shows something)
    check_exact(got, want, f"projection {model} {scene} {size} depth {depth}")


@pytest.mark.parametrize("model", prj.MODELS)
def test_strips_compose_to_the_frame(R, api, oracle, tex, sky, model):
    import torch  # noqa: F401
    W, H = 67, 45
    cam, proj, _ = view(api, model, "67x45")
    parts = []
    for first_row, rows in ((0, 16), (16, 21), (37, 8)):
        with rendering(R, scene_of("demo"), tex, sky, W, H, cam=cam, depth=5, strict=True, first_row=first_row, rows=rows, projection=proj) as r:
            parts.append(r.render())
    check_exact(np.concatenate(parts), expected_frame(oracle, api, "demo", tex, sky, model, "67x45", 5), f"projection {model} strips")
    check_exact(parts[1], expected_frame(oracle, api, "demo", tex, sky, model, "strip", 5), f"projection {model} strip 16+21")


@pytest.mark.parametrize("model", prj.MODELS)
def test_bands_compose_to_the_frame(R, api, oracle, tex, sky, model):
    """interleaved row bands (2, phase): the two renderers' rows, put back in frame order, are the oracle's frame"""
    import torch  # noqa: F401
    W, H = 64, 48
    cam, proj = prj.view_of(api, model, W, H)
    want, _ = oracle.trace_rays(api.projection_rays(cam, proj), scene_of("demo"), tex, sky, 5)
    frame = np.zeros(W * H, np.uint32)
    for phase in (0, 1):
        with rendering(R, scene_of("demo"), tex, sky, W, H, cam=cam, depth=5, strict=True, bands=(2, phase), projection=proj) as r:
            frame[prj.global_ids(W, H, bands=(2, phase))] = r.render()
    check_exact(frame, want, f"projection {model} bands")


# ------------------------------------------------------------------ G3. the fast frame against the parent's ray-buffer trace
def trace_uploaded(api, scene, tex, sky, rays, first_id, depth, strict):
    """The frame the library traces from `rays` uploaded as a caller's ray buffer: the drivers' protocol without a raygen launch, fuse off"""
    n = len(rays)
    with released(api.ClWrap()) as w:
        w.set_depth(depth)
        w.set_strict(strict)
        w.set_fuse(False)
        w.set_id_offset(first_id)
        w.load_global_data(0, 8, np.ascontiguousarray(rays, np.float32))
        w.load_single_data(1, 0, w.buffer_handle(0, 8))
        w.load_global_data(1, 1, scene.spheres, mem_flags=api.CL_MEM_READ_ONLY)
        w.load_global_data(1, 2, scene.planes, mem_flags=api.CL_MEM_READ_ONLY)
        w.load_global_data(1, 3, scene.lights, mem_flags=api.CL_MEM_READ_ONLY)
        for arg, count in zip((4, 5, 6), scene.counts):
            w.load_single_data(1, arg, np.uint32(count))
        w.load_single_data(1, 7, np.uint32(n))
        w.load_images_raw(1, 8, tex)
        w.load_images_raw(1, 9, sky)
        w.load_global_data(1, 10, None, 4 * n, api.CL_MEM_WRITE_ONLY)
        out = np.empty(n, np.uint32)
        w.output(n, out.nbytes, 1, 1, 10, out)
        return out, w.last_trace_flags()


@pytest.mark.parametrize("depth", [1, 5])
@pytest.mark.parametrize("size", ["67x45", "64x32", "9x1", "1x1", "strip"])
@pytest.mark.parametrize("scene", ["demo", "grid324", "glass16"])
@pytest.mark.parametrize("model", prj.MODELS)
def test_fast_frame_equals_the_same_records_uploaded_by_a_caller(R, api, tex, sky, model, scene, size, depth):
    import torch  # noqa: F401
    W, H, first_row, _, _ = SIZES[size]
    rays = view(api, model, size)[2]
    want, want_flags = trace_uploaded(api, scene_of(scene), tex, sky, rays, first_row * W, depth, False)
    with projected(R, api, scene, tex, sky, model, size, False, depth) as r:
        got = r.render()
        flags = r.w.last_trace_flags()
    differ = int((got != want).sum())
    print(f"fast {model} {scene} {size} depth {depth}: {differ} of {got.size} pixels differ from the uploaded records' frame; flags {flags}")
    assert flags == want_flags and flags & F.F_RAYS
    assert differ == 0


# ------------------------------------------------------------------ G4 / G5. the primary-hit pass
CHANNELS = ("depth", "normal", "point", "albedo")


def pick_pixels(W, H):
    return [(0, 0), (W - 1, H - 1), (W // 2, 0), (W // 2, H // 2), (W // 3, 2 * H // 3)]      # two corners, the pole row, two inside


@pytest.mark.parametrize("scene", list(SCENE_SIZE))
@pytest.mark.parametrize("model", prj.MODELS)
def test_strict_gbuffer_equals_the_expectation_from_the_host_records(R, api, oracle, tex, sky, model, scene):
    import torch  # noqa: F401
    e = expected_buffers(oracle, api, scene, tex, sky, model)
    W, H = SIZES[SCENE_SIZE[scene]][:2]
    with projected(R, api, scene, tex, sky, model, SCENE_SIZE[scene], True) as r:
        g = r.gbuffer()
        picks = [(x, y, r.pick(x, y)) for x, y in pick_pixels(W, H)]
        assert r.pick(W, 0) is None and r.pick(0, H) is None
    assert e["solid"].sum() > 50 and len(np.unique(e["id"])) >= 3
    differ = g["id"] != e["id"]
    print(f"gbuffer strict {model} {scene}: {int(differ.sum())} of {differ.size} ids differ; {len(np.unique(e['id']))} distinct ids")
    assert not differ.any()
    for k in CHANNELS:
        bad = (bits(g[k]) != bits(e[k])).reshape(differ.size, -1).any(1)
        print(f"  {k}: {int(bad.sum())} pixels differ in bits")
        assert not bad.any(), k
    for x, y, p in picks:
        i = y * W + x
        assert p is not None and p["id"] == int(g["id"][i]) and bits(p["depth"]) == bits(g["depth"][i]), (x, y)
        for k in ("point", "normal", "albedo"):
            assert np.array_equal(bits(p[k]), bits(g[k][i])), (x, y, k)


def check_fast_rule(g, e, W, what):
    """G5: equal ids -> expected bits; a differing id -> on an id boundary of the expected image, carrying a neighbour's id"""
    differ = g["id"] != e["id"]
    same = ~differ
    for k in ("depth", "point", "normal"):
        bad = (bits(g[k]) != bits(e[k])).reshape(differ.size, -1).any(1) & same
        print(f"{what}: {k}: {int(bad.sum())} pixels of equal id differ in bits")
        assert not bad.any(), k
    boundary, neighbours = prj.id_boundary(e["id"], W)
    carries = (neighbours == g["id"][:, None]).any(1)
    print(f"{what}: {int(differ.sum())} of {differ.size} ids differ; {int((differ & ~boundary).sum())} of them off a boundary, "
          f"{int((differ & ~carries).sum())} with an id no neighbour has")
    assert not (differ & ~boundary).any() and not (differ & ~carries).any()


@pytest.mark.parametrize("scene", list(SCENE_SIZE))
@pytest.mark.parametrize("model", prj.MODELS)
def test_fast_gbuffer_names_the_expected_object_or_a_neighbour(R, api, oracle, tex, sky, model, scene):
    import torch  # noqa: F401
    e = expected_buffers(oracle, api, scene, tex, sky, model)
    W = SIZES[SCENE_SIZE[scene]][0]
    check_fast_rule(e, e, W, f"gbuffer expectation {model} {scene}")      # the expectation itself: zero differing pixels
    with projected(R, api, scene, tex, sky, model, SCENE_SIZE[scene], False) as r:
        g = r.gbuffer()
    check_fast_rule(g, e, W, f"gbuffer fast {model} {scene}")


# ------------------------------------------------------------------ G6. the passes built on it
def test_objects_highlight_and_select_rect_under_the_orthographic_view(R, api, oracle, tex, sky):
    import torch  # noqa: F401
    W, H = SIZES["67x45"][:2]
    sc = scene_of("demo")
    e = expected_buffers(oracle, api, "demo", tex, sky, "ortho")
    frame = expected_frame(oracle, api, "demo", tex, sky, "ortho", "67x45", 5)
    want_table, want_summary = api.object_stats(e["id"], e["depth"], W, H, sc.counts)
    spheres = want_table["id"][api.id_kind(want_table["id"]) == api.ID_SPHERE]
    assert len(spheres) >= 2
    sel = spheres[:2]
    want_overlay = api.overlay(frame, e["id"], W, H, api.overlay_style(api.OV_OUTLINE | api.OV_FILL | api.OV_EDGES, 2, 0xFFFF00, 0x00FF00, 96, 0x808080), sel)
    with projected(R, api, "demo", tex, sky, "ortho", "67x45", True, 5) as r:
        got = r.render()
        check_exact(got, frame, "projection ortho demo 67x45 depth 5 (overlay's frame)")
        table = r.objects()
        overlay = r.highlight(sel, outline=0xFFFF00, radius=2, fill=0x00FF00, alpha=96, edges=0x808080)
        picked = r.select_rect(0, 0, W - 1, H - 1)
    assert table.tobytes() == want_table.tobytes() and want_summary["objects"] == len(table)
    assert np.array_equal(overlay, want_overlay) and (overlay != frame).any()
    solid = table[(api.id_kind(table["id"]) <= api.ID_PLANE) & (table["id"] != api.ID_NONE)]
    assert sorted(picked.tolist()) == sorted(solid["id"].tolist()) and len(picked) >= 3


# ------------------------------------------------------------------ G7. state
def test_clearing_the_projection_restores_the_pinhole(R, api, tex, sky, strict):
    from conftest import CAM
    W, H = 67, 45
    sc = scene_of("demo")
    with rendering(R, sc, tex, sky, W, H, depth=4, strict=strict) as fresh:
        want, want_flags, want_g = fresh.render(), fresh.w.last_trace_flags(), fresh.gbuffer()
    with rendering(R, sc, tex, sky, W, H, depth=4, strict=strict) as r:
        r.set_projection("equirect", axis=CAM["look"])
        assert r.w.get_projection().model == api.PROJ_EQUIRECT
        pano = r.render()
        assert r.w.last_trace_flags() & F.F_RAYS and (pano != want).any()
        r.set_projection(None)
        assert r.w.get_projection().model == api.PROJ_PERSPECTIVE
        got, flags, g = r.render(), r.w.last_trace_flags(), r.gbuffer()
        pin_rays = r.read_rays()
    assert not want_flags & F.F_RAYS and flags == want_flags
    assert np.array_equal(got, want)
    for k in want_g:
        assert np.array_equal(bits(g[k]), bits(want_g[k])), k
    # the ray buffer holds the pinhole's records again, not the panorama's
    assert np.array_equal(bits(pin_rays), bits(api.projection_rays(api.perspective(**CAM, width=W, height=H), api.projection(0))))


def test_a_still_view_generates_its_records_once(R, api, tex, sky, strict):
    W, H = 64, 32
    with projected(R, api, "demo", tex, sky, "equirect", "64x32", strict) as r:
        r.w.timing_reset()
        a = r.render()
        b = r.render()
        assert np.array_equal(a, b)
        assert r.w.timing_get(0)[0] == 1 and r.w.timing_get(1)[0] == 2        # one wt_raygen_proj, two traces
        r.gbuffer(api.GB_ID)
        assert r.w.timing_get(0)[0] == 1
        r.set_projection("equirect", axis=prj.VIEW["look"], span=(200, 90))      # only the span changes
        c = r.render()
        assert r.w.timing_get(0)[0] == 2 and (c != a).any()
        cam = view(api, "equirect", "64x32")[0]
        want = api.projection_rays(cam, api.projection(api.PROJ_EQUIRECT, prj.VIEW["look"], 0.0, (200, 90)))
        assert np.array_equal(bits(r.read_rays()), bits(want))
        assert r.w.timing_get(0)[0] == 2                                         # the read-back found them in place
        r.look(origin=(0.0, 2.0, -7.0), look=prj.VIEW["look"])                   # the camera moves: new records
        r.render()
        assert r.w.timing_get(0)[0] == 3


# ------------------------------------------------------------------ G8. refusals and the environment
REFUSED = {
    "supersampling": "supersample=2",
    "lens": "supersample=2, lens=(0.1, 5.0)",
    "moving spheres": "supersample=2, motion=np.ones((4, 3), np.float32)",
    "adaptive": "supersample=2, adaptive=32",
    "accumulation": "accumulate=4",
}


# (each combination under one model: the planner's host test runs all of them under both)
@pytest.mark.parametrize("what,model", [("supersampling", "ortho"), ("lens", "equirect"), ("moving spheres", "ortho"), ("adaptive", "equirect"),
                                        ("accumulation", "ortho"), ("accumulation", "equirect")])
def test_what_needs_the_fused_launch_exits_naming_the_projection(what, model):
    p = run_child(f"r = Renderer(sc, tex, sky, 32, 24, depth=2, projection={model!r}, {REFUSED[what]})\nr.look(**CAM)\nr.render()\nprint('NOT REFUSED')\n")
    print(p.stdout[-300:])
    assert p.returncode == 1 and "ERROR:" in p.stdout and "projection" in p.stdout and "NOT REFUSED" not in p.stdout


@pytest.mark.parametrize("name,value", [("CLWRAP_PROJECTION", "fisheye"), ("CLWRAP_ORTHO_WIDTH", "-2"), ("CLWRAP_PANO_SPAN", "400,90"),
                                        ("CLWRAP_PANO_SPAN", "90")])
def test_bad_environment_values_exit_naming_the_variable(name, value):
    p = run_child("r = Renderer(sc, tex, sky, 32, 24)\nprint('NOT REFUSED')\n", env=dict(os.environ, **{name: value}))
    print(p.stdout[-300:])
    assert p.returncode == 1 and "ERROR:" in p.stdout and name in p.stdout and "NOT REFUSED" not in p.stdout


def test_the_environment_renders_a_panorama(api, oracle, tex):
    """CLWRAP_PROJECTION=equirect over the drivers' unchanged protocol: the zero axis is the camera's own centre direction"""
    import torch  # noqa: F401
    from example_gui_opencl_raytracer_amd import textures
    W, H = 64, 32
    cam = api.perspective(prj.VIEW["origin"], prj.VIEW["look"], 90.0, 1.0, W, H)
    want, _ = oracle.trace_rays(api.projection_rays(cam, api.projection(api.PROJ_EQUIRECT, None, 0.0, (180.0, 90.0))), scene_of("demo"), tex,
                                textures.skybox_cross(64), 5)
    p = run_child(f"r = Renderer(sc, tex, sky, {W}, {H}, depth=5, strict=True)\nr.look(origin={prj.VIEW['origin']!r}, look={prj.VIEW['look']!r})\n"
                  "f = r.render()\nprint('FLAGS', r.w.last_trace_flags())\nprint('FRAME', f.tobytes().hex())\n",
                  env=dict(os.environ, CLWRAP_PROJECTION="equirect", CLWRAP_PANO_SPAN="180,90"))
    assert p.returncode == 0, p.stdout[-300:] + p.stderr[-300:]
    lines = dict(l.split(" ", 1) for l in p.stdout.splitlines() if l.startswith(("FLAGS ", "FRAME ")))
    assert int(lines["FLAGS"]) & F.F_RAYS
    got = np.frombuffer(bytes.fromhex(lines["FRAME"]), np.uint32)
    check_exact(got, want, "projection equirect from the environment")
